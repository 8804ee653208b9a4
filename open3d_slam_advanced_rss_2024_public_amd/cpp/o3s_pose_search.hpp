// o3s_pose_search.hpp — header-only C++17 shim over include/pose_search/o3s_pose_search.h, and the localisation step built on it:
// what replaces the interactive marker of SlamMapInitializer (ros/open3d_slam_ros/src/SlamMapInitializer.cpp:50-130) when the
// start pose in a loaded map is to be FOUND.  poseSearch scores a grid of poses around a prior against the submap's occupancy
// snapshot in one device call; localize is host policy over existing entries, the twin of pose_search.py's: every winner is
// refined by the scan-to-map chain (SubmapHip::setReference at the candidate, the scan's match cloud as the resident reading,
// o3s_icp_compute_resident from the candidate, IcpHip::evaluate) and the candidate with the highest fitness is kept — the
// earlier one wins a tie — and accepted when its fitness reaches minFitness.  Plain g++ against the C ABI.
#pragma once

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "o3s_icp.hpp"
#include "o3s_pose.hpp"
#include "o3s_scan.h"
#include "pose_search/o3s_pose_search.h"

namespace o3s {

struct PoseSearchParams : o3s_pose_search_params {
  PoseSearchParams() { o3s_pose_search_default_params(this); }
  void setCenter(const Mat4& priorMapToRangeSensor) {
    for (int k = 0; k < 16; ++k) center[k] = priorMapToRangeSensor.m[k];
  }
  std::int64_t count() const { return o3s_pose_search_count(this); }  // P; -1: parameters the search refuses
};

// the pose of grid index `index` (o3s_pose_search_pose)
inline Mat4 poseOf(const o3s_pose_search_params& p, std::int64_t index) {
  Mat4 T{};
  if (o3s_pose_search_pose(&p, index, T.m) != O3S_OK) throw std::invalid_argument("poseOf: refused parameters, or an index outside the grid");
  return T;
}

namespace detail {
inline void raisePoseSearch(int rc) {
  if (rc == O3S_ERR_BAD_ARGUMENT) throw std::invalid_argument("poseSearch: bad argument (parameters out of range, too many poses or points, another device)");
  if (rc == O3S_ERR_NOT_INITIALIZED) throw std::runtime_error("poseSearch: the submap has no occupancy snapshot (SubmapHip::buildVoxelMap)");
  if (rc != O3S_OK) throw std::runtime_error("o3s_submap_pose_search failed (status " + std::to_string(rc) + ")");
}
inline std::uint32_t* scoreRoom(const o3s_pose_search_params& p, std::vector<std::uint32_t>* scores) {
  if (!scores) return nullptr;
  const std::int64_t P = o3s_pose_search_count(&p);
  if (P < 0) throw std::invalid_argument("poseSearch: refused parameters");
  scores->assign((std::size_t)P, 0u);
  return scores->data();
}
}  // namespace detail

// host points (3 x N doubles, sensor frame); scores (nullable): the score of every pose
inline o3s_pose_search_result poseSearch(SubmapHip& submap, const double* points3xN, std::int64_t N, const o3s_pose_search_params& p,
                                         std::vector<std::uint32_t>* scores = nullptr) {
  o3s_pose_search_result r{};
  detail::raisePoseSearch(o3s_submap_pose_search(submap.handle(), points3xN, N, &p, &r, detail::scoreRoom(p, scores)));
  return r;
}
// a resident pre-processed scan; which: 0 merge cloud, 1 match cloud
inline o3s_pose_search_result poseSearch(SubmapHip& submap, const o3s_scan* scan, int which, const o3s_pose_search_params& p,
                                         std::vector<std::uint32_t>* scores = nullptr) {
  o3s_pose_search_result r{};
  detail::raisePoseSearch(o3s_submap_pose_search_scan(submap.handle(), scan, which, &p, &r, detail::scoreRoom(p, scores)));
  return r;
}

struct LocalizeCandidate {
  std::int64_t index = -1, score = 0;
  bool refined = false;  // false: the refinement failed (error says how) and the candidate was skipped
  Mat4 T = Mat4::identity();
  double fitness = std::numeric_limits<double>::quiet_NaN();
  int iterations = 0;
  std::string error;
};
struct LocalizeResult {
  bool ok = false;
  Mat4 T = Mat4::identity();  // the kept candidate's refined pose (meaningful when index >= 0)
  double fitness = std::numeric_limits<double>::quiet_NaN();
  std::int64_t index = -1, score = 0;  // the kept candidate's grid index and score; -1: none could be refined
  std::vector<LocalizeCandidate> candidates;
  o3s_pose_search_result search{};
};

// Builds nothing: a submap without a snapshot is the caller's error (std::runtime_error).
inline LocalizeResult localize(SubmapHip& submap, o3s_scan* scan, IcpHip& icp, const o3s_cropper& scanMatcherCropper, const o3s_pose_search_params& p,
                               double minFitness, double maxCorrespondenceDistance = 0.0) {
  LocalizeResult out;
  out.search = poseSearch(submap, scan, 1, p);
  int best = -1;
  for (int k = 0; k < out.search.n_found; ++k) {
    LocalizeCandidate c;
    c.index = out.search.index[k];
    c.score = out.search.score[k];
    const Mat4 T0 = poseOf(p, c.index);
    try {
      o3s_cropper patch = scanMatcherCropper;
      for (int a = 0; a < 3; ++a) patch.centre[a] = T0(a, 3);
      if (!submap.setReference(patch, T0.m, icp)) throw std::runtime_error("map patch is empty");
      if (o3s_scan_set_reading(scan, icp.handle()) != O3S_OK) throw std::runtime_error(o3s_last_error(icp.handle()));
      float t0[16], t1[16];
      for (int e = 0; e < 16; ++e) t0[e] = (float)T0.m[e];
      o3s_icp_stats st{};
      if (o3s_icp_compute_resident(icp.handle(), t0, t1, &st) != O3S_OK) throw std::runtime_error(o3s_last_error(icp.handle()));
      c.iterations = st.iterations;
      const o3s_icp_fitness f = icp.evaluate(nullptr, (float)maxCorrespondenceDistance);
      for (int e = 0; e < 16; ++e) c.T.m[e] = (double)t1[e];
      c.fitness = f.fitness;
      c.refined = true;
    } catch (const std::runtime_error& e) {
      c.error = e.what();
      (void)o3s_icp_synchronize(icp.handle());  // nothing of a failed compute may still be in flight when the next candidate rewrites its buffers
    }
    out.candidates.push_back(c);
    if (c.refined && (best < 0 || c.fitness > out.candidates[(std::size_t)best].fitness)) best = (int)out.candidates.size() - 1;
  }
  if (best < 0) return out;
  const LocalizeCandidate& b = out.candidates[(std::size_t)best];
  out.T = b.T;
  out.fitness = b.fitness;
  out.index = b.index;
  out.score = b.score;
  out.ok = b.fitness >= minFitness;
  return out;
}

}  // namespace o3s
