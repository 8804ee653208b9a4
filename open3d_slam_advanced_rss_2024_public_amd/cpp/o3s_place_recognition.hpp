// o3s_place_recognition.hpp — header-only C++17 restatement of o3d_slam::PlaceRecognition (open3d_slam/src/PlaceRecognition.cpp;
// line numbers below are its own) over resident submaps and the C ABI.  place_recognition.py is its Python mirror: same logic.
//
//   :50-176    buildLoopClosureConstraints: the candidates of a finished submap in groups of up to O3S_PLACE_MAX_TARGETS through
//              ONE o3s_submaps_registration_ransac call each (place_recognition/o3s_place_recognition.h: every candidate's feature
//              correspondences in two launches, then the RANSACs from the device pair buffer); the ransacMinCorrespondenceSetSize
//              gate and isRegistrationConsistent on the RANSAC pose; the survivors through ONE
//              o3s_o3d_registration_icp_submaps_overlap_batch_ex call (overlap selection, refinement, information matrix; up to four
//              pairs in flight); the minRefinementFitness gate and isRegistrationConsistent on the refined pose.  The reference's
//              loop is serial (its `omp parallel for` is commented out, :70); per candidate the results are the same.
//   :182-229   isRegistrationConsistent: toRPY(Eigen::Quaterniond(R)) as o3s_motion_from_poses restates it (csrc/undistort_dev.h),
//              without the normalisation that call adds; a value equal to its limit passes (the reference rejects on `>`)
//   :231-285   getLoopClosureCandidatesIdxs: not the active submap; not adjacent to the ACTIVE submap; centre within the search
//              radius of the FINISHED submap's centre; at least minSubmapsBetweenLoopClosures between the finished submap and the
//              nearest loop-closure submap (AdjacencyHip::getDistanceToNearestLoopClosureSubmap)
// Collection: numSubmaps(), submap(i) with .id and .mapToSubmapCenter(), adjacency(), submapMap(i) (SubmapCollectionHip).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "o3s_submap_collection.hpp"
#include "place_recognition/o3s_place_recognition.h"

namespace o3s {

struct ConsistencyCheckParams {  // LOOP_CLOSURE_CONSISTENCY_CHECK_PARAMETERS; the angles in radians, as they are compared
  double maxDriftRoll = 30.0 * 3.14159265358979323846 / 180.0;
  double maxDriftPitch = 30.0 * 3.14159265358979323846 / 180.0;
  double maxDriftYaw = 30.0 * 3.14159265358979323846 / 180.0;
  double maxDriftX = 80.0, maxDriftY = 80.0, maxDriftZ = 40.0;
};

struct PlaceRecognitionParams {  // PLACE_RECOGNITION_PARAMETERS (param/default/parameter_structure_definitions.lua:162-181)
  double loopClosureSearchRadius = 20.0;
  int minSubmapsBetweenLoopClosures = 2;
  o3s_ransac_params ransac = defaultRansac();
  bool mutualFilter = true;
  std::size_t ransacMinCorrespondenceSetSize = 25;
  double maxIcpCorrespondenceDistance = 0.3;
  double minRefinementFitness = 0.7;
  ConsistencyCheckParams consistencyCheck;
  double overlapVoxelSize = 0.0;  // magic::voxelExpansionFactorOverlapComputation x the map voxel size: the caller's, required
  std::int32_t registrationType = O3S_O3D_GENERALIZED;  // scan_to_map_refinement_type
  double gicpEpsilon = 1e-3;
  std::int32_t maxIcpIterations = 30;
  // not the reference's: match at ISS keypoints only (keypoints/o3s_keypoints.h).  min_neighbors 0, the zeroed struct = off: every
  // sparse point is matched.  PlaceRecognitionHip::computeFeatures hands it to the collection, nothing else reads it
  o3s_iss_params featureKeypoints{0.0, 0.0, 0.0, 0.0, 0, 0};
  static o3s_ransac_params defaultRansac() {
    o3s_ransac_params p;
    o3s_ransac_default_params(&p);
    return p;
  }
};

// toRPY(Eigen::Quaterniond(T.rotation())) (math.hpp:30-42)
inline void toRPY(const Mat4& T, double rpy[3]) {
  double q[4];  // w, x, y, z
  const double tr = (T(0, 0) + T(1, 1)) + T(2, 2);
  if (tr > 0.0) {
    double u = std::sqrt(tr + 1.0);
    q[0] = 0.5 * u;
    u = 0.5 / u;
    q[1] = (T(2, 1) - T(1, 2)) * u;
    q[2] = (T(0, 2) - T(2, 0)) * u;
    q[3] = (T(1, 0) - T(0, 1)) * u;
  } else {
    int i = 0;
    if (T(1, 1) > T(0, 0)) i = 1;
    if (T(2, 2) > T(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double u = std::sqrt(T(i, i) - T(j, j) - T(k, k) + 1.0);
    q[1 + i] = 0.5 * u;
    u = 0.5 / u;
    q[0] = (T(k, j) - T(j, k)) * u;
    q[1 + j] = (T(j, i) + T(i, j)) * u;
    q[1 + k] = (T(k, i) + T(i, k)) * u;
  }
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  rpy[0] = std::atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y));
  rpy[1] = std::asin(2 * (w * y - x * z));
  rpy[2] = std::atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z));
}

inline bool isRegistrationConsistent(const Mat4& T, const ConsistencyCheckParams& p) {  // :182-229
  double rpy[3];
  toRPY(T, rpy);
  return !(std::fabs(rpy[0]) > p.maxDriftRoll || std::fabs(rpy[1]) > p.maxDriftPitch || std::fabs(rpy[2]) > p.maxDriftYaw ||
           std::fabs(T(0, 3)) > p.maxDriftX || std::fabs(T(1, 3)) > p.maxDriftY || std::fabs(T(2, 3)) > p.maxDriftZ);
}

template <class Collection>
std::vector<std::size_t> getLoopClosureCandidatesIdxs(const Collection& collection, std::size_t lastFinishedSubmapIdx, std::size_t activeSubmapIdx,
                                                      const PlaceRecognitionParams& params) {  // :231-285
  std::vector<std::size_t> idxs;
  const std::size_t nSubmaps = collection.numSubmaps();
  const double* c0 = collection.submap(lastFinishedSubmapIdx).mapToSubmapCenter();
  for (std::size_t i = 0; i < nSubmaps; ++i) {
    if (i == activeSubmapIdx) continue;
    if (collection.adjacency().isAdjacent(collection.submap(i).id, collection.submap(activeSubmapIdx).id)) continue;
    const double* c = collection.submap(i).mapToSubmapCenter();
    const double dx = c0[0] - c[0], dy = c0[1] - c[1], dz = c0[2] - c[2];
    if (std::sqrt((dx * dx + dy * dy) + dz * dz) > params.loopClosureSearchRadius) continue;
    if (collection.adjacency().getDistanceToNearestLoopClosureSubmap(lastFinishedSubmapIdx) < params.minSubmapsBetweenLoopClosures) continue;
    idxs.push_back(i);
  }
  return idxs;
}

class PlaceRecognitionHip {
 public:
  enum class Rejected { None, RansacCorrespondences, RansacInconsistent, EmptyOverlap, RefinementScore, RefinementInconsistent };
  struct Candidate {  // what became of one candidate of the last call
    std::size_t targetSubmapIdx = 0;
    Rejected rejected = Rejected::None;
    o3s_ransac_result ransac{};
    std::int64_t numCorrespondences = 0;  // the size of the correspondence set the RANSAC ran on
    o3s_o3d_icp_result refinement{};      // valid from RefinementScore on
    std::int64_t overlap[2] = {0, 0};
  };

  explicit PlaceRecognitionHip(const PlaceRecognitionParams& p = PlaceRecognitionParams()) : params_(p) {}
  const PlaceRecognitionParams& params() const { return params_; }
  void setParams(const PlaceRecognitionParams& p) { params_ = p; }
  bool isRegistrationConsistent(const Mat4& T) const { return o3s::isRegistrationConsistent(T, params_.consistencyCheck); }
  // collection.computeFeatures(...) with this object's featureKeypoints: the one place where the keypoint selection is switched
  // on for everything buildLoopClosureConstraints later searches
  template <class Collection, class Finished>
  void computeFeatures(Collection& collection, const Finished& finished, const o3s_submap_feature_params* params = nullptr) {
    collection.computeFeatures(finished, params, params_.featureKeypoints.min_neighbors != 0 ? &params_.featureKeypoints : nullptr);
  }
  const std::vector<Candidate>& lastCandidates() const { return last_; }

  // (mapToRangeSensor is not used by the reference either: its distance test is commented out, :259)
  template <class Collection>
  std::vector<std::size_t> getLoopClosureCandidatesIdxs(const Mat4& /*mapToRangeSensor*/, const Collection& collection, std::size_t lastFinishedSubmapIdx,
                                                        std::size_t activeSubmapIdx) const {
    return o3s::getLoopClosureCandidatesIdxs(collection, lastFinishedSubmapIdx, activeSubmapIdx, params_);
  }

  // The Constraints of the accepted candidates in candidate order; lastCandidates() tells what became of each.  A submap that is
  // not a candidate is never touched.
  template <class Collection>
  Constraints buildLoopClosureConstraints(const Mat4& mapToRangeSensor, Collection& collection, std::size_t lastFinishedSubmapIdx,
                                          std::size_t activeSubmapIdx, double timestamp) {
    Constraints constraints;
    const std::vector<std::size_t> cand = getLoopClosureCandidatesIdxs(mapToRangeSensor, collection, lastFinishedSubmapIdx, activeSubmapIdx);
    last_.assign(cand.size(), Candidate());
    if (cand.empty()) return constraints;
    if (!(params_.overlapVoxelSize > 0.0)) throw std::invalid_argument("PlaceRecognitionParams::overlapVoxelSize is required");
    const o3s_submap* source = collection.submapMap(lastFinishedSubmapIdx).handle();
    for (std::size_t g0 = 0; g0 < cand.size(); g0 += O3S_PLACE_MAX_TARGETS) {
      const std::size_t K = std::min<std::size_t>(O3S_PLACE_MAX_TARGETS, cand.size() - g0);
      const o3s_submap* targets[O3S_PLACE_MAX_TARGETS];
      o3s_ransac_result results[O3S_PLACE_MAX_TARGETS];
      std::int64_t nCorr[O3S_PLACE_MAX_TARGETS];
      for (std::size_t k = 0; k < K; ++k) targets[k] = collection.submapMap(cand[g0 + k]).handle();
      const int rc = o3s_submaps_registration_ransac(source, targets, (std::int32_t)K, params_.mutualFilter ? 1 : 0, &params_.ransac, results, nullptr, nCorr);
      if (rc == O3S_ERR_NOT_INITIALIZED) throw std::logic_error("place recognition: every candidate needs features (computeFeatures)");
      if (rc != O3S_OK) throw std::runtime_error("o3s_submaps_registration_ransac failed (status " + std::to_string(rc) + ")");
      for (std::size_t k = 0; k < K; ++k) {
        last_[g0 + k].targetSubmapIdx = cand[g0 + k];
        last_[g0 + k].ransac = results[k];
        last_[g0 + k].numCorrespondences = nCorr[k];
      }
    }
    std::vector<std::size_t> survivors;
    for (std::size_t c = 0; c < last_.size(); ++c) {
      Mat4 T;
      for (int k = 0; k < 16; ++k) T.m[k] = last_[c].ransac.transformation[k];
      if ((std::size_t)last_[c].ransac.correspondences < params_.ransacMinCorrespondenceSetSize) {  // :86
        last_[c].rejected = Rejected::RansacCorrespondences;
      } else if (!isRegistrationConsistent(T)) {  // :92
        last_[c].rejected = Rejected::RansacInconsistent;
      } else {
        survivors.push_back(c);
      }
    }
    if (survivors.empty()) return constraints;
    const std::size_t n = survivors.size();
    std::vector<const o3s_submap*> srcs(n, source), tgts(n);
    std::vector<double> inits(16 * n), infos(36 * n);
    std::vector<o3s_o3d_icp_result> res(n);
    std::vector<std::int64_t> novs(2 * n);
    std::vector<std::int32_t> sts(n);
    for (std::size_t s = 0; s < n; ++s) {
      tgts[s] = collection.submapMap(last_[survivors[s]].targetSubmapIdx).handle();
      for (int k = 0; k < 16; ++k) inits[16 * s + k] = last_[survivors[s]].ransac.transformation[k];
    }
    o3s_o3d_estimation est;
    o3s_o3d_default_estimation(&est);
    est.type = params_.registrationType;
    est.gicp_epsilon = params_.gicpEpsilon;
    const o3s_o3d_icp_criteria criteria{1e-6, 1e-6, params_.maxIcpIterations};
    const int rc = o3s_o3d_registration_icp_submaps_overlap_batch_ex((std::int32_t)n, srcs.data(), tgts.data(), params_.maxIcpCorrespondenceDistance, inits.data(),
                                                                     &est, &criteria, params_.overlapVoxelSize, 1, res.data(), infos.data(), novs.data(), sts.data());
    if (rc != O3S_OK) throw std::runtime_error("o3s_o3d_registration_icp_submaps_overlap_batch_ex failed (status " + std::to_string(rc) + ")");
    for (std::size_t s = 0; s < n; ++s) {
      Candidate& c = last_[survivors[s]];
      c.overlap[0] = novs[2 * s];
      c.overlap[1] = novs[2 * s + 1];
      if (sts[s] == O3S_ERR_EMPTY_REFERENCE) {
        c.rejected = Rejected::EmptyOverlap;
        continue;
      }
      if (sts[s] != O3S_OK) throw std::runtime_error("loop-closure refinement failed (status " + std::to_string(sts[s]) + ")");
      c.refinement = res[s];
      Mat4 T;
      for (int k = 0; k < 16; ++k) T.m[k] = res[s].transformation[k];
      if (res[s].fitness < params_.minRefinementFitness) {  // :118
        c.rejected = Rejected::RefinementScore;
      } else if (!isRegistrationConsistent(T)) {  // :124
        c.rejected = Rejected::RefinementInconsistent;
      } else {  // :144-154
        Constraint k;
        k.sourceToTarget = T;
        k.sourceSubmapIdx = lastFinishedSubmapIdx;
        k.targetSubmapIdx = c.targetSubmapIdx;
        for (int e = 0; e < 36; ++e) k.informationMatrix[e] = infos[36 * s + e];
        k.isInformationMatrixValid = true;
        k.isOdometryConstraint = false;
        k.timestamp = timestamp;
        constraints.push_back(k);
      }
    }
    return constraints;
  }

 private:
  PlaceRecognitionParams params_;
  std::vector<Candidate> last_;
};

}  // namespace o3s
