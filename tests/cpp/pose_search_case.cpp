// pose_search_case.cpp — the localisation step as COMPILED host code: cpp/o3s_pose_search.hpp and MapperHip::localizeInitialPose
// (cpp/o3s_mapper.hpp), plain g++, linking only the C-ABI library.  tests/test_gpu_pose_search_localize.py writes the case and
// compares what is printed here with the Python path over the same library: integers exactly, the pose bit for bit.
//
// argv[1]: the case — int64 M, N; map points (3 x M doubles), map normals; scan points (3 x N), scan normals; the prior (16 doubles,
// column-major); doubles step_xy, step_z, step_yaw, yaw0, min_fitness, wide radius, narrow radius, scan voxel, snapshot voxel;
// int64 n_x, n_y, n_z, n_yaw, yaw_ring, point_stride, local_maxima, top_k, min_score.
// Output: "winners n", one "index score" line each, "ok 0|1", "kept index score", "fitness <%a>", "pose" + 16 x %a, "mapper" + 16 x %a
// (mapToRangeSensor after the call), "again 0|1" (a second call after a measurement must refuse).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "o3s_mapper.hpp"

namespace {
template <class T>
bool rd(std::FILE* f, T* p, std::size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::int64_t MN[2];
  if (!rd(f, MN, 2)) return 2;
  const std::int64_t M = MN[0], N = MN[1];
  std::vector<double> mp((std::size_t)M * 3), mn((std::size_t)M * 3), sp((std::size_t)N * 3), sn((std::size_t)N * 3);
  double center[16], d[9];
  std::int64_t q[9];
  if (!rd(f, mp.data(), mp.size()) || !rd(f, mn.data(), mn.size()) || !rd(f, sp.data(), sp.size()) || !rd(f, sn.data(), sn.size()) ||
      !rd(f, center, 16) || !rd(f, d, 9) || !rd(f, q, 9))
    return 2;
  std::fclose(f);
  try {
    o3s::MapperParams mpar;
    mpar.isUseInitialMap = true;
    mpar.isMergeScansIntoMap = false;
    mpar.mapBuilderCropper.kind = 1;
    mpar.mapBuilderCropper.p0 = d[5];
    mpar.scanMatcherCropper.kind = 1;
    mpar.scanMatcherCropper.p0 = d[6];
    mpar.scanVoxelSize = d[7];
    mpar.mapVoxelSize = 0.1;
    o3s_icp_config cfg;
    o3s_icp_default_config(&cfg);
    o3s::MapperHip mapper(mpar, cfg, 0);
    o3s::PoseSearchParams sp_;
    for (int k = 0; k < 16; ++k) sp_.center[k] = center[k];
    sp_.step_xy = d[0];
    sp_.step_z = d[1];
    sp_.step_yaw = d[2];
    sp_.yaw0 = d[3];
    sp_.n_x = (std::int32_t)q[0];
    sp_.n_y = (std::int32_t)q[1];
    sp_.n_z = (std::int32_t)q[2];
    sp_.n_yaw = (std::int32_t)q[3];
    sp_.yaw_ring = (std::int32_t)q[4];
    sp_.point_stride = (std::int32_t)q[5];
    sp_.local_maxima = (std::int32_t)q[6];
    sp_.top_k = (std::int32_t)q[7];
    sp_.min_score = q[8];
    // before the map is in: refused
    if (mapper.localizeInitialPose(sp.data(), sn.data(), N, sp_, d[4])) return 3;
    // the initial map goes straight into the active submap (o3s_submap.h: o3s_submap_upload holds the initial map)
    if (o3s_submap_upload(mapper.activeSubmap().handle(), mp.data(), mn.data(), M) != O3S_OK) return 4;
    mapper.activeSubmap().buildVoxelMap(d[8]);
    const bool ok = mapper.localizeInitialPose(sp.data(), sn.data(), N, sp_, d[4]);
    const o3s::LocalizeResult& r = mapper.lastLocalize();
    std::printf("winners %d\n", (int)r.search.n_found);
    for (int k = 0; k < r.search.n_found; ++k) std::printf("%lld %lld\n", (long long)r.search.index[k], (long long)r.search.score[k]);
    std::printf("ok %d\nkept %lld %lld\nfitness %a\npose", ok ? 1 : 0, (long long)r.index, (long long)r.score, r.fitness);
    for (int k = 0; k < 16; ++k) std::printf(" %a", r.T.m[k]);
    std::printf("\nmapper");
    for (int k = 0; k < 16; ++k) std::printf(" %a", mapper.mapToRangeSensor().m[k]);
    std::printf("\n");
    // the scan itself: registered at the localised pose (a pose reset: the given pose is adopted); then no second localisation
    const bool added = mapper.addRangeMeasurement(sp.data(), sn.data(), N, 0.0);
    std::printf("added %d reset %d\nafter", added ? 1 : 0, mapper.lastReferenceReset() ? 1 : 0);
    for (int k = 0; k < 16; ++k) std::printf(" %a", mapper.mapToRangeSensor().m[k]);
    std::printf("\nagain %d\n", mapper.localizeInitialPose(sp.data(), sn.data(), N, sp_, d[4]) ? 1 : 0);
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  return 0;
}
