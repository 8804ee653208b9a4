// Drives cpp/o3s_mapper.hpp over recorded sweeps under one degeneracy policy (MapperParams::degeneracyPolicy): plain g++, only
// libo3dslam_icp_hip.so at link time.
//
//   localizability_loop <scene.bin> <out.txt>
// scene.bin (little endian):
//   int64   policy (0 Off, 1 Report, 2 Remap), remap_min_category, K
//   double  scan_voxel, map_voxel, wide_radius, narrow_radius, ref_period, min_movement
//   double  filter_min, strong_min, sum_all_min, sum_strong_min, sum_partial_min
//   double  first_pose[16]                                         (column-major: the pose the first sweep is inserted at)
//   K x { double stamp; double odom[16]; int64 N; double pts[3N]; double normals[3N] }
// out.txt, one line per sweep:
//   "k ok inserted icp_threw replaced kept  cat(6)  n_strong(6)  T(16, %a)  T_icp(16, %a)  prior(16, %a)  centre(3, %a)  evec(18, %a)
//    sum_all(6, %a)  sum_strong(6, %a)"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "o3s_mapper.hpp"

template <typename T>
static T rd(std::ifstream& f) {
  T v;
  f.read(reinterpret_cast<char*>(&v), sizeof(T));
  if (!f) {
    std::fprintf(stderr, "scene truncated\n");
    std::exit(2);
  }
  return v;
}
static o3s::Mat4 rd_mat(std::ifstream& f) {
  o3s::Mat4 m;
  f.read(reinterpret_cast<char*>(m.m), sizeof(m.m));
  return m;
}
static void put(FILE* out, const double* v, int n) {
  std::fprintf(out, " ");
  for (int i = 0; i < n; ++i) std::fprintf(out, " %a", v[i]);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) return 2;
  const std::int64_t policy = rd<std::int64_t>(f), min_category = rd<std::int64_t>(f), K = rd<std::int64_t>(f);
  o3s::MapperParams p;
  p.scanVoxelSize = rd<double>(f);
  p.mapVoxelSize = rd<double>(f);
  p.mapBuilderCropper.kind = 1;  // MaxRadius
  p.mapBuilderCropper.p0 = rd<double>(f);
  p.scanMatcherCropper.kind = 1;
  p.scanMatcherCropper.p0 = rd<double>(f);
  p.referenceCloudSettingPeriod = rd<double>(f);
  p.minMovementBetweenMappingSteps = rd<double>(f);
  p.submaps.radius = 1.0e9;  // one submap
  p.submaps.minNumRangeData = 5;
  p.submaps.maxNumPoints = 1000000000000LL;
  p.submaps.numScansOverlap = 3;
  p.degeneracyPolicy = policy == 0 ? o3s::MapperParams::DegeneracyPolicy::Off
                                   : (policy == 1 ? o3s::MapperParams::DegeneracyPolicy::Report : o3s::MapperParams::DegeneracyPolicy::Remap);
  p.localizability.filter_min = rd<double>(f);
  p.localizability.strong_min = rd<double>(f);
  p.localizability.sum_all_min = rd<double>(f);
  p.localizability.sum_strong_min = rd<double>(f);
  p.localizability.sum_partial_min = rd<double>(f);
  p.remapMinCategory = (std::int32_t)min_category;
  const o3s::Mat4 first_pose = rd_mat(f);
  FILE* out = std::fopen(argv[2], "w");
  if (!out) return 2;
  try {
    o3s_icp_config cfg;
    o3s_icp_default_config(&cfg);  // icp.yaml
    o3s::MapperHip mapper(p, cfg, 0);
    mapper.setCalibration(o3s::Mat4::identity());
    mapper.setMapToRangeSensor(first_pose);
    for (std::int64_t k = 0; k < K; ++k) {
      const double stamp = rd<double>(f);
      const o3s::Mat4 odom = rd_mat(f);
      const std::int64_t N = rd<std::int64_t>(f);
      std::vector<double> pts((size_t)N * 3), nrm((size_t)N * 3);
      f.read(reinterpret_cast<char*>(pts.data()), (std::streamsize)(pts.size() * 8));
      f.read(reinterpret_cast<char*>(nrm.data()), (std::streamsize)(nrm.size() * 8));
      if (!f) throw std::runtime_error("scene truncated");
      mapper.addOdometryPose(stamp, odom);
      const bool ok = mapper.addRangeMeasurement(pts.data(), nrm.data(), N, stamp);
      const o3s_localizability& loc = mapper.getLatestLocalizability();
      std::fprintf(out, "%lld %d %d %d %d %lld ", (long long)k, ok ? 1 : 0, mapper.lastScanInserted() ? 1 : 0, mapper.lastIcpThrew() ? 1 : 0,
                   mapper.lastRemapReplaced(), (long long)loc.kept);
      for (int j = 0; j < 6; ++j) std::fprintf(out, " %d", (int)loc.category[j]);
      std::fprintf(out, " ");
      for (int j = 0; j < 6; ++j) std::fprintf(out, " %lld", (long long)loc.n_strong[j]);
      put(out, mapper.mapToRangeSensor().m, 16);
      put(out, mapper.lastRegistrationPose().m, 16);
      put(out, mapper.lastPrior().m, 16);
      put(out, loc.centre, 3);
      put(out, &loc.evec[0][0], 18);
      put(out, loc.sum_all, 6);
      put(out, loc.sum_strong, 6);
      std::fprintf(out, "\n");
    }
  } catch (const std::exception& e) {
    std::fprintf(out, "exception %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
