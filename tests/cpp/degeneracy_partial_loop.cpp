// Drives cpp/o3s_mapper.hpp over recorded sweeps under the Constrain policy with MapperParams::degeneracyPartial: plain g++, only
// libo3dslam_icp_hip.so at link time.
//
//   degeneracy_partial_loop <scene.bin> <out.txt>
// scene.bin: the layout of tests/cpp/degeneracy_loop.cpp with one more int64 behind iters: partial (0 or 1).
// out.txt, one line per sweep:
//   "k ok inserted icp_threw iterations kept  cat(6)  T(16, %a)  n_masks masks...  n_partial partial_masks... values(6 n_partial, %a)"
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
static void put(FILE* out, const double* v, size_t n) {
  std::fprintf(out, " ");
  for (size_t i = 0; i < n; ++i) std::fprintf(out, " %a", v[i]);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) return 2;
  const std::int64_t policy = rd<std::int64_t>(f), min_category = rd<std::int64_t>(f), K = rd<std::int64_t>(f);
  const std::int64_t iters = rd<std::int64_t>(f), partial = rd<std::int64_t>(f);
  using Policy = o3s::MapperParams::DegeneracyPolicy;
  static const Policy policies[] = {Policy::Off, Policy::Report, Policy::Remap, Policy::Constrain};
  if (policy < 0 || policy > 3) return 2;
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
  p.degeneracyPolicy = policies[policy];
  p.localizability.filter_min = rd<double>(f);
  p.localizability.strong_min = rd<double>(f);
  p.localizability.sum_all_min = rd<double>(f);
  p.localizability.sum_strong_min = rd<double>(f);
  p.localizability.sum_partial_min = rd<double>(f);
  p.remapMinCategory = (std::int32_t)min_category;
  p.degeneracyPartial = partial != 0;
  const o3s::Mat4 first_pose = rd_mat(f);
  FILE* out = std::fopen(argv[2], "w");
  if (!out) return 2;
  try {
    o3s_icp_config cfg;
    o3s_icp_default_config(&cfg);  // icp.yaml
    if (iters > 0) {
      cfg.use_differential = 0;
      cfg.max_iters = (std::int32_t)iters;
    }
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
                   k ? mapper.lastIterations() : 0, (long long)loc.kept);
      for (int j = 0; j < 6; ++j) std::fprintf(out, " %d", (int)loc.category[j]);
      put(out, mapper.mapToRangeSensor().m, 16);
      const std::vector<std::int32_t> masks = k ? mapper.icp().degeneracyTrace() : std::vector<std::int32_t>();
      std::fprintf(out, "  %d", (int)masks.size());
      for (std::int32_t m : masks) std::fprintf(out, " %d", (int)m);
      o3s::IcpHip::DegeneracyPartialTrace t;
      if (k) t = mapper.icp().degeneracyPartialTrace();
      std::fprintf(out, "  %d", (int)t.partialMasks.size());
      for (std::int32_t m : t.partialMasks) std::fprintf(out, " %d", (int)m);
      put(out, t.values.data(), t.values.size());
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
