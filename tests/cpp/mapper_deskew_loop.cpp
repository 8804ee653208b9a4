// Drives cpp/o3s_mapper.hpp with its motion compensation switched on (MapperHip::enableMotionCompensation:
// motionCompensationMap_ over getMapToRangeSensorBuffer(), SlamWrapper.cpp:445-447, 671) over recorded sweeps: plain g++, only
// libo3dslam_icp_hip.so at link time.
//
//   mapper_deskew_loop <sweeps.bin> <out.txt>
// sweeps.bin (little endian):
//   double scan_voxel, map_voxel, wide_radius, narrow_radius, ref_period, scan_duration;  int64 clockwise, num_poses, staged, K
//   K x { double stamp; int64 N; double pts[3N]; double normals[3N] }
// staged = 0: the sweeps are handed over as host arrays (de-skewed inside addRangeMeasurement); 1: the driver stages each sweep and
// calls MapperHip::undistort before it hands the staged sweep over.
// out.txt: one line per sweep "k ok buffer_size  T(16, %a)  v(3, %a) w(3, %a)".
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
    std::fprintf(stderr, "sweeps truncated\n");
    std::exit(2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) return 2;
  o3s::MapperParams p;
  p.scanVoxelSize = rd<double>(f);
  p.mapVoxelSize = rd<double>(f);
  p.mapBuilderCropper.kind = 1;  // MaxRadius
  p.mapBuilderCropper.p0 = rd<double>(f);
  p.scanMatcherCropper.kind = 1;
  p.scanMatcherCropper.p0 = rd<double>(f);
  p.referenceCloudSettingPeriod = rd<double>(f);
  const double scan_duration = rd<double>(f);
  const std::int64_t clockwise = rd<std::int64_t>(f), num_poses = rd<std::int64_t>(f), staged_mode = rd<std::int64_t>(f), K = rd<std::int64_t>(f);
  p.submaps.radius = 1.0e9;  // one submap
  p.submaps.minNumRangeData = 5;
  p.submaps.maxNumPoints = 1000000000000LL;
  p.submaps.numScansOverlap = 3;
  FILE* out = std::fopen(argv[2], "w");
  if (!out) return 2;
  try {
    o3s_icp_config cfg;
    o3s_icp_default_config(&cfg);
    o3s::MapperHip m(p, cfg, 0);
    m.setCalibration(o3s::Mat4::identity());
    if (m.isMotionCompensationEnabled()) throw std::runtime_error("the motion compensation must be off by default");
    m.enableMotionCompensation(scan_duration, clockwise != 0, (int)num_poses);
    o3s_raw_scan* staged = nullptr;
    if (staged_mode && o3s_raw_scan_create(0, &staged) != O3S_OK) throw std::runtime_error("o3s_raw_scan_create failed");
    std::vector<double> pts, nrm;
    for (std::int64_t k = 0; k < K; ++k) {
      const double stamp = rd<double>(f);
      const std::int64_t N = rd<std::int64_t>(f);
      pts.resize((size_t)N * 3);
      nrm.resize((size_t)N * 3);
      f.read(reinterpret_cast<char*>(pts.data()), (std::streamsize)(pts.size() * 8));
      f.read(reinterpret_cast<char*>(nrm.data()), (std::streamsize)(nrm.size() * 8));
      if (!f) throw std::runtime_error("sweeps truncated");
      bool ok;
      if (staged_mode) {
        if (o3s_raw_scan_upload(staged, pts.data(), nrm.data(), N) != O3S_OK) throw std::runtime_error("o3s_raw_scan_upload failed");
        m.undistort(staged, stamp);
        ok = m.addRangeMeasurement(staged, stamp);
      } else {
        ok = m.addRangeMeasurement(pts.data(), nrm.data(), N, stamp);
      }
      std::fprintf(out, "%lld %d %zu ", (long long)k, ok ? 1 : 0, m.getMapToRangeSensorBuffer().size());
      for (int i = 0; i < 16; ++i) std::fprintf(out, " %a", m.mapToRangeSensor().m[i]);
      for (int i = 0; i < 3; ++i) std::fprintf(out, " %a", m.lastMotion().linear_velocity[i]);
      for (int i = 0; i < 3; ++i) std::fprintf(out, " %a", m.lastMotion().angular_velocity_rpy[i]);
      std::fprintf(out, "\n");
    }
    o3s_raw_scan_destroy(staged);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mapper_deskew_loop: %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
