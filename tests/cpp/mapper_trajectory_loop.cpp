// Drives cpp/o3s_mapper.hpp with an external odometry source whose stamps are not the sweeps' (MapperParams::isInterpolateOdometry)
// and with the de-skew along that odometry (MapperHip::enableTrajectoryMotionCompensation) over recorded sweeps: plain g++, only
// libo3dslam_icp_hip.so at link time.
//
//   mapper_trajectory_loop <in.bin> <out.txt> <deskewed.bin>
// in.bin (little endian):
//   double scan_voxel, map_voxel, wide_radius, narrow_radius, ref_period, scan_duration, lead, calibration[16]
//   int64 clockwise, interpolate, trajectory, staged, M, K
//   M x { double stamp; double T[16] }                      the odometry poses, column-major, in stamp order
//   K x { double stamp; int64 N; int64 timed; double pts[3N]; double normals[3N]; double dt[N] if timed }
// Before sweep k every odometry pose with a stamp <= its stamp + lead is handed over.
// staged = 0: the sweeps are handed over as host arrays (de-skewed inside addRangeMeasurement, by azimuth); 1: the driver stages each
// sweep, sets its point times when it has some, calls MapperHip::undistortAlongOdometry, writes the staged sweep as it is then
// (read back through a pre-process that keeps every point) to deskewed.bin, and hands the staged sweep over.
// out.txt: one line per sweep "k ok buffer_size  T(16, %a)  prior(16, %a)".
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
    std::fprintf(stderr, "input truncated\n");
    std::exit(2);
  }
  return v;
}

static o3s::Mat4 rdMat(std::ifstream& f) {
  o3s::Mat4 T;
  for (int i = 0; i < 16; ++i) T.m[i] = rd<double>(f);
  return T;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
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
  const double scan_duration = rd<double>(f), lead = rd<double>(f);
  const o3s::Mat4 calibration = rdMat(f);
  const std::int64_t clockwise = rd<std::int64_t>(f), interpolate = rd<std::int64_t>(f), trajectory = rd<std::int64_t>(f);
  const std::int64_t staged_mode = rd<std::int64_t>(f), M = rd<std::int64_t>(f), K = rd<std::int64_t>(f);
  p.submaps.radius = 1.0e9;  // one submap
  p.submaps.minNumRangeData = 5;
  p.submaps.maxNumPoints = 1000000000000LL;
  p.submaps.numScansOverlap = 3;
  if (p.isInterpolateOdometry) {
    std::fprintf(stderr, "isInterpolateOdometry must be off by default\n");
    return 1;
  }
  p.isInterpolateOdometry = interpolate != 0;
  std::vector<double> odomStamps((size_t)M);
  std::vector<o3s::Mat4> odom((size_t)M);
  for (std::int64_t i = 0; i < M; ++i) {
    odomStamps[(size_t)i] = rd<double>(f);
    odom[(size_t)i] = rdMat(f);
  }
  FILE* out = std::fopen(argv[2], "w");
  FILE* cloud = std::fopen(argv[3], "wb");
  if (!out || !cloud) return 2;
  int status = 0;
  o3s_raw_scan* staged = nullptr;
  o3s_scan* readback = nullptr;
  try {
    o3s_icp_config cfg;
    o3s_icp_default_config(&cfg);
    o3s::MapperHip m(p, cfg, 0);
    m.setCalibration(calibration);
    if (m.isTrajectoryMotionCompensationEnabled()) throw std::runtime_error("the trajectory motion compensation must be off by default");
    if (trajectory) m.enableTrajectoryMotionCompensation(scan_duration, clockwise != 0);
    if (staged_mode) {
      if (o3s_raw_scan_create(0, &staged) != O3S_OK) throw std::runtime_error("o3s_raw_scan_create failed");
      if (o3s_scan_create(0, &readback) != O3S_OK) throw std::runtime_error("o3s_scan_create failed");
    }
    o3s_cropper everything{};
    everything.kind = 1;
    everything.p0 = 1.0e6;
    std::vector<double> pts, nrm, dt, back;
    std::int64_t fed = 0;
    for (std::int64_t k = 0; k < K; ++k) {
      const double stamp = rd<double>(f);
      const std::int64_t N = rd<std::int64_t>(f), timed = rd<std::int64_t>(f);
      pts.resize((size_t)N * 3);
      nrm.resize((size_t)N * 3);
      dt.resize(timed ? (size_t)N : 0);
      f.read(reinterpret_cast<char*>(pts.data()), (std::streamsize)(pts.size() * 8));
      f.read(reinterpret_cast<char*>(nrm.data()), (std::streamsize)(nrm.size() * 8));
      if (timed) f.read(reinterpret_cast<char*>(dt.data()), (std::streamsize)(dt.size() * 8));
      if (!f) throw std::runtime_error("sweeps truncated");
      while (fed < M && odomStamps[(size_t)fed] <= stamp + lead) {
        m.addOdometryPose(odomStamps[(size_t)fed], odom[(size_t)fed]);
        ++fed;
      }
      bool ok;
      if (staged_mode) {
        if (o3s_raw_scan_upload(staged, pts.data(), nrm.data(), N) != O3S_OK) throw std::runtime_error("o3s_raw_scan_upload failed");
        if (timed && o3s_raw_scan_set_point_times(staged, dt.data(), N) != O3S_OK) throw std::runtime_error("o3s_raw_scan_set_point_times failed");
        if (trajectory) m.undistortAlongOdometry(staged, stamp);
        std::int64_t nMerge = 0, nMatch = 0;
        if (o3s_scan_preprocess_staged(readback, &everything, 0.0, &everything, staged, &nMerge, &nMatch) != O3S_OK || nMerge != N)
          throw std::runtime_error("reading the staged sweep back failed");
        back.resize((size_t)N * 3);
        if (o3s_scan_get(readback, 0, back.data(), nullptr) != N) throw std::runtime_error("o3s_scan_get failed");
        std::fwrite(back.data(), 8, back.size(), cloud);
        ok = m.addRangeMeasurement(staged, stamp);
      } else {
        ok = m.addRangeMeasurement(pts.data(), nrm.data(), N, stamp);
      }
      std::fprintf(out, "%lld %d %zu ", (long long)k, ok ? 1 : 0, m.getMapToRangeSensorBuffer().size());
      for (int i = 0; i < 16; ++i) std::fprintf(out, " %a", m.mapToRangeSensor().m[i]);
      for (int i = 0; i < 16; ++i) std::fprintf(out, " %a", m.lastPrior().m[i]);
      std::fprintf(out, "\n");
    }
    // Mapper::getMapToRangeSensor / getMapToOdom at a stamp between two registered poses
    const o3s::Mat4 a = m.getMapToRangeSensor(0.234), b = m.getMapToOdom(0.234);
    std::fprintf(out, "at ");
    for (int i = 0; i < 16; ++i) std::fprintf(out, " %a", a.m[i]);
    for (int i = 0; i < 16; ++i) std::fprintf(out, " %a", b.m[i]);
    std::fprintf(out, "\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "mapper_trajectory_loop: %s\n", e.what());
    status = 1;
  }
  o3s_raw_scan_destroy(staged);
  o3s_scan_destroy(readback);
  std::fclose(out);
  std::fclose(cloud);
  return status;
}
