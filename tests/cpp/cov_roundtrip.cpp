// The pose covariance through the C++ shim (cpp/o3s_icp.hpp), the way a catkin package would read it: plain g++, only
// libo3dslam_icp_hip.so at link time.
//   cov_roundtrip <ref_xyzw.f32> <ref_normals.f32> <M> <scan_xyzw.f32> <scan_normals.f32> <N> <T_init.f32> <sensorStdDev>
// Prints "none <what getCovariance() does before a compute>", "T <16 floats>", "cov <36 doubles as hex bit patterns, column-major>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "o3s_icp.hpp"

static std::vector<float> read_f32(const char* path, size_t n) {
  std::vector<float> v(n);
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(float)));
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path);
    std::exit(2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 9) return 2;
  const long M = std::atol(argv[3]), N = std::atol(argv[6]);
  const auto ref = read_f32(argv[1], (size_t)M * 4), refn = read_f32(argv[2], (size_t)M * 3);
  const auto scan = read_f32(argv[4], (size_t)N * 4), scann = read_f32(argv[5], (size_t)N * 3);
  const auto T0 = read_f32(argv[7], 16);
  try {
    o3s_icp_config cfg;
    o3s_icp_default_config(&cfg);
    cfg.error_minimizer = 1;  // PointToPlaneWithCovErrorMinimizer
    cfg.sensor_std_dev = (float)std::atof(argv[8]);
    o3s::IcpHip icp(cfg, 0);
    try {
      (void)icp.getCovariance();
      std::printf("none no-throw\n");
    } catch (const std::runtime_error&) {
      std::printf("none runtime_error\n");
    }
    if (!icp.initReference(ref.data(), refn.data(), M)) return 3;
    float T[16];
    icp.compute(scan.data(), scann.data(), N, T0.data(), T);
    std::printf("T");
    for (float v : T) std::printf(" %.9g", v);
    const std::array<double, 36> c = icp.getCovariance();
    std::printf("\ncov");
    for (double v : c) {
      std::uint64_t bits;
      std::memcpy(&bits, &v, 8);
      std::printf(" %016" PRIx64, bits);
    }
    std::printf("\n");
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  return 0;
}
