// cpp/o3s_odometry.hpp's TransformInterpolationBuffer and getTransform on a scenario read from a file: plain g++, only
// libo3dslam_icp_hip.so at link time, no device is opened.
//
//   trajectory_cases <in.txt>
// in.txt (doubles as %a):  "limit P Q", then P lines "t T(16, column-major)" (the pushes, in order), then one line of Q query stamps.
// stdout: "size earliest latest", then per query "has lookup_ok  getTransform(16)  lookup(16, when it did not throw)".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "o3s_odometry.hpp"

static double rd(FILE* f) {
  char w[64];
  if (std::fscanf(f, "%63s", w) != 1) {
    std::fprintf(stderr, "input truncated\n");
    std::exit(2);
  }
  return std::strtod(w, nullptr);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int limit = (int)rd(f), P = (int)rd(f), Q = (int)rd(f);
  try {
    o3s::TransformInterpolationBuffer b((std::size_t)limit);
    if (!b.empty() || b.has(0.0)) throw std::runtime_error("a new buffer must be empty");
    for (int k = 0; k < P; ++k) {
      const double t = rd(f);
      o3s::Mat4 T;
      for (int i = 0; i < 16; ++i) T.m[i] = rd(f);
      b.push(t, T);
    }
    std::printf("%zu %a %a\n", b.size(), b.earliest_time(), b.latest_time());
    for (int k = 0; k < Q; ++k) {
      const double t = rd(f);
      const o3s::Mat4 G = o3s::getTransform(t, b);
      bool ok = true;
      o3s::Mat4 L{};
      try {
        L = b.lookup(t);
      } catch (const std::runtime_error&) {
        ok = false;
      }
      std::printf("%d %d", b.has(t) ? 1 : 0, ok ? 1 : 0);
      for (int i = 0; i < 16; ++i) std::printf(" %a", G.m[i]);
      if (ok)
        for (int i = 0; i < 16; ++i) std::printf(" %a", L.m[i]);
      std::printf("\n");
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "trajectory_cases: %s\n", e.what());
    return 1;
  }
  std::fclose(f);
  return 0;
}
