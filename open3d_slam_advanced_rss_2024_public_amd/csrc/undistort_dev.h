// undistort_dev.h — constant-velocity de-skew of a spinning-LiDAR sweep (include/o3s_scan.h: o3s_motion), gfx950 only:
// ConstantVelocityMotionCompensation::undistortInputPointCloud (O3S/src/MotionCompensation.cpp:73-127) restated per point,
// and the host arithmetic of estimateLinearAndAngularVelocity (:32-66).  Included by cloud_ops.hip after cloud_dev.h.
//
// fp64, no FMA contraction.  One lane per point; a lane reads and writes only its own 24 bytes, so the kernel runs in place.
// No LDS, no atomics, no scratch (profiles/undistort/resource_usage.txt).
#pragma once
#include "../../include/o3s_scan.h"
#include "cloud_dev.h"

#pragma clang fp contract(off)

namespace {
namespace o3s_cloud {

struct MotionArgs {  // o3s_motion as the kernel takes it (by value)
  double v[3], w[3], T;
  int clockwise;
};

// Hamilton product a * b, components (w, x, y, z)
__host__ __device__ __forceinline__ void quat_mul(const double a[4], const double b[4], double o[4]) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
  o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}

// computePhase (MotionCompensation.cpp:129-151): the share of the sweep that had passed when the beam looked along (x, y)
__host__ __device__ __forceinline__ double sweep_phase(double x, double y, int clockwise) {
  constexpr double kTwoPi = 2.0 * 3.14159265358979323846;
  const double angle = atan2(y, x);
  const double wrapped = angle < 0.0 ? (angle + kTwoPi) : angle;
  if (wrapped == 0.0) return 0.0;
  return clockwise ? 1.0 - wrapped / kTwoPi : wrapped / kTwoPi;
}

// p' = R(q) p + s v with q = yaw(s wz) * pitch(s wy) * roll(s wx) (math.cpp:32-37), normalised, s = phase * scan duration
__global__ void __launch_bounds__(kB) k_undistort(double* __restrict__ pts, int64_t N, MotionArgs m) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
  const double s = sweep_phase(px, py, m.clockwise) * m.T;
  const double hr = 0.5 * (s * m.w[0]), hp = 0.5 * (s * m.w[1]), hy = 0.5 * (s * m.w[2]);
  const double qr[4] = {cos(hr), sin(hr), 0.0, 0.0};
  const double qp[4] = {cos(hp), 0.0, sin(hp), 0.0};
  const double qy[4] = {cos(hy), 0.0, 0.0, sin(hy)};
  double qyp[4], q[4];
  quat_mul(qy, qp, qyp);
  quat_mul(qyp, qr, q);
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
  // Quaternion::toRotationMatrix
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const double r00 = 1.0 - (tyy + tzz), r01 = txy - twz, r02 = txz + twy;
  const double r10 = txy + twz, r11 = 1.0 - (txx + tzz), r12 = tyz - twx;
  const double r20 = txz - twy, r21 = tyz + twx, r22 = 1.0 - (txx + tyy);
  pts[3 * i] = (r00 * px + r01 * py + r02 * pz) + s * m.v[0];
  pts[3 * i + 1] = (r10 * px + r11 * py + r12 * pz) + s * m.v[1];
  pts[3 * i + 2] = (r20 * px + r21 * py + r22 * pz) + s * m.v[2];
}

// what every de-skew entry checks before it touches a device
inline bool motion_valid(const o3s_motion* m) { return m && m->scan_duration > 0.0; }
inline bool motion_is_zero(const o3s_motion& m) {
  for (int k = 0; k < 3; ++k)
    if (m.linear_velocity[k] != 0.0 || m.angular_velocity_rpy[k] != 0.0) return false;
  return true;
}

// N points at d_pts, in place, on stream s (N > 0, the motion is not zero)
inline int undistort_dev(double* d_pts, int64_t N, const o3s_motion& m, hipStream_t s) {
  MotionArgs a;
  for (int k = 0; k < 3; ++k) {
    a.v[k] = m.linear_velocity[k];
    a.w[k] = m.angular_velocity_rpy[k];
  }
  a.T = m.scan_duration;
  a.clockwise = m.is_spinning_clockwise ? 1 : 0;
  hipLaunchKernelGGL(k_undistort, dim3(nblk(N)), dim3(kB), 0, s, d_pts, N, a);
  CK(hipGetLastError());
  return O3S_OK;
}

// Eigen::Quaterniond(Matrix3d): the branch on the trace and the largest diagonal element; q = (w, x, y, z), not normalised
// (shared with trajectory_dev.h)
inline void quat_from_rotation(const double R[3][3], double q[4]) {
  const double tr = R[0][0] + R[1][1] + R[2][2];
  if (tr > 0.0) {
    double u = std::sqrt(tr + 1.0);
    q[0] = 0.5 * u;
    u = 0.5 / u;
    q[1] = (R[2][1] - R[1][2]) * u;
    q[2] = (R[0][2] - R[2][0]) * u;
    q[3] = (R[1][0] - R[0][1]) * u;
  } else {
    int i = 0;
    if (R[1][1] > R[0][0]) i = 1;
    if (R[2][2] > R[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double u = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
    q[1 + i] = 0.5 * u;
    u = 0.5 / u;
    q[0] = (R[k][j] - R[j][k]) * u;
    q[1 + j] = (R[j][i] + R[i][j]) * u;
    q[1 + k] = (R[k][i] + R[i][k]) * u;
  }
}

// estimateLinearAndAngularVelocity for start / finish already taken from the buffer (4x4 column-major isometries)
inline void motion_from_poses(const double A[16], double ta, const double B[16], double tb, o3s_motion* m) {
  for (int k = 0; k < 3; ++k) m->linear_velocity[k] = m->angular_velocity_rpy[k] = 0.0;
  const double dt = tb - ta;
  if (!(dt > 0.0)) return;
  // dT = start^-1 * finish: R = Ra^T Rb, t = Ra^T (tb - ta)
  double R[3][3], t[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      double v = A[r * 4 + 0] * B[c * 4 + 0];
      v = v + A[r * 4 + 1] * B[c * 4 + 1];
      v = v + A[r * 4 + 2] * B[c * 4 + 2];
      R[r][c] = v;
    }
    double v = A[r * 4 + 0] * (B[12] - A[12]);
    v = v + A[r * 4 + 1] * (B[13] - A[13]);
    v = v + A[r * 4 + 2] * (B[14] - A[14]);
    t[r] = v;
  }
  double q[4];  // w, x, y, z
  quat_from_rotation(R, q);
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  const double d = dt + 1e-6;
  // toRPY (math.hpp:30-42)
  m->angular_velocity_rpy[0] = std::atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)) / d;
  m->angular_velocity_rpy[1] = std::asin(2 * (w * y - x * z)) / d;
  m->angular_velocity_rpy[2] = std::atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z)) / d;
  for (int k = 0; k < 3; ++k) m->linear_velocity[k] = t[k] / d;
}

}  // namespace o3s_cloud
}  // namespace
