// trajectory_dev.h — poses at any stamp and the de-skew of a sweep along a measured trajectory
// (include/trajectory/o3s_trajectory.h), gfx950 only.  Included by cloud_ops.hip after undistort_dev.h.
//
// Host: interpolate / extrapolate (O3S/src/Transform.cpp:16-110) and TransformInterpolationBuffer::has / lookup / getTransform
// (TransformInterpolationBuffer.cpp:100-149, 189-220) over a table of stamped poses; Eigen's slerp, AngleAxis(Quaternion) and
// toRotationMatrix restated from the published algorithms.  The pieces a point needs are __host__ __device__, so the kernel and
// the host functions run the same statements.
//
// Device: k_undistort_trajectory, p' = A * G(stamp + s) * C^-1 * p.  fp64, no FMA contraction.  One lane per point; a lane reads
// and writes only its own 24 bytes (and its own time offset), so the kernel runs in place.  The table is K stamps followed by K
// knots {translation, quaternion} in global memory; a lane finds its segment by a binary search over the stamps (at most 11 steps
// for 2000 knots; the lanes of a wave look along neighbouring azimuths, so they walk the same few cache lines).  No LDS, no atomics,
// no scratch (profiles/trajectory/resource_usage.txt).
#pragma once
#include <vector>

#include "../../include/trajectory/o3s_trajectory.h"
#include "undistort_dev.h"

#pragma clang fp contract(off)

namespace {
namespace o3s_cloud {

// Eigen::Quaterniond::slerp(f, q1) of q0, components (w, x, y, z); the result is not normalised
__host__ __device__ __forceinline__ void quat_slerp(const double q0[4], const double q1[4], double f, double o[4]) {
  constexpr double kOne = 1.0 - 2.220446049250313e-16;
  const double d = q0[0] * q1[0] + q0[1] * q1[1] + q0[2] * q1[2] + q0[3] * q1[3];
  const double ad = fabs(d);
  double s0, s1;
  if (ad >= kOne) {
    s0 = 1.0 - f;
    s1 = f;
  } else {
    const double theta = acos(ad);
    const double st = sin(theta);
    s0 = sin((1.0 - f) * theta) / st;
    s1 = sin(f * theta) / st;
  }
  if (d < 0.0) s1 = -s1;
  o[0] = s0 * q0[0] + s1 * q1[0];
  o[1] = s0 * q0[1] + s1 * q1[1];
  o[2] = s0 * q0[2] + s1 * q1[2];
  o[3] = s0 * q0[3] + s1 * q1[3];
}

// Quaternion::toRotationMatrix of q as it is (no normalisation), row-major R[3 * r + c]
__host__ __device__ __forceinline__ void quat_to_rotation(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}

// interpolate (Transform.cpp:57-64) between two knots whose stamps are in order: t0 <= t <= t1
__host__ __device__ __forceinline__ void knot_interpolate(double t0, const double p0[3], const double q0[4], double t1, const double p1[3],
                                                          const double q1[4], double t, double p[3], double q[4]) {
  const double duration = t1 - t0;
  const double factor = (t - t0) / (duration + 1e-6);  // "avoid zero division": the end pose is never reached
  p[0] = p0[0] + (p1[0] - p0[0]) * factor;
  p[1] = p0[1] + (p1[1] - p0[1]) * factor;
  p[2] = p0[2] + (p1[2] - p0[2]) * factor;
  quat_slerp(q0, q1, factor, q);
}

// what extrapolate (Transform.cpp:76-104) keeps of its two poses: everything but the future stamp
struct Extrapolation {
  double t_end, p_end[3], q_end[4], velocity[3], axis[3], angle;
};

__host__ __device__ __forceinline__ void extrapolate_eval(const Extrapolation& e, double t, double p[3], double q[4]) {
  const double future = t - e.t_end;
  p[0] = e.p_end[0] + e.velocity[0] * future;
  p[1] = e.p_end[1] + e.velocity[1] * future;
  p[2] = e.p_end[2] + e.velocity[2] * future;
  const double half = 0.5 * (e.angle * future);  // the angle of the whole interval, per second: not divided by the duration
  const double sh = sin(half);
  const double turn[4] = {cos(half), sh * e.axis[0], sh * e.axis[1], sh * e.axis[2]};
  quat_mul(e.q_end, turn, q);
}

struct TrajectoryArgs {  // what the kernel takes by value
  double A[12], Cinv[12];  // rows of [R | t], row-major 3 x 4
  double stamp, t_first, t_last, T;
  int K, clockwise;
};

__host__ __device__ __forceinline__ void apply34(const double M[12], double x, double y, double z, double o[3]) {
  o[0] = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  o[1] = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  o[2] = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

// tab: K stamps, then K knots of 7 doubles (translation, quaternion w x y z), then the Extrapolation of the table's end (read by
// the lanes beyond the latest stamp only)
__global__ void __launch_bounds__(kB) k_undistort_trajectory(double* __restrict__ pts, const double* __restrict__ dt, int64_t N,
                                                             const double* __restrict__ tab, TrajectoryArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
  const double s = dt ? dt[i] : sweep_phase(px, py, a.clockwise) * a.T;
  const double t = a.stamp + s;
  const int K = a.K;
  const double* knots = tab + K;
  double p[3], q[4];
  int exact = -1;  // the knot to take as it is
  if (!(t == t)) {
    const double nan = t;
    pts[3 * i] = nan, pts[3 * i + 1] = nan, pts[3 * i + 2] = nan;
    return;
  }
  if (t < a.t_first) {
    exact = 0;
  } else if (t > a.t_last) {
    if (K < 3)
      exact = K - 1;
    else
      extrapolate_eval(*reinterpret_cast<const Extrapolation*>(tab + 8 * (size_t)K), t, p, q);
  } else {  // lookup: the first knot with t <= its stamp, which exists (t <= t_last)
    int lo = 0, hi = K - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t <= tab[mid])
        hi = mid;
      else
        lo = mid + 1;
    }
    const double t1 = tab[lo];
    if (t1 == t || lo == 0) {
      exact = lo;
    } else {
      const double* k0 = knots + 7 * (lo - 1);
      const double* k1 = knots + 7 * lo;
      const double p0[3] = {k0[0], k0[1], k0[2]}, q0[4] = {k0[3], k0[4], k0[5], k0[6]};
      const double p1[3] = {k1[0], k1[1], k1[2]}, q1[4] = {k1[3], k1[4], k1[5], k1[6]};
      knot_interpolate(tab[lo - 1], p0, q0, t1, p1, q1, t, p, q);
    }
  }
  if (exact >= 0) {
    const double* k = knots + 7 * exact;
    p[0] = k[0], p[1] = k[1], p[2] = k[2];
    q[0] = k[3], q[1] = k[4], q[2] = k[5], q[3] = k[6];
  }
  double R[9], c[3], g[3], o[3];
  quat_to_rotation(q, R);
  apply34(a.Cinv, px, py, pz, c);
  g[0] = ((R[0] * c[0] + R[1] * c[1]) + R[2] * c[2]) + p[0];
  g[1] = ((R[3] * c[0] + R[4] * c[1]) + R[5] * c[2]) + p[1];
  g[2] = ((R[6] * c[0] + R[7] * c[1]) + R[8] * c[2]) + p[2];
  apply34(a.A, g[0], g[1], g[2], o);
  pts[3 * i] = o[0];
  pts[3 * i + 1] = o[1];
  pts[3 * i + 2] = o[2];
}

// ---- host arithmetic ----

inline void pose_rotation(const double T[16], double R[3][3]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[r][c] = T[c * 4 + r];
}
inline void pose_quat(const double T[16], double q[4]) {
  double R[3][3];
  pose_rotation(T, R);
  quat_from_rotation(R, q);
}
inline void pose_from(const double p[3], const double q[4], double T[16]) {
  double R[9];
  quat_to_rotation(q, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[c * 4 + r] = R[3 * r + c];
    T[12 + r] = p[r];
    T[r * 4 + 3] = 0.0;
  }
  T[15] = 1.0;
}
// 4x4 column-major product and isometry inverse, plain k = 0..3 accumulation (cpp/o3s_pose.hpp)
inline void mul44(const double A[16], const double B[16], double C[16]) {
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      double s = A[r] * B[c * 4];
      s = s + A[4 + r] * B[c * 4 + 1];
      s = s + A[8 + r] * B[c * 4 + 2];
      s = s + A[12 + r] * B[c * 4 + 3];
      C[c * 4 + r] = s;
    }
}
inline void inverse_isometry44(const double T[16], double I[16]) {
  for (int k = 0; k < 16; ++k) I[k] = (k % 5 == 0) ? 1.0 : 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) I[c * 4 + r] = T[r * 4 + c];
  for (int r = 0; r < 3; ++r) {
    double s = I[r] * T[12];
    s = s + I[4 + r] * T[13];
    s = s + I[8 + r] * T[14];
    I[12 + r] = -s;
  }
}
inline void rows34(const double T[16], double M[12]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) M[4 * r + c] = T[c * 4 + r];
}

inline int transform_interpolate(const o3s_stamped_pose* start, const o3s_stamped_pose* end, double t, o3s_stamped_pose* out) {
  if (start->t > end->t) std::swap(start, end);  // "REPORT TO TURCAN" (Transform.cpp:20-40)
  if (t > end->t || t < start->t) return O3S_ERR_BAD_ARGUMENT;
  double q0[4], q1[4], p[3], q[4];
  pose_quat(start->T, q0);
  pose_quat(end->T, q1);
  knot_interpolate(start->t, start->T + 12, q0, end->t, end->T + 12, q1, t, p, q);
  o3s_stamped_pose r;
  r.t = t;
  pose_from(p, q, r.T);
  *out = r;
  return O3S_OK;
}

// the part of extrapolate that does not depend on the future stamp
inline int extrapolation_from(const o3s_stamped_pose* start, const o3s_stamped_pose* end, Extrapolation* e) {
  if (start->t > end->t) return O3S_ERR_BAD_ARGUMENT;
  const double duration = end->t - start->t;
  if (duration <= 0.0 || duration != duration) return O3S_ERR_BAD_ARGUMENT;
  double qs[4];
  pose_quat(start->T, qs);
  pose_quat(end->T, e->q_end);
  e->t_end = end->t;
  for (int k = 0; k < 3; ++k) {
    e->p_end[k] = end->T[12 + k];
    e->velocity[k] = (end->T[12 + k] - start->T[12 + k]) / duration;
  }
  // Quaternion::inverse: conjugate / squaredNorm
  const double n2 = qs[0] * qs[0] + qs[1] * qs[1] + qs[2] * qs[2] + qs[3] * qs[3];
  const double qi[4] = {qs[0] / n2, -qs[1] / n2, -qs[2] / n2, -qs[3] / n2};
  double d[4];
  quat_mul(e->q_end, qi, d);
  // AngleAxisd(Quaterniond)
  double n = std::sqrt(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
  if (n != 0.0) {
    e->angle = 2.0 * std::atan2(n, std::fabs(d[0]));
    if (d[0] < 0.0) n = -n;
    for (int k = 0; k < 3; ++k) e->axis[k] = d[1 + k] / n;
  } else {
    e->angle = 0.0;
    e->axis[0] = 1.0, e->axis[1] = 0.0, e->axis[2] = 0.0;
  }
  return O3S_OK;
}

inline int transform_extrapolate(const o3s_stamped_pose* start, const o3s_stamped_pose* end, double t, o3s_stamped_pose* out) {
  Extrapolation e;
  const int rc = extrapolation_from(start, end, &e);
  if (rc != O3S_OK) return rc;
  if (t - end->t < 0.0) {  // "Future time is before the end time": the end pose
    const o3s_stamped_pose r = *end;
    *out = r;
    return O3S_OK;
  }
  double p[3], q[4];
  extrapolate_eval(e, t, p, q);
  o3s_stamped_pose r;
  r.t = t;
  pose_from(p, q, r.T);
  *out = r;
  return O3S_OK;
}

inline bool trajectory_has(const o3s_stamped_pose* poses, int64_t K, double t) {
  return poses && K > 0 && poses[0].t <= t && t <= poses[K - 1].t;
}

inline int trajectory_lookup(const o3s_stamped_pose* poses, int64_t K, double t, double out[16]) {
  if (!trajectory_has(poses, K, t)) return O3S_ERR_BAD_ARGUMENT;
  int64_t j = 0;
  if (K > 1) {
    int64_t lo = 0, hi = K - 1;  // std::find_if(time <= tf.time_) over stamps that do not decrease; it exists (t <= latest)
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (t <= poses[mid].t)
        hi = mid;
      else
        lo = mid + 1;
    }
    j = lo;
  }
  if (K == 1 || poses[j].t == t || j == 0) {
    std::memmove(out, poses[j].T, sizeof(double) * 16);
    return O3S_OK;
  }
  o3s_stamped_pose r;
  const int rc = transform_interpolate(&poses[j - 1], &poses[j], t, &r);
  if (rc != O3S_OK) return rc;
  std::memcpy(out, r.T, sizeof(double) * 16);
  return O3S_OK;
}

inline int trajectory_get_transform(const o3s_stamped_pose* poses, int64_t K, double t, double out[16]) {
  if (!poses || K <= 0) return O3S_ERR_BAD_ARGUMENT;
  if (t < poses[0].t) {
    std::memmove(out, poses[0].T, sizeof(double) * 16);
    return O3S_OK;
  }
  if (t > poses[K - 1].t) {
    if (K < 3) {  // the departure: the reference reads before the front of its deque here
      std::memmove(out, poses[K - 1].T, sizeof(double) * 16);
      return O3S_OK;
    }
    o3s_stamped_pose r;
    const int rc = transform_extrapolate(&poses[K - 3], &poses[K - 1], t, &r);
    if (rc != O3S_OK) return rc;
    std::memcpy(out, r.T, sizeof(double) * 16);
    return O3S_OK;
  }
  return trajectory_lookup(poses, K, t, out);
}

// ---- one de-skew call: what the host prepares ----

inline bool trajectory_call_valid(const o3s_stamped_pose* poses, int64_t K, const o3s_trajectory_deskew* p, bool have_times) {
  if (!poses || !p || K < 1 || K > O3S_TRAJECTORY_MAX_POSES) return false;
  if (!have_times && !(p->scan_duration > 0.0)) return false;
  if (!(p->stamp == p->stamp)) return false;
  for (int64_t k = 0; k < K; ++k)
    if (!(poses[k].t == poses[k].t) || (k && poses[k].t < poses[k - 1].t)) return false;
  if (K >= 3 && !(poses[K - 1].t > poses[K - 3].t)) return false;
  return true;
}

// the kernel's arguments and its table (K stamps, K x {translation, quaternion}, the extrapolation) for a valid call
inline int trajectory_prepare(const o3s_stamped_pose* poses, int64_t K, const o3s_trajectory_deskew& p, TrajectoryArgs* a,
                              std::vector<double>* tab) {
  double Cinv[16], G[16], M[16], A[16];
  inverse_isometry44(p.calibration, Cinv);
  int rc = trajectory_get_transform(poses, K, p.stamp, G);
  if (rc != O3S_OK) return rc;
  mul44(G, Cinv, M);
  inverse_isometry44(M, A);
  rows34(A, a->A);
  rows34(Cinv, a->Cinv);
  Extrapolation ex{};
  if (K >= 3) {
    rc = extrapolation_from(&poses[K - 3], &poses[K - 1], &ex);
    if (rc != O3S_OK) return rc;
  }
  a->stamp = p.stamp;
  a->t_first = poses[0].t;
  a->t_last = poses[K - 1].t;
  a->T = p.scan_duration;
  a->K = (int)K;
  a->clockwise = p.is_spinning_clockwise ? 1 : 0;
  static_assert(sizeof(Extrapolation) == 15 * sizeof(double), "the table's tail is 15 doubles");
  tab->resize((size_t)K * 8 + 15);
  std::memcpy(tab->data() + 8 * (size_t)K, &ex, sizeof(ex));
  for (int64_t k = 0; k < K; ++k) {
    (*tab)[k] = poses[k].t;
    double* kn = tab->data() + K + 7 * k;
    for (int c = 0; c < 3; ++c) kn[c] = poses[k].T[12 + c];
    pose_quat(poses[k].T, kn + 3);
  }
  return O3S_OK;
}

// N points at d_pts (d_dt: their time offsets, or null), in place, on stream s; d_tab holds the table (N > 0, K > 1)
inline int undistort_trajectory_dev(double* d_pts, const double* d_dt, int64_t N, const double* d_tab, const TrajectoryArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_undistort_trajectory, dim3(nblk(N)), dim3(kB), 0, s, d_pts, d_dt, N, d_tab, a);
  CK(hipGetLastError());
  return O3S_OK;
}

}  // namespace o3s_cloud
}  // namespace
