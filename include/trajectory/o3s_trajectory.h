/*
 * o3s_trajectory.h — poses at any stamp, and the de-skew of a sweep along a measured trajectory (same shared library,
 * libo3dslam_icp_hip.so).  O3S = open3d_slam/src.
 *
 *   o3s_transform_interpolate     interpolate(start, end, time)                      O3S/src/Transform.cpp:16-67
 *   o3s_transform_extrapolate     extrapolate(start, end, future_time)               O3S/src/Transform.cpp:69-110
 *   o3s_trajectory_has / _lookup  TransformInterpolationBuffer::has / lookup         O3S/src/TransformInterpolationBuffer.cpp:100-149
 *   o3s_trajectory_get_transform  getTransform(time, buffer)                         O3S/src/TransformInterpolationBuffer.cpp:189-220
 *   o3s_*_undistort_trajectory    (no counterpart: the reference de-skews with a constant velocity only)
 *
 * The first five are host arithmetic: they open no device and work on a machine without a GPU (o3s_motion_from_poses set the
 * precedent).  fp64, no FMA contraction.  Eigen is not part of the tree, so its three pieces are restated from the published
 * algorithms (parity unpinned at the Eigen boundary):
 *   Quaterniond(Matrix3d)    the branch on the trace, then on the largest diagonal element; not renormalised
 *   slerp(f, other)          d = q0 . q1; |d| >= 1 - eps (eps = 2^-52): scales 1 - f and f; else theta = acos|d| and the scales are
 *                            sin((1 - f) theta) / sin theta and sin(f theta) / sin theta; the second scale is negated when d < 0
 *   AngleAxisd(Quaterniond)  n = |vec|; angle = 2 atan2(n, |w|); axis = vec / n, negated when w < 0; n == 0: angle 0 about x
 * and Quaternion::toRotationMatrix is applied to a slerp's result WITHOUT renormalising it, as Eigen does.
 *
 * (The header lives in a directory of its own: include/ itself holds the headers of the device-side ABI, one list.)
 * Conventions: poses are 4x4 doubles in column-major order, stamps are double seconds.  Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_TRAJECTORY_H
#define O3S_TRAJECTORY_H

#include <stdint.h>

#include "../o3s_icp.h"
#include "../o3s_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TimestampedTransform.  A table of K of them is in buffer order: the order of the pushes, stamps not decreasing. */
typedef struct o3s_stamped_pose {
  double t;
  double T[16];
} o3s_stamped_pose;

/* The largest table a de-skew accepts: the reference's buffer size limit (TransformInterpolationBuffer.cpp:16). */
#define O3S_TRAJECTORY_MAX_POSES 2000

/* interpolate: the ends are swapped when start->t > end->t; a query outside the ends is O3S_ERR_BAD_ARGUMENT (the reference
 * throws).  factor = (t - t0) / ((t1 - t0) + 1e-6) — NOT (t - t0) / (t1 - t0): the query at t1 stops short of the end pose —,
 * translation = p0 + (p1 - p0) factor, rotation = toRotationMatrix(Quaterniond(R0).slerp(factor, Quaterniond(R1))).
 * out->t = t; the last row of out->T is (0, 0, 0, 1). */
int o3s_transform_interpolate(const o3s_stamped_pose* start, const o3s_stamped_pose* end, double t, o3s_stamped_pose* out);

/* extrapolate: O3S_ERR_BAD_ARGUMENT for start->t > end->t and for a duration end->t - start->t <= 0 (the reference throws);
 * t < end->t returns *end (stamp included).  Else translation = p_end + (p_end - p_start) / duration * (t - end->t) and
 * rotation = q_end * AngleAxis(angle * (t - end->t), axis) with (angle, axis) = AngleAxis(q_end * q_start^-1).
 * The angle is NOT divided by the duration: the reference turns on by the whole angle between the two poses per second,
 * whatever time lies between them.  The quirk is kept. */
int o3s_transform_extrapolate(const o3s_stamped_pose* start, const o3s_stamped_pose* end, double t, o3s_stamped_pose* out);

/* has: 1 when K > 0 and poses[0].t <= t <= poses[K - 1].t, else 0 (also for a null table). */
int o3s_trajectory_has(const o3s_stamped_pose* poses, int64_t K, double t);

/* lookup: a stamp the table does not cover is O3S_ERR_BAD_ARGUMENT (the reference throws).  K == 1 returns that pose.  Else the
 * first entry with t <= entry.t (the first of equal stamps): an exact stamp returns that entry's pose untouched, every other
 * stamp interpolates from the entry before it. */
int o3s_trajectory_lookup(const o3s_stamped_pose* poses, int64_t K, double t, double out_T[16]);

/* getTransform: before the earliest stamp the earliest pose; after the latest, extrapolate(poses[K - 3], poses[K - 1], t) —
 * the start is the THIRD pose from the end (latest_offseted_measurement(2)); else lookup.
 * The one deliberate departure: with K < 3 the reference walks off the front of its deque there; this returns the latest
 * pose, which is what the reference's own commented-out line did.  K <= 0 is O3S_ERR_BAD_ARGUMENT. */
int o3s_trajectory_get_transform(const o3s_stamped_pose* poses, int64_t K, double t, double out_T[16]);

/* De-skew of a sweep along the trajectory.  Per point, in fp64, no contraction, in place, one lane per point:
 *   p'_i = A * G(stamp + s_i) * C^-1 * p_i,   A = (G(stamp) * C^-1)^-1
 * G = o3s_trajectory_get_transform over `poses` (clamp, exact knot, interpolation, extrapolation as above), C = calibration
 * (odometry frame to cloud frame; the identity is allowed), s_i = the point's time offset: dt[i] where point times were given,
 * else computePhase(x, y) * scan_duration as in o3s_motion.  This is the motion the mapper's own prior is made of
 * (odomToRangeSensorPrev^-1 * odomToRangeSensor, Mapper.cpp:270-276), evaluated per point: a point measured at stamp + s_i is
 * expressed in the sensor frame at `stamp`.  Only the points are rewritten (normals and colours stay).
 * The knot quaternions, A and C^-1 are computed once on the host.  A knot the kernel lands on exactly is used as
 * {translation, quaternion}: its rotation is toRotationMatrix of the knot's quaternion, an ulp or two from the pushed matrix.
 * K == 1 launches nothing (G is constant: the result is p, bit for bit); a table of equal poses does launch.
 * A point whose stamp + s_i is not a number comes out as NaN.
 * O3S_ERR_BAD_ARGUMENT: K < 1 or K > O3S_TRAJECTORY_MAX_POSES; stamps that decrease along the table; K >= 3 with
 * poses[K - 3].t == poses[K - 1].t (the extrapolation any point may ask for is undefined); no point times and
 * scan_duration <= 0. */
typedef struct o3s_trajectory_deskew {
  double stamp;          /* the sweep's stamp: the frame every point is expressed in afterwards */
  double scan_duration;  /* seconds; read only when no point times were given */
  double calibration[16];
  int32_t is_spinning_clockwise;
  int32_t reserved[3];
} o3s_trajectory_deskew;

/* Per-point time offsets (seconds after the sweep's stamp) of the sweep staged in r, from the driver.  N must equal the staged
 * size (else O3S_ERR_BAD_ARGUMENT, the sweep and earlier times untouched); the next o3s_raw_scan_upload drops them. */
int o3s_raw_scan_set_point_times(o3s_raw_scan* r, const double* dt, int64_t N);
/* In place on the staged sweep, on r's stream; call it before o3s_scan_preprocess_staged.  Returns when the sweep is rewritten.
 * A refused call has not touched the staged sweep. */
int o3s_raw_scan_undistort_trajectory(o3s_raw_scan* r, const o3s_stamped_pose* poses, int64_t K, const o3s_trajectory_deskew* params);
/* The same on host buffers of N points (3 doubles each, dt: N doubles or NULL); out may alias pts.  N == 0 is O3S_OK. */
int o3s_undistort_cloud_trajectory(int device, const o3s_stamped_pose* poses, int64_t K, const o3s_trajectory_deskew* params,
                                   const double* pts, const double* dt, int64_t N, double* out);

#ifdef __cplusplus
}
#endif

#endif
