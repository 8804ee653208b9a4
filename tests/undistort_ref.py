"""numpy restatement of the constant-velocity de-skew and of its velocity estimate — the yardstick of tests/test_gpu_undistort.py
and tests/test_undistort_ref.py (pinned there by analysis):

  compute_phase / undistort   ConstantVelocityMotionCompensation::computePhase / undistortInputPointCloud
                              (open3d_slam/src/MotionCompensation.cpp:73-151), fromRPY (math.cpp:32-37)
  motion_from_poses           estimateLinearAndAngularVelocity (:32-66), toRPY (math.cpp:39-46, math.hpp:30-42)

float64 throughout; written from the formulas, independently of the library and of synthetic.py."""
import math

import numpy as np

TWO_PI = 2.0 * math.pi


def compute_phase(x, y, clockwise):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    angle = np.arctan2(y, x)
    wrapped = np.where(angle < 0.0, angle + TWO_PI, angle)
    phase = 1.0 - wrapped / TWO_PI if clockwise else wrapped / TWO_PI
    return np.where(wrapped == 0.0, 0.0, phase)


def quat_mul(a, b):
    """Hamilton product of (..., 4) arrays, components (w, x, y, z)."""
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx], axis=-1)


def axis_quat(angle, axis):
    """Quaternion of Eigen::AngleAxisd(angle, unit axis `axis` in 0..2)."""
    angle = np.asarray(angle, np.float64)
    q = np.zeros(angle.shape + (4,))
    q[..., 0] = np.cos(0.5 * angle)
    q[..., 1 + axis] = np.sin(0.5 * angle)
    return q


def from_rpy(roll, pitch, yaw):
    """fromRPY: yaw_angle * pitch_angle * roll_angle."""
    return quat_mul(quat_mul(axis_quat(yaw, 2), axis_quat(pitch, 1)), axis_quat(roll, 0))


def quat_to_matrix(q):
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = (q[..., k] for k in range(4))
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1.0 - 2.0 * (y * y + z * z)
    R[..., 0, 1] = 2.0 * (x * y - w * z)
    R[..., 0, 2] = 2.0 * (x * z + w * y)
    R[..., 1, 0] = 2.0 * (x * y + w * z)
    R[..., 1, 1] = 1.0 - 2.0 * (x * x + z * z)
    R[..., 1, 2] = 2.0 * (y * z - w * x)
    R[..., 2, 0] = 2.0 * (x * z - w * y)
    R[..., 2, 1] = 2.0 * (y * z + w * x)
    R[..., 2, 2] = 1.0 - 2.0 * (x * x + y * y)
    return R


def undistort(points, lin_vel, ang_vel_rpy, scan_duration, clockwise):
    """motion(phase) * p for every point of an (N, 3) cloud."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v, w = np.asarray(lin_vel, np.float64), np.asarray(ang_vel_rpy, np.float64)
    s = compute_phase(p[:, 0], p[:, 1], clockwise) * scan_duration
    R = quat_to_matrix(from_rpy(s * w[0], s * w[1], s * w[2]))
    return np.einsum("nij,nj->ni", R, p) + s[:, None] * v[None, :]


def matrix_to_quat(R):
    """Eigen::Quaterniond(Matrix3d): the branch on the trace, then on the largest diagonal element."""
    q = np.zeros(4)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0.0:
        t = math.sqrt(tr + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def to_rpy(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([math.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), math.asin(2 * (w * y - x * z)),
                     math.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))])


def motion_from_poses(T_start, t_start, T_finish, t_finish):
    """(linear velocity, angular velocity rpy); zeros for dt <= 0."""
    dt = t_finish - t_start
    if not dt > 0.0:
        return np.zeros(3), np.zeros(3)
    A, B = np.asarray(T_start, np.float64), np.asarray(T_finish, np.float64)
    Ainv = np.eye(4)
    Ainv[:3, :3] = A[:3, :3].T
    Ainv[:3, 3] = -A[:3, :3].T @ A[:3, 3]
    dT = Ainv @ B
    return dT[:3, 3] / (dt + 1e-6), to_rpy(matrix_to_quat(dT[:3, :3])) / (dt + 1e-6)


def rpy_pose(rpy, xyz):
    T = np.eye(4)
    T[:3, :3] = quat_to_matrix(from_rpy(*[np.float64(a) for a in rpy]))
    T[:3, 3] = xyz
    return T


# the directions whose phase is known in closed form: (x, y, wrapped azimuth as a fraction of a turn)
AXIS_AND_DIAGONAL = [((1.0, 0.0), 0.0), ((1.0, 1.0), 0.125), ((0.0, 1.0), 0.25), ((-1.0, 1.0), 0.375), ((-1.0, 0.0), 0.5),
                     ((-1.0, -1.0), 0.625), ((0.0, -1.0), 0.75), ((1.0, -1.0), 0.875)]


def special_points():
    """Points on the edges of computePhase (no subnormal coordinate): the axis and diagonal directions at several ranges and
    heights, y = +-0.0 on both sides of x = 0, the origin of the xy plane, and y = +-1e-300 on the two sides of the wrap."""
    pts = []
    for (x, y), _ in AXIS_AND_DIAGONAL:
        for r, z in ((1.0, 0.0), (37.5, -2.25), (99.0, 11.0)):
            pts.append((x * r, y * r, z))
    for x in (3.0, -3.0, 80.0, -80.0):
        pts += [(x, 0.0, 1.0), (x, -0.0, 1.0)]
    pts += [(0.0, 0.0, 5.0), (0.0, -0.0, -5.0), (-0.0, 0.0, 0.0)]
    pts += [(10.0, 1e-300, 0.5), (10.0, -1e-300, 0.5), (-10.0, 1e-300, 0.5), (-10.0, -1e-300, 0.5)]
    return np.array(pts, np.float64)


def sample_cloud(n, seed=2024):
    """n points within +-100 m (seeded); once n reaches their number, the special points lead the cloud."""
    rng = np.random.default_rng(seed + n)
    p = rng.uniform(-100.0, 100.0, (n, 3))
    sp = special_points()
    if n >= len(sp):
        p[:len(sp)] = sp
    return p
