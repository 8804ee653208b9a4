"""numpy restatement of the poses-at-any-stamp arithmetic and of the de-skew along a trajectory — the yardstick of
tests/test_trajectory_ref.py (which pins it by analysis), tests/test_gpu_trajectory_deskew.py and tests/test_gpu_mapper_trajectory.py:

  interpolate / extrapolate    open3d_slam/src/Transform.cpp:16-110
  has / lookup / get_transform open3d_slam/src/TransformInterpolationBuffer.cpp:100-149, 189-220
  deskew                       p' = A G(stamp + s) C^-1 p, A = (G(stamp) C^-1)^-1   (include/trajectory/o3s_trajectory.h)

with Eigen's Quaterniond(Matrix3d), slerp, AngleAxisd(Quaterniond) and toRotationMatrix restated from the published algorithms.
Written from the formulas, independently of the library.  Every function takes the floating type to work in (`ft`): numpy.float64
is the restatement, numpy.longdouble (80 bits on x86-64) its twin, whose distance from the restatement on a test's inputs is what
that test's tolerance is derived from."""
import numpy as np

F64 = np.float64
LD = np.longdouble


def _pi(ft):
    return ft(4) * np.arctan(ft(1))


def mat_to_quat(R, ft=F64):
    """Eigen::Quaterniond(Matrix3d): the branch on the trace, then on the largest diagonal element; (w, x, y, z), not normalised."""
    R = np.asarray(R, ft)
    q = np.zeros(4, ft)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        t = np.sqrt(tr + ft(1))
        q[0] = ft(0.5) * t
        t = ft(0.5) / t
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + ft(1))
        q[1 + i] = ft(0.5) * t
        t = ft(0.5) / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def quat_mul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx], axis=-1)


def quat_to_matrix_raw(q):
    """Quaternion::toRotationMatrix of q AS IT IS (no normalisation); (..., 4) -> (..., 3, 3)."""
    w, x, y, z = (q[..., k] for k in range(4))
    R = np.empty(q.shape[:-1] + (3, 3), q.dtype)
    R[..., 0, 0] = 1 - 2 * (y * y + z * z)
    R[..., 0, 1] = 2 * (x * y - w * z)
    R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z)
    R[..., 1, 1] = 1 - 2 * (x * x + z * z)
    R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y)
    R[..., 2, 1] = 2 * (y * z + w * x)
    R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def slerp(q0, q1, f, ft=F64):
    """Eigen's slerp, vectorised: q0, q1 (..., 4), f (...).  eps is the DOUBLE's epsilon in either type: it is a threshold of the
    algorithm, not a rounding unit."""
    q0, q1, f = np.asarray(q0, ft), np.asarray(q1, ft), np.asarray(f, ft)
    d = (q0 * q1).sum(axis=-1)
    ad = np.abs(d)
    linear = ad >= ft(1) - ft(np.finfo(np.float64).eps)
    theta = np.arccos(np.where(linear, ft(0.5), ad))      # (any angle where the branch is not taken)
    st = np.sin(theta)
    s0 = np.where(linear, 1 - f, np.sin((1 - f) * theta) / st)
    s1 = np.where(linear, f, np.sin(f * theta) / st)
    s1 = np.where(d < 0, -s1, s1)
    return s0[..., None] * q0 + s1[..., None] * q1


def angle_axis(q, ft=F64):
    """Eigen::AngleAxisd(Quaterniond): (angle, axis)."""
    n = np.sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    if n != 0:
        angle = ft(2) * np.arctan2(n, np.abs(q[0]))
        if q[0] < 0:
            n = -n
        return angle, q[1:] / n
    return ft(0), np.array([1, 0, 0], ft)


def make_pose(R, p, ft=F64):
    T = np.eye(4, dtype=ft)
    T[:3, :3] = R
    T[:3, 3] = p
    return T


def interpolate(start, end, t, ft=F64):
    """(t, pose) between two (stamp, pose) pairs; ValueError where the reference throws."""
    (t0, T0), (t1, T1) = start, end
    if t0 > t1:
        (t0, T0), (t1, T1) = (t1, T1), (t0, T0)
    if t > t1 or t < t0:
        raise ValueError("query time is not between start and end time")
    T0, T1 = np.asarray(T0, ft), np.asarray(T1, ft)
    factor = (ft(t) - ft(t0)) / ((ft(t1) - ft(t0)) + ft(1e-6))
    p = T0[:3, 3] + (T1[:3, 3] - T0[:3, 3]) * factor
    q = slerp(mat_to_quat(T0[:3, :3], ft), mat_to_quat(T1[:3, :3], ft), factor, ft)
    return t, make_pose(quat_to_matrix_raw(q), p, ft)


def extrapolate(start, end, t, ft=F64):
    (t0, T0), (t1, T1) = start, end
    if t0 > t1:
        raise ValueError("start time is greater than end time")
    duration = ft(t1) - ft(t0)
    if duration <= 0:
        raise ValueError("invalid time duration between start and end")
    T0, T1 = np.asarray(T0, ft), np.asarray(T1, ft)
    velocity = (T1[:3, 3] - T0[:3, 3]) / duration
    q0, q1 = mat_to_quat(T0[:3, :3], ft), mat_to_quat(T1[:3, :3], ft)
    q0_inv = np.array([q0[0], -q0[1], -q0[2], -q0[3]], ft) / (q0 * q0).sum()
    angle, axis = angle_axis(quat_mul(q1, q0_inv), ft)
    future = ft(t) - ft(t1)
    if future < 0:
        return t1, np.asarray(end[1])
    half = ft(0.5) * (angle * future)              # the angle is not divided by the duration
    turn = np.concatenate([[np.cos(half)], np.sin(half) * axis]).astype(ft)
    return t, make_pose(quat_to_matrix_raw(quat_mul(q1, turn)), T1[:3, 3] + velocity * future, ft)


def has(stamps, t):
    return len(stamps) > 0 and stamps[0] <= t <= stamps[-1]


def lookup(stamps, poses, t, ft=F64):
    if not has(stamps, t):
        raise ValueError("missing transform")
    if len(stamps) == 1:
        return np.asarray(poses[0])
    j = next(k for k, tk in enumerate(stamps) if t <= tk)
    if stamps[j] == t:
        return np.asarray(poses[j])
    return interpolate((stamps[j - 1], poses[j - 1]), (stamps[j], poses[j]), t, ft)[1]


def get_transform(stamps, poses, t, ft=F64):
    if t < stamps[0]:
        return np.asarray(poses[0])
    if t > stamps[-1]:
        if len(stamps) < 3:
            return np.asarray(poses[-1])        # the departure: the reference walks off its deque
        return extrapolate((stamps[-3], poses[-3]), (stamps[-1], poses[-1]), t, ft)[1]
    return lookup(stamps, poses, t, ft)


def inv_iso(T):
    R = np.eye(4, dtype=T.dtype)
    R[:3, :3] = T[:3, :3].T
    R[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return R


def compute_phase(x, y, clockwise, ft=F64):
    two_pi = 2 * _pi(ft)
    angle = np.arctan2(y, x)
    wrapped = np.where(angle < 0, angle + two_pi, angle)
    phase = 1 - wrapped / two_pi if clockwise else wrapped / two_pi
    return np.where(wrapped == 0, ft(0), phase)


def point_offsets(points, dt, scan_duration, clockwise, ft=F64):
    p = np.asarray(points, ft).reshape(-1, 3)
    return np.asarray(dt, ft) if dt is not None else compute_phase(p[:, 0], p[:, 1], clockwise, ft) * ft(scan_duration)


def deskew(points, stamps, poses, stamp, calibration=None, dt=None, scan_duration=0.1, clockwise=True, ft=F64):
    """p'_i = A G(stamp + s_i) C^-1 p_i for an (N, 3) cloud, vectorised over the points: every point takes the branch of
    get_transform its stamp asks for."""
    p = np.asarray(points, ft).reshape(-1, 3)
    K = len(stamps)
    ts = np.asarray(stamps, ft)
    Ts = np.asarray(poses, ft).reshape(K, 4, 4)
    Cinv = inv_iso(np.eye(4, dtype=ft) if calibration is None else np.asarray(calibration, ft))
    A = inv_iso(np.asarray(get_transform(stamps, poses, stamp, ft), ft) @ Cinv)
    tq = ft(stamp) + point_offsets(p, dt, scan_duration, clockwise, ft)
    quats = np.stack([mat_to_quat(Ts[k, :3, :3], ft) for k in range(K)])
    R = np.empty((len(p), 3, 3), ft)
    tr = np.empty((len(p), 3), ft)

    def take(mask, k):
        R[mask], tr[mask] = Ts[k, :3, :3], Ts[k, :3, 3]

    before, after = tq < ts[0], tq > ts[-1]
    take(before, 0)
    if after.any():
        if K < 3:
            take(after, K - 1)
        else:
            duration = ts[-1] - ts[-3]
            velocity = (Ts[-1, :3, 3] - Ts[-3, :3, 3]) / duration
            q0 = quats[-3]
            q0_inv = np.array([q0[0], -q0[1], -q0[2], -q0[3]], ft) / (q0 * q0).sum()
            angle, axis = angle_axis(quat_mul(quats[-1], q0_inv), ft)
            future = tq[after] - ts[-1]
            half = ft(0.5) * (angle * future)
            turn = np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * axis[None, :]], axis=1)
            R[after] = quat_to_matrix_raw(quat_mul(quats[-1][None, :], turn))
            tr[after] = Ts[-1, :3, 3][None, :] + velocity[None, :] * future[:, None]
    inside = ~(before | after)
    j = np.minimum(np.searchsorted(ts, tq, side="left"), K - 1)      # the first knot with tq <= its stamp
    exact = inside & (ts[j] == tq)
    for k in np.unique(j[exact]):
        take(exact & (j == k), k)
    between = inside & ~exact
    if between.any():
        j1 = j[between]
        j0 = j1 - 1
        factor = (tq[between] - ts[j0]) / ((ts[j1] - ts[j0]) + ft(1e-6))
        R[between] = quat_to_matrix_raw(slerp(quats[j0], quats[j1], factor, ft))
        tr[between] = Ts[j0, :3, 3] + (Ts[j1, :3, 3] - Ts[j0, :3, 3]) * factor[:, None]
    c = p @ Cinv[:3, :3].T + Cinv[:3, 3]
    g = np.einsum("nij,nj->ni", R, c) + tr
    return g @ A[:3, :3].T + A[:3, 3]


# ---- inputs the tests share ----

def rot(axis, angle, ft=F64):
    """Rodrigues' rotation about a unit axis."""
    a = np.asarray(axis, ft)
    a = a / np.sqrt((a * a).sum())
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], ft)
    return np.eye(3, dtype=ft) + np.sin(ft(angle)) * Kx + (1 - np.cos(ft(angle))) * (Kx @ Kx)


def random_isometry(rng, reach=100.0):
    """A rotation by any angle about any axis (rounded to a rotation matrix in float64) and a translation within +-reach metres."""
    return make_pose(rot(rng.normal(size=3), rng.uniform(-np.pi, np.pi)), rng.uniform(-reach, reach, 3))


def trajectory(K, seed, t0=10.0, period=0.0025, step_angle=1e-3, step=0.01):
    """K knots of a 400 Hz odometry source by default: each pose is the one before times a turn of step_angle about a slowly
    changing axis and a move of `step` metres; starts at a seeded random isometry.  Returns (stamps, poses)."""
    rng = np.random.default_rng(seed)
    T = random_isometry(rng)
    stamps, poses = [], []
    for k in range(K):
        stamps.append(t0 + period * k)
        poses.append(T.copy())
        T = T @ make_pose(rot([np.sin(0.1 * k), np.cos(0.1 * k), 1.0], step_angle), [step, 0.2 * step * np.sin(0.3 * k), 0.0])
    return stamps, poses
