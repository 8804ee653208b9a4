"""CPU only.  Pins tests/undistort_ref.py — the numpy restatement the device de-skew is measured against — by analysis, checks the
library's host-only velocity estimate (o3s_motion_from_poses) against it, and the TransformBuffer of odometry.py against the
rules of TransformInterpolationBuffer.cpp."""
import ctypes as C
import math

import numpy as np
import pytest

import undistort_ref as ur
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import odometry as odo
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn

V, W, T = (4.0, -2.5, 0.7), (0.9, -0.6, 1.3), 0.1


@pytest.mark.parametrize("clockwise", [False, True])
def test_phase_of_the_axis_and_diagonal_directions(clockwise):
    for (x, y), turn in ur.AXIS_AND_DIAGONAL:
        for r in (1.0, 0.25, 64.0):
            want = 0.0 if turn == 0.0 else (1.0 - turn if clockwise else turn)
            assert abs(float(ur.compute_phase(x * r, y * r, clockwise)) - want) < 1e-15, (x, y, r)


@pytest.mark.parametrize("clockwise", [False, True])
def test_phase_at_signed_zeros_the_origin_and_the_wrap(clockwise):
    ph = lambda x, y: float(ur.compute_phase(x, y, clockwise))
    # y = +-0.0 ahead of the sensor: the wrapped angle is 0 -> phase 0 in both spin senses
    assert ph(3.0, 0.0) == 0.0 and ph(3.0, -0.0) == 0.0
    # y = +-0.0 behind it: atan2 gives +pi / -pi, both wrap to pi -> half a turn
    assert ph(-3.0, 0.0) == 0.5 and ph(-3.0, -0.0) == 0.5
    # x = y = 0: atan2(+-0, +0) = +-0 -> phase 0
    assert ph(0.0, 0.0) == 0.0 and ph(0.0, -0.0) == 0.0
    # y = +-1e-300 ahead of the sensor: the two sides of the wrap — just after the start of a turn, and its very end
    lo, hi = ph(10.0, 1e-300), ph(10.0, -1e-300)
    if clockwise:
        assert lo == 1.0 and hi == 0.0
    else:
        assert 0.0 < lo < 1e-300 and hi == 1.0
    assert ph(-10.0, 1e-300) == 0.5 and ph(-10.0, -1e-300) == 0.5


@pytest.mark.parametrize("clockwise", [False, True])
def test_a_pure_yaw_rate_is_a_planar_rotation(clockwise):
    p = ur.sample_cloud(257)
    wz = 1.3
    out = ur.undistort(p, (0, 0, 0), (0, 0, wz), T, clockwise)
    a = ur.compute_phase(p[:, 0], p[:, 1], clockwise) * T * wz
    want = np.c_[np.cos(a) * p[:, 0] - np.sin(a) * p[:, 1], np.sin(a) * p[:, 0] + np.cos(a) * p[:, 1], p[:, 2]]
    assert np.abs(out - want).max() < 1e-12


def test_zero_velocity_is_the_identity_and_the_rotation_order_matters():
    p = ur.sample_cloud(257)
    assert np.array_equal(ur.undistort(p, (0, 0, 0), (0, 0, 0), T, True), p)
    # the order yaw * pitch * roll is visible at the velocities the device test uses: roll * pitch * yaw moves the median point by
    # centimetres, ten orders above the device tolerance
    s = ur.compute_phase(p[:, 0], p[:, 1], True) * T
    q_swapped = ur.quat_mul(ur.quat_mul(ur.axis_quat(s * W[0], 0), ur.axis_quat(s * W[1], 1)), ur.axis_quat(s * W[2], 2))
    swapped = np.einsum("nij,nj->ni", ur.quat_to_matrix(q_swapped), p) + s[:, None] * np.array(V)
    assert np.median(np.linalg.norm(swapped - ur.undistort(p, V, W, T, True), axis=1)) > 0.01


def box_world(L=30.0, W_=20.0, H=6.0):
    """The inside of a box: floor, ceiling and four walls."""
    c = [(0, 0, 0), (0, 0, H), (L / 2, 0, H / 2), (-L / 2, 0, H / 2), (0, W_ / 2, H / 2), (0, -W_ / 2, H / 2)]
    u = [(L / 2, 0, 0), (L / 2, 0, 0), (0, W_ / 2, 0), (0, W_ / 2, 0), (L / 2, 0, 0), (L / 2, 0, 0)]
    v = [(0, W_ / 2, 0), (0, W_ / 2, 0), (0, 0, H / 2), (0, 0, H / 2), (0, 0, H / 2), (0, 0, H / 2)]
    n = [(0, 0, 1), (0, 0, -1), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0)]
    c, u, v, n = (np.asarray(a, np.float64) for a in (c, u, v, n))
    return syn.World(c, u, v, n, 4.0 * np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1), (L, W_, H))


def face_distance(world, p):
    """Distance of each point to the nearest face plane of the box."""
    return np.abs(np.einsum("nfk,fk->nf", p[:, None, :] - world.centres[None, :, :], world.normals)).min(axis=1)


@pytest.mark.parametrize("clockwise", [False, True])
def test_deskewing_a_moving_sweep_with_the_true_velocities_restores_the_box(clockwise):
    world = box_world()
    T_start = syn.make_T(syn.rot_axis_angle([0.1, -0.2, 1.0], 0.4), np.array([2.0, -1.5, 2.5]))
    ps, _ = syn.make_moving_lidar_scan(world, T_start, V, W, T, clockwise, beams=16, azimuths=256, sigma=0.0, dtype=np.float64)
    assert len(ps) == 16 * 256          # every ray hits the inside of a closed box
    to_world = lambda p: p @ T_start[:3, :3].T + T_start[:3, 3]
    skewed = face_distance(world, to_world(ps))
    fixed = face_distance(world, to_world(ur.undistort(ps, V, W, T, clockwise)))
    assert fixed.max() < 1e-9, fixed.max()
    assert np.median(skewed) > 0.01 and skewed.max() > 0.05, (np.median(skewed), skewed.max())
    # a sensor at rest: make_moving_lidar_scan is make_lidar_scan
    a, an = syn.make_moving_lidar_scan(world, T_start, (0, 0, 0), (0, 0, 0), T, clockwise, beams=8, azimuths=64, sigma=0.01, seed=3)
    b, bn = syn.make_lidar_scan(world, T_start, beams=8, azimuths=64, sigma=0.01, seed=3)
    assert np.allclose(a, b, atol=1e-5) and np.allclose(an, bn, atol=1e-6)


def seeded_poses(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        rpy = (rng.uniform(-math.pi, math.pi), rng.uniform(-math.pi / 3, math.pi / 3), rng.uniform(-math.pi, math.pi))   # |pitch| <= 60 deg
        out.append(ur.rpy_pose(rpy, rng.uniform(-5.0, 5.0, 3)))
    return out


def test_motion_from_poses_against_the_restatement():
    """toRPY is quadratic in q (q and -q give the same angles), so which branch of the matrix-to-quaternion conversion ran cannot
    matter; the relative pose start^-1 * finish of two seeded poses has |pitch| < 90 deg with room, away from asin's edge."""
    poses = seeded_poses(41, 7)
    rng = np.random.default_rng(8)
    for A, B in zip(poses[:-1], poses[1:]):
        small = ur.rpy_pose(rng.uniform(-0.5, 0.5, 3), rng.uniform(-1.0, 1.0, 3))    # the pitch of A^-1 B must itself stay within 60 deg
        for F in (A @ small, A @ ur.rpy_pose((rng.uniform(-3, 3), rng.uniform(-1.0, 1.0), rng.uniform(-3, 3)), rng.uniform(-2, 2, 3))):
            t0 = rng.uniform(0.0, 100.0)
            t1 = t0 + rng.uniform(0.05, 0.5)
            v, w = odo.motion_from_poses(A, t0, F, t1)
            rv, rw = ur.motion_from_poses(A, t0, F, t1)
            assert np.abs(v - rv).max() < 1e-12 and np.abs(w - rw).max() < 1e-12, (v - rv, w - rw)
    # dt <= 0: zeros; only the two velocity arrays are written
    for t1 in (5.0, 4.9):
        v, w = odo.motion_from_poses(poses[0], 5.0, poses[1], t1)
        assert not v.any() and not w.any()
    m = odo.make_motion((9, 9, 9), (9, 9, 9), 0.25, False)
    m.reserved[1] = 77
    L = odo._L()
    P = lambda T_: np.ascontiguousarray(T_.T).reshape(16).ctypes.data_as(C.POINTER(C.c_double))
    assert L.o3s_motion_from_poses(P(poses[0]), 1.0, P(poses[1]), 1.5, C.byref(m)) == _lib.OK
    assert m.scan_duration == 0.25 and m.is_spinning_clockwise == 0 and m.reserved[1] == 77 and m.linear_velocity[0] != 9
    assert L.o3s_motion_from_poses(None, 1.0, P(poses[1]), 1.5, C.byref(m)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_motion_from_poses(P(poses[0]), 1.0, P(poses[1]), 1.5, None) == _lib.ERR_BAD_ARGUMENT


def test_a_known_motion_is_recovered():
    """A pose that moved with constant sensor-frame velocities for dt seconds: the estimate is motion / (dt + 1e-6)."""
    A = ur.rpy_pose((0.3, -0.2, 1.1), (4.0, 5.0, 6.0))
    rpy, xyz, dt = np.array([0.02, -0.03, 0.05]), np.array([0.4, -0.1, 0.02]), 0.1
    v, w = odo.motion_from_poses(A, 10.0, A @ ur.rpy_pose(rpy, xyz), 10.0 + dt)
    assert np.abs(v - xyz / (dt + 1e-6)).max() < 1e-11 and np.abs(w - rpy / (dt + 1e-6)).max() < 1e-11


def test_deskew_entries_refuse_bad_arguments_before_any_device_call():
    """scan_duration <= 0 and NULL arguments are O3S_ERR_BAD_ARGUMENT on a machine with or without a GPU; N == 0 is O3S_OK."""
    L = odo._L()
    p = np.ones((4, 3))
    dp = p.ctypes.data_as(C.POINTER(C.c_double))
    good = odo.make_motion(V, W, T, True)
    for bad_T in (0.0, -0.1, float("nan")):
        bad = odo.make_motion(V, W, 1.0, True)
        bad.scan_duration = bad_T
        assert L.o3s_undistort_cloud(0, C.byref(bad), dp, 4, dp) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_undistort_cloud(0, None, dp, 4, dp) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_undistort_cloud(0, C.byref(good), None, 4, dp) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_undistort_cloud(0, C.byref(good), dp, 4, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_undistort_cloud(0, C.byref(good), dp, -1, dp) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_undistort_cloud(0, C.byref(good), None, 0, None) == _lib.OK
    assert L.o3s_raw_scan_undistort(None, C.byref(good)) == _lib.ERR_BAD_ARGUMENT
    # zero velocities: the result is p, without a device
    zero = odo.make_motion(scan_duration=T)
    out = np.zeros_like(p)
    assert L.o3s_undistort_cloud(0, C.byref(zero), dp, 4, out.ctypes.data_as(C.POINTER(C.c_double))) == _lib.OK and np.array_equal(out, p)
    assert L.o3s_scan_registration_icp(None, 0, None, 0, 1.0, None, None, None, None) == _lib.ERR_BAD_ARGUMENT
    with pytest.raises(ValueError):
        odo.LidarOdometry(odo.OdometryParams(downsampling_ratio=0.5))


def test_transform_buffer_push_rules_size_limit_and_accessors():
    b = odo.TransformBuffer(4)
    pose = lambda k: syn.make_T(None, np.array([float(k), 0.0, 0.0]))
    assert b.empty() and b.size() == 0 and not b.has(0.0)
    with pytest.raises(RuntimeError):
        b.latest_time()
    for k in (2, 3, 5):
        b.push(float(k), pose(k))
    b.push(1.0, pose(1))       # earlier than the earliest: ignored
    b.push(4.0, pose(4))       # earlier than the latest: ignored
    assert b.size() == 3 and b.latest_time() == 5.0 and b.earliest_time() == 2.0
    b.push(5.0, pose(50))      # the latest stamp again is NOT earlier than the latest: kept
    assert b.size() == 4 and b.latest_measurement()[1][0, 3] == 50.0
    assert b.lookup(5.0)[0, 3] == 5.0          # the first of two equal stamps
    b.push(6.0, pose(6))       # over the limit: the oldest goes
    assert b.size() == 4 and b.earliest_time() == 3.0 and not b.has(2.0) and b.has(3.0) and b.has(4.5) and not b.has(6.5)
    assert b.latest_offseted_measurement(0)[0] == 6.0 and b.latest_offseted_measurement(1)[1][0, 3] == 50.0
    assert b.latest_offseted_measurement(3)[0] == 3.0
    with pytest.raises(IndexError):
        b.latest_offseted_measurement(4)
    with pytest.raises(RuntimeError):
        b.lookup(4.5)          # no interpolation here
    assert odo.TransformBuffer().size_limit == 2000
    # the pose is copied at the push
    T_ = pose(7)
    b.push(7.0, T_)
    T_[0, 3] = -1.0
    assert b.lookup(7.0)[0, 3] == 7.0


def test_motion_compensation_is_zero_until_the_buffer_is_long_enough():
    b = odo.TransformBuffer()
    mc = odo.ConstantVelocityMotionCompensation(b, T, True, 3)
    poses = [ur.rpy_pose((0.0, 0.0, 0.02 * k), (0.25 * k, 0.01 * k * k, 0.0)) for k in range(6)]
    zero = lambda m: not any(m.linear_velocity[:]) and not any(m.angular_velocity_rpy[:])
    for k in range(6):
        m = mc.motion(0.1 * k)
        if k <= 3:              # size <= num_poses
            assert zero(m), k
        else:
            rv, rw = ur.motion_from_poses(poses[k - 4], 0.1 * (k - 4), poses[k - 1], 0.1 * (k - 1))
            assert np.abs(np.array(m.linear_velocity[:]) - rv).max() < 1e-12 and np.abs(np.array(m.angular_velocity_rpy[:]) - rw).max() < 1e-12
            assert abs(rv[0] - 2.5) < 0.05
        assert m.scan_duration == T and m.is_spinning_clockwise == 1
        b.push(0.1 * k, poses[k])
    assert zero(mc.motion(0.5)) and zero(mc.motion(0.4))     # the buffer's latest time is not earlier than the stamp
    with pytest.raises(ValueError):
        odo.ConstantVelocityMotionCompensation(b, 0.0)
