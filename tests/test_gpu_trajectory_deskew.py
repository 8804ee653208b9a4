"""The de-skew along a trajectory (csrc/trajectory_dev.h: o3s_undistort_cloud_trajectory, o3s_raw_scan_undistort_trajectory) against the
numpy restatement tests/trajectory_ref.py, which tests/test_trajectory_ref.py pins by analysis on the CPU.

Sizes: N = 1, 63 / 64 / 65 (one wave, its two neighbours), 257 (a second block of 256 with one lane in use) and 5 010 (twenty blocks
with a partial tail); K = 1 (no launch), 2 ("the latest pose" beyond the table), 3 (the smallest table that extrapolates), 33 and 257
(six and nine steps of the binary search, an odd number of knots).  The tables are a 400 Hz source (a knot every 2.5 ms, a turn of
1e-3 rad and a centimetre from the one before, from a random isometry within +-100 m); from K = 33 on, two knots share a stamp and
the orientations are turns of 3 rad about an axis that sweeps the xy plane by 1e-3 rad per knot through its -45 degree direction,
where Eigen's matrix-to-quaternion changes the diagonal element it branches on and with it the quaternion's sign: one segment of
2e-3 rad has d < 0 (a segment that turns by radians would do too, but a turn of 1 000 rad/s multiplies the rounding of the stamps).  The calibration is a turn of 0.4 rad and a
few decimetres.  Points are undistort_ref.sample_cloud (within +-100 m; from 63 points on it starts with the points on the edges of
computePhase).  Without point times the sweep's stamp lies 0.37 ms after a knot (the special points' phases are multiples of 1/8: on
a knot they would sit on the one discontinuity of the contract, the end of a segment that the + 1e-6 never lets reach its end pose);
with point times the stamp is a knot's, and the leading times sit exactly on a knot, on the first and on the last knot, before the
earliest and after the latest.

Tolerance 2e-10 m absolute.  Derivation: on exactly these inputs the float64 restatement and an 80-bit long-double twin of it differ
by at most 1.9e-13 m (CPU), times the three orders of tests/test_gpu_undistort.py, rounded up.  The smallest defect the test must see:
leaving the 1e-6 out of the factor changes it by 1e-6 / 2.5 ms = 4e-4 of a segment's motion (1 cm and 1e-3 rad x up to 173 m), up to
7e-5 m on some point of any cloud of 63 points or more and 4e-6 m on a point near the sensor; a knot off by one moves every point by a
centimetre or more; a dropped sign flip of the slerp and A applied on the wrong side move points by metres.  The tolerance lies four
orders below the smallest of them.
Largest difference seen on the MI355X: 1.2e-13 m."""
import ctypes as C

import numpy as np
import pytest

import trajectory_ref as tr
import undistort_ref as ur
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import odometry as odo

pytestmark = pytest.mark.gpu

TOL = 2e-10
SIZES = [1, 63, 64, 65, 257, 5010]
KNOTS = [1, 2, 3, 33, 257]
T_SCAN = 0.1
CALIB = tr.make_pose(tr.rot([0.0, 0.0, 1.0], 0.4), (0.2, -0.1, 0.05))


def knots(K):
    """(stamps, poses): the 400 Hz table; from K = 33 on with two equal stamps and a segment whose quaternions point apart."""
    stamps, poses = tr.trajectory(K, seed=100 + K)
    if K >= 33:
        j = K // 2
        stamps[j + 1] = stamps[j]
        for k in range(K):                      # a turn of 3 rad about an axis that sweeps through the xy plane's -45 degree direction
            a = -np.pi / 4 + (k - (j + 4.5)) * 1e-3
            poses[k] = tr.make_pose(tr.rot([np.cos(a), np.sin(a), 0.0], 3.0), poses[k][:3, 3])
        quats = [tr.mat_to_quat(T[:3, :3]) for T in poses]
        assert (quats[j + 4] * quats[j + 5]).sum() < -0.99 and all((quats[k] * quats[k + 1]).sum() > 0.99 for k in range(K - 1) if k != j + 4)
    return stamps, poses


def case(n, K, timed):
    """(points, stamps, poses, stamp, dt or None)"""
    p = ur.sample_cloud(n)
    stamps, poses = knots(K)
    m = K // 2 + 4 if K >= 33 else 0           # the sweep starts on the segment with d < 0
    if not timed:
        return p, stamps, poses, stamps[m] + 0.00037, None
    stamp = stamps[m]
    rng = np.random.default_rng(n * 1000 + K)
    dt = rng.uniform(stamps[0] - stamp - 0.01, stamps[-1] - stamp + 0.05, n)
    lead = [stamps[min(m + 1, K - 1)] - stamp, stamps[0] - stamp, stamps[-1] - stamp, stamps[0] - stamp - 1.0, stamps[-1] - stamp + 0.05,
            stamps[K // 2] - stamp, 0.0]
    dt[:min(n, len(lead))] = lead[:n]
    for k in range(min(n, 3)):                 # the sums are exact: those stamps ARE knots
        assert stamp + dt[k] in stamps
    return p, stamps, poses, stamp, dt


_want = {}


def restated(n, K, timed, clockwise):
    """The restatement's answer, computed once per case and shared."""
    key = (n, K, timed, clockwise)
    if key not in _want:
        p, stamps, poses, stamp, dt = case(n, K, timed)
        _want[key] = tr.deskew(p, stamps, poses, stamp, CALIB, dt, T_SCAN, clockwise)
        _want[key].setflags(write=False)
    return _want[key]


def staged_points(raw, n):
    """The points of a staged sweep, read back through a pre-process that keeps every point in order."""
    from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
    everything = co.croppingVolumeFactory("MaxRadius", 1.0e6)
    ps = ProcessedScan()
    odo.preprocess_staged(ps, everything, 0.0, everything, raw)
    assert ps.n_merge == n
    return ps.merge


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("timed", [False, True])
@pytest.mark.parametrize("K", KNOTS)
@pytest.mark.parametrize("n", SIZES)
def test_device_deskew_matches_the_restatement(n, K, timed):
    clockwise = bool((n + K) % 2)
    p, stamps, poses, stamp, dt = case(n, K, timed)
    want = restated(n, K, timed, clockwise)
    table = odo.pose_table(stamps, poses)
    params = odo.make_trajectory_deskew(stamp, T_SCAN, clockwise, CALIB)
    keep = p.copy()
    got = odo.undistort_cloud_trajectory(p, table, K, params, dt)
    assert np.array_equal(bits(p), bits(keep))                     # out is another buffer: the input is untouched
    if K == 1:
        assert np.array_equal(bits(got), bits(p))                  # one pose: G is constant, nothing is launched
    err = np.abs(got - want).max()
    print(f"n={n} K={K} timed={timed}: largest difference {err:.3e} m, largest move {np.abs(want - p).max():.3e} m")
    assert err <= TOL, err
    # a second run gives the same bits; so does out aliasing pts
    assert np.array_equal(bits(odo.undistort_cloud_trajectory(p, table, K, params, dt)), bits(got))
    q = p.copy()
    assert odo.undistort_cloud_trajectory(q, table, K, params, dt, in_place=True) is q
    assert np.array_equal(bits(q), bits(got))
    # the staged in-place call gives the same bits, and leaves the normals alone
    nrm = np.random.default_rng(n).normal(size=(n, 3))
    raw = odo.RawScan()
    raw.upload(p, nrm)
    if timed:
        raw.set_point_times(dt)
    raw.undistort_trajectory(table, K, params)
    sp, sn = staged_points(raw, n)
    assert np.array_equal(bits(sp), bits(got))
    assert np.array_equal(bits(sn), bits(nrm))


@pytest.mark.parametrize("timed", [False, True])
def test_a_table_of_equal_poses_returns_the_input_through_the_kernel(timed):
    """Equal orientations: d = |q|^2 >= 1 - eps, the slerp's linear branch, which no other case here takes — so the entry must launch
    for it (only K == 1 may skip the launch).  A G C^-1 is the identity up to rounding."""
    n, K = 257, 5
    p, stamps, _, stamp, dt = case(n, K, timed)
    T = tr.random_isometry(np.random.default_rng(77))
    assert (tr.mat_to_quat(T[:3, :3]) ** 2).sum() >= 1.0 - np.finfo(np.float64).eps
    poses = [T] * K
    table = odo.pose_table(stamps, poses)
    got = odo.undistort_cloud_trajectory(p, table, K, odo.make_trajectory_deskew(stamp, T_SCAN, True, CALIB), dt)
    want = tr.deskew(p, stamps, poses, stamp, CALIB, dt, T_SCAN, True)
    assert np.isfinite(got).all()
    assert np.abs(got - p).max() <= TOL and np.abs(got - want).max() <= TOL
    assert not np.array_equal(bits(got), bits(p))          # it went through the arithmetic: a product of three poses is not the identity to the bit


def test_point_times_are_dropped_by_the_next_upload():
    n, K = 65, 33
    p, stamps, poses, stamp, dt = case(n, K, True)
    table, params = odo.pose_table(stamps, poses), odo.make_trajectory_deskew(stamp, T_SCAN, True, CALIB)
    raw = odo.RawScan()
    raw.upload(p)
    raw.set_point_times(dt)
    raw.upload(p)                                            # the same sweep again: its times are gone, the azimuth times it
    raw.undistort_trajectory(table, K, params)
    sp, _ = staged_points_without_normals(raw, n)
    assert np.abs(sp - tr.deskew(p, stamps, poses, stamp, CALIB, None, T_SCAN, True)).max() <= TOL


def staged_points_without_normals(raw, n):
    from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
    everything = co.croppingVolumeFactory("MaxRadius", 1.0e6)
    ps = ProcessedScan()
    ps.set_normal_estimation(1.0, 5)
    odo.preprocess_staged(ps, everything, 0.0, everything, raw)
    assert ps.n_merge == n
    return ps.merge


def test_refused_calls_leave_the_staged_sweep_alone():
    L = odo._L()
    n, K = 65, 33
    p, stamps, poses, stamp, dt = case(n, K, True)
    keep = p.copy()
    dp = p.ctypes.data_as(C.POINTER(C.c_double))
    ddt = dt.ctypes.data_as(C.POINTER(C.c_double))
    table = odo.pose_table(stamps, poses)
    big = odo.pose_table([10.0 + 0.001 * k for k in range(2001)], [poses[0]] * 2001)
    good = odo.make_trajectory_deskew(stamp, T_SCAN, True, CALIB)
    raw = odo.RawScan()
    raw.upload(p)
    BAD = _lib.ERR_BAD_ARGUMENT
    # point times whose number is not the staged size
    assert L.o3s_raw_scan_set_point_times(raw._h, ddt, n - 1) == BAD and L.o3s_raw_scan_set_point_times(raw._h, ddt, n + 1) == BAD
    assert L.o3s_raw_scan_set_point_times(raw._h, None, n) == BAD
    # K = 0 and K above the buffer's size limit
    for tab, k in ((table, 0), (big, 2001), (None, K)):
        assert L.o3s_raw_scan_undistort_trajectory(raw._h, tab, k, C.byref(good)) == BAD
        assert L.o3s_undistort_cloud_trajectory(0, tab, k, C.byref(good), dp, None, n, dp) == BAD
    assert L.o3s_raw_scan_undistort_trajectory(raw._h, big, 2000, C.byref(good)) == _lib.OK      # the limit itself is served ...
    raw.upload(p)                                                                                # ... (and the sweep staged afresh)
    # no point times and no scan duration
    for bad_T in (0.0, -0.1):
        bad = odo.make_trajectory_deskew(stamp, 1.0, True, CALIB)
        bad.scan_duration = bad_T
        assert L.o3s_raw_scan_undistort_trajectory(raw._h, table, K, C.byref(bad)) == BAD
        assert L.o3s_undistort_cloud_trajectory(0, table, K, C.byref(bad), dp, None, n, dp) == BAD
    assert L.o3s_raw_scan_undistort_trajectory(raw._h, table, K, None) == BAD
    assert L.o3s_undistort_cloud_trajectory(0, table, K, None, dp, None, n, dp) == BAD
    # stamps that run backwards
    back = odo.pose_table(stamps[::-1], poses)
    assert L.o3s_raw_scan_undistort_trajectory(raw._h, back, K, C.byref(good)) == BAD
    assert np.array_equal(bits(p), bits(keep))
    sp, _ = staged_points_without_normals(raw, n)
    assert np.array_equal(bits(sp), bits(keep))              # no refused call has touched the staged sweep


def test_with_point_times_the_scan_duration_is_not_read():
    n, K = 64, 3
    p, stamps, poses, stamp, dt = case(n, K, True)
    table = odo.pose_table(stamps, poses)
    a = odo.undistort_cloud_trajectory(p, table, K, odo.make_trajectory_deskew(stamp, T_SCAN, True, CALIB), dt)
    b = odo.undistort_cloud_trajectory(p, table, K, odo.make_trajectory_deskew(stamp, 0.0, False, CALIB), dt)
    assert np.array_equal(bits(a), bits(b))


def test_empty_clouds_are_served():
    stamps, poses = knots(3)
    table, params = odo.pose_table(stamps, poses), odo.make_trajectory_deskew(stamps[0], T_SCAN, True, CALIB)
    assert odo.undistort_cloud_trajectory(np.zeros((0, 3)), table, 3, params).shape == (0, 3)
    empty = odo.RawScan()
    empty.undistort_trajectory(table, 3, params)
    assert len(empty) == 0


def test_a_constant_rate_trajectory_agrees_with_the_constant_velocity_kernel():
    """A yaw-only trajectory of constant rate w_z and constant linear velocity v, two knots 1 s apart, the sweep's stamp on the
    first, the identity calibration, points timed by azimuth: G(stamp)^-1 G(stamp + s) = [Rz(f w_z) | f v] with
    f = s / (1 s + 1e-6 s), where the constant-velocity kernel (o3s_undistort_cloud) applies [Rz(s w_z) | s v].  The two differ by
    the effect of the + 1e-6 alone: s - f < 1e-6 s / 1 s, so point by point
        |difference| <= 1e-6 / 1 s x (|v| s + |w_z| s r),     r = the point's range.
    The bound is asserted of the cloud as the issue states it, with s and r the sweep's largest (the scan duration, the farthest
    point), which leaves 1e-11 m above the first-order figure; point by point it is asserted with this file's rounding allowance
    added (both kernels round at 1e-14 m at 100 m, which is more than the bound itself where s is a few microseconds).  And the
    effect is there: the largest difference is at least a tenth of the cloud's bound, so the 1e-6 is in the kernel's factor."""
    v, wz = np.array([4.0, -2.5, 0.7]), 1.3
    p = ur.sample_cloud(5010)
    stamp = 50.0
    poses = [np.eye(4), tr.make_pose(tr.rot([0.0, 0.0, 1.0], wz), v)]
    table = odo.pose_table([stamp, stamp + 1.0], poses)
    r = np.linalg.norm(p, axis=1)
    for clockwise in (False, True):
        got = odo.undistort_cloud_trajectory(p, table, 2, odo.make_trajectory_deskew(stamp, T_SCAN, clockwise))
        cv = odo.undistort_cloud(p, odo.make_motion(v, (0.0, 0.0, wz), T_SCAN, clockwise))
        s = ur.compute_phase(p[:, 0], p[:, 1], clockwise) * T_SCAN
        diff = np.linalg.norm(got - cv, axis=1)
        bound = 1e-6 / 1.0 * (np.linalg.norm(v) * s + abs(wz) * s * r)
        cloud_bound = 1e-6 / 1.0 * (np.linalg.norm(v) * T_SCAN + abs(wz) * T_SCAN * r.max())
        print(f"clockwise={clockwise}: largest difference {diff.max():.3e} m, bound {cloud_bound:.3e} m")
        assert diff.max() <= cloud_bound
        assert (diff <= bound + TOL).all(), (diff - bound).max()
        assert diff.max() >= 0.1 * cloud_bound
