"""The odometry prior at any stamp (Mapper.interpolate_odometry, the mirror of MapperParams::isInterpolateOdometry; Mapper.cpp:
219-224, 237-261, 268-280) on the CPU, with the stand-ins of tests/test_mapper_logic.py: an "ICP" that shifts the prior by 0.25
along x, submaps that only count.  The odometry is a 100 Hz source whose stamps miss the 10 Hz scan stamps by 3 ms — what every
external source does — on a trajectory that turns and climbs; expectations come from the restatement tests/trajectory_ref.py
(pinned by analysis in tests/test_trajectory_ref.py) within that file's TOL, or are exact where the arithmetic is the same."""
import numpy as np
import pytest

import trajectory_ref as tr
from test_mapper_logic import PTS, make
from test_trajectory_ref import TOL

CALIB = tr.make_pose(tr.rot([0.0, 0.0, 1.0], 0.4), (0.2, -0.1, 0.05))


def odometry(n=80, t0=-0.003, period=0.01):
    """Stamps -0.003, 0.007, ...: 3 ms before every scan stamp 0.1 k, never on one."""
    return tr.trajectory(n, seed=21, t0=t0, period=period, step_angle=4e-3, step=0.02)


def feed(m, stamps, poses, upto):
    """The odometry poses with a stamp <= upto that the mapper has not been given yet."""
    fed = getattr(m, "_fed", 0)
    while fed < len(stamps) and stamps[fed] <= upto:
        m.add_odometry_pose(stamps[fed], poses[fed])
        fed += 1
    m._fed = fed


def expected_prior(T_prev, stamps, poses, fed, last, stamp, calib):
    Cinv = np.linalg.inv(calib)
    a = tr.get_transform(stamps[:fed], poses[:fed], last) @ Cinv
    b = tr.get_transform(stamps[:fed], poses[:fed], stamp) @ Cinv
    return T_prev @ np.linalg.inv(a) @ b


def test_off_is_the_default_and_a_missed_stamp_leaves_the_previous_pose_as_the_prior():
    stamps, poses = odometry()
    m = make(calibration=CALIB)
    assert m.interpolate_odometry is False
    for k in range(5):
        feed(m, stamps, poses, 0.1 * k + 0.02)
        T_before = m.T.copy()
        assert m.add(PTS, PTS, 0.1 * k)
        if k:
            assert np.array_equal(m.prior, T_before), k          # no pose carries the scan's stamp: no odometry motion


def test_on_the_prior_is_the_previous_pose_times_the_interpolated_odometry_motion():
    stamps, poses = odometry()
    m = make(calibration=CALIB)
    m.interpolate_odometry = True
    moved = 0.0
    for k in range(6):
        stamp = 0.1 * k
        feed(m, stamps, poses, stamp + 0.02)      # the source runs ahead of the scans: every scan stamp is inside the buffer
        T_prev, last = m.T_prev.copy(), m.last_stamp
        assert m.add(PTS, PTS, stamp)
        if k == 1:
            assert np.array_equal(m.prior, T_prev)               # lastMeasurementTimestamp_ is unset after the first scan
        if k >= 2:
            want = expected_prior(T_prev, stamps, poses, m._fed, last, stamp, CALIB)
            assert np.abs(m.prior - want).max() <= TOL, k
            moved = max(moved, np.abs(m.prior - T_prev).max())
    assert moved > 0.05                                           # the motion is there: ten odometry steps of 2 cm per scan


def test_a_scan_beyond_the_odometry_is_extrapolated_for_100_ms_and_no_longer():
    stamps, poses = odometry(n=30)                # the source stops at 0.287
    for beyond, expect_motion in ((0.05, True), (0.15, False)):
        m = make(calibration=CALIB)
        m.interpolate_odometry = True
        feed(m, stamps, poses, 10.0)
        for k in range(3):
            assert m.add(PTS, PTS, 0.1 * k)
        stamp = stamps[-1] + beyond
        T_prev = m.T_prev.copy()
        assert not m.odom_buffer.has(stamp)
        assert m.add(PTS, PTS, stamp)
        if expect_motion:      # isOdomOkay by "less than 100 ms after the latest pose": getTransform extrapolates from the third pose from the end
            want = expected_prior(T_prev, stamps, poses, len(stamps), 0.2, stamp, CALIB)
            ext = tr.extrapolate((stamps[-3], poses[-3]), (stamps[-1], poses[-1]), stamp)[1]
            assert np.array_equal(tr.get_transform(stamps, poses, stamp), ext)
            assert np.abs(m.prior - want).max() <= TOL and np.abs(m.prior - T_prev).max() > 0.05
        else:
            assert np.array_equal(m.prior, T_prev)


def test_the_out_of_order_branch_no_longer_throws():
    stamps, poses = odometry()
    off, on = make(calibration=CALIB), make(calibration=CALIB)
    on.interpolate_odometry = True
    for m in (off, on):
        feed(m, stamps, poses, 0.35)
        for k in range(3):
            assert m.add(PTS, PTS, 0.1 * k)
    with pytest.raises(KeyError):
        off.add(PTS, PTS, 0.15)                   # today: no odometry pose carries the last scan's stamp
    T_prev, calls = on.T_prev.copy(), len(on.icp.calls)
    assert on.add(PTS, PTS, 0.15)                 # Mapper.cpp:197-235: propagated by the motion from the last scan to the latest odometry pose
    latest = stamps[on._fed - 1]
    want = expected_prior(T_prev, stamps, poses, on._fed, 0.2, latest, CALIB)
    assert len(on.icp.calls) == calls and np.abs(on.T - want).max() <= TOL
    assert on.pose_buffer.latest_time() == latest and np.array_equal(on.T_prev, on.T)


def test_on_and_off_give_the_same_priors_bit_for_bit_when_the_odometry_carries_the_scan_stamps():
    stamps, poses = tr.trajectory(12, seed=22, t0=0.0, period=0.1, step_angle=0.03, step=0.2)
    off, on = make(calibration=CALIB), make(calibration=CALIB)
    on.interpolate_odometry = True
    for m in (off, on):
        for t, T in zip(stamps, poses):           # all of it first: every scan stamp lies inside the buffer's range
            m.add_odometry_pose(t, T)
    for k in range(10):
        assert off.add(PTS, PTS, stamps[k]) and on.add(PTS, PTS, stamps[k])
        assert np.array_equal(off.prior.view(np.uint64), on.prior.view(np.uint64)), k
        assert np.array_equal(off.T.view(np.uint64), on.T.view(np.uint64)), k
    assert np.abs(on.prior - on.T_prev).max() > 0.1


def test_poses_of_the_map_at_any_stamp():
    """Mapper::getMapToRangeSensor / getMapToOdom (Mapper.cpp:106-115) over the registered poses and the odometry."""
    stamps, poses = odometry()
    m = make(calibration=CALIB)
    m.interpolate_odometry = True
    for k in range(5):
        feed(m, stamps, poses, 0.1 * k + 0.02)
        assert m.add(PTS, PTS, 0.1 * k)
    bt, bT = m.pose_buffer._t, m.pose_buffer._T
    assert np.array_equal(m.getMapToRangeSensor(0.2), bT[2])
    want = tr.get_transform(bt, bT, 0.234)
    assert np.abs(m.getMapToRangeSensor(0.234) - want).max() <= TOL
    want = want @ np.linalg.inv(tr.get_transform(stamps[:m._fed], poses[:m._fed], 0.234))
    assert np.abs(m.getMapToOdom(0.234) - want).max() <= TOL
