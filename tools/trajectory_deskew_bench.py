"""GPU-box helper: what the de-skew along a trajectory (k_undistort_trajectory, csrc/trajectory_dev.h) costs beside the
constant-velocity de-skew (k_undistort, csrc/undistort_dev.h — the kernel of the parent commit, unchanged by this feature).

One 64 x 2048 sweep (131 072 returns in firing order: azimuth by azimuth, ranges 2 .. 60 m) staged in HBM, a table of KNOTS (40) poses
over 0.1 s of a sensor that drives at 4 m/s and turns at 1.3 rad/s, the sweep's stamp on the first knot.  Per kernel the device time
between two HIP events on the sweep's stream (the hooks build's o3s_test_deskew_kernel_ms), median of CALLS (11) calls after WARM (3),
the sweep staged afresh before every call:

  k_undistort                  the motion of the same trajectory as constant velocities
  k_undistort_trajectory       points timed by azimuth (the same computePhase), and with the driver's point times
  k_undistort_trajectory_2000  the same with a table of 2000 knots over 5 s (the buffer's size limit: 11 steps of the search)

and the host's share of one call — A, C^-1, the extrapolation, the knot quaternions, the table — as the mean of 2000 calls
(o3s_test_trajectory_prepare), for 40 and for 2000 knots.  OUT=<path> also writes the JSON there (profiles/trajectory/)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from open3d_slam_advanced_rss_2024_public_amd import _lib  # noqa: E402

CALLS = int(os.environ.get("CALLS", "11"))
WARM = int(os.environ.get("WARM", "3"))
KNOTS = int(os.environ.get("KNOTS", "40"))
BEAMS, AZIMUTHS, T_SCAN = 64, 2048, 0.1
V, WZ = (4.0, -2.5, 0.7), 1.3


def sweep():
    rng = np.random.default_rng(1)
    az = np.repeat(np.linspace(-np.pi, np.pi, AZIMUTHS, endpoint=False), BEAMS)
    el = np.tile(np.deg2rad(np.linspace(-22.5, 22.5, BEAMS)), AZIMUTHS)
    r = rng.uniform(2.0, 60.0, az.shape[0])
    return np.ascontiguousarray(np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1))


def pose_at(s):
    c, sn = np.cos(WZ * s), np.sin(WZ * s)
    T = np.eye(4)
    T[:3, :3] = [[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = np.asarray(V) * s
    return T


def main():
    with _lib.variant("hooks"):
        from open3d_slam_advanced_rss_2024_public_amd import odometry as odo
        L = odo._L()
        L.o3s_test_deskew_kernel_ms.argtypes = [C.c_void_p, C.POINTER(odo.MotionC), C.POINTER(odo.StampedPoseC), C.c_int64,
                                                C.POINTER(odo.TrajectoryDeskewC), C.POINTER(C.c_float)]
        L.o3s_test_trajectory_prepare.argtypes = [C.POINTER(odo.StampedPoseC), C.c_int64, C.POINTER(odo.TrajectoryDeskewC), C.c_int,
                                                  C.POINTER(C.c_double)]
        p = sweep()
        stamp = 100.0
        params = odo.make_trajectory_deskew(stamp, T_SCAN, True)
        phase = 1.0 - np.where(np.arctan2(p[:, 1], p[:, 0]) < 0, np.arctan2(p[:, 1], p[:, 0]) + 2 * np.pi, np.arctan2(p[:, 1], p[:, 0])) / (2 * np.pi)
        dt = np.ascontiguousarray(phase * T_SCAN)
        tables = {}
        for name, K, span in (("", KNOTS, T_SCAN), ("_2000", 2000, 5.0)):
            s = np.linspace(0.0, span, K)
            tables[name] = (odo.pose_table(list(stamp + s), [pose_at(x) for x in s]), K)
        motion = odo.make_motion(V, (0.0, 0.0, WZ), T_SCAN, True)
        raw = odo.RawScan()
        ms = C.c_float()

        def timed(call, times=None):
            out = []
            for k in range(WARM + CALLS):
                raw.upload(p)
                if times is not None:
                    raw.set_point_times(times)
                rc = call()
                assert rc == _lib.OK, rc
                if k >= WARM:
                    out.append(ms.value * 1e3)
            return {"gpu_us_median": float(np.median(out)), "gpu_us_min": float(min(out)), "gpu_us_max": float(max(out))}

        res = {"workload": f"{BEAMS} x {AZIMUTHS} sweep ({len(p)} points), {KNOTS} knots over {T_SCAN} s, median of {CALLS} calls after {WARM}"}
        res["k_undistort"] = timed(lambda: L.o3s_test_deskew_kernel_ms(raw._h, C.byref(motion), None, 0, None, C.byref(ms)))
        for name, (tab, K) in tables.items():
            call = lambda tab=tab, K=K: L.o3s_test_deskew_kernel_ms(raw._h, None, tab, K, C.byref(params), C.byref(ms))  # noqa: E731
            res["k_undistort_trajectory" + name] = timed(call)
            res["k_undistort_trajectory" + name + "_point_times"] = timed(call, dt)
            per = C.c_double()
            assert L.o3s_test_trajectory_prepare(tab, K, C.byref(params), 2000, C.byref(per)) == _lib.OK
            res["host_table_build_us" + name] = per.value * 1e3
        res["k_undistort_b"] = timed(lambda: L.o3s_test_deskew_kernel_ms(raw._h, C.byref(motion), None, 0, None, C.byref(ms)))
        base = min(res["k_undistort"]["gpu_us_median"], res["k_undistort_b"]["gpu_us_median"])
        res["k_undistort_spread_us"] = abs(res["k_undistort"]["gpu_us_median"] - res["k_undistort_b"]["gpu_us_median"])
        res["ratio_to_k_undistort"] = res["k_undistort_trajectory"]["gpu_us_median"] / base
        res["ratio_to_k_undistort_point_times"] = res["k_undistort_trajectory_point_times"]["gpu_us_median"] / base
        res["ratio_to_k_undistort_2000"] = res["k_undistort_trajectory_2000"]["gpu_us_median"] / base
    line = json.dumps(res)
    print(line)
    out = os.environ.get("OUT")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
