"""GPU-box helper: LiDAR-only odometry with the parameters of the reference's param/tutorial_1_LO.lua (odometry voxel 0.05 m, crop
2 .. 40 m, normals knn 10 / 1.0 m, GeneralizedIcp, 30 iterations, max correspondence distance 1.0 m; motion compensation: scan
duration 0.1 s, clockwise, 3 poses) on 64 x 2048-ray sweeps of a sensor that MOVES while it sweeps
(synthetic.make_moving_lidar_scan: constant sensor-frame velocities, one sweep per scan duration).

Per sweep, wall time around the blocking calls, median over the sweeps after the first WARM: staging (o3s_raw_scan_upload), de-skew
(o3s_raw_scan_undistort), pre-process (o3s_scan_preprocess_staged, normals estimated) and registration (o3s_scan_registration_icp).
Drift: the odometry's cumulative pose against ground truth, with the compensation and without it, at the end of the drive and as the
mean error of a step — over all steps, and over the steps after the compensation has started (it needs num_poses + 1 poses; the
step into the first de-skewed sweep pairs it with a skewed one).  Last, on one sweep: the staged pre-process alone — the path as it was before the de-skew existed — against
the de-skew followed by the staged pre-process, median of REPS.

SWEEPS (default 16), WARM (2), REPS (11), V="vx,vy,vz" m/s (default 3,0,0), W="wx,wy,wz" rad/s (default 0,0,0.4);
OUT=<path> also writes the JSON line there (profiles/undistort/)."""
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan, odometry as odo, synthetic as syn  # noqa: E402

SWEEPS = int(os.environ.get("SWEEPS", "16"))
WARM = int(os.environ.get("WARM", "2"))
REPS = int(os.environ.get("REPS", "11"))
V = tuple(float(x) for x in os.environ.get("V", "3,0,0").split(","))
W = tuple(float(x) for x in os.environ.get("W", "0,0,0.4").split(","))
SCAN_DURATION, CLOCKWISE, NUM_POSES = 0.1, True, 3


def clock(fn):
    gc.disable()
    t0 = time.perf_counter()
    r = fn()
    dt = (time.perf_counter() - t0) * 1e3
    gc.enable()
    return r, dt


def drive():
    """Ground-truth poses at the START of every sweep (constant twist: T_k+1 = T_k . motion(scan duration)) and the sweeps."""
    world = syn.make_world(20000.0, seed=7)
    T = syn.corridor_pose(world, 0)
    Rm, tm = syn.sweep_motion([SCAN_DURATION], V, W)
    step = syn.make_T(Rm[0], tm[0])
    poses, sweeps = [], []
    for k in range(SWEEPS):
        poses.append(T.copy())
        p, _ = syn.make_moving_lidar_scan(world, T, V, W, SCAN_DURATION, CLOCKWISE, seed=100 + k)
        sweeps.append(np.ascontiguousarray(p, np.float64))
        T = T @ step
    return poses, sweeps


def run(sweeps, compensate):
    o = odo.LidarOdometry(odo.OdometryParams())
    mc = odo.ConstantVelocityMotionCompensation(o.buffer, SCAN_DURATION, CLOCKWISE, NUM_POSES)
    raw = odo.RawScan()
    rows, cum, accepted, iters = [], [], [], []
    for k, p in enumerate(sweeps):
        stamp = SCAN_DURATION * k
        _, up = clock(lambda: raw.upload(p))
        dsk = 0.0
        if compensate:
            _, dsk = clock(lambda: mc.undistort(raw, stamp))
        ok, _ = clock(lambda: o.add_range_scan(None, None, stamp, raw=raw))
        accepted.append(bool(ok))
        cum.append(o.cumulative.copy())
        iters.append(o.last_result.iterations if o.last_result is not None else 0)
        rows.append((up, dsk, o.last_timings["preprocess_ms"], o.last_timings["registration_ms"]))
    return np.array(rows), cum, accepted, o, iters


def drift(poses, cum):
    gt = [np.linalg.inv(poses[0]) @ T for T in poses]
    end = float(np.linalg.norm(gt[-1][:3, 3] - cum[-1][:3, 3]))
    steps = []
    for k in range(1, len(cum)):
        a = np.linalg.inv(gt[k - 1]) @ gt[k]
        b = np.linalg.inv(cum[k - 1]) @ cum[k]
        steps.append(float(np.linalg.norm(a[:3, 3] - b[:3, 3])))
    # the compensation starts at sweep NUM_POSES + 1; the step into that sweep pairs a skewed cloud with a de-skewed one
    steady = steps[NUM_POSES + 1:]
    return end, float(np.mean(steps)), float(np.linalg.norm(gt[-1][:3, 3])), float(np.mean(steady)) if steady else None


def staged_preprocess_ab(sweep):
    """The staged pre-process of one sweep without and with a de-skew in front (fresh upload each time, not timed)."""
    prm = odo.OdometryParams()
    raw, scan = odo.RawScan(), ProcessedScan()
    scan.set_normal_estimation(prm.max_distance_knn, prm.knn)
    m = odo.make_motion(V, W, SCAN_DURATION, CLOCKWISE)
    plain, with_deskew, deskew_only = [], [], []
    for rep in range(WARM + REPS):
        raw.upload(sweep)
        _, a = clock(lambda: odo.preprocess_staged(scan, prm.cropper, prm.voxel_size, prm.cropper, raw))
        raw.upload(sweep)
        _, d = clock(lambda: raw.undistort(m))
        _, b = clock(lambda: odo.preprocess_staged(scan, prm.cropper, prm.voxel_size, prm.cropper, raw))
        if rep >= WARM:
            plain.append(a)
            deskew_only.append(d)
            with_deskew.append(d + b)
    return {"staged_preprocess_median_ms": float(np.median(plain)), "deskew_median_ms": float(np.median(deskew_only)),
            "deskew_then_staged_preprocess_median_ms": float(np.median(with_deskew))}


def main():
    poses, sweeps = drive()
    out = {"sweeps": SWEEPS, "returns_per_sweep": int(np.median([len(s) for s in sweeps])), "linear_velocity": V, "angular_velocity_rpy": W,
           "scan_duration": SCAN_DURATION}
    for name, comp in (("compensated", True), ("uncompensated", False)):
        rows, cum, accepted, o, iters = run(sweeps, comp)
        med = np.median(rows[WARM:], axis=0)
        end, step, length, steady = drift(poses, cum)
        out[name] = {"upload_median_ms": float(med[0]), "deskew_median_ms": float(med[1]), "preprocess_median_ms": float(med[2]),
                     "registration_median_ms": float(med[3]), "per_sweep_median_ms": float(np.median(rows[WARM:].sum(axis=1))),
                     "accepted": int(sum(accepted)), "merge_points": int(o.prev.n_merge), "end_drift_m": end, "mean_step_error_m": step,
                     "mean_step_error_after_sweep_%d_m" % (NUM_POSES + 1): steady, "path_length_m": length,
                     "registration_iterations_median": float(np.median(iters[WARM:]))}
    out["staged_preprocess"] = staged_preprocess_ab(sweeps[min(4, SWEEPS - 1)])
    line = json.dumps(out)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
