"""GPU-box helper: what RANSAC plane segmentation costs (include/plane_segmentation/o3s_plane_segmentation.h), written as one JSON
line to OUT (default profiles/plane_segmentation/plane_segmentation_bench.json).

  scan       the merge cloud of a 64 x 2048 sweep (voxel 0.1), resident: ProcessedScan.removePlanes (filtered and the match cloud
             re-cropped); the sweep is pre-processed again before every timed call (the removal works in place), outside the timed
             window
  submap     a 0.4 M-point resident submap (voxel 0.1): Submap.segmentPlanes (labels to the host) and Submap.removePlanes (in
             place); the map is uploaded again before every timed removal, outside the timed window
  replaced   the route the calls replace: download the map, the numpy restatement of the same algorithm (tests/plane_ref.py: every
             hypothesis of a block scored over the whole cloud in vectorised numpy), upload what is left; the host part also given on
             its own

each at num_iterations 100 and 1000, for one plane and for a peel of 4.  distance_threshold 0.1 m, ransac_n 3, confidence 1,
min_inliers 1000.  Medians of REPS (default 11) wall-clock calls after WARMUP (default 2), min - max beside them; the replaced route
HOST_REPS (default 3) calls after one, and a single call at 1000 iterations.  Same process, same clouds for all of it.
KERNELS_ONLY=1 runs the device calls alone, twice each (for `rocprofv3 --kernel-trace --stats`); CASES=1000x1,100x4 picks the
(num_iterations x max_planes) cases; HOST=0 leaves the replaced route out."""
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan, Submap  # noqa: E402
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co, synthetic as syn  # noqa: E402

REPS = int(os.environ.get("REPS", "11"))
WARMUP = int(os.environ.get("WARMUP", "2"))
HOST_REPS = int(os.environ.get("HOST_REPS", "3"))
SUBMAP = int(os.environ.get("SUBMAP", "400000"))
KERNELS_ONLY = os.environ.get("KERNELS_ONLY") == "1"
HOST = os.environ.get("HOST", "1") == "1"
OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "plane_segmentation", "plane_segmentation_bench.json")
MAP_VOXEL = 0.1
THR, RANSAC_N, MIN_INLIERS, SEED = 0.1, 3, 1000, 1
GRID = [(100, 1), (100, 4), (1000, 1), (1000, 4)]   # (num_iterations, max_planes)
if os.environ.get("CASES"):                        # e.g. CASES=1000x1,100x4
    GRID = [tuple(int(v) for v in c.split("x")) for c in os.environ["CASES"].split(",")]


def params(iters, planes):
    return co.plane_params(THR, RANSAC_N, iters, 1.0, SEED, planes, MIN_INLIERS)


def stats(us):
    v = np.asarray(us, np.float64) / 1e3
    return {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max())}


def timed(prepare, fn, reps, warmup=WARMUP):
    out, us = None, []
    for k in range(reps + warmup):
        prepare()
        gc.disable()
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e6
        gc.enable()
        if k >= warmup:
            us.append(dt)
    return us, out


def main():
    world = syn.make_world(1.25 * SUBMAP * MAP_VOXEL * MAP_VOXEL, seed=1234)
    mp, mn = syn.make_map(world, SUBMAP, MAP_VOXEL, seed=1234)
    mp, mn = np.asarray(mp, np.float64), np.asarray(mn, np.float64)
    big = co.croppingVolumeFactory("MaxRadius", 1000.0)
    narrow = co.croppingVolumeFactory("MaxRadius", 30.0)
    T_gt = syn.make_T(syn.rot_rpy_deg(0.0, 0.0, 37.0), np.array([6.5, -5.5, 1.5]))
    sweep, sweep_n = syn.make_lidar_scan(world, T_gt)
    sweep, sweep_n = np.asarray(sweep, np.float64), np.asarray(sweep_n, np.float64)
    sc = ProcessedScan()
    sm = Submap(0.0, big)
    if KERNELS_ONLY:
        for iters, planes in GRID:
            q = params(iters, planes)
            for _ in range(2):
                sc.preprocess(big, 0.1, narrow, sweep, sweep_n)
                sc.removePlanes(narrow, q)
                sm.setMapPointCloud(mp, mn)
                sm.segmentPlanes(q)
                sm.removePlanes(q)
        return
    res = {"workload": f"medians of {REPS} wall-clock calls after {WARMUP} warm-ups", "map_points": int(len(mp)), "sweep_points": int(len(sweep)),
           "distance_threshold": THR, "ransac_n": RANSAC_N, "min_inliers": MIN_INLIERS, "cases": {}}
    co.plane_reserve(max(len(mp), len(sweep)), 1000)
    for iters, planes in GRID:
        q = params(iters, planes)
        case = {}
        us, (n_merge, n_match, models) = timed(lambda: sc.preprocess(big, 0.1, narrow, sweep, sweep_n), lambda: sc.removePlanes(narrow, q), REPS)
        before = sc.preprocess(big, 0.1, narrow, sweep, sweep_n)
        case["scan_remove"] = dict(stats(us), merge_before=int(before[0]), merge_after=int(n_merge), match_after=int(n_match), n_planes=int(len(models)))
        sm.setMapPointCloud(mp, mn)
        us, (lab_dev, models_dev, counts_dev) = timed(lambda: None, lambda: sm.segmentPlanes(q), REPS)
        case["submap_segment"] = dict(stats(us), n_planes=int(len(counts_dev)), counts=[int(c) for c in counts_dev])
        us, (removed, _) = timed(lambda: sm.setMapPointCloud(mp, mn), lambda: sm.removePlanes(q), REPS)
        case["submap_remove"] = dict(stats(us), removed=int(removed))
        if HOST:
            import plane_ref as pr

            host_only = []

            def replaced():
                p, n = sm.getMapPointCloud()
                t0 = time.perf_counter()
                lab, models, counts = pr.segment_planes(p, THR, planes, MIN_INLIERS, RANSAC_N, iters, 1.0, SEED)
                keep = lab < 0
                host_only.append((time.perf_counter() - t0) * 1e6)
                sm.setMapPointCloud(p[keep], n[keep])
                return lab, models

            reps, warm = (HOST_REPS, 1) if iters <= 100 else (1, 0)
            us, (lab_host, models_host) = timed(lambda: sm.setMapPointCloud(mp, mn), replaced, reps, warm)
            case["replaced_numpy"] = dict(stats(us), host_alone=stats(host_only[warm:]), labels_equal=bool(np.array_equal(lab_host, lab_dev)),
                                          models_equal=bool(np.array_equal(models_host, models_dev)))
        res["cases"][f"iters{iters}_planes{planes}"] = case
        print(f"iters {iters} planes {planes}: {json.dumps(case)}", flush=True)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
