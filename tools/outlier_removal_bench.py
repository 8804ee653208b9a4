"""GPU-box helper: what the outlier filters cost (include/outlier_removal/o3s_outlier_removal.h), written as one JSON line to OUT
(default profiles/outlier_removal/outlier_removal_bench.json).

  scan       the merge cloud of a 64 x 2048 sweep (voxel 0.1), resident: ProcessedScan.removeOutliers, radius {0.5 m, 3} and
             statistical {20, 2.0}; the sweep is pre-processed again before every timed call (the filter works in place), outside
             the timed window
  submap     a 0.4 M-point resident submap (voxel 0.1): Submap.removeOutliers, the same two filters; the map is uploaded again
             before every timed call, outside the timed window
  replaced   the route the call replaces: download the map, filter on the host, upload the result — the host filter is
             scipy's cKDTree on 16 threads (neighbour counts within the radius / the 20 nearest), given beside it on its own

Medians of REPS (default 9) wall-clock calls after one warm-up, min - max beside them.  Same process, same clouds for all of it."""
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan, Submap  # noqa: E402
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co, synthetic as syn  # noqa: E402

REPS = int(os.environ.get("REPS", "9"))
SUBMAP = int(os.environ.get("SUBMAP", "400000"))
OUT = os.environ.get("OUT") or os.path.join(ROOT, "profiles", "outlier_removal", "outlier_removal_bench.json")
MAP_VOXEL = 0.1
RADIUS = co.outlier_params("radius", 3, 0.5)
STAT = co.outlier_params("statistical", 20, 2.0)


def stats(us):
    v = np.asarray(us, np.float64) / 1e3
    return {"ms_median": float(np.median(v)), "ms_min": float(v.min()), "ms_max": float(v.max())}


def timed(prepare, fn, reps):
    out, us = None, []
    for k in range(reps + 1):   # the first call warms up
        prepare()
        gc.disable()
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e6
        gc.enable()
        if k:
            us.append(dt)
    return us, out


def host_filter(p, q):
    from scipy.spatial import cKDTree

    tree = cKDTree(p)
    if q.kind == 1:
        cnt = tree.query_ball_point(p, q.value, workers=16, return_length=True)
        return cnt > q.nb
    d, _ = tree.query(p, k=q.nb, workers=16)
    avg = d.mean(axis=1)
    return avg < avg.mean() + q.value * avg.std(ddof=1)


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
    res = {"workload": f"medians of {REPS} wall-clock calls after one warm-up", "map_points": int(len(mp)), "sweep_points": int(len(sweep)),
           "radius": {"nb_points": RADIUS.nb, "radius": RADIUS.value}, "statistical": {"nb_neighbors": STAT.nb, "std_ratio": STAT.value}}
    for name, q in (("radius", RADIUS), ("statistical", STAT)):
        us, (n_merge, n_match) = timed(lambda: sc.preprocess(big, 0.1, narrow, sweep, sweep_n), lambda: sc.removeOutliers(narrow, q), REPS)
        before = sc.preprocess(big, 0.1, narrow, sweep, sweep_n)
        res[f"scan_{name}"] = dict(stats(us), merge_before=int(before[0]), merge_after=int(n_merge), match_after=int(n_match))
        us, (removed, _) = timed(lambda: sm.setMapPointCloud(mp, mn), lambda: sm.removeOutliers(q), REPS)
        res[f"submap_{name}"] = dict(stats(us), removed=int(removed))
        kept_dev = sm.getMapPointCloud()[0]

        host_only = []

        def replaced():
            p, n = sm.getMapPointCloud()
            t0 = time.perf_counter()
            keep = host_filter(p, q)
            host_only.append((time.perf_counter() - t0) * 1e6)
            sm.setMapPointCloud(p[keep], n[keep])
            return int(keep.sum())

        us, kept_host = timed(lambda: sm.setMapPointCloud(mp, mn), replaced, max(3, REPS // 3))
        res[f"replaced_{name}"] = dict(stats(us), host_filter_alone=stats(host_only[1:]), kept_host=kept_host, kept_device=int(len(kept_dev)))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
