"""GPU-box helper: the map of all resident submaps (AssembledMap, include/assembled_map/o3s_assembled_map.h) against the only route a
user had before it.  A ring of K resident submaps of N points each, built as tools/pose_graph_bench.py builds them; per voxel size
(0.1 = SlamWrapperRos::publishMaps' assembledMapVoxelSize_, then 0.0 = the plain concatenation saveMap writes), each as the median
of REPS (>= 11) timed calls after WARM warm-up calls, with min and max as the spread:
  build_ms             AssembledMap.build alone (returns with the result complete in HBM)
  build_download_ms    build + getPointCloud(): the result crosses the bus once
  route_ms             getMapPointCloud() of every submap, np.concatenate, cloud_ops.voxelize_attr on the host arrays (voxel 0.0: the
                       route ends at the concatenation) — code this tool's subject does not touch, timed in the same run on the same
                       data, the three alternating call by call
and whether the two results are the same bytes.  `accept` = build + download is faster than the route by more than the two spreads
together (route min - build_download max > 0 is the stronger form, reported as `gap_ms`).
N=600000 K=8 REPS=11 WARM=2 by default; OUT=<path> also writes the JSON line there.  TRACE=1: a short run for
`rocprofv3 --kernel-trace --stats -- python tools/assemble_bench.py` (three builds per voxel size, no route, no timing).
Wall-clock times of whole calls: no bandwidth figure is derived from them."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from open3d_slam_advanced_rss_2024_public_amd import AssembledMap, Submap, cloud_ops as co, synthetic as syn  # noqa: E402
from open3d_slam_advanced_rss_2024_public_amd.mapper import mul4  # noqa: E402

N = int(os.environ.get("N", "600000"))
K = int(os.environ.get("K", "8"))
REPS = max(int(os.environ.get("REPS", "11")), 11)
WARM = int(os.environ.get("WARM", "2"))
TRACE = os.environ.get("TRACE") == "1"
VOXELS = (0.1, 0.0)


def stat(ms):
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(np.min(ms)), 4), "max_ms": round(float(np.max(ms)), 4), "n": len(ms)}


# ---- the ring: one cloud of N points, K resident copies at the poses of a ring, copy k drifted by D^k (tools/pose_graph_bench.py) ----
world = syn.make_world(9000.0, seed=3)
T0 = syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.3), np.array([1.0, 2.0, 1.5]))
bp, bn = syn.make_scan(world, N, T0, radius=25.0, sigma=0.005, seed=4)
bp, bn = bp.astype(np.float64), bn.astype(np.float64)
big = co.croppingVolumeFactory("MaxRadius", 1.0e6)
drift = syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.002), np.array([0.04, -0.03, 0.005]))
D, maps = np.eye(4), []
for k in range(K):
    a = 2 * np.pi * k / K
    pose = mul4(D, syn.make_T(syn.rot_axis_angle([0, 0, 1], a), np.array([40.0 * np.cos(a), 40.0 * np.sin(a), 0.0])))
    m = Submap(0.0, big)
    m.setMapPointCloud(bp @ pose[:3, :3].T + pose[:3, 3], bn @ pose[:3, :3].T)
    maps.append(m)
    D = mul4(drift, D)
total = int(sum(len(m) for m in maps))
print(f"{K} resident submaps, {total} points in total", flush=True)

am = AssembledMap()

if TRACE:
    for voxel in VOXELS:
        for _ in range(3):
            am.build(maps, voxel)
    print(json.dumps({"trace_run": True, "submaps": K, "points_total": total, "sizes": {str(v): am.build(maps, v) for v in VOXELS}}))
    sys.exit(0)


def route(voxel):
    """What a user did at the parent commit: every submap over the bus, concatenate, push the host cloud through the voxeliser."""
    clouds = [m.getMapPointCloud() for m in maps]
    P, Nn = np.concatenate([c[0] for c in clouds]), np.concatenate([c[1] for c in clouds])
    if voxel <= 0.0:
        return P, Nn
    gp, gn, _, _, _ = co.voxelize_attr(voxel, P, Nn)
    return gp, gn


out = {"submaps": K, "points_per_submap": [len(m) for m in maps], "points_total": total, "reps": REPS, "warmup": WARM, "voxel": {}}
for voxel in VOXELS:
    t_build, t_both, t_route = [], [], []
    got = want = None
    for r in range(WARM + REPS):
        t0 = time.perf_counter()
        am.build(maps, voxel)
        t1 = time.perf_counter()
        am.build(maps, voxel)
        got = am.getPointCloud()
        t2 = time.perf_counter()
        want = route(voxel)
        t3 = time.perf_counter()
        if r >= WARM:
            t_build.append((t1 - t0) * 1e3)
            t_both.append((t2 - t1) * 1e3)
            t_route.append((t3 - t2) * 1e3)
    b, bd, ro = stat(t_build), stat(t_both), stat(t_route)
    spreads = (bd["max_ms"] - bd["min_ms"]) + (ro["max_ms"] - ro["min_ms"])
    out["voxel"][str(voxel)] = {
        "result_points": len(am), "same_bytes_as_route": bool(got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()),
        "build": b, "build_download": bd, "route": ro, "device_bytes": am.device_bytes(),
        "median_gain_ms": round(ro["median_ms"] - bd["median_ms"], 4), "spreads_ms": round(spreads, 4), "gap_ms": round(ro["min_ms"] - bd["max_ms"], 4),
        "accept": bool(ro["median_ms"] - bd["median_ms"] > spreads)}
line = json.dumps(out)
print(line)
if os.environ.get("OUT"):
    os.makedirs(os.path.dirname(os.environ["OUT"]) or ".", exist_ok=True)
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
