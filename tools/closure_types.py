"""GPU-box helper: one loop-closure refinement (PlaceRecognition.cpp:97-150 — overlap selection, RegistrationICP, information
matrix) between two resident submaps of N points each, with each of the reference's three CloudRegistrationTypes, the three
alternating in one process; median of REPS calls each after WARM warm-up rounds.  Run under `rocprofv3 --kernel-trace --stats`
for the per-kernel picture.  N=600000 REPS=11 WARM=2 by default; OUT=<path> also writes the JSON line there."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from open3d_slam_advanced_rss_2024_public_amd import Submap, cloud_ops as co, registration as reg, synthetic as syn  # noqa: E402

N = int(os.environ.get("N", "600000"))
REPS = int(os.environ.get("REPS", "11"))
WARM = int(os.environ.get("WARM", "2"))
TYPES = ("PointToPlaneIcp", "PointToPointIcp", "GeneralizedIcp")

world = syn.make_world(9000.0, seed=3)
T = syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.3), np.array([1.0, 2.0, 1.5]))
tp, tn = syn.make_scan(world, N, T, radius=25.0, sigma=0.0, seed=4)
R, t = T[:3, :3], T[:3, 3]
tgt = tp.astype(np.float64) @ R.T + t
tgt_n = tn.astype(np.float64) @ R.T
sp, sn = syn.make_scan(world, N, T, radius=22.0, sigma=0.005, seed=5)
src = sp.astype(np.float64)
big = co.croppingVolumeFactory("MaxRadius", 1.0e6)
a, b = Submap(0.0, big), Submap(0.0, big)
nudge = syn.make_T(None, np.array([0.25, 0.0, 0.0]))
a.insertScan(src - np.array([0.25, 0.0, 0.0]), sn.astype(np.float64), nudge)   # GICP builds the source's covariances from its normals
b.insertScan(tgt - np.array([0.25, 0.0, 0.0]), tgt_n, nudge)
init = syn.perturb_pose(T, 0.03, 0.3, seed=4)   # what the RANSAC pose of a closure is off by (closed-loop run: 1.7 - 3 cm)
reg.reserve(len(a) + 16, len(b) + 16)

ms = {k: [] for k in TYPES}
last = {}
for rep in range(WARM + REPS):
    for kind in TYPES:
        t0 = time.perf_counter()
        res, info, n_ov = reg.registration_icp_submaps_overlap(a, b, 1.0, init, 2.0, registration_type=kind)
        dt_ms = (time.perf_counter() - t0) * 1e3
        if rep >= WARM:
            ms[kind].append(round(dt_ms, 3))
        last[kind] = (res, n_ov)
out = {"points": [len(a), len(b)], "reps": REPS, "warmup": WARM, "types": {}}
for kind in TYPES:
    res, n_ov = last[kind]
    Tr = np.asarray(res.transformation)
    dt = float(np.linalg.norm(Tr[:3, 3] - T[:3, 3]))
    ang = float(np.arccos(np.clip((np.trace(Tr[:3, :3].T @ T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    out["types"][kind] = {"overlap_points": list(map(int, n_ov)), "updates": int(res.iterations), "fitness": res.fitness,
                          "correspondences": int(res.correspondences), "median_ms": float(np.median(ms[kind])), "ms": ms[kind],
                          "offset_m": round(dt, 5), "offset_rad": round(ang, 6)}
base = out["types"]["PointToPlaneIcp"]["median_ms"]
for kind in TYPES:
    out["types"][kind]["vs_point_to_plane"] = round(out["types"][kind]["median_ms"] / base, 3)
line = json.dumps(out)
print(line)
if os.environ.get("OUT"):
    os.makedirs(os.path.dirname(os.environ["OUT"]) or ".", exist_ok=True)
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
