"""GPU-box helper: the RANSAC registration on resident submaps (Submap.ransacRegistration; contract: include/o3s_registration.h
"RANSAC") on the sweep-size and closure-size pairs of tools/features_bench.py.  Per pair, wall time around the blocking call, median of
REPS calls after WARM warm-ups with the garbage collector off during the timed calls:
  * the reference's default parameters (10 000 000 iterations at most, confidence 0.999: the loop ends at est_k);
  * confidence = 1.0 with a fixed 1 000 000 iterations: hypotheses per second;
  * as context only, the numpy restatement (tests/ransac_ref.py) of the default run on this job's CPUs (REF=0 skips it).
The call includes the feature correspondences in front of the loop (k_feat_nn); `correspondences_median_ms` is that part alone.
Run under `rocprofv3 --kernel-trace --stats` for the per-kernel shares (REF=0 REPS=3 WARM=1 there).  OUT=<path> also writes the JSON
line there."""
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from open3d_slam_advanced_rss_2024_public_amd import Submap, cloud_ops as co, registration as reg, submap as sm, synthetic as syn  # noqa: E402

REPS = int(os.environ.get("REPS", "11"))
WARM = int(os.environ.get("WARM", "3"))
REF = os.environ.get("REF", "1") != "0"
FIXED = int(os.environ.get("FIXED", "1000000"))


def timed(fn):
    ms = []
    for rep in range(WARM + REPS):
        gc.collect()
        gc.disable()
        t0 = time.perf_counter()
        r = fn()
        dt = (time.perf_counter() - t0) * 1e3
        gc.enable()
        if rep >= WARM:
            ms.append(dt)
    return r, float(np.median(ms)), [round(x, 4) for x in ms]


def one_size(area, n_map):
    world = syn.make_world(area, seed=21)
    mp, _ = syn.make_map(world, n_map, 0.1, seed=22)
    mp = mp.astype(np.float64) + np.random.default_rng(23).normal(0.0, 0.01, (n_map, 3))
    big = co.croppingVolumeFactory("MaxRadius", 1.0e6)
    a, b = Submap(0.1, big), Submap(0.1, big)
    half = mp[:, 0] < np.median(mp[:, 0]) + 0.15 * (mp[:, 0].max() - mp[:, 0].min())     # b: 65 % of the map, overlapping a's
    a.setMapPointCloud(mp, None)
    b.setMapPointCloud(np.ascontiguousarray(mp[half]), None)
    prm = sm.featureParams()
    n, m = a.computeFeatures(prm), b.computeFeatures(prm)
    (pairs, _), cmed, _ = timed(lambda: a.featureCorrespondences(b, True, 3))
    reg.ransac_reserve(len(pairs))
    dflt = reg.RansacParams(seed=1)
    r, med, ms = timed(lambda: a.ransacRegistration(b, dflt))
    fixed = reg.RansacParams(seed=1, max_iteration=FIXED, confidence=1.0)
    rf, fmed, fms = timed(lambda: a.ransacRegistration(b, fixed))
    loop_ms = max(fmed - cmed, 1e-9)
    out = {"map_points": int(n_map), "sparse_points": int(n), "target_sparse_points": int(m), "correspondences": int(len(pairs)),
           "correspondences_median_ms": cmed,
           "default_median_ms": med, "default_ms": ms, "default_est_k": r.est_k, "default_winner": r.best_iteration,
           "default_evaluated": r.evaluated, "default_inliers": int(len(r.correspondence_set)), "default_fitness": r.fitness,
           "fixed_iterations": FIXED, "fixed_median_ms": fmed, "fixed_ms": fms, "fixed_evaluated": rf.evaluated,
           "fixed_hypotheses_per_s": FIXED / (loop_ms * 1e-3), "fixed_evaluations_per_s": rf.evaluated / (loop_ms * 1e-3),
           # a subtraction-free count of the evaluation's work: 9 mul + 9 add for T s, 3 sub, 3 mul + 2 add, sqrt, compare, mul + add
           "fixed_evaluation_flop": int(rf.evaluated) * int(len(pairs)) * 29}
    if REF:
        import ransac_ref as rr

        pa, pb = a.getSparseMapPointCloud()[0], b.getSparseMapPointCloud()[0]
        t0 = time.perf_counter()
        w = rr.ransac(pa, pb, pairs, seed=1)
        out["numpy_restatement_default_s"] = round(time.perf_counter() - t0, 3)
        out["numpy_restatement_agrees"] = bool((w.best_iteration, w.est_k, w.evaluated) == (r.best_iteration, r.est_k, r.evaluated))
        out["numpy_flagged_evaluated"] = int(w.flagged_evaluated)
    return out


res = {"tool": "ransac_bench", "reps": REPS, "warm": WARM,
       "sweep_size": one_size(700.0, 60000), "closure_size": one_size(9000.0, 400000)}
line = json.dumps(res)
print(line)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as f:
        f.write(line + "\n")
