"""The one JSON line `bench.py` prints: the contract's fields, and that what `config` says is what `value` was measured on."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_bench_line_describes_the_run_that_was_timed():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu", "--full"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout            # exactly one line on stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["scaling"] == "weak"
    c = d["config"]
    assert c["workload"].startswith("C2") and c["scan_points"] == 100_000 and c["map_points"] == 2_000_000 and c["iterations_per_step"] == 50
    # ONE pair per GPU was timed: the "8 pairs in flight" figure is an `extra`, it must not leak into the description of `value`
    assert c["pairs_per_gpu"] == 1 and c["parallelism"].startswith("1 independent scan/map pair, 1 per GPU")
    assert abs(d["value"] - 50 * d["steps"] / (d["ms_per_step"] * d["steps"] * 1e-3)) <= 1e-3 * d["value"]
    assert d["extra"]["batched_on_one_gpu"]["pairs_in_flight"] == 8 and d["extra"]["batched_on_one_gpu"]["value"] > d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["kernel"] == "k_match2" and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    assert {k_["kernel"] for k_ in d["roofline_kernels"]} == {"k_match2", "k_classify", "k_sel_ne", "k_solve"}
    # the matcher's first iteration (no incumbents) apart from the converged ones: bytes and time of the SAME launches on each side
    sp = r["split"]
    f, c_ = sp["first_iteration"], sp["converged_iterations"]
    for side in (f, c_):
        assert abs(side["frac"] - side["achieved"] / r["peak"]) < 1e-4
        assert abs(side["achieved"] - side["alg_bytes_per_launch"] / (side["avg_launch_ms"] * 1e-3) / 1e9) <= 1e-2 * side["achieved"]
    assert f["cbar_candidates_per_query"] > c_["cbar_candidates_per_query"] and f["avg_launch_ms"] > c_["avg_launch_ms"]
    assert abs((f["cbar_candidates_per_query"] + 49 * c_["cbar_candidates_per_query"]) / 50 - r["cbar_candidates_per_query"]) < 0.02
    assert "converged_microbench_frac" not in r
    # BASELINE config 4 rides in the same --full line: its own value, roofline and split
    c4 = d["extra"]["c4"]
    assert c4["workload"].startswith("C4: 500000-pt scan vs 20000000-pt") and c4["value"] > 1000 and c4["pose_error_vs_ground_truth_m"] < 5e-3
    assert abs(c4["value"] - 50 * c4["steps"] / (c4["ms_per_step"] * c4["steps"] * 1e-3)) <= 1e-3 * c4["value"]
    r4 = c4["roofline"]
    assert r4["kernel"] == "k_match2" and abs(r4["frac"] - r4["achieved"] / r4["peak"]) < 1e-4 and r4["frac"] <= 1.0
    assert r4["split"]["first_iteration"]["avg_launch_ms"] > r4["split"]["converged_iterations"]["avg_launch_ms"]
    # the chain open3d_slam runs, call by call: no call may stall (round 4's driver line had a 39 ms garbage collection of the
    # bench's interpreter inside the loop: 2.2 ms mean over 0.27 ms calls), no wait may end on the 2 ms stream guard, and a
    # registration costs the host what its kernels take plus at most 0.1 ms
    for y in (d["extra"]["icp_yaml_chain"], c4["icp_yaml_chain"]):
        pc = y["ms_per_call"]
        assert pc["min"] <= pc["median"] <= pc["p99"] <= pc["max"]
        # no call may stall: the second slowest of the calls within 2 x the median (ONE call may meet a hiccup of the box's host —
        # a pre-empted polling thread shows as host_wait in `slowest_calls` — but a stall of the path would hit every call or many)
        assert y["slowest_calls"][1]["ms"] <= 2.0 * pc["median"] and pc["max"] <= 10.0 * pc["median"], y["slowest_calls"]
        assert pc["median"] <= y["gpu_chain_ms"] + y["gpu_prepare_ms"] + 0.1, y
        assert y["ms_per_registration"] == pc["median"]
        assert y["waits_ended_by"]["stream_guard"] == 0 and y["waits_ended_by"]["post"] >= y["calls"]
        assert y["issued"]["replayed"] == y["calls"] and y["issued"]["eager"] == 0 and y["issued"]["captured"] == 0
        assert y["python_gc"]["collections_while_timed"] == []
    assert d["extra"]["icp_yaml_chain"]["iterations"] == 5 and d["extra"]["icp_yaml_chain"]["ms_per_call"]["median"] <= 0.32
    # BASELINE configs 3 and 5 ride in the same line too: every config has a driver-timed number
    c3 = d["extra"]["c3"]
    assert "error" not in c3, c3
    assert c3["pairs"] == 64 and c3["workload"].startswith("C3 on one GPU: 64 pairs, 100000-pt scan vs 400000-pt")
    assert c3["same_pose_as_single_calls"] is True and c3["pose_error_vs_ground_truth_m_max"] < 5e-3
    assert c3["value"] == c3["in_flight_64"]["icp_iterations_per_s"] > d["value"]          # 64 chains in flight beat one
    assert abs(c3["all_pairs_ms"] * 1e-3 * c3["pairs_per_s"] - 64) < 0.5 and 64 * 3 <= c3["in_flight_64"]["iterations_total"] <= 64 * 15
    c5 = d["extra"]["c5"]
    assert "error" not in c5 and "error" not in c5["closed_loop"], c5
    assert c5["pipeline_hz_steady_state"] > 500 and c5["ms_per_call_median"] < 2.0 and c5["pose_error_m_max"] < 0.1
    assert c5["value"] == max(c5["pipeline_hz_steady_state"], c5["three_stages_page_locked"]["pipeline_hz_steady_state"]) and "value_is" in c5
    cpu5 = c5["cpu_host_loop"]
    assert cpu5["kind"] == "port" and cpu5["cores"] >= 1 and cpu5["hz"] > 0 and c5["gpu_vs_cpu_hz"] > 1.0
    assert set(c5["mapper_stopwatches_ms_median"]) == {"auxiliary (pre-process)", "reference re-init", "scan2map registration", "scan insertion"}
    r2 = c5["reference_renewed_every_2_s"]      # the renewal period the reference's parameter files set, on the same sweeps
    assert r2["reference_renewal_period_s"] == 2.0 and r2["pipeline_hz_steady_state"] > 500 and r2["pose_error_m_max"] < 0.1
    assert r2["ms_per_scan_median"] <= c5["ms_per_call_median"] * 1.1      # nineteen of twenty sweeps skip the re-initialisation
    t3 = c5["three_stages_page_locked"]         # staging, pre-processing and mapping on three host threads
    assert "error" not in t3 and t3["pipeline_hz_steady_state"] > 500 and t3["pose_error_m_max"] < 0.1
    assert t3["reference_renewed_every_2_s"]["pipeline_hz_steady_state"] > 500
    cl = c5["closed_loop"]
    assert cl["submaps"] >= 2 and cl["refinements"] == len(cl["refinement_ms"]) >= 1 and max(cl["refinement_ms"]) < 10.0
    assert d["extra"]["sharded_one_pair"] is None                     # one process, no process group: nothing to shard over
    assert any("libamdhip64" in p_ for p_ in d["extra"]["rocm_runtime"])


def test_plain_bench_line_is_the_headline_alone():
    """Without --full the run sets up, warms up, times the steps and prints the headline: the contract's fields mean what they mean
    in a --full line, every measurement beyond the timed steps is null, and the run spends at most 30 s outside its steps."""
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    wall_s = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["full"] is False and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["metric"] == "ICP iterations/s (100k-pt scan vs 2M-pt map)" and d["unit"] == "ICP iterations/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["scaling"] == "weak"
    assert d["config"]["workload"].startswith("C2") and d["config"]["pairs_per_gpu"] == 1 and d["config"]["iterations_per_step"] == 50
    assert abs(d["value"] - 50 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    assert d["roofline"] is None and d["roofline_kernels"] is None and d["cpu_baseline"] is None
    e = d["extra"]
    for k in ("pcie_inclusive_value", "batched_on_one_gpu", "icp_yaml_chain", "c3", "c4", "c5", "sharded_one_pair"):
        assert e[k] is None, k
    assert e["pose_error_vs_ground_truth_m"] < 5e-3 and e["kept_pairs"] > 0
    assert wall_s - (d["steps"] + d["warmup"]) * d["ms_per_step"] * 1e-3 <= 30.0, wall_s


def test_dump_outputs_writes_the_last_timed_step_and_repeats_it(tmp_path):
    """--dump-outputs DIR: the pose and ICP stats the last timed step returned, as .npy files; the inputs are seeded, so a second run
    with the same arguments writes the same arrays, and `steps` / `ms_per_step` describe the timed loop that was asked for."""
    import numpy as np

    runs = []
    for k, steps in enumerate((2, 3)):
        d_out = tmp_path / f"run{k}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--timing-only",
                              "--dump-outputs", str(d_out)], capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1])
        assert d["ms_per_step"] > 0 and abs(d["value"] - 50 / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
        files = sorted(os.listdir(d_out))
        assert files == sorted(["pose.npy", "iterations.npy", "max_iters_reached.npy", "kept_pairs.npy", "matched_pairs.npy",
                                "point_used_ratio.npy", "weighted_point_used_ratio.npy", "last_trim_limit.npy"]), files
        arrs = {f[:-len(".npy")]: np.load(d_out / f) for f in files}
        assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        runs.append(arrs)
    a, b = runs
    assert a["pose"].shape == (1, 4, 4) and a["iterations"].tolist() == [50.0] and a["kept_pairs"][0] > 0
    for f in a:
        assert np.array_equal(a[f], b[f]), f


def test_n_gpu_line_also_measures_the_one_pair_sharded_mode():
    """The N > 1 run is the only one that will ever see several GPUs: besides the pairs measurement (mode 1) its --full line must time
    the one-pair-sharded mode (mode 2) on the same ranks — rehearsed here with a process group of one rank on the one GPU
    (O3S_BENCH_FORCE_DIST=1: RCCL at world size 1)."""
    env = dict(os.environ, O3S_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu", "--batch-pairs", "0",
                          "--full"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1])
    assert d["scaling"] == "weak" and d["config"]["pairs_per_gpu"] == 1
    sh = d["extra"]["sharded_one_pair"]
    assert sh is not None and "error" not in sh, sh
    assert sh["ranks"] == 1 and sh["collectives_per_iteration"] == 3 and sh["bytes_per_iteration_per_rank"] == 16 * 2048 * 4 + 8192 * 4 + (128 + 34 * 128 + 34 * 196) * 8
    assert sh["value"] > 1000 and sh["pose_error_vs_ground_truth_m"] < 5e-3
    rs = sh["roofline"]                                       # a line that can be graded on the day a node exists: per-rank roofline, RCCL ranks counted
    assert rs["kernel"] == "k_match2" and rs["per"] == "rank" and rs["points_per_rank"] == 100_000 and sh["rccl_ranks"] == 1
    assert abs(rs["frac"] - rs["achieved"] / rs["peak"]) < 1e-4 and 0.0 < rs["frac"] <= 1.0
    assert abs(rs["achieved"] - rs["alg_bytes_per_launch"] / (rs["avg_launch_ms"] * 1e-3) / 1e9) <= 1e-2 * rs["achieved"]
    assert sh["rccl_collectives_total"] >= 3 * 50            # RCCL saw the exchanges (eager call + graph capture)
    assert d["extra"]["c4"] is None and d["extra"]["c3"] is None and d["extra"]["c5"] is None   # those extras belong to the plain N = 1 line
