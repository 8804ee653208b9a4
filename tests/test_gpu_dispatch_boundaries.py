"""The ICP chain on both sides of its dispatch switches, against the oracle.

csrc/o3s_icp.hip picks its kernels per call from the reading size, the map density and the config: k_match2 or
k_match_mirror; the row-disc or the ring far search; the first-iteration index of dense maps or the main one in iteration 0;
4 or 2 lanes per query; the matched normal fetched by k_match2 or gathered by k_classify; one k_sel_ne launch or
k_sel_finish + k_normal_eq; the single- or multi-block candidate sweep; the speculative trim limit or level 1 only; eager,
captured or replayed.  Every case here is compared with oracle.OracleIcp under the contract of test_gpu_fuzz.py (status,
iteration count and per-iteration kept counts equal; trim limits bit-equal or within 1e-5 relative where fp64 summation
order differs; pose within 1e-5 m / 1e-5 rad), eager, captured and replayed calls are bit-identical, and the hooks build's
O3S_PRINT_CHAIN report proves that each case took the side of every switch it is named for."""
import functools
import re

import numpy as np
import pytest

from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn

pytestmark = pytest.mark.gpu

THREADS = 16
INF = float("inf")


# ---- data -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nominal_pair(hi):
    """icp.yaml scale: a 0.1 m map a few times the reading (its cell stays at maxDist / 3: no first-iteration index)."""
    return syn.make_scan_pair(hi, 3 * hi, 0.1, seed=hi % 97)


@functools.lru_cache(maxsize=None)
def dense_pair():
    """A 0.02 m map of 10^6 points: the matcher shrinks its cell and builds the first-iteration index."""
    return syn.make_scan_pair(262_145, 1_000_000, 0.02, seed=5, radius=5.0)


@functools.lru_cache(maxsize=None)
def mirror_box(k):
    """conditioning_cases row k on 50 k-point boxes (same cloud: reading point i is reference point i), dense enough at
    maxDist 1.0 for the first-iteration index (at 10 k points the density probe lands right at the 0.85 cut)."""
    return syn.conditioning_cases(50_000, 1.0, 0.135, 20.0, True)[k]


def oracle_config(kw):
    o = {k: v for k, v in kw.items() if k not in ("grid_cell", "sort_queries", "use_graph")}
    o["matcher"] = 1 if o.get("matcher") == "MirrorMatcher" else 0
    for k in ("trim_ratio", "max_normal_angle", "max_dist_outlier"):
        if k in o and o[k] is None:
            o[k] = -1.0
    return orc.OracleConfig(**o)


# ---- runs and checks --------------------------------------------------------------------------------------------------
def run_calls(kw, ref, refn, read, readn, T_init, calls=3):
    """`calls` compute_resident calls on one handle: with use_graph on, eager, captured, replayed."""
    g = ICP(IcpConfig(**kw))
    assert g.init_reference(ref, refn)
    g.set_reading(read, readn)
    out = []
    for _ in range(calls):
        T = g.compute_resident(T_init)
        n = g.stats.iterations
        out.append(dict(T=T, n=n, limit=g.stats.trace_limit[:n].copy(), kept=g.stats.trace_kept[:n].copy(),
                        trace_T=g.stats.trace_T[:n].copy(), issued=g.host_split_ex()["issued"]))
    g.close()
    return out


def assert_bit_identical(a, b, ctx):
    assert a["n"] == b["n"], ctx
    assert np.array_equal(a["T"], b["T"]), ctx
    assert np.array_equal(a["limit"].view(np.uint32), b["limit"].view(np.uint32)), ctx
    assert np.array_equal(a["kept"], b["kept"]) and np.array_equal(a["trace_T"], b["trace_T"]), ctx


def run_oracle(kw, ref, refn, read, readn, T_init):
    o = orc.OracleIcp(oracle_config(kw), threads=THREADS)
    assert o.init_reference(ref, refn) == orc.OK
    To, code = o.compute(read, readn, T_init, raise_on_error=False)
    return o, To, code


def assert_agrees_with_oracle(r, o, To, code, ctx):
    assert code == orc.OK, (ctx, code)
    assert r["n"] == o.stats.iterations, (ctx, r["n"], o.stats.iterations)
    n = r["n"]
    assert np.array_equal(r["kept"], o.trace_kept[:n]), (ctx, r["kept"], o.trace_kept[:n])
    gl, ol = r["limit"], o.trace_limit[:n]
    if not np.array_equal(gl, ol, equal_nan=True):
        fin = np.isfinite(ol)
        assert np.array_equal(np.isfinite(gl), fin) and np.all(np.abs(gl[fin] - ol[fin]) <= 1e-5 * np.abs(ol[fin])), (ctx, gl, ol)
    dt, ang = orc.pose_error(To, r["T"])
    assert np.linalg.norm(dt) <= 1e-5 and ang <= 1e-5, (ctx, dt, ang)


def check_three_calls(out, ctx):
    assert [r["issued"] for r in out] == ["eager", "captured", "replayed"], ctx
    for r in out[1:]:
        assert_bit_identical(out[0], r, ctx)


# ---- the case list ----------------------------------------------------------------------------------------------------
# Options spread over the size boundaries so that each meets every boundary at least once:
#   nrm = no reading normals (has_n false), out = max_dist_outlier set, notrim = trim_ratio None, inf = max_dist inf (ring search)
OPTS = {"nrm": {}, "out": dict(max_dist_outlier=0.3), "notrim": dict(trim_ratio=None), "inf": dict(max_dist=INF)}
BOUNDARIES = [(65_535, 65_536, ("nrm", "out"), ("notrim", "inf")),          # lanes per query 4 / 2
              (131_072, 131_073, ("notrim", "inf"), ("nrm", "out")),       # one k_sel_ne launch / k_sel_finish + k_normal_eq
              (199_999, 200_000, ("nrm", "inf"), ("out", "notrim")),       # k_classify gathers the normal / k_match2 fetches it
              (262_144, 262_145, ("out", "notrim"), ("nrm", "inf"))]       # single- / multi-block candidate sweep
DENSE = [(199_999, ()), (200_000, ("nrm",)), (262_144, ("out",)), (262_145, ("notrim", "nrm"))]


def kdtree_cases():
    cases = []
    for lo, hi, opts_lo, opts_hi in BOUNDARIES:
        for N, opts in ((lo, opts_lo), (hi, opts_hi)):
            cases.append(("nominal", hi, N, opts))
    for N, opts in DENSE:
        cases.append(("dense", None, N, opts))
    return cases


KD_CASES = kdtree_cases()
KD_IDS = [f"{m}-{N}-{'+'.join(o) or 'yaml'}" for m, _, N, o in KD_CASES]
# (conditioning row, reading size, normal gate): N = M and N < M, gate on and off
MIRROR_CASES = [(8, 50_000, True), (8, 50_000, False), (16, 30_011, True), (16, 30_011, False)]
MIRROR_IDS = [f"row{k}-N{N}-{'gate' if g else 'nogate'}" for k, N, g in MIRROR_CASES]


def kdtree_inputs(kind, hi, N, opts, **over):
    sp = nominal_pair(hi) if kind == "nominal" else dense_pair()
    kw = dict(use_graph=True)
    for o in opts:
        kw.update(OPTS[o])
    kw.update(over)
    readn = None if "nrm" in opts else sp.scan_normals[:N]
    return kw, (sp.map_xyz, sp.map_normals, sp.scan_xyz[:N], readn, sp.T_init)


def mirror_inputs(k, N, gate, max_dist, **over):
    c = mirror_box(k)
    kw = dict(matcher="MirrorMatcher", max_dist=max_dist, trim_ratio=0.9, max_normal_angle=1.57 if gate else None,
              use_differential=True, min_diff_rot=1e-5, min_diff_trans=1e-4, smooth_length=3, max_iters=30, use_graph=True)
    kw.update(over)
    return kw, (c.ref_xyz, c.ref_normals, c.read_xyz[:N], c.read_normals[:N], c.initial_guess)


def expected_paths(N, mirror, first_index, kw, has_n):
    """The side of every switch a case is named for (csrc/o3s_icp.hip: chain_args, chain_index, normals_from_matcher)."""
    finite = np.isfinite(kw.get("max_dist", 0.5))
    e = dict(N=N, matcher="mirror" if mirror else "kdtree", far="rows" if finite else "ring",
             it0_index="first" if first_index else "main", normals_from_matcher=int(N >= 200_000 and not mirror),
             fused=N <= 131_072, partial=int(N > 262_144), spec=int(kw.get("trim_ratio", 0.9) is not None and not mirror),
             has_n=int(has_n))
    if not mirror:
        e["match_g"] = 4 if N < 65_536 else 2
        e["first_g"] = 4 if (finite and N < 200_000) else e["match_g"]
    return e


CHAIN_RE = re.compile(r"^o3s chain: (.*)$", re.M)
GRID_RE = re.compile(r"^o3s grid: M (\d+) cell ([0-9.]+) .* first-iteration cell ([0-9.]+)$", re.M)


def parse_chain(err):
    out = []
    for m in CHAIN_RE.finditer(err):
        tok = m.group(1).split()
        out.append({tok[i]: tok[i + 1] for i in range(0, len(tok), 2)})
    return out


def assert_paths(rep, e, ctx):
    assert int(rep["N"]) == e["N"], (ctx, rep)
    for k in ("matcher", "far", "it0_index"):
        assert rep[k] == e[k], (ctx, k, rep)
    for k in ("normals_from_matcher", "partial", "spec", "has_n", "match_g", "first_g"):
        if k in e:
            assert int(rep[k]) == e[k], (ctx, k, rep)
    nbf = int(rep["nb_fused"])
    assert (nbf > 0) == e["fused"] and (nbf == 0 or nbf == (e["N"] + 511) // 512), (ctx, rep)


# ---- 3a: mirror on a dense reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,N,gate", MIRROR_CASES, ids=MIRROR_IDS)
def test_mirror_chain_on_a_dense_reference_agrees_with_the_oracle(k, N, gate):
    """MirrorMatcher with a finite maxDist on a map dense enough for the first-iteration index: k_match_mirror writes slots
    in the main index's order, so every iteration (iteration 0 of every replayed chunk included) must gather its normals
    there.  Every pair has d2 = 0, so the chain's bits cannot depend on maxDist: finite and unbounded give the same bits."""
    res = {}
    for md in (1.0, INF):
        kw, data = mirror_inputs(k, N, gate, md)
        out = run_calls(kw, *data)
        ctx = (k, N, gate, md)
        o, To, code = run_oracle(kw, *data)
        assert_agrees_with_oracle(out[0], o, To, code, ctx)
        assert out[0]["n"] > 5, ctx   # the chunked replay (5 iterations a chunk) runs iteration 0 of its second chunk
        check_three_calls(out, ctx)
        res[md] = out[0]
    assert_bit_identical(res[1.0], res[INF], (k, N, gate, "finite vs inf"))


# ---- 3b: size boundaries, KDTree --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,hi,N,opts", KD_CASES, ids=KD_IDS)
def test_kdtree_chain_on_both_sides_of_each_size_boundary_agrees_with_the_oracle(kind, hi, N, opts):
    """The icp.yaml chain on both sides of 65 536 (lanes per query), 131 072 (fused selection), 200 000 (matched normal from
    k_match2; first-iteration lanes) and 262 144 (multi-block sweep), on nominal maps and on a dense one (first-iteration
    index crossed with k_match2's normal fetch); eager, captured and replayed."""
    kw, data = kdtree_inputs(kind, hi, N, opts)
    ctx = (kind, N, opts)
    out = run_calls(kw, *data)
    o, To, code = run_oracle(kw, *data)
    assert_agrees_with_oracle(out[0], o, To, code, ctx)
    check_three_calls(out, ctx)


# ---- 3c: the paths the cases above take -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [("kd",) + c for c in KD_CASES] + [("mirror",) + c for c in MIRROR_CASES], ids=KD_IDS + MIRROR_IDS)
def test_each_case_takes_the_path_it_is_named_for(case, monkeypatch, hooks_lib, capfd):
    """The same cases on the hooks build with O3S_PRINT_CHAIN / O3S_PRINT_GRID, two iterations (0 and 1) per call: the report
    of every call shows the side of every switch the case is named for, and the map has the first-iteration index exactly
    where the case needs one (dense maps, the mirror boxes)."""
    monkeypatch.setenv("O3S_PRINT_CHAIN", "1")
    monkeypatch.setenv("O3S_PRINT_GRID", "1")
    if case[0] == "kd":
        _, kind, hi, N, opts = case
        kw, data = kdtree_inputs(kind, hi, N, opts, max_iters=2)
        dense, mirror = kind == "dense", False
        first = dense and np.isfinite(kw.get("max_dist", 0.5))
    else:
        _, k, N, gate = case
        kw, data = mirror_inputs(k, N, gate, 1.0, max_iters=2)
        dense, mirror, first = True, True, False   # a mirror chain never searches the first-iteration index
    capfd.readouterr()
    out = run_calls(kw, *data)
    err = capfd.readouterr().err
    grid = GRID_RE.findall(err)
    assert len(grid) == 1, err
    assert (float(grid[0][2]) > 0) == dense, (case, grid)
    reps = parse_chain(err)
    assert [r["issued"] for r in reps] == ["eager", "captured", "replayed"] == [r["issued"] for r in out], (case, err)
    e = expected_paths(N, mirror, first, kw, data[3] is not None)
    for rep in reps:
        assert_paths(rep, e, case)
    for r in out:
        assert r["n"] == 2, case


# ---- 3d: a seeded campaign over the axes test_gpu_fuzz.py never draws ----------------------------------------------------
CAMPAIGN_SEED = 20261021


def campaign_case(rng):
    """One case of the campaign: test_gpu_fuzz.py's sizes and chain axes plus the matcher, MaxDistOutlierFilter, a dense map
    and missing reading normals."""
    mirror = bool(rng.random() < 0.4)
    dense = bool(rng.random() < 0.4)
    N = int(rng.integers(200, 5000))
    M = int(rng.integers(2000, 40000))
    voxel = 0.02 if dense else float(rng.choice([0.05, 0.1, 0.2]))
    sp = syn.make_scan_pair(N, M, voxel, seed=int(rng.integers(0, 10**6)), radius=2.0 if dense else 15.0,
                            trans=float(rng.uniform(0, 0.3)), rot_deg=float(rng.uniform(0, 6)))
    ref, refn = sp.map_xyz, sp.map_normals
    if mirror:   # reading i = reference point i under a small rigid motion, plus noise; the reference shuffled first
        perm = rng.permutation(len(ref))
        ref, refn = ref[perm], refn[perm]
        N = min(N, len(ref))
        T_gt = syn.make_T(syn.rot_axis_angle(rng.normal(size=3), np.radians(float(rng.uniform(0, 6)))), rng.uniform(-0.3, 0.3, 3))
        read, readn = syn.transform_cloud(np.linalg.inv(T_gt), ref[:N].astype(np.float64), refn[:N].astype(np.float64))
        read = (read + rng.normal(0, 0.003, read.shape)).astype(np.float32)
        readn = readn.astype(np.float32)
        T_init = np.eye(4)
    else:
        read, readn, T_init = sp.scan_xyz, sp.scan_normals, sp.T_init
    md_choices = [0.5, 1.0] if dense else [0.1, 0.3, 0.5, 1.0, INF]
    kw = dict(matcher="MirrorMatcher" if mirror else "KDTreeMatcher", max_dist=float(rng.choice(md_choices)),
              trim_ratio=[None, 0.5, 0.9, 1.0][int(rng.integers(0, 4))], max_normal_angle=[None, 0.5, 1.57][int(rng.integers(0, 3))],
              max_dist_outlier=[None, None, 0.05, 0.2, 1.0][int(rng.integers(0, 5))], use_differential=bool(rng.integers(0, 2)),
              max_iters=int(rng.integers(1, 20)), smooth_length=int(rng.integers(0, 5)), counter_first=bool(rng.integers(0, 2)),
              grid_cell=0.0 if dense else float(rng.choice([0.0, 0.0, 0.07, 0.31])), sort_queries=bool(rng.integers(0, 2)),
              use_graph=bool(rng.integers(0, 2)))
    if rng.random() < 0.25:
        readn = None
    return mirror, dense, kw, (ref, refn, read, readn, T_init)


def test_random_matchers_outlier_filters_and_dense_maps_agree_with_the_oracle(monkeypatch, hooks_lib, capfd):
    """test_random_configurations_agree_with_the_oracle's sizes and chain axes, plus the matcher (mirror readings are a
    perturbed copy of the reference's first N points), MaxDistOutlierFilter, dense maps (0.02 m voxels, small radius: the
    first-iteration index) and missing reading normals.  Run on the hooks build so that the report counts the paths the
    campaign reached."""
    monkeypatch.setenv("O3S_PRINT_CHAIN", "1")
    monkeypatch.setenv("O3S_PRINT_GRID", "1")
    rng = np.random.default_rng(CAMPAIGN_SEED)
    cases, errors, exact = 20, 0, 0
    reached = dict(mirror_dense=0, first_index=0, mirror=0, outlier=0, no_normals=0)
    for case in range(cases):
        mirror, dense, kw, (ref, refn, read, readn, T_init) = campaign_case(rng)
        N = len(read)
        ctx = (case, N, len(ref), dense, kw)
        capfd.readouterr()
        g = ICP(IcpConfig(**kw))
        assert g.init_reference(ref, refn)
        eg = None
        try:
            Tg = g.compute(read, readn, T_init)
        except Exception as e:  # noqa: BLE001
            eg = type(e).__name__
        err = capfd.readouterr().err
        o, To, code = run_oracle(kw, ref, refn, read, readn, T_init)
        assert (eg is None) == (code == orc.OK), (ctx, eg, code)
        grid = GRID_RE.findall(err)
        reps = parse_chain(err)
        assert len(grid) == 1 and len(reps) <= 1, (ctx, err)
        if reps:
            rep = reps[0]
            assert rep["matcher"] == ("mirror" if mirror else "kdtree") and int(rep["has_n"]) == (readn is not None), (ctx, rep)
            if rep["it0_index"] == "first":
                reached["first_index"] += 1
            if mirror and float(grid[0][2]) > 0 and rep["far"] == "rows":
                assert rep["it0_index"] == "main", (ctx, rep)
                reached["mirror_dense"] += 1
        reached["mirror"] += mirror
        reached["outlier"] += kw["max_dist_outlier"] is not None
        reached["no_normals"] += readn is None
        g.close()
        if eg is not None:
            errors += 1
            continue
        n = g.stats.iterations
        r = dict(T=Tg, n=n, limit=g.stats.trace_limit[:n].copy(), kept=g.stats.trace_kept[:n].copy())
        assert_agrees_with_oracle(r, o, To, code, ctx)
        exact += int(np.array_equal(r["limit"], o.trace_limit[:n], equal_nan=True))
    assert errors <= cases // 4 and exact >= cases // 2, (errors, exact)
    assert all(v >= 2 for v in reached.values()), reached


# ---- 3e: the graph key covers the first-iteration grid --------------------------------------------------------------
def test_graph_key_covers_the_first_iteration_grid(monkeypatch, hooks_lib, capfd):
    """A captured iteration 0 bakes the first-iteration grid in by value.  Re-initialising a handle on the same reference with a
    coarser first-iteration edge keeps every allocation (and the main grid): the graph key must still tell the two chains
    apart, so the next three calls go out eager, captured, replayed and give the bits of a fresh handle with that edge."""
    sp = dense_pair()
    N = 40_000
    kw = dict(use_differential=True, max_iters=15, use_graph=True)
    read, readn = sp.scan_xyz[:N], sp.scan_normals[:N]
    monkeypatch.setenv("O3S_PRINT_GRID", "1")
    monkeypatch.setenv("O3S_PRINT_CHAIN", "1")
    monkeypatch.setenv("O3S_FIRST_GRID", "0.061")
    capfd.readouterr()
    g = ICP(IcpConfig(**kw))
    assert g.init_reference(sp.map_xyz, sp.map_normals)
    g.set_reading(read, readn)
    before = [g.compute_resident(sp.T_init) for _ in range(3)]
    monkeypatch.setenv("O3S_FIRST_GRID", "0.15")
    assert g.init_reference(sp.map_xyz, sp.map_normals)
    g.set_reading(read, readn)
    again = []
    for _ in range(3):
        T = g.compute_resident(sp.T_init)
        n = g.stats.iterations
        again.append(dict(T=T, n=n, limit=g.stats.trace_limit[:n].copy(), kept=g.stats.trace_kept[:n].copy(),
                          trace_T=g.stats.trace_T[:n].copy(), issued=g.host_split_ex()["issued"]))
    g.close()
    fresh = run_calls(kw, sp.map_xyz, sp.map_normals, read, readn, sp.T_init)
    err = capfd.readouterr().err
    cells = [float(c[2]) for c in GRID_RE.findall(err)]
    assert cells == pytest.approx([0.061, 0.15, 0.15], abs=1e-4), err
    assert all(r["it0_index"] == "first" for r in parse_chain(err)), err
    assert [r["issued"] for r in again] == ["eager", "captured", "replayed"], [r["issued"] for r in again]
    check_three_calls(fresh, "fresh")
    for a, b in zip(again, fresh):
        assert_bit_identical(a, b, "re-initialised vs fresh")
    assert all(np.array_equal(T, fresh[0]["T"]) for T in before)   # exact search on either grid: the edge moves no bit


# ---- 3f: where the host looks at the chain's post ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def schedule_pair():
    """A small icp.yaml pair: 5 iterations from its initial guess, 7 from one 0.3 m further off, 3 from the truth."""
    sp = syn.make_scan_pair(4000, 12000, 0.1, seed=3)
    far = sp.T_init.copy()
    far[:3, 3] += 0.3
    return sp, {"init": sp.T_init, "far": far, "gt": sp.T_gt}


def expected_looks(kw, n, prev, issued):
    """The iterations issued at each look at the post of a call that ran n iterations on a handle whose previous call ran prev (4 on
    a fresh handle): a replayed graph goes out `chunk` iterations at a time until max_iters or more are out (5 for a chain that can
    stop by itself and has more than 7, else max_iters); an eager chain first as far as the previous call needed, clamped to
    [2, 8], then 2 at a time; a profiled one whole, or 16 at a time without a Counter checker."""
    mi = kw.get("max_iters", 15) or 0
    cap = mi if mi > 0 else 4096
    clamp = True
    if issued == "profiled":
        first = step = cap if mi > 0 else 16
    elif issued in ("captured", "replayed"):
        first = step = 5 if kw.get("use_differential", True) and mi > 7 else mi
        clamp = False   # whole replays: the iterations past max_iters are no-ops
    else:
        first, step = min(max(prev, 2), 8), 2
    k = min(first, cap)
    looks = [k]
    while k < n and k < cap:
        k = min(k + step, cap) if clamp else k + step
        looks.append(k)
    return looks


SCHEDULE_CASES = {   # config, the calls on one handle (initial guesses), how they are issued
    "eager": (dict(use_graph=False), ["init", "far", "gt", "far"], "resident"),
    "eager-split": (dict(use_graph=False), ["init", "far", "gt", "far"], "split"),
    "chunked-graph": (dict(), ["far", "far", "far", "init"], "resident"),
    "chunked-graph-split": (dict(), ["far", "far", "far", "init"], "split"),
    "fixed-graph": (dict(use_differential=False, max_iters=6), ["init", "init", "far"], "resident"),
    "profiled": (dict(), ["far", "init"], "profiled"),
    "profiled-no-counter": (dict(max_iters=0), ["far", "init"], "profiled"),
    "no-counter": (dict(max_iters=0), ["init", "far", "gt", "far"], "resident"),
}


@pytest.mark.parametrize("case", list(SCHEDULE_CASES))
def test_host_looks_at_the_post_where_the_schedule_says(case, monkeypatch, hooks_lib, capfd):
    """The O3S_PRINT_CHAIN report of every call lists the iterations issued at each look at the chain's post: they follow the
    schedule of csrc/o3s_icp.hip for eager calls on a fresh and on a warm handle (compute_resident and the two halves), captured
    and replayed chunked chains (one that needs a second chunk), a fixed-length graph, profiled calls and chains without a
    Counter checker."""
    kw, calls, how = SCHEDULE_CASES[case]
    sp, guesses = schedule_pair()
    monkeypatch.setenv("O3S_PRINT_CHAIN", "1")
    capfd.readouterr()
    g = ICP(IcpConfig(**kw))
    assert g.init_reference(sp.map_xyz, sp.map_normals)
    g.set_reading(sp.scan_xyz, sp.scan_normals)
    g.set_profiling(how == "profiled")
    iters = []
    for name in calls:
        if how == "split":
            g.compute_resident_launch(guesses[name])
            g.compute_resident_finish()
        else:
            g.compute_resident(guesses[name])
        iters.append(g.stats.iterations)
    g.close()
    reps = parse_chain(capfd.readouterr().err)
    assert len(reps) == len(calls), reps
    issued = [r["issued"] for r in reps]
    if how == "profiled":
        assert issued == ["profiled"] * len(calls), issued
    elif kw.get("use_graph", True) and kw.get("max_iters", 15):
        assert issued == ["eager", "captured", "replayed", "replayed"][:len(calls)], issued
    else:
        assert issued == ["eager"] * len(calls), issued
    looks = []
    for k, rep in enumerate(reps):
        prev = iters[k - 1] if k else 4
        want = expected_looks(kw, iters[k], prev, rep["issued"])
        looks.append(rep["looks"])
        assert rep["looks"] == ",".join(map(str, want)), (case, k, iters, rep)
    if case.startswith("chunked-graph"):
        assert iters[1] > 5 and looks[1] == looks[2] == "5,10", (iters, looks)   # a second chunk replays
    if case.startswith("eager"):
        assert len(looks[1].split(",")) > 1, looks   # the warm call looks more than once
