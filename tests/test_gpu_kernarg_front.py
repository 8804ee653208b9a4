"""Every launch site of the kernels whose parameters were reordered for kernarg preloading, at sizes that
run in seconds, against the oracle.

The chain kernels take what their first round trip reads through as their leading arguments (they arrive in SGPRs at wave launch)
and by-value structs last; the reading's six arrays and its normals go in as one base each.  Several neighbouring parameters have
the same type (mq / mn, pos / d2 / cert, hist_rep / hist2 / spec), so a swap at a launch site compiles: what catches it is a result.
Every case is held to the contract of test_gpu_dispatch_boundaries.py with that file's own helpers (status, iteration count and
per-iteration kept counts equal to the oracle's; trim limits bit-equal or within 1e-5 relative; pose within 1e-5 m / 1e-5 rad; eager,
captured and replayed calls bit-identical).

Launch sites and the case that reaches them (csrc/o3s_icp.hip):
  launch_match2 (row-disc and ring search; first iteration, certificates, settle front), launch_iteration's k_classify, k_sel_ne and
  k_solve                                          the fused chain, eager / captured / replayed; no reading normals (rn null); no sort
  launch_iteration's k_sel_finish + k_normal_eq + k_solve      compute_batch (the two-kernel chain), and O3S_FUSE=0 on the hooks build
  k_match_mirror + k_classify with the gate folded into `mode`   MirrorMatcher with and without the normal gate
  a chunked replay (iteration 0 of a second chunk)             the Differential checker from a far initial guess

Not reached at these sizes, and where they are:
  k_sel_partial needs more than 512 classify blocks, N >= 262 145 (O3S_SEL_PARTIAL can only switch it off): the nominal-262145 and
  dense-262145 cases of test_gpu_dispatch_boundaries.py run it against the oracle.
  The sharded chain's k_classify launch: test_gpu_sharded.py has no fixture to import (its world-1 case builds its handles inline),
  and the sharded chain is not bit-comparable with the oracle; test_world1_noop_exchange_equals_unsharded_chain covers that site.
  The module-level launch sites (o3s_icp_outlier_weights, o3s_icp_minimize): test_gpu_parity.py's module tests."""
import functools

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig, compute_batch
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn
from test_gpu_dispatch_boundaries import (INF, assert_agrees_with_oracle, assert_bit_identical, check_three_calls, run_calls, run_oracle,
                                          schedule_pair)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def pair():
    """3 000 / 20 000: one k_sel_ne launch of 6 blocks, 4 lanes per query, 12 classify blocks, odd tails in every kernel's last block."""
    return syn.make_scan_pair(3000, 20000, 0.1, seed=11)


def inputs(sp, normals=True):
    return sp.map_xyz, sp.map_normals, sp.scan_xyz, sp.scan_normals if normals else None, sp.T_init


@functools.lru_cache(maxsize=None)
def oracle_of(key):
    """The oracle's run of a named case, computed once and shared."""
    kw, data = CASES[key]()
    return run_oracle(kw, *data)


CASES = {
    "fused": lambda: (dict(use_graph=True), inputs(pair())),
    "no-reading-normals": lambda: (dict(use_graph=True), inputs(pair(), normals=False)),
    "no-sort": lambda: (dict(use_graph=True, sort_queries=False), inputs(pair())),
    "ring-search": lambda: (dict(use_graph=True, max_dist=INF), inputs(pair())),
    "outlier-notrim": lambda: (dict(use_graph=True, trim_ratio=None, max_dist_outlier=0.3), inputs(pair())),
    "normal-gate": lambda: (dict(use_graph=True, max_normal_angle=1.0), inputs(pair())),
}


@pytest.mark.parametrize("key", list(CASES))
def test_fused_chain_eager_captured_and_replayed_agrees_with_the_oracle(key):
    """The same pair three times on one handle: the second call captures the graph and the third replays it.  The fused chain
    (k_match2 of the first iteration, with certificates and the settle front; k_classify; k_sel_ne; k_solve) with the reading's
    normals and without, unsorted, on the ring search, without a trim (no speculative words: spec null), and with the normal gate
    (kModeGate in `mode`)."""
    kw, data = CASES[key]()
    out = run_calls(kw, *data)
    o, To, code = oracle_of(key)
    assert_agrees_with_oracle(out[0], o, To, code, key)
    check_three_calls(out, key)
    assert out[0]["n"] >= 3, key   # launches 0, 1 and at least one with the settle front


def test_two_kernel_chain_of_a_batch_gives_the_single_calls_bytes():
    """o3s_icp_compute_batch runs k_sel_finish + k_normal_eq instead of k_sel_ne: two handles in one batch give, byte for byte, the
    poses of the single calls, which agree with the oracle."""
    kw, data = CASES["fused"]()
    sp = pair()
    single = run_calls(kw, *data, calls=1)[0]
    o, To, code = oracle_of("fused")
    assert_agrees_with_oracle(single, o, To, code, "single")
    hs = []
    for _ in range(2):
        g = ICP(IcpConfig(**kw))
        assert g.init_reference(sp.map_xyz, sp.map_normals)
        g.set_reading(sp.scan_xyz, sp.scan_normals)
        hs.append(g)
    poses, codes, _ = compute_batch(hs, [sp.T_init, sp.T_init])
    assert list(codes) == [0, 0]
    for T in poses:
        assert np.array_equal(T, single["T"])
    for g in hs:
        g.close()


def test_two_kernel_chain_on_the_hooks_build_gives_the_fused_bits(monkeypatch, hooks_lib):
    """O3S_FUSE=0 forces k_sel_finish + k_normal_eq at 3 000 points on the hooks build (whose kernels take their two extra
    arguments behind the reordered ones): the bits of its own fused chain, eager, captured and replayed, and the oracle's result.
    (k_sel_partial cannot be forced at this size: see the module's docstring.)"""
    kw, data = CASES["fused"]()
    o, To, code = oracle_of("fused")
    res = {}
    for fuse in ("1", "0"):
        monkeypatch.setenv("O3S_FUSE", fuse)
        out = run_calls(kw, *data)
        assert_agrees_with_oracle(out[0], o, To, code, fuse)
        check_three_calls(out, fuse)
        res[fuse] = out[0]
    assert_bit_identical(res["1"], res["0"], "fused vs two kernels")


@functools.lru_cache(maxsize=None)
def mirror_case():
    """2 000 / 2 000: reading point i is reference point i under a small rigid motion, plus noise."""
    rng = np.random.default_rng(7)
    sp = syn.make_scan_pair(500, 6000, 0.1, seed=13)
    ref, refn = sp.map_xyz[:2000], sp.map_normals[:2000]
    assert len(ref) == 2000
    T_gt = syn.make_T(syn.rot_axis_angle(rng.normal(size=3), np.radians(3.0)), rng.uniform(-0.2, 0.2, 3))
    read, readn = syn.transform_cloud(np.linalg.inv(T_gt), ref.astype(np.float64), refn.astype(np.float64))
    read = (read + rng.normal(0, 0.003, read.shape)).astype(np.float32)
    return ref, refn, read, readn.astype(np.float32), np.eye(4)


@pytest.mark.parametrize("gate", [False, True], ids=["nogate", "gate"])
def test_mirror_chain_agrees_with_the_oracle(gate):
    """MirrorMatcher, 2 000 / 2 000: k_match_mirror in front of the reordered k_classify (no speculative words, max_r2 = inf), with
    and without the SurfaceNormalOutlierFilter, whose flag now travels in `mode`."""
    kw = dict(matcher="MirrorMatcher", max_dist=1.0, trim_ratio=0.9, max_normal_angle=1.57 if gate else None, use_differential=True,
              min_diff_rot=1e-5, min_diff_trans=1e-4, smooth_length=3, max_iters=30, use_graph=True)
    data = mirror_case()
    out = run_calls(kw, *data)
    o, To, code = run_oracle(kw, *data)
    assert_agrees_with_oracle(out[0], o, To, code, gate)
    check_three_calls(out, gate)


def test_differential_chain_replays_a_second_chunk():
    """The icp.yaml chain (Differential checker) from a guess 0.3 m off: 7 iterations, so the replayed graph goes out in two
    chunks of five and iteration 0's kernels (no certificates, first-iteration lanes) are not what launch 5 runs."""
    sp, guesses = schedule_pair()
    kw = dict(use_differential=True, max_iters=15, use_graph=True)
    data = (sp.map_xyz, sp.map_normals, sp.scan_xyz, sp.scan_normals, guesses["far"])
    out = run_calls(kw, *data)
    o, To, code = run_oracle(kw, *data)
    assert_agrees_with_oracle(out[0], o, To, code, "far")
    assert out[0]["n"] > 5
    check_three_calls(out, "far")
