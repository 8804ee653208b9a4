"""The trim limit resolved in k_classify from the previous iteration's limit (k_match2 counts the next digits of the pairs that
share its 11 / 21 leading bits): the limit stays the exact order statistic, whatever the previous limit predicted, and every path
of the chain gives the bits it gave with the level-1 selection alone (O3S_NO_SPEC_SELECT=1, hooks build)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def sel_depth(L, g):
    """Leading bits of the limit k_classify resolved in each iteration of g's last call (32, 21, 11; 0: no speculation)."""
    n = g.stats.iterations
    out = np.zeros(max(n, 1), np.int32)
    got = L.o3s_icp_hook_sel_depth(g._h, out.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(n))
    assert got == n
    return out[:n]


def run(sp, cfg, calls=1, resident=False):
    g = ICP(IcpConfig(**cfg))
    assert g.init_reference(sp.map_xyz, sp.map_normals)
    if resident:
        g.set_reading(sp.scan_xyz, sp.scan_normals)
        Ts = [g.compute_resident(sp.T_init) for _ in range(calls)]
        assert all(np.array_equal(Ts[0], T) for T in Ts[1:])
        T = Ts[0]
    else:
        T = g.compute(sp.scan_xyz, sp.scan_normals, sp.T_init)
    return g, (T, g.stats.iterations, g.stats.trace_limit.view(np.uint32).copy(), g.stats.trace_kept.copy())


def oracle_run(sp, cfg):
    o = orc.OracleIcp(orc.OracleConfig(**cfg), threads=16)
    assert o.init_reference(sp.map_xyz, sp.map_normals) == orc.OK
    o.compute(sp.scan_xyz, sp.scan_normals, sp.T_init)
    return o


def assert_same(a, b):
    assert a[1] == b[1]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.timeout(600)
def test_bench_pair_resolves_the_limit_and_changes_no_bit(monkeypatch, hooks_lib):
    """The bench pair (C2, 50 fixed iterations): the limit is resolved in k_classify in almost every iteration after the first
    (the oracle's limits keep their 21-bit prefix from iteration 4 on), and limits, kept counts, iterations and the pose are those
    of the level-1 selection and of the oracle."""
    sp = syn.make_scan_pair(100_000, 2_000_000, 0.1, seed=0)
    cfg = dict(use_differential=False, max_iters=50)
    g, on = run(sp, cfg, calls=3, resident=True)  # eager, captured, replayed
    depth = sel_depth(hooks_lib, g)
    assert depth[0] == 11  # no previous limit in the first iteration
    assert np.count_nonzero(depth[1:] == 32) >= 40, depth
    monkeypatch.setenv("O3S_NO_SPEC_SELECT", "1")
    g2, off = run(sp, cfg, calls=3, resident=True)
    assert np.all(sel_depth(hooks_lib, g2) == 0)
    assert_same(on, off)
    o = oracle_run(sp, cfg)
    assert np.array_equal(on[2], o.trace_limit.view(np.uint32)) and np.array_equal(on[3], o.trace_kept)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("seed,offset", [(5, 0.1), (6, 0.3), (7, 0.5)])
def test_limits_that_change_bins_and_ties_at_the_limit_stay_exact(monkeypatch, hooks_lib, seed, offset):
    """Pairs whose limit leaves the previous limit's level-1 bin between iterations (larger initial offsets), with every tenth
    reading point duplicated (ties at the limit): limits and kept counts bit-exact against the oracle, and the same bits as the
    level-1 selection."""
    sp = syn.make_scan_pair(20_000, 200_000, offset, seed=seed)
    dup = np.arange(0, len(sp.scan_xyz), 10)
    sp.scan_xyz = np.concatenate([sp.scan_xyz, sp.scan_xyz[dup]])
    sp.scan_normals = np.concatenate([sp.scan_normals, sp.scan_normals[dup]])
    cfg = dict(max_dist=0.5, trim_ratio=0.9, max_normal_angle=1.57, use_differential=False, max_iters=15)
    o = oracle_run(sp, cfg)
    ol = o.trace_limit.view(np.uint32)
    assert np.any((ol[1:] >> 20) != (ol[:-1] >> 20)), ol  # the limit crosses a level-1 bin at least once
    g, on = run(sp, cfg)
    assert np.array_equal(on[2], ol) and np.array_equal(on[3], o.trace_kept)
    depth = sel_depth(hooks_lib, g)
    same11 = np.concatenate([[False], (ol[1:] >> 20) == (ol[:-1] >> 20)])
    assert np.all(depth[~same11] == 11), (depth, ol)  # the first iteration, and a bin change: level 1 only
    monkeypatch.setenv("O3S_NO_SPEC_SELECT", "1")
    _, off = run(sp, cfg)
    assert_same(on, off)


@pytest.mark.timeout(600)
def test_a_call_that_stops_early_leaves_nothing_for_the_next_one():
    """A call stopped early by the Differential checker, then a longer call on the same handle (a start further away), eagerly
    issued and replayed: the second call gives the bits of a fresh handle that never ran the first."""
    sp = syn.make_scan_pair(30_000, 300_000, 0.1, seed=11)
    cfg = IcpConfig(max_iters=50)  # icp.yaml's chain, 50 iterations at most
    c, s_ = np.cos(0.06), np.sin(0.06)
    T_far = sp.T_init @ np.array([[c, -s_, 0, 0.25], [s_, c, 0, -0.2], [0, 0, 1, 0.05], [0, 0, 0, 1]], np.float32)
    for resident in (False, True):
        def go(h, T):
            if resident:
                Ts = [h.compute_resident(T) for _ in range(3)]  # eager, captured, replayed
                assert all(np.array_equal(Ts[0], X) for X in Ts[1:])
                return Ts[0]
            return h.compute(sp.scan_xyz, sp.scan_normals, T)
        handles = []
        for _ in range(2):
            h = ICP(cfg)
            assert h.init_reference(sp.map_xyz, sp.map_normals)
            if resident:
                h.set_reading(sp.scan_xyz, sp.scan_normals)
            handles.append(h)
        used, fresh = handles
        go(used, sp.T_init)
        n_short = used.stats.iterations
        assert n_short < 50
        T_used = go(used, T_far)
        T_fresh = go(fresh, T_far)
        assert used.stats.iterations > n_short
        assert_same((T_used, used.stats.iterations, used.stats.trace_limit.view(np.uint32).copy(), used.stats.trace_kept.copy()),
                    (T_fresh, fresh.stats.iterations, fresh.stats.trace_limit.view(np.uint32).copy(), fresh.stats.trace_kept.copy()))


@pytest.mark.timeout(900)
def test_every_path_gives_the_bits_of_the_level1_selection(monkeypatch, hooks_lib):
    """Fused and two-kernel chains (O3S_FUSE), the multi-block sweep of large readings (O3S_SEL_PARTIAL) and
    o3s_icp_compute_batch against single calls: the same limits, kept counts, iterations and poses with and without the
    speculation, eager and replayed."""
    from open3d_slam_advanced_rss_2024_public_amd import compute_batch

    cfg = dict(use_differential=False, max_iters=12)
    sp = syn.make_scan_pair(30_000, 200_000, 0.1, seed=31)
    ref = None
    for fuse in ("1", "0"):
        for no_spec in ("0", "1"):
            monkeypatch.setenv("O3S_FUSE", fuse)
            monkeypatch.setenv("O3S_NO_SPEC_SELECT", no_spec)
            g, out = run(sp, cfg, calls=3, resident=True)
            if no_spec == "0":
                assert np.count_nonzero(sel_depth(hooks_lib, g)[1:] == 32) > 0
            ref = out if ref is None else ref
            assert_same(out, ref)
    monkeypatch.setenv("O3S_FUSE", "1")
    pairs = [syn.make_scan_pair(6000, 40000, 0.1, seed=50 + k) for k in range(4)]
    for no_spec in ("0", "1"):
        monkeypatch.setenv("O3S_NO_SPEC_SELECT", no_spec)
        icps, solo = [], []
        for p in pairs:
            icp = ICP(IcpConfig(**cfg))
            icp.init_reference(p.map_xyz, p.map_normals)
            icp.set_reading(p.scan_xyz, p.scan_normals)
            icps.append(icp)
            solo.append(run(p, cfg)[1])
        poses, codes, stats = compute_batch(icps, [p.T_init for p in pairs])
        for k in range(len(pairs)):
            assert codes[k] == 0 and np.array_equal(poses[k], solo[k][0]) and stats[k].iterations == solo[k][1]
        if no_spec == "0":
            spec_solo = solo
        else:
            for a, b in zip(spec_solo, solo):
                assert_same(a, b)
    big = syn.make_scan_pair(270_000, 600_000, 0.05, seed=41)  # 528 classify blocks: the multi-block sweep (k_sel_partial)
    cfg8 = dict(use_differential=False, max_iters=8)
    ref = None
    for part in ("1", "0"):
        for no_spec in ("0", "1"):
            monkeypatch.setenv("O3S_SEL_PARTIAL", part)
            monkeypatch.setenv("O3S_NO_SPEC_SELECT", no_spec)
            g, out = run(big, cfg8, calls=3, resident=True)
            if ref is None:
                ref = out
            assert np.array_equal(out[2], ref[2]) and np.array_equal(out[3], ref[3]) and out[1] == ref[1]
            if part == "1":
                assert np.array_equal(out[0], ref[0])  # same path, with and without the speculation: the same pose bits
            else:
                assert np.abs(out[0] - ref[0]).max() <= 1e-6  # the single-block sweep folds its sums in another fixed order
