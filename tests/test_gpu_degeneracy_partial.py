"""Values for the partially localizable directions of the degeneracy-aware ICP step (include/degeneracy/o3s_degeneracy_partial.h)
on the GPU against the numpy restatement (tests/degeneracy_partial_ref.py).  MI355X only.

Bounds, from the contract and the number formats:
  num, den  every term is the same fp64 product on both sides (promoted fp32 values, the device's own directions, no FMA); the device
            adds them in another order than math.fsum: |delta| <= (K + 8) * 2^-53 * sum |terms|.  The strong set is the same when no
            contribution lies within 1e-9 of strong_min (asserted).
  A'        |delta| <= 64 * 2^-24 * max|A| against the restated projection of the device's own unconstrained A, b (the bound of
            tests/test_gpu_degeneracy.py).
  b'        |delta| <= 64 * 2^-24 * (max|b| + 7 max|A| max|d|): b' = P (b - A xc) + mu (C^T d): six entries of b, and six of A xc plus
            one mu, each at most max|A| max|d|.
  x         bit-equal to orc.solve6 on the device's own A', b'.
  C x = d   |e . x - d| <= max(8 x the restatement's own (solve6 on the restated A', b'), 4 * 2^-24 |x|).
  chain     the restatement is evaluated per iteration on the pairs under the DEVICE's own pose of that iteration (its trace), so
            that the sums' bound applies: d_j within that bound propagated through -num / den, with the directions of two eigen
            solvers 16 * 2^-52 apart at most (the eigen bound of tests/test_gpu_localizability.py).  Categories are decided by sums
            that stay 10 % away from every threshold (asserted on the restatement).  Pose: the 1e-4 m / 1e-4 rad of
            tests/test_gpu_parity.py against the restated chain.
Comparisons between two ways of issuing the same chain are bit for bit."""
import functools

import numpy as np
import pytest

import degeneracy_partial_ref as pref
import degeneracy_ref as dref
import localizability_ref as lref
from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig, _lib
from open3d_slam_advanced_rss_2024_public_amd import localizability as loc
from open3d_slam_advanced_rss_2024_public_amd.icp import compute_batch
from test_gpu_degeneracy import COV, FIXED_CHAIN, ITERS, NB_SIZES, SETS, assert_same_result, basis, bits, minimize_case, new_handle, restated
from test_gpu_localizability import EIG_C, SIZES, assert_same_snapshot, params_of, same_bits, snapshot
from test_gpu_parity import assert_pose_close

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
DIR_ERR = EIG_C * 2.0 ** -52


# ---- 1. the strong-pair sums at module level ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    return ICP(IcpConfig())


@functools.lru_cache(maxsize=None)
def module_case(scene, K):
    """Centred pairs of the scene with the matches a small seeded offset away, and thresholds in order."""
    p, n = lref.centred_pairs(scene, K, seed=K % 89)
    rng = np.random.default_rng(31 * K + len(scene))
    q = (p - rng.normal(0.0, 0.01, p.shape).astype(np.float32)).astype(np.float32)
    return p, q, n, (0.5 * K, 0.25 * K, 0.05 * K)


@pytest.mark.parametrize("K", SIZES)
@pytest.mark.parametrize("scene", ["room", "corridor", "tunnel"])
def test_partial_estimate_matches_the_restated_sums(handle, scene, K):
    p, q, n, ks = module_case(scene, K)
    got_loc, got = loc.partial_estimate(handle, p, q, n, params_of(ks))
    assert same_bits(got_loc, handle.estimate_localizability(p, n, params_of(ks)))
    con = lref.contributions(p, n, got_loc.evec)                  # the device's own directions
    gap = np.abs(con[np.isfinite(con)] - lref.KAPPA_S)
    assert gap.size == 0 or gap.min() > 1e-9, ("a contribution at strong_min", gap.min())
    want = pref.strong_sums(p, q, n, got_loc.evec, con)
    bn, bd = pref.sum_bounds(want, K)
    for j in range(6):
        dn, dd = abs(got.num[j] - want["num"][j]), abs(got.den[j] - want["den"][j])
        print(f"{scene} K {K} direction {j}: |dnum| {dn:.3e} (bound {bn[j]:.3e})  |dden| {dd:.3e} (bound {bd[j]:.3e})  value {got.value[j]:+.6e}")
        assert dn <= bn[j] and dd <= bd[j]
        assert got.value[j] == pref.quotient(got.num[j], got.den[j])
    assert np.array_equal(got.category, got_loc.category)
    assert got.partial_mask == sum(1 << j for j in range(6) if got_loc.category[j] == 1)
    assert got.constrained_mask == sum(1 << j for j in range(6) if got_loc.category[j] < 2)
    again_loc, again = loc.partial_estimate(handle, p, q, n, params_of(ks))
    assert same_bits(got_loc, again_loc)
    for f in ("num", "den", "value", "category"):
        assert np.array_equal(getattr(got, f), getattr(again, f)), f


def test_partial_estimate_statuses(handle):
    p, q, n, ks = module_case("room", 65)
    z = np.zeros((0, 3), np.float32)
    with pytest.raises(Exception) as e:
        loc.partial_estimate(handle, z, z, z, params_of(ks))
    assert f"[{_lib.ERR_NO_POINTS}]" in str(e.value)
    with pytest.raises(Exception) as e:
        loc.partial_estimate(handle, p, q, n, loc.LocalizabilityParams())
    assert f"[{_lib.ERR_BAD_CONFIG}]" in str(e.value)


# ---- 2. the algebra: k_constrain with the caller's values --------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,n", NB_SIZES)
@pytest.mark.parametrize("kind", ["generic", "corridor"])
def test_minimize_with_values_matches_the_restated_projection(kind, nb, n):
    g, inputs, (T0, A0, b0, x0) = minimize_case(kind, n)
    tolA = 64 * EPS32 * np.abs(A0).max()
    for k, (n_rot, n_trans) in enumerate(SETS):
        rot, trans = basis(100 * nb + k, n_rot), basis(200 * nb + k, n_trans)
        if kind == "corridor" and n_trans == 1:
            trans = np.array([[1.0, 0.0, 0.0]])                   # the axis nothing sees
        dset = loc.DegeneracySet(rot, trans)
        plain = g.minimize_degeneracy(*inputs, dset)
        rng = np.random.default_rng(1000 * nb + k)
        for label, rv, tv in (("seeded", rng.uniform(-0.05, 0.05, n_rot), rng.uniform(-0.05, 0.05, n_trans)), ("zeros", np.zeros(n_rot), np.zeros(n_trans))):
            T, A, b, x = g.minimize_degeneracy(*inputs, dset, values=(rv, tv))
            if label == "zeros" or n_rot + n_trans == 0:          # C x = 0, or the empty set: minimize_degeneracy's bits
                for got, want in zip((T, A, b, x), plain):
                    assert np.array_equal(bits(got), bits(want)), label
                continue
            d = np.concatenate([rv, tv])
            Ar, br = pref.project_values(A0, b0, rot, trans, d)
            tolb = 64 * EPS32 * (np.abs(b0).max() + 7 * np.abs(A0).max() * np.abs(d).max())
            dA, db = np.abs(A - Ar).max(), np.abs(b - br).max()
            x6, _ = orc.solve6(A, b)
            xr, _ = orc.solve6(Ar.astype(np.float32), br.astype(np.float32))
            leak, leak_ref = pref.value_leakage(x, rot, trans, d), pref.value_leakage(xr, rot, trans, d)
            bound = max(8.0 * leak_ref, 4 * EPS32 * float(np.linalg.norm(x)))
            print(f"{kind} nb {nb} N {n} set {n_rot}+{n_trans}: |dA| {dA:.3e} (tol {tolA:.3e})  |db| {db:.3e} (tol {tolb:.3e})  "
                  f"|e.x - d| {leak:.3e} (restatement {leak_ref:.3e}, bound {bound:.3e})")
            assert np.array_equal(bits(A), bits(A.T)) and np.array_equal(bits(A), bits(plain[1]))   # A' is the A' of C x = 0
            assert dA <= tolA and db <= tolb
            assert np.array_equal(bits(x), bits(x6)), (x, x6)
            assert leak <= bound
            again = g.minimize_degeneracy(*inputs, dset, values=(rv, tv))
            assert all(np.array_equal(bits(u), bits(v)) for u, v in zip((T, A, b, x), again))
        # o3s_icp_minimize_degen_values itself with NULL arrays: both NULL is o3s_icp_minimize_degeneracy, one NULL means zeros
        none = g.minimize_degeneracy(*inputs, dset, values=(None, None))
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(plain, none))
        rv, tv = rng.uniform(-0.05, 0.05, n_rot), rng.uniform(-0.05, 0.05, n_trans)
        for one_sided, explicit in (((None, tv), (np.zeros(n_rot), tv)), ((rv, None), (rv, np.zeros(n_trans)))):
            got, want = g.minimize_degeneracy(*inputs, dset, values=one_sided), g.minimize_degeneracy(*inputs, dset, values=explicit)
            assert all(np.array_equal(bits(u), bits(v)) for u, v in zip(got, want))
            if (one_sided[0] is None and n_trans) or (one_sided[1] is None and n_rot):     # the side that is given is applied
                assert not np.array_equal(bits(got[2]), bits(plain[2]))


def test_minimize_with_values_refuses_a_non_finite_value_with_the_handle():
    g, inputs, _ = minimize_case("generic", NB_SIZES[0][1])
    with pytest.raises(ValueError) as e:
        g.minimize_degeneracy(*inputs, loc.DegeneracySet(trans=np.array([[1.0, 0, 0]])), values=([], [float("nan")]))
    assert f"[{_lib.ERR_BAD_ARGUMENT}]" in str(e.value)


# ---- 3. the chain on the door scene --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def door():
    """The door pair, the oracle on its reference, thresholds from the restatement's first iteration."""
    pair = pref.door_pair()
    M, Mn, S, Sn, T_true, T_init = pair
    o = orc.OracleIcp(orc.OracleConfig(use_differential=False, max_iters=ITERS), threads=8)
    assert o.init_reference(M, Mn) == orc.OK
    prep = pref.prepare(orc, o, M, Mn, S, Sn, T_init)
    ks = pref.door_thresholds(pref.iteration(orc, o, prep, np.eye(4, dtype=np.float32), (1.0, 1.0, 1.0))["res"])
    return pair, o, prep, ks


def armed(pair, ks, min_category, partial, **cfg):
    g = new_handle(pair, **(cfg or FIXED_CHAIN))
    g.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks), min_category=min_category)
    if partial:
        g.set_degeneracy_partial(True)
    return g


@pytest.mark.parametrize("min_category", [1, 2])
def test_the_chain_constrains_the_partial_direction_to_its_strong_pairs(min_category):
    pair, o, prep, ks = door()
    M, Mn, S, Sn, T_true, T_init = pair
    ref = pref.constrained_chain(orc, o, M, Mn, S, Sn, T_init, ITERS, ks, min_category=min_category)
    g = armed(pair, ks, min_category, True)
    T = g.compute(S, Sn, T_init)
    assert g.stats.iterations == ITERS
    masks = g.degeneracy_trace()
    pmasks, values = g.degeneracy_partial_trace()
    assert masks.tolist() == ref["masks"] and pmasks.tolist() == ref["pmasks"] and values.shape == (ITERS, 6)
    for it in range(ITERS):                                        # the restatement on the device's own pose of the iteration
        T_prev = np.eye(4, dtype=np.float32) if it == 0 else g.stats.trace_T[it - 1]
        here = pref.iteration(orc, o, prep, T_prev, ks)
        margin = dref.threshold_margins(here["res"], ks)
        in_set, part, val = pref.iteration_set(here, min_category)
        assert margin >= 0.10 and here["res"]["category"].tolist() == [1, 2, 2, 2, 2, 2] == ref["analyses"][it]["category"].tolist()
        assert masks[it] == sum(1 << j for j in range(6) if in_set[j]) and pmasks[it] == sum(1 << j for j in range(6) if part[j])
        assert here["kept"] == g.stats.trace_kept[it]
        for j in range(6):
            bound = pref.value_bound(here["sums"], here["kept"], j, DIR_ERR) if part[j] else 0.0
            print(f"min_category {min_category} iteration {it} direction {j}: d {values[it, j]:+.9e}  restated {val[j]:+.9e}  "
                  f"|delta| {abs(values[it, j] - val[j]):.3e} (bound {bound:.3e})  margin {margin:.3f}")
            assert abs(values[it, j] - val[j]) <= bound
    on, last = g.last_degeneracy_partial()
    assert on and last.partial_mask == pmasks[-1] and last.constrained_mask == masks[-1] and last.category.tolist() == [1, 2, 2, 2, 2, 2]
    assert last.value[0] == values[-1, 0] and last.value[0] == pref.quotient(last.num[0], last.den[0]) and last.den[0] > 0
    assert_pose_close(T, ref["T"])
    # the property: the axis is found where the zero-constrained chain of the same handle cannot move
    g.set_degeneracy_partial(False)
    flag, stale = g.last_degeneracy_partial()                      # nothing computed since the flag was set: nothing to report
    assert not flag and stale.constrained_mask == 0 and not stale.den.any()
    g.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks), min_category=2)
    T_zero = g.compute(S, Sn, T_init)
    assert g.degeneracy_trace().tolist() == [1] * ITERS and len(g.degeneracy_partial_trace()[0]) == 0
    e, e_zero = pref.axis_error(T, T_true), pref.axis_error(T_zero, T_true)
    print(f"min_category {min_category}: axis error valued {1e3 * e:.3f} mm (restated {1e3 * pref.axis_error(ref['T'], T_true):.3f} mm)  "
          f"zero-constrained {1e3 * e_zero:.3f} mm")
    assert e <= 0.1 * e_zero


# ---- 4. what the flag leaves alone ----------------------------------------------------------------------------------------------------------
def test_in_the_room_the_flag_changes_nothing():
    pair, ks, free, ref = restated("room")
    assert ref["masks"] == [0] * ITERS
    T_init = pair[5]
    cfg = dict(error_minimizer=COV, **FIXED_CHAIN)
    off, on = armed(pair, ks, 2, False, **cfg), armed(pair, ks, 2, True, **cfg)
    want = snapshot(off, off.compute(*pair[2:4], T_init))
    assert_same_snapshot(want, snapshot(on, on.compute(*pair[2:4], T_init)))
    pmasks, values = on.degeneracy_partial_trace()
    assert np.array_equal(pmasks, np.zeros(ITERS, np.int32)) and not values.any() and np.array_equal(on.degeneracy_trace(), np.zeros(ITERS, np.int32))
    assert len(off.degeneracy_partial_trace()[0]) == 0
    flag, last = on.last_degeneracy_partial()
    assert flag and last.constrained_mask == 0 and not last.den.any()


def test_every_way_of_issuing_the_flagged_chain_gives_the_same_bits():
    pair, o, prep, ks = door()
    T_init = pair[5]
    cfg = dict(error_minimizer=COV, **FIXED_CHAIN)
    g = armed(pair, ks, 2, True, **cfg)
    want = snapshot(g, g.compute(*pair[2:4], T_init))             # eager
    masks, (pmasks, values) = g.degeneracy_trace(), g.degeneracy_partial_trace()
    assert pmasks.tolist() == [1] * ITERS
    # o3s_icp_localizability behind the flagged compute: the last iteration's analysis, the bits the chain used
    after = g.localizability(params_of(ks))
    assert after.category.tolist() == [1, 2, 2, 2, 2, 2] and same_bits(after, g.localizability(params_of(ks)))
    last_set = g.last_degeneracy_set()
    assert np.array_equal(last_set.trans, after.evec[:1]) and len(last_set.rot) == 0
    assert g.last_degeneracy_partial()[1].value[0] == values[-1, 0]
    g.set_reading(*pair[2:4])
    for round_ in range(3):                                        # captured, then replayed
        assert_same_snapshot(want, snapshot(g, g.compute_resident(T_init)))
        pm, v = g.degeneracy_partial_trace()
        assert np.array_equal(g.degeneracy_trace(), masks) and np.array_equal(pm, pmasks) and np.array_equal(v, values)
    assert g.host_split_ex()["issued"] == "replayed"
    p = armed(pair, ks, 2, True, **cfg)                            # profiled
    p.set_profiling(True)
    assert_same_snapshot(want, snapshot(p, p.compute(*pair[2:4], T_init)))
    assert np.array_equal(p.degeneracy_partial_trace()[1], values)
    others = [armed(pair, ks, 2, True, **cfg) for _ in range(2)]   # o3s_icp_compute_batch
    poses, codes, _ = compute_batch(others, [T_init, T_init])
    assert codes == [0, 0]
    for h, T in zip(others, poses):
        assert_same_result(want, snapshot(h, T))
        assert np.array_equal(h.degeneracy_partial_trace()[1], values) and np.array_equal(h.degeneracy_trace(), masks)


def test_flag_off_after_on_gives_the_unflagged_bits_again():
    pair, o, prep, ks = door()
    T_init = pair[5]
    g = armed(pair, ks, 2, False, error_minimizer=COV, **FIXED_CHAIN)
    off = [snapshot(g, g.compute_resident(T_init)) for _ in range(3)]            # eager, captured, replayed
    assert g.host_split_ex()["issued"] == "replayed"
    g.set_degeneracy_partial(True)
    on = [snapshot(g, g.compute_resident(T_init)) for _ in range(3)]
    assert g.host_split_ex()["issued"] == "replayed" and g.degeneracy_partial_trace()[0].tolist() == [1] * ITERS
    g.set_degeneracy_partial(False)
    back = [snapshot(g, g.compute_resident(T_init)) for _ in range(3)]
    assert g.host_split_ex()["issued"] == "replayed" and len(g.degeneracy_partial_trace()[0]) == 0
    for s in off[1:] + back:
        assert_same_snapshot(off[0], s)
    for s in on[1:]:
        assert_same_snapshot(on[0], s)
    assert not np.array_equal(on[0]["T"], off[0]["T"])
    fixed = new_handle(pair, **FIXED_CHAIN)                                       # FIXED ignores the flag
    fixed.set_degeneracy(loc.DEGENERACY_FIXED, fixed_set=loc.DegeneracySet(trans=np.array([[1.0, 0, 0]])))
    a = fixed.compute(*pair[2:4], T_init)
    fixed.set_degeneracy_partial(True)
    assert np.array_equal(a, fixed.compute(*pair[2:4], T_init)) and len(fixed.degeneracy_partial_trace()[0]) == 0
