"""CPU-only: the numpy restatement of the partial-direction treatment (tests/degeneracy_partial_ref.py,
include/degeneracy/o3s_degeneracy_partial.h) on its own: the projection onto C x = d against the null-space method, and the
restated chain on the "door" scene — a corridor whose axis only a small panel sees — against the oracle's module calls.

Bounds: the solve is fp32 (orc.solve6), so e_j . x holds d_j to a few fp32 roundings of |x|: 4 * 2^-24 |x|, the floor the GPU tests
give the device.  The chain's categories are decided by sums that stay 10 % away from every threshold (the rule of
tests/test_gpu_degeneracy.py)."""
import functools

import numpy as np
import pytest

import degeneracy_partial_ref as pref
import degeneracy_ref as dref
import localizability_ref as lref
from oracle import oracle as orc
from test_degeneracy_ref import normal_equations

EPS32 = 2.0 ** -24
ITERS = 6


# ---- the projection ------------------------------------------------------------------------------------------------------------------------
def test_zero_values_give_the_bits_of_the_zero_constraint():
    A, b = normal_equations("corridor")
    q = np.linalg.qr(np.random.default_rng(3).normal(size=(3, 3)))[0].T
    for rot, trans in (([], q[:1]), (q[:2], q[1:]), (q, q)):
        Ap, bp = dref.project(A, b, rot, trans)
        Av, bv = pref.project_values(A, b, rot, trans, np.zeros(len(rot) + len(trans)))
        assert np.array_equal(Av, Ap) and np.array_equal(bv, bp)


def test_the_empty_set_returns_the_input():
    A, b = normal_equations("room")
    Ap, bp = pref.project_values(A, b, [], [], [])
    assert np.array_equal(Ap, A) and np.array_equal(bp, b)


@pytest.mark.parametrize("n_rot,n_trans", [(0, 1), (1, 0), (1, 1), (2, 3), (3, 3)])
def test_values_are_held_and_the_rest_minimises_the_same_quadratic(n_rot, n_trans):
    A, b = normal_equations("room")
    rng = np.random.default_rng(10 * n_rot + n_trans)
    rot = np.linalg.qr(rng.normal(size=(3, 3)))[0].T[:n_rot]
    trans = np.linalg.qr(rng.normal(size=(3, 3)))[0].T[:n_trans]
    d = rng.uniform(-0.05, 0.05, n_rot + n_trans)
    Ap, bp = pref.project_values(A, b, rot, trans, d)
    assert np.array_equal(Ap, dref.project(A, b, rot, trans)[0])
    x = np.linalg.solve(Ap, bp)
    assert pref.value_leakage(x, rot, trans, d) <= 1e-12 * max(np.linalg.norm(x), np.abs(d).max())
    # the minimiser of 1/2 x^T A x - b^T x over C x = d, by the null-space method
    C, _ = dref.rows_of(rot, trans)
    xc = C.T @ d
    if len(C) < 6:
        Z = np.linalg.svd(C)[2][len(C):].T
        want = xc + Z @ np.linalg.solve(Z.T @ A @ Z, Z.T @ (b - A @ xc))
    else:
        want = xc
    assert np.allclose(x, want, rtol=1e-8, atol=1e-12)


def test_the_quotient_is_zero_where_it_means_nothing():
    assert pref.quotient(1.0, 0.0) == 0.0 and pref.quotient(0.0, 0.0) == 0.0
    assert pref.quotient(float("inf"), 1.0) == 0.0 and pref.quotient(float("nan"), 1.0) == 0.0 and pref.quotient(1e300, 1e-300) == 0.0
    assert pref.quotient(3.0, 2.0) == -1.5 and pref.quotient(-0.0, 2.0) == 0.0


def test_strong_sums_recover_a_shift_along_a_direction_only_strong_pairs_see():
    """Pairs whose reading sits `shift` off its matches: along a direction the strong pairs see squarely, -num / den is the step
    that takes the shift back."""
    p, n = lref.centred_pairs("room", 2000)
    shift = np.float32([0.02, -0.01, 0.015])
    q = (p - shift).astype(np.float32)
    res = lref.analyse(p, n, 1.0, 1.0, 1.0)
    sums = pref.strong_sums(p, q, n, res["evec"], res["contrib"])
    for j in range(3):
        want = -float(res["evec"][j] @ shift.astype(np.float64))
        assert abs(sums["value"][j] - want) <= 2e-3 * np.linalg.norm(shift), (j, sums["value"][j], want)   # (the normals' 1e-3 rad jitter)
    assert (sums["den"][:3] > 0).all() and (sums["abs_num"] >= np.abs(sums["num"])).all()
    for j in range(6):                                             # a direction no strong pair sees: den 0, value 0
        if res["n_strong"][j] == 0:
            assert sums["den"][j] == 0.0 and sums["value"][j] == 0.0


# ---- the chain on the door scene ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def door_case():
    pair = pref.door_pair()
    M, Mn, S, Sn, T_true, T_init = pair
    o = orc.OracleIcp(orc.OracleConfig(use_differential=False, max_iters=ITERS), threads=8)
    assert o.init_reference(M, Mn) == orc.OK
    first = pref.constrained_chain(orc, o, M, Mn, S, Sn, T_init, 1, ks=(1.0, 1.0, 1.0))["analyses"][0]
    ks = pref.door_thresholds(first)
    valued = {mc: pref.constrained_chain(orc, o, M, Mn, S, Sn, T_init, ITERS, ks, min_category=mc) for mc in (1, 2)}
    zero = pref.constrained_chain(orc, o, M, Mn, S, Sn, T_init, ITERS, ks, min_category=2, partial=False)
    plain = dref.constrained_chain(orc, o, M, Mn, S, Sn, T_init, ITERS, ks=ks, min_category=2)
    return pair, ks, valued, zero, plain


def test_the_door_scene_decides_its_categories_with_a_margin():
    pair, ks, valued, zero, plain = door_case()
    assert len(pair[2]) == 3000 and len(pair[0]) == 12000
    print("thresholds", ks)
    assert ks[0] == ks[1] and ks[2] < ks[1]
    # the scene's figures: 60 panel points of the reading, each a contribution of about 1 along the axis (k3 = a quarter of their sum),
    # and k1 = half the smallest sum_all of the five other directions; a scene that drifts shows here before it reaches a threshold
    assert abs(ks[2] - 15.0) <= 0.05 and abs(ks[0] - 84.4) <= 0.5, ks
    for mc, ref in valued.items():
        for it, res in enumerate(ref["analyses"]):
            margin = dref.threshold_margins(res, ks)
            print(f"min_category {mc} iteration {it}: margin {margin:.3f}  categories {res['category']}  value {ref['values'][it][0]:+.6f}")
            assert margin >= 0.10, (it, margin)                   # the rule of the chain tests ...
            assert margin >= 0.28, (it, margin)                   # ... and what this scene has: 28.9 % (sum_strong[0] = 4 k3 against k2 = k1)
            assert res["category"].tolist() == [1, 2, 2, 2, 2, 2]
            assert abs(res["evec"][0][0]) > 0.999                 # direction 0 is the corridor's axis
        assert ref["masks"] == [1] * ITERS and ref["pmasks"] == [1] * ITERS


def test_the_restated_solve_holds_the_value_at_the_leakage_level():
    pair, ks, valued, zero, plain = door_case()
    for mc, ref in valued.items():
        for it, leak in enumerate(ref["leaks"]):
            scale = max(abs(ref["values"][it][0]), 1e-3)          # |x| >= |d_0|; millimetres at the least in this scene
            print(f"min_category {mc} iteration {it}: |e.x - d| {leak:.3e}  (d {ref['values'][it][0]:+.3e})")
            assert leak <= 4 * EPS32 * scale


def test_the_valued_chain_finds_the_axis_the_zero_constrained_chain_cannot():
    pair, ks, valued, zero, plain = door_case()
    T_true = pair[4]
    assert np.array_equal(zero["T"], plain["T"]) and zero["masks"] == plain["masks"]    # partial=False is degeneracy_ref's chain
    e_zero = pref.axis_error(zero["T"], T_true)
    for mc, ref in valued.items():
        e = pref.axis_error(ref["T"], T_true)
        print(f"min_category {mc}: axis error valued {1e3 * e:.3f} mm  zero-constrained {1e3 * e_zero:.3f} mm")
        assert e <= 0.1 * e_zero
    assert e_zero > 0.02                                           # it cannot move along x: most of the 30 mm stay
