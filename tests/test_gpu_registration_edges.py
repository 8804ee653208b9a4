"""The loop-closure registration (include/o3s_registration.h, csrc/o3d_icp_impl.h) where its other tests never take it: one to a
thousand points per cloud, degenerate geometry, the branches of k_o3d_cov.  MI355X only; staged, so that one stage's slack cannot hide
the next stage's error — every stage judges the device's output against a reference fed with the previous stage's DEVICE output:

  1  correspondences of the first pass (o3s_test_o3d_first_pass, hooks build) against exact nearest neighbours on lattice scenes;
  2  k_o3d_cov against covariance_mp, entry by entry, and which triangle of a caller's covariance is read;
  3  the 30 sums against first_pass_sums over the device's correspondences and covariances: |sum_dev - sum_ref| <= B_k;
  4  the host update (o3s_test_o3d_update) made of the device's sums, under the contract of tests/test_o3d_update_host.py;
  5  one iteration end to end on the degenerate scenes;  6  full ICP at tiny sizes;  7  bystanders, repeatability, work-area reuse;
  and the resident path on two tiny submaps.

The judges and the scenes are tests/o3d_solve_ref.py (pinned on the CPU by tests/test_o3d_solve_ref.py, where every scene used
here is shown to have no nearest-neighbour tie and no pair at the radius).

Measured on an MI355X (printed with -s):
  stage 2, largest |C_dev - C_mp| / bound: 0.12.
  stage 3, largest |sum_dev - sum_ref| / B_k over the cases: point-to-plane 0.16, point-to-point 0.0 (lattice coordinates and a
    dyadic shift: the device's sums are exact), GICP 2.6e-3 (the per-term part of B_k is a worst case of the cofactor inverse).
  stage 5, sum of squared residuals above the linearised optimum, restatement / device, of 2.0e-2 before: tilted plane 3.6e-9 /
    1.4e-11, corridor -3.5e-18 / -3.5e-18, cylinder (optimum 1.98e-2) -2.9e-7 / -1.9e-6.
  stage 6, largest |T_dev - T_ref|: point-to-plane 2.2e-16, point-to-point 1.3e-15, GICP 2.2e-16.
  The file runs in 11 s.

Seeded one at a time into a scratch copy, these turn the following red: h_ldlt_solve6 without its in-between swap loop, and its
pseudo-inverse dividing instead of zeroing: the LDLT tests of tests/test_o3d_update_host.py (on the CPU); h_umeyama without
the det U det V sign: the reflected and the rank <= 2 cases of test_umeyama there; the source covariance read without the pose's
rotation: stage 3 (GICP, every case under the quarter turn); `c <= -0.99` in k_o3d_cov: stage 2; the hook returning the
correspondences in search order: stage 1; k_o3d_fold's lane loop started at l + 1: stages 1 and 3 (the count itself is wrong)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import registration as reg

import o3d_registration_ref as oref
import o3d_solve_ref as sr
from test_o3d_update_host import VEC6_BOUND, check_umeyama, lib_update, rel

pytestmark = pytest.mark.gpu

U = sr.U
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def first_pass(L, kind, src, tgt, max_dist, init=None, src_n=None, tgt_n=None, src_cov=None, tgt_cov=None, eps=1e-3):
    """o3s_test_o3d_first_pass -> dict(sums, corr by source index, scov / tcov by point index as 3 x 3, shift)"""
    f = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    s_, t_, sn, tn, sc, tc = f(src), f(tgt), f(src_n), f(tgt_n), f(src_cov), f(tgt_cov)
    ns, nt = len(s_), len(t_)
    sums, corr = np.full(30, np.nan), np.full(ns, -9, np.int32)
    scov, tcov, shift = np.full((ns, 6), np.nan), np.full((nt, 6), np.nan), np.full(3, np.nan)
    est = reg._Estimation(sr.TYPE_ID[kind], eps)
    rc = L.o3s_test_o3d_first_pass(0, _dp(s_), _dp(sn), _dp(sc), ns, _dp(t_), _dp(tn), _dp(tc), nt, float(max_dist),
                                   _dp(reg._pose(np.eye(4) if init is None else init)), C.byref(est), _dp(sums),
                                   corr.ctypes.data_as(C.POINTER(C.c_int32)), _dp(scov), _dp(tcov), _dp(shift))
    assert rc == 0, rc
    unpack = lambda c6: c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    return {"sums": sums, "corr": corr, "scov": unpack(scov), "tcov": unpack(tcov), "shift": shift}


def scene_args(kind, sc):
    if kind == "PointToPlaneIcp":
        return dict(tgt_n=sc["tgt_n"])
    if kind == "GeneralizedIcp":
        return dict(src_n=sc["src_n"], tgt_n=sc["tgt_n"])
    return {}


_FP = {}


def edge_first_pass(L, case, kind):
    """the device's first pass on one of the lattice scenes, once per process"""
    if (case, kind) not in _FP:
        sc = sr.edge_case(*case)
        _FP[(case, kind)] = first_pass(L, kind, sc["src"], sc["tgt"], sc["max_dist"], sc["init"], **scene_args(kind, sc))
    return _FP[(case, kind)]


_ids = lambda c: "%d-%d-%s" % c if isinstance(c, tuple) else str(c)


# ---- stage 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("case", sr.EDGE_CASES, ids=_ids)
def test_stage1_correspondences(hooks_lib, case, kind):
    """One wave, one block, a block with one lane in use, a one-point target grid, fewer points than lanes per group; source points
    beyond max_dist and non-finite ones; under the identity (no placement) and under a pose.  Integer for integer."""
    sc = sr.edge_case(*case)
    assert sc["fragile"] == []
    fp = edge_first_pass(hooks_lib, case, kind)
    assert np.array_equal(fp["corr"], sc["corr"]), np.nonzero(fp["corr"] != sc["corr"])[0][:10]
    assert fp["sums"][29] == float((sc["corr"] >= 0).sum())


# ---- stage 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(64, 257, "identity"), (257, 65, "quarter")], ids=_ids)
def test_stage2_covariances_from_normals(hooks_lib, case):
    """Both clouds' covariances, by point index (the source's as placed: not turned), against 60 digits within the bound counted from
    the reference's |Rx|: random unit normals, e1, -e1, n_x = -0.99 exactly (the formula, factor 100) and one ulp below (the
    identity), the zero vector, a non-unit normal and one of length 1e3."""
    sc = sr.edge_case(*case, long_normal=True)
    assert sc["fragile"] == []
    fp = first_pass(hooks_lib, "GeneralizedIcp", sc["src"], sc["tgt"], sc["max_dist"], sc["init"], src_n=sc["src_n"], tgt_n=sc["tgt_n"])
    assert np.array_equal(fp["corr"], sc["corr"])
    assert sc["src_n"][2, 0] == -0.99 and sc["src_n"][3, 0] == np.nextafter(-0.99, -1.0) and np.linalg.norm(sc["tgt_n"][6]) > 900.0
    worst = 0.0
    for normals, cov in ((sc["src_n"], fp["scov"]), (sc["tgt_n"], fp["tcov"])):
        for k in range(len(normals)):
            Cm, b = sr.covariance_mp(normals[k], 1e-3)
            err = np.abs(cov[k] - Cm)
            assert np.all(err <= b), (k, normals[k], err, b)
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
        assert np.array_equal(cov[1], np.diag([1e-3, 1.0, 1.0])) and np.array_equal(cov[3], np.diag([1e-3, 1.0, 1.0]))   # the identity branch
        assert abs(cov[2][0, 0] - (1.0 - 0.999 * 0.9801)) < 1e-9                                                       # the formula at -0.99
    print("stage 2", case, "largest |C_dev - C_mp| / bound:", worst)


def test_stage2_caller_covariances_come_back_bit_for_bit(hooks_lib):
    """A caller's covariances win over the normals and are used as they are; of a matrix that is not symmetric the library reads
    m[0], m[3], m[6], m[4], m[7], m[8] of the nine column-major doubles: the upper triangle (row <= column)."""
    sc = sr.edge_case(65, 257, "quarter")
    assert sc["fragile"] == []
    rng = np.random.default_rng(5)
    out = {}
    for name, ns in (("src", 65), ("tgt", 257)):
        m = rng.uniform(0.5, 1.5, size=(ns, 9))          # nine doubles per point, all different
        m[:, [0, 4, 8]] += 3.0
        out[name] = m
    fp = first_pass(hooks_lib, "GeneralizedIcp", sc["src"], sc["tgt"], sc["max_dist"], sc["init"], src_n=sc["src_n"], tgt_n=sc["tgt_n"],
                    src_cov=out["src"], tgt_cov=out["tgt"])
    assert np.array_equal(fp["corr"], sc["corr"])
    for m, cov in ((out["src"], fp["scov"]), (out["tgt"], fp["tcov"])):
        colmajor = m.reshape(-1, 3, 3).transpose(0, 2, 1)          # [row, column] of the column-major matrix
        upper = np.triu(colmajor) + np.transpose(np.triu(colmajor, 1), (0, 2, 1))
        assert np.array_equal(cov, upper)
        assert not np.array_equal(cov, np.tril(colmajor) + np.transpose(np.tril(colmajor, -1), (0, 2, 1)))


# ---- stage 3 --------------------------------------------------------------------------------------------------------------------
SUM_RATIO = {k: 0.0 for k in sr.KINDS}


def reference_sums(kind, sc, fp):
    """first_pass_sums over the DEVICE's correspondences (stage 1 holds them to the reference's) and the DEVICE's covariances (stage
    2), the source's turned by the lattice pose (a signed permutation: exact)"""
    si = np.nonzero(fp["corr"] >= 0)[0]
    tj = fp["corr"][si]
    kw = {}
    if kind == "PointToPlaneIcp":
        kw["tn"] = sc["tgt_n"][tj]
    elif kind == "PointToPointIcp":
        kw["shift"] = fp["shift"]
    else:
        R = sc["init"][:3, :3]
        kw["cs"], kw["ct"] = R[None] @ fp["scov"][si] @ R.T[None], fp["tcov"][tj]
    return sr.first_pass_sums(kind, sc["placed"][si], sc["tgt"][tj], **kw), (si, tj)


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("case", sr.EDGE_CASES, ids=_ids)
def test_stage3_sums(hooks_lib, case, kind):
    sc = sr.edge_case(*case)
    fp = edge_first_pass(hooks_lib, case, kind)
    (ref, B), _ = reference_sums(kind, sc, fp)
    err = np.abs(fp["sums"] - ref)
    ratio = float((err[B > 0] / B[B > 0]).max()) if (B > 0).any() else 0.0
    SUM_RATIO[kind] = max(SUM_RATIO[kind], ratio)
    print("stage 3", case, kind, "largest |sum_dev - sum_ref| / B_k: %.3g; so far:" % ratio, SUM_RATIO)
    assert np.all(err <= B), (np.nonzero(err > B)[0], fp["sums"], ref, B)
    assert fp["sums"][29] == ref[29]                                         # slot 29 is exactly the count


# ---- stage 4 --------------------------------------------------------------------------------------------------------------------
def _resid(A, b, x):
    return float(np.linalg.norm((A.astype(LD) @ x.astype(LD) - b.astype(LD)).astype(np.float64)))


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("case", sr.EDGE_CASES, ids=_ids)
def test_stage4_update_from_the_device_sums(hooks_lib, case, kind):
    """o3s_test_o3d_update on the device's own sums against the references' update of those same sums.  Full rank: x within 16 times
    the restatement's error against mpmath, never less than kappa u (one system, not a group: the a-priori form of the bound is the
    floor).  One, two or three pairs leave the system rank-deficient: the residual and the range component, as in
    tests/test_o3d_update_host.py.  Point-to-point: the Umeyama contract against the pairs themselves."""
    sc = sr.edge_case(*case)
    fp = edge_first_pass(hooks_lib, case, kind)
    si = np.nonzero(fp["corr"] >= 0)[0]
    tj = fp["corr"][si]
    n = len(si)
    if kind == "PointToPointIcp":
        T, _ = lib_update(hooks_lib, kind, fp["sums"], fp["shift"])
        q, t = sc["placed"][si], sc["tgt"][tj]
        rank = min(3, len(np.unique(tj)) - 1)      # the centred targets span (distinct matched target points - 1) dimensions, the sources more
        assert np.linalg.matrix_rank(q - q.mean(axis=0)) >= rank
        check_umeyama(T, q, t, rank, fp["shift"], fp["sums"], "%s" % (case,))
        return
    T, x = lib_update(hooks_lib, kind, fp["sums"])
    assert np.all(np.isfinite(x))
    assert np.abs(T - sr.vec6_to_T_mp(x)).max() <= VEC6_BOUND
    A, b = sr.sums_to_system(fp["sums"])
    # the rank the scene has: one row per pair with a non-zero normal (point-to-plane); [-[q]x | I] of one point has rank 3, of two
    # points 3 + rank([q1 - q2]x) = 5, of three or more 6 (GICP)
    # (a target of one or two points carries the normals e1 and -e1 only: a plane scene, rank 3, with rx, ty, tz exactly dead)
    if kind == "PointToPlaneIcp":
        rank = min(3 if case[1] <= 2 else 6, int((np.abs(sc["tgt_n"][tj]).sum(axis=1) > 0).sum()))
        if case[1] <= 2:
            assert np.all(x[[0, 4, 5]] == 0.0), x
    else:
        rank = {1: 3, 2: 5}.get(n, 6)
    lam = np.sort(np.abs(np.linalg.eigvalsh(A)))[::-1]
    assert lam[rank - 1] > 1e-9 * lam[0] and (rank == 6 or lam[rank] <= 1e-12 * lam[0]), (rank, lam)
    xr = sr.ldlt_solve6(A, b)
    if rank == 6:
        xm, _, lm = sr.solve_mp(A, b)
        kappa = lm.max() / lm.min()
        e_ref, e_lib = rel(xr, xm), rel(x, xm)
        assert e_lib <= 16 * max(e_ref, kappa * U), (e_lib, e_ref, kappa)
    else:
        xp, P, lm = sr.solve_mp(A, b, rank)
        nb = float(np.linalg.norm(b))
        res_ref, res_lib = _resid(A, b, xr), _resid(A, b, x)
        assert res_lib <= 64 * max(res_ref, U * nb), (res_lib, res_ref)
        if res_ref <= 1e-9 * nb and np.linalg.norm(xp) > 0:
            assert rel(P @ x, xp) <= 16 * max(rel(P @ xr, xp), U * lm.max() / lm.min())


# ---- stage 5 --------------------------------------------------------------------------------------------------------------------
def degenerate_scene(name, seed=0):
    """clouds of a degenerate scene: the target is the surface with its normals, the source the lifted points plus a few far away"""
    q, t, tn, rank = sr.degenerate_pairs(name, 200, seed)
    far = q[:9] + np.array([60.0, -70.0, 80.0])
    src = np.concatenate([q[:100], far, q[100:]])
    src_n = np.concatenate([tn[:100], tn[:9], tn[100:]])
    assert len(sr.fragile_pairs(src, t, 0.25)) == 0
    return src, src_n, t, tn, rank


def one_iteration(kind, src, src_n, tgt, tgt_n, max_dist, init=None):
    if kind == "PointToPlaneIcp":
        return reg.registration_icp(src, tgt, tgt_n, max_dist, init, max_iteration=1)
    if kind == "PointToPointIcp":
        return reg.registration_icp_point_to_point(src, tgt, max_dist, init, max_iteration=1)
    return reg.registration_generalized_icp(src, tgt, max_dist, init, source_normals=src_n, target_normals=tgt_n, max_iteration=1)


@pytest.mark.parametrize("kind", ["PointToPlaneIcp", "GeneralizedIcp"])
@pytest.mark.parametrize("name", ["plane_z", "two_planes", "line", "tilted_plane", "tilted_corridor", "tilted_cylinder"])
def test_stage5_one_iteration_on_degenerate_scenes(hooks_lib, name, kind):
    """max_iteration = 1 (on the hooks build, which shares every kernel and the host loop with the product): the pose is update . init
    with the update stage 4 judged; iterations, count and fitness are exact.  On the axis-aligned plane the translation in the plane
    stays exactly zero.  The sum of squared residuals along the normals over the first pass's pairs, recomputed from the returned
    pose, is the optimum of the linearised problem: within 16 times what the restatement's pose leaves above (or, by the second-order
    part, below) it (never less than
    1e-12 of the sum before, the second-order part of a 1e-2 step that the linearisation does not see)."""
    src, src_n, tgt, tgt_n, rank = degenerate_scene(name)
    fp = first_pass(hooks_lib, kind, src, tgt, 0.25, None, src_n=src_n if kind == "GeneralizedIcp" else None, tgt_n=tgt_n)
    si = np.nonzero(fp["corr"] >= 0)[0]
    tj = fp["corr"][si]
    assert len(si) == 200 and np.array_equal(tj, np.arange(200))           # every lifted point finds the point it was lifted from
    upd, x = lib_update(hooks_lib, kind, fp["sums"])
    g = one_iteration(kind, src, src_n, tgt, tgt_n, 0.25)
    assert np.array_equal(g.transformation, upd)                           # update . identity, bit for bit
    assert g.iterations == 1 and g.correspondences == 200 and g.fitness == 200.0 / 209.0
    if name == "plane_z" and kind == "PointToPlaneIcp":
        assert x[2] == 0.0 and x[3] == 0.0 and x[4] == 0.0
        assert g.transformation[0, 3] == 0.0 and g.transformation[1, 3] == 0.0
    if kind != "PointToPlaneIcp":
        return
    A, b = sr.sums_to_system(fp["sums"])
    q, t, n = src[si], tgt[tj], tgt_n[tj]
    ssr = lambda T: float((((q @ T[:3, :3].T + T[:3, 3] - t) * n).sum(axis=1) ** 2).sum())
    before = ssr(np.eye(4))
    xp, _, _ = sr.solve_mp(A, b, rank)
    optimum = float(fp["sums"][27] - b @ xp)                                 # |r|^2 - b^T A^+ b
    left_ref = ssr(sr.vec6_to_T_quat(sr.ldlt_solve6(A, b))) - optimum
    left_dev = ssr(g.transformation) - optimum
    print("stage 5", name, "SSR before %.3e optimum %.3e; above it: restatement %.3e device %.3e" % (before, optimum, left_ref, left_dev))
    assert abs(left_dev) <= 16 * max(abs(left_ref), 1e-12 * before), (left_dev, left_ref)
    assert optimum <= 1e-3 * before or name == "tilted_cylinder"             # a rigid step takes the lifted planes back


@pytest.mark.parametrize("name,k", [("one", 1), ("two", 2), ("collinear", 5), ("coplanar", 12)])
def test_stage5_point_to_point_on_few_pairs(hooks_lib, name, k):
    """Point-to-point with one, two, collinear and coplanar correspondence sets, chosen through max_dist: the other source points are
    further than max_dist from every target point.  The returned pose is a proper rotation that attains the optimum of the pairs
    (which one, below rank 2, is not specified) and carries the pairs' means onto each other."""
    rng = np.random.default_rng(30 + k)
    tgt = sr.lattice(rng, 300, 0.0, 4.0)
    if name == "collinear":
        base = np.array([1.0, 1.0, 1.0]) + np.outer(np.arange(k) * 0.5, np.array([1.0, 0.5, 0.25]))
    elif name == "coplanar":
        base = np.concatenate([sr.lattice(rng, k, 0.5, 3.5)[:, :2], np.full((k, 1), 2.0)], axis=1)
    else:
        base = sr.lattice(rng, k, 0.5, 3.5)
    tgt[:k] = base
    src_near = base + np.array([1.0, -2.0, 0.5]) * 2.0 ** -6
    src = np.concatenate([src_near, sr.lattice(rng, 40, 0.0, 4.0) + 50.0])
    r = 0.04
    d = np.linalg.norm(tgt[None, k:, :] - src_near[:, None, :], axis=2)
    assert d.min() > 3 * r and len(sr.fragile_pairs(src, tgt, r)) == 0
    fp = first_pass(hooks_lib, "PointToPointIcp", src, tgt, r)
    assert np.array_equal(fp["corr"], np.concatenate([np.arange(k), np.full(40, -1)]).astype(np.int32))
    g = one_iteration("PointToPointIcp", src, None, tgt, None, r)
    upd, _ = lib_update(hooks_lib, "PointToPointIcp", fp["sums"], fp["shift"])
    assert np.array_equal(g.transformation, upd) and g.iterations == 1
    rank = {"one": 0, "two": 1, "collinear": 1, "coplanar": 2}[name]
    check_umeyama(g.transformation, src_near, base, rank, fp["shift"], fp["sums"], name)


# ---- stage 6 --------------------------------------------------------------------------------------------------------------------
def three_planes(ns, seed):
    """three mutually tilted planes through one corner, generic coordinates: a well-conditioned system at any size"""
    rng = np.random.default_rng(seed)
    u, v, w = sr.tilted_frame()
    org = np.array([0.3, -0.2, 0.6])
    nt = 3 * ns
    ab = rng.uniform(0.1, 2.0, size=(nt, 2))
    k = np.arange(nt) % 3
    axes = [(u, v, w), (v, w, u), (w, u, v)]
    tgt = np.stack([org + ab[i, 0] * axes[k[i]][0] + ab[i, 1] * axes[k[i]][1] for i in range(nt)])
    tgt_n = np.stack([axes[k[i]][2] for i in range(nt)])
    pick = rng.permutation(nt)[:ns]
    T_gt = oref.vec6_to_T(np.array([0.02, -0.015, 0.01, 0.03, -0.02, 0.025]))
    inv = np.linalg.inv(T_gt)
    src = (tgt[pick] + rng.normal(scale=0.002, size=(ns, 3))) @ inv[:3, :3].T + inv[:3, 3]
    src_n = tgt_n[pick] @ inv[:3, :3].T
    return src, src_n, tgt, tgt_n, T_gt


POSE_DIFF = {k: 0.0 for k in sr.KINDS}


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("ns", [65, 257])
def test_stage6_full_icp_at_tiny_sizes(ns, kind):
    src, src_n, tgt, tgt_n, T_gt = three_planes(ns, 40 + ns)
    kw = {}
    if kind == "PointToPlaneIcp":
        g = reg.registration_icp(src, tgt, tgt_n, 0.3)
        kw = dict(target_normals=tgt_n)
    elif kind == "PointToPointIcp":
        g = reg.registration_icp_point_to_point(src, tgt, 0.3)
    else:
        g = reg.registration_generalized_icp(src, tgt, 0.3, source_normals=src_n, target_normals=tgt_n)
        kw = dict(source_normals=src_n, target_normals=tgt_n)
    o = oref.registration_icp(src, tgt, 0.3, None, kind, **kw)
    assert g.iterations == o["iterations"] and g.correspondences == o["correspondences"] and g.fitness == o["fitness"]
    assert g.iterations > 1 and g.correspondences > ns // 2
    diff = float(np.abs(g.transformation - o["transformation"]).max())
    POSE_DIFF[kind] = max(POSE_DIFF[kind], diff)
    print("stage 6", ns, kind, "pose difference %.2e; so far:" % diff, POSE_DIFF)
    assert diff <= 1e-9 and abs(g.inlier_rmse - o["inlier_rmse"]) <= 1e-9 * max(1.0, o["inlier_rmse"])


# ---- stage 7 --------------------------------------------------------------------------------------------------------------------
def _bytes(r):
    return (np.asarray(r.transformation).tobytes(), r.fitness, r.inlier_rmse, r.correspondences, r.iterations)


def bystander_scene():
    src, src_n, tgt, tgt_n, _ = three_planes(257, 77)
    far_s = src[:20] + np.array([300.0, 200.0, -100.0])
    far_t = tgt[:30] + np.array([-400.0, 100.0, 250.0])
    return (np.concatenate([src, far_s]), np.concatenate([src_n, src_n[:20]]), np.concatenate([tgt, far_t]), np.concatenate([tgt_n, tgt_n[:30]]))


def test_stage7_points_without_a_correspondence_are_never_read():
    """A NaN or zero normal, or a singular covariance, on a point that has no correspondence in any pass changes no bit of the result;
    two calls give the same bytes."""
    src, src_n, tgt, tgt_n = bystander_scene()
    ns, nt = len(src) - 20, len(tgt) - 30
    for bad in (np.nan, 0.0):
        sn2, tn2 = src_n.copy(), tgt_n.copy()
        sn2[ns:], tn2[nt:] = bad, bad
        a = reg.registration_generalized_icp(src, tgt, 0.3, source_normals=src_n, target_normals=tgt_n)
        b = reg.registration_generalized_icp(src, tgt, 0.3, source_normals=sn2, target_normals=tn2)
        assert a.correspondences > 200 and _bytes(a) == _bytes(b)
        assert _bytes(a) == _bytes(reg.registration_generalized_icp(src, tgt, 0.3, source_normals=src_n, target_normals=tgt_n))
        p = reg.registration_icp(src, tgt, tgt_n, 0.3)
        assert _bytes(p) == _bytes(reg.registration_icp(src, tgt, tn2, 0.3)) == _bytes(reg.registration_icp(src, tgt, tgt_n, 0.3))
    cs, ct = oref.covariances_from_normals(src_n, 1e-3), oref.covariances_from_normals(tgt_n, 1e-3)
    cs2, ct2 = cs.copy(), ct.copy()
    cs2[ns:], ct2[nt:] = 0.0, 0.0                                            # singular: M = 0 would have no inverse
    a = reg.registration_generalized_icp(src, tgt, 0.3, source_covariances=cs, target_covariances=ct)
    b = reg.registration_generalized_icp(src, tgt, 0.3, source_covariances=cs2, target_covariances=ct2)
    assert a.correspondences > 200 and _bytes(a) == _bytes(b)
    pp = reg.registration_icp_point_to_point(src, tgt, 0.3)
    assert _bytes(pp) == _bytes(reg.registration_icp_point_to_point(src, tgt, 0.3))


_TINY = """
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
from test_gpu_registration_edges import tiny_calls
print("RESULT", tiny_calls(large_first=False))
"""


def tiny_calls(large_first):
    """the three registrations of a 65-point scene, as hex; large_first: each after a call of a few thousand points on the same
    (pooled) work area"""
    out = []
    src, src_n, tgt, tgt_n, _ = three_planes(65, 105)
    if large_first:
        S, Sn, T, Tn, _ = three_planes(3000, 9)
    for kind in sr.KINDS:
        if large_first:
            r = one_iteration(kind, S, Sn, T, Tn, 0.3)
            assert r.correspondences > 2000
        if kind == "PointToPlaneIcp":
            r = reg.registration_icp(src, tgt, tgt_n, 0.3)
        elif kind == "PointToPointIcp":
            r = reg.registration_icp_point_to_point(src, tgt, 0.3)
        else:
            r = reg.registration_generalized_icp(src, tgt, 0.3, source_normals=src_n, target_normals=tgt_n)
        out.append(np.asarray(r.transformation).tobytes().hex() + ":%r:%r:%d:%d" % (r.fitness, r.inlier_rmse, r.correspondences, r.iterations))
    return "|".join(out)


def test_stage7_tiny_call_after_a_large_one_equals_a_fresh_process():
    """The work areas are pooled and only grow: a 65-point call that finds the buffers, the index and the certificates of a
    3000-point call gives the bytes of the same call in a process that has done nothing else (this test is about that second
    process: one child, one device)."""
    here = tiny_calls(large_first=True)
    out = subprocess.run([sys.executable, "-c", _TINY % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    fresh = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):]
    assert fresh == here


# ---- the resident path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sr.KINDS)
def test_resident_refinement_of_tiny_submaps_equals_host_path(kind):
    """registration_icp_submaps_overlap on two submaps of a few hundred points — one plane and a strip of wall — equals the host
    registration on the selected points bit for bit, as test_gpu_registration_types.py shows at size."""
    from test_gpu_registration_types import _resident, bits

    rng = np.random.default_rng(8)

    def cloud(n, x0, x1):
        floor = np.stack([rng.uniform(x0, x1, n), rng.uniform(0.0, 3.0, n), 0.002 * rng.normal(size=n)], axis=1)
        m = n // 4
        wall = np.stack([rng.uniform(x0, x1, m), 3.0 + 0.002 * rng.normal(size=m), rng.uniform(0.0, 0.6, m)], axis=1)
        return (np.concatenate([floor, wall]), np.concatenate([np.tile([0.0, 0.0, 1.0], (n, 1)), np.tile([0.0, -1.0, 0.0], (m, 1))]))

    tgt, tgt_n = cloud(320, 0.0, 4.0)
    src, src_n = cloud(240, 1.5, 5.5)                                      # shares a strip of floor and wall with the target
    a, b = _resident(src, src_n, tgt, tgt_n)
    sa, sna = a.getMapPointCloud()
    tb, tnb = b.getMapPointCloud()
    init = oref.vec6_to_T(np.array([0.004, -0.003, 0.002, 0.01, -0.015, 0.02]))
    res, info, n_ov = reg.registration_icp_submaps_overlap(a, b, 0.3, init, 0.5, registration_type=kind)
    gs, gt = reg.compute_indices_of_overlapping_points(sa, tb, init, 0.5)
    assert n_ov == (len(gs), len(gt)) and 50 < len(gs) < len(sa) and 50 < len(gt) < len(tb)
    if kind == "GeneralizedIcp":
        h = reg.registration_generalized_icp(sa[gs], tb[gt], 0.3, init, source_normals=sna[gs], target_normals=tnb[gt])
    elif kind == "PointToPointIcp":
        h = reg.registration_icp_point_to_point(sa[gs], tb[gt], 0.3, init)
    else:
        h = reg.registration_icp(sa[gs], tb[gt], tnb[gt], 0.3, init)
    bits(res, h)
    assert res.correspondences > 50
    oi = oref.information_matrix(sa[gs], tb[gt], 0.3, res.transformation)
    assert np.abs(info - oi).max() <= 1e-9 * max(1.0, np.abs(oi).max())
