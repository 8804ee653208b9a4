"""Pins tests/o3d_solve_ref.py — the judge of tests/test_o3d_update_host.py and tests/test_gpu_registration_edges.py — on the CPU,
against mpmath and against the older restatement tests/o3d_registration_ref.py.

Measured here (x86-64, numpy 2, mpmath 1.3; printed by the tests with -s):
  ldlt_solve6 against solve_mp on 200 random SPD systems, kappa 1 .. 1e3: largest |x - x_mp| / (kappa u |x|) = 0.99 (allowed: 64).
  B_k on the lattice scenes, fp64 terms added forwards / backwards / pairwise: largest |sum - exact| / B_k = 0.056 / 0.057 / 0.028
    (point-to-plane), 0 / 0 / 0 (point-to-point: lattice coordinates and a dyadic shift make every fp64 term and sum exact),
    7.5e-4 / 7.5e-4 / 7.5e-4 (GICP: the per-term part is a worst case of the cofactor inverse, the fp64 terms here use an LU inverse).
  B_k is tight: the smallest, over the scenes and the pairs tried, of max_k<28 |change| / B_k is 7.3e6 for a dropped pair, 1.9e6 for two
    swapped coordinates, 1.2e10 for the source covariances left unturned."""
import numpy as np
import pytest

import o3d_registration_ref as oref
import o3d_solve_ref as sr

U = sr.U


def spd(rng, sv):
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    A = (Q * np.asarray(sv)) @ Q.T
    return 0.5 * (A + A.T)


def test_ldlt_equals_mpmath_on_well_conditioned_systems():
    """Backward stability of LDLT with diagonal pivoting (Higham 10.3 / 11.1 for n = 6): |x - x*| <= c n u kappa |x*| with a small c;
    64 kappa u allowed, 1.6 measured."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in range(200):
        kappa = 10.0 ** rng.uniform(0, 3)
        A = spd(rng, np.geomspace(1.0, 1.0 / kappa, 6) * 10.0 ** rng.uniform(-3, 3))
        b = rng.normal(size=6)
        x, P, lam = sr.solve_mp(A, b)
        assert np.array_equal(P, np.eye(6)) and abs(lam[0] / lam[-1] / kappa - 1) < 1e-6
        err = np.linalg.norm(sr.ldlt_solve6(A, b) - x) / (kappa * U * np.linalg.norm(x))
        worst = max(worst, err)
    print("ldlt vs mp, worst error / (kappa u |x|):", worst)
    assert worst <= 64.0


def test_ldlt_reads_the_lower_triangle_and_pivots_symmetrically():
    rng = np.random.default_rng(2)
    A = spd(rng, [5, 4, 3, 2, 1, 0.5])
    b = rng.normal(size=6)
    x = sr.ldlt_solve6(A, b)
    junk = A + np.triu(rng.normal(size=(6, 6)), 1)          # the strict upper triangle is never read
    assert np.array_equal(sr.ldlt_solve6(junk, b), x)
    assert np.allclose(A @ x, b, rtol=0, atol=1e-13)
    for perm in ([5, 4, 3, 2, 1, 0], [2, 0, 5, 1, 4, 3]):   # a symmetric permutation of the system permutes the answer
        p = np.array(perm)
        assert np.allclose(sr.ldlt_solve6(A[np.ix_(p, p)], b[p]), x[p], rtol=0, atol=1e-13)


@pytest.mark.parametrize("name,dead", [("plane_z", [2, 3, 4]), ("two_planes", [4]), ("line", [0, 2, 3, 4])])
def test_ldlt_gives_exact_zeros_on_exactly_zero_pivots(name, dead):
    q, t, tn, rank = sr.degenerate_pairs(name)
    sums, _ = sr.first_pass_sums("PointToPlaneIcp", q, t, tn=tn)
    A, b = sr.sums_to_system(sums)
    assert not A[dead].any() and not A[:, dead].any() and not b[dead].any()      # exact zeros in the system: dyadic coordinates
    assert np.linalg.matrix_rank(A) == rank == 6 - len(dead)
    x = sr.ldlt_solve6(A, b)
    assert np.all(x[dead] == 0.0)
    live = [i for i in range(6) if i not in dead]
    xm, P, lam = sr.solve_mp(A, b, rank)
    assert np.abs(xm[dead]).max() <= 1e-50 and np.abs(np.diag(P)[dead]).max() <= 1e-50     # (the eigenvectors are good to 60 digits)
    kappa = lam.max() / lam.min()
    assert np.linalg.norm(x[live] - xm[live]) <= 64 * kappa * U * np.linalg.norm(xm)
    assert abs(x[5] + 2.0 ** -7) <= 1e-12                           # the shift along e3 that takes the lifted source back


def _scene_inputs(kind, sc, turn=True):
    """what first_pass_sums reads, from a lattice scene: the corresponded pairs and, for GICP, covariances from the normals (fp64),
    the source's turned by the lattice pose (exact)"""
    si = np.nonzero(sc["corr"] >= 0)[0]
    tj = sc["corr"][si]
    kw = {}
    if kind == "PointToPlaneIcp":
        kw["tn"] = sc["tgt_n"][tj]
    elif kind == "PointToPointIcp":
        kw["shift"] = np.array([2.0, 2.0, 2.0])
    else:
        with np.errstate(invalid="ignore"):      # (the restatement forms 0 * inf for the normal -e1 before it takes the identity branch)
            cs = oref.covariances_from_normals(sc["src_n"], 1e-3)[si]
            ct = oref.covariances_from_normals(sc["tgt_n"], 1e-3)[tj]
        if turn:
            R = sc["init"][:3, :3]
            cs = R[None] @ cs @ R.T[None]
        kw["cs"], kw["ct"] = cs, ct
    return sc["placed"][si], sc["tgt"][tj], kw


def _pairwise(v):
    n = len(v)
    if n <= 2:
        return v.sum(axis=0) if n else 0.0
    return _pairwise(v[:n // 2]) + _pairwise(v[n // 2:])


CPU_SCENES = [(65, 65, "identity"), (64, 65, "quarter"), (257, 1000, "quarter"), (1000, 1000, "identity"), (1000, 1000, "quarter"), (1000, 2, "quarter")]


@pytest.mark.parametrize("case", sr.EDGE_CASES, ids=lambda c: "%d-%d-%s" % c)
def test_no_scene_has_a_tie_or_a_pair_at_the_radius(case):
    sc = sr.edge_case(*case)
    assert sc["fragile"] == []
    n_hit = int((sc["corr"] >= 0).sum())
    assert n_hit >= 1 and (case[0] < 12 or n_hit < case[0])     # something to sum; from 12 points on, some without a neighbour
    fin = np.isfinite(sc["src"]).all(axis=1)
    assert not (sc["placed"][fin] / sr.LAT % 1).any() and not (sc["tgt"] / sr.LAT % 1).any()     # on the lattice: d^2 is exact


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("case", CPU_SCENES, ids=lambda c: "%d-%d-%s" % c)
def test_bound_holds_for_fp64_sums_in_three_orders(case, kind):
    q, t, kw = _scene_inputs(kind, sr.edge_case(*case))
    sums, B = sr.first_pass_sums(kind, q, t, **kw)
    terms = sr.pass_terms(kind, q, t, **kw)
    assert sums[29] == len(q) and B[29] == 0.0
    fwd = np.zeros(30)
    for row in terms:
        fwd = fwd + row
    bwd = np.zeros(30)
    for row in terms[::-1]:
        bwd = bwd + row
    ratios = []
    for got in (fwd, bwd, _pairwise(terms)):
        err = np.abs(got - sums)
        assert np.all(err <= B), (kind, np.nonzero(err > B)[0], err, B)
        ratios.append(float(np.max(err[B > 0] / B[B > 0])))
    print(kind, case, "largest |sum - exact| / B_k forwards, backwards, pairwise:", ratios)


@pytest.mark.parametrize("kind", sr.KINDS)
@pytest.mark.parametrize("case", sr.EDGE_CASES, ids=lambda c: "%d-%d-%s" % c)
def test_bound_is_tight(case, kind):
    """A term left out, two coordinates swapped in one term and (GICP) the source's covariances read as placed each move some sum of
    the system (slots 0..27) by more than its bound."""
    sc = sr.edge_case(*case)
    q, t, kw = _scene_inputs(kind, sc)
    sums, B = sr.first_pass_sums(kind, q, t, **kw)
    n = len(q)
    exact = sr.pass_terms(kind, q, t, **kw, dtype=sr.LD)
    sys_k = np.arange(28)
    least = {"drop": np.inf, "swap": np.inf}
    for i in sorted(set(np.linspace(0, n - 1, 12).astype(int))):
        change = np.abs(exact[i].astype(np.float64))                       # dropping pair i removes its term
        m = float(np.max(change[sys_k][B[sys_k] > 0] / B[sys_k][B[sys_k] > 0]))
        assert m > 1.0, ("drop", i, m)
        least["drop"] = min(least["drop"], m)
        if q[i, 0] == q[i, 1]:
            continue
        q2 = q[i:i + 1].copy()
        q2[0, [0, 1]] = q2[0, [1, 0]]
        kw_i = {k: (v[i:i + 1] if k != "shift" else v) for k, v in kw.items()}
        other = sr.pass_terms(kind, q2, t[i:i + 1], **kw_i, dtype=sr.LD)[0]
        one = sr.pass_terms(kind, q[i:i + 1], t[i:i + 1], **kw_i, dtype=sr.LD)[0]
        change = np.abs((other - one).astype(np.float64))
        m = float(np.max(change[sys_k][B[sys_k] > 0] / B[sys_k][B[sys_k] > 0]))
        assert m > 1.0, ("swap", i, m)
        least["swap"] = min(least["swap"], m)
    if kind == "GeneralizedIcp" and case[2] == "quarter":
        q_, t_, kw_ = _scene_inputs(kind, sc, turn=False)
        unturned, _ = sr.first_pass_sums(kind, q_, t_, **kw_)
        m = float(np.max(np.abs(unturned - sums)[sys_k] / B[sys_k]))
        assert m > 1.0, ("unturned", m)
        least["unturned"] = m
    print(kind, case, "smallest max_k |change| / B_k:", least)


def test_older_restatement_agrees_at_full_rank():
    """update_point_to_plane, update_generalized and umeyama of tests/o3d_registration_ref.py against the new pieces on a lattice
    scene with random normals (full rank, kappa ~ 1e2): 1e-9, the figure the GPU tests hold the library to."""
    sc = sr.edge_case(1000, 1000, "quarter")
    si = np.nonzero(sc["corr"] >= 0)[0]
    tj = sc["corr"][si]
    for kind in ("PointToPlaneIcp", "GeneralizedIcp"):
        q, t, kw = _scene_inputs(kind, sc)
        sums, _ = sr.first_pass_sums(kind, q, t, **kw)
        A, b = sr.sums_to_system(sums)
        x, _, lam = sr.solve_mp(A, b)
        assert lam[0] / lam[-1] < 1e6
        T = sr.vec6_to_T_mp(x)
        if kind == "PointToPlaneIcp":
            old = oref.update_point_to_plane(sc["placed"], sc["tgt"], sc["tgt_n"], si, tj)
            ldl = oref.update_point_to_plane(sc["placed"], sc["tgt"], sc["tgt_n"], si, tj, solver=sr.ldlt_solve6)
        else:
            cs = np.zeros((len(sc["src"]), 3, 3))
            cs[si] = kw["cs"]
            ct = oref.covariances_from_normals(sc["tgt_n"], 1e-3)
            old = oref.update_generalized(sc["placed"], sc["tgt"], cs, ct, si, tj)
            ldl = oref.update_generalized(sc["placed"], sc["tgt"], cs, ct, si, tj, solver=sr.ldlt_solve6)
        assert np.abs(old - T).max() <= 1e-9 and np.abs(ldl - T).max() <= 1e-9, (kind, np.abs(old - T).max(), np.abs(ldl - T).max())
    um = sr.umeyama_mp(sc["placed"][si], sc["tgt"][tj], 3)
    old = oref.umeyama(sc["placed"][si], sc["tgt"][tj])
    assert um["unique"] and um["sign"] == 1
    assert np.abs(old[:3, :3] - um["R"]).max() <= 1e-12 and np.abs(old[:3, 3] - um["t"]).max() <= 1e-12
    sums, _ = sr.first_pass_sums("PointToPointIcp", sc["placed"][si], sc["tgt"][tj], shift=np.array([2.0, 2.0, 2.0]))
    T2, sigma = sr.umeyama_from_sums(sums, np.array([2.0, 2.0, 2.0]))
    assert np.abs(sigma - um["sigma"]).max() <= 1e-13 and np.abs(T2 - old).max() <= 1e-12


def test_umeyama_reference_on_known_cases():
    """The reflection case of Umeyama's paper in 3-D: e1, e2, e3, 0 -> e1, e2, -e3, 0: singular values 4, 4, 1 of 16 sigma, det < 0, a
    simple smallest one: unique, optimum (4 + 4 - 1) / 16; with e1 and e2 also flipped in scale the top value is double."""
    src = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [0, 0, 0]])
    dst = src * np.array([1.0, 1.0, -1.0])
    um = sr.umeyama_mp(src, dst, 3)
    assert np.allclose(um["sv"] * 16, [4.0, 4.0, 1.0], atol=1e-15) and um["sign"] == -1 and um["unique"]
    assert abs(um["optimum"] - 7.0 / 16.0) < 1e-16 and abs(np.linalg.det(um["R"]) - 1.0) < 1e-15
    assert abs(np.trace(um["R"] @ um["sigma"].T) - um["optimum"]) < 1e-15
    one = sr.umeyama_mp(src[:1], dst[:1], 0)
    assert not one["unique"] and one["optimum"] == 0.0 and one["R"] is None
    rng = np.random.default_rng(4)
    flat = np.concatenate([rng.normal(size=(20, 2)), np.zeros((20, 1))], axis=1)
    Rz = oref.vec6_to_T(np.array([0.0, 0.0, 0.7, 0, 0, 0]))[:3, :3]
    for flip in (1.0, -1.0):   # coplanar, rotated in the plane (and mirrored across a line of it: still a proper rotation in 3-D)
        um = sr.umeyama_mp(flat, (flat * np.array([1.0, flip, 1.0])) @ Rz.T, 2)
        assert um["unique"] and um["sv"][2] == 0.0 and abs(np.linalg.det(um["R"]) - 1.0) < 1e-14
        assert np.abs(um["R"] - Rz @ np.diag([1.0, flip, flip])).max() < 1e-14


def test_covariance_reference_branches():
    eps = 1e-3
    for n in ([1.0, 0, 0], [-1.0, 0, 0], [0.0, 0, 0], [float(np.nextafter(-0.99, -1.0)), 0.1, 0.0]):
        C, b = sr.covariance_mp(n, eps)
        assert np.array_equal(C, np.diag([eps, 1.0, 1.0])), n
    C, b = sr.covariance_mp([-0.99, 0.0, np.sqrt(1 - 0.99 ** 2)], eps)
    assert np.abs(C - np.diag([eps, 1.0, 1.0])).max() > 0.1                      # the formula, not the identity branch
    assert np.abs(C - oref.covariances_from_normals(np.array([[-0.99, 0.0, np.sqrt(1 - 0.99 ** 2)]]), eps)[0]).max() <= b.max()
    rng = np.random.default_rng(5)
    nn = sr.special_normals(rng, 60, long_normal=True)
    Cs = oref.covariances_from_normals(nn, eps)
    for k in range(60):
        C, b = sr.covariance_mp(nn[k], eps)
        assert np.all(np.abs(Cs[k] - C) <= b), (k, nn[k])


def test_vec6_restatement_is_within_its_counted_bound():
    """The quaternion form in fp64 against 60 digits; the count is in tests/test_o3d_update_host.py (VEC6_BOUND)."""
    from test_o3d_update_host import VEC6_ANGLES, VEC6_BOUND

    for slot in range(3):
        for a in VEC6_ANGLES:
            x = np.array([0.3, -0.2, 0.1, 1.0, 2.0, 3.0])
            x[slot] = a
            assert np.abs(sr.vec6_to_T_quat(x) - sr.vec6_to_T_mp(x)).max() <= VEC6_BOUND, (slot, a)
