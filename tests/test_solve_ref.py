"""The scenes of tests/solve_ref.py and the oracle's 6x6 solver, pinned on the CPU so that tests/test_gpu_solver_branches.py can
trust both: which solver branch every scene reaches (orc.solve6: 0 LLT, 1 minimum norm, 2 fp64 fallback), and the oracle's x
against a float64 SVD minimum-norm solution wherever the system is away from the rank decision.

Measured |x_orc - x_f64| / |x_f64| (g++ -O2, x86-64):
  exact-rank scenes, pairs(K), sphere, generic   3.2e-6 at most (pairs(6), kappa 5.4e3)
  sweep points with kappa <= 5e5 or >= 1e7       6.8e-7 at most (plane, ordinary motion, kappa 5.0e4)
  branch-2 points (rcond 6 * 2^-52)              4.7e-8 at most
A dropped or spurious direction shows as 1e3 and more on the in-null-space sweeps (three corridor points between kappa 1.4e6 and
1.8e6, where the QR still says rank 6 and the float64 SVD rank 5, are in the excluded band).  The bound is 1e-4: 30 times the
largest figure, a tenth of the 1e-3 ceiling.
"""
import functools

import numpy as np
import pytest

import solve_ref as sr
from oracle import oracle as orc


@functools.lru_cache(maxsize=None)
def records():
    out = []
    for name, make, kind in sr.all_cases():
        _, _, _, A, b, x, br = sr.oracle_system(orc, make())
        out.append((name, kind, A, b, x, br, sr.kappa2(A)))
    return out


def by_name(name):
    return next(r for r in records() if r[0] == name)


def test_scene_builders_are_what_they_say():
    for make in (sr.generic, sr.plane, sr.corridor, sr.cylinder, sr.sphere):
        ref, nrm, reading, w = make()
        assert ref.shape == nrm.shape == reading.shape == (sr.N, 3) and w.shape == (sr.N,) and np.all(w == 1)
        assert ref.dtype == nrm.dtype == reading.dtype == w.dtype == np.float32
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
        R = sr.rodrigues_f64(sr.ORDINARY[0])
        assert np.allclose(reading, ref.astype(np.float64) @ R.T + np.array(sr.ORDINARY[1]), atol=1e-6)
    ref, nrm, _, _ = sr.corridor()
    assert set(np.unique(nrm)) == {-1.0, 0.0, 1.0} and np.all(nrm[:, 0] == 0)     # exact in fp32: A's x row and column are exact zeros
    assert np.all(ref[: sr.N // 2, 2] == -1) and np.all(ref[sr.N // 2:, 1] == 1)
    ref, nrm, _, _ = sr.cylinder()
    assert np.allclose(np.hypot(ref[:, 0], ref[:, 1]), 1.5, atol=1e-6) and np.all(nrm[:, 2] == 0)
    ref, _, _, _ = sr.sphere()
    assert np.allclose(np.linalg.norm(ref, axis=1), 2.0, atol=1e-6)
    for K in range(1, 7):
        assert np.count_nonzero(sr.pairs(K)[3]) == K
    a, b = sr.tilted("plane", 1e-2), sr.tilted("plane", 1e-3)
    da, db = a[1] - sr.plane()[1], b[1] - sr.plane()[1]
    assert np.abs(da[:, :2]).max() > 1e-2 and np.allclose(da[:, :2], 10 * db[:, :2], rtol=0, atol=2e-3)   # one noise draw, scaled by eps


def test_rodrigues_and_min_norm_are_plain():
    R = sr.rodrigues_f64((0.0, 0.0, np.pi / 2))
    assert np.allclose(R, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    rv = np.array([0.3, -2.0, 1.1])
    R = sr.rodrigues_f64(rv)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(R), 1.0) and np.allclose(R @ rv, rv, atol=1e-14)
    assert np.isclose(np.trace(R), 1 + 2 * np.cos(np.linalg.norm(rv)))
    assert np.array_equal(sr.rodrigues_f64((0, 0, 0)), np.eye(3))
    A = np.diag([4.0, 2.0, 1.0, 1e-9, 0.0, 0.0])
    b = np.ones(6)
    assert np.allclose(sr.min_norm_f64(A, b, sr.RCOND32), [0.25, 0.5, 1, 0, 0, 0])
    assert np.allclose(sr.min_norm_f64(A, b, sr.RCOND64), [0.25, 0.5, 1, 1e9, 0, 0])
    assert np.array_equal(sr.min_norm_f64(np.zeros((6, 6)), b, sr.RCOND32), np.zeros(6))


@pytest.mark.parametrize("name,rank", [("plane", 3), ("corridor", 5), ("cylinder", 5)])
def test_exact_rank_scenes_take_the_minimum_norm_branch(name, rank):
    _, _, A, _, _, br, _ = by_name(name)
    assert br == 1 and sr.rank_f64(A) == rank == sr.EXACT_RANK[name]
    if name == "corridor":
        assert np.all(A[3, :] == 0) and np.all(A[:, 3] == 0)


@pytest.mark.parametrize("K", range(1, 7))
def test_pairs_give_rank_k(K):
    _, _, A, b, x, br, _ = by_name(f"pairs{K}")
    assert sr.rank_f64(A) == K
    assert br == (0 if K == 6 else 1)
    if K == 1:
        assert np.all(b == 0) and np.all(x == 0)


def test_zero_normals_give_the_rank_0_return():
    _, _, A, b, x, br, _ = by_name("no_normals")
    assert np.all(A == 0) and np.all(b == 0) and sr.rank_f64(A) == 0
    assert br == 1 and np.all(x == 0)


def test_generic_and_sphere_are_full_rank():
    assert by_name("generic")[5] == 0 and by_name("generic")[6] < 10
    assert by_name("sphere")[5] == 0 and 1e3 < by_name("sphere")[6] < 4e3       # ill-conditioned, kappa about 2e3


def test_plane_sweep_crosses_the_fast_path_bound_and_the_rank_threshold():
    sweep = [r for r in records() if r[0].startswith("tilted-plane-ordinary")]
    kap = np.array([r[6] for r in sweep])
    br = np.array([r[5] for r in sweep])
    assert np.all(np.diff(kap) > 0)                                             # eps slides kappa monotonically
    assert kap[0] < sr.KAPPA_FAST and kap[-1] > 1e11
    last0 = np.max(np.nonzero(br == 0)[0])
    assert np.all(br[: last0 + 1] == 0) and np.all(br[last0 + 1:] == 1)         # branch 0 up to the threshold, then branch 1
    assert 3e5 < kap[last0] < 1.4e6 < kap[last0 + 1]                            # ... which is the QR's 1 / (6 eps) = 1.4e6


@pytest.mark.parametrize("kind,least", [("plane", 25), ("corridor", 20), ("cylinder", 14)])
def test_in_null_space_sweeps_land_in_the_fp64_fallback(kind, least):
    """Measured: 30, 23 and 17 of 49."""
    sweep = [r for r in records() if r[0].startswith(f"tilted-{kind}-innull")]
    assert len(sweep) == 49 and sum(1 for r in sweep if r[5] == 2) >= least


def test_sweeps_reach_every_way_through_the_solver():
    got = sr.reach([(r[5], r[6]) for r in records() if r[1] == "sweep"])
    for what, least in sr.REACH_MIN.items():
        assert got[what] >= least, (what, got)


def test_oracle_solver_against_float64():
    worst = {}
    checked = 0
    for name, kind, A, b, x, br, kap in records():
        if not sr.well_separated(kind, br, kap):
            continue
        err = sr.rel_err(x, sr.min_norm_f64(A, b, sr.RCOND64 if br == 2 else sr.RCOND32))
        grp = kind if br != 2 else "fp64"
        if err > worst.get(grp, (0.0, ""))[0]:
            worst[grp] = (err, name)
        checked += 1
        assert err < sr.X_F64_BOUND, (name, br, kap, err)
    print("oracle against float64, worst per group:", worst)
    assert checked >= 140 and set(worst) == {"fixed", "sweep", "fp64"}
