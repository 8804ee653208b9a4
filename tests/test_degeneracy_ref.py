"""CPU-only: the known answers of the numpy restatement of the degeneracy-aware step (tests/degeneracy_ref.py): the projection of
the normal equations onto C x = 0 as include/degeneracy/o3s_degeneracy.h states it."""
import numpy as np
import pytest

import degeneracy_ref as dref
import localizability_ref as lref

K = 4000


def normal_equations(scene, seed=0, shift=(0.02, -0.01, 0.015)):
    """A = sum G G^T and b = -sum G h of the scene's centred pairs with the reading `shift` off its matches, fp64."""
    p, n = lref.centred_pairs(scene, K, seed)
    p, n = p.astype(np.float64), n.astype(np.float64)
    G = np.concatenate([np.cross(p, n), n], axis=1)
    h = n @ np.asarray(shift, np.float64)
    return G.T @ G, -(G.T @ h)


AXIS_SETS = [([], [[1, 0, 0]]), ([[1, 0, 0]], [[1, 0, 0]]), ([[0, 0, 1]], [[1, 0, 0], [0, 1, 0]]), (np.eye(3), np.eye(3)), (np.eye(3)[[2, 0]], [])]


@pytest.mark.parametrize("rot,trans", AXIS_SETS)
def test_axis_aligned_sets_hold_the_constraint_exactly(rot, trans):
    A, b = normal_equations("room")
    Ap, bp = dref.project(A, b, rot, trans)
    C, _ = dref.rows_of(rot, trans)
    assert np.array_equal(Ap, Ap.T)
    assert np.array_equal(C @ bp, np.zeros(len(C)))              # P b has exact zeros there: 1 - 1 and products with 0
    x = np.linalg.solve(Ap, bp)
    # A' is block diagonal between the constrained axes and the rest, exactly: the constrained rows hold mu on the diagonal and zeros
    for row in C:
        a = int(np.argmax(row))
        want = np.zeros(6)
        want[a] = Ap[a, a]
        assert np.array_equal(Ap[a], want) and Ap[a, a] > 0
        assert x[a] == 0.0
    assert dref.leakage(x, rot, trans) == 0.0
    # ... and on the rest x minimises the same quadratic: the free block of A x = b
    free = [a for a in range(6) if not C[:, a].any()]
    if free:
        assert np.allclose(x[free], np.linalg.solve(A[np.ix_(free, free)], b[free]), rtol=1e-9, atol=0)


def test_the_empty_set_returns_the_input():
    A, b = normal_equations("corridor")
    Ap, bp = dref.project(A, b, [], [])
    assert np.array_equal(Ap, A) and np.array_equal(bp, b)


def test_the_corridor_becomes_positive_definite_at_the_scale_of_a():
    A, b = normal_equations("corridor")
    ev = np.linalg.eigvalsh(A)
    assert ev[0] < 1e-5 * ev[-1]                                  # the axis is (nearly) free: ill-conditioned as it stands
    p, n = lref.centred_pairs("corridor", K)
    first = lref.analyse(p, n, 1.0, 1.0, 1.0)
    free = lref.free_mask("corridor", first["evec"])
    trans = first["evec"][:3][free[:3]]
    assert len(trans) == 1 and abs(trans[0][0]) > 0.999
    Ap, bp = dref.project(A, b, [], trans)
    assert np.array_equal(Ap, Ap.T)
    evp = np.linalg.eigvalsh(Ap)
    assert evp[0] > 0 and evp[-1] / evp[0] < 1e-2 * (ev[-1] / ev[0])
    mu_t = (A[3, 3] + A[4, 4] + A[5, 5]) / 3.0
    e = np.concatenate([np.zeros(3), trans[0]])
    assert abs(e @ Ap @ e - mu_t) <= 1e-12 * mu_t                  # the filled-in direction sits at mu_t
    x = np.linalg.solve(Ap, bp)
    assert dref.leakage(x, [], trans) <= 1e-12 * np.linalg.norm(x)
    # the minimiser of the same quadratic over C x = 0, by the null-space method
    Z = np.linalg.svd(e[None, :])[2][1:].T
    want = Z @ np.linalg.solve(Z.T @ A @ Z, Z.T @ b)
    assert np.allclose(x, want, rtol=1e-8, atol=1e-12)


@pytest.mark.parametrize("trace", [0.0, float("nan"), float("inf")])
def test_a_zero_or_non_finite_scale_is_replaced_by_one(trace):
    A = np.zeros((6, 6))
    A[3, 3] = trace
    assert dref._mu(A, 0) == 1.0 and dref._mu(A, 3) == 1.0       # the rotation block is all zeros; the translation block's trace
    if trace == 0.0:                                              # (a non-finite A stays non-finite wherever P A P touches it)
        Ap, _ = dref.project(A, np.zeros(6), [[0, 0, 1]], [[0, 1, 0]])
        want = np.zeros((6, 6))
        want[2, 2] = want[4, 4] = 1.0
        assert np.array_equal(Ap, want)


def test_step_from_x_is_a_rotation_about_the_reading_centroid():
    x = np.float32([0.01, -0.02, 0.03, 0.1, 0.2, -0.3])
    mp, mq = np.float32([1, 2, 3]), np.float32([1.5, 2.5, 2.0])
    T = dref.step_from_x(x, mp, mq).astype(np.float64)
    want = lref.make_T(x[:3].astype(np.float64), [0, 0, 0])
    assert np.allclose(T[:3, :3], want[:3, :3], atol=1e-7)
    assert np.allclose(T[:3, :3] @ mp + T[:3, 3], mq + x[3:], atol=1e-6)   # the centroid goes to mq + t
