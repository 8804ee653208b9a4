"""CPU-only: the known answers of the numpy restatement of the localizability analysis (tests/localizability_ref.py) on its four
scenes, and the properties of the library's host remap (o3s_localizability_remap: fp64 host arithmetic, no device)."""
import math

import numpy as np
import pytest

import localizability_ref as lref
from open3d_slam_advanced_rss_2024_public_amd import localizability as loc

K = 4000


def analysed(scene, seed=0):
    p, n = lref.centred_pairs(scene, K, seed)
    first = lref.analyse(p, n, 1.0, 1.0, 1.0)
    k1, k2, k3, free = lref.thresholds(scene, first)
    return lref.analyse(p, n, k1, k2, k3), (k1, k2, k3), free


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
def test_a_plane_with_exact_normals():
    P, Nn = lref.plane(K, jitter=False)
    p, n = (P - P.mean(0)).astype(np.float32), Nn.astype(np.float32)
    assert np.array_equal(n, np.tile(np.float32([0, 0, 1]), (K, 1)))
    res = lref.analyse(p, n, K / 2.0, K / 4.0, K / 100.0)
    want = np.zeros((3, 3))
    want[2, 2] = K
    assert np.array_equal(res["A_t"], want)                                  # A_t = K e_z e_z^T exactly
    assert np.array_equal(res["eval"][:3], [0.0, 0.0, float(K)])
    assert np.array_equal(res["evec"][:3], np.eye(3))
    assert list(res["category"][:3]) == [0, 0, 2]                            # translation x and y are not localizable
    assert np.array_equal(res["sum_all"][:3], [0.0, 0.0, float(K)]) and list(res["n_strong"][:3]) == [0, 0, K]
    # rotation: c = (py, -px, 0): nothing about z
    assert res["eval"][3] == 0.0 and abs(res["evec"][3][2]) == 1.0 and res["category"][3] == 0 and list(res["category"][4:]) == [2, 2]


@pytest.mark.parametrize("scene,lost", [("room", []), ("corridor", [0]), ("tunnel", [0, 3]), ("plane", [0, 1, 3])])
def test_each_scene_loses_exactly_its_free_directions(scene, lost):
    res, (k1, k2, k3), free = analysed(scene)
    assert sorted(np.flatnonzero(free)) == lost, (free, res["evec"])         # the free directions are the smallest eigenvalues' of a block
    big_free = max([0.0] + [max(res["sum_all"][j], res["sum_strong"][j]) for j in lost])
    small_con = min(res["sum_all"][j] for j in range(6) if j not in lost)
    print(scene, "free", big_free, "constrained", small_con, "eval", res["eval"])
    assert 4.0 * big_free < 0.5 * small_con and k1 >= k2 >= k3 > 0.0         # the geometry separates them, not the thresholds
    assert list(res["category"]) == [0 if j in lost else 2 for j in range(6)]
    if scene in ("corridor", "tunnel"):
        assert abs(res["evec"][0][0]) > 0.999                                # ... along x
    if scene == "tunnel":
        assert abs(res["evec"][3][0]) > 0.999                                # ... and about x


def test_jacobi_against_eigh():
    rng = np.random.default_rng(3)
    worst = 0.0
    for k in range(200):
        G = rng.normal(size=(rng.integers(1, 40), 3)) * rng.uniform(0.1, 10.0, 3)
        A = G.T @ G
        e, v = lref.jacobi3(A)
        V = v.T
        tr = np.trace(A)
        assert np.all(np.diff(e) >= 0)
        r = max(np.abs(A @ V - V * e).max(), np.abs(V.T @ V - np.eye(3)).max() * tr, np.abs(e - np.linalg.eigh(A)[0]).max()) / (2.0 ** -52 * tr)
        worst = max(worst, r)
        for j in range(3):
            assert v[j][np.argmax(np.abs(v[j]))] > 0
    print("largest residual / (2^-52 trace):", worst)
    assert worst < 16.0
    e, v = lref.jacobi3(np.full((3, 3), np.nan))
    assert np.isnan(e).all() and np.isnan(v).all()
    e, v = lref.jacobi3(np.zeros((3, 3)))
    assert np.array_equal(e, np.zeros(3)) and np.array_equal(v, np.eye(3))


# ---- the remap, through the library -------------------------------------------------------------------------------------------------------
def rigid(rvec, t):
    rvec = np.asarray(rvec, np.float64)
    th = np.linalg.norm(rvec)
    T = np.eye(4)
    if th > 0:
        k = rvec / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx
    T[:3, 3] = t
    return T


def as_result(res, centre):
    return loc.Localizability(res["eval"], res["evec"], res["sum_all"], res["sum_strong"], res["n_strong"], res["category"], res["kept"],
                              np.asarray(centre, np.float64))


T_PRIOR = rigid([0.02, -0.3, 0.5], [12.0, -3.0, 0.7])
T_ICP = rigid([0.012, -0.02, 0.03], [0.21, -0.05, 0.03]) @ T_PRIOR
CENTRE = np.array([14.0, -2.0, 1.0])


def test_remap_with_every_direction_kept_is_the_icp_pose_bit_for_bit():
    res, _, _ = analysed("room")
    T, n = loc.remap_pose(as_result(res, CENTRE), T_PRIOR, T_ICP)
    assert n == 0 and np.array_equal(T, T_ICP)
    T, n = loc.remap_pose(as_result(res, CENTRE), T_PRIOR, T_ICP, min_category=2)
    assert n == 0 and np.array_equal(T, T_ICP)


def test_remap_with_no_direction_kept_is_the_prior():
    res, _, _ = analysed("room")
    r = as_result(res, CENTRE)
    r.category = np.zeros(6, np.int32)
    T, n = loc.remap_pose(r, T_PRIOR, T_ICP)
    assert n == 6 and np.abs(T - T_PRIOR).max() <= 1e-12
    r.category = np.ones(6, np.int32)    # partially localizable everywhere: kept at 1, replaced at 2
    assert loc.remap_pose(r, T_PRIOR, T_ICP, 1)[1] == 0 and loc.remap_pose(r, T_PRIOR, T_ICP, 2)[1] == 6


@pytest.mark.parametrize("scene", ["corridor", "tunnel", "plane"])
def test_remap_is_idempotent_and_touches_only_the_free_directions(scene):
    res, _, free = analysed(scene)
    r = as_result(res, CENTRE)
    T1, n1 = loc.remap_pose(r, T_PRIOR, T_ICP)
    assert n1 == int(free.sum()) and not np.array_equal(T1, T_ICP)
    T2, n2 = loc.remap_pose(r, T_PRIOR, T1)
    assert n2 == n1 and np.abs(T2 - T1).max() <= 1e-12
    u0, r0 = lref.correction(T_PRIOR, T_ICP, CENTRE)
    u1, r1 = lref.correction(T_PRIOR, T1, CENTRE)
    for j in range(6):
        d = res["evec"][j]
        before, after = (d @ u0, d @ u1) if j < 3 else (d @ r0, d @ r1)
        if free[j]:
            assert abs(after) <= 1e-12, (j, after)                           # v_x . u' = 0
        else:
            assert abs(after - before) <= 1e-12, (j, before, after)         # the other components are unchanged
    assert np.abs(T1[:3, :3].T @ T1[:3, :3] - np.eye(3)).max() <= 1e-14 and np.array_equal(T1[3], [0, 0, 0, 1])


def test_remap_refuses_what_it_cannot_linearise():
    res, _, _ = analysed("corridor")
    r = as_result(res, CENTRE)
    for bad in (0, 3, -1):
        with pytest.raises(ValueError):
            loc.remap_pose(r, T_PRIOR, T_ICP, min_category=bad)
    with pytest.raises(ValueError):
        loc.remap_pose(r, T_PRIOR, rigid([0, 0, 1.6], [0, 0, 0]) @ T_PRIOR)   # a correction of more than pi / 2
    bad = T_ICP.copy()
    bad[0, 3] = np.nan
    with pytest.raises(ValueError):
        loc.remap_pose(r, T_PRIOR, bad)


def test_default_params():
    d = loc.default_params()
    assert d.filter_min == math.cos(math.radians(80.0)) == lref.KAPPA_F and d.strong_min == math.cos(math.radians(35.0)) == lref.KAPPA_S
    assert math.isnan(d.sum_all_min) and math.isnan(d.sum_strong_min) and math.isnan(d.sum_partial_min)
    assert loc.LocalizabilityParams().filter_min == d.filter_min and loc.LocalizabilityParams().strong_min == d.strong_min
