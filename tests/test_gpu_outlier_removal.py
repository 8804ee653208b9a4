"""The outlier filters on host arrays (o3s_remove_outliers: k_or_count, k_or_knn_mean, k_or_stats_*, k_or_mask in
csrc/outlier_dev.h) against tests/outlier_ref.py.  MI355X only.

Contract of every case: the radius mask equals the reference's; avg_dist is bit-equal; mean, std and thr lie within the bound of
outlier_ref.stats_bounds (same terms, another order of addition: derived, not measured); the statistical mask equals the
reference's; the output is the input restricted to the mask, in order, normals with it; out_indices are the kept indices; a second
call gives the same bits.

The statistical mask could hide a flip only through the order of the two cloud-wide sums, so its inputs are chosen: every cloud
below (seeds fixed) keeps each avg_i at a relative distance of at least 1e-9 from the threshold — more than two orders above
N 2^-52 at N <= 20 200 — and the test asserts that itself.  Where at most two terms are positive (N <= 2, or nb_neighbors = 1,
where every avg is 0) there is nothing to choose: floating-point addition is commutative, every order gives the same bits, and
N = 2 with nb_neighbors >= 2 always has avg_0 = avg_1 = thr."""
import contextlib
import os
import tempfile

import numpy as np
import pytest

import outlier_ref as R
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 33, 63, 64, 65, 257, 4099)
NB_NEIGHBORS = (1, 2, 20, 32)
NB_POINTS = (1, 5, 40)
STD_RATIO = 1.5
MIN_GAP = 1e-9
TREE_FROM = 4099   # the reference takes its candidate sets from cKDTree from this size on


# ---- inputs (seeds fixed; check_stat asserts the gap condition on every one of them) ------------------------------------------------
def cloud(N, seed=0):
    """a bumpy sheet with a sprinkle of points off it, coordinates of both signs, no duplicates"""
    rng = np.random.default_rng(1000 + 7 * N + seed)
    p = np.empty((N, 3))
    p[:, 0] = rng.uniform(-6.0, 4.0, N)
    p[:, 1] = rng.uniform(-3.0, 5.0, N)
    p[:, 2] = 0.3 * np.sin(p[:, 0]) + 0.05 * rng.normal(size=N)
    off = rng.random(N) < 0.06
    p[off, 2] += rng.uniform(0.5, 3.0, int(off.sum())) * rng.choice([-1.0, 1.0], int(off.sum()))
    return p


def spacing(N):
    return (80.0 / max(N, 1)) ** 0.5   # mean spacing of N points on the 10 x 8 sheet


def clustered():
    """20 000 points in 25 clusters and 200 strays in the box around them"""
    rng = np.random.default_rng(77)
    c = rng.uniform(-20.0, 20.0, (25, 3)) * np.array([1.0, 1.0, 0.2])
    p = c[rng.integers(0, 25, 20000)] + rng.normal(size=(20000, 3)) * np.array([0.8, 0.8, 0.15])
    s = rng.uniform(-30.0, 30.0, (200, 3))
    q = np.concatenate([p, s])
    return q[rng.permutation(len(q))]


def normals_for(p):
    """any payload that identifies its point: what rides along must arrive unchanged"""
    n = np.empty_like(p)
    n[:, 0] = np.arange(len(p))
    n[:, 1] = -2.0 * np.arange(len(p)) - 1.0
    n[:, 2] = 0.5
    return n


_REF = {}


def ref_radius(key, p, nb, radius, tree):
    k = ("r", key, nb, radius)
    if k not in _REF:
        ck = ("rc", key, radius)
        if ck not in _REF:
            _REF[ck] = R.radius_counts(p, radius, tree)
        _REF[k] = _REF[ck] > nb
    return _REF[k]


def ref_stat(key, p, nb, ratio, tree):
    k = ("s", key, nb, ratio)
    if k not in _REF:
        _REF[k] = R.statistical_outlier(p, nb, ratio, tree)
    return _REF[k]


# ---- checks -----------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_output(p, nrm, mask, op, on, idx):
    assert (idx == np.flatnonzero(mask)).all() and len(idx) == int(mask.sum())
    assert same_bits(op, p[mask]), "kept points: not the input restricted to the mask, in order"
    assert same_bits(on, nrm[mask]), "normals did not follow their points"


def check_radius(key, p, nb, radius, tree=False):
    nrm = normals_for(p)
    mask = ref_radius(key, p, nb, radius, tree)
    op, on, idx = co.remove_radius_outlier(p, nb, radius, normals=nrm)
    got = np.zeros(len(p), bool)
    got[idx] = True
    assert (got == mask).all(), (key, nb, radius, np.flatnonzero(got != mask)[:10])
    check_output(p, nrm, mask, op, on, idx)
    op2, on2, idx2 = co.remove_radius_outlier(p, nb, radius, normals=nrm)
    assert same_bits(op, op2) and same_bits(on, on2) and same_bits(idx, idx2)
    return mask


def few_terms(ref):
    return int((ref["avg"] > 0.0).sum()) <= 2


def check_stat(key, p, nb, ratio=STD_RATIO, tree=False):
    N = len(p)
    nrm = normals_for(p)
    ref = ref_stat(key, p, nb, ratio, tree)
    op, on, idx, avg, st = co.remove_statistical_outlier(p, nb, ratio, normals=nrm)
    assert same_bits(avg, ref["avg"]), (key, nb, np.flatnonzero(avg != ref["avg"])[:10])
    assert st[3] == ref["valid"]
    loose, tight = R.stats_bounds(ref, N, ratio)
    for j, name in enumerate(("mean", "std", "thr")):
        want, got = ref[name], st[j]
        print(f"{key} nb {nb}: {name} ref {want!r} device {got!r} diff {abs(got - want)!r} bound {loose[name]!r}"
              + (f" tight {tight[name]!r}" if tight else ""))
        if np.isnan(want):
            assert np.isnan(got), name
            continue
        assert abs(got - want) <= loose[name], (name, got, want, loose[name])
        if tight:
            assert abs(got - want) <= tight[name], (name, got, want, tight[name])
    if not few_terms(ref):
        assert ref["gap"] >= MIN_GAP, f"the input {key} was chosen badly: an avg lies {ref['gap']:.3g} (relative) from the threshold"
    got = np.zeros(N, bool)
    got[idx] = True
    assert (got == ref["keep"]).all(), (key, nb, np.flatnonzero(got != ref["keep"])[:10])
    check_output(p, nrm, ref["keep"], op, on, idx)
    again = co.remove_statistical_outlier(p, nb, ratio, normals=nrm)
    for a, b in zip((op, on, idx, avg, st), again):
        assert same_bits(a, b), "two calls, different bits"
    return ref


# ---- the size x parameter grid ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", NB_POINTS)
@pytest.mark.parametrize("N", SIZES)
def test_radius_filter_equals_reference(N, nb):
    p = cloud(N)
    s = spacing(N)
    for radius in (1.2 * s, 2.5 * s, 4.0 * s):   # supports of a few, ~20 and ~50 points: below, around and above every nb_points
        check_radius(("cloud", N), p, nb, radius, tree=N >= TREE_FROM)


@pytest.mark.parametrize("nb", NB_NEIGHBORS)
@pytest.mark.parametrize("N", SIZES)
def test_statistical_filter_equals_reference(N, nb):
    ref = check_stat(("cloud", N), cloud(N), nb, tree=N >= TREE_FROM)
    if N >= 33 and nb >= 2:
        assert 0 < ref["keep"].sum() < N   # the case removes something and keeps something


def test_clustered_cloud_with_strays():
    p = clustered()
    m = check_radius("clustered", p, 5, 0.6, tree=True)
    assert 15000 < m.sum() < 20100
    check_radius("clustered", p, 40, 0.6, tree=True)
    ref = check_stat("clustered", p, 20, 2.0, tree=True)
    assert 15000 < ref["keep"].sum() < 20200
    check_stat("clustered", p, 32, 1.0, tree=True)


# ---- radius: edge cases ---------------------------------------------------------------------------------------------------------
def test_radius_cloud_within_one_cell():
    p = cloud(257)
    for radius, nb in ((20.0, 5), (20.0, 256), (20.0, 257), (1e6, 40)):   # every point sees every point: 257 > nb decides
        m = check_radius(("cloud", 257), p, nb, radius)
        assert m.all() == (257 > nb) and m.any() == (257 > nb)


def test_radius_sliver_of_3000_cells():
    """1 x 1 x 3 000 cells of the radius: the grid's extent / 512 floor makes the cell coarser than the radius"""
    rng = np.random.default_rng(31)
    r = 0.05
    p = np.stack([rng.uniform(0, r, 3000), rng.uniform(0, r, 3000), rng.uniform(0, 3000 * r, 3000)], axis=1)
    p[0, 2], p[1, 2] = 0.0, 3000 * r
    for nb in (1, 5):
        m = check_radius("sliver", p, nb, r)
        assert 0 < m.sum() < 3000


def test_radius_points_on_cell_faces_and_negative_coordinates():
    """a lattice whose spacing is the grid's cell edge, radius (1 + 1e-6), shifted so that the minimum is far below zero: every point
    sits on a corner of its cell; its axis neighbours are at exactly one cell — beyond the radius; with the radius a hair wider they
    are inside."""
    r = 0.25
    cell = r * (1.0 + 1e-6)
    g = np.arange(9, dtype=np.float64) * cell
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) - np.array([1000.0, 2.0, 0.5])
    m = check_radius("faces", p, 1, r)
    assert not m.any()   # d2 = cell^2 > r^2: every point is alone
    m = check_radius("faces", p, 4, r * 1.001)
    assert m.sum() == 729 - 8   # axis neighbours inside: the corners have 1 + 3, not > 4; the edges 1 + 4
    p2 = np.stack(np.meshgrid(np.arange(9.0) * r, np.arange(9.0) * r, np.arange(9.0) * r, indexing="ij"), axis=-1).reshape(-1, 3) - 3.0
    m = check_radius("lattice_r", p2, 1, r)   # neighbours at (about) the radius itself: the strict comparison on the squared distance decides
    check_radius("lattice_r", p2, 6, np.nextafter(r * 1.5, 1.0))


@contextlib.contextmanager
def _environ(values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _with_cell_cap(cap, fn):
    """fn() on the hooks build with the cap on the grid's cell arrays lowered; -> (fn's result, the O3S_PRINT_NGRID records)"""
    with tempfile.TemporaryFile() as f, _environ({"O3S_PRINT_NGRID": "1", "O3S_OR_MAX_CELLS": str(cap)}), _lib.variant("hooks"):
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        recs = []
        for ln in f.read().decode().splitlines():
            if ln.startswith("o3s ngrid:"):
                t = ln.split()
                recs.append(dict(cell=float(t[t.index("cell") + 1]), cap_steps=int(t[t.index("cap_steps") + 1]),
                                 dims=[int(x) for x in t[t.index("dims") + 1:t.index("dims") + 4]]))
    return out, recs


def test_coarser_cell_fallback_gives_the_same_result():
    """The dense cell arrays would not fit (the cap is lowered to 512 cells on the hooks build): the host picks a coarser cell, and
    nothing in the result moves — the neighbour sets are exact for any cell."""
    N = 4099
    p, s = cloud(N), spacing(N)
    nrm = normals_for(p)
    radius = 1.2 * s
    (op, on, idx), recs = _with_cell_cap(512, lambda: co.remove_radius_outlier(p, 5, radius, normals=nrm))
    assert len(recs) == 1 and recs[0]["cap_steps"] > 0 and recs[0]["cell"] > 2 * radius and np.prod(recs[0]["dims"]) <= 512, recs
    mask = ref_radius(("cloud", N), p, 5, radius, True)
    check_output(p, nrm, mask, op, on, idx)
    a = co.remove_radius_outlier(p, 5, radius, normals=nrm)   # the product build, the radius cell
    assert same_bits(a[2], idx)
    res, recs = _with_cell_cap(512, lambda: co.remove_statistical_outlier(p, 20, STD_RATIO, normals=nrm))
    assert recs and all(np.prod(r["dims"]) <= 512 for r in recs) and recs[-1]["cap_steps"] > 0, recs
    b = co.remove_statistical_outlier(p, 20, STD_RATIO, normals=nrm)
    for x, y in zip(res, b):
        assert same_bits(x, y)
    assert same_bits(res[3], ref_stat(("cloud", N), p, 20, STD_RATIO, True)["avg"])


# ---- statistical: edge cases ----------------------------------------------------------------------------------------------------
def test_statistical_duplicates():
    p = cloud(257, seed=3)
    p[100:140] = p[60:100]        # pairs of coincident points: ties at distance 0, broken by index
    p[200:210] = p[0]             # eleven copies of one point: with nb_neighbors <= 11 their avg is 0 and they are removed
    for nb in (2, 11, 20):
        ref = check_stat("dup", p, nb)
        if nb <= 11:
            assert (ref["avg"][200:210] == 0.0).all() and not ref["keep"][200:210].any()
    q = np.tile(p[:1], (65, 1))   # a cloud of coincident points keeps nothing
    ref = check_stat("coincident", q, 5)
    assert not ref["keep"].any() and ref["thr"] == 0.0


def test_non_finite_points():
    p = cloud(257, seed=5)
    bad = [0, 63, 64, 130, 256]
    p[0, 0] = np.nan
    p[63, 1] = np.inf
    p[64, 2] = -np.inf
    p[130] = np.nan
    p[256, 2] = np.nan
    for nb in (2, 20):
        ref = check_stat("nonfinite", p, nb)
        assert (ref["avg"][bad] == -1.0).all() and ref["valid"] == 252 and not ref["keep"][bad].any()
    s = spacing(257)
    for nb in (1, 5):
        m = check_radius("nonfinite", p, nb, 2.5 * s)
        assert not m[bad].any() and m.any()
    q = np.full((33, 3), np.nan)   # nothing finite at all
    assert len(co.remove_radius_outlier(q, 1, 1.0)[2]) == 0
    ref = check_stat("all_nan", q, 5)   # valid = 0: mean = 0 / 0, std = sqrt(0 / -1) = -0.0, thr = NaN
    assert not ref["keep"].any() and (ref["avg"] == -1.0).all() and ref["valid"] == 0 and np.isnan(ref["thr"])


def test_one_point_a_kilometre_away():
    """served by walking rings to the grid's extent"""
    p = cloud(4099, seed=9)
    p[1234] = [1000.0, 0.5, -0.25]
    ref = check_stat("far", p, 20, tree=True)
    assert not ref["keep"][1234] and ref["avg"][1234] > 900.0   # (0 + 19 distances of about 996 m) / 20
    ref = check_stat("far", p, 2, tree=True)
    assert not ref["keep"][1234]
    m = check_radius("far", p, 1, 2.5 * spacing(4099), tree=True)
    assert not m[1234]


def test_empty_cloud():
    e = np.zeros((0, 3))
    assert len(co.remove_radius_outlier(e, 3, 0.5)[0]) == 0
    assert len(co.remove_statistical_outlier(e, 3, 0.5)[0]) == 0
