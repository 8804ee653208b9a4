"""Known answers of tests/outlier_ref.py, worked out by hand from the contract of include/outlier_removal/o3s_outlier_removal.h
(CPU only): the reference the GPU tests compare against is itself pinned here."""
import math

import numpy as np
import pytest

import outlier_ref as R


def lattice(n=5):
    g = np.arange(n, dtype=np.float64)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def on_border(p, n=5):
    return ((p == 0) | (p == n - 1)).sum(axis=1)   # 3: corner, 2: edge, 1: face, 0: inside


@pytest.mark.parametrize("use_tree", [False, True])
def test_radius_on_a_unit_lattice(use_tree):
    """radius 1.5 reaches d2 in {0, 1, 2}: the point, its 6 axis neighbours and its 12 face diagonals where the lattice has them.
    Inside: 1 + 6 + 12 = 19.  On a face (one axis cut on one side): 1 + 5 + (4 + 2 + 2) = 14.  On an edge (two axes cut):
    1 + 4 + (1 + 2 + 2) = 10.  At a corner: 1 + 3 + 3 = 7.  (The issue that asked for this test wrote 15 and 11 for face and edge;
    counting the diagonals as above gives 14 and 10, and the brute force agrees.)"""
    p = lattice()
    b = on_border(p)
    cnt = R.radius_counts(p, 1.5, use_tree)
    assert (cnt[b == 0] == 19).all() and (cnt[b == 1] == 14).all() and (cnt[b == 2] == 10).all() and (cnt[b == 3] == 7).all()
    assert ((b == 3).sum(), (b == 2).sum(), (b == 1).sum()) == (8, 36, 54)
    for nb, kept in ((6, b <= 3), (7, b <= 2), (9, b <= 2), (10, b <= 1), (11, b <= 1), (13, b <= 1), (14, b == 0), (18, b == 0), (19, b < 0)):
        assert (R.radius_outlier(p, nb, 1.5, use_tree) == kept).all(), nb
    assert R.radius_outlier(p, 11, 1.5).sum() == 125 - 8 - 36


def test_radius_comparison_is_strict_on_the_squared_distance():
    """(0,0,0), (3,4,0), radius 5: d2 = 25 is not < 25; each point counts itself alone, and 1 > 1 is false."""
    p = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]])
    assert (R.radius_counts(p, 5.0) == 1).all()
    assert not R.radius_outlier(p, 1, 5.0).any()
    assert R.radius_outlier(p, 1, np.nextafter(5.0, 6.0)).all()


def test_statistical_on_four_collinear_points():
    """x = 0, 1, 2, 10, nb_neighbors = 2: every list is the point itself (0) and its nearest other point — 1, 1 (a tie between the
    points at 0 and 2: the lower index, same distance), 1, 8 — so avg = 0.5, 0.5, 0.5, 4.  valid = 4, mean = 5.5 / 4 = 1.375; the
    deviations are -0.875 (three times) and 2.625: 3 * 0.765625 + 6.890625 = 9.1875; / 3 = 3.0625; std = 1.75, all exact in fp64.
    thr = 1.375 + ratio * 1.75: ratio 1 -> 3.125 keeps the first three; ratio 1.5 -> 4.0 and 4 < 4 is false; ratio 2 -> 4.875 keeps all."""
    p = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [10.0, 0, 0]])
    r = R.statistical_outlier(p, 2, 1.0)
    assert r["avg"].tolist() == [0.5, 0.5, 0.5, 4.0]
    assert (r["valid"], r["mean"], r["std"], r["thr"]) == (4, 1.375, 1.75, 3.125)
    assert r["keep"].tolist() == [True, True, True, False]
    assert (r["sum_abs"], r["sum_sq"]) == (5.5, 9.1875)
    assert r["gap"] == (4.0 - 3.125) / 3.125
    r = R.statistical_outlier(p, 2, 1.5)
    assert r["thr"] == 4.0 and r["keep"].tolist() == [True, True, True, False] and r["gap"] == 0.0
    assert R.statistical_outlier(p, 2, 2.0)["keep"].all()
    assert R.statistical_outlier(p, 2, 1.0, use_tree=True)["avg"].tolist() == [0.5, 0.5, 0.5, 4.0]


def test_statistical_single_point_keeps_nothing():
    """N = 1: the list is the point itself, avg = 0; valid = 1, mean = 0 / 1, std = sqrt(0 / 0) = NaN: nothing is kept."""
    r = R.statistical_outlier(np.array([[1.0, 2.0, 3.0]]), 5, 1.0)
    assert r["avg"].tolist() == [0.0] and r["valid"] == 1 and r["mean"] == 0.0
    assert math.isnan(r["std"]) and math.isnan(r["thr"]) and not r["keep"].any()


def test_statistical_coincident_points_keep_nothing():
    """Seven copies of one point: every avg is 0, no term enters either sum, mean = std = thr = 0 and avg > 0 fails everywhere."""
    r = R.statistical_outlier(np.tile([[0.25, -3.0, 7.0]], (7, 1)), 3, 2.0)
    assert (r["avg"] == 0.0).all() and (r["valid"], r["mean"], r["std"], r["thr"]) == (7, 0.0, 0.0, 0.0)
    assert not r["keep"].any()


def test_statistical_with_fewer_points_than_neighbours():
    """Three points at x = 0, 3, 4 and nb_neighbors = 10: k = 3, every list is the whole cloud.  avg = 7/3, 4/3, 5/3."""
    p = np.array([[0.0, 0, 0], [3.0, 0, 0], [4.0, 0, 0]])
    r = R.statistical_outlier(p, 10, 1.0)
    assert r["avg"].tolist() == [(0.0 + 3.0 + 4.0) / 3.0, (0.0 + 1.0 + 3.0) / 3.0, (0.0 + 1.0 + 4.0) / 3.0]
    assert r["valid"] == 3
    mean = ((7.0 / 3.0 + 4.0 / 3.0) + 5.0 / 3.0) / 3.0
    assert r["mean"] == mean
    assert r["keep"].tolist() == [bool(a < r["thr"]) for a in r["avg"]]
    assert r["keep"].tolist() == [False, True, True]   # std = 0.509..., thr = 2.287... < 7/3


def test_non_finite_points_are_no_ones_neighbours_and_always_removed():
    p = np.array([[0.0, 0, 0], [np.nan, 0, 0], [1.0, 0, 0], [0, np.inf, 0], [2.0, 0, 0]])
    assert R.radius_counts(p, 1.5).tolist() == [2, 0, 3, 0, 2]
    assert R.radius_outlier(p, 1, 1.5).tolist() == [True, False, True, False, True]
    r = R.statistical_outlier(p, 4, 10.0)
    assert r["avg"].tolist() == [1.0, -1.0, 2.0 / 3.0, -1.0, 1.0] and r["valid"] == 3   # k = min(4, 3 finite points)
    assert r["keep"].tolist() == [True, False, True, False, True]


def test_tree_route_equals_brute_force_bit_for_bit():
    rng = np.random.default_rng(5)
    p = rng.normal(size=(700, 3))
    p[50:60] = p[40:50]   # duplicates: ties in distance
    assert (R.radius_counts(p, 0.4, True) == R.radius_counts(p, 0.4, False)).all()
    a, b = R.statistical_outlier(p, 20, 1.5, True), R.statistical_outlier(p, 20, 1.5, False)
    assert (a["avg"] == b["avg"]).all() and a["thr"] == b["thr"] and (a["keep"] == b["keep"]).all()
