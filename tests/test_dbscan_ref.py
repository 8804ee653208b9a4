"""tests/dbscan_ref.py against itself and against known answers (CPU only): the closed form of the contract equals Open3D's
sequential loop whatever order its set is popped in, equals scikit-learn's DBSCAN where that is installed, and gives the answers
worked out by hand below."""
import numpy as np
import pytest

import dbscan_ref as R

SEEDS = range(60)


def seeded_cloud(seed):
    """320 points: 2 - 6 Gaussian clusters and 60 uniform strays, shuffled; every fifth cloud has NaN rows"""
    r = np.random.default_rng(seed)
    k = int(r.integers(2, 7))
    c = r.uniform(-2, 2, (k, 3))
    p = np.concatenate([c[r.integers(0, k, 260)] + r.normal(0, 0.18, (260, 3)), r.uniform(-3, 3, (60, 3))])
    r.shuffle(p)
    if seed % 5 == 0:
        p[r.integers(0, len(p), 3)] = np.nan
    return p, float(r.uniform(0.12, 0.3)), int(r.integers(1, 9))


def contested(nb, labels, min_points):
    """the non-core points with core neighbours in more than one cluster"""
    core = np.array([len(x) >= min_points and len(x) > 0 for x in nb])
    return [i for i in range(len(nb)) if not core[i] and len(nb[i]) and len({int(labels[j]) for j in nb[i] if core[j]}) > 1]


_RUNS = {}


def run(seed):
    if seed not in _RUNS:
        p, eps, mp = seeded_cloud(seed)
        nb = R.neighbours(p, eps)
        _RUNS[seed] = (p, eps, mp, nb, R.dbscan(p, eps, mp, nbrs=nb))
    return _RUNS[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_closed_form_equals_open3d_loop_in_any_pop_order(seed):
    p, eps, mp, nb, (lab, n, sizes) = run(seed)
    a, na = R.dbscan_sequential(p, eps, mp, nbrs=nb)
    assert na == n and np.array_equal(a, lab)
    b, nb_ = R.dbscan_sequential(p, eps, mp, rng=np.random.default_rng(1000 + seed), nbrs=nb)
    assert nb_ == n and np.array_equal(b, lab)
    assert np.array_equal(sizes, np.bincount(lab[lab >= 0], minlength=n)) and (lab[~np.isfinite(p).all(1)] == -1).all()


def test_the_seeded_clouds_hold_contested_borders():
    total = sum(len(contested(run(s)[3], run(s)[4][0], run(s)[2])) for s in SEEDS)
    assert total >= 1, "no border point between two clusters in any cloud: the min-id rule went untested"


@pytest.mark.parametrize("seed", SEEDS)
def test_closed_form_equals_sklearn(seed):
    cluster = pytest.importorskip("sklearn.cluster")
    p, eps, mp, nb, (lab, n, _) = run(seed)
    fin = np.isfinite(p).all(1)
    s = cluster.DBSCAN(eps=eps, min_samples=mp).fit(p[fin]).labels_
    # sklearn's predicate is d <= eps on its own distance; no pair of these clouds lies within rounding of eps (asserted)
    f = p[fin]
    d = np.sqrt(((f[:, None, :] - f[None, :, :]) ** 2).sum(-1))
    assert not (np.abs(d - eps) < 1e-12).any()
    assert np.array_equal(s, lab[fin])


def test_tree_route_equals_brute_force():
    p, eps, mp = seeded_cloud(7)
    a = R.dbscan(p, eps, mp, use_tree=False)
    b = R.dbscan(p, eps, mp, use_tree=True)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_strict_comparison_by_hand():
    """two points exactly eps apart are no neighbours; one ulp closer they are"""
    p = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
    lab, n, sizes = R.dbscan(p, 0.5, 2)
    assert n == 0 and (lab == -1).all() and len(sizes) == 0
    lab, n, sizes = R.dbscan(p, 0.5, 1)            # each is its own neighbour: two clusters of one
    assert n == 2 and lab.tolist() == [0, 1] and sizes.tolist() == [1, 1]
    p[1, 0] = np.nextafter(0.5, 0)
    lab, n, sizes = R.dbscan(p, 0.5, 2)
    assert n == 1 and lab.tolist() == [0, 0] and sizes.tolist() == [2]


def test_known_answers_by_hand():
    """a line of five points at 1.0, eps 1.5, min_points 3: the ends have two neighbours (border), the middle three are core;
    an isolated point is noise; a NaN row is noise.  Then the contested border: two cores' clusters, a point between them."""
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 50.0])
    p = np.stack([x, np.zeros(6), np.zeros(6)], axis=1)
    p = np.concatenate([p, [[np.nan, 0.0, 0.0]]])
    lab, n, sizes = R.dbscan(p, 1.5, 3)
    assert n == 1 and lab.tolist() == [0, 0, 0, 0, 0, -1, -1] and sizes.tolist() == [5]
    assert R.keep_mask(lab, sizes, 5).tolist() == [True] * 5 + [False, False]
    assert not R.keep_mask(lab, sizes, 6).any()
    assert R.keep_mask(lab, sizes, 0).tolist() == [True] * 5 + [False, False]
    # blob B = {0, 1, 2, 3} around x = 2, blob A = {4, 5, 6, 7} around x = 0, point 8 at x = 1 between them: eps 0.75,
    # min_points 4 — 8 sees one core of each side (2 at 1.7, 6 at 0.3) and itself: 3 neighbours, not core.  B holds the smaller
    # core index, so B is cluster 0, and 8 takes min(0, 1) = 0
    q = np.array([[2.0, 0, 0], [2.2, 0, 0], [1.7, 0, 0], [2.1, 0.1, 0],
                  [0.0, 0, 0], [-0.2, 0, 0], [0.3, 0, 0], [-0.1, 0.1, 0], [1.0, 0, 0]])
    lab, n, sizes = R.dbscan(q, 0.75, 4)
    assert n == 2 and lab.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0] and sizes.tolist() == [5, 4]
    seq, ns = R.dbscan_sequential(q, 0.75, 4, rng=np.random.default_rng(5))
    assert ns == 2 and np.array_equal(seq, lab)
    lab2, n2, _ = R.dbscan(q[::-1].copy(), 0.75, 4)   # reversed order: the other blob gets id 0, and the point between goes with it
    assert n2 == 2 and lab2.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]


def test_empty_and_all_nan():
    lab, n, sizes = R.dbscan(np.zeros((0, 3)), 0.5, 3)
    assert len(lab) == 0 and n == 0 and len(sizes) == 0
    lab, n, _ = R.dbscan(np.full((5, 3), np.nan), 0.5, 1)
    assert n == 0 and (lab == -1).all()
    assert R.dbscan_sequential(np.full((5, 3), np.nan), 0.5, 1)[0].tolist() == [-1] * 5
