"""The fast exact neighbour-list reference (tests/normals_ref.py) against the oracle's brute force (CPU only): identical lists,
and bit-identical normals through oracle.normals_from_neighbours, on a ray-cast sweep, shuffled lattices whose distances tie
exactly, duplicate clusters larger than max_nn, and every max_nn from 1 to 32."""
import numpy as np
import pytest

import normals_ref as nr
from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn


def check_against_brute_force(p, radius, max_nn):
    """Returns how many queries needed the ball-query fallback."""
    on, oi = orc.estimate_normals(p, radius, max_nn, want_neighbours=True)
    st = nr.Stats()
    fn, fi = nr.estimate_normals(p, radius, max_nn, stats=st)
    assert np.array_equal(fi, oi)
    assert np.array_equal(fn.view(np.uint64), on.view(np.uint64))
    # the shared back half on the oracle's own lists gives the oracle's bits
    assert np.array_equal(orc.normals_from_neighbours(p, oi).view(np.uint64), on.view(np.uint64))
    assert st.queries == p.shape[0]
    return st.fallback


def lattice(n, pitch, seed, planar=False):
    g = np.arange(n) * pitch
    if planar:
        x, y = np.meshgrid(g, g, indexing="ij")
        p = np.c_[x.ravel(), y.ravel(), np.full(x.size, 1.5)]
    else:
        x, y, z = np.meshgrid(g, g, g, indexing="ij")
        p = np.c_[x.ravel(), y.ravel(), z.ravel()] + np.array([2.0, -3.0, 0.5])
    return p[np.random.default_rng(seed).permutation(p.shape[0])]


@pytest.fixture(scope="module")
def sweep_subset():
    world = syn.make_world(60000.0, seed=11)
    sp, _ = syn.make_lidar_scan(world, syn.corridor_pose(world, 3, 0.25), 64, 2048, max_range=60.0, sigma=0.01, seed=303)
    return np.ascontiguousarray(sp[::6], np.float64)


@pytest.mark.parametrize("radius,max_nn", [(1.0, 10), (0.5, 5), (3.0, 20), (1.0, 32)])
def test_sweep_subset_matches_brute_force(sweep_subset, radius, max_nn):
    assert sweep_subset.shape[0] > 20000
    check_against_brute_force(sweep_subset, radius, max_nn)


@pytest.mark.parametrize("max_nn", [7, 8, 19, 20, 27, 28])
def test_shuffled_cubic_lattice_ties(max_nn):
    # 0.125 is exact in binary: every distance is exact and each shell (6, 12, 8 at 1, sqrt 2, sqrt 3 pitches) ties exactly
    p = lattice(14, 0.125, seed=max_nn)
    fb = 0
    for radius in (0.125 * np.sqrt(2.0), 0.25, 0.5):
        fb += check_against_brute_force(p, radius, max_nn)
    if max_nn == 8:   # the 8th lies in the 12-point shell and so does the farthest of the 16 candidates: no certificate
        assert fb > 0


@pytest.mark.parametrize("max_nn", [4, 5, 8, 9, 13])
def test_shuffled_planar_lattice_ties(max_nn):
    p = lattice(60, 0.25, seed=100 + max_nn, planar=True)
    check_against_brute_force(p, 0.5, max_nn)
    check_against_brute_force(p, 0.25, max_nn)     # the radius exactly on the first shell: the strict cut drops it


def test_duplicate_clusters_larger_than_max_nn():
    rng = np.random.default_rng(7)
    base = rng.uniform(-4.0, 4.0, (3000, 3))
    dup = np.repeat(rng.uniform(-4.0, 4.0, (6, 3)), 45, axis=0)     # 45 copies of each of six points
    p = np.concatenate([base, dup, base[:40]])[rng.permutation(3000 + 270 + 40)]
    fb = 0
    for max_nn in (10, 32):
        fb += check_against_brute_force(p, 1.0, max_nn)
    assert fb >= 270


@pytest.mark.parametrize("max_nn", range(1, 33))
def test_every_max_nn(max_nn):
    rng = np.random.default_rng(max_nn)
    p = rng.normal(size=(1500, 3)) * np.array([3.0, 3.0, 0.3])
    check_against_brute_force(p, 0.6, max_nn)      # cuts most lists
    check_against_brute_force(p, 5.0, max_nn)      # fills them


def test_tiny_clouds():
    for p in (np.array([[1.0, 2.0, 3.0]]), np.array([[0.0, 0.0, 1.0], [0.0, 0.5, 1.0]]), np.zeros((3, 3)) + 2.0,
              np.array([[0.0, 0.0, 1.0], [0.0, 0.5, 1.0], [0.3, 0.1, 1.2]])):
        for max_nn in (1, 2, 3, 10):
            check_against_brute_force(p, 1.0, max_nn)
