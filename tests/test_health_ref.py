"""The numpy restatement of the two health quantities (tests/health_ref.py) on cases small enough to check by hand."""
import math

import numpy as np

import health_ref as href

I4 = np.eye(4)


def lattice():
    """one point in the middle of each voxel of a 2 x 2 x 2 block of 0.5 m voxels at the origin"""
    g = np.array([0.25, 0.75])
    return np.array([[x, y, z] for z in g for y in g for x in g])


def test_a_2x2x2_lattice_occupies_eight_voxels():
    vm = href.voxel_map(lattice(), 0.5)
    assert vm == {(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)}
    # all eight again, two in a voxel outside the block, one far away: 8 of 11
    scan = np.vstack([lattice() + 0.1, [[1.1, 0.2, 0.2], [-0.1, 0.2, 0.2], [30.0, 0.0, 0.0]]])
    n, f = href.overlap_fitness(vm, scan, I4, 0.5)
    assert n == 8 and f == 8 / 11


def test_points_on_voxel_faces_belong_to_the_upper_voxel():
    # 0.5 / 0.5 = 1 exactly: floor gives voxel 1; 1.0 -> 2; -0.5 -> -1; 0.0 -> 0
    k = href.voxel_keys([[0.5, 1.0, -0.5], [0.0, -0.0, 0.4999999999999999]], 0.5)
    assert k.tolist() == [[1.0, 2.0, -1.0], [0.0, 0.0, 0.0]]
    # the reciprocal form: 0.3 * (1 / 0.1) = 3.0000000000000004 -> 3, while 0.3 / 0.1 = 2.9999999999999996 -> 2
    assert href.voxel_keys([[0.3, 0.0, 0.0]], 0.1)[0, 0] == 3.0
    vm = href.voxel_map([[0.75, 0.75, 0.75]], 0.5)   # voxel (1, 1, 1)
    assert href.overlap_fitness(vm, [[0.5, 0.5, 0.5]], I4, 0.5) == (1, 1.0)
    assert href.overlap_fitness(vm, [[0.4999999999999999, 0.5, 0.5]], I4, 0.5) == (0, 0.0)


def test_negative_coordinates_floor_towards_minus_infinity():
    assert href.voxel_keys([[-0.01, -0.5, -0.51]], 0.5).tolist() == [[-1.0, -1.0, -2.0]]
    vm = href.voxel_map([[-0.25, -0.25, -0.25]], 0.5)
    assert vm == {(-1, -1, -1)}
    assert href.overlap_fitness(vm, [[-0.01, -0.49, -0.3], [0.01, -0.49, -0.3]], I4, 0.5) == (1, 0.5)


def test_the_pose_is_applied_as_rotation_then_translation():
    Rz = np.array([[0.0, -1.0, 0.0, 2.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, -1.0], [0.0, 0.0, 0.0, 1.0]])
    assert href.isometry_apply(Rz, [[1.0, 0.25, 1.25]]).tolist() == [[1.75, 1.0, 0.25]]
    vm = href.voxel_map([[1.8, 1.2, 0.3]], 0.5)   # voxel (3, 2, 0)
    assert href.overlap_fitness(vm, [[1.0, 0.25, 1.25]], Rz, 0.5) == (1, 1.0)
    assert href.overlap_fitness(vm, [[1.0, 0.25, 1.25]], I4, 0.5) == (0, 0.0)


def test_an_empty_scan_is_nan_and_an_empty_map_is_zero():
    vm = href.voxel_map(lattice(), 0.5)
    n, f = href.overlap_fitness(vm, np.zeros((0, 3)), I4, 0.5)
    assert n == 0 and math.isnan(f)
    assert href.overlap_fitness(href.voxel_map(np.zeros((0, 3)), 0.5), lattice(), I4, 0.5) == (0, 0.0)
    assert href.overlap_fitness(None, lattice(), I4, 0.5) == (0, 0.0)
    n, f = href.overlap_fitness(None, np.zeros((0, 3)), I4, 0.5)
    assert n == 0 and math.isnan(f)


def test_keys_outside_the_packable_range_name_no_voxel():
    far = (href.PACK_BIAS + 0.5) * 0.5
    assert href.packable(href.voxel_keys([[far, 0, 0], [-far, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [far - 0.5, 0, 0]], 0.5)).tolist() == \
        [False, False, False, False, True]
    assert href.voxel_map([[far, 0.0, 0.0]], 0.5) == set()
    vm = href.voxel_map([[0.1, 0.1, 0.1]], 0.5)
    assert href.overlap_fitness(vm, [[far, 0.1, 0.1], [np.nan, 0.1, 0.1], [0.2, 0.2, 0.2]], I4, 0.5) == (1, 1 / 3)


def test_registration_fitness_counts_matches_within_the_radius():
    ids = np.array([4, -1, 7, 2, 9], np.int32)
    d2 = np.array([0.04, np.inf, 0.25, 0.0, 0.2500001], np.float32)
    # r = 0: the chain's max_dist 0.5 -> r2 = 0.25: 0.04, 0.25 (inclusive) and 0 count
    k, f, rmse = href.registration_fitness(ids, d2, 0.0, 0.5)
    assert (k, f) == (3, 0.6)
    assert rmse == math.sqrt((float(np.float32(0.04)) + 0.25) / 3)
    # r = 0.3 -> r2 = fl32(0.09): only 0.04 and 0
    k, f, rmse = href.registration_fitness(ids, d2, 0.3, 0.5)
    assert (k, f) == (2, 0.4) and rmse == math.sqrt(float(np.float32(0.04)) / 2)
    assert href.radius2(0.3, 0.5) == np.float32(np.float32(0.3) * np.float32(0.3))


def test_registration_fitness_without_matches_is_zero_not_nan():
    k, f, rmse = href.registration_fitness(np.full(5, -1), np.full(5, np.inf, np.float32))
    assert (k, f, rmse) == (0, 0.0, 0.0)
    # an unbounded max_dist: +inf <= +inf must not count a point that has no match
    k, f, rmse = href.registration_fitness(np.array([-1, 3]), np.array([np.inf, 4.0], np.float32), 0.0, np.inf)
    assert (k, f, rmse) == (1, 0.5, 2.0)
