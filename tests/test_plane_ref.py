"""Known answers of tests/plane_ref.py, the restatement the device plane segmentation is held to
(include/plane_segmentation/o3s_plane_segmentation.h).  CPU only; everything is exact: lattice coordinates make every product and sum
representable."""
import numpy as np

import plane_ref as pr
from ransac_ref import sample_indices as ransac_sample_indices


def lattice_plane(nx, ny, z=0.0, x0=0.0, y0=0.0):
    g = np.stack(np.meshgrid(np.arange(nx, dtype=np.float64) + x0, np.arange(ny, dtype=np.float64) + y0, indexing="ij"), axis=-1).reshape(-1, 2)
    return np.concatenate([g, np.full((len(g), 1), z)], axis=1)


def test_plane_zero_of_the_stream_is_the_registration_stream():
    it = np.arange(50)
    assert np.array_equal(pr.sample_indices(7, it, 5, 1234, 0), ransac_sample_indices(7, it, 5, 1234))
    assert not np.array_equal(pr.sample_indices(7, it, 5, 1234, 1), pr.sample_indices(7, it, 5, 1234, 0))


def test_lattice_plane_with_planted_samples():
    plane = lattice_plane(6, 5)                                      # 30 points on z = 0
    off = np.array([[0.0, 0.0, 3.0], [2.0, 1.0, -4.0], [5.0, 5.0, 2.0], [1.0, 3.0, 0.5]])
    pts = np.concatenate([off[:2], plane, off[2:]])
    on = np.arange(2, 32)
    samples = [[0, 5, 33], [2, 2 + 5, 2 + 1], [2 + 7, 2 + 20, 2 + 3]]   # one through the strays, two on the lattice
    r = pr.segment_plane(pts, 0.25, 3, 100, 1.0, samples=samples)
    assert r.best_iteration == 1 and r.evaluated == 3 and r.est_k == 3
    assert np.array_equal(np.abs(r.plane), [0.0, 0.0, 1.0, 0.0])
    assert np.array_equal(np.abs(r.model), [0.0, 0.0, 1.0, 0.0])
    assert np.array_equal(r.inliers, on)
    # the threshold is strict: a point at exactly the threshold is no inlier
    r = pr.segment_plane(pts, 0.5, 3, 100, 1.0, samples=samples)
    assert np.array_equal(r.inliers, on)
    r = pr.segment_plane(pts, 0.5 + 2.0 ** -40, 3, 100, 1.0, samples=samples)
    assert np.array_equal(r.inliers, np.arange(2, 33 + 1)[np.r_[0:30, 31]])


def test_outcomes_in_their_order():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [0.0, 1.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 1.0], [3.0, 0.0, 1.0]])
    rows = [[0, 1, 2],        # collinear
            [0, 1, 3],        # good
            [0, 0, 3],        # repeated
            [0, 4, 3],        # NaN among the first three
            [4, 4, 3],        # repeated comes before non-finite
            [5, 1, 3],        # inf
            [0, 0, 0]]        # repeated comes before degenerate
    out, planes, n_in, err = pr.evaluate_samples(pts, rows, 0.1)
    assert list(out) == [pr.DEGENERATE, pr.PASS, pr.REPEATED, pr.NONFINITE, pr.REPEATED, pr.NONFINITE, pr.REPEATED]
    assert (planes[out != pr.PASS] == 0).all() and (n_in[out != pr.PASS] == 0).all() and (err[out != pr.PASS] == 0).all()
    # the plane through (0,0,0), (1,1,1), (0,1,0): n = e0 x e1 = (1,1,1) x (0,1,0) = (-1, 0, 1)
    s = 1.0 / np.sqrt(2.0)
    assert np.array_equal(planes[1], [-1.0 / np.sqrt(2.0), 0.0, s, 0.0])
    assert n_in[1] == 4          # the three collinear points and (0,1,0); the non-finite points never are
    # with ransac_n 4 only the first three must be finite, but all four distinct
    out4, _, _, _ = pr.evaluate_samples(pts, [[0, 1, 3, 4], [0, 1, 3, 3], [0, 1, 3, 6]], 0.1)
    assert list(out4) == [pr.PASS, pr.REPEATED, pr.PASS]
    assert pr.segment_plane(pts[:2], 0.1).best_iteration == -1                    # M < ransac_n
    r = pr.segment_plane(pts, 0.1, samples=[[0, 1, 2], [0, 0, 1]])                # nothing passes
    assert r.best_iteration == -1 and r.evaluated == 0 and r.est_k == 2 and not r.model.any() and len(r.inliers) == 0


def tie_cloud():
    """Two parallel lattice planes with 24 inliers each under threshold 0.5: around z = 0 the off-plane points lie at +-0.25, around
    z = 8 at +-0.125 — equal counts, err 12 * 0.25 = 3.0 against 12 * 0.125 = 1.5."""
    a = lattice_plane(6, 4)
    a[12:, 2] = np.where(np.arange(12) % 2 == 0, 0.25, -0.25)
    b = lattice_plane(6, 4, z=8.0, x0=10.0)
    b[12:, 2] += np.where(np.arange(12) % 2 == 0, 0.125, -0.125)
    return np.concatenate([a, b])


def test_a_tie_on_the_count_is_decided_by_err():
    pts = tie_cloud()
    wide, tight = [0, 4, 1], [24, 28, 25]                            # exact samples on z = 0 and on z = 8
    out, planes, n_in, err = pr.evaluate_samples(pts, [wide, tight], 0.5)
    assert list(n_in) == [24, 24] and list(err) == [3.0, 1.5]
    r = pr.segment_plane(pts, 0.5, samples=[wide, tight])
    assert r.best_iteration == 1 and np.array_equal(r.inliers, np.arange(24, 48)) and len(r.trace) == 2
    r = pr.segment_plane(pts, 0.5, samples=[tight, wide])
    assert r.best_iteration == 0 and np.array_equal(r.inliers, np.arange(24, 48)) and len(r.trace) == 1
    r = pr.segment_plane(pts, 0.5, samples=[wide, wide])             # equal rmse: the earlier one stays
    assert r.best_iteration == 0


def test_est_k_by_hand():
    """10 points, 6 on a plane, ransac_n 3, confidence 0.9: r = 0.6, r^3 = 0.216, log(0.1) / log(0.784) = 9.46.. -> est_k = 10"""
    pts = np.concatenate([lattice_plane(3, 2), [[0.0, 0.0, 5.0], [1.0, 0.0, 7.0], [0.0, 1.0, 9.0], [2.0, 2.0, 11.0]]])
    samples = [[0, 1, 3]] * 40
    r = pr.segment_plane(pts, 0.5, 3, 40, 0.9, samples=samples)
    assert 9.4 < np.log(0.1) / np.log(1 - 0.216) < 9.5
    assert r.trace == [(0, 10)] and r.est_k == 10 and r.evaluated == 10 and r.best_iteration == 0
    r = pr.segment_plane(pts, 0.5, 3, 40, 1.0, samples=samples)     # confidence 1 never stops early
    assert r.est_k == 40 and r.evaluated == 40
    r = pr.segment_plane(pts, 0.5, 3, 5, 0.9, samples=samples)      # est_k only ever shrinks
    assert r.est_k == 5 and r.evaluated == 5


def test_refit_of_a_unit_square_through_the_three_branches():
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    for axis, h in ((0, 2.0), (1, -3.0), (2, 0.5)):
        q = np.insert(sq, axis, h, axis=1)
        want = np.zeros(4)
        want[axis], want[3] = 1.0, -h            # det of the two in-plane axes = 1 * 1 - 0, the others 0: the normal is the axis
        assert np.array_equal(pr.refit(q), want), axis
    # a tilted square, x = z: xx = zz = xz = 1, yy = 1 -> det_x = det_z = 1 * 1 - 0 and det_y = 0: the last branch, normal (-1, 0, 1) / sqrt 2
    q = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 1.0, 1.0]])
    m = pr.refit(q)
    assert np.array_equal(m, [-1.0 / np.sqrt(2.0), 0.0, 1.0 / np.sqrt(2.0), 0.0])
    assert not pr.refit(np.array([[1.0, 2.0, 3.0]])).any()           # one point: zero norm -> (0, 0, 0, 0)
    # chunk order: 1300 inliers are three chunks
    rng = np.random.default_rng(3)
    q = np.concatenate([rng.random((1300, 2)), np.zeros((1300, 1))], axis=1)
    assert np.array_equal(np.abs(pr.refit(q)), [0.0, 0.0, 1.0, 0.0])
    v = rng.random(1300)
    parts = [np.cumsum(v[k:k + 512])[-1] for k in (0, 512, 1024)]
    assert pr.chunk_sum(v) == (np.float64(0.0) + parts[0] + parts[1]) + parts[2]


def test_peel_of_two_planes_and_min_inliers_cuts_the_third():
    rng = np.random.default_rng(5)
    a, b = lattice_plane(8, 6), lattice_plane(6, 5, z=0.0)[:, [2, 0, 1]] + [20.0, 0.0, 3.0]   # 48 on z = 0, 30 on x = 20
    noise = rng.random((7, 3)) * 40.0 + 50.0
    pts = np.concatenate([noise[:3], a, noise[3:5], b, noise[5:]])
    ia, ib = np.arange(3, 51), np.arange(53, 83)
    labels, models, counts = pr.segment_planes(pts, 0.01, 4, min_inliers=8, num_iterations=300, seed=11)
    assert list(counts) == [48, 30] and models.shape == (2, 4)
    assert (labels[ia] == 0).all() and (labels[ib] == 1).all() and (labels == -1).sum() == 7
    assert np.array_equal(np.abs(models[0]), [0.0, 0.0, 1.0, 0.0]) and np.array_equal(np.abs(models[1]), [1.0, 0.0, 0.0, 20.0])
    # with min_inliers 3 a third "plane" through three strays is reported as well
    labels3, models3, counts3 = pr.segment_planes(pts, 0.01, 3, min_inliers=3, num_iterations=300, seed=11)
    assert len(counts3) == 3 and list(counts3[:2]) == [48, 30] and counts3[2] >= 3 and np.array_equal(labels3 >= 0, (labels >= 0) | (labels3 == 2))
    # plane 1 is a segmentation of the compacted remainder with the stream of plane 1
    left = np.flatnonzero(labels != 0)
    r1 = pr.segment_plane(pts[left], 0.01, 3, 300, 1.0, 11, plane=1)
    assert np.array_equal(left[r1.inliers], ib) and np.array_equal(r1.model, models[1])
