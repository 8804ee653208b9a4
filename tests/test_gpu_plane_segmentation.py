"""RANSAC plane segmentation on the device (include/plane_segmentation/o3s_plane_segmentation.h) against the numpy restatement of its
contract (tests/plane_ref.py), stage by stage through o3s_plane_evaluate_samples, then end to end.  MI355X only.

Every comparison is exact: the results are integers, or fp64 values formed by +, -, x, / and sqrt in a pinned order.  n_in and err
are compared GIVEN THE DEVICE'S OWN PLANES (as tests/test_gpu_ransac.py does with T), and the planes themselves are compared too —
exactly; a last-bit difference in a plane would show there and nowhere else.

  1. outcomes     an explicit table with repeated, non-finite, collinear and good rows
  2. evaluation   n_in and err bit for bit across the chunk (512 points) and block (64 hypotheses) edges
  3. selection    table = stream; batch sizes in the hooks build equal the product build; an early stop inside the second batch; the tie
                  on n_in that err decides
  4. end to end   non-finite rows in the cloud, a threshold so small that a sample's own points are its only inliers, run to run
  5. the peel     three planted planes plus noise, and min_inliers ends it"""
import os

import numpy as np
import pytest

import plane_ref as pr
from cloud_edge_cases import non_finite_points
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from test_plane_ref import tie_cloud

pytestmark = pytest.mark.gpu

THR = 0.05


def planted(N, seed, share=0.6, sigma=0.01):
    """uniform points in a 20 x 20 x 6 box, a share of them moved onto z = 0.3 x - 0.2 y + 1 (sigma noise along z), in random order"""
    rng = np.random.default_rng(seed)
    p = (rng.random((N, 3)) - 0.5) * [20.0, 20.0, 6.0]
    on = rng.random(N) < share
    p[on, 2] = 0.3 * p[on, 0] - 0.2 * p[on, 1] + 1.0 + sigma * rng.standard_normal(int(on.sum()))
    return p


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_stages(pts, thr, rows, dev):
    """(outcome, planes, n_in, err) of the device against the restatement for the sample rows"""
    outcome, planes, n_in, err = dev
    ro, rp, _, _ = pr.evaluate_samples(pts, rows, thr)
    assert np.array_equal(outcome, ro)
    assert np.array_equal(planes, rp), np.abs(planes - rp).max()
    _, _, rn, re = pr.evaluate_samples(pts, rows, thr, given_planes=planes)
    assert np.array_equal(n_in, rn)
    assert np.array_equal(err, re), np.abs(err - re).max()
    return ro


def check_result(r, ref):
    assert (r.best_iteration, r.est_k, r.evaluated) == (ref.best_iteration, ref.est_k, ref.evaluated)
    assert np.array_equal(r.inliers, ref.inliers) and r.inliers.dtype == np.int64
    assert np.array_equal(r.plane_model, ref.model), (r.plane_model, ref.model)


def same_result(a, b):
    return ((a.best_iteration, a.est_k, a.evaluated) == (b.best_iteration, b.est_k, b.evaluated) and same(a.inliers, b.inliers) and
            same(a.plane_model, b.plane_model))


# ---- 1. outcomes ---------------------------------------------------------------------------------------------------------------------

def test_stage_outcomes_of_an_explicit_table():
    bad = non_finite_points()                                   # 12 rows, the first is finite
    pts = np.concatenate([planted(700, 1), bad, [[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [4.0, 4.0, 4.0]]])
    nb, col = 700, 700 + len(bad)
    rows = np.array([[0, 1, 2], [5, 5, 9], [nb + 1, 3, 4], [3, nb + 4, 4], [3, 4, nb + 11], [col, col + 1, col + 2], [10, 20, 30],
                     [nb + 2, nb + 2, 7], [col, col, col], [699, 0, nb], [40, 41, 40], [col + 2, col, col + 1]], np.int32)
    ro = check_stages(pts, THR, rows, co.plane_evaluate_samples(pts, THR, samples=rows))
    P, R, F, D = pr.PASS, pr.REPEATED, pr.NONFINITE, pr.DEGENERATE
    assert list(ro) == [P, R, F, F, F, D, P, R, R, P, R, D]
    # ransac_n 5: only the first three define the plane and must be finite, all five must differ
    rows5 = np.array([[0, 1, 2, nb + 1, nb + 2], [0, 1, 2, 3, 2], [nb + 1, 1, 2, 3, 4], [6, 7, 8, 9, 10]], np.int32)
    ro = check_stages(pts, THR, rows5, co.plane_evaluate_samples(pts, THR, ransac_n=5, samples=rows5))
    assert list(ro) == [P, R, F, P]


# ---- 2. evaluation -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [3, 63, 64, 65, 511, 512, 513, 1537, 5000])
def test_stage_counts_and_err_across_the_chunk_edges(N):
    pts = planted(N, 10 + N)
    H = 65
    rows = pr.sample_indices(5, np.arange(H), 3, N)
    ro = check_stages(pts, THR, rows, co.plane_evaluate_samples(pts, THR, seed=5, count=H))
    assert (ro == pr.PASS).any() and ((ro == pr.REPEATED).any() or N > 65)
    if N >= 64:   # a later window of the stream, and four indices per sample (the fourth only has to differ)
        rows = pr.sample_indices(5, np.arange(1000, 1000 + H), 4, N)
        check_stages(pts, THR, rows, co.plane_evaluate_samples(pts, THR, ransac_n=4, seed=5, first_iteration=1000, count=H))


@pytest.mark.parametrize("H", [1, 63, 64, 65, 1000])
def test_stage_counts_and_err_across_the_block_edges(H):
    N = 1537
    pts = planted(N, 3)
    rows = pr.sample_indices(2 ** 40 + 9, np.arange(H), 3, N)   # a seed with a high word
    check_stages(pts, THR, rows, co.plane_evaluate_samples(pts, THR, seed=2 ** 40 + 9, count=H))
    check_stages(pts, THR, rows, co.plane_evaluate_samples(pts, THR, samples=rows))


def test_stage_batches_and_block_sizes_of_the_hooks_build_change_nothing():
    N, H = 1537, 300
    pts = planted(N, 4)
    prod = co.plane_evaluate_samples(pts, THR, seed=1, count=H)
    with _lib.variant("hooks"):
        try:
            for batch, block in ((8, 64), (64, 128), (1000, 256), (100000, 64)):
                os.environ["O3S_PLANE_BATCH"], os.environ["O3S_PLANE_EVAL_BLOCK"] = str(batch), str(block)
                got = co.plane_evaluate_samples(pts, THR, seed=1, count=H)
                assert all(same(a, b) for a, b in zip(got, prod)), (batch, block)
        finally:
            os.environ.pop("O3S_PLANE_BATCH", None)
            os.environ.pop("O3S_PLANE_EVAL_BLOCK", None)


# ---- 3. selection --------------------------------------------------------------------------------------------------------------------

def test_selection_with_table_equal_to_the_stream():
    N = 1537
    pts = planted(N, 6)
    ref = pr.segment_plane(pts, THR, 3, 200, 1.0, seed=21)
    assert ref.best_iteration >= 0 and 0.5 * N < len(ref.inliers) < 0.7 * N and ref.evaluated <= 200 == ref.est_k
    r = co.segment_plane(pts, THR, 3, 200, 1.0, seed=21)
    check_result(r, ref)
    t = co.segment_plane(pts, THR, 3, 200, 1.0, seed=99, samples=pr.sample_indices(21, np.arange(200), 3, N))
    assert same_result(t, r)
    short = co.segment_plane(pts, THR, 3, 200, 1.0, samples=pr.sample_indices(21, np.arange(50), 3, N))   # min(num_iterations, H) rows
    check_result(short, pr.segment_plane(pts, THR, 3, 200, 1.0, samples=pr.sample_indices(21, np.arange(50), 3, N)))
    assert short.est_k == 50
    # the refit is not the sample's plane: the list is the sample's, the model the list's
    assert np.array_equal(r.inliers, np.flatnonzero(pr.distances(ref.plane[None], pts)[0] < THR)) and not np.array_equal(r.plane_model, ref.plane)


def test_batch_size_does_not_change_the_result():
    """Hooks build: O3S_PLANE_BATCH is read per call.  With confidence < 1 and batches of 8 the host also reads est_k back and stops
    issuing; the product build runs the same iterations as one batch."""
    N = 1537
    pts = planted(N, 7)
    want = [pr.segment_plane(pts, THR, 3, 1000, 1.0, seed=3), pr.segment_plane(pts, THR, 3, 1000, 0.99, seed=3),
            pr.segment_plane(pts, THR, 4, 1000, 0.999, seed=4)]
    assert want[0].est_k == 1000 and 10 < want[1].est_k < 100 and want[1].est_k < want[2].est_k < 1000

    def runs():
        return [co.segment_plane(pts, THR, 3, 1000, 1.0, seed=3), co.segment_plane(pts, THR, 3, 1000, 0.99, seed=3),
                co.segment_plane(pts, THR, 4, 1000, 0.999, seed=4)]

    prod = runs()
    for r, ref in zip(prod, want):
        check_result(r, ref)
    with _lib.variant("hooks"):
        try:
            for batch in (8, 64, 1000, 100000):
                os.environ["O3S_PLANE_BATCH"] = str(batch)
                for r, p in zip(runs(), prod):
                    assert same_result(r, p), batch
        finally:
            os.environ.pop("O3S_PLANE_BATCH", None)


def test_an_early_stop_inside_the_second_batch():
    """A planted 60 % plane and confidence 0.99: r^3 = 0.216 gives est_k = ceil(log 0.01 / log 0.784) = 19 once a sample lies on the
    plane.  The batch is chosen so that est_k falls inside the second one: its kernels start, the rule stops in their middle."""
    N = 5000
    pts = planted(N, 8)
    ref = pr.segment_plane(pts, THR, 3, 1000, 0.99, seed=12)
    batch = (2 * ref.est_k + 2) // 3
    assert 15 <= ref.est_k <= 25 and batch < ref.est_k < 2 * batch and batch <= ref.best_iteration and len(ref.trace) >= 3   # replacements in both batches
    with _lib.variant("hooks"):
        try:
            os.environ["O3S_PLANE_BATCH"] = str(batch)
            check_result(co.segment_plane(pts, THR, 3, 1000, 0.99, seed=12), ref)
        finally:
            os.environ.pop("O3S_PLANE_BATCH", None)
    check_result(co.segment_plane(pts, THR, 3, 1000, 0.99, seed=12), ref)


def test_a_tie_on_the_count_is_decided_by_err():
    pts = tie_cloud()
    wide, tight = [0, 4, 1], [24, 28, 25]
    _, _, n_in, err = co.plane_evaluate_samples(pts, 0.5, samples=[wide, tight])
    assert list(n_in) == [24, 24] and list(err) == [3.0, 1.5]
    for rows, best in (([wide, tight], 1), ([tight, wide], 0), ([wide, wide], 0), ([wide, tight, wide, tight], 1)):
        r = co.segment_plane(pts, 0.5, samples=rows)
        check_result(r, pr.segment_plane(pts, 0.5, samples=rows))
        assert r.best_iteration == best


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------------

def test_a_cloud_with_non_finite_rows():
    bad = non_finite_points()[1:]
    pts = planted(1537, 9)
    where = np.r_[0, 5, 511, 512, 513, 1000:1005, 1536]
    pts[where] = bad
    ref = pr.segment_plane(pts, THR, 3, 300, 1.0, seed=2)
    assert ref.best_iteration >= 0 and not np.isin(where, ref.inliers).any()
    check_result(co.segment_plane(pts, THR, 3, 300, 1.0, seed=2), ref)
    rows = pr.sample_indices(2, np.arange(300), 3, len(pts))
    ro = check_stages(pts, THR, rows, co.plane_evaluate_samples(pts, THR, seed=2, count=300))
    assert (ro == pr.NONFINITE).any()
    allbad = np.tile(bad, (3, 1))                                                  # nothing can pass
    r = co.segment_plane(allbad, THR, 3, 50, 1.0)
    check_result(r, pr.segment_plane(allbad, THR, 3, 50, 1.0))
    assert r.best_iteration == -1 and not r.plane_model.any() and len(r.inliers) == 0


def test_a_threshold_so_small_that_a_samples_own_points_are_its_only_inliers():
    N = 1537
    rng = np.random.default_rng(11)
    pts = (rng.random((N, 3)) - 0.5) * 20.0
    thr = 1e-11
    rows = pr.sample_indices(0, np.arange(200), 3, N)
    _, _, n_in, _ = co.plane_evaluate_samples(pts, thr, count=200)
    ro = check_stages(pts, thr, rows, co.plane_evaluate_samples(pts, thr, count=200))
    assert n_in[ro == pr.PASS].max() == 3 and n_in[ro == pr.PASS].min() >= 1       # p0 always: its distance is exactly 0
    ref = pr.segment_plane(pts, thr, 3, 200, 1.0)
    r = co.segment_plane(pts, thr, 3, 200, 1.0)
    check_result(r, ref)
    assert len(r.inliers) == 3 and np.array_equal(np.sort(rows[r.best_iteration]), r.inliers)


def test_run_to_run_and_default_arguments():
    pts = planted(5000, 13)
    a = co.segment_plane(pts, THR)
    check_result(a, pr.segment_plane(pts, THR))
    model, inliers = a
    assert model.shape == (4,) and a.est_k == 100
    for _ in range(2):
        assert same_result(co.segment_plane(pts, THR), a)
    with pytest.raises(RuntimeError):
        co.segment_plane(pts, 0.0)
    with pytest.raises(RuntimeError):
        co.segment_plane(pts, THR, samples=[[0, 1, len(pts)]])


# ---- 5. the peel ---------------------------------------------------------------------------------------------------------------------

def three_planes(N=5000, seed=17):
    """45 % on z = 0.3 x - 0.2 y + 1, 25 % on x = 4 + 0.1 z, 15 % on y = -5, the rest uniform; shuffled, with a NaN row and an inf row"""
    rng = np.random.default_rng(seed)
    p = (rng.random((N, 3)) - 0.5) * [20.0, 20.0, 6.0]
    u = rng.random(N)
    a, b, c = u < 0.45, (u >= 0.45) & (u < 0.70), (u >= 0.70) & (u < 0.85)
    p[a, 2] = 0.3 * p[a, 0] - 0.2 * p[a, 1] + 1.0 + 0.01 * rng.standard_normal(int(a.sum()))
    p[b, 0] = 4.0 + 0.1 * p[b, 2] + 0.01 * rng.standard_normal(int(b.sum()))
    p[c, 1] = -5.0 + 0.01 * rng.standard_normal(int(c.sum()))
    p[77] = [np.nan, 0.0, 0.0]
    p[4 * N // 5] = [1.0, np.inf, 2.0]
    return p


def test_peel_of_three_planted_planes_and_min_inliers_ends_it():
    pts = three_planes()
    N = len(pts)
    kw = dict(ransac_n=3, num_iterations=100, confidence=1.0, seed=31)
    rl, rm, rc = pr.segment_planes(pts, THR, 4, min_inliers=300, **kw)
    assert len(rc) == 3 and 0.40 * N < rc[0] and 0.2 * N < rc[1] < rc[0] and 0.1 * N < rc[2] < rc[1]   # the fourth plane finds too little
    labels, models, counts = co.segment_planes(pts, THR, 4, min_inliers=300, **kw)
    assert labels.dtype == np.int32 and np.array_equal(labels, rl)
    assert np.array_equal(models, rm), (models, rm)
    assert np.array_equal(counts, rc) and counts.dtype == np.int64
    assert labels[77] == -1 and labels[4000] == -1 and np.array_equal(np.bincount(labels[labels >= 0]), rc)
    # max_planes ends it earlier; min_inliers 3 lets a fourth plane through the noise in
    for max_planes, min_inliers in ((2, 300), (1, 300), (4, 3), (3, 10 ** 6)):
        got = co.segment_planes(pts, THR, max_planes, min_inliers=min_inliers, **kw)
        want = pr.segment_planes(pts, THR, max_planes, min_inliers=min_inliers, **kw)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (max_planes, min_inliers)
        assert len(got[2]) == {(2, 300): 2, (1, 300): 1, (4, 3): 4, (3, 10 ** 6): 0}[(max_planes, min_inliers)]
    # plane 0 of the peel is the single segmentation
    one = co.segment_plane(pts, THR, **kw)
    assert np.array_equal(one.plane_model, models[0]) and np.array_equal(one.inliers, np.flatnonzero(labels == 0))
    # fewer points than a sample, and an early stop per plane
    few = co.segment_planes(pts[:2], THR, 4, **kw)
    assert list(few[0]) == [-1, -1] and len(few[2]) == 0
    kw["confidence"] = 0.99
    got, want = co.segment_planes(pts, THR, 4, min_inliers=300, **kw), pr.segment_planes(pts, THR, 4, min_inliers=300, **kw)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_a_reserved_area_serves_every_call_without_growing():
    pts = three_planes(5000, 18)
    co.plane_release()
    assert co.plane_device_bytes() == 0
    co.plane_reserve(5000, 100)
    held = co.plane_device_bytes()
    assert held > 5000 * 24
    a = co.segment_planes(pts, THR, 4, min_inliers=300, seed=1)
    assert co.plane_device_bytes() == held
    co.segment_plane(pts[:3000], THR, seed=1)
    b = co.segment_planes(pts, THR, 4, min_inliers=300, seed=1)
    assert co.plane_device_bytes() == held and all(same(x, y) for x, y in zip(a, b))
    co.plane_release()
    co.plane_release()                                        # twice is fine
    assert co.plane_device_bytes() == 0
    c = co.segment_planes(pts, THR, 4, min_inliers=300, seed=1)   # an area made on demand: the same bits, and the second call allocates nothing
    grown = co.plane_device_bytes()
    d = co.segment_planes(pts, THR, 4, min_inliers=300, seed=1)
    assert 0 < grown == co.plane_device_bytes() and all(same(x, y) for x, y in zip(a, c)) and all(same(x, y) for x, y in zip(a, d))
