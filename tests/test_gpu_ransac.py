"""The device RANSAC registration (include/o3s_registration.h "RANSAC": the contract; csrc/ransac_dev.h) against the numpy
restatement of tests/ransac_ref.py, in stages.  MI355X only.

  1. edge-length outcomes      equal outside the flagged set (o3s_ransac_evaluate_samples, distance checker off)
  2. per-hypothesis T          against umeyama by LAPACK's SVD.  Tolerance: the spread between two independent fp64 restatements
                               (SVD umeyama and Horn's quaternion method) on the test's own 40 000 samples, times 10 for the
                               device's different rotation sequence (one-sided Jacobi).  Measured on the CPU for these samples
                               (ransac_n = 3, the worst-conditioned sample has sigma_2 / sigma_1 = 1.4e-4): largest spread 1.25e-12
                               on a rotation entry and 2.3e-11 m on a translation entry, so the tolerances are 1.25e-11 and
                               2.3e-10 m (ransac_n = 5: 8.7e-14 and 1.2e-12 m, tolerances ten times that); the test recomputes
                               the spreads and asserts with what it computed.
  3. evaluation                given the device's own T, n_in and err2 equal the restatement's bit for bit (sum in the documented
                               chunk order) — for every hypothesis the device evaluated, no exceptions
  4. selection                 given the device's own per-hypothesis table, winner, final est_k and evaluated count equal the
                               serial rule exactly
  5. end to end                table = stream, three and more batch sizes (hooks build), run to run, early exits against the
                               restatement, resident submaps, the loop-closure composition, degenerate inputs

The flagged set (ransac_ref.py) is skipped and nothing else; its share, computed by the restatement alone, must stay <= 1 % of what
is compared, and no hypothesis the serial rule evaluates may be flagged in an end-to-end case."""
import ctypes as C
import os

import numpy as np
import pytest

import ransac_ref as rr
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import registration as reg

pytestmark = pytest.mark.gpu

SIGMA = 0.05
# (K, planted share, seed): the three inputs of tests/test_ransac_ref.py and one whose est_k ends the loop inside the second batch
CASES = [(2000, 0.10, 11), (4000, 0.05, 12), (600, 0.30, 13), (3000, 0.06, 14)]   # est_k on the CPU: 5 716, 36 811, 249, 26 348


def case(K, share, seed):
    src, tgt, corr, T0, planted = rr.planted_case(K, share, seed, SIGMA)
    return src, tgt, corr


def params(seed=0, **kw):
    return reg.RansacParams(seed=seed, **kw)


def test_stage1_edge_length_outcomes():
    src, tgt, corr = case(*CASES[0])
    H, seed = 60000, 5
    out, _, _, _ = reg.ransac_evaluate_samples(src, tgt, corr, params(seed, check_distance=False), count=H)
    rows = rr.sample_indices(seed, np.arange(H), 3, len(corr))
    rec = rr.records(src, tgt, corr)
    rep = rr.repeated(rows)
    S = rec[rows]
    ok, flagged = rr.edge_check(S[..., :3], S[..., 3:], 0.6)
    print(f"hypotheses {H}, repeated {int(rep.sum())}, edge passes {int((ok & ~rep).sum())}, flagged {int(flagged.sum())}")
    assert flagged.mean() <= 0.01
    assert np.array_equal(out == rr.REPEATED, rep)
    keep = ~flagged & ~rep
    assert np.array_equal(out[keep] == rr.EDGE, ~ok[keep]) and (ok & ~rep).sum() > 20
    # a later range of the stream, and the checker switched off: nothing fails on an edge
    out2, _, _, _ = reg.ransac_evaluate_samples(src, tgt, corr, params(seed, check_distance=False), first_iteration=H - 1000, count=2000)
    assert np.array_equal(out2[:1000], out[H - 1000:])
    out3, _, _, _ = reg.ransac_evaluate_samples(src, tgt, corr, params(seed, check_distance=False, check_edge_length=False), count=2000)
    assert np.array_equal(out3 == rr.REPEATED, rep[:2000]) and not (out3 == rr.EDGE).any()


def test_stage2_per_hypothesis_transformation():
    src, tgt, corr = case(*CASES[1])
    rec = rr.records(src, tgt, corr)
    worst = {}
    for n, H in ((3, 30000), (5, 10000)):
        prm = params(9, ransac_n=n, check_distance=False, check_edge_length=False)
        out, T, _, _ = reg.ransac_evaluate_samples(src, tgt, corr, prm, count=H)
        rows = rr.sample_indices(9, np.arange(H), n, len(corr))
        live = ~rr.repeated(rows)
        assert np.array_equal(out == rr.PASS, live)
        S = rec[rows[live]]
        Msvd, ratio = rr.umeyama_svd(S[..., :3], S[..., 3:])
        Mhorn = rr.umeyama_horn(S[..., :3], S[..., 3:])
        keep = ratio >= rr.SIGMA_RATIO
        assert (~keep).mean() <= 0.01
        spread_R = np.abs(Msvd[keep, :3, :3] - Mhorn[keep, :3, :3]).max()
        spread_t = np.abs(Msvd[keep, :3, 3] - Mhorn[keep, :3, 3]).max()
        err_R = np.abs(T[live][keep, :3, :3] - Msvd[keep, :3, :3]).max()
        err_t = np.abs(T[live][keep, :3, 3] - Msvd[keep, :3, 3]).max()
        print(f"ransac_n {n}: {int(keep.sum())} samples, spread SVD/Horn R {spread_R:.2e} t {spread_t:.2e}; device - SVD R {err_R:.2e} t {err_t:.2e}")
        worst[n] = (spread_R, spread_t, err_R, err_t)
        assert np.array_equal(T[live][:, 3], np.tile([0.0, 0, 0, 1], (int(live.sum()), 1)))
        assert (np.abs(np.linalg.det(T[live][keep, :3, :3]) - 1.0) < 1e-12).all()       # proper rotations: the fix-up
    for n, (spread_R, spread_t, err_R, err_t) in worst.items():
        assert err_R <= 10 * spread_R and err_t <= 10 * spread_t, (n, worst[n])


@pytest.mark.parametrize("which,n", [(0, 3), (1, 3), (2, 4)])
def test_stage3_evaluation_bit_for_bit(which, n):
    src, tgt, corr = case(*CASES[which])
    rec = rr.records(src, tgt, corr)
    H = 20000
    # the distance checker off lets more hypotheses through to the evaluation; both settings are compared
    for prm in (params(21, ransac_n=n), params(22, ransac_n=n, check_distance=False, edge_length_similarity=0.9)):
        out, T, n_in, err2 = reg.ransac_evaluate_samples(src, tgt, corr, prm, count=H)
        live = np.flatnonzero(out == rr.PASS)
        assert len(live) > 0
        want_n, want_e, _, _ = rr.evaluate(T[live], rec, prm.max_correspondence_distance)
        print(f"K {len(corr)} ransac_n {n}: {len(live)} evaluated, n_in up to {int(n_in.max())}")
        assert np.array_equal(n_in[live], want_n)
        assert np.array_equal(err2[live], want_e)                        # bit for bit
        dead = out != rr.PASS
        assert not n_in[dead].any() and not err2[dead].any()


def _device_table(src, tgt, corr, prm, n_iter):
    out, T, n_in, err2 = reg.ransac_evaluate_samples(src, tgt, corr, prm, count=n_iter)
    return out == rr.PASS, T, n_in, err2


@pytest.mark.parametrize("confidence,checkers", [(0.999, True), (1.0, True), (0.999, False), (0.9, False), (1.0, False)])
def test_stage4_selection_equals_the_serial_rule(confidence, checkers):
    src, tgt, corr = case(*CASES[0])
    n_iter = 40000 if checkers else 3000
    prm = params(31, max_iteration=n_iter, confidence=confidence, check_distance=checkers, check_edge_length=checkers)
    passed, T, n_in, err2 = _device_table(src, tgt, corr, prm, n_iter)
    want = rr.serial_select(passed, n_in, err2, len(corr), 3, n_iter, confidence)
    got = reg.registration_ransac_based_on_correspondence(src, tgt, corr, prm)
    print(f"confidence {confidence} checkers {checkers}: survivors {int(passed.sum())}, winner {want.best}, est_k {want.est_k}, evaluated {want.evaluated}")
    assert (got.best_iteration, got.est_k, got.evaluated) == (want.best, want.est_k, want.evaluated)
    assert got.fitness == want.fitness and got.inlier_rmse == want.rmse and len(got.correspondence_set) == want.n_in
    assert np.array_equal(got.transformation, T[want.best])
    if confidence == 1.0:
        assert got.est_k == n_iter and got.evaluated == int(passed.sum())


def _same(a, b):
    return ((a.best_iteration, a.est_k, a.evaluated, a.fitness, a.inlier_rmse) == (b.best_iteration, b.est_k, b.evaluated, b.fitness, b.inlier_rmse)
            and np.array_equal(a.transformation, b.transformation) and np.array_equal(a.correspondence_set, b.correspondence_set))


def test_stage5_table_equals_stream_and_runs_repeat():
    src, tgt, corr = case(*CASES[0])
    prm = params(11, max_iteration=100000)
    a = reg.registration_ransac_based_on_correspondence(src, tgt, corr, prm)
    assert 0 <= a.best_iteration < a.est_k < 100000
    tab = rr.sample_indices(11, np.arange(a.est_k + 5000), 3, len(corr))
    b = reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(999, max_iteration=100000), samples=tab)
    assert _same(a, b)
    for _ in range(3):
        assert _same(a, reg.registration_ransac_based_on_correspondence(src, tgt, corr, prm))
    assert not _same(a, reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(12, max_iteration=100000)))
    # the inlier list is the winner's, ascending, and consistent with fitness
    rec = rr.records(src, tgt, corr)
    d = rr.transformed_distance(a.transformation[None], rec)[0]
    assert np.array_equal(a.correspondence_set, corr[d < 0.75]) and a.fitness == len(a.correspondence_set) / len(corr)


def test_stage5_batch_size_does_not_change_the_result():
    """Hooks build: O3S_RANSAC_BATCH is read per call.  8 is smaller than the survivor count of a default batch with the checkers
    off (every non-repeated sample survives) and than that of the checked stream (~15 per 16 384)."""
    src, tgt, corr = case(*CASES[0])
    runs = {}
    with _lib.variant("hooks"):
        try:
            for batch in (8, 1000, 16384, 100000):
                os.environ["O3S_RANSAC_BATCH"] = str(batch)
                runs[batch] = (reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(11, max_iteration=100000)),
                               reg.registration_ransac_based_on_correspondence(
                                   src, tgt, corr, params(11, max_iteration=2500, confidence=0.9, check_distance=False, check_edge_length=False)))
            os.environ["O3S_NO_MAILBOX"] = "1"     # the host learns est_k from a copy of the header instead of the post
            os.environ["O3S_RANSAC_BATCH"] = "1000"
            no_post = reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(11, max_iteration=100000))
        finally:
            os.environ.pop("O3S_RANSAC_BATCH", None)
            os.environ.pop("O3S_NO_MAILBOX", None)
    prod = reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(11, max_iteration=100000))
    for batch, (a, b) in runs.items():
        assert _same(a, prod), batch
        assert _same(b, runs[8][1]), batch
    assert _same(no_post, prod)
    assert prod.est_k % 1000 != 0 and prod.est_k > 16384 // 4


@pytest.mark.parametrize("K,share,seed", CASES)
def test_stage5_early_exit_equals_the_restatement(K, share, seed):
    src, tgt, corr = case(K, share, seed)
    want = rr.ransac(src, tgt, corr, seed=seed)
    print(f"K {K}: est_k {want.est_k}, winner {want.best_iteration}, evaluated {want.evaluated}, inliers {len(want.inliers)}, "
          f"flagged evaluated {want.flagged_evaluated}, flagged below est_k {want.flagged_below_est_k}, margin {want.min_margin:.2e}")
    assert want.flagged_evaluated == 0 and want.flagged_below_est_k <= 0.01 * want.est_k      # conditions on the input, CPU only
    got = reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(seed))
    assert (got.best_iteration, got.est_k, got.evaluated) == (want.best_iteration, want.est_k, want.evaluated)
    assert np.array_equal(got.correspondence_set, corr[want.inliers]) and got.fitness == want.fitness
    assert np.abs(got.transformation - want.transformation).max() < 1e-9 and abs(got.inlier_rmse - want.inlier_rmse) < 1e-9
    assert want.est_k % 16384 not in (0, 16383) and 0 < want.est_k < 10_000_000
    if seed == 14:
        assert 16384 < want.est_k < 2 * 16384        # the loop ends in the middle of the second batch


def test_degenerate_inputs_and_bad_parameters():
    src, tgt, corr = case(*CASES[2])
    empty = lambda r: (r.best_iteration == -1 and r.fitness == 0 and r.inlier_rmse == 0 and len(r.correspondence_set) == 0
                       and np.array_equal(r.transformation, np.eye(4)))
    assert empty(reg.registration_ransac_based_on_correspondence(src, tgt, corr[:2], params()))                 # K < ransac_n
    assert empty(reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(ransac_n=2)))
    assert empty(reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(max_correspondence_distance=0.0)))
    assert empty(reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(max_iteration=0)))
    r = reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(), samples=[[1, 1, 2], [3, 4, 3], [5, 5, 5]])
    assert empty(r) and r.evaluated == 0 and r.est_k == 3                                                        # all samples repeated
    # no survivor: similarity 1 asks for equal edge lengths, which unrelated pairs never have
    rng = np.random.default_rng(2)
    r = reg.registration_ransac_based_on_correspondence(rng.random((500, 3)) * 50, rng.random((500, 3)) * 50, corr[:500],
                                                        params(max_iteration=20000, edge_length_similarity=1.0))
    assert empty(r) and r.evaluated == 0 and r.est_k == 20000
    for bad in (params(ransac_n=9), params(confidence=1.5), params(confidence=-0.1), params(max_iteration=-1)):
        with pytest.raises(ValueError):
            reg.registration_ransac_based_on_correspondence(src, tgt, corr, bad)
    far = corr.copy()
    far[7, 1] = len(tgt)                                      # a correspondence that names no point
    with pytest.raises(ValueError):
        reg.registration_ransac_based_on_correspondence(src, tgt, far, params())
    with pytest.raises(ValueError):
        reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(), samples=[[0, 1, len(corr)]])
    with pytest.raises(ValueError):
        reg.ransac_evaluate_samples(src, tgt, corr[:2], params(), count=10)
    L = reg._L()
    res, prm = reg._RansacResult(), params().to_c()
    assert L.o3s_registration_ransac_correspondence(0, None, 0, None, 0, None, 0, None, None, 0, C.byref(res), None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_registration_ransac_correspondence(0, None, 0, None, 0, None, 0, C.byref(prm), None, 0, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_submap_registration_ransac(None, None, 1, C.byref(prm), C.byref(res), None, None) == _lib.ERR_BAD_ARGUMENT
    d = reg.default_ransac_params()
    assert (d.max_correspondence_distance, d.ransac_n, d.distance_threshold, d.edge_length_similarity, d.max_iteration, d.confidence) == \
        (0.75, 3, 0.8, 0.6, 10_000_000, 0.999) and d == reg.RansacParams()
    reg.ransac_reserve(5000)
    a = reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(13))
    reg.ransac_release()
    assert _same(a, reg.registration_ransac_based_on_correspondence(src, tgt, corr, params(13)))


def test_resident_submaps_and_the_loop_closure_composition():
    from test_gpu_features import BIG, map_cloud, two_overlapping_submaps
    from open3d_slam_advanced_rss_2024_public_amd import Submap

    a, b = two_overlapping_submaps()
    L = reg._L()
    res, prm = reg._RansacResult(), params().to_c()
    assert L.o3s_submap_registration_ransac(a._h, b._h, 1, C.byref(prm), C.byref(res), None, None) == _lib.ERR_NOT_INITIALIZED
    with pytest.raises(RuntimeError):
        a.ransacRegistration(b)                      # missing features
    a.computeFeatures()
    assert L.o3s_submap_registration_ransac(a._h, b._h, 1, C.byref(prm), C.byref(res), None, None) == _lib.ERR_NOT_INITIALIZED
    b.computeFeatures()
    got = a.ransacRegistration(b, params(3))
    pa, pb = a.getSparseMapPointCloud()[0], b.getSparseMapPointCloud()[0]
    host = reg.registration_ransac_based_on_feature_matching(pa, pb, a.getFeatures(), b.getFeatures(), True, params(3))
    print(f"K {got.n_correspondences}, est_k {got.est_k}, winner {got.best_iteration}, inliers {len(got.correspondence_set)}, rmse {got.inlier_rmse:.3f}")
    assert _same(got, host) and got.n_correspondences == host.n_correspondences == len(a.featureCorrespondences(b, True, 3)[0])
    # both submaps are cut from one map in one frame: ground truth is the identity.  The RANSAC pose must lie where the overlap
    # refinement converges to it; the overlap's points are the SAME points in both submaps, so the identity is the refinement's exact
    # minimum.  Bounds from the map's noise: sigma = 0.01 m on the translation, sigma over the map's 15 m half-width on a rotation entry
    assert got.best_iteration >= 0 and len(got.correspondence_set) >= 25
    c = reg.loop_closure_constraint(a, b, params(3), overlap_voxel_size=20 * 0.1, registration_type="PointToPointIcp")
    assert c.rejected is None, c.rejected
    print(f"refinement fitness {c.refinement.fitness:.3f} rmse {c.refinement.inlier_rmse:.2e} overlap {c.n_overlap}")
    assert _same(c.ransac, got)
    assert c.refinement.fitness >= 0.7 and np.abs(c.source_to_target[:3, 3]).max() < 0.01 and np.abs(c.source_to_target[:3, :3] - np.eye(3)).max() < 0.01 / 15.0
    assert c.information_matrix.shape == (6, 6) and np.allclose(c.information_matrix, c.information_matrix.T) and c.information_matrix[3, 3] > 100
    # A pair with nothing in common.  Two disjoint parts of THIS map will not do: the room is a square with a regular pillar grid, so
    # its halves are congruent under a half turn and a closure between them is a correct answer (fitness 0.85 when it was tried).  The
    # target is therefore a surface no rigid motion lays on the room: an undulating terrain with incommensurate wavelengths
    rng = np.random.default_rng(5)
    xy = rng.uniform(-15.0, 15.0, (200000, 2))
    z = 3.0 + 1.5 * np.sin(xy[:, 0] / 3.1) + 1.2 * np.cos(xy[:, 1] / 2.3) + 0.8 * np.sin((xy[:, 0] + xy[:, 1]) / 1.7)
    far = Submap(0.1, BIG)
    far.setMapPointCloud(np.ascontiguousarray(np.column_stack([xy, z + rng.normal(0.0, 0.01, len(z))])), None)
    assert far.computeFeatures() > 2000
    cf = reg.loop_closure_constraint(a, far, params(3, max_iteration=1_000_000), overlap_voxel_size=20 * 0.1, registration_type="PointToPointIcp")
    print(f"ransac inliers {len(cf.ransac.correspondence_set)} of {cf.ransac.n_correspondences}, est_k {cf.ransac.est_k}, "
          f"refinement {None if cf.refinement is None else cf.refinement.fitness}")
    print(f"non-overlapping pair: {cf.rejected}")
    assert cf.rejected is not None and cf.source_to_target is None
