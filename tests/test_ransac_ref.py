"""Pins the numpy restatement of the RANSAC contract (tests/ransac_ref.py; contract: include/o3s_registration.h "RANSAC") on the
CPU: the sample stream, umeyama, the checkers, the serial selection rule and the recovery of a planted pose.

Philox4x32-10: the known-answer vectors are Random123's (kat_vectors); the zero vector and a second one were confirmed against an
independent implementation (ATen's at::Philox4_32, compiled on the host) before they were written here.

Recovery bounds, derived from the noise level sigma (per axis, on the planted targets; rms noise norm = sigma sqrt 3):
  * every planted pair is an inlier of the winner (the noise is 9 sigma sqrt 3 away from the 0.75 m threshold);
  * rmse of the winner <= 1.5 sigma sqrt 3: the least-squares pose has rmse ~ sigma sqrt 3, a 3-point pose on a well-spread triangle
    (sides ~ 30 m) adds a rotation error ~ sigma / 30 rad, which at the box's 42 m lever arm is ~ 0.07 m: sqrt(0.087^2 + 0.07^2) =
    0.11 m, and the winner is the smallest rmse of many such hypotheses;
  * then the rms displacement between the winner's and the planted pose over the planted points is at most rmse + sigma sqrt 3 =
    2.5 sigma sqrt 3 (triangle inequality in l2).  About the planted centroid c that displacement splits exactly into
    |dT c|^2 + (2 sin(theta / 2))^2 mean |perpendicular lever|^2, and the mean squared lever about any axis is at least the sum of
    the two smaller eigenvalues of the points' covariance: a bound on the translation at c and on ||R_w - R_0||_F =
    2 sqrt 2 sin(theta / 2)."""
import numpy as np
import pytest

import ransac_ref as rr


def test_philox4x32_10_known_answers():
    def px(ctr, key):
        return [int(v) for v in rr.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))]

    assert px([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert px([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert px([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # counter (0, 0, 0x13198a2e, 0x03707344), key (0xa4093822, 0x299f31d0): from the independent implementation
    assert px([0, 0, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xb60a410e, 0x61bd7780, 0xa53f3958, 0x3d51eb3f]


def test_sample_indices_follow_the_counter_layout():
    K, seed = 1000, 0x0123456789abcdef
    rows = rr.sample_indices(seed, [0, 5, (1 << 32) + 7], 6, K)
    key = [seed & 0xffffffff, seed >> 32]
    for row, itr in zip(rows, [0, 5, (1 << 32) + 7]):
        for j in range(6):
            w = rr.philox4x32_10(np.array([itr & 0xffffffff, itr >> 32, j // 4, 0], np.uint64), np.array(key, np.uint64))
            assert row[j] == (int(w[j % 4]) * K) >> 32
    assert rows.min() >= 0 and rows.max() < K
    # one stream per seed, a pure function of (seed, itr)
    assert (rr.sample_indices(seed, [5], 6, K)[0] == rows[1]).all()
    assert (rr.sample_indices(seed + 1, [5], 6, K)[0] != rows[1]).any()
    assert list(rr.repeated(np.array([[1, 2, 3], [4, 2, 4], [7, 7, 7]]))) == [False, True, True]


def _rot(ax, ang):
    ax = np.asarray(ax, float) / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def test_umeyama_on_hand_made_triples():
    S = np.array([[0.0, 0, 0], [4, 0, 0], [0, 3, 0]])
    R, t = _rot([1, 2, 3], 0.7), np.array([1.0, -2.0, 0.5])
    T = S @ R.T + t
    M, ratio = rr.umeyama_svd(S[None], T[None])
    assert np.allclose(M[0, :3, :3], R, atol=1e-14) and np.allclose(M[0, :3, 3], t, atol=1e-13) and ratio[0] > 0.1
    assert np.allclose(rr.umeyama_horn(S[None], T[None])[0], M[0], atol=1e-13)
    # four points and their mirror image: the best ORTHOGONAL map is a reflection, so the determinant fix-up must fire —
    # umeyama returns a proper rotation, not the reflection that would fit exactly
    S4 = np.array([[0.0, 0, 0], [4, 0, 0], [0, 3, 0], [0, 0, 2]])
    T4 = S4 * np.array([1.0, 1.0, -1.0])
    M4, _ = rr.umeyama_svd(S4[None], T4[None])
    R4 = M4[0, :3, :3]
    assert abs(np.linalg.det(R4) - 1.0) < 1e-14 and np.allclose(R4 @ R4.T, np.eye(3), atol=1e-14)
    assert not np.allclose(S4 @ R4.T + M4[0, :3, 3], T4, atol=0.1)
    U, _, Vt = np.linalg.svd(rr._sigma(S4[None], T4[None])[2][0])
    assert np.linalg.det(U @ Vt) < 0   # without the fix-up U V^T is a reflection
    assert np.allclose(rr.umeyama_horn(S4[None], T4[None])[0, :3, :3], R4, atol=1e-13)
    # a collinear sample is flagged by its singular-value ratio
    Sc = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2]])
    assert rr.umeyama_svd(Sc[None], Sc[None])[1][0] < rr.SIGMA_RATIO


def test_checkers_on_constructed_cases():
    S = np.array([[[0.0, 0, 0], [10, 0, 0], [0, 10, 0]]])
    same = S.copy()
    ok, fl = rr.edge_check(S, same, 0.6)
    assert ok[0] and not fl[0]
    short = S * np.array([0.5, 1.0, 1.0])    # the edge 0-1 shrinks to half: 5 < 10 * 0.6
    ok, fl = rr.edge_check(S, short, 0.6)
    assert not ok[0] and not fl[0]
    ok, _ = rr.edge_check(short, S, 0.6)     # symmetric: the other inequality
    assert not ok[0]
    edge = S.copy()
    edge[0, 1, 0] = 6.0                       # exactly at the bound on one edge: passes (>=), and is flagged
    ok, fl = rr.edge_check(S, edge, 0.6)
    assert ok[0] and fl[0]
    # distance checker: identity pose, one sample pair 0.7 / 0.8 / 0.9 m away
    M = np.eye(4)[None]
    for off, want_ok, want_fl in ((0.7, True, False), (0.8, True, True), (0.9, False, False), (0.8 + 5e-8, False, True)):
        rec = np.zeros((1, 3, 6))
        rec[0, :, :3] = S[0]
        rec[0, :, 3:] = S[0]
        rec[0, 2, 5] = off
        ok, fl = rr.distance_check(M, rec, 0.8)
        assert (bool(ok[0]), bool(fl[0])) == (want_ok, want_fl), off


def test_evaluation_sums_in_chunk_order():
    rng = np.random.default_rng(3)
    K = 3 * rr.CHUNK + 17
    rec = rng.random((K, 6))
    rec[:, 3:] = rec[:, :3] + 0.3 * rng.standard_normal((K, 3))
    M = np.eye(4)[None]
    n_in, err2, _, _ = rr.evaluate(M, rec, 0.5)
    d = rr.transformed_distance(M, rec)[0]
    inl = d < 0.5
    assert n_in[0] == inl.sum()
    tot = 0.0
    for c0 in range(0, K, rr.CHUNK):
        part = 0.0
        for k in range(c0, min(K, c0 + rr.CHUNK)):
            if inl[k]:
                part = part + d[k] * d[k]
        tot = tot + part
    assert err2[0] == tot           # bit for bit: the documented order


def test_serial_rule_on_hand_made_sequences():
    K, n = 100, 3
    sel = lambda p, ni, e, mi, conf: rr.serial_select(np.array(p, bool), np.array(ni), np.array(e, float), K, n, mi, conf)
    # a fitness tie is broken by the smaller rmse, never by the later iteration
    s = sel([1, 1, 1, 1], [10, 10, 10, 10], [4.0, 1.0, 1.0, 2.0], 4, 1.0)
    assert (s.best, s.n_in, s.evaluated, s.est_k) == (1, 10, 4, 4) and s.rmse == np.sqrt(1.0 / 10)
    # confidence 1.0 never stops early, whatever the ratio below 1
    s = sel([1] * 6, [99, 50, 60, 99, 99, 99], [1.0] * 6, 6, 1.0)
    assert s.est_k == 6 and s.evaluated == 6 and s.best == 0
    # ratio 1 stops at once: est_k = 0, nothing after the winner is evaluated
    s = sel([0, 1, 1, 1], [0, 100, 100, 100], [0, 5.0, 1.0, 1.0], 4, 0.999)
    assert (s.best, s.est_k, s.evaluated) == (1, 0, 1)
    # est_k = ceil(log(1 - c) / log(1 - r^n)) and the loop ends at the first itr >= est_k
    e = np.log(1 - 0.999) / np.log(1 - 0.5 ** 3)
    s = sel([1] + [0] * 60 + [1, 1], [50] + [0] * 60 + [80, 90], [1.0] * 63, 63, 0.999)
    assert s.est_k == int(np.ceil(e)) == 52 and s.best == 0 and s.evaluated == 1
    # ... while a better one BELOW est_k is taken and lowers it again, which ends the loop in front of the next
    s = sel([1] + [0] * 40 + [1, 1], [50] + [0] * 40 + [80, 90], [1.0] * 43, 43, 0.999)
    assert s.best == 41 and s.evaluated == 2 and s.est_k == int(np.ceil(np.log(1 - 0.999) / np.log(1 - 0.8 ** 3))) == 10
    assert s.trace == [(0, 43), (41, 10)]   # 52 does not lower an est_k of 43; itr 42 >= 10 is never looked at
    # the empty result: nothing passes, or what passes has no inlier (fitness 0 does not beat the empty best)
    s = sel([0, 0, 0], [5, 5, 5], [1.0] * 3, 3, 0.999)
    assert (s.best, s.fitness, s.rmse, s.evaluated, s.est_k) == (-1, 0.0, 0.0, 0, 3)
    s = sel([1, 1], [0, 0], [0.0, 0.0], 2, 0.999)
    assert s.best == -1 and s.evaluated == 2
    # the rule can be continued block by block
    a = rr.serial_select(np.array([1, 0, 1], bool), np.array([10, 0, 20]), np.array([1.0, 0, 1.0]), K, n, 1000, 0.999)
    b = rr.serial_select(np.array([1, 1], bool), np.array([20, 30]), np.array([0.5, 9.0]), K, n, 1000, 0.999, first_itr=3, state=a)
    whole = sel([1, 0, 1, 1, 1], [10, 0, 20, 20, 30], [1.0, 0, 1.0, 0.5, 9.0], 1000, 0.999)
    assert (b.best, b.est_k, b.evaluated, b.rmse) == (whole.best, whole.est_k, whole.evaluated, whole.rmse) and b.best == 4


def test_trivial_inputs_give_the_empty_result():
    src, tgt, corr, _, _ = rr.planted_case(50, 0.5, 1)
    for kw in (dict(ransac_n=2), dict(max_dist=0.0), dict(max_dist=-1.0)):
        r = rr.ransac(src, tgt, corr, max_iteration=100, **kw)
        assert r.best_iteration == -1 and r.fitness == 0 and r.inlier_rmse == 0 and np.array_equal(r.transformation, np.eye(4))
    assert rr.ransac(src, tgt, corr[:2], max_iteration=100).best_iteration == -1
    # every row repeated: skipped, nothing evaluated
    r = rr.ransac(src, tgt, corr, samples=np.array([[1, 1, 2], [3, 4, 3]]), max_iteration=100)
    assert r.best_iteration == -1 and r.evaluated == 0 and r.est_k == 2


SIGMA = 0.05
CASES = [(2000, 0.10, 11), (4000, 0.05, 12), (600, 0.30, 13)]


@pytest.mark.parametrize("K,share,seed", CASES)
def test_recovers_a_planted_pose(K, share, seed):
    src, tgt, corr, T0, planted = rr.planted_case(K, share, seed, SIGMA)
    r = rr.ransac(src, tgt, corr, seed=seed, max_iteration=10_000_000, confidence=0.999)
    noise = SIGMA * np.sqrt(3.0)
    print(f"K {K} share {share}: est_k {r.est_k} winner {r.best_iteration} inliers {len(r.inliers)} planted {int(planted.sum())} "
          f"rmse {r.inlier_rmse:.4f} evaluated {r.evaluated} flagged {r.flagged_evaluated}/{r.flagged_below_est_k} margin {r.min_margin:.2e}")
    assert 0 <= r.best_iteration < r.est_k < 10_000_000          # the confidence rule ended the loop
    assert r.flagged_evaluated == 0 and r.flagged_below_est_k <= 0.01 * r.est_k
    assert set(np.flatnonzero(planted)) <= set(r.inliers)         # every planted pair found
    assert r.fitness == len(r.inliers) / K
    assert r.inlier_rmse <= 1.5 * noise
    P = src[planted] @ T0[:3, :3].T + T0[:3, 3]
    c = P.mean(axis=0)
    lam = np.sort(np.linalg.eigvalsh(np.cov((P - c).T, bias=True)))
    disp = 2.5 * noise
    dT = r.transformation @ np.linalg.inv(T0)
    assert np.linalg.norm(dT[:3, :3] @ c + dT[:3, 3] - c) <= disp
    theta = disp / np.sqrt(lam[0] + lam[1])
    assert np.linalg.norm(r.transformation[:3, :3] - T0[:3, :3]) <= 2 * np.sqrt(2.0) * np.sin(theta / 2)
    # the same stream through an explicit table gives the same result
    tab = rr.sample_indices(seed, np.arange(r.est_k), 3, K)
    r2 = rr.ransac(src, tgt, corr, samples=tab, max_iteration=10_000_000, confidence=0.999)
    assert (r2.best_iteration, r2.est_k, r2.evaluated, r2.inlier_rmse) == (r.best_iteration, r.est_k, r.evaluated, r.inlier_rmse)
