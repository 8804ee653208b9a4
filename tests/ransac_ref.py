"""numpy restatement of the RANSAC contract of include/o3s_registration.h ("RANSAC"): Open3D v0.15.1's
RegistrationRANSACBasedOnCorrespondence with TransformationEstimationPointToPoint(false), the edge-length and the distance
checker, made deterministic (Philox4x32-10 sample stream, serial selection).  fp64 throughout; every sum whose order the
contract fixes is formed in that order (np.cumsum adds sequentially).

The module also computes the FLAGGED SET: the hypotheses whose outcome another correct implementation could decide differently —
an edge comparison within relative 1e-12 of equality, a checker or inlier distance within 1e-7 m of its threshold, a sample
whose covariance has sigma_2 / sigma_1 < 1e-6.  Comparisons against this restatement skip these and nothing else."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

CHUNK = 512            # correspondences per chunk of the err2 sum (the contract's summation order)
PASS, REPEATED, EDGE, DISTANCE = 0, 1, 2, 3
EDGE_REL, DIST_ABS, SIGMA_RATIO = 1e-12, 1e-7, 1e-6

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: (..., 4) uint32-valued, key: (..., 2) -> (..., 4) uint32 (Random123's philox4x32-10)."""
    c = [np.asarray(counter)[..., k].astype(np.uint64) for k in range(4)]
    k0, k1 = (np.asarray(key)[..., k].astype(np.uint64) for k in range(2))
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0 = (k0 + np.uint64(_W0)) & _MASK
        k1 = (k1 + np.uint64(_W1)) & _MASK
    return np.stack(c, axis=-1).astype(np.uint32)


def sample_indices(seed: int, itrs, ransac_n: int, K: int) -> np.ndarray:
    """Rows of ransac_n correspondence indices of the iterations `itrs` (step 1 of the contract)."""
    itrs = np.asarray(itrs, np.uint64)
    out = np.zeros((itrs.shape[0], ransac_n), np.int64)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    for q in range((ransac_n + 3) // 4):
        ctr = np.stack([itrs & _MASK, itrs >> np.uint64(32), np.full_like(itrs, q), np.zeros_like(itrs)], axis=-1)
        w = philox4x32_10(ctr, key).astype(np.uint64)
        for u in range(4):
            j = 4 * q + u
            if j < ransac_n:
                out[:, j] = ((w[:, u] * np.uint64(K)) >> np.uint64(32)).astype(np.int64)
    return out


def records(source, target, corr) -> np.ndarray:
    """K x 6: (s, t) coordinates of every correspondence."""
    corr = np.asarray(corr)
    return np.concatenate([np.asarray(source, np.float64)[corr[:, 0]], np.asarray(target, np.float64)[corr[:, 1]]], axis=1)


def repeated(samples) -> np.ndarray:
    s = np.sort(np.asarray(samples), axis=1)
    return (s[:, 1:] == s[:, :-1]).any(axis=1)


def _norm3(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def edge_check(S, T, similarity):
    """S, T: H x n x 3 sample coordinates -> (passes, flagged)."""
    n = S.shape[1]
    ok = np.ones(S.shape[0], bool)
    flagged = np.zeros(S.shape[0], bool)
    for a in range(n):
        for b in range(a + 1, n):
            ds, dt = _norm3(S[:, a] - S[:, b]), _norm3(T[:, a] - T[:, b])
            ok &= ~((ds < dt * similarity) | (dt < ds * similarity))
            flagged |= np.abs(ds - dt * similarity) <= EDGE_REL * np.maximum(ds, dt * similarity)
            flagged |= np.abs(dt - ds * similarity) <= EDGE_REL * np.maximum(dt, ds * similarity)
    return ok, flagged


def _sigma(S, T):
    n = S.shape[1]
    ms, mt = S.sum(axis=1) / n, T.sum(axis=1) / n
    sig = np.einsum("hja,hjb->hab", T - mt[:, None], S - ms[:, None]) / n
    return ms, mt, sig


def _pose(R, ms, mt):
    M = np.zeros((R.shape[0], 4, 4))
    M[:, :3, :3] = R
    M[:, :3, 3] = mt - np.einsum("hab,hb->ha", R, ms)
    M[:, 3, 3] = 1.0
    return M


def umeyama_svd(S, T):
    """Eigen::umeyama(S, T, false) per sample (LAPACK's SVD) -> (H x 4 x 4, sigma_2 / sigma_1)."""
    ms, mt, sig = _sigma(S, T)
    U, sv, Vt = np.linalg.svd(sig)
    d = np.ones((S.shape[0], 3))
    d[:, 2] = np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0)
    R = np.einsum("hak,hk,hkb->hab", U, d, Vt)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(sv[:, 0] > 0, sv[:, 1] / sv[:, 0], 0.0)
    return _pose(R, ms, mt), ratio


def umeyama_horn(S, T):
    """The same rigid motion by Horn's closed form (unit quaternion = top eigenvector of a 4 x 4 matrix): an independent fp64 route."""
    ms, mt, sig = _sigma(S, T)
    M = np.swapaxes(sig, 1, 2)  # M[a][b] = sum s_a t_b
    N = np.zeros((S.shape[0], 4, 4))
    Sxx, Sxy, Sxz = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2]
    Syx, Syy, Syz = M[:, 1, 0], M[:, 1, 1], M[:, 1, 2]
    Szx, Szy, Szz = M[:, 2, 0], M[:, 2, 1], M[:, 2, 2]
    N[:, 0, 0] = Sxx + Syy + Szz
    N[:, 0, 1] = N[:, 1, 0] = Syz - Szy
    N[:, 0, 2] = N[:, 2, 0] = Szx - Sxz
    N[:, 0, 3] = N[:, 3, 0] = Sxy - Syx
    N[:, 1, 1] = Sxx - Syy - Szz
    N[:, 1, 2] = N[:, 2, 1] = Sxy + Syx
    N[:, 1, 3] = N[:, 3, 1] = Szx + Sxz
    N[:, 2, 2] = -Sxx + Syy - Szz
    N[:, 2, 3] = N[:, 3, 2] = Syz + Szy
    N[:, 3, 3] = -Sxx - Syy + Szz
    _, vec = np.linalg.eigh(N)
    q = vec[:, :, 3]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.zeros((S.shape[0], 3, 3))
    R[:, 0, 0] = w * w + x * x - y * y - z * z
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = w * w - x * x + y * y - z * z
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = w * w - x * x - y * y + z * z
    return _pose(R, ms, mt)


def transformed_distance(M, rec):
    """M: H x 4 x 4, rec: H x n x 6 or K x 6 (broadcast over H) -> d = |M s - t| in the contract's order of operations."""
    if rec.ndim == 2:
        rec = rec[None]
    Mx = M[:, None]
    p = [((Mx[..., r, 0] * rec[..., 0] + Mx[..., r, 1] * rec[..., 1]) + Mx[..., r, 2] * rec[..., 2]) + Mx[..., r, 3] for r in range(3)]
    dx, dy, dz = p[0] - rec[..., 3], p[1] - rec[..., 4], p[2] - rec[..., 5]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def distance_check(M, rec_samples, threshold):
    d = transformed_distance(M, rec_samples)
    return (d <= threshold).all(axis=1), (np.abs(d - threshold) <= DIST_ABS).any(axis=1)


def evaluate(M, rec, max_dist, block: int = 256):
    """Step 5 for every pose of M over the K records: (n_in, err2 in the contract's order, flagged, smallest inlier margin)."""
    H, K = M.shape[0], rec.shape[0]
    n_in, err2 = np.zeros(H, np.int64), np.zeros(H)
    flagged, margin = np.zeros(H, bool), np.full(H, np.inf)
    pad = (-K) % CHUNK
    for h0 in range(0, H, block):
        d = transformed_distance(M[h0:h0 + block], rec)
        inl = d < max_dist
        n_in[h0:h0 + block] = inl.sum(axis=1)
        m = np.abs(d - max_dist)
        margin[h0:h0 + block] = m.min(axis=1)
        flagged[h0:h0 + block] = (m <= DIST_ABS).any(axis=1)
        e = np.where(inl, d * d, 0.0)
        e = np.pad(e, ((0, 0), (0, pad))).reshape(e.shape[0], -1, CHUNK)
        part = np.cumsum(e, axis=2)[:, :, -1]          # within a chunk: sequentially, ascending index
        err2[h0:h0 + block] = np.cumsum(part, axis=1)[:, -1]  # the chunks: sequentially, ascending
    return n_in, err2, flagged, margin


@dataclass
class Hypotheses:
    outcome: np.ndarray      # PASS / REPEATED / EDGE / DISTANCE
    T: np.ndarray            # H x 4 x 4 (identity where nothing was estimated)
    n_in: np.ndarray
    err2: np.ndarray
    flagged: np.ndarray      # the flagged set
    margin: np.ndarray       # smallest |d - max_dist| of an evaluated hypothesis (inf otherwise)


def evaluate_samples(rec, samples, ransac_n=3, max_dist=0.75, distance_threshold=0.8, similarity=0.6, check_distance=True,
                     check_edge=True, given_T=None) -> Hypotheses:
    """Steps 1 - 5 for the sample rows.  given_T (H x 4 x 4): evaluate THESE poses for the rows that pass steps 1 - 2 (the tests
    pass the device's own T, so that n_in and err2 can be compared bit for bit)."""
    samples = np.asarray(samples, np.int64)
    H, K = samples.shape[0], rec.shape[0]
    outcome = np.zeros(H, np.int32)
    flagged = np.zeros(H, bool)
    bad = repeated(samples) | (samples < 0).any(axis=1) | (samples >= K).any(axis=1)
    outcome[bad] = REPEATED
    R = rec[np.clip(samples, 0, K - 1)]
    S, T = R[..., :3], R[..., 3:]
    if check_edge:
        ok, fl = edge_check(S, T, similarity)
        flagged |= fl & ~bad
        outcome[(outcome == PASS) & ~ok] = EDGE
    M = np.tile(np.eye(4), (H, 1, 1))
    live = outcome == PASS
    if live.any():
        Ms, ratio = umeyama_svd(S[live], T[live])
        if given_T is not None:
            Ms = np.asarray(given_T)[live]
        M[live] = Ms
        fl = ratio < SIGMA_RATIO
        if check_distance:
            ok, fd = distance_check(Ms, R[live], distance_threshold)
            fl |= fd
            o = outcome[live]
            o[~ok] = DISTANCE
            outcome[live] = o
        flagged[live] |= fl
    n_in, err2, margin = np.zeros(H, np.int64), np.zeros(H), np.full(H, np.inf)
    live = outcome == PASS
    if live.any():
        n, e, fe, mg = evaluate(M[live], rec, max_dist)
        n_in[live], err2[live], margin[live] = n, e, mg
        flagged[live] |= fe
    return Hypotheses(outcome, M, n_in, err2, flagged, margin)


@dataclass
class Selection:
    best: int = -1            # index into the sequence (the winning itr when the sequence starts at itr 0)
    est_k: int = 0
    evaluated: int = 0
    fitness: float = 0.0
    rmse: float = 0.0
    n_in: int = 0
    trace: list = field(default_factory=list)   # (itr, est_k after) of every replacement


def est_k_update(n_in: int, K: int, ransac_n: int, confidence: float):
    r = np.float64(n_in) / np.float64(K)
    p = r
    for _ in range(1, ransac_n):
        p = p * r
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(np.float64(1.0) - np.float64(confidence)) / np.log(np.float64(1.0) - p)


def serial_select(passed, n_in, err2, K: int, ransac_n: int, max_iteration: int, confidence: float, first_itr: int = 0,
                  state: Selection = None) -> Selection:
    """Rule 6 over a (pass, n_in, err2) sequence whose element i is iteration first_itr + i.  `state` continues an earlier part."""
    st = Selection(est_k=int(max_iteration)) if state is None else state
    for i in np.flatnonzero(np.asarray(passed)):
        itr = first_itr + int(i)
        if itr >= st.est_k:
            break
        st.evaluated += 1
        n = int(n_in[i])
        fit = np.float64(n) / np.float64(K)
        rmse = np.sqrt(np.float64(err2[i]) / np.float64(n)) if n else np.float64(0.0)
        if fit > st.fitness or (fit == st.fitness and rmse < st.rmse):
            st.best, st.fitness, st.rmse, st.n_in = itr, float(fit), float(rmse), n
            e = est_k_update(n, K, ransac_n, confidence)
            if e < st.est_k:
                st.est_k = int(np.ceil(e))
            st.trace.append((itr, st.est_k))
    return st


@dataclass
class RansacResult:
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    inliers: np.ndarray          # indices into the correspondence list, ascending
    best_iteration: int
    est_k: int
    evaluated: int
    flagged_evaluated: int       # flagged hypotheses among those the serial rule evaluated (must be 0 in an end-to-end case)
    flagged_below_est_k: int     # flagged iterations below the final est_k, and how many iterations that is
    min_margin: float


def ransac(source, target, corr, ransac_n=3, max_dist=0.75, distance_threshold=0.8, similarity=0.6, check_distance=True, check_edge=True,
           max_iteration=10_000_000, confidence=0.999, seed=0, samples=None, block: int = 65536) -> RansacResult:
    """The whole contract, block by block of iterations until the serial loop ends."""
    corr = np.asarray(corr).reshape(-1, 2)
    K = corr.shape[0]
    n_iter = int(max_iteration) if samples is None else min(int(max_iteration), len(samples))
    empty = RansacResult(np.eye(4), 0.0, 0.0, np.zeros(0, np.int64), -1, n_iter, 0, 0, 0, np.inf)
    if ransac_n < 3 or K < ransac_n or not max_dist > 0:
        return empty
    rec = records(source, target, corr)
    st = Selection(est_k=n_iter)
    best_T, fl_eval, fl_below, margin = np.eye(4), 0, [], np.inf
    itr0 = 0
    while itr0 < st.est_k:
        cnt = min(block, n_iter - itr0)
        if cnt <= 0:
            break
        rows = sample_indices(seed, np.arange(itr0, itr0 + cnt), ransac_n, K) if samples is None else np.asarray(samples)[itr0:itr0 + cnt]
        hyp = evaluate_samples(rec, rows, ransac_n, max_dist, distance_threshold, similarity, check_distance, check_edge)
        before = st.evaluated
        prev_best = st.best
        st = serial_select(hyp.outcome == PASS, hyp.n_in, hyp.err2, K, ransac_n, n_iter, confidence, itr0, st)
        if st.best != prev_best:
            best_T = hyp.T[st.best - itr0]
        # the survivors the rule reached in this block: the first (evaluated - before) of them
        reached = np.flatnonzero(hyp.outcome == PASS)[:st.evaluated - before]
        fl_eval += int(hyp.flagged[reached].sum())
        if reached.size:
            margin = min(margin, float(hyp.margin[reached].min()))
        fl_below.append((itr0, hyp.flagged))
        itr0 += cnt
    below = sum(int(f[:max(0, min(len(f), st.est_k - i0))].sum()) for i0, f in fl_below)
    if st.best < 0:
        empty.est_k, empty.evaluated, empty.flagged_evaluated, empty.flagged_below_est_k = st.est_k, st.evaluated, fl_eval, below
        return empty
    d = transformed_distance(best_T[None], rec)[0]
    return RansacResult(best_T, st.fitness, st.rmse, np.flatnonzero(d < max_dist), st.best, st.est_k, st.evaluated, fl_eval, below, margin)


def planted_case(K: int, inlier_share: float, seed: int, sigma: float = 0.05, box=(60.0, 60.0, 6.0)):
    """Uniform points in a box, a planted rigid motion on a share of the pairs (sigma noise on their targets), the rest paired with
    unrelated uniform points.  Returns (source K x 3, target K x 3, corr K x 2, T planted, planted mask)."""
    rng = np.random.default_rng(seed)
    box = np.asarray(box)
    src = (rng.random((K, 3)) - 0.5) * box
    ang = np.array([0.05, -0.04, 0.6])
    cx, cy, cz = np.cos(ang)
    sx, sy, sz = np.sin(ang)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = [3.0, -2.0, 0.5]
    planted = rng.random(K) < inlier_share
    tgt = (rng.random((K, 3)) - 0.5) * box
    tgt[planted] = src[planted] @ T[:3, :3].T + T[:3, 3] + sigma * rng.standard_normal((int(planted.sum()), 3))
    corr = np.stack([np.arange(K), np.arange(K)], axis=1).astype(np.int32)
    return src, tgt, corr, T, planted
