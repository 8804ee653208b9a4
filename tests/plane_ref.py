"""numpy restatement of the contract of include/plane_segmentation/o3s_plane_segmentation.h: Open3D v0.15.1's
PointCloud::SegmentPlane (geometry/PointCloudSegmentation.cpp, TriangleMesh::ComputeTrianglePlane, GetPlaneFromPoints) made
deterministic the way the registration RANSAC was (the Philox4x32-10 sample stream and the serial selection rule of
tests/ransac_ref.py, imported, not copied).  fp64 throughout; numpy does not contract a * b + c, np.cumsum adds sequentially, and
every sum whose order the contract fixes is formed in that order: chunks of 512, each summed from 0.0 in ascending index, then the
chunk sums from 0.0 in ascending chunk order.  Every comparison against this module is exact."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ransac_ref import _MASK, est_k_update, philox4x32_10

CHUNK = 512
PASS, REPEATED, NONFINITE, DEGENERATE = 0, 1, 2, 3


def sample_indices(seed: int, itrs, ransac_n: int, M: int, plane: int = 0) -> np.ndarray:
    """Rows of ransac_n point indices of the iterations `itrs`: counter (itr low, itr high, j / 4, plane), key (seed low, seed high)."""
    itrs = np.asarray(itrs, np.uint64)
    out = np.zeros((itrs.shape[0], ransac_n), np.int64)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    for q in range((ransac_n + 3) // 4):
        ctr = np.stack([itrs & _MASK, itrs >> np.uint64(32), np.full_like(itrs, q), np.full_like(itrs, plane)], axis=-1)
        w = philox4x32_10(ctr, key).astype(np.uint64)
        for u in range(4):
            j = 4 * q + u
            if j < ransac_n:
                out[:, j] = ((w[:, u] * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
    return out


def chunk_sum(v) -> np.float64:
    """The contract's sum of a 1-D array (0.0 for an empty one).  Padding with +0.0 changes no partial sum: all of them start at +0.0."""
    v = np.asarray(v, np.float64)
    if v.size == 0:
        return np.float64(0.0)
    part = np.cumsum(np.pad(v, (0, (-v.size) % CHUNK)).reshape(-1, CHUNK), axis=1)[:, -1]
    return np.cumsum(part)[-1]


def sample_planes(pts, rows):
    """Outcome and plane (a, b, c, d; zeros unless PASS) of every sample row."""
    rows = np.asarray(rows, np.int64)
    H, M = rows.shape[0], pts.shape[0]
    outcome = np.zeros(H, np.int32)
    s = np.sort(rows, axis=1)
    outcome[(s[:, 1:] == s[:, :-1]).any(axis=1) | (rows < 0).any(axis=1) | (rows >= M).any(axis=1)] = REPEATED
    P = pts[np.clip(rows[:, :3], 0, M - 1)]                      # H x 3 x 3: the first three define the plane
    outcome[(outcome == PASS) & ~np.isfinite(P).all(axis=(1, 2))] = NONFINITE
    planes = np.zeros((H, 4))
    with np.errstate(all="ignore"):
        p0, e0, e1 = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        nx = e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1]
        ny = e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2]
        nz = e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]
        norm = np.sqrt((nx * nx + ny * ny) + nz * nz)
        live = outcome == PASS
        outcome[live & (norm == 0.0)] = DEGENERATE
        outcome[live & (norm != 0.0) & ~np.isfinite(norm)] = NONFINITE   # finite points whose cross product overflows
        a, b, c = nx / norm, ny / norm, nz / norm
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
    ok = outcome == PASS
    planes[ok] = np.stack([a, b, c, d], axis=1)[ok]
    return outcome, planes


def distances(planes, pts):
    """H x M: |((a x + b y) + c z) + d|."""
    pl = np.asarray(planes)[:, None, :]
    with np.errstate(all="ignore"):
        return np.abs(((pl[..., 0] * pts[None, :, 0] + pl[..., 1] * pts[None, :, 1]) + pl[..., 2] * pts[None, :, 2]) + pl[..., 3])


def evaluate(planes, pts, threshold, block: int = 64):
    """(n_in, err in the contract's order) of every plane over all points."""
    H, M = len(planes), pts.shape[0]
    n_in, err = np.zeros(H, np.int64), np.zeros(H)
    pad = (-M) % CHUNK
    for h0 in range(0, H, block):
        d = distances(planes[h0:h0 + block], pts)
        inl = d < threshold                                         # false for a non-finite point
        n_in[h0:h0 + block] = inl.sum(axis=1)
        e = np.pad(np.where(inl, d, 0.0), ((0, 0), (0, pad))).reshape(d.shape[0], -1, CHUNK)
        part = np.cumsum(e, axis=2)[:, :, -1]
        err[h0:h0 + block] = np.cumsum(part, axis=1)[:, -1]
    return n_in, err


def evaluate_samples(pts, rows, threshold, given_planes=None):
    """(outcome, planes, n_in, err) of the sample rows; n_in and err are zero where the outcome is not PASS.  given_planes: evaluate
    THESE planes for the rows that pass (the device's own, should a plane ever differ in its last bit)."""
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    outcome, planes = sample_planes(pts, rows)
    ok = outcome == PASS
    if given_planes is not None:
        planes = np.where(ok[:, None], np.asarray(given_planes), 0.0)
    n_in, err = np.zeros(len(outcome), np.int64), np.zeros(len(outcome))
    if ok.any():
        n_in[ok], err[ok] = evaluate(planes[ok], pts, threshold)
    return outcome, planes, n_in, err


@dataclass
class Selection:
    best: int = -1
    est_k: int = 0
    evaluated: int = 0
    fitness: float = 0.0
    rmse: float = 0.0
    n_in: int = 0
    trace: list = field(default_factory=list)   # (itr, est_k after) of every replacement


def serial_select(outcome, n_in, err, M: int, ransac_n: int, num_iterations: int, confidence: float, first_itr: int = 0,
                  state: Selection = None) -> Selection:
    """The selection rule over a sequence whose element i is iteration first_itr + i: a serial loop."""
    st = Selection(est_k=int(num_iterations)) if state is None else state
    for i in range(len(outcome)):
        itr = first_itr + i
        if itr >= st.est_k:
            break
        if outcome[i] != PASS:
            continue
        st.evaluated += 1
        n = int(n_in[i])
        fit = np.float64(n) / np.float64(M)
        rmse = np.float64(err[i]) / np.sqrt(np.float64(n)) if n else np.float64(0.0)
        if fit > st.fitness or (fit == st.fitness and rmse < st.rmse):
            st.best, st.fitness, st.rmse, st.n_in = itr, float(fit), float(rmse), n
            e = est_k_update(n, M, ransac_n, confidence)
            if e < st.est_k:
                st.est_k = int(np.ceil(e))
            st.trace.append((itr, st.est_k))
    return st


def refit(q) -> np.ndarray:
    """GetPlaneFromPoints of the inlier list q (L x 3, L >= 1) in the contract's order of operations."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    L = np.float64(q.shape[0])
    with np.errstate(all="ignore"):
        c = np.array([chunk_sum(q[:, k]) for k in range(3)]) / L
        r = q - c
        xx, xy, xz = chunk_sum(r[:, 0] * r[:, 0]), chunk_sum(r[:, 0] * r[:, 1]), chunk_sum(r[:, 0] * r[:, 2])
        yy, yz, zz = chunk_sum(r[:, 1] * r[:, 1]), chunk_sum(r[:, 1] * r[:, 2]), chunk_sum(r[:, 2] * r[:, 2])
        det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
        if det_x > det_y and det_x > det_z:
            n = np.array([det_x, xz * yz - xy * zz, xy * yz - xz * yy])
        elif det_y > det_z:
            n = np.array([xz * yz - xy * zz, det_y, xy * xz - yz * xx])
        else:
            n = np.array([xy * yz - xz * yy, xy * xz - yz * xx, det_z])
        norm = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        if norm == 0.0:
            return np.zeros(4)
        n = n / norm
        return np.array([n[0], n[1], n[2], -((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2])])


@dataclass
class PlaneResult:
    model: np.ndarray          # the refit (zeros: nothing passed)
    inliers: np.ndarray        # ascending indices, of the winning sample's plane
    best_iteration: int
    est_k: int
    evaluated: int
    plane: np.ndarray          # the winning sample's plane
    trace: list


def segment_plane(points, distance_threshold, ransac_n=3, num_iterations=100, confidence=1.0, seed=0, samples=None, plane=0,
                  block: int = 256) -> PlaneResult:
    """One segmentation: block by block of iterations until the serial loop ends."""
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    M = pts.shape[0]
    n_iter = int(num_iterations) if samples is None else min(int(num_iterations), len(samples))
    empty = PlaneResult(np.zeros(4), np.zeros(0, np.int64), -1, n_iter, 0, np.zeros(4), [])
    if M < ransac_n:
        return empty
    st = Selection(est_k=n_iter)
    best_plane = np.zeros(4)
    itr0 = 0
    while itr0 < min(st.est_k, n_iter):
        cnt = min(block, n_iter - itr0)
        rows = sample_indices(seed, np.arange(itr0, itr0 + cnt), ransac_n, M, plane) if samples is None else np.asarray(samples)[itr0:itr0 + cnt]
        outcome, planes, n_in, err = evaluate_samples(pts, rows, distance_threshold)
        prev = st.best
        st = serial_select(outcome, n_in, err, M, ransac_n, n_iter, confidence, itr0, st)
        if st.best != prev:
            best_plane = planes[st.best - itr0]
        itr0 += cnt
    if st.best < 0:
        empty.est_k, empty.evaluated = st.est_k, st.evaluated
        return empty
    inl = np.flatnonzero(distances(best_plane[None], pts)[0] < distance_threshold)
    return PlaneResult(refit(pts[inl]), inl, st.best, st.est_k, st.evaluated, best_plane, st.trace)


def segment_planes(points, distance_threshold, max_planes, min_inliers=3, ransac_n=3, num_iterations=100, confidence=1.0, seed=0):
    """The peel -> (labels, models (n_planes x 4), counts)."""
    pts = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    labels = np.full(pts.shape[0], -1, np.int32)
    left = np.arange(pts.shape[0])
    models, counts = [], []
    for k in range(int(max_planes)):
        r = segment_plane(pts[left], distance_threshold, ransac_n, num_iterations, confidence, seed, None, plane=k)
        if r.best_iteration < 0 or len(r.inliers) < min_inliers:
            break
        labels[left[r.inliers]] = k
        models.append(r.model)
        counts.append(len(r.inliers))
        left = np.delete(left, r.inliers)
    return labels, np.array(models).reshape(-1, 4), np.array(counts, np.int64)
