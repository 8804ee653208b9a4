"""The contract of include/outlier_removal/o3s_outlier_removal.h in numpy: Open3D v0.15.1's PointCloud::RemoveRadiusOutliers and
PointCloud::RemoveStatisticalOutliers, restated from its published PointCloud.cpp (Open3D itself is not available here).

Every floating-point operation is written out as the contract orders it: numpy's elementwise operations round once each (no fused
multiply-add), np.sqrt is correctly rounded, and the sums that the contract calls sequential are Python loops or np.add.accumulate,
which adds left to right.  Two routes to the neighbour sets:
  brute force   O(N^2), in row blocks — the bit-level reference;
  cKDTree       candidates only (a ball a hair wider than the radius, or a few neighbours more than asked for); distances, order
                and ties are then decided by the contract's own expression, and a list that the candidates cannot settle is redone
                with more of them.  For the few larger sizes.
"""
import math

import numpy as np

U = 2.0 ** -52


def d2(q, p):
    """squared distances of the points p (M, 3) from q (3,) or (B, 1, 3): ((dx dx + dy dy) + dz dz), each operation rounded once"""
    dx = q[..., 0] - p[..., 0]
    dy = q[..., 1] - p[..., 1]
    dz = q[..., 2] - p[..., 2]
    d = dx * dx
    d = d + dy * dy
    d = d + dz * dz
    return d


def finite_mask(p):
    return np.isfinite(p).all(axis=1)


def radius_counts(pts, radius, use_tree=False):
    """#{ j finite : d2(i, j) < radius * radius } for every finite i (0 for a non-finite point)"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    fin = finite_mask(p)
    idx = np.flatnonzero(fin)
    f = p[idx]
    r2 = radius * radius
    cnt = np.zeros(p.shape[0], np.int64)
    if len(f) == 0:
        return cnt
    if use_tree:
        from scipy.spatial import cKDTree

        tree = cKDTree(f)
        cand = tree.query_ball_point(f, radius * (1.0 + 1e-9) + 1e-300)
        for k, c in enumerate(cand):
            c = np.asarray(c, np.int64)
            cnt[idx[k]] = int((d2(f[k], f[c]) < r2).sum())
        return cnt
    B = 256
    for a in range(0, len(f), B):
        d = d2(f[a:a + B, None, :], f[None, :, :])
        cnt[idx[a:a + B]] = (d < r2).sum(axis=1)
    return cnt


def radius_outlier(pts, nb_points, radius, use_tree=False):
    """-> keep mask (N,) bool: kept iff the count, the point itself included, exceeds nb_points"""
    return radius_counts(pts, radius, use_tree) > nb_points


def knn_d2(pts, k, use_tree=False):
    """the k nearest finite points of every finite point, itself included, ascending (d2, index) -> (rows of f, (F, k) d2)"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    idx = np.flatnonzero(finite_mask(p))
    f = p[idx]
    F = len(f)
    k = min(k, F)
    out = np.zeros((F, k))
    if F == 0:
        return idx, out
    if use_tree:
        from scipy.spatial import cKDTree

        tree = cKDTree(f)
        extra = 8
        todo = np.arange(F)
        while len(todo):
            kk = min(F, k + extra)
            _, nn = tree.query(f[todo], k=kk)
            nn = np.asarray(nn).reshape(len(todo), kk)
            again = []
            for row, i in enumerate(todo):
                c = nn[row]
                d = d2(f[i], f[c])
                o = np.lexsort((c, d))
                d = d[o]
                # settled when every candidate beyond the k-th is strictly farther than the tree's own margin can hide
                if kk < F and not d[k - 1] * (1.0 + 1e-9) < d[kk - 1]:
                    again.append(i)
                    continue
                out[i] = d[:k]
            todo = np.asarray(again, np.int64)
            extra *= 4
        return idx, out
    B = 256
    for a in range(0, F, B):
        d = d2(f[a:a + B, None, :], f[None, :, :])
        for row in range(d.shape[0]):
            o = np.lexsort((np.arange(F), d[row]))[:k]
            out[a + row] = d[row][o]
    return idx, out


def statistical_outlier(pts, nb_neighbors, std_ratio, use_tree=False):
    """-> dict(keep, avg, mean, std, thr, valid, gap, sum_abs, sum_sq): the contract's statistical filter.  gap: the smallest
    relative distance |avg_i - thr| / thr of a point with avg_i > 0 from the threshold (inf when there is none or thr is NaN);
    sum_abs / sum_sq: the sums of the magnitudes of the terms of the two cloud-wide sums (what an error bound of another
    summation order is stated in)."""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    N = p.shape[0]
    idx, dk = knn_d2(p, nb_neighbors, use_tree)
    avg = np.full(N, -1.0)
    if len(idx):
        k = dk.shape[1]
        s = np.zeros(len(idx))
        for c in range(k):  # sequential from 0.0, ascending distance
            s = s + np.sqrt(dk[:, c])
        avg[idx] = s / float(k)
    valid = int((avg >= 0.0).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        tot = 0.0
        for a in avg:
            if a > 0.0:
                tot = tot + float(a)
        mean = np.float64(tot) / np.float64(valid)
        sq = 0.0
        for a in avg:
            if a > 0.0:
                dd = np.float64(a) - mean
                sq = sq + float(dd * dd)
        std = np.sqrt(np.float64(sq) / (np.float64(valid) - np.float64(1.0)))
        thr = mean + np.float64(std_ratio) * std
        keep = (avg > 0.0) & (avg < thr)
        pos = avg[avg > 0.0]
        gap = float(np.min(np.abs(pos - thr) / thr)) if len(pos) and np.isfinite(thr) and thr > 0 else math.inf
    return dict(keep=keep, avg=avg, mean=float(mean), std=float(std), thr=float(thr), valid=valid, gap=gap, sum_abs=float(tot), sum_sq=float(sq))


def stats_bounds(ref, N, std_ratio):
    """How far mean, std and thr of an implementation that adds the SAME terms in another order may lie from the sequential reference.
    A sum of n terms in any order is within (n - 1) 2^-53 sum|t| of the exact sum (to first order), two orders therefore within
    n 2^-52 sum|t| of each other: that is the bound on the two sums, and — the issue's figure — an upper bound on what reaches mean,
    std and thr.  What actually reaches them is smaller and asserted too (`tight`): mean = S1 / valid; std = sqrt(S2 / (valid - 1)),
    so d std = d S2 / (2 std (valid - 1)), where S2's terms also move with the mean: |d S2| <= 2 |d mean| sum|a - mean| + valid
    d mean^2; each result adds a few roundings of its own (4 ulp allowed)."""
    v = ref["valid"]
    loose = dict(mean=N * U * ref["sum_abs"], std=N * U * ref["sum_sq"], thr=N * U * (ref["sum_abs"] + std_ratio * ref["sum_sq"]))
    if v < 2 or not np.isfinite(ref["std"]) or ref["std"] == 0.0:
        return loose, None
    dm = N * U * ref["sum_abs"] / v + 4 * U * abs(ref["mean"])
    ds2 = N * U * ref["sum_sq"] + 2 * dm * math.sqrt(ref["sum_sq"] * v) + v * dm * dm   # sum|a - m| <= sqrt(v S2)
    dstd = ds2 / (2 * ref["std"] * (v - 1)) + 4 * U * ref["std"]
    tight = dict(mean=dm, std=dstd, thr=dm + std_ratio * dstd + 4 * U * abs(ref["thr"]))
    return loose, tight
