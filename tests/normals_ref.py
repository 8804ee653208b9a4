"""Exact neighbour lists of Open3D's EstimateNormals(Hybrid(radius, max_nn)) at sweep and map sizes (test infrastructure).

The oracle's orc_estimate_normals is brute force (O(N^2): about 8 s per parameter set at 131 k points).  This module gives the
same lists from a kd-tree: candidates from scipy's cKDTree (eps 0), their squared distances recomputed in the association the
device and the oracle use, ((dx dx + dy dy) + dz dz), ordered by (d2, original index), the first max_nn kept and cut at
d2 < radius^2.  A query's list is accepted only with a certificate that no point outside its candidates can enter it: either the
tree found fewer candidates than asked within a bound above the radius (then every point that can pass the cut is a candidate),
or the max_nn-th re-ranked d2 lies below the farthest candidate's by a relative 1e-9 (the tree's own distances differ from the
recomputed ones by rounding only).  Queries without one (ties, duplicate clusters) are redone with a ball query that holds every
point up to the max_nn-th candidate distance.  Normals then come from oracle.normals_from_neighbours on these lists.
"""
import os

import numpy as np
from scipy.spatial import cKDTree

from oracle import oracle as orc

_REL = 1e-9      # certificate margin (relative, on d2)
_CHUNK = 65536   # queries per block (bounds the N x k temporaries)


def threads() -> int:
    """Worker threads: OMP_NUM_THREADS (the CPUs a job may use), never the machine's core count."""
    try:
        return max(1, int(os.environ.get("OMP_NUM_THREADS", "4")))
    except ValueError:
        return 4


def _d2(q, p):
    """((dx dx + dy dy) + dz dz), q: (n, 3), p: (n, k, 3)."""
    dx = q[:, None, 0] - p[..., 0]
    dy = q[:, None, 1] - p[..., 1]
    dz = q[:, None, 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _rank(d2, idx, max_nn, r2):
    """Rows ordered by (d2, idx), the first max_nn kept, cut at d2 < r2, -1 padded; also the max_nn-th d2 of each row."""
    order = np.lexsort((idx, d2), axis=-1)
    d2 = np.take_along_axis(d2, order, axis=-1)
    idx = np.take_along_axis(idx, order, axis=-1)
    k = min(max_nn, d2.shape[1])
    out = np.full((d2.shape[0], max_nn), -1, np.int32)
    keep = d2[:, :k] < r2
    out[:, :k] = np.where(keep, idx[:, :k], -1)
    kth = d2[:, max_nn - 1] if d2.shape[1] >= max_nn else np.full(d2.shape[0], np.inf)
    return out, kth


class Stats:
    def __init__(self):
        self.queries = 0
        self.fallback = 0


def neighbour_lists(pts, radius, max_nn, extra=None, stats=None, tree=None):
    """N x max_nn int32 neighbour lists (-1 padded), exactly what the brute-force oracle gives."""
    p = np.ascontiguousarray(pts, np.float64)
    N = p.shape[0]
    assert 1 <= max_nn and radius > 0 and N >= 1
    r2 = float(radius) * float(radius)
    tree = tree if tree is not None else cKDTree(p, balanced_tree=False, compact_nodes=False)
    kq = min(N, max_nn + (extra if extra is not None else max(8, max_nn)))
    dub = float(radius) * (1.0 + 1e-6) + 1e-300
    out = np.empty((N, max_nn), np.int32)
    redo = []
    for b in range(0, N, _CHUNK):
        q = p[b:b + _CHUNK]
        _, idx = tree.query(q, k=kq, eps=0, distance_upper_bound=dub, workers=threads())
        idx = np.asarray(idx).reshape(q.shape[0], kq)
        found = idx < N
        safe = np.where(found, idx, 0)
        d2 = np.where(found, _d2(q, p[safe]), np.inf)
        idx = np.where(found, safe, np.iinfo(np.int32).max).astype(np.int64)
        lists, kth = _rank(d2, idx, max_nn, r2)
        out[b:b + q.shape[0]] = lists
        if kq == N:
            continue                                  # every point is a candidate
        short = ~found.all(axis=1)                    # all points within dub > radius are candidates
        far = np.where(found, d2, -np.inf).max(axis=1)
        ok = short | (kth < far * (1.0 - _REL))
        redo.extend((b + np.nonzero(~ok)[0]).tolist())
    for i in redo:
        # every point with d2 <= the max_nn-th candidate's (which bounds the true max_nn-th from above), ties included
        _, idx = tree.query(p[i:i + 1], k=kq, eps=0, workers=1)
        idx = np.asarray(idx).reshape(-1)
        kth = np.sort(_d2(p[i:i + 1], p[idx][None])[0])[max_nn - 1]
        ball = np.asarray(tree.query_ball_point(p[i], np.sqrt(kth) * (1.0 + 1e-6) + 1e-300, eps=0), np.int64)
        d2 = _d2(p[i:i + 1], p[ball][None])
        lists, _ = _rank(d2, ball[None], max_nn, r2)
        out[i] = lists[0]
    if stats is not None:
        stats.queries += N
        stats.fallback += len(redo)
    return out


def estimate_normals(pts, radius, max_nn, stats=None):
    """(normals, lists): the oracle's normals on the exact lists of neighbour_lists."""
    nn = neighbour_lists(pts, radius, max_nn, stats=stats)
    return orc.normals_from_neighbours(pts, nn), nn
