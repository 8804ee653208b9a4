"""The contract of include/clustering/o3s_clustering.h in numpy: Open3D v0.15.1's PointCloud::ClusterDBSCAN(eps, min_points),
restated from its published PointCloudCluster.cpp (Open3D itself is not available here), twice:

  dbscan(...)             the closed form the header states: core points by count, clusters = connected components of the core
                          graph numbered by their smallest core index, border points to the smallest id among their core
                          neighbours, everything else -1;
  dbscan_sequential(...)  Open3D's loop, statement by statement: ascending idx, a set of neighbours to visit that is popped in
                          arbitrary order (std::unordered_set there; a seeded random order here), noise (-2 -> -1) relabelled
                          when a cluster reaches it.

tests/test_dbscan_ref.py shows that the two agree.  The neighbour predicate is the contract's own expression (outlier_ref.d2:
every operation rounded once, no fused multiply-add, strict comparison with eps * eps).  Two routes to the neighbour sets, as in
outlier_ref: brute force below TREE_FROM points, cKDTree candidates (a ball a hair wider than eps) with the predicate re-applied
from there on.
"""
import numpy as np

from outlier_ref import d2, finite_mask

TREE_FROM = 4099


def neighbours(pts, eps, use_tree=None):
    """-> list over all N points of int64 arrays: the neighbours (input indices, ascending, the point itself included) of every
    finite point; an empty array for a non-finite one"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    N = p.shape[0]
    idx = np.flatnonzero(finite_mask(p))
    f = p[idx]
    r2 = eps * eps
    out = [np.zeros(0, np.int64) for _ in range(N)]
    if len(f) == 0:
        return out
    if use_tree is None:
        use_tree = N >= TREE_FROM
    if use_tree:
        from scipy.spatial import cKDTree

        tree = cKDTree(f)
        cand = tree.query_ball_point(f, eps * (1.0 + 1e-9) + 1e-300)
        for k, c in enumerate(cand):
            c = np.sort(np.asarray(c, np.int64))
            out[idx[k]] = idx[c[d2(f[k], f[c]) < r2]]
        return out
    B = 256
    for a in range(0, len(f), B):
        d = d2(f[a:a + B, None, :], f[None, :, :])
        for row in range(d.shape[0]):
            out[idx[a + row]] = idx[np.flatnonzero(d[row] < r2)]
    return out


def _components_union_find(N, ei, ej):
    """root[x] = the smallest member of x's component under the edges (ei, ej): a plain union-find, the smaller root on top"""
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(ei.tolist(), ej.tolist()):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(N)], np.int64)


def _components_scipy(N, ei, ej):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components

    g = csr_matrix((np.ones(len(ei), np.int8), (ei, ej)), shape=(N, N))
    _, comp = connected_components(g, directed=False)
    smallest = np.full(comp.max() + 1 if N else 0, N, np.int64)
    np.minimum.at(smallest, comp, np.arange(N))
    return smallest[comp]


def dbscan(pts, eps, min_points, use_tree=None, nbrs=None):
    """the closed form -> (labels (N,) int32, n_clusters, sizes (n_clusters,) int64)"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    N = p.shape[0]
    if use_tree is None:
        use_tree = N >= TREE_FROM
    nb = neighbours(p, eps, use_tree) if nbrs is None else nbrs
    cnt = np.array([len(x) for x in nb], np.int64)
    core = (cnt >= min_points) & (cnt > 0)
    # all ordered neighbour pairs (i, j)
    ei = np.repeat(np.arange(N), cnt)
    ej = np.concatenate(nb) if N else np.zeros(0, np.int64)
    cc = core[ei] & core[ej]                                   # the edges of the core graph
    root = (_components_scipy if use_tree else _components_union_find)(N, ei[cc], ej[cc])
    roots = np.unique(root[core])                              # ascending: the smallest core index of every cluster
    cid = np.full(N, -1, np.int64)
    cid[core] = np.searchsorted(roots, root[core])
    labels = cid.copy()
    bc = ~core[ei] & core[ej]                                  # border i, core neighbour j: the smallest id wins
    best = np.full(N, np.iinfo(np.int64).max)
    np.minimum.at(best, ei[bc], cid[ej[bc]])
    got = best != np.iinfo(np.int64).max
    labels[got] = best[got]
    n = len(roots)
    sizes = np.bincount(labels[labels >= 0], minlength=n).astype(np.int64)
    return labels.astype(np.int32), n, sizes


def dbscan_sequential(pts, eps, min_points, rng=None, use_tree=None, nbrs=None):
    """Open3D's loop (PointCloudCluster.cpp, v0.15.1):

        labels(N, -2); cluster_label = 0
        for idx in 0 .. N-1:
            if labels[idx] != -2: continue                       // already noise or in a cluster
            if nbs[idx].size() < min_points: labels[idx] = -1; continue
            nbs_next(nbs[idx]); nbs_visited = {idx}; labels[idx] = cluster_label
            while !nbs_next.empty():
                nb = *nbs_next.begin(); nbs_next.erase(begin); nbs_visited.insert(nb)
                if labels[nb] == -1: labels[nb] = cluster_label  // noise becomes border
                if labels[nb] != -2: continue                    // labelled before: not expanded, not relabelled
                labels[nb] = cluster_label
                if nbs[nb].size() >= min_points:
                    for qnb in nbs[nb]: if qnb not in nbs_visited: nbs_next.insert(qnb)
            cluster_label++

    A radius search from a non-finite point finds nothing; a non-finite point is found by none (the predicate is false on NaN and
    on an infinite distance), so it ends as noise for min_points >= 1.  rng: the order the set is popped in (None: ascending).
    -> (labels (N,) int32, n_clusters)"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    N = p.shape[0]
    nb = neighbours(p, eps, use_tree) if nbrs is None else nbrs
    labels = np.full(N, -2, np.int64)
    cluster = 0
    for idx in range(N):
        if labels[idx] != -2:
            continue
        if len(nb[idx]) < min_points:
            labels[idx] = -1
            continue
        nxt = set(int(j) for j in nb[idx])
        visited = {idx}
        labels[idx] = cluster
        while nxt:
            if rng is None:
                q = min(nxt)
            else:
                lst = sorted(nxt)
                q = lst[int(rng.integers(len(lst)))]
            nxt.discard(q)
            visited.add(q)
            if labels[q] == -1:
                labels[q] = cluster
            if labels[q] != -2:
                continue
            labels[q] = cluster
            if len(nb[q]) >= min_points:
                for j in nb[q]:
                    if int(j) not in visited:
                        nxt.add(int(j))
        cluster += 1
    return labels.astype(np.int32), cluster


def keep_mask(labels, sizes, min_cluster_size):
    """removal: kept iff label >= 0 and size[label] >= min_cluster_size"""
    labels = np.asarray(labels)
    ok = labels >= 0
    out = np.zeros(len(labels), bool)
    out[ok] = np.asarray(sizes)[labels[ok]] >= min_cluster_size
    return out
