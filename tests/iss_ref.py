"""The contract of include/keypoints/o3s_keypoints.h in numpy: Open3D v0.15.1's geometry::keypoint::ComputeISSKeypoints, restated
from its published Keypoint.cpp (Open3D itself is not available here).

Neighbour candidates come from scipy's cKDTree at r (1 + 1e-9) (or, brute force, from the whole cloud); distances are then
recomputed in the contract's association ((dx dx + dy dy) + dz dz, each operation rounded once) and cut strictly, as
tests/outlier_ref.py does.  Eigenvalues: np.linalg.eigvalsh.

What an implementation may differ in is the order in which S_i is summed and its 3 x 3 eigen solver.  Per point the reference
therefore also returns the bound
    B_i = (3 n_i + 64) 2^-52 trace(S_i).
First term: every entry of S_i is a sum of n_i terms whose magnitudes add up to at most trace(S_i) (|dx dy| <= (dx^2 + dy^2) / 2),
so two orders of addition differ by at most n_i 2^-52 trace(S_i) per entry — the bound the outlier header states for its sums —
and a symmetric 3 x 3 perturbation of that size per entry moves an eigenvalue by at most three times it (its spectral norm is at
most three times its largest entry; Weyl).  Second term: the allowance for two backward-stable 3 x 3 eigen solvers, a few ulps of
||S|| <= trace(S) each.

The fragile set: the points for which a comparison they enter changes when every eigenvalue involved moves by +- its B — l3 > 0,
the two ratio tests, the non-max comparison against each neighbour (coincident points excepted: the contract gives them the same
bits), and the two count thresholds when a candidate lies within a relative 1e-12 of r^2.  A point with a fragile neighbour in its
non-max set is fragile too."""
import math

import numpy as np

from outlier_ref import d2, finite_mask

U = 2.0 ** -52
EDGE = 1e-12


SHEETS = {2000: (0.6, 0.4), 20000: (0.4, 0.25)}   # the GPU test's clouds: cloud(N) of tests/test_gpu_outlier_removal.py -> radii
GAMMAS = (0.975, 0.8)
_CACHE = {}


def sheet(N):
    from test_gpu_outlier_removal import cloud

    return cloud(N)


def sheet_ref(N, gamma):
    """the reference on sheet(N) at its radii of SHEETS, computed once per process"""
    if (N, gamma) not in _CACHE:
        rs, rn = SHEETS[N]
        _CACHE[(N, gamma)] = iss(sheet(N), rs, rn, gamma, gamma, 5)
    return _CACHE[(N, gamma)]


def _candidates(f, r, use_tree):
    F = len(f)
    if not use_tree:
        everyone = np.arange(F, dtype=np.int64)
        return [everyone] * F
    from scipy.spatial import cKDTree

    tree = cKDTree(f)
    return [np.sort(np.asarray(c, np.int64)) for c in tree.query_ball_point(f, r * (1.0 + 1e-9) + 1e-300)]


def resolution(pts, use_tree=True):
    """(sum over the finite points of sqrt(d2 to the nearest other finite point)) / (number of finite points); 0 below two points"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    f = p[finite_mask(p)]
    F = len(f)
    if F < 2:
        return 0.0
    near = np.empty(F)
    if use_tree:
        from scipy.spatial import cKDTree

        k = min(F, 9)
        _, nn = cKDTree(f).query(f, k=k)
        nn = np.asarray(nn).reshape(F, k)
        for i in range(F):
            c = nn[i][nn[i] != i]
            near[i] = d2(f[i], f[c]).min()
    else:
        for i in range(F):
            d = d2(f[i], f)
            d[i] = math.inf
            near[i] = d.min()
    return math.fsum(np.sqrt(near)) / float(F)


def iss(pts, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, use_tree=True):
    """-> dict of per-point arrays over the N input points: n (salient count), n_nm (non-max count), trace, eig (N, 3) descending,
    sal, flag (bool), B, fragile (bool); and radii (2,), margin_ratio / margin_tie (the closest relative ratio-test margin and
    non-max tie, for the record)."""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    N = p.shape[0]
    out = dict(n=np.zeros(N, np.int64), n_nm=np.zeros(N, np.int64), trace=np.zeros(N), eig=np.zeros((N, 3)), sal=np.zeros(N),
               flag=np.zeros(N, bool), B=np.zeros(N), fragile=np.zeros(N, bool), margin_ratio=math.inf, margin_tie=math.inf)
    if salient_radius == 0.0 or non_max_radius == 0.0:
        res = resolution(p, use_tree)
        salient_radius, non_max_radius = 6.0 * res, 4.0 * res
    out["radii"] = np.array([salient_radius, non_max_radius])
    idx = np.flatnonzero(finite_mask(p))
    f = p[idx]
    F = len(f)
    if F == 0 or not max(salient_radius, non_max_radius) > 0.0:
        return out
    n = np.zeros(F, np.int64)
    tr = np.zeros(F)
    eig = np.zeros((F, 3))
    sal = np.zeros(F)
    B = np.zeros(F)
    own = np.zeros(F, bool)   # fragile through the point's own tests
    rs2 = salient_radius * salient_radius
    cand = _candidates(f, salient_radius, use_tree)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(F):
            c = cand[i]
            d = d2(f[i], f[c])
            hit = d < rs2
            n[i] = int(hit.sum())
            edge = int((np.abs(d - rs2) <= EDGE * rs2).sum())
            if edge and (n[i] - edge < min_neighbors <= n[i] + edge):
                own[i] = True
            D = f[c[hit]] - f[i]
            S = D.T @ D
            tr[i] = S[0, 0] + S[1, 1] + S[2, 2]
            B[i] = (3 * n[i] + 64) * U * tr[i]
            if n[i] < min_neighbors or not S.any():
                continue
            l3, l2, l1 = np.linalg.eigvalsh(S)
            eig[i] = (l1, l2, l3)
            if l2 / l1 < gamma_21 and l3 / l2 < gamma_32:
                sal[i] = l3
            b = B[i]
            m21, m32 = abs(l2 - gamma_21 * l1), abs(l3 - gamma_32 * l2)
            out["margin_ratio"] = min(out["margin_ratio"], m21 / l1, m32 / l1)
            if abs(l3) <= b or m21 <= b * (1.0 + gamma_21) or m32 <= b * (1.0 + gamma_32):
                own[i] = True
    rn2 = non_max_radius * non_max_radius
    if non_max_radius > salient_radius:   # else the salient candidates hold the non-max ones
        cand = _candidates(f, non_max_radius, use_tree)
    n_nm = np.zeros(F, np.int64)
    flag = np.zeros(F, bool)
    fragile = own.copy()
    for i in range(F):
        c = cand[i]
        d = d2(f[i], f[c])
        hit = d < rn2
        n_nm[i] = int(hit.sum())
        nb = c[hit]
        edge = int((np.abs(d - rn2) <= EDGE * rn2).sum())
        if sal[i] > 0.0 and edge and (n_nm[i] - edge < min_neighbors <= n_nm[i] + edge):
            fragile[i] = True
        if own[nb].any():
            fragile[i] = True
        if not sal[i] > 0.0:
            continue
        flag[i] = n_nm[i] >= min_neighbors and not (sal[nb] > sal[i]).any()
        other = nb[(d[hit] > 0.0) & (sal[nb] > 0.0)]   # coincident points share their bits; a neighbour at 0 stays at 0 unless fragile itself
        if len(other):
            gap = np.abs(sal[other] - sal[i])
            out["margin_tie"] = min(out["margin_tie"], float((gap / sal[i]).min()))
            if (gap <= B[other] + B[i]).any():
                fragile[i] = True
    out["n"][idx] = n
    out["n_nm"][idx] = n_nm
    out["trace"][idx] = tr
    out["eig"][idx] = eig
    out["sal"][idx] = sal
    out["flag"][idx] = flag
    out["B"][idx] = B
    out["fragile"][idx] = fragile
    return out


def iss_brute(pts, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors):
    """The contract once more, O(N^2) and without any shared helper beyond d2: (sal, flag) — the check of iss() itself."""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    N = p.shape[0]
    fin = finite_mask(p)
    sal = np.zeros(N)
    within_nm = [None] * N
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(N):
            if not fin[i]:
                continue
            d = np.where(fin, d2(p[i], np.where(fin[:, None], p, 0.0)), math.inf)
            within_nm[i] = np.flatnonzero(d < non_max_radius * non_max_radius)
            nb = np.flatnonzero(d < salient_radius * salient_radius)
            if len(nb) < min_neighbors:
                continue
            S = np.zeros((3, 3))
            for j in nb:
                v = p[j] - p[i]
                S += np.outer(v, v)
            if not S.any():
                continue
            l3, l2, l1 = np.linalg.eigvalsh(S)
            if l2 / l1 < gamma_21 and l3 / l2 < gamma_32:
                sal[i] = l3
    flag = np.zeros(N, bool)
    for i in range(N):
        if fin[i] and sal[i] > 0.0 and len(within_nm[i]) >= min_neighbors:
            flag[i] = not (sal[within_nm[i]] > sal[i]).any()
    return sal, flag
