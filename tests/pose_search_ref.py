"""numpy restatement of the initial pose search (include/pose_search/o3s_pose_search.h): pose matrices in the header's operation
order, scores by membership of packed voxel keys, the local-maximum rule and the top-K ordering.  Imports nothing of the library.

A grid is a plain dict: center (4 x 4), step_xy, step_z, step_yaw, yaw0, n_x, n_y, n_z, n_yaw, yaw_ring, point_stride,
local_maxima, top_k, min_score."""
import math

import numpy as np

BIAS = 1 << 20   # a voxel index packs when it lies in [-2^20, 2^20)


def grid(center=None, step_xy=0.5, step_z=0.5, step_yaw=math.radians(5.0), yaw0=0.0, n_x=8, n_y=8, n_z=0, n_yaw=72, yaw_ring=True,
         point_stride=1, local_maxima=True, top_k=8, min_score=1):
    return dict(center=np.eye(4) if center is None else np.asarray(center, np.float64).reshape(4, 4), step_xy=float(step_xy),
                step_z=float(step_z), step_yaw=float(step_yaw), yaw0=float(yaw0), n_x=int(n_x), n_y=int(n_y), n_z=int(n_z), n_yaw=int(n_yaw),
                yaw_ring=bool(yaw_ring), point_stride=int(point_stride), local_maxima=bool(local_maxima), top_k=int(top_k),
                min_score=int(min_score))


def cells(g):
    return 2 * g["n_x"] + 1, 2 * g["n_y"] + 1, 2 * g["n_z"] + 1, g["n_yaw"]


def count(g):
    cx, cy, cz, cl = cells(g)
    return cx * cy * cz * cl


def split(g, p):
    """p -> (i, j, k, l): x runs fastest"""
    cx, cy, cz, _ = cells(g)
    return p % cx, p // cx % cy, p // (cx * cy) % cz, p // (cx * cy * cz)


def rotation(g, l):
    """R = Rz(psi_l) R_c, element by element: row 0 = (c Rc0) - (s Rc1), row 1 = (s Rc0) + (c Rc1), row 2 = Rc2"""
    psi = g["yaw0"] + float(l) * g["step_yaw"]
    c, s = math.cos(psi), math.sin(psi)
    Rc = g["center"][:3, :3]
    R = np.zeros((3, 3))
    R[0] = (c * Rc[0]) - (s * Rc[1])
    R[1] = (s * Rc[0]) + (c * Rc[1])
    R[2] = Rc[2]
    return R


def translation(g, i, j, k):
    tc = g["center"][:3, 3]
    return np.array([tc[0] + float(i - g["n_x"]) * g["step_xy"], tc[1] + float(j - g["n_y"]) * g["step_xy"],
                     tc[2] + float(k - g["n_z"]) * g["step_z"]])


def pose(g, p):
    i, j, k, l = split(g, p)
    T = np.eye(4)
    T[:3, :3] = rotation(g, l)
    T[:3, 3] = translation(g, i, j, k)
    return T


def pack(pts, voxel):
    """(keys, ok): the packed voxel key of every point — floor(q * (1 / voxel)) in fp64 — and whether it packs (a NaN does not)"""
    inv = 1.0 / voxel
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(np.asarray(pts, np.float64).reshape(-1, 3) * inv)
        ok = np.all((f >= -float(BIAS)) & (f < float(BIAS)), axis=1)
    fi = np.where(ok[:, None], f, 0.0).astype(np.int64) + BIAS
    return (fi[:, 2] << 42) | (fi[:, 1] << 21) | fi[:, 0], ok


def voxel_keys(map_pts, voxel):
    """the snapshot: the sorted distinct keys of the map points that pack"""
    k, ok = pack(map_pts, voxel)
    return np.unique(k[ok])


def scores(map_keys, voxel, scan, g, poses=None):
    """score of every pose (or of the listed ones): the strided scan points whose key at q = ((R0 x + R1 y) + R2 z) + t is in the map"""
    pts = np.asarray(scan, np.float64).reshape(-1, 3)[:: g["point_stride"]]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    which = np.arange(count(g), dtype=np.int64) if poses is None else np.asarray(poses, np.int64).reshape(-1)
    out = np.zeros(len(which), np.int64)
    yaw_of = np.array([split(g, int(p))[3] for p in which], np.int64)
    for l in np.unique(yaw_of):                     # the poses of one yaw together: the same operations, on arrays
        R = rotation(g, int(l))
        at = np.flatnonzero(yaw_of == l)
        t = np.array([translation(g, *split(g, int(p))[:3]) for p in which[at]])          # (n, 3)
        with np.errstate(invalid="ignore", over="ignore"):
            s = [(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z for r in range(3)]
            q = np.stack([s[r][None, :] + t[:, r][:, None] for r in range(3)], axis=2)    # (n, M, 3)
        key, ok = pack(q.reshape(-1, 3), voxel)
        hit = ok & np.isin(key, map_keys)
        out[at] = hit.reshape(len(at), -1).sum(axis=1)
    return out


def local_maxima(sc, g):
    """mask of the poses no neighbour beats: q beats p when score[q] > score[p], or the scores are equal and q < p"""
    cx, cy, cz, cl = cells(g)
    s = np.asarray(sc, np.int64).reshape(cl, cz, cy, cx)
    idx = np.arange(s.size, dtype=np.int64).reshape(s.shape)
    ring = g["yaw_ring"] and cl >= 3
    keep = np.ones(s.shape, bool)
    for dl in (-1, 0, 1):
        for dk in (-1, 0, 1):
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    if (dl, dk, dj, di) == (0, 0, 0, 0):
                        continue
                    for l in range(cl):
                        ql = l + dl
                        if ql < 0 or ql >= cl:
                            if not ring:
                                continue
                            ql %= cl
                        k0, k1 = max(0, -dk), min(cz, cz - dk)
                        j0, j1 = max(0, -dj), min(cy, cy - dj)
                        i0, i1 = max(0, -di), min(cx, cx - di)
                        if k0 >= k1 or j0 >= j1 or i0 >= i1:
                            continue
                        a = s[l, k0:k1, j0:j1, i0:i1]
                        b = s[ql, k0 + dk:k1 + dk, j0 + dj:j1 + dj, i0 + di:i1 + di]
                        ia = idx[l, k0:k1, j0:j1, i0:i1]
                        ib = idx[ql, k0 + dk:k1 + dk, j0 + dj:j1 + dj, i0 + di:i1 + di]
                        keep[l, k0:k1, j0:j1, i0:i1] &= ~((b > a) | ((b == a) & (ib < ia)))
    return keep.reshape(-1)


def select(sc, g):
    """(indices, scores) of the first top_k eligible poses by (score descending, index ascending)"""
    sc = np.asarray(sc, np.int64).reshape(-1)
    el = sc >= g["min_score"]
    if g["local_maxima"]:
        el &= local_maxima(sc, g)
    cand = np.flatnonzero(el)
    order = cand[np.lexsort((cand, -sc[cand]))][: g["top_k"]]
    return order.astype(np.int64), sc[order]
