"""numpy restatement of the two registration health quantities (include/o3s_icp.h "registration fitness", include/o3s_submap.h
"occupancy snapshot"): what the GPU tests compare against, itself checked on hand-computed cases in test_health_ref.py.

1. Registration fitness = Open3D's RegistrationResult (fitness_, inlier_rmse_) over the matcher's output: a reading point counts when
   it has a match (id >= 0) whose fp32 squared distance is <= r2, r2 = fl32(r * r), r = 0 meaning the chain's max_dist.
2. Overlap fitness = the body of SubmapCollection::isSwitchingSubmapsConsistant: the share of scan points, moved by
   mapToRangeSensor (an Eigen::Isometry3d product: R p + t), whose voxel getVoxelIdx(p, 1 / voxel) holds a map point.
"""
import math

import numpy as np

PACK_BIAS = 1 << 20   # voxel indices the device packs into one key: [-2^20, 2^20) per axis


def radius2(r, max_dist):
    """fl32(r * r); r == 0 stands for the chain's max_dist."""
    r = np.float32(max_dist if r == 0 else r)
    return np.float32(r * r)


def registration_fitness(ids, d2, r=0.0, max_dist=0.5):
    """(n_correspondences, fitness, inlier_rmse) of N matches (ids: -1 = none, d2: fp32 squared distances, +inf = none)."""
    ids = np.asarray(ids)
    d2 = np.asarray(d2, np.float32)
    n = len(ids)
    inl = (ids >= 0) & (d2 <= radius2(r, max_dist))
    k = int(inl.sum())
    s = math.fsum(float(v) for v in d2[inl])   # the exact sum of the promoted fp32 values, rounded once
    return k, (k / n if n else float("nan")), (math.sqrt(s / k) if k else 0.0)


def voxel_keys(pts, voxel):
    """getVoxelIdx(p, InverseVoxelSize) (VoxelHashMap.hpp:43-51): floor(p * (1 / voxel)) in fp64, per axis; (N, 3) float64 of
    integral values (NaN where the coordinate is not a number)."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    inv = 1.0 / float(voxel)
    with np.errstate(invalid="ignore"):
        return np.floor(p * inv)


def packable(keys):
    """rows whose three indices fit the device's packed key (NaN and +-inf do not)."""
    k = np.asarray(keys, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return np.all((k >= -PACK_BIAS) & (k < PACK_BIAS), axis=1)


def voxel_map(pts, voxel):
    """The occupancy snapshot: the set of voxel keys of the map points."""
    k = voxel_keys(pts, voxel)
    return {tuple(int(v) for v in row) for row in k[packable(k)]}


def isometry_apply(T, pts):
    """mapToRangeSensor * p of an Eigen::Isometry3d: ((R0 x + R1 y) + R2 z) + t per row, fp64 (numpy does not contract)."""
    T = np.asarray(T, np.float64)
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.empty_like(p)
    for a in range(3):
        s = T[a, 0] * p[:, 0]
        s = s + T[a, 1] * p[:, 1]
        s = s + T[a, 2] * p[:, 2]
        out[:, a] = s + T[a, 3]
    return out


def overlap_fitness(vmap, pts, T, voxel):
    """(n_overlapping, fitness); vmap None = no snapshot.  0 / 0 = NaN for an empty scan, as the reference's expression."""
    p = np.asarray(pts, np.float64).reshape(-1, 3)
    n = len(p)
    if n == 0:
        return 0, float("nan")
    if not vmap:
        return 0, 0.0
    k = voxel_keys(isometry_apply(T, p), voxel)
    ok = packable(k)
    hits = sum(1 for row, good in zip(k, ok) if good and tuple(int(v) for v in row) in vmap)
    return hits, hits / n
