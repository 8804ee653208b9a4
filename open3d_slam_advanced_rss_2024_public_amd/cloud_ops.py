"""Host-side mirror of the open3d_slam point-cloud helpers around the ICP path, over the C ABI
(include/o3s_cloud_ops.h).  Function names follow the reference (open3d_slam/src/helpers.cpp, croppers.cpp,
include/open3d_slam/VoxelHashMap.hpp, open3d_conversions.cpp); all arithmetic runs on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


class CropperC(C.Structure):
    _fields_ = [("kind", C.c_int32), ("invert", C.c_int32), ("p0", C.c_double), ("p1", C.c_double), ("p2", C.c_double),
                ("centre", C.c_double * 3)]


_KINDS = {"CroppingVolume": 0, "MaxRadius": 1, "MinRadius": 2, "MinMaxRadius": 3, "Cylinder": 4}


def _L():
    L = _lib.lib()
    if _lib.needs_binding(L, __name__):  # once per loaded library (product or test-hook build)
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int32)
        fp = C.POINTER(C.c_float)
        L.o3s_voxel_idx.argtypes = [C.c_int, dp, C.c_int64, C.c_double, ip]
        L.o3s_voxel_hash.argtypes = [C.c_int, ip, C.c_int64, C.POINTER(C.c_uint64)]
        L.o3s_crop.argtypes = [C.c_int, C.POINTER(CropperC), dp, dp, C.c_int64, dp, dp, C.POINTER(C.c_int64)]
        L.o3s_voxelize_within_crop.argtypes = [C.c_int, C.POINTER(CropperC), C.c_double, dp, dp, C.c_int64, dp, dp, ip,
                                               C.POINTER(C.c_int64)]
        L.o3s_voxel_downsample.argtypes = [C.c_int, C.c_double, dp, dp, C.c_int64, dp, dp, ip, C.POINTER(C.c_int64)]
        L.o3s_o3d_to_pm.argtypes = [C.c_int, dp, dp, C.c_int64, fp, fp]
        L.o3s_estimate_normals.argtypes = [C.c_int, dp, C.c_int64, C.c_double, C.c_int32, dp, ip]
        L.o3s_compute_fpfh.argtypes = [C.c_int, dp, dp, C.c_int64, C.c_double, C.c_int32, dp, dp, ip]
    return L


def _check(rc, what):
    if rc != _lib.OK:
        raise RuntimeError(f"{what} failed with o3s_status {rc}")


def _d(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _i(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def croppingVolumeFactory(kind: str = "MaxRadius", p0=0.0, p1=0.0, p2=0.0, centre=(0.0, 0.0, 0.0), invert=False) -> CropperC:
    """croppingVolumeFactory (croppers.cpp:14-51) + setPose / setIsInvertVolume."""
    return CropperC(_KINDS[kind], int(invert), float(p0), float(p1), float(p2), (C.c_double * 3)(*[float(v) for v in centre]))


def getVoxelIdx(points, voxel_size: float, device: int = 0) -> np.ndarray:
    p = np.ascontiguousarray(points, np.float64)
    out = np.zeros((p.shape[0], 3), np.int32)
    _check(_L().o3s_voxel_idx(device, _d(p), p.shape[0], float(voxel_size), _i(out)), "o3s_voxel_idx")
    return out


def voxelHash(idx, device: int = 0) -> np.ndarray:
    i = np.ascontiguousarray(idx, np.int32)
    out = np.zeros(i.shape[0], np.uint64)
    _check(_L().o3s_voxel_hash(device, _i(i), i.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint64))), "o3s_voxel_hash")
    return out


def crop(cropper: CropperC, points, normals=None, device: int = 0):
    """CroppingVolume::crop (croppers.cpp:76-106)."""
    p = np.ascontiguousarray(points, np.float64)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64)
    op = np.zeros_like(p)
    on = np.zeros_like(p) if n is not None else None
    k = C.c_int64()
    _check(_L().o3s_crop(device, C.byref(cropper), _d(p), _d(n), p.shape[0], _d(op), _d(on), C.byref(k)), "o3s_crop")
    return op[:k.value].copy(), (on[:k.value].copy() if n is not None else None)


def voxelizeWithinCroppingVolume(voxel_size: float, cropper: CropperC, points, normals=None, device: int = 0):
    """voxelizeWithinCroppingVolume (helpers.cpp:117-192) -> (points, normals, voxel_idx)."""
    p = np.ascontiguousarray(points, np.float64)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64)
    op = np.zeros_like(p)
    on = np.zeros_like(p) if n is not None else None
    oi = np.zeros((p.shape[0], 3), np.int32)
    k = C.c_int64()
    _check(_L().o3s_voxelize_within_crop(device, C.byref(cropper), float(voxel_size), _d(p), _d(n), p.shape[0], _d(op), _d(on),
                                         _i(oi), C.byref(k)), "o3s_voxelize_within_crop")
    return op[:k.value].copy(), (on[:k.value].copy() if n is not None else None), oi[:k.value].copy()


def voxelize(voxel_size: float, points, normals=None, device: int = 0):
    """o3d_slam::voxelize (helpers.cpp:108-115) = Open3D v0.15.1 VoxelDownSample -> (points, normals, voxel_idx)."""
    p = np.ascontiguousarray(points, np.float64)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64)
    op = np.zeros_like(p)
    on = np.zeros_like(p) if n is not None else None
    oi = np.zeros((p.shape[0], 3), np.int32)
    k = C.c_int64()
    _check(_L().o3s_voxel_downsample(device, float(voxel_size), _d(p), _d(n), p.shape[0], _d(op), _d(on), _i(oi), C.byref(k)),
           "o3s_voxel_downsample")
    return op[:k.value].copy(), (on[:k.value].copy() if n is not None else None), oi[:k.value].copy()


def open3dToPointmatcher(points, normals=None, device: int = 0):
    """open3dToPointmatcher (open3d_conversions.cpp:57-118) -> (xyzw (N,4) fp32, normals (N,3) fp32 | None)."""
    p = np.ascontiguousarray(points, np.float64)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64)
    xyzw = np.zeros((p.shape[0], 4), np.float32)
    on = np.zeros((p.shape[0], 3), np.float32) if n is not None else None
    fp = C.POINTER(C.c_float)
    _check(_L().o3s_o3d_to_pm(device, _d(p), _d(n), p.shape[0], xyzw.ctypes.data_as(fp), None if on is None else on.ctypes.data_as(fp)),
           "o3s_o3d_to_pm")
    return xyzw, on


def estimateNormals(points, max_radius: float, knn: int, want_neighbours: bool = False, device: int = 0):
    """EstimateNormals(KDTreeSearchParamHybrid(max_radius, knn)) + NormalizeNormals + OrientNormalsTowardsCameraLocation
    (CloudRegistration.cpp:71-74)."""
    p = np.ascontiguousarray(points, np.float64)
    out = np.zeros_like(p)
    nn = np.zeros((p.shape[0], knn), np.int32) if want_neighbours else None
    _check(_L().o3s_estimate_normals(device, _d(p), p.shape[0], float(max_radius), int(knn), _d(out), _i(nn)), "o3s_estimate_normals")
    return (out, nn) if want_neighbours else out


def computeFPFHFeature(points, normals, radius: float, knn: int, want_spfh: bool = False, want_neighbours: bool = False, device: int = 0):
    """registration::ComputeFPFHFeature(cloud, KDTreeSearchParamHybrid(radius, knn)) (Submap.cpp:272): the N x 33 features (row i =
    Open3D's feature column i); with want_spfh / want_neighbours also the SPFH and the N x knn neighbour lists (-1 padded)."""
    p = np.ascontiguousarray(points, np.float64)
    n = np.ascontiguousarray(normals, np.float64)
    if n.shape != p.shape:
        raise ValueError("points and normals differ in shape")
    N = p.shape[0]
    out = np.zeros((N, 33), np.float64)
    spfh = np.zeros((N, 33), np.float64) if want_spfh else None
    nn = np.zeros((N, max(int(knn), 0)), np.int32) if want_neighbours else None
    _check(_L().o3s_compute_fpfh(device, _d(p), _d(n), N, float(radius), int(knn), _d(out), _d(spfh), _i(nn)), "o3s_compute_fpfh")
    res = (out,) + ((spfh,) if want_spfh else ()) + ((nn,) if want_neighbours else ())
    return res if len(res) > 1 else out


# ---- Open3D's outlier filters (include/outlier_removal/o3s_outlier_removal.h) --------------------------------------------------
class OutlierParamsC(C.Structure):   # o3s_outlier_params
    _fields_ = [("kind", C.c_int32), ("nb", C.c_int32), ("value", C.c_double)]


OUTLIER_NONE, OUTLIER_RADIUS, OUTLIER_STATISTICAL = 0, 1, 2


def outlier_params(kind=OUTLIER_NONE, nb: int = 0, value: float = 0.0) -> OutlierParamsC:
    """kind: 0 / 'none', 1 / 'radius' (nb = nb_points, value = search radius), 2 / 'statistical' (nb = nb_neighbors, value = std_ratio)"""
    k = {"none": 0, "radius": 1, "statistical": 2}.get(kind, kind)
    return OutlierParamsC(int(k), int(nb), float(value))


def _remove_outliers(params: OutlierParamsC, points, normals, device):
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    if n is not None and n.shape != p.shape:
        raise ValueError("points and normals differ in shape")
    N = p.shape[0]
    op = np.zeros_like(p)
    on = np.zeros_like(p) if n is not None else None
    idx = np.zeros(N, np.int64)
    stat = params.kind == OUTLIER_STATISTICAL
    avg = np.zeros(N, np.float64) if stat else None
    st = np.zeros(4, np.float64) if stat else None
    k = C.c_int64()
    fn = _L().o3s_remove_outliers
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(OutlierParamsC), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double),
                   C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    _check(fn(device, C.byref(params), _d(p), _d(n), N, _d(op), _d(on), idx.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(k), _d(avg), _d(st)),
           "o3s_remove_outliers")
    m = k.value
    return op[:m].copy(), (None if on is None else on[:m].copy()), idx[:m].copy(), avg, st


def remove_radius_outlier(points, nb_points: int, radius: float, normals=None, device: int = 0):
    """PointCloud::RemoveRadiusOutliers(nb_points, radius) -> (points, normals | None, kept indices): a point stays iff more than
    nb_points points (itself included) lie at a squared distance < radius^2.  Input order is kept."""
    op, on, idx, _, _ = _remove_outliers(outlier_params(OUTLIER_RADIUS, nb_points, radius), points, normals, device)
    return op, on, idx


def remove_statistical_outlier(points, nb_neighbors: int, std_ratio: float, normals=None, device: int = 0):
    """PointCloud::RemoveStatisticalOutliers(nb_neighbors, std_ratio) -> (points, normals | None, kept indices, avg_dist (N,),
    stats = [mean, std, thr, valid]): a point stays iff the mean distance to its nb_neighbors nearest points (itself included) is
    positive and below mean + std_ratio * std of those means over the cloud.  Input order is kept."""
    return _remove_outliers(outlier_params(OUTLIER_STATISTICAL, nb_neighbors, std_ratio), points, normals, device)


# ---- DBSCAN clustering and small-cluster removal (include/clustering/o3s_clustering.h) ---------------------------------------
class DbscanParamsC(C.Structure):   # o3s_dbscan_params
    _fields_ = [("eps", C.c_double), ("min_points", C.c_int32), ("min_cluster_size", C.c_int32)]


def dbscan_params(eps: float = 0.0, min_points: int = 0, min_cluster_size: int = 0) -> DbscanParamsC:
    """eps: neighbourhood radius; min_points: neighbours, itself included, that make a point core (0 = off); min_cluster_size:
    clusters with fewer points are removed (0 / 1: only noise goes)"""
    return DbscanParamsC(float(eps), int(min_points), int(min_cluster_size))


def cluster_dbscan(points, eps: float, min_points: int, device: int = 0):
    """PointCloud::ClusterDBSCAN(eps, min_points) -> (labels (N,) int32 with -1 = noise, n_clusters, sizes (n_clusters,) int32):
    clusters are numbered by their smallest core index; a border point takes the smallest id among its core neighbours."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    N = p.shape[0]
    labels = np.full(N, -1, np.int32)
    sizes = np.zeros(N, np.int32)
    k = C.c_int32()
    fn = _L().o3s_cluster_dbscan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(DbscanParamsC), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    q = dbscan_params(eps, min_points, 0)
    _check(fn(device, C.byref(q), _d(p), N, labels.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k), sizes.ctypes.data_as(C.POINTER(C.c_int32))),
           "o3s_cluster_dbscan")
    return labels, int(k.value), sizes[:k.value].copy()


def remove_small_clusters(points, eps: float, min_points: int, min_cluster_size: int, normals=None, device: int = 0):
    """ClusterDBSCAN(eps, min_points), then every point without a cluster or in a cluster of fewer than min_cluster_size points is
    dropped -> (points, normals | None, kept indices, labels of the INPUT points).  Input order is kept."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    if n is not None and n.shape != p.shape:
        raise ValueError("points and normals differ in shape")
    N = p.shape[0]
    op = np.zeros_like(p)
    on = np.zeros_like(p) if n is not None else None
    idx = np.zeros(N, np.int64)
    labels = np.full(N, -1, np.int32)
    k, nc = C.c_int64(), C.c_int32()
    fn = _L().o3s_remove_small_clusters
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(DbscanParamsC), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double),
                   C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    q = dbscan_params(eps, min_points, min_cluster_size)
    _check(fn(device, C.byref(q), _d(p), _d(n), N, _d(op), _d(on), idx.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(k),
              labels.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nc)), "o3s_remove_small_clusters")
    m = k.value
    return op[:m].copy(), (None if on is None else on[:m].copy()), idx[:m].copy(), labels


# ---- ISS keypoints (include/keypoints/o3s_keypoints.h) -------------------------------------------------------------------------
class IssParamsC(C.Structure):   # o3s_iss_params
    _fields_ = [("salient_radius", C.c_double), ("non_max_radius", C.c_double), ("gamma_21", C.c_double), ("gamma_32", C.c_double),
                ("min_neighbors", C.c_int32), ("reserved", C.c_int32)]


def iss_params(salient_radius: float = 0.0, non_max_radius: float = 0.0, gamma_21: float = 0.0, gamma_32: float = 0.0,
               min_neighbors: int = 0) -> IssParamsC:
    """salient_radius / non_max_radius: 0 = six / four times the cloud's resolution; gamma_21 / gamma_32: the bounds on the
    eigenvalue ratios (Open3D: 0.975); min_neighbors: neighbours, itself included, below which a point has no saliency (Open3D: 5;
    0 = off, the zeroed struct)"""
    return IssParamsC(float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32), int(min_neighbors), 0)


def compute_iss_keypoints(points, salient_radius: float = 0.0, non_max_radius: float = 0.0, gamma_21: float = 0.975, gamma_32: float = 0.975,
                          min_neighbors: int = 5, normals=None, device: int = 0):
    """geometry::keypoint::ComputeISSKeypoints -> (points, normals | None, indices, saliency (N,) of the INPUT points, radii =
    [salient, non_max] as used).  Keypoints come as ascending input indices; normals ride along."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64).reshape(-1, 3)
    if n is not None and n.shape != p.shape:
        raise ValueError("points and normals differ in shape")
    N = p.shape[0]
    op = np.zeros_like(p)
    on = np.zeros_like(p) if n is not None else None
    idx = np.zeros(N, np.int64)
    sal = np.zeros(N, np.float64)
    radii = np.zeros(2, np.float64)
    k = C.c_int64()
    fn = _L().o3s_iss_keypoints
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(IssParamsC), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double),
                   C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    q = iss_params(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
    _check(fn(device, C.byref(q), _d(p), _d(n), N, _d(op), _d(on), idx.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(k), _d(sal), _d(radii)),
           "o3s_iss_keypoints")
    m = k.value
    return op[:m].copy(), (None if on is None else on[:m].copy()), idx[:m].copy(), sal, radii


# ---- RANSAC plane segmentation (include/plane_segmentation/o3s_plane_segmentation.h) -----------------------------------------
PLANE_PASS, PLANE_REPEATED, PLANE_NONFINITE, PLANE_DEGENERATE = 0, 1, 2, 3


class PlaneParamsC(C.Structure):   # o3s_plane_params
    _fields_ = [("distance_threshold", C.c_double), ("confidence", C.c_double), ("seed", C.c_uint64), ("num_iterations", C.c_int32),
                ("ransac_n", C.c_int32), ("max_planes", C.c_int32), ("min_inliers", C.c_int32)]


def plane_params(distance_threshold: float = 0.0, ransac_n: int = 0, num_iterations: int = 0, confidence: float = 0.0, seed: int = 0,
                 max_planes: int = 0, min_inliers: int = 0) -> PlaneParamsC:
    """distance_threshold: a point is an inlier iff its distance to the plane is below it; ransac_n: indices per sample (3 .. 8, the
    first three define the plane); num_iterations: 0 = off (the zeroed struct); confidence: (0, 1], 1 never stops early; max_planes:
    planes peeled one after another (1 .. 16); min_inliers: a plane with fewer inliers ends the peel."""
    return PlaneParamsC(float(distance_threshold), float(confidence), int(seed), int(num_iterations), int(ransac_n), int(max_planes),
                        int(min_inliers))


class PlaneResult:
    """What segment_plane found beside (plane_model, inliers): best_iteration (-1: nothing passed), the final est_k and the number of
    PASS iterations the serial loop reached."""

    def __init__(self, plane_model, inliers, best_iteration, est_k, evaluated):
        self.plane_model, self.inliers = plane_model, inliers
        self.best_iteration, self.est_k, self.evaluated = int(best_iteration), int(est_k), int(evaluated)

    def __iter__(self):   # plane_model, inliers = segment_plane(...)
        return iter((self.plane_model, self.inliers))


def _samples(samples, ransac_n):
    if samples is None:
        return None, 0
    t = np.ascontiguousarray(samples, np.int32).reshape(-1, ransac_n)
    return t, t.shape[0]


def segment_plane(points, distance_threshold: float, ransac_n: int = 3, num_iterations: int = 100, confidence: float = 1.0, seed: int = 0,
                  samples=None, device: int = 0) -> PlaneResult:
    """PointCloud::SegmentPlane(distance_threshold, ransac_n, num_iterations) -> (plane_model (4,), inliers (n,) int64 ascending), a
    PlaneResult that unpacks as that pair.  Reproducible: the samples come from a counter-based stream of `seed` (or from the rows of
    `samples`), and the result does not depend on how the device batches the hypotheses."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    N = p.shape[0]
    t, nt = _samples(samples, ransac_n)
    model = np.zeros(4)
    idx = np.zeros(max(N, 1), np.int64)
    k, best, est, ev = C.c_int64(0), C.c_int64(-1), C.c_int64(0), C.c_int64(0)
    lp = C.POINTER(C.c_int64)
    fn = _L().o3s_segment_plane
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(PlaneParamsC), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_double), lp, lp, lp,
                   lp, lp]
    q = plane_params(distance_threshold, ransac_n, num_iterations, confidence, seed, 1, 0)
    _check(fn(device, C.byref(q), _d(p), N, _i(t), nt, _d(model), idx.ctypes.data_as(lp), C.byref(k), C.byref(best), C.byref(est), C.byref(ev)),
           "o3s_segment_plane")
    return PlaneResult(model, idx[:k.value].copy(), best.value, est.value, ev.value)


def segment_planes(points, distance_threshold: float, max_planes: int, min_inliers: int = 3, ransac_n: int = 3, num_iterations: int = 100,
                   confidence: float = 1.0, seed: int = 0, device: int = 0):
    """Up to max_planes planes peeled one after another, each a segment_plane of what the planes before left ->
    (labels (N,) int32 with -1 = no plane, models (n_planes, 4), counts (n_planes,) int64)."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    N = p.shape[0]
    labels = np.full(N, -1, np.int32)
    models = np.zeros((max(int(max_planes), 1), 4))
    counts = np.zeros(max(int(max_planes), 1), np.int64)
    k = C.c_int32(0)
    fn = _L().o3s_segment_planes
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(PlaneParamsC), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                   C.POINTER(C.c_int64)]
    q = plane_params(distance_threshold, ransac_n, num_iterations, confidence, seed, max_planes, min_inliers)
    _check(fn(device, C.byref(q), _d(p), N, _i(labels), C.byref(k), _d(models), counts.ctypes.data_as(C.POINTER(C.c_int64))), "o3s_segment_planes")
    return labels, models[:k.value].copy(), counts[:k.value].copy()


def plane_evaluate_samples(points, distance_threshold: float, ransac_n: int = 3, seed: int = 0, samples=None, first_iteration: int = 0,
                           count: int = None, device: int = 0):
    """The stages of a segmentation for `count` iterations of the stream from first_iteration, or for the rows of `samples`, nothing
    selected -> (outcome (count,) int32, planes (count, 4), n_in (count,) int64, err (count,)); zeros where the outcome is not PASS."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    t, nt = _samples(samples, ransac_n)
    H = nt if count is None else int(count)
    outcome = np.zeros(H, np.int32)
    planes = np.zeros((H, 4))
    n_in = np.zeros(H, np.int64)
    err = np.zeros(H)
    fn = _L().o3s_plane_evaluate_samples
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(PlaneParamsC), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.c_int64, C.c_int64, C.POINTER(C.c_int32),
                   C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    q = plane_params(distance_threshold, ransac_n, max(H, 1), 1.0, seed, 1, 0)
    _check(fn(device, C.byref(q), _d(p), p.shape[0], _i(t), int(first_iteration), H, _i(outcome), _d(planes), n_in.ctypes.data_as(C.POINTER(C.c_int64)),
              _d(err)), "o3s_plane_evaluate_samples")
    return outcome, planes, n_in, err


def plane_reserve(max_points: int, num_iterations: int, device: int = 0) -> None:
    fn = _L().o3s_plane_reserve
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int64, C.c_int32]
    _check(fn(device, int(max_points), int(num_iterations)), "o3s_plane_reserve")


def plane_release(device: int = 0) -> None:
    fn = _L().o3s_plane_release
    fn.restype = C.c_int
    fn.argtypes = [C.c_int]
    _check(fn(device), "o3s_plane_release")


def plane_device_bytes(device: int = 0) -> int:
    fn = _L().o3s_plane_device_bytes
    fn.restype = C.c_int64
    fn.argtypes = [C.c_int]
    return int(fn(device))


# ---- the same operators with colours / covariances riding along (include/o3s_cloud_ops.h, *_attr entry points) ----------
def _attr_call(fn_name, lead_args, points, normals, colors, covariances, want_idx, device):
    p = np.ascontiguousarray(points, np.float64)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64)
    col = None if colors is None else np.ascontiguousarray(colors, np.float64)
    cov = None if covariances is None else np.ascontiguousarray(covariances, np.float64).reshape(-1, 9)
    op = np.zeros_like(p)
    on = np.zeros_like(p) if n is not None else None
    oc = np.zeros_like(p) if col is not None else None
    ov = np.zeros((p.shape[0], 9)) if cov is not None else None
    oi = np.zeros((p.shape[0], 3), np.int32) if want_idx else None
    k = C.c_int64()
    L = _L()
    fn = getattr(L, fn_name)
    dp = C.POINTER(C.c_double)
    args = [device] + lead_args + [_d(p), _d(n), _d(col), _d(cov), C.c_int64(p.shape[0]), _d(op), _d(on), _d(oc), _d(ov)]
    if want_idx:
        args.append(_i(oi))
    args.append(C.byref(k))
    fn.restype = C.c_int
    fn.argtypes = None
    _check(fn(*args), fn_name)
    m = k.value
    out = [op[:m].copy(), None if on is None else on[:m].copy(), None if oc is None else oc[:m].copy(), None if ov is None else ov[:m].copy()]
    if want_idx:
        out.append(oi[:m].copy())
    return tuple(out)


def crop_attr(cropper: CropperC, points, normals=None, colors=None, covariances=None, device: int = 0):
    """CroppingVolume::crop with colours and covariances (croppers.cpp:76-106) -> (points, normals, colors, covariances)."""
    return _attr_call("o3s_crop_attr", [C.byref(cropper)], points, normals, colors, covariances, False, device)


def _rgb(v):
    return None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (3,)))


def color_range_crop(points, normals=None, colors=None, covariances=None, rgb_min=None, rgb_max=None, device: int = 0):
    """ColorRangeCropper::crop (croppers.cpp:178-244) -> (points, normals, colors, covariances): the points whose colour lies in
    [rgb_min, rgb_max] (inclusive; None: the reference's 0 / 1), in order; a cloud without colours comes back whole."""
    lo, hi = _rgb(rgb_min), _rgb(rgb_max)
    return _attr_call("o3s_color_range_crop", [_d(lo), _d(hi)], points, normals, colors, covariances, False, device)


def voxelizeWithinCroppingVolume_attr(voxel_size: float, cropper: CropperC, points, normals=None, colors=None, covariances=None, device: int = 0):
    """voxelizeWithinCroppingVolume with colours (last colour of the voxel) and covariances (mean) -> (p, n, col, cov, voxel_idx)."""
    return _attr_call("o3s_voxelize_within_crop_attr", [C.byref(cropper), C.c_double(float(voxel_size))], points, normals, colors, covariances, True, device)


def voxelize_attr(voxel_size: float, points, normals=None, colors=None, covariances=None, device: int = 0):
    """Open3D VoxelDownSample with mean colours / covariances -> (p, n, col, cov, voxel_idx)."""
    return _attr_call("o3s_voxel_downsample_attr", [C.c_double(float(voxel_size))], points, normals, colors, covariances, True, device)


def transform(T, points, normals=None, covariances=None, device: int = 0):
    """o3d_slam::transform (helpers.cpp:283-318) -> (points, normals, covariances); an (almost-)identity T doubles the cloud."""
    p = np.ascontiguousarray(points, np.float64)
    n = None if normals is None else np.ascontiguousarray(normals, np.float64)
    cov = None if covariances is None else np.ascontiguousarray(covariances, np.float64).reshape(-1, 9)
    Tc = np.ascontiguousarray(np.asarray(T, np.float64).T).reshape(16)
    op = np.zeros((2 * p.shape[0], 3))
    on = np.zeros((2 * p.shape[0], 3)) if n is not None else None
    ov = np.zeros((2 * p.shape[0], 9)) if cov is not None else None
    k = C.c_int64()
    L = _L()
    L.o3s_transform_cloud.restype = C.c_int
    L.o3s_transform_cloud.argtypes = None
    _check(L.o3s_transform_cloud(device, _d(Tc), _d(p), _d(n), _d(cov), C.c_int64(p.shape[0]), _d(op), _d(on), _d(ov), C.byref(k)), "o3s_transform_cloud")
    m = k.value
    return op[:m].copy(), (None if on is None else on[:m].copy()), (None if ov is None else ov[:m].copy())
