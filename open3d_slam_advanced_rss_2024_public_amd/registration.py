"""Host-side mirror of the Open3D registration calls the reference makes outside the scan-to-map path (loop-closure
refinement, odometry constraints) over the C ABI (include/o3s_registration.h).  Names follow Open3D."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .cloud_ops import _d


class _Criteria(C.Structure):
    _fields_ = [("relative_fitness", C.c_double), ("relative_rmse", C.c_double), ("max_iteration", C.c_int32)]


class _Result(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("correspondences", C.c_int64), ("iterations", C.c_int32)]


class _Pair(C.Structure):
    _fields_ = [("source", C.POINTER(C.c_double)), ("n_source", C.c_int64), ("target", C.POINTER(C.c_double)),
                ("target_normals", C.POINTER(C.c_double)), ("n_target", C.c_int64), ("init", C.c_double * 16)]


class _Estimation(C.Structure):
    _fields_ = [("type", C.c_int32), ("gicp_epsilon", C.c_double), ("reserved", C.c_int32 * 4)]


# CloudRegistrationType (open3d_slam Parameters.hpp:37-42): the strings of scan_to_map_refinement_type -> o3s_o3d_estimation_type
REGISTRATION_TYPES = {"PointToPlaneIcp": 0, "PointToPointIcp": 1, "GeneralizedIcp": 2}


def _estimation(registration_type, epsilon=1e-3):
    if registration_type not in REGISTRATION_TYPES:
        raise ValueError(f"registration_type must be one of {sorted(REGISTRATION_TYPES)}, not {registration_type!r}")
    return _Estimation(REGISTRATION_TYPES[registration_type], float(epsilon))


@dataclass
class RegistrationResult:
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    correspondences: int
    iterations: int


class _RansacParams(C.Structure):
    _fields_ = [("max_correspondence_distance", C.c_double), ("ransac_n", C.c_int32), ("distance_threshold", C.c_double),
                ("edge_length_similarity", C.c_double), ("check_distance", C.c_int32), ("check_edge_length", C.c_int32),
                ("max_iteration", C.c_int32), ("confidence", C.c_double), ("seed", C.c_uint64)]


class _RansacResult(C.Structure):
    _fields_ = [("transformation", C.c_double * 16), ("fitness", C.c_double), ("inlier_rmse", C.c_double), ("correspondences", C.c_int64),
                ("best_iteration", C.c_int64), ("est_k", C.c_int64), ("evaluated", C.c_int64)]


@dataclass
class RansacParams:
    """o3s_ransac_params; the defaults are the reference's (param_robosense_rs16.lua place_recognition: ransac_max_correspondence_dist,
    ransac_model_size, the two checkers of PlaceRecognition.cpp, ransac_num_iter, ransac_probability)."""
    max_correspondence_distance: float = 0.75
    ransac_n: int = 3
    distance_threshold: float = 0.8
    edge_length_similarity: float = 0.6
    check_distance: bool = True
    check_edge_length: bool = True
    max_iteration: int = 10_000_000
    confidence: float = 0.999
    seed: int = 0

    def to_c(self) -> _RansacParams:
        return _RansacParams(float(self.max_correspondence_distance), int(self.ransac_n), float(self.distance_threshold),
                             float(self.edge_length_similarity), int(bool(self.check_distance)), int(bool(self.check_edge_length)),
                             int(self.max_iteration), float(self.confidence), int(self.seed) & 0xFFFFFFFFFFFFFFFF)


@dataclass
class RansacResult:
    """Open3D's RegistrationResult of a RANSAC (transformation_, fitness_, inlier_rmse_, correspondence_set_) and the deterministic
    loop's account of itself: the winning iteration (-1: the empty result), the final est_k, the hypotheses evaluated."""
    transformation: np.ndarray
    fitness: float
    inlier_rmse: float
    correspondence_set: np.ndarray
    best_iteration: int
    est_k: int
    evaluated: int
    n_correspondences: int = 0   # K, the size of the correspondence set the RANSAC ran on




def _L():
    L = _lib.lib()
    if _lib.needs_binding(L, __name__):  # once per loaded library (product or test-hook build)
        dp = C.POINTER(C.c_double)
        L.o3s_o3d_registration_icp.argtypes = [C.c_int, dp, C.c_int64, dp, dp, C.c_int64, C.c_double, dp, C.POINTER(_Criteria), C.POINTER(_Result)]
        L.o3s_o3d_information_matrix.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_double, dp, dp]
        L.o3s_o3d_registration_icp_submaps.argtypes = [C.c_void_p, C.c_void_p, C.c_double, dp, C.POINTER(_Criteria), C.POINTER(_Result), dp]
        L.o3s_o3d_registration_icp_ex.argtypes = [C.c_int, dp, dp, dp, C.c_int64, dp, dp, dp, C.c_int64, C.c_double, dp, C.POINTER(_Estimation),
                                                  C.POINTER(_Criteria), C.POINTER(_Result)]
        L.o3s_o3d_default_estimation.argtypes = [C.POINTER(_Estimation)]
        L.o3s_o3d_default_estimation.restype = None
        L.o3s_o3d_registration_icp_batch.argtypes = [C.c_int, C.c_int32, C.POINTER(_Pair), C.c_double, C.POINTER(_Criteria), C.POINTER(_Result), dp,
                                                     C.POINTER(C.c_int32)]
        ip = C.POINTER(C.c_int32)
        L.o3s_feature_correspondences.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, ip, C.POINTER(C.c_int64), ip]
        rp, rr, lp = C.POINTER(_RansacParams), C.POINTER(_RansacResult), C.POINTER(C.c_int64)
        L.o3s_ransac_default_params.argtypes = [rp]
        L.o3s_ransac_default_params.restype = None
        L.o3s_registration_ransac_correspondence.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, ip, C.c_int64, rp, ip, C.c_int64, rr, ip]
        L.o3s_registration_ransac_feature_matching.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, dp, dp, C.c_int32, C.c_int32, rp, rr, ip, lp]
        L.o3s_ransac_evaluate_samples.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, ip, C.c_int64, rp, ip, C.c_int64, C.c_int64, ip, dp, lp, dp]
        L.o3s_ransac_reserve.argtypes = [C.c_int, C.c_int64]
        L.o3s_ransac_release.argtypes = [C.c_int]
        L.o3s_submap_registration_ransac.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, rp, rr, ip, lp]
    return L


def featureCorrespondences(source_feature, target_feature, mutual_filter: bool = True, ransac_n: int = 3, device: int = 0):
    """The head of RegistrationRANSACBasedOnFeatureMatching (PlaceRecognition.cpp:81-84): (pairs, used_fallback) with pairs a K x 2
    int32 array of (source index, target index) — nearest target feature of every source feature, kept where the relation is mutual
    (all of them when fewer than 3 ransac_n are, or without mutual_filter).  Features are N x dim arrays (row i = feature column i)."""
    a = np.ascontiguousarray(source_feature, np.float64)
    b = np.ascontiguousarray(target_feature, np.float64)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("features must be N x dim arrays of one dim")
    pairs = np.zeros((a.shape[0], 2), np.int32)
    n_out, fb = C.c_int64(0), C.c_int32(0)
    rc = _L().o3s_feature_correspondences(device, _d(a), a.shape[0], _d(b), b.shape[0], a.shape[1], int(bool(mutual_filter)), int(ransac_n),
                                          pairs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_out), C.byref(fb))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_feature_correspondences failed with o3s_status {rc}")
    return pairs[:n_out.value].copy(), bool(fb.value)


def _pose(T):
    return np.ascontiguousarray(np.asarray(T, np.float64).T).reshape(16)


def registration_icp(source, target, target_normals, max_correspondence_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                     max_iteration=30, device: int = 0) -> RegistrationResult:
    """RegistrationICP(source, target, max_correspondence_distance, init, TransformationEstimationPointToPlane(), criteria)."""
    s_ = np.ascontiguousarray(source, np.float64)
    t_ = np.ascontiguousarray(target, np.float64)
    n_ = None if target_normals is None else np.ascontiguousarray(target_normals, np.float64)
    cr = _Criteria(float(relative_fitness), float(relative_rmse), int(max_iteration))
    r = _Result()
    rc = _L().o3s_o3d_registration_icp(device, _d(s_), s_.shape[0], _d(t_), _d(n_), t_.shape[0], float(max_correspondence_distance),
                                       _d(_pose(np.eye(4) if init is None else init)), C.byref(cr), C.byref(r))
    if rc == _lib.ERR_BAD_SHAPE:
        raise RuntimeError("TransformationEstimationPointToPlane requires target normals")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_o3d_registration_icp failed with o3s_status {rc}")
    return RegistrationResult(np.array(r.transformation).reshape(4, 4).T.copy(), r.fitness, r.inlier_rmse, int(r.correspondences), int(r.iterations))


def _result(r):
    return RegistrationResult(np.array(r.transformation).reshape(4, 4).T.copy(), r.fitness, r.inlier_rmse, int(r.correspondences), int(r.iterations))


def _cloud(a, width):
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float64)
    return a.reshape(a.shape[0], width) if width == 9 else a


def _registration_icp_ex(est, source, target, max_correspondence_distance, init, source_normals, target_normals, source_covariances,
                         target_covariances, relative_fitness, relative_rmse, max_iteration, device):
    s_ = np.ascontiguousarray(source, np.float64)
    t_ = np.ascontiguousarray(target, np.float64)
    sn, tn = _cloud(source_normals, 3), _cloud(target_normals, 3)
    sc, tc = _cloud(source_covariances, 9), _cloud(target_covariances, 9)
    for a, n_, what in ((sn, s_.shape[0], "source normals"), (tn, t_.shape[0], "target normals"), (sc, s_.shape[0], "source covariances"),
                        (tc, t_.shape[0], "target covariances")):
        if a is not None and a.shape[0] != n_:
            raise ValueError(f"{what}: {a.shape[0]} rows for {n_} points")
    cr = _Criteria(float(relative_fitness), float(relative_rmse), int(max_iteration))
    r = _Result()
    rc = _L().o3s_o3d_registration_icp_ex(device, _d(s_), _d(sn), _d(sc), s_.shape[0], _d(t_), _d(tn), _d(tc), t_.shape[0],
                                          float(max_correspondence_distance), _d(_pose(np.eye(4) if init is None else init)), C.byref(est),
                                          C.byref(cr), C.byref(r))
    if rc == _lib.ERR_BAD_SHAPE:
        raise RuntimeError("the registration needs normals or covariances the clouds do not carry (point-to-plane: target normals; "
                           "Generalized ICP: normals or covariances on both clouds)")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_o3d_registration_icp_ex failed with o3s_status {rc}")
    return _result(r)


def registration_generalized_icp(source, target, max_correspondence_distance, init=None, epsilon=1e-3, source_normals=None, target_normals=None,
                                 source_covariances=None, target_covariances=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                                 device: int = 0) -> RegistrationResult:
    """RegistrationGeneralizedICP(source, target, max_correspondence_distance, init, TransformationEstimationForGeneralizedICP(epsilon),
    criteria) — the loop-closure refinement the reference's parameters select (CloudRegistration.cpp:16-21).  Each cloud needs normals
    (covariances eps / 1 / 1 around them, the normal as given) or covariances (N x 3 x 3 or N x 9, column-major per point; they win)."""
    return _registration_icp_ex(_estimation("GeneralizedIcp", epsilon), source, target, max_correspondence_distance, init, source_normals,
                                target_normals, source_covariances, target_covariances, relative_fitness, relative_rmse, max_iteration, device)


def registration_icp_point_to_point(source, target, max_correspondence_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                                    max_iteration=30, device: int = 0) -> RegistrationResult:
    """RegistrationICP(source, target, max_correspondence_distance, init, TransformationEstimationPointToPoint(false), criteria)
    (CloudRegistration.cpp:88-101): Eigen::umeyama over the correspondences, no normals needed."""
    return _registration_icp_ex(_estimation("PointToPointIcp"), source, target, max_correspondence_distance, init, None, None, None, None,
                                relative_fitness, relative_rmse, max_iteration, device)


def default_estimation():
    """o3s_o3d_default_estimation: (registration type name, epsilon) the reference's parameters select."""
    e = _Estimation()
    _L().o3s_o3d_default_estimation(C.byref(e))
    return {v: k for k, v in REGISTRATION_TYPES.items()}[e.type], e.gicp_epsilon


def get_information_matrix_from_point_clouds(source, target, max_correspondence_distance, transformation, device: int = 0) -> np.ndarray:
    s_ = np.ascontiguousarray(source, np.float64)
    t_ = np.ascontiguousarray(target, np.float64)
    out = np.zeros(36)
    rc = _L().o3s_o3d_information_matrix(device, _d(s_), s_.shape[0], _d(t_), t_.shape[0], float(max_correspondence_distance),
                                         _d(_pose(transformation)), _d(out))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_o3d_information_matrix failed with o3s_status {rc}")
    return out.reshape(6, 6).T.copy()


def registration_icp_batch(pairs, max_correspondence_distance, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                           with_information: bool = False, device: int = 0):
    """RegistrationICP over independent candidate pairs, run concurrently on one device (the loop-closure candidates of
    PlaceRecognition.cpp:70-150).  pairs: sequence of (source, target, target_normals, init | None).
    Returns [RegistrationResult] — and [6x6 information matrix] with with_information."""
    n = len(pairs)
    if n == 0:
        return ([], []) if with_information else []
    keep = []  # the arrays the structs point into
    arr = (_Pair * n)()
    for k, (src, tgt, tn, init) in enumerate(pairs):
        s_ = np.ascontiguousarray(src, np.float64)
        t_ = np.ascontiguousarray(tgt, np.float64)
        if tn is None:
            raise RuntimeError("TransformationEstimationPointToPlane requires target normals")
        n_ = np.ascontiguousarray(tn, np.float64)
        keep += [s_, t_, n_]
        arr[k].source, arr[k].n_source = _d(s_), s_.shape[0]
        arr[k].target, arr[k].target_normals, arr[k].n_target = _d(t_), _d(n_), t_.shape[0]
        arr[k].init = (C.c_double * 16)(*_pose(np.eye(4) if init is None else init))
    cr = _Criteria(float(relative_fitness), float(relative_rmse), int(max_iteration))
    res = (_Result * n)()
    status = (C.c_int32 * n)()
    infos = np.zeros((n, 36)) if with_information else None
    rc = _L().o3s_o3d_registration_icp_batch(device, n, arr, float(max_correspondence_distance), C.byref(cr), res, _d(infos), status)
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_o3d_registration_icp_batch failed with o3s_status {rc} (per pair: {list(status)})")
    out = [RegistrationResult(np.array(r.transformation).reshape(4, 4).T.copy(), r.fitness, r.inlier_rmse, int(r.correspondences), int(r.iterations))
           for r in res]
    if with_information:
        return out, [infos[k].reshape(6, 6).T.copy() for k in range(n)]
    return out


def registration_icp_submaps(source_submap, target_submap, max_correspondence_distance, init=None, relative_fitness=1e-6, relative_rmse=1e-6,
                             max_iteration=30, with_information: bool = False):
    """RegistrationICP between the map clouds of two device-resident Submap objects (constraint_builders.cpp:55-75,
    PlaceRecognition.cpp:111): neither cloud leaves HBM.  Returns RegistrationResult (and the 6x6 information matrix)."""
    cr = _Criteria(float(relative_fitness), float(relative_rmse), int(max_iteration))
    r = _Result()
    info = np.zeros(36) if with_information else None
    rc = _L().o3s_o3d_registration_icp_submaps(source_submap._h, target_submap._h, float(max_correspondence_distance),
                                               _d(_pose(np.eye(4) if init is None else init)), C.byref(cr), C.byref(r), _d(info))
    if rc == _lib.ERR_BAD_SHAPE:
        raise RuntimeError("TransformationEstimationPointToPlane requires target normals")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_o3d_registration_icp_submaps failed with o3s_status {rc}")
    res = RegistrationResult(np.array(r.transformation).reshape(4, 4).T.copy(), r.fitness, r.inlier_rmse, int(r.correspondences), int(r.iterations))
    return (res, info.reshape(6, 6).T.copy()) if with_information else res


def compute_indices_of_overlapping_points(source, target, source_to_target, voxel_size, min_num_points_per_voxel: int = 1, device: int = 0):
    """computeIndicesOfOverlappingPoints (open3d_slam/src/helpers.cpp:319-345): (idxsSource, idxsTarget), ascending."""
    s_ = np.ascontiguousarray(source, np.float64)
    t_ = np.ascontiguousarray(target, np.float64)
    i_s = np.zeros(max(s_.shape[0], 1), np.int64)
    i_t = np.zeros(max(t_.shape[0], 1), np.int64)
    ns, nt = C.c_int64(), C.c_int64()
    L = _L()
    ip = C.POINTER(C.c_int64)
    L.o3s_overlap_indices.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.c_double,
                                      C.c_int64, ip, ip, ip, ip]
    rc = L.o3s_overlap_indices(device, _d(s_), s_.shape[0], _d(t_), t_.shape[0], _d(_pose(source_to_target)), float(voxel_size),
                               int(min_num_points_per_voxel), i_s.ctypes.data_as(ip), C.byref(ns), i_t.ctypes.data_as(ip), C.byref(nt))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_overlap_indices failed with o3s_status {rc}")
    return i_s[:ns.value].copy(), i_t[:nt.value].copy()


def registration_icp_submaps_overlap(source_submap, target_submap, max_correspondence_distance, init, overlap_voxel_size,
                                     min_num_points_per_voxel: int = 1, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                                     with_information: bool = True, registration_type: str = "PointToPlaneIcp", gicp_epsilon: float = 1e-3):
    """The loop-closure refinement of PlaceRecognition::buildLoopClosureConstraints (PlaceRecognition.cpp:97-150) between two
    device-resident Submap objects: overlap selection at `init`, RegistrationICP on the selections, information matrix.
    registration_type: the reference's CloudRegistrationType string ("PointToPlaneIcp", "PointToPointIcp", "GeneralizedIcp" — the
    last is what its parameter sets select); the default keeps the point-to-plane refinement.
    Returns (RegistrationResult, information 6x6 or None, (n_source_overlap, n_target_overlap)); an empty overlap gives None."""
    est = _estimation(registration_type, gicp_epsilon)
    cr = _Criteria(float(relative_fitness), float(relative_rmse), int(max_iteration))
    r = _Result()
    info = np.zeros(36) if with_information else None
    n_ov = (C.c_int64 * 2)()
    L = _L()
    if est.type == 0:
        L.o3s_o3d_registration_icp_submaps_overlap.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(_Criteria),
                                                               C.c_double, C.c_int64, C.POINTER(_Result), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        rc = L.o3s_o3d_registration_icp_submaps_overlap(source_submap._h, target_submap._h, float(max_correspondence_distance), _d(_pose(init)),
                                                        C.byref(cr), float(overlap_voxel_size), int(min_num_points_per_voxel), C.byref(r), _d(info), n_ov)
        name = "o3s_o3d_registration_icp_submaps_overlap"
    else:
        L.o3s_o3d_registration_icp_submaps_overlap_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(_Estimation),
                                                                  C.POINTER(_Criteria), C.c_double, C.c_int64, C.POINTER(_Result), C.POINTER(C.c_double),
                                                                  C.POINTER(C.c_int64)]
        rc = L.o3s_o3d_registration_icp_submaps_overlap_ex(source_submap._h, target_submap._h, float(max_correspondence_distance), _d(_pose(init)),
                                                           C.byref(est), C.byref(cr), float(overlap_voxel_size), int(min_num_points_per_voxel),
                                                           C.byref(r), _d(info), n_ov)
        name = "o3s_o3d_registration_icp_submaps_overlap_ex"
    if rc == _lib.ERR_EMPTY_REFERENCE:
        return None, None, (int(n_ov[0]), int(n_ov[1]))
    if rc == _lib.ERR_BAD_SHAPE:
        raise RuntimeError("TransformationEstimationPointToPlane requires target normals" if est.type == 0 else
                           f"{registration_type} needs normals the submaps do not carry")
    if rc != _lib.OK:
        raise RuntimeError(f"{name} failed with o3s_status {rc}")
    res = RegistrationResult(np.array(r.transformation).reshape(4, 4).T.copy(), r.fitness, r.inlier_rmse, int(r.correspondences), int(r.iterations))
    return res, (info.reshape(6, 6).T.copy() if with_information else None), (int(n_ov[0]), int(n_ov[1]))


def registration_icp_submaps_overlap_batch(pairs, max_correspondence_distance, overlap_voxel_size, min_num_points_per_voxel: int = 1,
                                           relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, registration_type: str = "PointToPlaneIcp",
                                           gicp_epsilon: float = 1e-3):
    """o3s_o3d_registration_icp_submaps_overlap_batch: the loop-closure refinement for several (source Submap, target Submap, init)
    triples at once, up to four in flight on the device.  registration_type as in registration_icp_submaps_overlap.  Returns a list
    of (RegistrationResult | None, information 6x6 | None, (n_source_overlap, n_target_overlap), status) — None for a pair whose
    overlap is empty (or, with status O3S_ERR_BAD_SHAPE, whose submaps lack the normals the type needs)."""
    est = _estimation(registration_type, gicp_epsilon)
    n = len(pairs)
    if n == 0:
        return []
    cr = _Criteria(float(relative_fitness), float(relative_rmse), int(max_iteration))
    srcs = (C.c_void_p * n)(*[p_[0]._h for p_ in pairs])
    tgts = (C.c_void_p * n)(*[p_[1]._h for p_ in pairs])
    inits = np.ascontiguousarray(np.stack([_pose(p_[2]) for p_ in pairs]), np.float64)
    res = (_Result * n)()
    infos = np.zeros((n, 36))
    novs = (C.c_int64 * (2 * n))()
    sts = (C.c_int32 * n)()
    L = _L()
    if est.type == 0:
        L.o3s_o3d_registration_icp_submaps_overlap_batch.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_double,
                                                                     C.POINTER(C.c_double), C.POINTER(_Criteria), C.c_double, C.c_int64, C.POINTER(_Result),
                                                                     C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        rc = L.o3s_o3d_registration_icp_submaps_overlap_batch(n, srcs, tgts, float(max_correspondence_distance), _d(inits), C.byref(cr),
                                                              float(overlap_voxel_size), int(min_num_points_per_voxel), res, _d(infos), novs, sts)
        name = "o3s_o3d_registration_icp_submaps_overlap_batch"
    else:
        L.o3s_o3d_registration_icp_submaps_overlap_batch_ex.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_double,
                                                                        C.POINTER(C.c_double), C.POINTER(_Estimation), C.POINTER(_Criteria), C.c_double,
                                                                        C.c_int64, C.POINTER(_Result), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                                                        C.POINTER(C.c_int32)]
        rc = L.o3s_o3d_registration_icp_submaps_overlap_batch_ex(n, srcs, tgts, float(max_correspondence_distance), _d(inits), C.byref(est), C.byref(cr),
                                                                 float(overlap_voxel_size), int(min_num_points_per_voxel), res, _d(infos), novs, sts)
        name = "o3s_o3d_registration_icp_submaps_overlap_batch_ex"
    if rc != _lib.OK:
        raise RuntimeError(f"{name} failed with o3s_status {rc}")
    out = []
    for k in range(n):
        nov = (int(novs[2 * k]), int(novs[2 * k + 1]))
        if sts[k] != _lib.OK:
            out.append((None, None, nov, int(sts[k])))
            continue
        r = res[k]
        out.append((RegistrationResult(np.array(r.transformation).reshape(4, 4).T.copy(), r.fitness, r.inlier_rmse, int(r.correspondences), int(r.iterations)),
                    infos[k].reshape(6, 6).T.copy(), nov, 0))
    return out


def reserve(max_source_points: int, max_target_points: int, device: int = 0):
    """o3s_o3d_registration_reserve: sizes the device's registration work area once, so that no registration of clouds up to these
    sizes allocates (an allocation stalls every stream of the device for milliseconds)."""
    L = _L()
    L.o3s_o3d_registration_reserve.argtypes = [C.c_int, C.c_int64, C.c_int64]
    rc = L.o3s_o3d_registration_reserve(int(device), int(max_source_points), int(max_target_points))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_o3d_registration_reserve failed with o3s_status {rc}")


def reserve_n(max_source_points: int, max_target_points: int, count: int, device: int = 0):
    """o3s_o3d_registration_reserve_n: `count` work areas of that size (the lanes of the batch entries)."""
    L = _L()
    L.o3s_o3d_registration_reserve_n.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int32]
    rc = L.o3s_o3d_registration_reserve_n(int(device), int(max_source_points), int(max_target_points), int(count))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_o3d_registration_reserve_n failed with o3s_status {rc}")


def release(device: int = 0):
    """o3s_o3d_registration_release: the idle registration work areas of the device go back to the allocator."""
    L = _L()
    L.o3s_o3d_registration_release.argtypes = [C.c_int]
    rc = L.o3s_o3d_registration_release(int(device))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_o3d_registration_release failed with o3s_status {rc}")


# ---- RANSAC on feature correspondences (include/o3s_registration.h, "RANSAC": the contract) ------------------------------------
def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _ransac_result(r, inl, k) -> RansacResult:
    n = int(r.correspondences)
    return RansacResult(np.array(r.transformation).reshape(4, 4).T.copy(), r.fitness, r.inlier_rmse, inl[:n].copy(), int(r.best_iteration),
                        int(r.est_k), int(r.evaluated), int(k))


def _ransac_params(params) -> _RansacParams:
    return (RansacParams() if params is None else params).to_c()


def default_ransac_params() -> RansacParams:
    """o3s_ransac_default_params."""
    c = _RansacParams()
    _L().o3s_ransac_default_params(C.byref(c))
    return RansacParams(c.max_correspondence_distance, c.ransac_n, c.distance_threshold, c.edge_length_similarity, bool(c.check_distance),
                        bool(c.check_edge_length), c.max_iteration, c.confidence, c.seed)


def registration_ransac_based_on_correspondence(source, target, corres, params: RansacParams = None, samples=None, device: int = 0) -> RansacResult:
    """RegistrationRANSACBasedOnCorrespondence(source, target, corres, max_correspondence_distance, TransformationEstimationPointToPoint(false),
    ransac_n, {edge length, distance}, RANSACConvergenceCriteria(max_iteration, confidence)), deterministic in (seed, iteration).
    corres: K x 2 int32 (source index, target index); samples (optional): H x ransac_n rows used instead of the Philox draws."""
    s_ = np.ascontiguousarray(source, np.float64)
    t_ = np.ascontiguousarray(target, np.float64)
    c_ = np.ascontiguousarray(corres, np.int32).reshape(-1, 2)
    prm = _ransac_params(params)
    tab = None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(-1, max(int(prm.ransac_n), 1))
    inl = np.zeros((max(c_.shape[0], 1), 2), np.int32)
    r = _RansacResult()
    rc = _L().o3s_registration_ransac_correspondence(device, _d(s_), s_.shape[0], _d(t_), t_.shape[0], _ip(c_), c_.shape[0], C.byref(prm), _ip(tab),
                                                     0 if tab is None else tab.shape[0], C.byref(r), _ip(inl))
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError("o3s_registration_ransac_correspondence: bad argument (ransac_n <= 8, confidence in [0, 1], indices within the clouds)")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_registration_ransac_correspondence failed with o3s_status {rc}")
    return _ransac_result(r, inl, c_.shape[0])


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, mutual_filter: bool = True,
                                                  params: RansacParams = None, device: int = 0) -> RansacResult:
    """RegistrationRANSACBasedOnFeatureMatching (PlaceRecognition.cpp:81-84): featureCorrespondences chained into the RANSAC above.
    Features are N x dim arrays (row i = feature column i)."""
    s_ = np.ascontiguousarray(source, np.float64)
    t_ = np.ascontiguousarray(target, np.float64)
    a = np.ascontiguousarray(source_feature, np.float64)
    b = np.ascontiguousarray(target_feature, np.float64)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or a.shape[0] != s_.shape[0] or b.shape[0] != t_.shape[0]:
        raise ValueError("features must be N x dim arrays of one dim, one row per point")
    prm = _ransac_params(params)
    inl = np.zeros((max(s_.shape[0], 1), 2), np.int32)
    r, k = _RansacResult(), C.c_int64(0)
    rc = _L().o3s_registration_ransac_feature_matching(device, _d(s_), s_.shape[0], _d(t_), t_.shape[0], _d(a), _d(b), a.shape[1],
                                                       int(bool(mutual_filter)), C.byref(prm), C.byref(r), _ip(inl), C.byref(k))
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError("o3s_registration_ransac_feature_matching: bad argument")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_registration_ransac_feature_matching failed with o3s_status {rc}")
    return _ransac_result(r, inl, k.value)


def ransac_evaluate_samples(source, target, corres, params: RansacParams = None, samples=None, first_iteration: int = 0, count: int = None,
                            device: int = 0):
    """Steps 1 - 5 of the contract for given sample rows (H x ransac_n), or for the Philox draws of iterations first_iteration ..
    first_iteration + count - 1: (outcome H int32: 0 passed, 1 repeated index, 2 edge-length, 3 distance; T H x 4 x 4; n_in H; err2 H)."""
    s_ = np.ascontiguousarray(source, np.float64)
    t_ = np.ascontiguousarray(target, np.float64)
    c_ = np.ascontiguousarray(corres, np.int32).reshape(-1, 2)
    prm = _ransac_params(params)
    tab = None if samples is None else np.ascontiguousarray(samples, np.int32).reshape(-1, max(int(prm.ransac_n), 1))
    H = int(count) if tab is None else tab.shape[0]
    out = np.zeros(max(H, 1), np.int32)
    T = np.zeros((max(H, 1), 16))
    n_in = np.zeros(max(H, 1), np.int64)
    err2 = np.zeros(max(H, 1))
    rc = _L().o3s_ransac_evaluate_samples(device, _d(s_), s_.shape[0], _d(t_), t_.shape[0], _ip(c_), c_.shape[0], C.byref(prm), _ip(tab),
                                          int(first_iteration), H, _ip(out), _d(T), n_in.ctypes.data_as(C.POINTER(C.c_int64)), _d(err2))
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError("o3s_ransac_evaluate_samples: bad argument")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_ransac_evaluate_samples failed with o3s_status {rc}")
    return out[:H], T[:H].reshape(H, 4, 4).transpose(0, 2, 1).copy(), n_in[:H], err2[:H]


def ransac_reserve(max_correspondences: int, device: int = 0):
    """o3s_ransac_reserve: sizes one RANSAC work area ahead of time, so that closures up to that many correspondences do not allocate."""
    rc = _L().o3s_ransac_reserve(int(device), int(max_correspondences))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_ransac_reserve failed with o3s_status {rc}")


def ransac_release(device: int = 0):
    rc = _L().o3s_ransac_release(int(device))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_ransac_release failed with o3s_status {rc}")


@dataclass
class LoopClosureConstraint:
    """What PlaceRecognition::buildLoopClosureConstraints keeps of an accepted pair (Constraint: sourceToTarget_, informationMatrix_),
    or why the pair was rejected (`rejected`: None when accepted)."""
    rejected: str = None
    source_to_target: np.ndarray = None
    information_matrix: np.ndarray = None
    ransac: RansacResult = None
    refinement: RegistrationResult = None
    n_overlap: tuple = None


def loop_closure_constraint(source_submap, target_submap, ransac_params: RansacParams = None, mutual_filter: bool = True,
                            ransac_min_correspondence_set_size: int = 25, max_icp_correspondence_distance: float = 0.3,
                            overlap_voxel_size: float = None, min_refinement_fitness: float = 0.7, registration_type: str = "GeneralizedIcp",
                            gicp_epsilon: float = 1e-3, max_iteration: int = 30) -> LoopClosureConstraint:
    """One candidate pair of PlaceRecognition::buildLoopClosureConstraints (PlaceRecognition.cpp:78-152) on two resident submaps with
    feature sets: RANSAC on the feature correspondences, the ransac_min_corresondence_set_size gate, overlap selection at the RANSAC
    pose and refinement with the chosen registration type, the min_refinement_fitness gate, the information matrix.
    overlap_voxel_size: magic::voxelExpansionFactorOverlapComputation x the map voxel size (the caller's; required).
    isRegistrationConsistent and the choice of candidates are place_recognition.PlaceRecognition's, which runs a finished submap
    against all its candidates at once; this call stays the per-pair yardstick."""
    if overlap_voxel_size is None:
        raise ValueError("overlap_voxel_size is required (voxelExpansionFactorOverlapComputation x map voxel size)")
    rr = source_submap.ransacRegistration(target_submap, ransac_params, mutual_filter)
    if len(rr.correspondence_set) < ransac_min_correspondence_set_size:
        return LoopClosureConstraint(rejected=f"ransac: {len(rr.correspondence_set)} correspondences", ransac=rr)
    res, info, n_ov = registration_icp_submaps_overlap(source_submap, target_submap, max_icp_correspondence_distance, rr.transformation,
                                                       overlap_voxel_size, 1, max_iteration=max_iteration, with_information=True,
                                                       registration_type=registration_type, gicp_epsilon=gicp_epsilon)
    if res is None:
        return LoopClosureConstraint(rejected="refinement: empty overlap", ransac=rr, n_overlap=n_ov)
    if res.fitness < min_refinement_fitness:
        return LoopClosureConstraint(rejected=f"refinement score: {res.fitness}", ransac=rr, refinement=res, n_overlap=n_ov)
    return LoopClosureConstraint(None, res.transformation, info, rr, res, n_ov)
