"""Place recognition of a finished submap against all its candidates at once: PlaceRecognition::buildLoopClosureConstraints
(open3d_slam/src/PlaceRecognition.cpp:50-176) with its host policy — getLoopClosureCandidatesIdxs (:231-285), the two
isRegistrationConsistent gates (:182-229) — over the one-to-many front end of the library
(include/place_recognition/o3s_place_recognition.h) and the batched loop-closure refinement
(registration.registration_icp_submaps_overlap_batch).  Python mirror of cpp/o3s_place_recognition.hpp: the same logic."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from . import registration as reg
from .pose_graph import Constraint

MAX_TARGETS = 16   # O3S_PLACE_MAX_TARGETS


def _L(L=None):
    """the library in use, or the one a submap handle belongs to, with this module's argtypes bound"""
    L = reg._L() if L is None else L
    if _lib.needs_binding(L, __name__):
        dp, ip, lp, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_void_p
        L.o3s_feature_correspondences_multi.argtypes = [C.c_int, dp, C.c_int64, C.POINTER(dp), lp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, lp, ip]
        L.o3s_submaps_feature_correspondences.argtypes = [vp, C.POINTER(vp), C.c_int32, C.c_int32, C.c_int32, ip, lp, ip]
        L.o3s_submaps_registration_ransac.argtypes = [vp, C.POINTER(vp), C.c_int32, C.c_int32, C.POINTER(reg._RansacParams),
                                                      C.POINTER(reg._RansacResult), ip, lp]
    return L


def _check(rc, name):
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError(f"{name}: bad argument (1 to {MAX_TARGETS} targets on the source's device, valid parameters)")
    if rc == _lib.ERR_NOT_INITIALIZED:
        raise RuntimeError(f"{name}: every submap needs features: call computeFeatures first")
    if rc != _lib.OK:
        raise RuntimeError(f"{name} failed with o3s_status {rc}")


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def feature_correspondences_multi(source_feature, target_features, mutual_filter: bool = True, ransac_n: int = 3, device: int = 0):
    """registration.featureCorrespondences of one source against up to 16 targets in one call (o3s_feature_correspondences_multi):
    a list of (pairs, used_fallback), one per target, each what the per-pair call gives.  Features are N x dim arrays."""
    a = np.ascontiguousarray(source_feature, np.float64)
    bs = [np.ascontiguousarray(b, np.float64) for b in target_features]
    if a.ndim != 2 or any(b.ndim != 2 or b.shape[1] != a.shape[1] for b in bs):
        raise ValueError("features must be N x dim arrays of one dim")
    K, n = len(bs), a.shape[0]
    dp = C.POINTER(C.c_double)
    ptrs = (dp * max(K, 1))(*[b.ctypes.data_as(dp) for b in bs])
    n_tgt = np.array([b.shape[0] for b in bs] + [0] * (K == 0), np.int64)
    pairs = np.zeros((max(K, 1), max(n, 1), 2), np.int32)
    n_out, fb = np.zeros(max(K, 1), np.int64), np.zeros(max(K, 1), np.int32)
    _check(_L().o3s_feature_correspondences_multi(device, a.ctypes.data_as(dp), n, ptrs, _lp(n_tgt), K, a.shape[1], int(bool(mutual_filter)),
                                                  int(ransac_n), _ip(pairs), _lp(n_out), _ip(fb)), "o3s_feature_correspondences_multi")
    flat = pairs.reshape(-1, 2)
    return [(flat[k * n:k * n + int(n_out[k])].copy(), bool(fb[k])) for k in range(K)]


def _handles(source, targets):
    n = source.features_size()
    if n < 0 or any(t.features_size() < 0 for t in targets):
        raise RuntimeError("every submap needs features: call computeFeatures first")
    return n, (C.c_void_p * max(len(targets), 1))(*[t._h for t in targets])


def submaps_feature_correspondences(source, targets, mutual_filter: bool = True, ransac_n: int = 3):
    """Submap.featureCorrespondences of `source` against up to 16 target submaps in one call (o3s_submaps_feature_correspondences):
    a list of (pairs, used_fallback), one per target; no feature set and no index array leaves HBM."""
    n, hs = _handles(source, targets)
    K = len(targets)
    pairs = np.zeros((max(K, 1), max(n, 1), 2), np.int32)
    n_out, fb = np.zeros(max(K, 1), np.int64), np.zeros(max(K, 1), np.int32)
    _check(_L(source._lib).o3s_submaps_feature_correspondences(source._h, hs, K, int(bool(mutual_filter)), int(ransac_n), _ip(pairs), _lp(n_out), _ip(fb)),
           "o3s_submaps_feature_correspondences")
    flat = pairs.reshape(-1, 2)
    return [(flat[k * n:k * n + int(n_out[k])].copy(), bool(fb[k])) for k in range(K)]


def submaps_registration_ransac(source, targets, params: reg.RansacParams = None, mutual_filter: bool = True):
    """Submap.ransacRegistration of `source` against up to 16 target submaps in one call (o3s_submaps_registration_ransac): a list of
    registration.RansacResult, one per target, each what the per-pair call gives bit for bit."""
    n, hs = _handles(source, targets)
    K = len(targets)
    prm = reg._ransac_params(params)
    inl = np.zeros((max(K, 1), max(n, 1), 2), np.int32)
    res = (reg._RansacResult * max(K, 1))()
    ks = np.zeros(max(K, 1), np.int64)
    _check(_L(source._lib).o3s_submaps_registration_ransac(source._h, hs, K, int(bool(mutual_filter)), C.byref(prm), res, _ip(inl), _lp(ks)),
           "o3s_submaps_registration_ransac")
    return [reg._ransac_result(res[k], inl[k] if n else inl[k][:0], int(ks[k])) for k in range(K)]


# ---- parameters (param/default/parameter_structure_definitions.lua:153-181) ---------------------------------------------------

@dataclass
class ConsistencyCheckParameters:
    """PlaceRecognitionConsistencyCheckParameters: LOOP_CLOSURE_CONSISTENCY_CHECK_PARAMETERS, the angles in RADIANS as
    isRegistrationConsistent compares them (the parameter loader converts the file's degrees)."""
    max_drift_roll: float = math.radians(30.0)
    max_drift_pitch: float = math.radians(30.0)
    max_drift_yaw: float = math.radians(30.0)
    max_drift_x: float = 80.0
    max_drift_y: float = 80.0
    max_drift_z: float = 40.0


@dataclass
class PlaceRecognitionParameters:
    """PlaceRecognitionParameters with the defaults of PLACE_RECOGNITION_PARAMETERS.  overlap_voxel_size is
    magic::voxelExpansionFactorOverlapComputation x the map voxel size — the caller's, required by buildLoopClosureConstraints;
    registration_type / gicp_epsilon / max_icp_iterations describe the refinement (scan_to_map_refinement_type, GeneralizedIcp in the
    reference's parameter sets; icpRunUntilConvergenceNumberOfIterations is the caller's to raise).  feature_keypoints is not the
    reference's: PlaceRecognition.computeFeatures hands it to the collection, which then reduces every finished submap's feature
    set to its ISS keypoints."""
    loop_closure_search_radius: float = 20.0
    min_submaps_between_loop_closures: int = 2
    ransac: reg.RansacParams = field(default_factory=reg.RansacParams)
    mutual_filter: bool = True
    ransac_min_correspondence_set_size: int = 25
    max_icp_correspondence_distance: float = 0.3
    min_refinement_fitness: float = 0.7
    consistency_check: ConsistencyCheckParameters = field(default_factory=ConsistencyCheckParameters)
    overlap_voxel_size: float = None
    registration_type: str = "GeneralizedIcp"
    gicp_epsilon: float = 1e-3
    max_icp_iterations: int = 30
    feature_keypoints: object = None   # cloud_ops.iss_params: match at ISS keypoints only (None = off: every sparse point)


# ---- host policy ---------------------------------------------------------------------------------------------------------------

def to_rpy(T) -> np.ndarray:
    """toRPY(Eigen::Quaterniond(T.rotation())) (math.hpp:30-42), the restatement of o3s_motion_from_poses (csrc/undistort_dev.h):
    Eigen's matrix-to-quaternion branches, then roll, pitch, yaw."""
    R = np.asarray(T, np.float64)[:3, :3]
    q = [0.0, 0.0, 0.0, 0.0]   # w, x, y, z
    tr = (R[0, 0] + R[1, 1]) + R[2, 2]
    if tr > 0.0:
        u = math.sqrt(tr + 1.0)
        q[0] = 0.5 * u
        u = 0.5 / u
        q[1], q[2], q[3] = (R[2, 1] - R[1, 2]) * u, (R[0, 2] - R[2, 0]) * u, (R[1, 0] - R[0, 1]) * u
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        u = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[1 + i] = 0.5 * u
        u = 0.5 / u
        q[0] = (R[k, j] - R[j, k]) * u
        q[1 + j] = (R[j, i] + R[i, j]) * u
        q[1 + k] = (R[k, i] + R[i, k]) * u
    w, x, y, z = (float(v) for v in q)
    with np.errstate(invalid="ignore"):   # (a matrix that is no rotation can leave asin's domain: NaN, as in the reference)
        pitch = float(np.arcsin(2 * (w * y - x * z)))
    return np.array([math.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y)), pitch, math.atan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))])


def is_registration_consistent(T, check: ConsistencyCheckParameters = None) -> bool:
    """PlaceRecognition::isRegistrationConsistent (:182-229): every |roll|, |pitch|, |yaw|, |x|, |y|, |z| of T within its limit
    (a value equal to its limit passes: the reference rejects on `>`)."""
    p = check or ConsistencyCheckParameters()
    T = np.asarray(T, np.float64)
    roll, pitch, yaw = to_rpy(T)
    return not (abs(roll) > p.max_drift_roll or abs(pitch) > p.max_drift_pitch or abs(yaw) > p.max_drift_yaw or
                abs(T[0, 3]) > p.max_drift_x or abs(T[1, 3]) > p.max_drift_y or abs(T[2, 3]) > p.max_drift_z)


def get_loop_closure_candidates_idxs(collection, last_finished_submap_idx: int, active_submap_idx: int,
                                     params: PlaceRecognitionParameters = None) -> list:
    """PlaceRecognition::getLoopClosureCandidatesIdxs (:231-285) over a submap_collection.SubmapCollection, in index order.  Skipped:
    the active submap; a submap adjacent to the ACTIVE one; a submap whose centre is farther than the search radius from the
    FINISHED submap's centre; and every submap while fewer than min_submaps_between_loop_closures submaps lie between the finished
    submap and the nearest loop-closure submap."""
    p = params or PlaceRecognitionParameters()
    idxs = []
    c0 = collection.centre(last_finished_submap_idx)
    for i in range(len(collection.maps)):
        if i == active_submap_idx:
            continue
        if collection.adjacent(collection.ids[i], collection.ids[active_submap_idx]):
            continue
        if collection.dist(c0, collection.centre(i)) > p.loop_closure_search_radius:
            continue
        if collection.getDistanceToNearestLoopClosureSubmap(last_finished_submap_idx) < p.min_submaps_between_loop_closures:
            continue
        idxs.append(i)
    return idxs


@dataclass
class LoopClosureCandidate:
    """What became of one candidate: `rejected` is None for an accepted pair (its Constraint is in the returned list), else the
    reason, worded as registration.LoopClosureConstraint.rejected words it."""
    target_submap_idx: int
    rejected: str = None
    ransac: reg.RansacResult = None
    refinement: reg.RegistrationResult = None
    n_overlap: tuple = None


REJECTED_RANSAC_INCONSISTENT = "ransac: inconsistent registration"
REJECTED_ICP_INCONSISTENT = "refinement: inconsistent registration"


class PlaceRecognition:
    """o3d_slam::PlaceRecognition over resident submaps.  ransac_fn(source, targets, ransac_params, mutual_filter) -> list of
    RansacResult and refine_fn(pairs, params) -> list of (RegistrationResult | None, information | None, n_overlap, status) stand
    in for the device calls in the CPU tests of the orchestration; the defaults are the real thing."""

    def __init__(self, params: PlaceRecognitionParameters = None, ransac_fn=None, refine_fn=None):
        self.params = params or PlaceRecognitionParameters()
        self._ransac = ransac_fn or submaps_registration_ransac
        self._refine = refine_fn or self._refine_on_device
        self.last_candidates = []    # LoopClosureCandidate of every candidate of the last call, in candidate order

    @staticmethod
    def _refine_on_device(pairs, p):
        if p.overlap_voxel_size is None:
            raise ValueError("PlaceRecognitionParameters.overlap_voxel_size is required (voxelExpansionFactorOverlapComputation x map voxel size)")
        return reg.registration_icp_submaps_overlap_batch(pairs, p.max_icp_correspondence_distance, p.overlap_voxel_size, 1,
                                                          max_iteration=p.max_icp_iterations, registration_type=p.registration_type,
                                                          gicp_epsilon=p.gicp_epsilon)

    def isRegistrationConsistent(self, T) -> bool:
        return is_registration_consistent(T, self.params.consistency_check)

    def computeFeatures(self, collection, finished, params=None):
        """collection.computeFeatures(finished, params) with this object's feature_keypoints: the one place where the keypoint
        selection is switched on for everything buildLoopClosureConstraints later searches."""
        return collection.computeFeatures(finished, params, keypoints=self.params.feature_keypoints)

    def getLoopClosureCandidatesIdxs(self, mapToRangeSensor, collection, lastFinishedSubmapIdx, activeSubmapIdx):
        # (mapToRangeSensor is not used by the reference either: its distance test was commented out, :259)
        return get_loop_closure_candidates_idxs(collection, lastFinishedSubmapIdx, activeSubmapIdx, self.params)

    def buildLoopClosureConstraints(self, mapToRangeSensor, collection, lastFinishedSubmapIdx, activeSubmapIdx, timestamp):
        """PlaceRecognition::buildLoopClosureConstraints: the Constraints of the accepted candidates, in candidate order;
        self.last_candidates tells what became of each candidate.  The candidates go through the RANSAC in groups of up to 16
        (one one-to-many call each); the survivors of the correspondence-count gate and of the consistency gate on the RANSAC
        pose go through ONE batched refinement call (up to four pairs in flight in it), then the fitness gate and the
        consistency gate on the refined pose.  A submap that is not a candidate is never touched."""
        p = self.params
        cand = self.getLoopClosureCandidatesIdxs(mapToRangeSensor, collection, lastFinishedSubmapIdx, activeSubmapIdx)
        self.last_candidates = out = [LoopClosureCandidate(i) for i in cand]
        if not cand:
            return []
        source = collection.maps[lastFinishedSubmapIdx]
        for g0 in range(0, len(cand), MAX_TARGETS):
            group = cand[g0:g0 + MAX_TARGETS]
            rrs = self._ransac(source, [collection.maps[i] for i in group], p.ransac, p.mutual_filter)
            for c, rr in zip(out[g0:g0 + len(group)], rrs):
                c.ransac = rr
        survivors = []
        for c in out:
            n = len(c.ransac.correspondence_set)
            if n < p.ransac_min_correspondence_set_size:
                c.rejected = f"ransac: {n} correspondences"
            elif not self.isRegistrationConsistent(c.ransac.transformation):
                c.rejected = REJECTED_RANSAC_INCONSISTENT
            else:
                survivors.append(c)
        constraints = []
        if survivors:
            refined = self._refine([(source, collection.maps[c.target_submap_idx], c.ransac.transformation) for c in survivors], p)
            for c, (res, info, n_ov, status) in zip(survivors, refined):
                c.refinement, c.n_overlap = res, n_ov
                if res is None:
                    if status not in (_lib.OK, _lib.ERR_EMPTY_REFERENCE):
                        raise RuntimeError(f"loop-closure refinement of submap {lastFinishedSubmapIdx} with {c.target_submap_idx} failed with o3s_status {status}")
                    c.rejected = "refinement: empty overlap"
                elif res.fitness < p.min_refinement_fitness:
                    c.rejected = f"refinement score: {res.fitness}"
                elif not self.isRegistrationConsistent(res.transformation):
                    c.rejected = REJECTED_ICP_INCONSISTENT
                else:
                    constraints.append(Constraint(np.array(res.transformation, np.float64), lastFinishedSubmapIdx, c.target_submap_idx,
                                                  np.array(info, np.float64), True, False, timestamp))
        return constraints
