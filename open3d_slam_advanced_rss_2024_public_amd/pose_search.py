"""Initial pose search in a resident map (include/pose_search/o3s_pose_search.h) and the localisation step built on it.

The reference's localisation mode waits for a person: SlamMapInitializer (ros/open3d_slam_ros/src/SlamMapInitializer.cpp:50-130)
loads the map and lets the user drag a marker until the scan lies on it.  `search` scores a grid of candidate poses around a
prior against the submap's occupancy snapshot in one device call; `localize` is host policy over existing entries — every winner
is refined by the scan-to-map chain and judged by its fitness — like PlaceRecognition it adds no C entry of its own."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .cloud_ops import _d
from .submap import ProcessedScan, Submap, _pose

PoseSearchParamsC, PoseSearchResultC = _lib.PoseSearchParamsC, _lib.PoseSearchResultC


def _L():
    return _lib.lib()   # (the argtypes of the pose-search entries are bound where the library is loaded)


@dataclass
class PoseSearchParams:
    """o3s_pose_search_params; the defaults are o3s_pose_search_default_params'."""
    center: np.ndarray = field(default_factory=lambda: np.eye(4))   # prior T_map_sensor (4 x 4)
    step_xy: float = 0.5
    step_z: float = 0.5
    step_yaw: float = math.radians(5.0)
    yaw0: float = 0.0
    n_x: int = 8
    n_y: int = 8
    n_z: int = 0
    n_yaw: int = 72
    yaw_ring: bool = True
    point_stride: int = 1
    local_maxima: bool = True
    top_k: int = 8
    min_score: int = 1

    def to_c(self) -> PoseSearchParamsC:
        c = PoseSearchParamsC()
        c.center[:] = list(_pose(np.asarray(self.center, np.float64).reshape(4, 4)))
        c.step_xy, c.step_z, c.step_yaw, c.yaw0 = float(self.step_xy), float(self.step_z), float(self.step_yaw), float(self.yaw0)
        c.n_x, c.n_y, c.n_z, c.n_yaw = int(self.n_x), int(self.n_y), int(self.n_z), int(self.n_yaw)
        c.yaw_ring, c.point_stride, c.local_maxima = int(self.yaw_ring), int(self.point_stride), int(self.local_maxima)
        c.top_k, c.min_score = int(self.top_k), int(self.min_score)
        return c

    def count(self) -> int:
        """P, the number of poses of the grid; -1 for parameters the search refuses (o3s_pose_search_count)."""
        return int(_L().o3s_pose_search_count(C.byref(self.to_c())))


@dataclass
class PoseSearchResult:
    n_poses: int
    index: np.ndarray            # (n_found,) int64: pose indices of the winners, best first
    score: np.ndarray            # (n_found,) int64
    n_points_counted: int
    gpu_ms: float
    scores: np.ndarray = None    # (P,) uint32 when asked for

    @property
    def n_found(self) -> int:
        return int(self.index.shape[0])


def pose(params: PoseSearchParams, index: int) -> np.ndarray:
    """T_map_sensor of pose `index` of the grid (o3s_pose_search_pose): 4 x 4."""
    T = np.zeros(16)
    rc = _L().o3s_pose_search_pose(C.byref(params.to_c()), int(index), _d(T))
    if rc != _lib.OK:
        raise ValueError("pose: refused parameters, or an index outside the grid")
    return T.reshape(4, 4).T.copy()


def search(submap: Submap, scan_or_points, params: PoseSearchParams, which: int = 1, with_scores: bool = False) -> PoseSearchResult:
    """Scores every pose of the grid against the submap's snapshot (Submap.buildVoxelMap) and returns the winners
    (o3s_submap_pose_search[_scan]).  `scan_or_points`: (N, 3) host points in the sensor frame, or a ProcessedScan whose merge
    (which = 0) or match (1) cloud is read where it is.  ValueError: a refused argument; RuntimeError: no snapshot."""
    L = _L()
    pc = params.to_c()
    res = PoseSearchResultC()
    scores = None
    if with_scores:
        P = int(L.o3s_pose_search_count(C.byref(pc)))
        if P < 0:
            raise ValueError("search: refused parameters")
        scores = np.zeros(P, np.uint32)
    sp = None if scores is None else scores.ctypes.data_as(C.POINTER(C.c_uint32))
    if isinstance(scan_or_points, ProcessedScan):
        rc = L.o3s_submap_pose_search_scan(submap._h, scan_or_points._h, int(which), C.byref(pc), C.byref(res), sp)
    else:
        p = np.ascontiguousarray(scan_or_points, np.float64).reshape(-1, 3)
        rc = L.o3s_submap_pose_search(submap._h, _d(p), p.shape[0], C.byref(pc), C.byref(res), sp)
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError("search: bad argument (parameters out of range, too many poses or points, `which` not 0 / 1, another device)")
    if rc == _lib.ERR_NOT_INITIALIZED:
        raise RuntimeError("search: the submap has no occupancy snapshot (Submap.buildVoxelMap)")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_submap_pose_search failed with o3s_status {rc}")
    n = int(res.n_found)
    return PoseSearchResult(int(res.n_poses), np.array(res.index[:n], np.int64), np.array(res.score[:n], np.int64),
                            int(res.n_points_counted), float(res.gpu_ms), scores)


@dataclass
class LocalizeCandidate:
    index: int
    score: int
    T: np.ndarray = None          # the refined pose (None: the refinement failed)
    fitness: float = float("nan")
    iterations: int = 0
    error: str = None             # what the refinement raised


@dataclass
class LocalizeResult:
    ok: bool
    T: np.ndarray                 # the accepted pose; the best refined candidate's when ok is False and there is one; else None
    fitness: float
    index: int                    # grid index of the kept candidate (-1: none)
    score: int
    candidates: list
    search: PoseSearchResult


def localize(submap: Submap, scan: ProcessedScan, icp, scan_matcher_cropper, params: PoseSearchParams, min_fitness: float,
             max_correspondence_distance: float = 0.0) -> LocalizeResult:
    """The localisation step that replaces the interactive marker: search, then for every winner in order the scan-to-map chain
    from that pose — submap.set_reference(cropper, T_cand, icp), the scan's match cloud as the resident reading,
    icp.compute_resident(T_cand), icp.evaluate() — and the candidate with the highest fitness is kept (the earlier one wins a
    tie) and accepted when its fitness >= min_fitness.  A candidate whose refinement raises is skipped and recorded.  Nothing is
    built here: a submap without a snapshot is the caller's error."""
    found = search(submap, scan, params, which=1)
    cands, best = [], None
    for k in range(found.n_found):
        c = LocalizeCandidate(int(found.index[k]), int(found.score[k]))
        cands.append(c)
        T0 = pose(params, c.index)
        try:
            submap.set_reference(scan_matcher_cropper, T0, icp)
            scan.set_reading(icp)   # (after the reference, as the mapper does on every scan)
            T32 = icp.compute_resident(T0.astype(np.float32))
            c.iterations = int(icp.stats.iterations)
            fit = icp.evaluate(None, max_correspondence_distance)
        except (RuntimeError, ValueError) as e:
            c.error = f"{type(e).__name__}: {e}"
            continue
        c.T = np.asarray(T32, np.float64)
        c.fitness = float(fit.fitness)
        if best is None or c.fitness > best.fitness:
            best = c
    if best is None:
        return LocalizeResult(False, None, float("nan"), -1, 0, cands, found)
    return LocalizeResult(bool(best.fitness >= min_fitness), best.T.copy(), best.fitness, best.index, best.score, cands, found)
