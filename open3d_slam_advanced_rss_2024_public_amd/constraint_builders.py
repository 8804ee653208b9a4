"""The odometry constraints between a submap and its parent: O3S/src/constraint_builders.cpp restated over a collection of
device-resident submaps, and the device call behind it (include/constraints/o3s_constraints.h).  Python mirror of
cpp/o3s_constraint_builders.hpp: the same logic, the compiled header is checked against it.

With the refinement off — every parameter file of the reference sets isRefineOdometryConstraintsBetweenSubmaps = false — a
constraint is the overlap selection and Open3D's information matrix at the identity, and all the pairs one invocation has to
build go into ONE o3s_submaps_odometry_constraints call.  With it on, each pair runs the existing loop-closure refinement
(registration.registration_icp_submaps_overlap, point-to-plane, 100 iterations), which needs target normals as the reference does.

Kept where it looks odd:
  * a pair whose overlap is empty STILL yields its constraint, with the zero information matrix: the reference emits it (Open3D's
    matrix over no correspondences is zero), and hasConstraint — so every later invocation — depends on it being there;
  * build_constraint sets is_odometry_constraint itself and build_odometry_constraint sets it again (:40, :77);
  * the candidates overload reads the active submap's id and does not use it (:94)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .pose_graph import Constraint

# magic.hpp:12-15
VOXEL_SIZE_CORRESPONDENCE_SEARCH_IF_MAP_VOXEL_SIZE_IS_ZERO = 0.04
ICP_RUN_UNTIL_CONVERGENCE_NUMBER_OF_ITERATIONS = 100
VOXEL_EXPANSION_FACTOR_OVERLAP_COMPUTATION = 20.0
VOXEL_EXPANSION_FACTOR_ICP_CORRESPONDENCE_DISTANCE = 1.5


def get_map_voxel_size(map_voxel_size: float, value_if_zero: float) -> float:
    """getMapVoxelSize (helpers.cpp:356-358)"""
    return value_if_zero if abs(map_voxel_size) <= 1e-3 else map_voxel_size


def _L():
    L = _lib.lib()
    if _lib.needs_binding(L, __name__):
        dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        L.o3s_submaps_odometry_constraints.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), dp, C.c_double, C.c_int64, C.c_double,
                                                       dp, lp, lp, C.POINTER(C.c_int32)]
    return L


def submaps_odometry_constraints(pairs, overlap_voxel_size, max_correspondence_distance, min_num_points_per_voxel: int = 1, Ts=None):
    """o3s_submaps_odometry_constraints for a list of (source Submap, target Submap): one device call.  Ts: one 4x4 per pair, or
    None for the identity everywhere.  Returns a list of (information 6x6, (n_source_overlap, n_target_overlap), n_correspondences,
    o3s_status): O3S_ERR_EMPTY_REFERENCE (zero matrix) for an empty submap or overlap, O3S_ERR_BAD_ARGUMENT for a pair with a
    non-finite point.  Raises ValueError when the library refuses the call's arguments."""
    n = len(pairs)
    src = (C.c_void_p * max(n, 1))(*[s._h.value for s, _ in pairs])
    tgt = (C.c_void_p * max(n, 1))(*[t._h.value for _, t in pairs])
    T = None
    if Ts is not None:
        T = np.ascontiguousarray(np.stack([np.asarray(M, np.float64).T.reshape(16) for M in Ts]) if n else np.zeros((1, 16)))
    infos = np.zeros((max(n, 1), 36))
    n_ov = np.zeros((max(n, 1), 2), np.int64)
    n_co = np.zeros(max(n, 1), np.int64)
    st = np.full(max(n, 1), -1, np.int32)
    dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    rc = _L().o3s_submaps_odometry_constraints(n, src, tgt, None if T is None else T.ctypes.data_as(dp), float(overlap_voxel_size),
                                               int(min_num_points_per_voxel), float(max_correspondence_distance), infos.ctypes.data_as(dp),
                                               n_ov.ctypes.data_as(lp), n_co.ctypes.data_as(lp), st.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError("o3s_submaps_odometry_constraints refused its arguments")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_submaps_odometry_constraints failed with o3s_status {rc}")
    return [(infos[k].reshape(6, 6).T.copy(), (int(n_ov[k, 0]), int(n_ov[k, 1])), int(n_co[k]), int(st[k])) for k in range(n)]


def _refine(source, target, max_correspondence_distance, overlap_voxel_size, min_num_points_per_voxel, max_iteration):
    from .registration import registration_icp_submaps_overlap

    return registration_icp_submaps_overlap(source, target, max_correspondence_distance, np.eye(4), overlap_voxel_size, min_num_points_per_voxel,
                                            max_iteration=max_iteration, with_information=True, registration_type="PointToPlaneIcp")


def has_constraint(source_idx: int, target_idx: int, constraints) -> bool:
    """:23-30"""
    return any(c.source_submap_idx == source_idx and c.target_submap_idx == target_idx for c in constraints)


def build_constraints(pairs, collection, is_compute_overlap, icp_max_correspondence_distance, voxel_size_overlap_compute,
                      is_estimate_information_matrix, is_skip_icp_refinement, device_call=None, refine_call=None):
    """buildConstraint (:43-90) for a list of (source_idx, target_idx): one device call for all of them when the refinement is
    skipped.  The reference's only caller passes is_compute_overlap = is_estimate_information_matrix = True; nothing else is built.
    device_call / refine_call: stand-ins for submaps_odometry_constraints / the refinement (the CPU tests of the rules)."""
    if not is_compute_overlap or not is_estimate_information_matrix:
        raise ValueError("build_constraint: only the overlap-selected constraint with an information matrix is built (its one caller's form)")
    pairs = [(int(s), int(t)) for s, t in pairs]
    if not pairs:
        return []
    maps = [(collection.maps[s], collection.maps[t]) for s, t in pairs]
    min_num_points_per_voxel = 1
    out = []
    if is_skip_icp_refinement:
        call = device_call or submaps_odometry_constraints
        res = call(maps, voxel_size_overlap_compute, icp_max_correspondence_distance, min_num_points_per_voxel)
        for (s, t), (info, _, _, status) in zip(pairs, res):
            if status not in (_lib.OK, _lib.ERR_EMPTY_REFERENCE):
                raise RuntimeError(f"odometry constraint {s} -> {t}: o3s_status {status}")
            out.append(Constraint(np.eye(4), s, t, np.array(info, np.float64), True, True))
        return out
    call = refine_call or _refine
    for (s, t), (src, tgt) in zip(pairs, maps):
        r, info, _ = call(src, tgt, icp_max_correspondence_distance, voxel_size_overlap_compute, min_num_points_per_voxel,
                          ICP_RUN_UNTIL_CONVERGENCE_NUMBER_OF_ITERATIONS)
        T = np.eye(4) if r is None else np.array(r.transformation, np.float64)
        out.append(Constraint(T, s, t, np.zeros((6, 6)) if info is None else np.array(info, np.float64), True, True))
    return out


def build_constraint(source_idx, target_idx, collection, is_compute_overlap, icp_max_correspondence_distance, voxel_size_overlap_compute,
                     is_estimate_information_matrix, is_skip_icp_refinement, device_call=None, refine_call=None) -> Constraint:
    """buildConstraint (:43-90)"""
    return build_constraints([(source_idx, target_idx)], collection, is_compute_overlap, icp_max_correspondence_distance, voxel_size_overlap_compute,
                             is_estimate_information_matrix, is_skip_icp_refinement, device_call, refine_call)[0]


def build_odometry_constraints(pairs, collection, device_call=None, refine_call=None):
    """buildOdometryConstraint (:33-41) for a list of (source_idx, target_idx)"""
    map_voxel_size = get_map_voxel_size(collection.map_voxel, VOXEL_SIZE_CORRESPONDENCE_SEARCH_IF_MAP_VOXEL_SIZE_IS_ZERO)
    cs = build_constraints(pairs, collection, True, VOXEL_EXPANSION_FACTOR_ICP_CORRESPONDENCE_DISTANCE * map_voxel_size,
                           VOXEL_EXPANSION_FACTOR_OVERLAP_COMPUTATION * map_voxel_size, True,
                           not getattr(collection, "refine_odometry_constraints", False), device_call, refine_call)
    for c in cs:
        c.is_odometry_constraint = True
    return cs


def build_odometry_constraint(source_idx, target_idx, collection, device_call=None, refine_call=None) -> Constraint:
    """buildOdometryConstraint (:33-41)"""
    return build_odometry_constraints([(source_idx, target_idx)], collection, device_call, refine_call)[0]


def _append_missing(pairs, collection, constraints, device_call, refine_call):
    # hasConstraint against the list as it grows: a pair named twice in one invocation is built once
    todo = []
    for p in pairs:
        if not has_constraint(p[0], p[1], constraints) and p not in todo:
            todo.append(p)
    constraints.extend(build_odometry_constraints(todo, collection, device_call, refine_call))


def compute_odometry_constraints(collection, constraints, candidates=None, device_call=None, refine_call=None):
    """Both overloads of computeOdometryConstraints (:92-118); `constraints` is extended in place.
    candidates given — (submap id, time stamp) of finished submaps (:92-105): ids below 1 are skipped, the pair is
    (parent(target), target).  candidates None — every submap from 1 on (:107-118), also skipping the pairs whose source or target
    is the active submap."""
    pairs = []
    if candidates is not None:
        for cand in candidates:
            target = int(cand[0])
            if target < 1:
                continue
            pairs.append((int(collection.parents[target]), target))
    else:
        active = collection.ids[collection.active]
        for target in range(1, len(collection.maps)):
            source = int(collection.parents[target])
            if source != active and target != active:
                pairs.append((source, target))
    _append_missing(pairs, collection, constraints, device_call, refine_call)
    return constraints
