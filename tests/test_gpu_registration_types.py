"""Generalized ICP and point-to-point ICP (o3s_o3d_registration_icp_ex and the resident _overlap_ex / _overlap_batch_ex refinements)
against the NumPy restatement of Open3D v0.15.1 (tests/o3d_registration_ref.py).  MI355X only.  Iterations, correspondence counts
and fitness are exact; pose, RMSE and the information matrix agree to 1e-9 (fp64 sums in another order; GICP's M^-1 form
against Open3D's W = M^-1.sqrt() form)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import registration as reg
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn

from o3d_registration_ref import covariances_from_normals, registration_icp as ref_icp

pytestmark = pytest.mark.gpu

TYPES = ("PointToPlaneIcp", "PointToPointIcp", "GeneralizedIcp")


def submap_pair(ns=5000, nt=8000, seed=3, noise=0.005):
    """Two overlapping clouds of one world: target in the map frame, source in its sensor frame, both with unit normals."""
    world = syn.make_world(9000.0, seed=seed)
    T = syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.3), np.array([1.0, 2.0, 1.5]))
    tp, tn = syn.make_scan(world, nt, T, radius=12.0, sigma=0.0, seed=seed + 1)
    tgt = tp.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    tgt_n = tn.astype(np.float64) @ T[:3, :3].T
    sp, sn = syn.make_scan(world, ns, T, radius=10.0, sigma=noise, seed=seed + 2)
    return sp.astype(np.float64), sn.astype(np.float64), tgt, tgt_n, T


def same(g, o, tol=1e-9):
    assert g.iterations == o["iterations"] and g.correspondences == o["correspondences"], (g, o["iterations"], o["correspondences"])
    assert g.fitness == o["fitness"]
    assert abs(g.inlier_rmse - o["inlier_rmse"]) <= tol * max(1.0, o["inlier_rmse"])
    assert np.abs(g.transformation - o["transformation"]).max() <= tol


def bits(a, b):
    assert (a.iterations, a.correspondences, a.fitness, a.inlier_rmse) == (b.iterations, b.correspondences, b.fitness, b.inlier_rmse)
    assert np.array_equal(np.asarray(a.transformation), np.asarray(b.transformation))


@pytest.mark.parametrize("cov", ["unit_normals", "voxel_normals", "covariances"])
@pytest.mark.parametrize("max_dist,max_iter", [(1.0, 30), (0.3, 100), (2.0, 3)])
def test_generalized_icp_matches_restatement(max_dist, max_iter, cov):
    src, src_n, tgt, tgt_n, T_gt = submap_pair()
    kw = {}
    if cov == "voxel_normals":  # voxel means of unit normals (VoxelDownSample): not unit, used as they are
        src, src_n, _ = orc.voxel_downsample_o3d(0.25, src, src_n)
        tgt, tgt_n, _ = orc.voxel_downsample_o3d(0.25, tgt, tgt_n)
        assert np.abs(np.linalg.norm(tgt_n, axis=1) - 1.0).max() > 0.05
        kw = dict(source_normals=src_n, target_normals=tgt_n)
    elif cov == "covariances":  # the caller's covariances win over the normals (here: another epsilon than the call's)
        kw = dict(source_covariances=covariances_from_normals(src_n, 0.05), target_covariances=covariances_from_normals(tgt_n, 0.05),
                  source_normals=src_n, target_normals=tgt_n)
    else:
        kw = dict(source_normals=src_n, target_normals=tgt_n)
    init = syn.perturb_pose(T_gt, 0.1, 2.0, seed=5)
    g = reg.registration_generalized_icp(src, tgt, max_dist, init, max_iteration=max_iter, **kw)
    o = ref_icp(src, tgt, max_dist, init, "GeneralizedIcp", max_iteration=max_iter, **kw)
    same(g, o)
    if max_iter >= 30:
        dt, ang = orc.pose_error(T_gt, g.transformation)
        assert np.linalg.norm(dt) < 0.03 and ang < 0.01


@pytest.mark.parametrize("max_dist,max_iter", [(1.0, 30), (0.3, 100), (2.0, 3)])
def test_point_to_point_matches_restatement(max_dist, max_iter):
    src, _, tgt, _, T_gt = submap_pair()
    init = syn.perturb_pose(T_gt, 0.1, 2.0, seed=5)
    g = reg.registration_icp_point_to_point(src, tgt, max_dist, init, max_iteration=max_iter)
    o = ref_icp(src, tgt, max_dist, init, "PointToPointIcp", max_iteration=max_iter)
    same(g, o)


def test_identity_init_and_no_overlap():
    """constraint_builders.cpp passes Identity (Open3D then leaves the cloud and its covariances as they are); a source far from the
    target has no correspondence: identity updates, one iteration, fitness 0."""
    src, src_n, tgt, tgt_n, T_gt = submap_pair(2000, 3000)
    src_map = src @ T_gt[:3, :3].T + T_gt[:3, 3]
    src_map_n = src_n @ T_gt[:3, :3].T
    g = reg.registration_generalized_icp(src_map, tgt, 0.5, source_normals=src_map_n, target_normals=tgt_n)
    same(g, ref_icp(src_map, tgt, 0.5, None, "GeneralizedIcp", source_normals=src_map_n, target_normals=tgt_n))
    p = reg.registration_icp_point_to_point(src_map, tgt, 0.5)
    same(p, ref_icp(src_map, tgt, 0.5, None, "PointToPointIcp"))
    far = src_map + 500.0
    for r in (reg.registration_generalized_icp(far, tgt, 0.5, source_normals=src_map_n, target_normals=tgt_n),
              reg.registration_icp_point_to_point(far, tgt, 0.5)):
        assert r.correspondences == 0 and r.fitness == 0.0 and r.inlier_rmse == 0.0
        assert r.iterations == 1 and np.array_equal(r.transformation, np.eye(4))
    with pytest.raises(RuntimeError, match="normals"):
        reg.registration_generalized_icp(src_map, tgt, 0.5, target_normals=tgt_n)   # no KNN(20) normal estimation here


def test_generalized_icp_is_deterministic():
    src, src_n, tgt, tgt_n, T_gt = submap_pair(6000, 9000, seed=11)
    init = syn.perturb_pose(T_gt, 0.1, 2.0, seed=3)
    a = reg.registration_generalized_icp(src, tgt, 1.0, init, source_normals=src_n, target_normals=tgt_n)
    b = reg.registration_generalized_icp(src, tgt, 1.0, init, source_normals=src_n, target_normals=tgt_n)
    bits(a, b)


def _ex_host(est_type, src, tgt, tgt_n, max_dist, init):
    """o3s_o3d_registration_icp_ex called directly (the Python wrappers route point-to-plane through the old entry point)."""
    L = reg._L()
    s_ = np.ascontiguousarray(src, np.float64)
    t_ = np.ascontiguousarray(tgt, np.float64)
    n_ = np.ascontiguousarray(tgt_n, np.float64)
    cr = reg._Criteria(1e-6, 1e-6, 30)
    r = reg._Result()
    rc = L.o3s_o3d_registration_icp_ex(0, reg._d(s_), None, None, len(s_), reg._d(t_), reg._d(n_), None, len(t_), float(max_dist),
                                       reg._d(reg._pose(init)), C.byref(reg._Estimation(est_type, 1e-3)), C.byref(cr), C.byref(r))
    assert rc == _lib.OK
    return reg._result(r)


def _resident(src, src_n, tgt, tgt_n):
    from open3d_slam_advanced_rss_2024_public_amd import Submap
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

    big = co.croppingVolumeFactory("MaxRadius", 1.0e6)
    a, b = Submap(0.0, big), Submap(0.0, big)
    nudge = syn.make_T(None, np.array([0.25, 0.0, 0.0]))
    a.insertScan(src - np.array([0.25, 0.0, 0.0]), src_n, nudge)
    b.insertScan(tgt - np.array([0.25, 0.0, 0.0]), tgt_n, nudge)
    return a, b


@pytest.mark.parametrize("kind", TYPES)
def test_resident_refinement_equals_host_path(kind):
    """PlaceRecognition.cpp:97-150 with each registration type on two resident submaps = download x 2 + o3s_overlap_indices + the host
    registration on the selections (the source's normals selected with its points) + the information matrix."""
    src, src_n, tgt, tgt_n, T_gt = submap_pair(20000, 30000)
    a, b = _resident(src, src_n, tgt, tgt_n)
    sa, sna = a.getMapPointCloud()
    tb, tnb = b.getMapPointCloud()
    init = syn.make_T(None, np.array([5.0, 0.0, 0.0])) @ syn.perturb_pose(T_gt, 0.1, 2.0, seed=4)   # part of the source misses the target
    res, info, n_ov = reg.registration_icp_submaps_overlap(a, b, 1.0, init, 2.0, registration_type=kind)
    gs, gt = reg.compute_indices_of_overlapping_points(sa, tb, init, 2.0)
    assert n_ov == (len(gs), len(gt)) and 0 < len(gs) < len(sa)
    if kind == "GeneralizedIcp":
        h = reg.registration_generalized_icp(sa[gs], tb[gt], 1.0, init, source_normals=sna[gs], target_normals=tnb[gt])
        o = ref_icp(sa[gs], tb[gt], 1.0, init, kind, source_normals=sna[gs], target_normals=tnb[gt])
    elif kind == "PointToPointIcp":
        h = reg.registration_icp_point_to_point(sa[gs], tb[gt], 1.0, init)
        o = ref_icp(sa[gs], tb[gt], 1.0, init, kind)
    else:
        h = reg.registration_icp(sa[gs], tb[gt], tnb[gt], 1.0, init)
        o = ref_icp(sa[gs], tb[gt], 1.0, init, kind, target_normals=tnb[gt])
    bits(res, h)
    same(res, o)
    oi = orc.o3d_information_matrix(sa[gs], tb[gt], 1.0, res.transformation)
    assert np.abs(info - oi).max() <= 1e-9 * max(1.0, np.abs(oi).max())
    if kind == "PointToPointIcp":  # needs no normals: a target without them is refined too
        from open3d_slam_advanced_rss_2024_public_amd import Submap
        from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

        bare = Submap(0.0, co.croppingVolumeFactory("MaxRadius", 1.0e6))
        bare.insertScan(tgt - np.array([0.25, 0.0, 0.0]), None, syn.make_T(None, np.array([0.25, 0.0, 0.0])))
        r2, i2, n2 = reg.registration_icp_submaps_overlap(a, bare, 1.0, init, 2.0, registration_type=kind)
        assert n2 == n_ov
        bits(r2, res)
        assert np.array_equal(i2, info)


@pytest.mark.parametrize("kind", ["PointToPointIcp", "GeneralizedIcp"])
def test_batch_of_resident_refinements_equals_single_calls(kind):
    pairs, singles = [], []
    for k in range(4):
        src, src_n, tgt, tgt_n, T_gt = submap_pair(8000 + 2000 * k, 12000 + 1000 * k, seed=60 + k)
        a, b = _resident(src, src_n, tgt, tgt_n)
        init = syn.perturb_pose(T_gt, 0.08, 1.5, seed=70 + k)
        pairs.append((a, b, init))
        singles.append(reg.registration_icp_submaps_overlap(a, b, 1.0, init, 2.0, registration_type=kind))
    out = reg.registration_icp_submaps_overlap_batch(pairs, 1.0, 2.0, registration_type=kind)
    for (r, info, nov, st), (rs, infos, novs) in zip(out, singles):
        assert st == 0 and nov == novs
        bits(r, rs)
        assert np.array_equal(info, infos)


def test_point_to_plane_through_every_ex_form_is_bit_identical():
    L = reg._L()
    src, src_n, tgt, tgt_n, T_gt = submap_pair(6000, 9000, seed=13)
    init = syn.perturb_pose(T_gt, 0.1, 2.0, seed=6)
    bits(_ex_host(0, src, tgt, tgt_n, 0.8, init), reg.registration_icp(src, tgt, tgt_n, 0.8, init))
    a, b = _resident(src, src_n, tgt, tgt_n)
    r0, i0, n0 = reg.registration_icp_submaps_overlap(a, b, 1.0, init, 2.0)
    dp = C.POINTER(C.c_double)
    L.o3s_o3d_registration_icp_submaps_overlap_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_double, dp, C.POINTER(reg._Estimation),
                                                              C.POINTER(reg._Criteria), C.c_double, C.c_int64, C.POINTER(reg._Result), dp,
                                                              C.POINTER(C.c_int64)]
    cr = reg._Criteria(1e-6, 1e-6, 30)
    est = reg._Estimation(0, 1e-3)
    r = reg._Result()
    info = np.zeros(36)
    nov = (C.c_int64 * 2)()
    assert L.o3s_o3d_registration_icp_submaps_overlap_ex(a._h, b._h, 1.0, reg._d(reg._pose(init)), C.byref(est), C.byref(cr), 2.0, 1, C.byref(r),
                                                         reg._d(info), nov) == _lib.OK
    bits(reg._result(r), r0)
    assert np.array_equal(info.reshape(6, 6).T, i0) and (nov[0], nov[1]) == n0
    L.o3s_o3d_registration_icp_submaps_overlap_batch_ex.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_double, dp,
                                                                    C.POINTER(reg._Estimation), C.POINTER(reg._Criteria), C.c_double, C.c_int64,
                                                                    C.POINTER(reg._Result), dp, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    srcs = (C.c_void_p * 2)(a._h, a._h)
    tgts = (C.c_void_p * 2)(b._h, b._h)
    inits = np.ascontiguousarray(np.stack([reg._pose(init), reg._pose(init)]))
    res = (reg._Result * 2)()
    infos = np.zeros((2, 36))
    novs = (C.c_int64 * 4)()
    sts = (C.c_int32 * 2)()
    assert L.o3s_o3d_registration_icp_submaps_overlap_batch_ex(2, srcs, tgts, 1.0, reg._d(inits), C.byref(est), C.byref(cr), 2.0, 1, res,
                                                               reg._d(infos), novs, sts) == _lib.OK
    for k in range(2):
        assert sts[k] == 0
        bits(reg._result(res[k]), r0)
        assert np.array_equal(infos[k].reshape(6, 6).T, i0)


def test_generalized_needs_source_normals_on_resident_submaps():
    from open3d_slam_advanced_rss_2024_public_amd import Submap
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

    src, src_n, tgt, tgt_n, T_gt = submap_pair(4000, 6000, seed=19)
    bare = Submap(0.0, co.croppingVolumeFactory("MaxRadius", 1.0e6))
    bare.insertScan(src - np.array([0.25, 0.0, 0.0]), None, syn.make_T(None, np.array([0.25, 0.0, 0.0])))
    _, b = _resident(src, src_n, tgt, tgt_n)
    with pytest.raises(RuntimeError, match="normals"):
        reg.registration_icp_submaps_overlap(bare, b, 1.0, T_gt, 2.0, registration_type="GeneralizedIcp")
