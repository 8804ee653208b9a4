"""The numpy restatement of FPFH and of the feature correspondences (tests/fpfh_ref.py) pinned by analysis, not by itself (CPU
only): inputs whose features are known in closed form, hand-computed pairs through every branch, and the invariants the
definition implies.  The GPU tests (tests/test_gpu_fpfh.py, tests/test_gpu_features.py) lean on this module."""
import math

import numpy as np

import fpfh_ref as fr
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn


def small_cloud():
    p, n, _ = fr.sparse_cloud(area=600.0, n_map=50000)
    return p, n


def test_plane_patch_has_all_mass_in_the_middle_bins():
    """z = 0, all normals (0, 0, 1): every pair has f0 = f1 = f2 = 0 exactly and no swap."""
    rng = np.random.default_rng(5)
    p = np.c_[rng.uniform(0.0, 12.0, (800, 2)), np.zeros(800)]
    n = np.tile([0.0, 0.0, 1.0], (800, 1))
    r = fr.compute_fpfh(p, n, 2.5, 100)
    ln = (r.nn >= 0).sum(axis=1)
    assert (ln > 1).all() and ln.max() == 100 and ln.min() < 100     # the cap is active for some queries only
    assert not r.sensitive.any()
    mid = np.zeros(33, bool)
    mid[[5, 16, 27]] = True
    assert np.abs(r.spfh[:, mid] - 100.0).max() <= 1e-9 and np.abs(r.fpfh[:, mid] - 200.0).max() <= 1e-9
    assert (r.spfh[:, ~mid] == 0.0).all() and (r.fpfh[:, ~mid] == 0.0).all()


def test_hand_computed_pairs_and_three_point_cloud():
    z, y = [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]
    o, b = [0.0, 0.0, 0.0], [0.0, 3.0, 4.0]
    f, close = fr.pair_features(o, z, b, y)                        # a1 = 0.8, a2 = 0.6: no swap
    assert np.array_equal(f, [math.atan2(1.0, 0.0), 0.0, 0.8, 5.0]) and not close
    f, _ = fr.pair_features(o, y, b, z)                            # a1 = 0.6, a2 = 0.8: roles swapped, dp negated
    assert np.array_equal(f, [math.atan2(-1.0, 0.0), 0.0, -0.8, 5.0])
    f, _ = fr.pair_features(o, z, o, y)                            # f3 == 0
    assert np.array_equal(f, [0.0, 0.0, 0.0, 0.0])
    f, _ = fr.pair_features(o, z, [1.0, 0.0, 0.0], [1.0, 0.0, 0.0])  # swap, then dp parallel to n1': |v| == 0
    assert np.array_equal(f, [0.0, 0.0, 0.0, 0.0])
    # A = origin (0, 0, 1), B = (0, 3, 4) (0, 1, 0), C = a duplicate of A: lists by (d2, index)
    p = np.array([o, b, o])
    n = np.array([z, y, z])
    r = fr.compute_fpfh(p, n, 10.0, 3)
    assert np.array_equal(r.nn, [[0, 2, 1], [1, 0, 2], [0, 2, 1]]) and np.array_equal(r.d2, [[0, 0, 25], [0, 25, 25], [0, 0, 25]])
    sa = np.zeros(33)
    sa[[5, 27]] = 50.0         # the duplicate: f = 0 -> the middle bins
    sa[[8, 31]] = 50.0         # B: f0 = pi / 2 -> floor(8.25), f2 = 0.8 -> floor(9.9)
    sa[16] = 100.0             # f1 = 0 for both
    sb = np.zeros(33)
    sb[[8, 16, 31]] = 100.0    # B sees A and C alike (swap branch, same feature as A -> B)
    assert np.array_equal(r.spfh, [sa, sb, sa])
    fa = sa.copy()
    fa[[8, 16, 31]] += 100.0   # the duplicate is skipped (d == 0); B weighs 1 / 25: val 4 per group, 100 / 4 = 25
    assert np.array_equal(r.fpfh[0], fa) and np.array_equal(r.fpfh[2], fa)
    assert np.allclose(r.fpfh.reshape(3, 3, 11).sum(axis=2), 200.0, atol=1e-9)


def test_every_group_sums_to_100_and_200():
    p, n = small_cloud()
    r = fr.compute_fpfh(p, n, 2.5, 100)
    ok = (r.nn >= 0).sum(axis=1) > 1
    assert ok.sum() > 1000
    assert np.abs(r.spfh[ok].reshape(-1, 3, 11).sum(axis=2) - 100.0).max() <= 1e-9
    assert np.abs(r.fpfh[ok].reshape(-1, 3, 11).sum(axis=2) - 200.0).max() <= 1e-9
    assert (r.spfh[~ok] == 0.0).all() and (r.fpfh[~ok] == 0.0).all()
    assert r.sensitive.mean() <= 0.01


def test_rigid_motion_leaves_the_features_alone():
    p, n = small_cloud()
    r = fr.compute_fpfh(p, n, 2.5, 100)
    R = syn.rot_axis_angle([0.3, -0.5, 0.8], 0.7)
    q = p @ R.T + np.array([4.0, -7.0, 2.5])
    m = n @ R.T
    s = fr.compute_fpfh(q, m, 2.5, 100, nn=r.nn)      # same lists: the feature arithmetic is what is under test
    keep = ~(r.tainted | s.tainted)
    assert keep.mean() >= 0.75
    assert np.abs(r.fpfh[keep] - s.fpfh[keep]).max() <= 1e-9


def test_mutual_filter_and_fallback():
    e = np.eye(33)
    src = np.stack([e[0], e[1], e[2], e[3], 0.9 * e[3] + 0.1 * e[4]])
    tgt = np.stack([e[1], e[0], e[3], e[2] * 1.5, e[20]])
    # ij = [1, 0, 3, 2, 2]; ji = [1, 0, 3, 2, ...]: source 4 points at target 2, which prefers source 3
    pairs, fb, flagged = fr.feature_correspondences(src, tgt, True, 1)
    assert not fb and np.array_equal(pairs, [[0, 1], [1, 0], [2, 3], [3, 2]]) and not flagged.any()
    pairs, fb, _ = fr.feature_correspondences(src, tgt, True, 3)          # 4 < 9 mutual pairs: every (i, ij[i])
    assert fb and np.array_equal(pairs, [[0, 1], [1, 0], [2, 3], [3, 2], [4, 2]])
    pairs, fb, _ = fr.feature_correspondences(src, tgt, False, 3)
    assert not fb and np.array_equal(pairs, [[0, 1], [1, 0], [2, 3], [3, 2], [4, 2]])
    # ties go to the lower index, and are flagged
    pairs, _, flagged = fr.feature_correspondences(np.stack([e[0]]), np.stack([e[5], e[6], e[0] * 3.0]), False, 3)
    assert np.array_equal(pairs, [[0, 0]]) and flagged.all()


def test_feature_entry_points_are_declared_and_exported():
    """The C ABI of the feature front end: declared in include/ and exported by the product library (argument checks need no GPU)."""
    import ctypes as C
    import os
    import re

    from open3d_slam_advanced_rss_2024_public_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "o3s_cloud_ops.h")).read() + open(os.path.join(root, "include", "o3s_submap.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.lib()
    for s in ("o3s_compute_fpfh", "o3s_feature_correspondences", "o3s_submap_feature_params_default", "o3s_submap_compute_features",
              "o3s_submap_features_size", "o3s_submap_download_features", "o3s_submap_feature_correspondences"):
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(L, s), s
    from open3d_slam_advanced_rss_2024_public_amd import submap as sm

    sm._L()
    prm = sm.FeatureParamsC()
    L.o3s_submap_feature_params_default(C.byref(prm))
    assert (prm.feature_voxel_size, prm.normal_radius, prm.normal_knn, prm.feature_radius, prm.feature_knn) == (0.5, 2.0, 20, 2.5, 100)
    assert L.o3s_submap_compute_features(None, C.byref(prm)) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_submap_features_size(None) == -1
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

    co._L()
    assert L.o3s_compute_fpfh(0, None, None, 5, 2.5, 129, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_compute_fpfh(0, None, None, 5, 2.5, 0, None, None, None) == _lib.ERR_BAD_ARGUMENT
    assert L.o3s_compute_fpfh(0, None, None, 0, 2.5, 100, None, None, None) == _lib.OK      # nothing to do
