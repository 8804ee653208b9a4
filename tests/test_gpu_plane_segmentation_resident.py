"""RANSAC plane segmentation on resident clouds (o3s_submap_segment_planes, o3s_submap_remove_planes, o3s_scan_remove_planes) against
the host-array entry (o3s_segment_planes, itself held to tests/plane_ref.py by test_gpu_plane_segmentation.py).  MI355X only.

Submap: the labels, models and counts are the host entry's on the downloaded cloud, with a pending insert settled first, and
segmenting moves no byte of the map; after removePlanes the map is, bit for bit and in order, the downloaded cloud without the
labelled points — normals and colours following — and the next insert gives the bits of a submap uploaded from that cloud.  Scan:
the merge cloud loses the labelled points, the match cloud is the crop of what is left; num_iterations 0 leaves both alone.  A second
call of the same size leaves the work area's size where it was."""
import ctypes as C

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan, Submap
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from test_gpu_outlier_removal_resident import VOXEL, cropper, same, trajectory

pytestmark = pytest.mark.gpu

THR, MAX_PLANES, MIN_INLIERS = 0.08, 3, 150
KW = dict(ransac_n=3, num_iterations=120, confidence=1.0, seed=5)
Q = co.plane_params(THR, max_planes=MAX_PLANES, min_inliers=MIN_INLIERS, **KW)


def host_planes(p):
    return co.segment_planes(p, THR, MAX_PLANES, min_inliers=MIN_INLIERS, **KW)


def test_submap_labels_equal_the_host_entry_and_the_map_stays():
    traj = trajectory(n_scans=2)
    a = Submap(VOXEL, cropper())
    for sp, sn, T in traj:
        a.insertScan(sp, sn, T)
    p0, n0 = a.getMapPointCloud()
    lab_h, models_h, counts_h = host_planes(p0)
    assert 1 <= len(counts_h) <= MAX_PLANES and counts_h[0] >= MIN_INLIERS and (lab_h == -1).any()
    lab, models, counts = a.segmentPlanes(Q)
    assert lab.dtype == np.int32 and same(lab, lab_h) and same(models, models_h) and same(counts, counts_h)
    p1, n1 = a.getMapPointCloud()
    assert same(p1, p0) and same(n1, n0) and len(a) == len(p0)
    with pytest.raises(RuntimeError):
        a.segmentPlanes(co.plane_params(0.0, 3, 100, 1.0, 0, 1, 3))
    e = Submap(VOXEL, cropper())   # an empty map
    lab, models, counts = e.segmentPlanes(Q)
    assert len(lab) == 0 and len(counts) == 0 and models.shape == (0, 4)
    removed, models = e.removePlanes(Q)
    assert removed == 0 and len(models) == 0
    removed, models = a.removePlanes(co.plane_params())   # off
    assert removed == 0 and len(models) == 0 and len(a) == len(p0)


def test_submap_removal_equals_the_host_labels_and_the_next_insert_works():
    traj = trajectory()
    a = Submap(VOXEL, cropper())
    for sp, sn, T in traj[:3]:
        a.insertScan(sp, sn, T)
    p0, n0 = a.getMapPointCloud()
    lab_h, models_h, _ = host_planes(p0)
    keep = lab_h < 0
    assert 0 < keep.sum() < len(p0)
    co.plane_release()
    removed, models = a.removePlanes(Q)
    held = co.plane_device_bytes()
    assert removed == len(p0) - keep.sum() and len(a) == keep.sum() and same(models, models_h)
    gp, gn = a.getMapPointCloud()
    assert same(gp, p0[keep]) and same(gn, n0[keep])
    # a submap uploaded from the cleaned cloud; then the same insert on both
    b = Submap(VOXEL, cropper())
    b.setMapPointCloud(p0[keep], n0[keep])
    sp, sn, T = traj[3]
    a.insertScan(sp, sn, T)
    b.insertScan(sp, sn, T)
    (pa, na), (pb, nb) = a.getMapPointCloud(), b.getMapPointCloud()
    assert len(pa) > keep.sum() and same(pa, pb) and same(na, nb)
    # a second removal, on the grown map: still the host labels — and the host entry has sized the work area for this cloud, so
    # the resident calls of the same size allocate nothing
    lab1, _, _ = host_planes(pa)
    held_host = co.plane_device_bytes()
    a.removePlanes(Q)
    gp, gn = a.getMapPointCloud()
    assert same(gp, pa[lab1 < 0]) and same(gn, na[lab1 < 0])
    assert held > 0 and co.plane_device_bytes() == held_host > 0
    b.removePlanes(Q)
    assert co.plane_device_bytes() == held_host and same(b.getMapPointCloud()[0], gp)
    with pytest.raises(RuntimeError):
        a.removePlanes(co.plane_params(THR, 2, 100, 1.0, 0, 1, 3))


def test_submap_removal_carries_colours():
    traj = trajectory(n_scans=2)
    a = Submap(VOXEL, cropper())
    for k, (sp, sn, T) in enumerate(traj):
        col = np.stack([np.linspace(0.0, 1.0, len(sp)), np.full(len(sp), 0.25 * (k + 1)), (np.arange(len(sp)) % 7) / 7.0], axis=1)
        a.insertScanColored(sp, sn, col, T)
    assert a.hasColors()
    p0, n0 = a.getMapPointCloud()
    c0 = a.getMapColors()
    keep = host_planes(p0)[0] < 0
    assert 0 < keep.sum() < len(p0)
    a.removePlanes(Q)
    gp, gn = a.getMapPointCloud()
    assert same(gp, p0[keep]) and same(gn, n0[keep]) and same(a.getMapColors(), c0[keep])


def test_a_pending_insert_is_settled_first():
    """o3s_submap_insert_processed leaves the merge insert enqueued; segmentation and removal work on the map AFTER it"""
    wide, narrow = co.croppingVolumeFactory("MaxRadius", 10.0), co.croppingVolumeFactory("MaxRadius", 8.0)
    traj = trajectory(n_scans=3)
    ps = ProcessedScan()
    for call in ("segment", "remove"):
        a, b = Submap(0.1, wide), Submap(0.1, wide)
        pending = []
        for sp, sn, T in traj:
            ps.preprocess(wide, 0.1, narrow, sp, sn)
            mp_, mn_ = ps.merge
            a.insertProcessed(ps, T)
            lo, hi = a.size_bounds()                            # never waits
            pending.append(hi > lo)
            b.insertScan(mp_, mn_, T)                           # the insert that waits
        assert pending[-1], pending                             # the last insert was still pending when the call was issued
        mp, mn = b.getMapPointCloud()
        lab_h, models_h, counts_h = host_planes(mp)
        if call == "segment":
            fn = a._lib.o3s_submap_segment_planes               # straight through the ABI: Submap.segmentPlanes asks for the size first
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
            lab = np.full(len(mp), -7, np.int32)
            models, counts = np.zeros((16, 4)), np.zeros(16, np.int64)
            k = C.c_int32()
            assert fn(a._h, C.byref(Q), lab.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k), models.ctypes.data_as(C.POINTER(C.c_double)),
                      counts.ctypes.data_as(C.POINTER(C.c_int64))) == 0
            assert k.value == len(counts_h) >= 1 and same(lab, lab_h) and same(models[:k.value], models_h) and same(counts[:k.value], counts_h)
        else:
            removed, models = a.removePlanes(Q)
            assert removed == (lab_h >= 0).sum() > 0 and same(models, models_h)
            gp, gn = a.getMapPointCloud()
            assert same(gp, mp[lab_h < 0]) and same(gn, mn[lab_h < 0])


def test_scan_removal_equals_crop_of_the_filtered_merge_cloud():
    sp, sn, T = trajectory(n_scans=1, n_pts=20000, strays=60)[0]
    wide, narrow = co.croppingVolumeFactory("MaxRadius", 11.0), co.croppingVolumeFactory("MaxRadius", 6.0)
    sc = ProcessedScan()
    sc.preprocess(wide, VOXEL, narrow, sp, sn)
    mp, mn = sc.merge
    xp, xn = sc.match
    # num_iterations 0: nothing moves
    n_merge, n_match, models = sc.removePlanes(narrow, co.plane_params())
    assert (n_merge, n_match) == (len(mp), len(xp)) and len(models) == 0
    assert same(sc.merge[0], mp) and same(sc.merge[1], mn) and same(sc.match[0], xp) and same(sc.match[1], xn)
    lab_h, models_h, _ = host_planes(mp)
    keep = lab_h < 0
    op, on = mp[keep], mn[keep]
    cp, cn = co.crop(narrow, op, on)
    assert 0 < len(op) < len(mp) and 0 < len(cp) <= len(xp)
    n_merge, n_match, models = sc.removePlanes(narrow, Q)
    assert (n_merge, n_match) == (len(op), len(cp)) and same(models, models_h)
    assert same(sc.merge[0], op) and same(sc.merge[1], on)
    assert same(sc.match[0], cp) and same(sc.match[1], cn)
    # the cleaned merge cloud is what an insert takes
    m1, m2 = Submap(VOXEL, cropper()), Submap(VOXEL, cropper())
    m1.insertProcessed(sc, T)
    sc2 = ProcessedScan()
    sc2.preprocess(wide, 0.0, narrow, op, on)   # voxel size 0: the cloud as it is
    m2.insertProcessed(sc2, T)
    (pa, na), (pb, nb) = m1.getMapPointCloud(), m2.getMapPointCloud()
    assert same(pa, pb) and same(na, nb)
    with pytest.raises(RuntimeError):
        sc.removePlanes(narrow, co.plane_params(float("nan"), 3, 100, 1.0, 0, 1, 3))
