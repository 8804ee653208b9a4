"""The C++ shim's plane segmentation (cpp/o3s_icp.hpp: o3s::segmentPlane, o3s::segmentPlanes, SubmapHip::segmentPlanes and
SubmapHip::removePlanes) as compiled host code: tests/cpp/plane_segmentation_case.cpp is built with plain g++ against the shim and
the C-ABI library, run on a case written here, and what it prints is compared with the Python path over the same library —
integers exactly, doubles bit for bit.  MI355X only."""
import os
import struct
import subprocess

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import Submap
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from test_gpu_plane_segmentation import three_planes

pytestmark = pytest.mark.gpu

THR, CONF, VOXEL, RADIUS = 0.05, 1.0, 0.1, 30.0
SEED, ITERS, RANSAC_N, MAX_PLANES, MIN_INLIERS = 2 ** 33 + 7, 100, 3, 4, 300


def hexes(words):
    return np.array([float.fromhex(v) for v in words])


def test_compiled_path_equals_the_python_path(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "open3d_slam_advanced_rss_2024_public_amd")
    exe = tmp_path / "plane_segmentation_case"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-I" + os.path.join(root, "include"), "-I" + os.path.join(pkg, "cpp"),
                           os.path.join(root, "tests", "cpp", "plane_segmentation_case.cpp"), "-L" + pkg, "-lo3dslam_icp_hip", "-Wl,-rpath," + pkg,
                           "-o", str(exe)])
    pts = three_planes(3000, 23)
    pts = pts[np.isfinite(pts).all(axis=1)]
    nrm = np.roll(pts, 1, axis=1) * 0.5 + 1.0          # any values: they only have to follow their points
    with open(tmp_path / "case.bin", "wb") as f:
        f.write(struct.pack("<6q", len(pts), SEED, ITERS, RANSAC_N, MAX_PLANES, MIN_INLIERS))
        f.write(struct.pack("<4d", THR, CONF, VOXEL, RADIUS))
        f.write(np.ascontiguousarray(pts, np.float64).tobytes())
        f.write(np.ascontiguousarray(nrm, np.float64).tobytes())
    out = subprocess.run([str(exe), str(tmp_path / "case.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout[-600:], out.stderr[-600:])
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert lines[0] == ["size", str(len(pts))]
    # the Python path
    one = co.segment_plane(pts, THR, RANSAC_N, ITERS, CONF, SEED)
    labels, models, counts = co.segment_planes(pts, THR, MAX_PLANES, MIN_INLIERS, RANSAC_N, ITERS, CONF, SEED)
    assert len(counts) == 3
    assert lines[1][:5] == ["host_one", str(one.best_iteration), str(one.est_k), str(one.evaluated), str(len(one.inliers))]
    assert hexes(lines[1][5:]).tobytes() == one.plane_model.tobytes()
    at = 2
    for tag in ("host_peel", "submap_peel"):
        assert lines[at][:2] == [tag, str(len(counts))]
        if tag == "submap_peel":
            assert int(lines[at][2]) == int(((labels.astype(np.int64) + 2) * (np.arange(len(labels)) + 1)).sum())
        for k in range(len(counts)):
            ln = lines[at + 1 + k]
            assert ln[:2] == ["plane", str(counts[k])] and hexes(ln[2:]).tobytes() == models[k].tobytes()
        at += 1 + len(counts)
    keep = labels < 0
    assert lines[at] == ["removed", str(int((~keep).sum())), "size", str(int(keep.sum()))]
    assert lines[at + 1][0] == "first" and hexes(lines[at + 1][1:]).tobytes() == np.concatenate([pts[keep][0], nrm[keep][0]]).tobytes()
    assert lines[at + 2][0] == "last" and hexes(lines[at + 2][1:]).tobytes() == np.concatenate([pts[keep][-1], nrm[keep][-1]]).tobytes()
    # ... and the same removal through Submap.removePlanes
    m = Submap(VOXEL, co.croppingVolumeFactory("MaxRadius", RADIUS))
    m.setMapPointCloud(pts, nrm)
    removed, models_r = m.removePlanes(co.plane_params(THR, RANSAC_N, ITERS, CONF, SEED, MAX_PLANES, MIN_INLIERS))
    gp, gn = m.getMapPointCloud()
    assert removed == int((~keep).sum()) and gp.tobytes() == pts[keep].tobytes() and gn.tobytes() == nrm[keep].tobytes()
    assert models_r.tobytes() == models.tobytes()
