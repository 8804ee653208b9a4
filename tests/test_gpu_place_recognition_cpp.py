"""cpp/o3s_place_recognition.hpp on the device: PlaceRecognitionHip::buildLoopClosureConstraints, compiled with plain g++ against the C
ABI (tests/cpp/place_recognition_cases.cpp), returns the bits of the Python mirror on the same resident clouds.  MI355X only."""
import math
import os
import subprocess

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import place_recognition as pr
from open3d_slam_advanced_rss_2024_public_amd import registration as reg
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn
from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection
from test_gpu_place_recognition import NoScan, disc, rigid, submap_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")
REJECTED = {0: None, 1: "ransac:", 2: pr.REJECTED_RANSAC_INCONSISTENT, 3: "refinement: empty overlap", 4: "refinement score:",
            5: pr.REJECTED_ICP_INCONSISTENT}      # PlaceRecognitionHip::Rejected


def _mat(words, n):
    return np.array([float.fromhex(w) for w in words]).reshape(n, n).T


def test_compiled_place_recognition_returns_the_mirrors_bits(tmp_path):
    _lib.build()
    exe = tmp_path / "place_recognition_cases"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "place_recognition_cases.cpp"), "-L" + PKG, "-lo3dslam_icp_hip", "-Wl,-rpath," + PKG,
                           "-o", str(exe)])
    world = syn.make_world(3000.0, seed=21)
    centres = [syn.loop_pose(world, k)[:3, 3] for k in (0, 20, 40)]
    Ti = np.linalg.inv(rigid(math.radians(10.0), (0.5, -0.3, 0.0)))
    clouds = [disc(centres[0], 16.0), disc(centres[1], 16.0), None, None, np.ascontiguousarray(disc(centres[2], 16.0) @ Ti[:3, :3].T + Ti[:3, 3]), None]
    cents = [centres[0], centres[1], centres[2] + [100.0, 0.0, 0.0], centres[2] + [0.0, 20.5, 0.0], centres[2], centres[2]]
    script = []
    for i, (c, ctr) in enumerate(zip(clouds, cents)):
        path = "-"
        if c is not None:
            path = str(tmp_path / f"cloud_{i}.bin")
            c.tofile(path)
        script.append(f"cloud {path} {float(ctr[0])!r} {float(ctr[1])!r} {float(ctr[2])!r} {int(c is not None)}")
    script += [f"edge {i} {i + 1}" for i in range(5)]
    script += [f"closures 4 5 2.0 1 3 {math.radians(30.0)!r}", f"closures 4 5 2.0 1 3 {math.radians(5.0)!r}"]      # 1: O3S_O3D_POINT_TO_POINT
    out = subprocess.run([str(exe), "device"], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    lines = out.stdout.splitlines()
    # the mirror on the same clouds
    maps = [submap_of(c) if c is not None else submap_of(disc((0.0, 0.0), 3.0), features=False) for c in clouds]
    it = iter(maps)
    col = SubmapCollection(20.0, 3, 10 ** 9, 2, 0.1, ("MaxRadius", 1000.0), submap_factory=lambda: next(it), scan_factory=NoScan)
    for _ in range(5):
        col.create(np.zeros(3))
    for i in range(5):
        col.add_edge(i, i + 1)
    col.centers = cents
    at = 0
    for yaw in (30.0, 5.0):
        p = pr.PlaceRecognitionParameters(ransac=reg.RansacParams(seed=3), overlap_voxel_size=2.0, registration_type="PointToPointIcp",
                                          consistency_check=pr.ConsistencyCheckParameters(max_drift_yaw=math.radians(yaw)))
        place = pr.PlaceRecognition(p)
        want = place.buildLoopClosureConstraints(np.eye(4), col, 4, 5, 42.0)
        end = lines.index("end", at)
        got_c = [ln.split() for ln in lines[at:end] if ln.startswith("candidate")]
        got_k = [ln.split() for ln in lines[at:end] if ln.startswith("constraint")]
        at = end + 1
        assert len(got_c) == len(place.last_candidates) == 2 and len(got_k) == len(want)
        for w, c in zip(got_c, place.last_candidates):
            reason = REJECTED[int(w[2])]
            assert int(w[1]) == c.target_submap_idx and (c.rejected is None if reason is None else (c.rejected or "").startswith(reason))
            assert int(w[3]) == c.ransac.n_correspondences and int(w[4]) == len(c.ransac.correspondence_set)
            assert np.array_equal(_mat(w[5:21], 4), c.ransac.transformation)
        for w, k in zip(got_k, want):
            assert (int(w[1]), int(w[2]), int(w[3]), int(w[4]), float.fromhex(w[5])) == (4, k.target_submap_idx, 1, 0, 42.0)
            assert np.array_equal(_mat(w[6:22], 4), k.source_to_target) and np.array_equal(_mat(w[22:58], 6), k.information_matrix)
        if yaw == 30.0:
            assert 1 in [k.target_submap_idx for k in want]
        else:
            assert want == [] and place.last_candidates[1].rejected == pr.REJECTED_RANSAC_INCONSISTENT
