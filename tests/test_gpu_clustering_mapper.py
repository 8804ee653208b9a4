"""Small-cluster removal inside the mapping loop (Mapper.scan_cluster_removal, MapperParams::scanClusterRemoval): a supported blob
reaches neither the registration nor the map.  MI355X only.

Four sweeps of the synthetic room (synthetic.make_world), each with a blob of 25 points — a 5 x 5 patch at 0.12 m spacing, so that
every point keeps a scan voxel of its own — hung in the air more than 2 m from every surface.  A sweep's merge cloud is one cluster
without noise at eps 0.5 m, min_points 4 (the room's surfaces are connected and dense; asserted on the first sweep), the blob a
second one of 25 points: the outlier filter {0.5 m, 3} keeps it, min_cluster_size 50 removes exactly it.

  field unset          mapper.py and cpp/o3s_mapper.hpp (tests/cpp/cluster_mapper_loop.cpp, plain g++) give the poses and the map, bit
                       for bit, of a run that never heard of the field: a Mapper whose pre-processing is written out below;
  field set            both give those of the manual sequence — pre-process, outlier filter if set, removeSmallClusters, register,
                       insert — with the outlier filter unset and set;
  the blob             is in the map of the first run, nowhere near the map of the second, and what a sweep loses is exactly it."""
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn
from open3d_slam_advanced_rss_2024_public_amd.mapper import Mapper
from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection
from test_gpu_outlier_removal_mapper import face_distance

pytestmark = pytest.mark.gpu

SCAN_VOXEL, MAP_VOXEL, WIDE_R, NARROW_R, REF_PERIOD, MIN_MOVE = 0.1, 0.1, 9.0, 7.0, 0.25, 0.0
K, BLOB = 4, 25
CLUSTER = (0.5, 4, 50)     # eps, min_points, min_cluster_size
OUTLIER = (1, 3, 0.5)      # radius filter: nb_points 3, 0.5 m — the blob passes it


_SCENARIO = {}


def scenario():
    if _SCENARIO:
        return _SCENARIO
    world = syn.make_world(9000.0, seed=3)
    rng = np.random.default_rng(2025)
    g = (np.arange(5) - 2.0) * 0.12
    patch = np.stack([np.repeat(g, 5), np.tile(g, 5), np.zeros(25)], axis=1)
    poses, sweeps, blobs = [], [], []
    for k in range(K):
        T = syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.04 * k), np.array([-6.0 + 0.45 * k, 0.5 + 0.1 * k, 1.5]))
        sp, sn = syn.make_scan(world, 12000, T, radius=10.0, sigma=0.01, seed=400 + k)
        sp, sn = sp.astype(np.float64), sn.astype(np.float64)
        c = T[:3, 3] + rng.uniform([-7.0, -7.0, 0.3], [7.0, 7.0, 2.7], (4000, 3))
        ok = (np.linalg.norm(c - T[:3, 3], axis=1) < WIDE_R - 1.0) & (face_distance(world, c) > 2.4)
        if blobs:
            ok &= np.linalg.norm(c[:, None, :] - np.array(blobs)[None, :, :], axis=2).min(axis=1) > 2.0
        assert ok.any(), "the room has no place for this sweep's blob"
        centre = c[np.flatnonzero(ok)[0]]
        blobs.append(centre)
        Ti = np.linalg.inv(T)
        bs = (centre + patch) @ Ti[:3, :3].T + Ti[:3, 3]
        bdir = -bs / np.linalg.norm(bs, axis=1, keepdims=True)
        at = np.sort(rng.choice(len(sp) + 1, BLOB, replace=False))   # scattered through the sweep, not appended
        sp, sn = np.insert(sp, at, bs, axis=0), np.insert(sn, at, bdir, axis=0)
        poses.append(T)
        sweeps.append((sp, sn))
    blobs = np.array(blobs)
    assert (face_distance(world, (blobs[:, None, :] + patch[None, :, :]).reshape(-1, 3)) > 2.0).all()
    _SCENARIO.update(poses=poses, sweeps=sweeps, blobs=blobs, stamps=[0.1 * k for k in range(K)])
    return _SCENARIO


class ManualMapper(Mapper):
    """the pre-processing written out, without a word about Mapper.scan_cluster_removal: pre-process, outlier filter if set,
    removeSmallClusters if asked for here; registration and insert are Mapper.add's"""
    manual_outlier = None
    manual_cluster = None
    spy = None

    def preprocess(self, sp, sn, stamp=None, point_times=None):
        self.ps.preprocess(self.wide, self.scan_voxel, self.narrow, sp, sn)
        if self.manual_outlier is not None:
            self.ps.removeOutliers(self.narrow, self.manual_outlier)
        if self.manual_cluster is not None:
            before = self.ps.merge[0] if self.spy is not None else None
            self.ps.removeSmallClusters(self.narrow, self.manual_cluster)
            if self.spy is not None:
                self.spy.append((before, self.ps.merge[0]))


def run_python(outlier, cluster, manual, spy=None):
    sc = scenario()
    col = SubmapCollection(1.0e9, 5, 10 ** 12, 3, MAP_VOXEL, ("MaxRadius", WIDE_R))
    m = (ManualMapper if manual else Mapper)(ICP(IcpConfig()), col, co.croppingVolumeFactory("MaxRadius", WIDE_R),
                                            co.croppingVolumeFactory("MaxRadius", NARROW_R), SCAN_VOXEL, REF_PERIOD, MIN_MOVE)
    m.set_calibration(np.eye(4))
    q = None if outlier is None else co.outlier_params(*outlier)
    c = None if cluster is None else co.dbscan_params(*cluster)
    if manual:
        m.manual_outlier, m.manual_cluster, m.spy = q, c, spy
    else:
        m.scan_outlier_removal = q
        if cluster is not None:   # unset: the attribute is left as the constructor made it
            m.scan_cluster_removal = c
    out = []
    for k in range(K):
        m.odom[sc["stamps"][k]] = sc["poses"][k]
        if k == 0:
            m.T = sc["poses"][0].copy()
        assert m.add(*sc["sweeps"][k], sc["stamps"][k])
        assert m.flags[0] == 1 and m.flags[2] == 0   # inserted; the ICP did not throw
        out.append(m.T.copy())
    mp, mn = m.sm.getMapPointCloud()
    return out, mp, mn


def run_compiled(tmp_path, outlier, cluster):
    sc = scenario()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "open3d_slam_advanced_rss_2024_public_amd")
    exe = tmp_path / "cluster_mapper_loop"
    if not exe.exists():
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-I" + os.path.join(root, "include"), "-I" + os.path.join(pkg, "cpp"),
                               os.path.join(root, "tests", "cpp", "cluster_mapper_loop.cpp"), "-L" + pkg, "-lo3dslam_icp_hip", "-Wl,-rpath," + pkg,
                               "-o", str(exe)])
    path = tmp_path / "scenario.bin"
    if not path.exists():
        cm = lambda T: np.ascontiguousarray(np.asarray(T, np.float64).T).tobytes()   # noqa: E731  column-major
        with open(path, "wb") as f:
            f.write(np.array([SCAN_VOXEL, MAP_VOXEL, WIDE_R, NARROW_R, REF_PERIOD, MIN_MOVE]).tobytes())
            f.write(np.int64(K).tobytes())
            for k in range(K):
                sp, sn = sc["sweeps"][k]
                f.write(np.float64(sc["stamps"][k]).tobytes() + cm(sc["poses"][k]) + cm(sc["poses"][k]) + np.int64(len(sp)).tobytes())
                f.write(np.ascontiguousarray(sp).tobytes() + np.ascontiguousarray(sn).tobytes())
    kind, nb, value = (0, 0, 0.0) if outlier is None else outlier
    args = [str(exe), str(path), str(tmp_path / "out.bin"), str(kind), str(nb), repr(float(value))]
    if cluster is not None:   # unset: the driver does not touch the field
        args += [repr(float(cluster[0])), str(cluster[1]), str(cluster[2])]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.float64)
    poses = [raw[16 * k:16 * k + 16].reshape(4, 4).T for k in range(K)]
    n = int(np.frombuffer(raw[16 * K:16 * K + 1].tobytes(), np.int64)[0])
    body = raw[16 * K + 1:]
    assert len(body) == 6 * n
    return poses, body[:3 * n].reshape(n, 3), body[3 * n:].reshape(n, 3)


def same_run(a, b):
    (pa, ma, na), (pb, mb, nb) = a, b
    return all(np.array_equal(x, y) for x, y in zip(pa, pb)) and ma.tobytes() == mb.tobytes() and na.tobytes() == nb.tobytes()


def test_field_unset_is_the_loop_that_never_heard_of_it(tmp_path):
    for outlier in (None, OUTLIER):
        plain = run_python(outlier, None, manual=True)
        assert same_run(run_python(outlier, None, manual=False), plain), outlier
        assert same_run(run_compiled(tmp_path, outlier, None), plain), outlier
    blobs = scenario()["blobs"]
    d, _ = cKDTree(plain[1]).query(blobs)
    assert (d < 0.15).all(), "without the removal every blob is in the map — also behind the outlier filter, which it passes"
    fresh = Mapper(ICP(IcpConfig()), SubmapCollection(1.0e9, 5, 10 ** 12, 3, MAP_VOXEL, ("MaxRadius", WIDE_R)), co.croppingVolumeFactory("MaxRadius", WIDE_R),
                   co.croppingVolumeFactory("MaxRadius", NARROW_R), SCAN_VOXEL, REF_PERIOD, MIN_MOVE)
    assert fresh.scan_cluster_removal is None   # the default


def test_field_set_is_the_manual_sequence_and_the_blob_is_gone(tmp_path):
    sc = scenario()
    spy = []
    manual = run_python(None, CLUSTER, manual=True, spy=spy)
    assert same_run(run_python(None, CLUSTER, manual=False), manual)
    assert same_run(run_compiled(tmp_path, None, CLUSTER), manual)
    both = run_python(OUTLIER, CLUSTER, manual=True)
    assert same_run(run_python(OUTLIER, CLUSTER, manual=False), both)
    assert same_run(run_compiled(tmp_path, OUTLIER, CLUSTER), both)
    # every sweep lost exactly its blob
    assert len(spy) == K
    g = (np.arange(5) - 2.0) * 0.12
    patch = np.stack([np.repeat(g, 5), np.tile(g, 5), np.zeros(25)], axis=1)
    for k, (before, after) in enumerate(spy):
        if k == 0:   # the claim the scenario rests on: the room is one cluster without noise, the blob a second one of 25
            lab, n, sizes = co.cluster_dbscan(before, CLUSTER[0], CLUSTER[1])
            assert n == 2 and (lab >= 0).all() and sorted(sizes.tolist()) == [BLOB, len(before) - BLOB]
        kept = np.isin(before.view([("", before.dtype)] * 3).ravel(), after.view([("", after.dtype)] * 3).ravel())
        gone = before[~kept]
        assert len(gone) == BLOB and len(after) == len(before) - BLOB, (k, len(gone), len(before), len(after))
        assert after.tobytes() == before[kept].tobytes()      # the rest in order
        Ti = np.linalg.inv(sc["poses"][k])
        want = (sc["blobs"][k] + patch) @ Ti[:3, :3].T + Ti[:3, 3]
        assert (cKDTree(want).query(gone)[0] < 1e-9).all(), k
    for run in (manual, both):
        d, _ = cKDTree(run[1]).query(sc["blobs"])
        assert (d > 1.0).all(), f"map points within 1 m of {(d <= 1.0).sum()} blob positions"
