"""The outlier filter inside the mapping loop (Mapper.scan_outlier_removal, MapperParams::scanOutlierRemoval): stray returns reach
neither the registration nor the map.  MI355X only.

Eight sweeps of the synthetic room (synthetic.make_world: floor, ceiling, walls, pillars), each with 30 points hung in the air at
known positions — more than 2 m from every surface and more than 0.7 m from each other.
  filter off                  every stray is in the map;
  radius filter {0.5 m, 3}    no stray is in the map (nothing within 1 m of any of the 240 positions), and every other point of the
                              unfiltered map is still there;
  compiled == restatement     cpp/o3s_mapper.hpp (tests/cpp/outlier_mapper_loop.cpp, plain g++) and mapper.py give the same poses and the
                              same map, bit for bit, with the filter on and with it off.

"Still there": both runs register every sweep to within centimetres of the same pose (asserted: 2 cm), so a surface sample lands in
the same map voxel or a neighbouring one; a map point is the mean of its voxel's samples, hence within one voxel diagonal of each
of them, and the filtered map's point for that sample within one more: TOL = 2 sqrt(3) voxel + 0.05 m = 0.40 m — below the filter's
radius and far below the 2 m that separate a stray from everything else.  The filter's own contract removes a surface sample that
has no more than 3 points within 0.5 m in its sweep; those samples (known exactly: the sweep's merge cloud before and after) are
excused, and there must be next to none of them (0.5 % of a sweep at most)."""
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig, ProcessedScan
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn
from open3d_slam_advanced_rss_2024_public_amd.mapper import Mapper
from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection

pytestmark = pytest.mark.gpu

SCAN_VOXEL, MAP_VOXEL, WIDE_R, NARROW_R, REF_PERIOD, MIN_MOVE = 0.1, 0.1, 9.0, 7.0, 0.25, 0.0
K, STRAYS = 8, 30
STRAY_SEPARATION = 0.7   # above the filter's radius: no stray is another stray's support
FILTER = (1, 3, 0.5)   # radius, nb_points 3, 0.5 m
TOL = 2.0 * np.sqrt(3.0) * MAP_VOXEL + 0.05


def face_distance(world, p):
    """distance of the points p (M, 3) from the nearest rectangle of the world"""
    best = np.full(len(p), np.inf)
    for c, u, v in zip(world.centres, world.u, world.v):
        lu, lv = np.linalg.norm(u), np.linalg.norm(v)
        d = p - c
        a = np.clip(d @ (u / lu), -lu, lu)
        b = np.clip(d @ (v / lv), -lv, lv)
        q = c + a[:, None] * (u / lu) + b[:, None] * (v / lv)
        best = np.minimum(best, np.linalg.norm(p - q, axis=1))
    return best


_SCENARIO = {}


def scenario():
    if _SCENARIO:
        return _SCENARIO
    world = syn.make_world(9000.0, seed=3)
    rng = np.random.default_rng(2024)
    poses, sweeps, strays_world = [], [], np.zeros((0, 3))
    for k in range(K):
        T = syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.04 * k), np.array([-6.0 + 0.45 * k, 0.5 + 0.1 * k, 1.5]))
        sp, sn = syn.make_scan(world, 30000, T, radius=10.0, sigma=0.01, seed=400 + k)
        sp, sn = sp.astype(np.float64), sn.astype(np.float64)
        mine = np.zeros((0, 3))
        for _ in range(50):   # rejection: in the air, inside the wide crop of this sweep, apart from every other stray
            c = T[:3, 3] + rng.uniform([-8.0, -8.0, 0.55], [8.0, 8.0, 2.45], (400, 3))
            c = c[(np.linalg.norm(c - T[:3, 3], axis=1) < WIDE_R - 0.5) & (face_distance(world, c) > 2.0)]
            for q in c:
                others = np.concatenate([strays_world, mine])
                if len(mine) < STRAYS and (len(others) == 0 or np.linalg.norm(others - q, axis=1).min() > STRAY_SEPARATION):
                    mine = np.concatenate([mine, q[None]])
            if len(mine) == STRAYS:
                break
        assert len(mine) == STRAYS, "the room has no place left for this sweep's strays"
        strays_world = np.concatenate([strays_world, mine])
        Ti = np.linalg.inv(T)
        ss = mine @ Ti[:3, :3].T + Ti[:3, 3]
        sdir = -ss / np.linalg.norm(ss, axis=1, keepdims=True)
        at = rng.choice(len(sp) + 1, STRAYS, replace=False)   # scattered through the sweep, not appended
        sp, sn = np.insert(sp, at, ss, axis=0), np.insert(sn, at, sdir, axis=0)
        poses.append(T)
        sweeps.append((sp, sn))
    assert len(strays_world) == K * STRAYS and face_distance(world, strays_world).min() > 2.0
    _SCENARIO.update(poses=poses, sweeps=sweeps, strays=strays_world, stamps=[0.1 * k for k in range(K)])
    return _SCENARIO


def run_python(filt, record=None):
    sc = scenario()
    col = SubmapCollection(1.0e9, 5, 10 ** 12, 3, MAP_VOXEL, ("MaxRadius", WIDE_R))
    m = Mapper(ICP(IcpConfig()), col, co.croppingVolumeFactory("MaxRadius", WIDE_R), co.croppingVolumeFactory("MaxRadius", NARROW_R), SCAN_VOXEL,
               REF_PERIOD, MIN_MOVE)
    m.set_calibration(np.eye(4))
    m.scan_outlier_removal = None if filt is None else co.outlier_params(*filt)
    out = []
    for k in range(K):
        m.odom[sc["stamps"][k]] = sc["poses"][k]
        if k == 0:
            m.T = sc["poses"][0].copy()
        if record is not None:
            record["k"] = k
        assert m.add(*sc["sweeps"][k], sc["stamps"][k])
        assert m.flags[0] == 1 and m.flags[2] == 0   # inserted; the ICP did not throw
        out.append(m.T.copy())
    mp, mn = m.sm.getMapPointCloud()
    return out, mp, mn


def run_compiled(tmp_path, filt):
    sc = scenario()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "open3d_slam_advanced_rss_2024_public_amd")
    exe = tmp_path / "outlier_mapper_loop"
    if not exe.exists():
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-I" + os.path.join(root, "include"), "-I" + os.path.join(pkg, "cpp"),
                               os.path.join(root, "tests", "cpp", "outlier_mapper_loop.cpp"), "-L" + pkg, "-lo3dslam_icp_hip", "-Wl,-rpath," + pkg,
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
    kind, nb, value = (0, 0, 0.0) if filt is None else filt
    res = tmp_path / f"out_{kind}.bin"
    out = subprocess.run([str(exe), str(path), str(res), str(kind), str(nb), repr(float(value))], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    raw = np.fromfile(res, np.float64)
    poses = [raw[16 * k:16 * k + 16].reshape(4, 4).T for k in range(K)]
    n = int(np.frombuffer(raw[16 * K:16 * K + 1].tobytes(), np.int64)[0])
    body = raw[16 * K + 1:]
    assert len(body) == 6 * n
    return poses, body[:3 * n].reshape(n, 3), body[3 * n:].reshape(n, 3)


def test_strays_reach_the_map_without_the_filter_and_not_with_it(tmp_path, monkeypatch):
    sc = scenario()
    strays = sc["strays"]
    poses_off, map_off, _ = run_python(None)
    tree_off = cKDTree(map_off)
    d_off, _ = tree_off.query(strays)
    assert (d_off < 0.15).all(), f"filter off: {(d_off >= 0.15).sum()} of {len(strays)} strays are missing from the map"

    # filter on; the sweeps' merge clouds before and after, to know exactly which surface samples the filter took
    taken, sizes, rec = [], [], {}
    plain = ProcessedScan.removeOutliers

    def spying(self, cropper, params):
        before = self.merge[0]
        res = plain(self, cropper, params)
        after = self.merge[0]
        gone = before[~np.isin(before.view([("", before.dtype)] * 3).ravel(), after.view([("", after.dtype)] * 3).ravel())]
        taken.append((rec["k"], gone))
        sizes.append(len(before))
        return res

    monkeypatch.setattr(ProcessedScan, "removeOutliers", spying)
    poses_on, map_on, nrm_on = run_python(FILTER, rec)
    monkeypatch.undo()
    assert len(taken) == K
    for a, b in zip(poses_off, poses_on):   # both runs register every sweep at (nearly) the same pose
        assert np.linalg.norm(a[:3, 3] - b[:3, 3]) < 0.02
    tree_on = cKDTree(map_on)
    d_on, _ = tree_on.query(strays)
    assert (d_on > 1.0).all(), f"filter on: map points within 1 m of {(d_on <= 1.0).sum()} stray positions"
    # the surface samples the filter took, in the map frame
    excused = np.zeros((0, 3))
    for (k, gone), n_before in zip(taken, sizes):
        T = poses_on[k]
        w = gone @ T[:3, :3].T + T[:3, 3]
        surf = w[cKDTree(strays).query(w)[0] > 0.3]
        assert len(gone) - len(surf) == STRAYS, (k, len(gone), len(surf))       # every stray of the sweep was taken ...
        assert len(surf) <= 0.005 * n_before, (k, len(surf), n_before)           # ... and next to nothing else
        excused = np.concatenate([excused, surf])
    non_stray = map_off[cKDTree(strays).query(map_off)[0] > 0.3]
    assert len(non_stray) == len(map_off) - len(strays)
    d, _ = tree_on.query(non_stray)
    missing = non_stray[d > TOL]
    if len(missing):
        assert len(excused) and (cKDTree(excused).query(missing)[0] <= TOL).all(), f"{len(missing)} surface points of the unfiltered map are gone"
    assert len(map_on) > 0.98 * (len(map_off) - len(strays))

    # the compiled mapper: same poses, same map, bit for bit — with the filter on and with it off
    for filt, (pp, pm, pn) in ((FILTER, (poses_on, map_on, nrm_on)), (None, run_python(None))):
        cp, cmap, cn = run_compiled(tmp_path, filt)
        for k in range(K):
            assert np.array_equal(cp[k], pp[k]), (filt, k)
        assert cmap.tobytes() == pm.tobytes() and cn.tobytes() == pn.tobytes(), filt
