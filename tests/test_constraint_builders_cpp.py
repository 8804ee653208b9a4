"""cpp/o3s_constraint_builders.hpp, compiled with plain g++ against the C ABI (tests/cpp/constraint_builders_cases.cpp), gives what
constraint_builders.py gives: the same pair lists and constraints with stand-in device calls on the CPU, and on the GPU the same
bits for a two-pair collection of resident submaps."""
import os
import subprocess

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import constraint_builders as cb
from open3d_slam_advanced_rss_2024_public_amd import pose_graph as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    _lib.build()
    out = tmp_path_factory.mktemp("cb") / "constraint_builders_cases"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "constraint_builders_cases.cpp"), "-L" + PKG, "-lo3dslam_icp_hip", "-Wl,-rpath," + PKG,
                           "-o", str(out)])
    return str(out)


def run(exe, script, *args):
    out = subprocess.run([exe, *args], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.splitlines()


def constraints_of(lines):
    out = []
    for ln in lines:
        w = ln.split()
        if w[0] == "constraint":
            v = [float.fromhex(x) for x in w[5:]]
            out.append((int(w[1]), int(w[2]), int(w[3]), int(w[4]), np.array(v[:16]).reshape(4, 4).T, np.array(v[16:]).reshape(6, 6).T))
    return out


class Col:
    def __init__(self, parents, active, map_voxel, maps=None):
        self.maps = maps if maps is not None else list(range(len(parents)))
        self.ids = list(range(len(parents)))
        self.parents, self.active, self.map_voxel = list(parents), active, map_voxel
        self.refine_odometry_constraints = False


def same_constraints(got, want):
    assert len(got) == len(want)
    for g, c in zip(got, want):
        assert g[:4] == (c.source_submap_idx, c.target_submap_idx, int(c.is_information_matrix_valid), int(c.is_odometry_constraint))
        assert np.array_equal(g[4], c.source_to_target) and np.array_equal(g[5], c.information_matrix)


def test_compiled_builders_follow_the_mirrors_rules(exe):
    parents, empty = [0, 0, 1, 2, 2, 4], {(2, 3)}
    log = []

    def dev(pairs, voxel, dist, min_pts):
        log.append("call %d %s %s %d " % (len(pairs), float(voxel).hex(), float(dist).hex(), min_pts) + " ".join(f"{s}:{t}" for s, t in pairs))
        return [(np.zeros((6, 6)), (0, 0), 0, _lib.ERR_EMPTY_REFERENCE) if p in empty else (np.full((6, 6), k + 1.0), (1, 1), 1, _lib.OK)
                for k, p in enumerate(pairs)]

    def refine(s, t, dist, voxel, min_pts, iters):
        log.append("refine %d %d %s %s %d %d" % (s, t, float(dist).hex(), float(voxel).hex(), min_pts, iters))
        if (s, t) in empty:
            return None, None, (0, 0)
        T = np.eye(4)
        T[0, 3] = 0.5

        class R:
            transformation = T
        return R(), np.full((6, 6), 3.0), (1, 1)

    script = [f"submap {p}" for p in parents] + ["voxel 0.25", "active 2", "empty 2 3", "have 1 2",
                                                 "candidates 0 3 1 5 3", "all", "active 5", "all", "clear", "voxel 0.0005", "refine 1", "candidates 3 5"]
    lines = run(exe, script)
    col = Col(parents, 2, 0.25)
    cs = [pg.Constraint(source_submap_idx=1, target_submap_idx=2)]
    want_blocks = []
    cb.compute_odometry_constraints(col, cs, [(0, 0.0), (3, 0.0), (1, 0.0), (5, 0.0), (3, 0.0)], dev, refine)
    want_blocks.append(list(cs))
    cb.compute_odometry_constraints(col, cs, None, dev, refine)
    want_blocks.append(list(cs))
    col.active = 5
    cb.compute_odometry_constraints(col, cs, None, dev, refine)
    want_blocks.append(list(cs))
    cs, col.map_voxel, col.refine_odometry_constraints = [], 0.0005, True
    cb.compute_odometry_constraints(col, cs, [(3, 0.0), (5, 0.0)], dev, refine)
    want_blocks.append(list(cs))

    def words(ln):                                                        # (%a and float.hex spell the same number differently)
        return [float.fromhex(w) if "0x" in w else w for w in ln.split()]

    assert [words(ln) for ln in lines if ln.startswith(("call", "refine"))] == [words(entry) for entry in log]
    # one device call per invocation that has something to build (the first `all` has not), one refinement per pair
    assert [entry.split()[0] for entry in log] == ["call", "call", "refine", "refine"]
    at = 0
    for want in want_blocks:
        end = lines.index("end", at)
        same_constraints(constraints_of(lines[at:end]), want)
        at = end + 1
    assert at == len(lines)


@pytest.mark.gpu
def test_compiled_builders_return_the_mirrors_bits_on_the_device(exe, tmp_path):
    from open3d_slam_advanced_rss_2024_public_amd import Submap
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

    rng = np.random.default_rng(11)
    base = rng.uniform(-4.0, 4.0, (3000, 3))
    clouds = [base[(base[:, 0] > -4.0 + 1.5 * k)] + rng.normal(0.0, 0.01, (int((base[:, 0] > -4.0 + 1.5 * k).sum()), 3)) for k in range(3)]
    script = []
    for k, c in enumerate(clouds):
        path = str(tmp_path / f"cloud_{k}.bin")
        np.ascontiguousarray(c).tofile(path)
        script.append(f"submap {max(k - 1, 0)} {path}")
    script += ["voxel 0.1", "active 2", "candidates 1 2"]
    got = constraints_of(run(exe, script, "device"))
    big = co.croppingVolumeFactory("MaxRadius", 1.0e6)
    maps = []
    for c in clouds:
        m = Submap(0.0, big)
        m.setMapPointCloud(c, None)
        maps.append(m)
    want = cb.compute_odometry_constraints(Col([0, 0, 1], 2, 0.1, maps), [], [(1, 0.0), (2, 0.0)])
    same_constraints(got, want)
    assert [g[:2] for g in got] == [(0, 1), (1, 2)] and all(g[5][3, 3] > 1000 for g in got)
