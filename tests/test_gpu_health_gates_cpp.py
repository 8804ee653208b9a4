"""The two registration health gates as COMPILED host code — cpp/o3s_mapper.hpp and cpp/o3s_submap_collection.hpp driven by
tests/cpp/health_gates.cpp (plain g++, links only the C-ABI library) — against the Python mirror, step for step, on the scenes of
tests/health_scenes.py: every flag, count, fitness and pose must be the same bits."""
import math
import os
import subprocess

import numpy as np
import pytest

import health_scenes as hs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("health_gates") / "health_gates"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "health_gates.cpp"), "-L" + PKG, "-lo3dslam_icp_hip", "-Wl,-rpath," + PKG, "-o", str(exe)])
    return exe


def run_driver(exe, tmp_path, name, *scene_args, **scene_kw):
    scene, out = tmp_path / (name + ".bin"), tmp_path / (name + ".txt")
    hs.write_scene(scene, *scene_args, **scene_kw)
    r = subprocess.run([str(exe), str(scene), str(out)], capture_output=True, text=True, timeout=300)
    text = open(out).read() if os.path.exists(out) else ""
    assert r.returncode == 0, (r.stdout, r.stderr, text[-400:])
    return [ln.split() for ln in text.strip().splitlines()]


def same_float(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize("ignore", [False, True])
def test_compiled_mapper_takes_the_fitness_gate_as_the_mirror_does(driver, tmp_path, ignore):
    lines = run_driver(driver, tmp_path, "fitness", 0, hs.fitness_scene(), hs.NEVER_SWITCH, hs.WIDE_R, hs.NARROW_R, ignore=ignore)
    want = hs.fitness_run(ignore)
    assert len(lines) == len(want) == 4
    for k, (w, r) in enumerate(zip(lines, want)):
        got = dict(ok=int(w[1]), inserted=int(w[2]), refreset=int(w[3]), threw=int(w[4]), rejected=int(w[5]), n_corr=int(w[6]), n_points=int(w[7]),
                   map_size=int(w[8]))
        for a, v in got.items():
            assert v == r[a], (k, a, v, r[a])
        assert same_float(float.fromhex(w[9]), r["fitness"]) and same_float(float.fromhex(w[10]), r["rmse"]), k
        T = np.array([float.fromhex(v) for v in w[11:27]]).reshape(4, 4).T
        assert np.array_equal(T, r["T"]), k
    assert [int(w[5]) for w in lines] == ([0, 0, 0, 0] if ignore else [0, 0, 1, 0])


@pytest.mark.parametrize("shifted,check", [(False, True), (True, True), (True, False)])
def test_compiled_collection_takes_the_revisit_check_as_the_mirror_does(driver, tmp_path, shifted, check):
    lines = run_driver(driver, tmp_path, "revisit", 1, hs.revisit_scene(shifted), hs.REVISIT, hs.BIG_WIDE_R, hs.BIG_WIDE_R, check=check)
    want = hs.revisit_run(shifted, check)
    assert len(lines) == len(want)
    for k, (w, r) in enumerate(zip(lines, want)):
        assert (int(w[1]), int(w[2]), int(w[3])) == (r["active"], r["n_submaps"], r["switched"]), k
        assert [int(v) for v in w[4:-1]] == r["snapshots"], k
        assert same_float(float.fromhex(w[-1]), r["fitness"]), k
