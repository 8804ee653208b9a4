"""The mapper's degeneracy policy (MapperParams::degeneracyPolicy / Mapper.degeneracy_policy) as COMPILED host code —
cpp/o3s_mapper.hpp driven by tests/cpp/localizability_loop.cpp (plain g++, links only the C-ABI library) — and through the Python
mirror, on a dozen sweeps down the corridor and through the room of tests/localizability_ref.py.  The odometry carries the true
along-axis motion plus 2 cm per sweep, so the prior is off along x by a known amount and the corridor cannot correct it.

Thresholds (sum_all_min, sum_strong_min, sum_partial_min) = (100, 50, 10): a free direction's contributions are the normals'
jitter (1e-3), far below kappa_f = cos 80 deg, so its sums are exactly 0; every constrained direction collects several hundred of
the ~4000 kept pairs of a sweep (the weakest, the rotation about the corridor's axis, about a tenth of them at 0.3 each).

  Off      the same binary with the flag off, the same bits as the Python mirror (whose Off path is the code as it was);
  Report   the same poses as Off, bit for bit, and the corridor's categories;
  Remap    in the corridor the along-axis component of every pose's correction to its prior is <= 1e-12 m and the other five
           components are those of the ICP's own pose of that sweep to 1e-9 (sweep 1, where Off has the same map and prior, also
           against Off's pose); in the room every pose is Off's, bit for bit."""
import os
import struct
import subprocess

import numpy as np
import pytest

import localizability_ref as lref
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import localizability as loc
from open3d_slam_advanced_rss_2024_public_amd.mapper import Mapper
from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")
SCAN_VOXEL, MAP_VOXEL, WIDE_R, NARROW_R, REF_PERIOD, MIN_MOVE = 0.1, 0.1, 7.0, 5.5, 0.25, 0.0
PARAMS = loc.LocalizabilityParams(sum_all_min=100.0, sum_strong_min=50.0, sum_partial_min=10.0)
POLICY = {"Off": 0, "Report": 1, "Remap": 2}
N_SWEEPS = 12
_cache = {}


def scene_of(name):
    if name not in _cache:
        _cache[name] = lref.sweeps(name, N_SWEEPS)
    return _cache[name]


def write_scene(path, sc, policy, min_category=1, params=PARAMS):
    cm = lambda T: np.ascontiguousarray(np.asarray(T, np.float64).T).tobytes()   # noqa: E731  column-major
    with open(path, "wb") as f:
        f.write(struct.pack("<3q", POLICY[policy], min_category, len(sc["scans"])))
        f.write(struct.pack("<6d", SCAN_VOXEL, MAP_VOXEL, WIDE_R, NARROW_R, REF_PERIOD, MIN_MOVE))
        f.write(struct.pack("<5d", params.filter_min, params.strong_min, params.sum_all_min, params.sum_strong_min, params.sum_partial_min))
        f.write(cm(sc["poses"][0]))
        for k, (sp, sn) in enumerate(sc["scans"]):
            f.write(struct.pack("<d", sc["stamps"][k]))
            f.write(cm(sc["odom"][k]))
            f.write(struct.pack("<q", len(sp)))
            f.write(np.ascontiguousarray(sp, np.float64).tobytes())
            f.write(np.ascontiguousarray(sn, np.float64).tobytes())


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("localizability_loop") / "localizability_loop"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "localizability_loop.cpp"), "-L" + PKG, "-lo3dslam_icp_hip", "-Wl,-rpath," + PKG, "-o", str(exe)])
    return exe


def hexes(words):
    return np.array([float.fromhex(w) for w in words])


@pytest.fixture(scope="module")
def compiled(driver, tmp_path_factory):
    """(scene, policy) -> the driver's rows, each run made once."""
    tmp = tmp_path_factory.mktemp("runs")
    done = {}

    def run(scene, policy):
        if (scene, policy) in done:
            return done[(scene, policy)]
        path, out = tmp / f"{scene}_{policy}.bin", tmp / f"{scene}_{policy}.txt"
        write_scene(path, scene_of(scene), policy)
        r = subprocess.run([str(driver), str(path), str(out)], capture_output=True, text=True, timeout=300)
        text = open(out).read() if os.path.exists(out) else ""
        assert r.returncode == 0, (r.stdout, r.stderr, text[-400:])
        rows = []
        for ln in text.strip().splitlines():
            w = ln.split()
            mat = lambda i: hexes(w[i:i + 16]).reshape(4, 4).T   # noqa: E731
            rows.append(dict(ok=int(w[1]), inserted=int(w[2]), threw=int(w[3]), replaced=int(w[4]), kept=int(w[5]), category=[int(v) for v in w[6:12]],
                             n_strong=[int(v) for v in w[12:18]], T=mat(18), T_icp=mat(34), prior=mat(50), centre=hexes(w[66:69]),
                             evec=hexes(w[69:87]).reshape(6, 3), sum_all=hexes(w[87:93]), sum_strong=hexes(w[93:99])))
        assert len(rows) == N_SWEEPS
        done[(scene, policy)] = rows
        return rows

    return run


def mirror_run(scene, policy):
    key = ("mirror", scene, policy)
    if key in _cache:
        return _cache[key]
    sc = scene_of(scene)
    col = SubmapCollection(1.0e9, 5, 10 ** 12, 3, MAP_VOXEL, ("MaxRadius", WIDE_R))
    m = Mapper(ICP(IcpConfig()), col, co.croppingVolumeFactory("MaxRadius", WIDE_R), co.croppingVolumeFactory("MaxRadius", NARROW_R), SCAN_VOXEL,
               REF_PERIOD, MIN_MOVE)
    m.set_calibration(np.eye(4))
    m.T = np.array(sc["poses"][0], np.float64)
    m.degeneracy_policy = policy
    m.localizability_params = PARAMS
    rows = []
    for k, (sp, sn) in enumerate(sc["scans"]):
        m.add_odometry_pose(sc["stamps"][k], sc["odom"][k])
        ok = m.add(sp, sn, sc["stamps"][k])
        rows.append(dict(ok=int(ok), inserted=m.flags[0], threw=m.flags[2], replaced=m.last_remap_replaced, T=m.T.copy(), loc=m.last_localizability))
    _cache[key] = rows
    return rows


def components(row, T):
    """The six components of T's correction to the row's prior (as the chain was handed it: fp32) along the row's directions."""
    prior = row["prior"].astype(np.float32).astype(np.float64)
    u, r = lref.correction(prior, T, row["centre"])
    return np.array([row["evec"][j] @ (u if j < 3 else r) for j in range(6)])


# ---- Off: today's mapper --------------------------------------------------------------------------------------------------------------
def test_off_is_the_mapper_as_it_was(compiled):
    rows, want = compiled("corridor", "Off"), mirror_run("corridor", "Off")
    for k, (r, w) in enumerate(zip(rows, want)):
        assert (r["ok"], r["inserted"], r["threw"], r["replaced"]) == (w["ok"], w["inserted"], 0, 0), k
        assert np.array_equal(r["T"], w["T"]), k
        assert r["kept"] == -1 and w["loc"] is None        # no analysis was run
        assert np.array_equal(r["T"], r["T_icp"]) or k == 0


# ---- Report -----------------------------------------------------------------------------------------------------------------------------
def test_report_changes_no_pose_and_names_the_corridor(compiled):
    off, rep, mirror = compiled("corridor", "Off"), compiled("corridor", "Report"), mirror_run("corridor", "Report")
    for k in range(N_SWEEPS):
        assert np.array_equal(off[k]["T"], rep[k]["T"]) and np.array_equal(rep[k]["T"], mirror[k]["T"]), k
        assert rep[k]["replaced"] == 0
        if k == 0:                                          # the first sweep founds the map: nothing was registered
            assert rep[k]["kept"] == -1 and mirror[k]["loc"] is None
            continue
        print(k, "kept", rep[k]["kept"], "sum_all", np.round(rep[k]["sum_all"], 1), "sum_strong", np.round(rep[k]["sum_strong"], 1))
        assert rep[k]["category"] == [0, 2, 2, 2, 2, 2], (k, rep[k]["category"], rep[k]["sum_all"], rep[k]["sum_strong"])
        assert abs(rep[k]["evec"][0][0]) > 0.999 and rep[k]["kept"] > 1000
        got = mirror[k]["loc"]                              # the mirror's analysis is the same call on the same state
        assert got.kept == rep[k]["kept"] and np.array_equal(got.category, rep[k]["category"]) and np.array_equal(got.evec, rep[k]["evec"])
        assert np.array_equal(got.sum_all, rep[k]["sum_all"]) and np.array_equal(got.centre, rep[k]["centre"])


# ---- Remap ------------------------------------------------------------------------------------------------------------------------------
def test_remap_keeps_the_prior_along_the_corridor(compiled):
    off, rem, mirror = compiled("corridor", "Off"), compiled("corridor", "Remap"), mirror_run("corridor", "Remap")
    moved = 0.0
    for k in range(1, N_SWEEPS):
        r = rem[k]
        assert r["category"] == [0, 2, 2, 2, 2, 2] and r["replaced"] == 1 and r["threw"] == 0, (k, r["category"])
        assert np.array_equal(r["T"], mirror[k]["T"]) and mirror[k]["replaced"] == 1, k
        c_out, c_icp = components(r, r["T"]), components(r, r["T_icp"])
        print(k, "along-axis component of the correction: remapped", c_out[0], " ICP's own", c_icp[0], " others differ by", np.abs(c_out[1:] - c_icp[1:]).max())
        assert abs(c_out[0]) <= 1e-12, (k, c_out[0])
        assert np.abs(c_out[1:] - c_icp[1:]).max() <= 1e-9, (k, c_out, c_icp)
        moved = max(moved, abs(c_icp[0]))
    assert moved > 1e-6        # the ICP did slide along the axis: the remap had something to undo
    # sweep 1: Off saw the same map and the same prior
    assert np.array_equal(off[1]["prior"], rem[1]["prior"]) and np.array_equal(off[1]["T_icp"], rem[1]["T_icp"])
    assert np.abs(components(rem[1], rem[1]["T"])[1:] - components(rem[1], off[1]["T"])[1:]).max() <= 1e-9


def test_remap_in_the_room_is_off_bit_for_bit(compiled):
    off, rem = compiled("room", "Off"), compiled("room", "Remap")
    for k in range(N_SWEEPS):
        assert np.array_equal(off[k]["T"], rem[k]["T"]), k
        if k:
            assert rem[k]["category"] == [2] * 6 and rem[k]["replaced"] == 0, (k, rem[k]["category"], rem[k]["sum_all"], rem[k]["sum_strong"])


def test_unset_thresholds_are_refused_when_the_policy_needs_them(driver, tmp_path):
    sc = dict(scene_of("room"))
    sc["scans"], sc["stamps"], sc["odom"] = sc["scans"][:1], sc["stamps"][:1], sc["odom"][:1]
    path, out = tmp_path / "unset.bin", tmp_path / "unset.txt"
    write_scene(path, sc, "Report", params=loc.LocalizabilityParams())
    r = subprocess.run([str(driver), str(path), str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "thresholds are unset" in open(out).read()
