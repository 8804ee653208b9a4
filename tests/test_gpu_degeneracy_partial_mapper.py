"""MapperParams::degeneracyPartial / Mapper.degeneracy_partial under the Constrain policy as COMPILED host code — cpp/o3s_mapper.hpp
driven by tests/cpp/degeneracy_partial_loop.cpp (plain g++, links only the C-ABI library) — and through the Python mirror, on sweeps
of the "door" scene (tests/degeneracy_partial_ref.py): a corridor whose axis only a small panel sees.

The thresholds come from the analysis of the first registration (a Report run of the mirror): the axis falls between
sum_partial_min and sum_strong_min, every other direction above sum_all_min (degeneracy_partial_ref.door_thresholds).
  flag set    compiled and mirror agree bit for bit: poses, masks, partial masks and the values the rows carried; every iteration of
              every registration constrains the axis to a value, and the poses differ from the zero-constrained ones;
  flag unset  the driver's poses and masks are those of tests/cpp/degeneracy_loop.cpp (Constrain before the flag existed) and of the
              mirror, bit for bit, and there is no partial trace."""
import os
import struct
import subprocess

import numpy as np
import pytest

import degeneracy_partial_ref as pref
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import localizability as loc
from open3d_slam_advanced_rss_2024_public_amd.mapper import Mapper
from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection
from test_gpu_localizability_mapper import MAP_VOXEL, MIN_MOVE, NARROW_R, PKG, ROOT, SCAN_VOXEL, WIDE_R, hexes

pytestmark = pytest.mark.gpu

N_SWEEPS = 6
ITERS = 5
REF_PERIOD = 0.0            # every sweep renews the reference
CONSTRAIN = 3
_cache = {}


def scene():
    if "scene" not in _cache:
        _cache["scene"] = pref.door_sweeps(N_SWEEPS)
    return _cache["scene"]


def mirror_run(policy, params, partial=False):
    key = ("mirror", policy, partial)
    if key in _cache:
        return _cache[key]
    sc = scene()
    col = SubmapCollection(1.0e9, 5, 10 ** 12, 3, MAP_VOXEL, ("MaxRadius", WIDE_R))
    m = Mapper(ICP(IcpConfig(use_differential=False, max_iters=ITERS)), col, co.croppingVolumeFactory("MaxRadius", WIDE_R),
               co.croppingVolumeFactory("MaxRadius", NARROW_R), SCAN_VOXEL, REF_PERIOD, MIN_MOVE)
    m.set_calibration(np.eye(4))
    m.T = np.array(sc["poses"][0], np.float64)
    m.degeneracy_policy = policy
    m.localizability_params = params
    m.remap_min_category = 2
    m.degeneracy_partial = partial
    rows = []
    for k, (sp, sn) in enumerate(sc["scans"]):
        m.add_odometry_pose(sc["stamps"][k], sc["odom"][k])
        ok = m.add(sp, sn, sc["stamps"][k])
        pm, values = m.icp.degeneracy_partial_trace() if k else (np.zeros(0, np.int32), np.zeros((0, 6)))
        rows.append(dict(ok=int(ok), T=m.T.copy(), loc=m.last_localizability, masks=m.icp.degeneracy_trace().tolist() if k else [],
                         pmasks=pm.tolist(), values=values))
    _cache[key] = rows
    return rows


def thresholds():
    """From the first registration's analysis (Report: the chain itself is unconstrained)."""
    if "params" not in _cache:
        first = mirror_run("Report", loc.LocalizabilityParams(sum_all_min=1.0, sum_strong_min=1.0, sum_partial_min=1.0))[1]["loc"]
        k1, k2, k3 = pref.door_thresholds(dict(sum_all=first.sum_all, sum_strong=first.sum_strong))
        print(f"thresholds {k1:.2f} {k2:.2f} {k3:.2f} from sum_all {first.sum_all} sum_strong {first.sum_strong}")
        assert abs(first.evec[0][0]) > 0.999 and k3 < first.sum_strong[0] < k2
        _cache["params"] = loc.LocalizabilityParams(sum_all_min=k1, sum_strong_min=k2, sum_partial_min=k3)
    return _cache["params"]


def write_scene(path, params, partial):
    """partial None: the layout of tests/cpp/degeneracy_loop.cpp; else one more int64 behind iters."""
    sc = scene()
    cm = lambda T: np.ascontiguousarray(np.asarray(T, np.float64).T).tobytes()   # noqa: E731  column-major
    with open(path, "wb") as f:
        f.write(struct.pack("<4q", CONSTRAIN, 2, len(sc["scans"]), ITERS))
        if partial is not None:
            f.write(struct.pack("<q", int(partial)))
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
def compiled(tmp_path_factory):
    """partial (True, False, or None: the driver from before the flag) -> the driver's rows, each run made once."""
    bin_dir = tmp_path_factory.mktemp("degeneracy_partial_loop")
    exes = {}
    for name in ("degeneracy_partial_loop", "degeneracy_loop"):
        exes[name] = bin_dir / name
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
                               os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L" + PKG, "-lo3dslam_icp_hip", "-Wl,-rpath," + PKG, "-o", str(exes[name])])
    tmp = tmp_path_factory.mktemp("runs")
    done = {}

    def run(partial):
        if partial in done:
            return done[partial]
        path, out = tmp / f"door_{partial}.bin", tmp / f"door_{partial}.txt"
        write_scene(path, thresholds(), partial)
        exe = exes["degeneracy_loop" if partial is None else "degeneracy_partial_loop"]
        r = subprocess.run([str(exe), str(path), str(out)], capture_output=True, text=True, timeout=300)
        text = open(out).read() if os.path.exists(out) else ""
        assert r.returncode == 0, (r.stdout, r.stderr, text[-400:])
        rows = []
        for ln in text.strip().splitlines():
            w = ln.split()
            row = dict(ok=int(w[1]), iterations=int(w[4]), kept=int(w[5]), category=[int(v) for v in w[6:12]], T=hexes(w[12:28]).reshape(4, 4).T)
            if partial is None:                                    # ... prior(16) evec(18) n_masks masks
                n_masks = int(w[62])
                row["masks"] = [int(v) for v in w[63:63 + n_masks]]
            else:
                n_masks = int(w[28])
                row["masks"] = [int(v) for v in w[29:29 + n_masks]]
                at = 29 + n_masks
                n_p = int(w[at])
                row["pmasks"] = [int(v) for v in w[at + 1:at + 1 + n_p]]
                row["values"] = hexes(w[at + 1 + n_p:at + 1 + 7 * n_p]).reshape(n_p, 6)
            rows.append(row)
        assert len(rows) == N_SWEEPS
        done[partial] = rows
        return rows

    return run


def test_compiled_and_mirror_agree_with_the_flag_set(compiled):
    got, mirror, zero = compiled(True), mirror_run("Constrain", thresholds(), True), compiled(False)
    sc = scene()
    for k in range(N_SWEEPS):
        assert got[k]["ok"] == mirror[k]["ok"] and np.array_equal(got[k]["T"], mirror[k]["T"]), k
        if k == 0:
            continue
        assert got[k]["masks"] == mirror[k]["masks"] == [1] * ITERS, (k, got[k]["masks"])
        assert got[k]["pmasks"] == mirror[k]["pmasks"] and np.array_equal(got[k]["values"], mirror[k]["values"]), (k, got[k]["pmasks"])
        assert np.array_equal(mirror[k]["loc"].category, got[k]["category"]) and not got[k]["values"][:, 1:].any()
        if k == 1:      # against a map of one sweep no strong pair sees the axis under the prior: category 0, pinned, in both
            continue
        assert got[k]["pmasks"] == [1] * ITERS and got[k]["values"][:, 0].all() and got[k]["category"] == [1, 2, 2, 2, 2, 2], (k, got[k]["pmasks"])
        truth = sc["poses"][k][0, 3]
        print(f"sweep {k}: along the axis: valued {got[k]['T'][0, 3] - truth:+.4f} m  zero-constrained {zero[k]['T'][0, 3] - truth:+.4f} m  "
              f"values {got[k]['values'][:, 0]}")
        assert not np.array_equal(got[k]["T"], zero[k]["T"])


def test_with_the_flag_unset_constrain_is_what_it_was(compiled):
    got, before, mirror = compiled(False), compiled(None), mirror_run("Constrain", thresholds(), False)
    for k in range(N_SWEEPS):
        assert np.array_equal(got[k]["T"], before[k]["T"]) and np.array_equal(got[k]["T"], mirror[k]["T"]), k
        assert got[k]["masks"] == before[k]["masks"] == mirror[k]["masks"] and got[k]["category"] == before[k]["category"]
        assert got[k]["pmasks"] == [] and mirror[k]["pmasks"] == []
        if k:
            assert got[k]["masks"] == [1] * ITERS
