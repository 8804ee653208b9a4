"""The loop-closure refinement (o3d_icp_impl.h) at the size it runs at — 0.1-0.6 M source points against ~0.9 M target points —
against the NumPy restatement of Open3D v0.15.1 (tests/o3d_registration_ref.py, exact cKDTree neighbours), with each of the three
registration types.  At these sizes the launches change shape: k_o3d_corr's grid is capped at 2 048 blocks and strides, the later
passes' search is capped at 2 048 blocks, both far-search instantiations stride over their lists, the grid cell meets its clamps and
the 2^24-cell cap, the source's placement sort switches algorithm.  A wrong stride or bound there drops or double-counts points
without a fault; the suite's other registration tests never get that big.  test_launch_switches_are_crossed shows from the hooks
build's per-pass line that these cases cross every switch.  MI355X only.

Contract (as in test_gpu_registration_types.py): iterations, correspondence counts and fitness exact; pose and RMSE to 1e-9;
information matrix to 1e-9 x max(1, |I|max)."""
import os
import re
from dataclasses import dataclass

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import Submap
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import registration as reg
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn

from o3d_registration_ref import information_matrix as ref_information, registration_icp as ref_icp

pytestmark = pytest.mark.gpu

TYPES = ("PointToPlaneIcp", "PointToPointIcp", "GeneralizedIcp")
WORKERS = min(16, os.cpu_count() or 1)
SLAB_X, SLAB_HALF = 6.0, 3.0   # the target loses every point with |x - (t_x + 6)| < 3 m (map frame)


@dataclass
class Scene:
    src: np.ndarray    # sensor frame
    src_n: np.ndarray
    tgt: np.ndarray    # map frame
    tgt_n: np.ndarray
    T: np.ndarray      # ground truth source -> target


@pytest.fixture(scope="module")
def scene():
    """tools/closure_types.py's pair: one world, target 1 M points within 25 m (a 6 m slab cut out of it), source 600 k within
    22 m with 5 mm noise.  The source points over the slab lie inside the target's grid with no neighbour within 1 m."""
    world = syn.make_world(9000.0, seed=3)
    T = syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.3), np.array([1.0, 2.0, 1.5]))
    tp, tn = syn.make_scan(world, 1_000_000, T, radius=25.0, sigma=0.0, seed=4)
    tgt = tp.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    tgt_n = tn.astype(np.float64) @ T[:3, :3].T
    keep = np.abs(tgt[:, 0] - (T[0, 3] + SLAB_X)) >= SLAB_HALF
    sp, sn = syn.make_scan(world, 600_000, T, radius=22.0, sigma=0.005, seed=5)
    s = Scene(sp.astype(np.float64), sn.astype(np.float64), np.ascontiguousarray(tgt[keep]), np.ascontiguousarray(tgt_n[keep]), T)
    inside = np.abs((s.src @ T[:3, :3].T + T[:3, 3])[:, 0] - (T[0, 3] + SLAB_X)) < SLAB_HALF - 1.2
    assert inside.sum() > 40_000, inside.sum()   # > 32 768: the first passes' far list is longer than k_o3d_search_far<16>'s groups
    return s


_REF = {}


def cached(key, fn):
    """Restatement results shared between the tests of the module (the restatement is the slow side)."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def normals_kw(kind, src_n, tgt_n):
    if kind == "GeneralizedIcp":
        return {"source_normals": src_n, "target_normals": tgt_n}
    return {"target_normals": tgt_n} if kind == "PointToPlaneIcp" else {}


def gpu(kind, src, src_n, tgt, tgt_n, max_dist, init, max_iteration=30):
    if kind == "PointToPlaneIcp":
        return reg.registration_icp(src, tgt, tgt_n, max_dist, init, max_iteration=max_iteration)
    if kind == "PointToPointIcp":
        return reg.registration_icp_point_to_point(src, tgt, max_dist, init, max_iteration=max_iteration)
    return reg.registration_generalized_icp(src, tgt, max_dist, init, source_normals=src_n, target_normals=tgt_n, max_iteration=max_iteration)


def ref(kind, src, src_n, tgt, tgt_n, max_dist, init, max_iteration=30):
    return ref_icp(src, tgt, max_dist, init, kind, max_iteration=max_iteration, workers=WORKERS, bounded=True, **normals_kw(kind, src_n, tgt_n))


def same(g, o, tol=1e-9):
    assert g.iterations == o["iterations"] and g.correspondences == o["correspondences"], (g, o["iterations"], o["correspondences"])
    assert g.fitness == o["fitness"]
    assert abs(g.inlier_rmse - o["inlier_rmse"]) <= tol * max(1.0, o["inlier_rmse"])
    assert np.abs(g.transformation - o["transformation"]).max() <= tol


def bits(a, b):
    assert (a.iterations, a.correspondences, a.fitness, a.inlier_rmse) == (b.iterations, b.correspondences, b.fitness, b.inlier_rmse)
    assert np.array_equal(np.asarray(a.transformation), np.asarray(b.transformation))


def same_info(got, want, tol=1e-9):
    assert want[3, 3] > 0
    assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max()), np.abs(got - want).max()


def closure_source(scene, kind):
    """The 600 k source; for GICP 1 % of it not finite (NaN, +inf, -inf in turn): such points are never a correspondence."""
    src = scene.src.copy()
    if kind == "GeneralizedIcp":
        bad = np.random.default_rng(7).choice(len(src), len(src) // 100, replace=False)
        src[bad[0::3], 0] = np.nan
        src[bad[1::3], 1] = np.inf
        src[bad[2::3], 2] = -np.inf
    return src


def closure_init(scene):
    return syn.perturb_pose(scene.T, 0.1, 2.0, seed=5)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", TYPES)
def test_closure_size_matches_restatement(scene, kind):
    """600 k source points (k_o3d_corr: 2 048 blocks striding; Onesweep placement sort) against 0.9 M, 30 iterations at 1 m, then
    the information matrix at the result."""
    src, init = closure_source(scene, kind), closure_init(scene)
    g = gpu(kind, src, scene.src_n, scene.tgt, scene.tgt_n, 1.0, init)
    o = cached(("closure", kind), lambda: ref(kind, src, scene.src_n, scene.tgt, scene.tgt_n, 1.0, init))
    same(g, o)
    assert g.iterations >= 4 and 0.5 < g.fitness < 0.97, (g.iterations, g.fitness)   # converging, and the slab's points unmatched
    info = reg.get_information_matrix_from_point_clouds(src, scene.tgt, 1.0, g.transformation)
    same_info(info, ref_information(src, scene.tgt, 1.0, g.transformation, workers=WORKERS, bounded=True))


RHOS = (1, 3, 12, 48, 400)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", TYPES)
def test_cell_size_sweep_matches_restatement(scene, kind, hooks_lib, monkeypatch):
    """150 k against 0.9 M with the grid's points-per-cell target (O3S_O3D_RHO, hooks build) from 1 — the 2^24-cell cap grows the
    cell — to 400 — the cell meets its upper clamp, max_dist.  The sums follow the placement order, so the bits may differ between
    cell sizes; the correspondences and the iterations may not, and every size meets the contract."""
    src = scene.src[:150_000]
    init = closure_init(scene)
    o = cached(("sweep", kind), lambda: ref(kind, src, scene.src_n[:150_000], scene.tgt, scene.tgt_n, 1.0, init))
    for rho in RHOS:
        monkeypatch.setenv("O3S_O3D_RHO", str(rho))
        g = gpu(kind, src, scene.src_n[:150_000], scene.tgt, scene.tgt_n, 1.0, init)
        same(g, o)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("max_dist", [25.0, 0.02])
@pytest.mark.parametrize("kind", TYPES)
def test_radius_extremes_match_restatement(scene, kind, max_dist):
    """100 k against 0.9 M, 5 iterations at 25 m (r_cap far beyond the 64-lane row path; every point a correspondence) and at 2 cm
    (the cell at its lower clamp, ext / 1024, and the 2^24-cell cap; the pose is started 5 mm / 0.01 deg off so that some points
    find a neighbour)."""
    src, src_n = scene.src[:100_000], scene.src_n[:100_000]
    init = closure_init(scene) if max_dist > 1 else syn.perturb_pose(scene.T, 0.005, 0.01, seed=5)
    g = gpu(kind, src, src_n, scene.tgt, scene.tgt_n, max_dist, init, max_iteration=5)
    o = cached(("radius", kind, max_dist), lambda: ref(kind, src, src_n, scene.tgt, scene.tgt_n, max_dist, init, max_iteration=5))
    same(g, o)
    assert g.correspondences > 1000


def resident(src, src_n, tgt, tgt_n):
    big = co.croppingVolumeFactory("MaxRadius", 1.0e6)
    a, b = Submap(0.0, big), Submap(0.0, big)
    nudge = syn.make_T(None, np.array([0.25, 0.0, 0.0]))
    a.insertScan(src - np.array([0.25, 0.0, 0.0]), src_n, nudge)
    b.insertScan(tgt - np.array([0.25, 0.0, 0.0]), tgt_n, nudge)
    return a, b


@pytest.fixture(scope="module")
def resident_pair(scene):
    return resident(scene.src, scene.src_n, scene.tgt, scene.tgt_n)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", TYPES)
def test_resident_refinement_at_closure_size(scene, resident_pair, kind):
    """PlaceRecognition.cpp:97-150 on the 600 k / 0.9 M pair held as resident submaps (0.36 M / 0.52 M points in the overlap):
    bit-equal to the host path on the downloaded selections, within the contract of the restatement, information matrix included;
    then a batch of two refinements (two areas reserved first) is bit-equal to the single calls."""
    a, b = resident_pair
    sa, sna = a.getMapPointCloud()
    tb, tnb = b.getMapPointCloud()
    init = closure_init(scene)
    res, info, n_ov = reg.registration_icp_submaps_overlap(a, b, 1.0, init, 2.0, registration_type=kind)
    gs, gt = reg.compute_indices_of_overlapping_points(sa, tb, init, 2.0)
    assert n_ov == (len(gs), len(gt)) and len(gs) > 300_000, n_ov   # 0.36 M / 0.52 M selected at 2 m voxels
    h = gpu(kind, sa[gs], sna[gs], tb[gt], tnb[gt], 1.0, init)
    bits(res, h)
    o = ref(kind, sa[gs], sna[gs], tb[gt], tnb[gt], 1.0, init)
    same(res, o)
    same_info(info, ref_information(sa[gs], tb[gt], 1.0, res.transformation, workers=WORKERS, bounded=True))
    init2 = syn.perturb_pose(scene.T, 0.05, 1.0, seed=9)
    r2, i2, n2 = reg.registration_icp_submaps_overlap(a, b, 1.0, init2, 2.0, registration_type=kind)
    reg.reserve_n(len(a) + 16, len(b) + 16, 2)
    try:
        out = reg.registration_icp_submaps_overlap_batch([(a, b, init), (a, b, init2)], 1.0, 2.0, registration_type=kind)
    finally:
        reg.release()
    for (r, i, nov, st), (rs, infs, novs) in zip(out, [(res, info, n_ov), (r2, i2, n2)]):
        assert st == 0 and nov == novs
        bits(r, rs)
        assert np.array_equal(i, infs)


@pytest.mark.timeout(600)
def test_point_to_point_far_from_the_origin(scene):
    """Both clouds shifted by (4000, -3000, 120) m (300 k source points): the point-to-point sums are formed about a fixed shift c
    near the clouds; without it the centring in the host's umeyama would cancel digits.  Correspondences exact, rotation to 1e-9,
    translation to 1e-9 |shift|."""
    shift = np.array([4000.0, -3000.0, 120.0])
    S = syn.make_T(None, shift)
    src = scene.src[:300_000] + shift
    tgt = scene.tgt + shift
    init = S @ closure_init(scene) @ np.linalg.inv(S)
    g = reg.registration_icp_point_to_point(src, tgt, 1.0, init)
    o = ref("PointToPointIcp", src, None, tgt, None, 1.0, init)
    assert g.iterations == o["iterations"] and g.correspondences == o["correspondences"] and g.fitness == o["fitness"]
    assert np.abs(g.transformation[:3, :3] - o["transformation"][:3, :3]).max() <= 1e-9
    assert np.abs(g.transformation[:3, 3] - o["transformation"][:3, 3]).max() <= 1e-9 * np.linalg.norm(shift)
    assert g.correspondences > 200_000


PASS_LINE = re.compile(r"o3d pass: Ns=(\d+) searched=(\d+) far=(\d+) cell=(\S+) grid=(\d+)x(\d+)x(\d+) later_pass=(\d) pass=(\d+) r_cap=(\d+)")


def passes(text):
    out = []
    for m in PASS_LINE.finditer(text):
        ns, searched, far = int(m[1]), int(m[2]), int(m[3])
        cell = float(m[4])
        nx, ny, nz = int(m[5]), int(m[6]), int(m[7])
        out.append(dict(ns=ns, searched=searched, far=far, cell=cell, cells=nx * ny * nz, later=int(m[8]), pass_no=int(m[9]),
                        r_cap=int(m[10])))
    return out


@pytest.mark.timeout(900)
def test_launch_switches_are_crossed(scene, hooks_lib, monkeypatch, capfd):
    """The hooks build's per-pass line (O3S_O3D_DBG=1; O3S_O3D_KDBG=64: every later pass searches the whole list) for three of the
    cases above shows each launch switch crossed; with the line on the results are bit-identical to those with it off, and within
    the contract of the restatement."""
    init = closure_init(scene)
    cases = {  # name: (kind, source, source normals, max_dist, max_iteration, rho, restatement key)
        "closure": ("PointToPlaneIcp", scene.src, scene.src_n, 1.0, 30, None, ("closure", "PointToPlaneIcp")),
        "radius25": ("PointToPointIcp", scene.src[:100_000], scene.src_n[:100_000], 25.0, 5, None, ("radius", "PointToPointIcp", 25.0)),
        "rho1": ("GeneralizedIcp", scene.src[:150_000], scene.src_n[:150_000], 1.0, 30, 1, ("sweep", "GeneralizedIcp")),
    }
    monkeypatch.setenv("O3S_O3D_KDBG", "64")
    seen = {}
    for name, (kind, src, src_n, max_dist, max_iter, rho, key) in cases.items():
        if rho is not None:
            monkeypatch.setenv("O3S_O3D_RHO", str(rho))
        else:
            monkeypatch.delenv("O3S_O3D_RHO", raising=False)
        monkeypatch.delenv("O3S_O3D_DBG", raising=False)
        quiet = gpu(kind, src, src_n, scene.tgt, scene.tgt_n, max_dist, init, max_iter)
        capfd.readouterr()
        monkeypatch.setenv("O3S_O3D_DBG", "1")
        loud = gpu(kind, src, src_n, scene.tgt, scene.tgt_n, max_dist, init, max_iter)
        p = passes(capfd.readouterr().err)
        bits(loud, quiet)
        same(loud, cached(key, lambda: ref(kind, src, src_n, scene.tgt, scene.tgt_n, max_dist, init, max_iter)))
        assert len(p) == loud.iterations + 1 and [q["pass_no"] for q in p] == list(range(len(p))), [q["pass_no"] for q in p]
        for q in p:
            assert q["ns"] == len(src) and q["later"] == (q["pass_no"] > 0)
            assert q["r_cap"] == int(np.ceil(1.1 * max_dist / q["cell"]) + 1.0)   # o3d_corr_pass's reach, from the printed cell
        seen[name] = p
    summary = {n: [(q["pass_no"], q["searched"], q["far"], round(q["cell"], 4), q["cells"], q["r_cap"]) for q in p] for n, p in seen.items()}
    allp = [q for p in seen.values() for q in p]
    # k_o3d_corr: more than 2 048 blocks' worth of source points, so its grid strides
    assert any(q["ns"] > 524_288 for q in allp), summary
    # k_o3d_search in a later pass: the list is longer than 2 048 blocks x 64 points
    assert any(q["later"] and q["searched"] > 131_072 for q in allp), summary
    # k_o3d_search_far<16> (passes 0-2): more far points than its 32 768 groups; <64> (later passes): more than its 2 048
    assert any(q["pass_no"] < 3 and q["far"] > 32_768 for q in allp), summary
    assert any(q["pass_no"] >= 3 and q["far"] > 2_048 for q in allp), summary
    # the far search's reach: the 64-lane row path holds every shell (r_cap <= 7), and a case whose reach exceeds what 64 lanes'
    # rows hold (r_cap >= 32) with points on the far list under both instantiations
    assert any(q["r_cap"] <= 7 for q in allp), summary
    assert any(all(q["r_cap"] >= 32 for q in p) and any(q["far"] > 0 and q["pass_no"] < 3 for q in p)
               and any(q["far"] > 0 and q["pass_no"] >= 3 for q in p) for p in seen.values()), summary
    # the 2^24-cell cap grew the cell: the grid lands within a factor 1.26^3 ~ 2 below the cap
    assert any((1 << 23) < q["cells"] <= (1 << 24) for q in allp), summary
    print(summary)
