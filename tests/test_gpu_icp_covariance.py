"""The pose covariance of the scan-to-map ICP (PointToPlaneWithCovErrorMinimizer, include/o3s_icp.h "pose covariance") on the GPU
against the numpy restatement (tests/icp_covariance_ref.py).

Tolerance of every comparison with the restatement: |delta_ij| / sqrt(c_ii c_jj) <= 256 * 2^-52 * cond_2(H_ref)
(icp_covariance_ref.bound; cond_2(H_ref) < 1e6 is asserted wherever it is used).  Comparisons between two ways of issuing the
same registration are bit for bit.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import icp_covariance_ref as cref
from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig, _lib
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn
from open3d_slam_advanced_rss_2024_public_amd.icp import compute_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")
COV = "PointToPlaneWithCovErrorMinimizer"
SIGMA = 0.01


def kernel_constant(name, header):
    """A `constexpr int` of the kernels as built (csrc/)."""
    text = open(os.path.join(PKG, "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


ONE_BLOCK = kernel_constant("kBlock", "icp_kernels.h") * kernel_constant("kNePPT", "icp_kernels.h")   # pairs one block of k_cov takes per trip
ONE_GENERATION = ONE_BLOCK * kernel_constant("kMaxPartialBlocks", "icp_types.h")                       # ... and its largest grid
SIZES = [6, 63, 64, 65, ONE_BLOCK - 1, ONE_BLOCK, ONE_BLOCK + 1, ONE_GENERATION + 1, 131073]


def check(cov, p, q, n, T, sigma=SIGMA, mode="fsum"):
    """cov against the restatement on the same centred pairs and step; returns (distance, bound)."""
    ref, H = cref.covariance(p, q, n, T, sigma, mode)
    cond = float(np.linalg.cond(H, 2))
    assert cond < 1e6, cond
    d = cref.rel_distance(cov, ref)
    print(f"K {len(p)}: cond {cond:.1f} bound {cref.bound(H):.3e} distance {d:.3e}")
    assert np.isfinite(cov).all() and d <= cref.bound(H), (d, cref.bound(H))
    return d, cref.bound(H)


@pytest.fixture(scope="module")
def plain_handle():
    return ICP(IcpConfig())


@functools.lru_cache(maxsize=None)
def pair():
    return syn.make_scan_pair(10_000, 30_000, 0.1)


def run(cfg, sp=None, scan=None, normals=None):
    sp = sp or pair()
    g = ICP(cfg)
    assert g.init_reference(sp.map_xyz, sp.map_normals)
    T = g.compute(sp.scan_xyz if scan is None else scan, sp.scan_normals if normals is None else normals, sp.T_init)
    return g, T


def check_own_elements(g):
    """get_covariance() of the handle against the restatement on the handle's own error elements and last step."""
    p, q, n, idx = g.error_elements()
    assert len(p) == g.stats.trace_kept[-1] == g.stats.kept_pairs
    return check(g.get_covariance(), p, q, n, g.last_step(), g.config.sensor_std_dev, "fsum" if len(p) <= 20000 else "pairwise")


# ---- 1. kernel arithmetic -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,deg", [(K, 3.0) for K in SIZES] + [(ONE_BLOCK + 1, 0.0)])
def test_estimate_covariance_matches_the_restatement(plain_handle, K, deg):
    p, q, n = cref.room_pairs(K, seed=K % 97)
    T = cref.rot_step(deg) if deg else cref.rot_step(0.0, t=None)
    cov = plain_handle.estimate_covariance(p, q, n, T, SIGMA)
    check(cov, p, q, n, T, SIGMA, "fsum" if K <= 20000 else "pairwise")
    assert np.array_equal(cov, plain_handle.estimate_covariance(p, q, n, T, SIGMA))   # the order of the sums is fixed
    c2 = plain_handle.estimate_covariance(p, q, n, T, 0.02)
    # sigma2 multiplies last: one rounding each for the two products, the ratio and the division
    assert cref.rel_distance(c2 / (cref.sigma2(0.02) / cref.sigma2(SIGMA)), cov) <= 4 * 2.0 ** -52


def test_estimate_covariance_refuses_no_pairs(plain_handle):
    z = np.zeros((0, 3), np.float32)
    with pytest.raises(Exception) as e:
        plain_handle.estimate_covariance(z, z, z, np.eye(4), SIGMA)
    assert f"[{_lib.ERR_NO_POINTS}]" in str(e.value)


def test_a_singular_hessian_gives_nan_and_ok(plain_handle):
    p, q, n = cref.room_pairs(65)
    n = np.zeros_like(n)
    n[:, 2] = 1.0   # one wall: H has no rank in x, y
    cov = plain_handle.estimate_covariance(p * np.float32([1, 1, 0]), q, n, np.eye(4), SIGMA)
    assert np.isnan(cov).all()


# ---- 2. fused path, C1-scale pair -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused():
    a, Ta = run(IcpConfig())
    b, Tb = run(IcpConfig(error_minimizer=COV, sensor_std_dev=SIGMA))
    return a, Ta, b, Tb


def test_configuring_the_covariance_changes_nothing_else(fused):
    a, Ta, b, Tb = fused
    assert np.array_equal(Ta, Tb)
    for f in ("trace_T", "trace_limit", "trace_kept"):
        assert np.array_equal(getattr(a.stats, f), getattr(b.stats, f), equal_nan=True), f
    for f in ("iterations", "max_iters_reached", "kept_pairs", "matched_pairs", "point_used_ratio", "weighted_point_used_ratio", "last_trim_limit",
              "candidates_examined", "cells_probed"):
        assert getattr(a.stats, f) == getattr(b.stats, f), f
    assert np.array_equal(a.get_covariance(), np.zeros((6, 6)))   # the base class's getCovariance
    for x, y in zip(a.error_elements(), b.error_elements()):        # the elements do not depend on the minimiser
        assert np.array_equal(x, y)
    assert np.array_equal(a.last_step(), b.last_step())


def test_fused_covariance_matches_the_restatement_on_the_error_elements(fused):
    b = fused[2]
    cov = b.get_covariance()
    _, bound = check_own_elements(b)
    assert cref.rel_distance(cov.T, cov) <= bound and np.all(np.diag(cov) > 0)
    # the module-level entry on the same pairs: the same kernel, the pairs in other blocks (compacted), so another order of the sums
    p, q, n, _ = b.error_elements()
    assert cref.rel_distance(b.estimate_covariance(p, q, n, b.last_step()), cov) <= bound


def test_error_elements_agree_with_the_oracle(fused):
    """The last iteration rebuilt with the oracle's modules: the reading at the previous trace pose, its closest points, the outlier
    weights, the means of the kept pairs.  Same pairs apart from at most those at the trim limit; coordinates within 1e-5 m."""
    b = fused[2]
    sp = pair()
    p, q, n, idx = b.error_elements()
    o = orc.OracleIcp(orc.OracleConfig(), threads=8)
    assert o.init_reference(sp.map_xyz, sp.map_normals) == orc.OK
    mean = o.reference_mean()
    assert np.array_equal(mean, b.reference_mean())
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = -mean
    T0 = (T0.astype(np.float64) @ sp.T_init.astype(np.float32).astype(np.float64)).astype(np.float32)
    r0, n0 = orc.rigid_transform(T0, sp.scan_xyz, sp.scan_normals)
    it = b.stats.iterations
    T_prev = b.stats.trace_T[it - 2] if it >= 2 else np.eye(4, dtype=np.float32)
    S, Sn = orc.rigid_transform(T_prev, r0, n0)
    ids, d2 = o.find_closests(S)
    w = o.outlier_weights(Sn, ids, d2)
    kept = np.flatnonzero(w > 0)
    odd = np.setxor1d(kept, idx)
    limit = b.stats.trace_limit[-1]
    print(f"kept {len(kept)} / {len(idx)}; pairs in one set only: {len(odd)}")
    assert len(odd) <= 8 and np.all(np.abs(d2[odd] - limit) <= 1e-5 * limit)
    assert len(np.unique(idx)) == len(idx)
    common = np.intersect1d(kept, idx)
    ref_c = sp.map_xyz.astype(np.float32) - mean
    mp = S[kept].astype(np.float64).mean(0)
    mq = ref_c[ids[kept]].astype(np.float64).mean(0)
    pos = {int(v): k for k, v in enumerate(idx)}
    rows = np.array([pos[int(v)] for v in common])
    assert np.abs(p[rows] - (S[common] - mp)).max() <= 1e-5
    assert np.abs(q[rows] - (ref_c[ids[common]] - mq)).max() <= 1e-5
    assert np.abs(n[rows] - sp.map_normals.astype(np.float32)[ids[common]]).max() <= 1e-6


# ---- 3. independence of issue ---------------------------------------------------------------------------------------------------------
def test_covariance_bits_do_not_depend_on_how_the_chain_is_issued(fused):
    sp = pair()
    want_T, want = fused[3], fused[2].get_covariance()
    g = ICP(IcpConfig(error_minimizer=COV, sensor_std_dev=SIGMA))
    assert g.init_reference(sp.map_xyz, sp.map_normals)
    g.set_reading(sp.scan_xyz, sp.scan_normals)
    for issued in ("eager", "captured", "replayed"):
        T = g.compute_resident(sp.T_init)
        assert g.host_split_ex()["issued"] == issued
        assert np.array_equal(T, want_T) and np.array_equal(g.get_covariance(), want), issued
    g.compute_resident_launch(sp.T_init)
    T = g.compute_resident_finish()
    assert np.array_equal(T, want_T) and np.array_equal(g.get_covariance(), want)


def test_batch_equals_sequential_calls():
    pairs = [syn.make_scan_pair(3000 + 700 * k, 20_000, 0.1, seed=40 + k) for k in range(3)]
    cfg = IcpConfig(error_minimizer=COV, sensor_std_dev=SIGMA)
    seq, bat = [], []
    for sp in pairs:
        for lst in (seq, bat):
            g = ICP(cfg)
            assert g.init_reference(sp.map_xyz, sp.map_normals)
            g.set_reading(sp.scan_xyz, sp.scan_normals)
            lst.append(g)
    Ts = [g.compute_resident(sp.T_init) for g, sp in zip(seq, pairs)]
    poses, codes, _ = compute_batch(bat, [sp.T_init for sp in pairs])
    assert codes == [0, 0, 0]
    for k in range(3):
        assert np.array_equal(poses[k], Ts[k])
        assert np.array_equal(bat[k].get_covariance(), seq[k].get_covariance()) and np.isfinite(seq[k].get_covariance()).all()


def test_query_order_moves_the_covariance_by_no_more_than_the_bound(fused):
    b = fused[2]
    u, Tu = run(IcpConfig(error_minimizer=COV, sensor_std_dev=SIGMA, sort_queries=False))
    p, q, n, _ = b.error_elements()
    _, H = cref.covariance(p, q, n, b.last_step(), SIGMA, "pairwise")
    assert cref.rel_distance(u.get_covariance(), b.get_covariance()) <= cref.bound(H)
    check_own_elements(u)


# ---- 4. where the chain ends ----------------------------------------------------------------------------------------------------------
def test_one_iteration_starts_from_the_identity():
    g, _ = run(IcpConfig(error_minimizer=COV, use_differential=False, max_iters=1))
    assert g.stats.iterations == 1
    check_own_elements(g)


def test_counter_stop_in_the_middle_of_a_graph_chunk():
    sp = pair()
    g = ICP(IcpConfig(error_minimizer=COV, min_diff_rot=0.0, min_diff_trans=0.0, max_iters=8))   # chunks of five: 8 ends inside the second
    assert g.init_reference(sp.map_xyz, sp.map_normals)
    g.set_reading(sp.scan_xyz, sp.scan_normals)
    covs = []
    for issued in ("eager", "captured", "replayed"):
        g.compute_resident(sp.T_init)
        assert g.host_split_ex()["issued"] == issued and g.stats.iterations == 8 and g.stats.max_iters_reached
        covs.append(g.get_covariance())
    check_own_elements(g)
    assert np.array_equal(covs[0], covs[1]) and np.array_equal(covs[0], covs[2])


def test_differential_stop(fused):
    b = fused[2]
    assert 1 < b.stats.iterations < 15 and not b.stats.max_iters_reached
    check_own_elements(b)


def test_a_reading_of_131073_points():
    """The two-kernel chain (more blocks than the fused selection + normal-equation kernel takes)."""
    sp = pair()
    rng = np.random.default_rng(5)
    reps = 131073 // len(sp.scan_xyz) + 1
    scan = (np.tile(sp.scan_xyz, (reps, 1))[:131073] + rng.normal(0, 0.002, (131073, 3))).astype(np.float32)
    normals = np.tile(sp.scan_normals, (reps, 1))[:131073]
    g, _ = run(IcpConfig(error_minimizer=COV), scan=scan, normals=normals)
    check_own_elements(g)


# ---- 5. statuses ------------------------------------------------------------------------------------------------------------------------
def test_statuses():
    sp = pair()
    L = _lib.lib()
    buf = np.zeros(36)
    dp = buf.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))
    g = ICP(IcpConfig(error_minimizer=COV))
    assert L.o3s_icp_get_covariance(g._h, dp) == _lib.ERR_NOT_INITIALIZED
    assert g.error_elements()[0].shape == (0, 3)
    assert g.init_reference(sp.map_xyz, sp.map_normals)
    assert L.o3s_icp_get_covariance(g._h, dp) == _lib.ERR_NOT_INITIALIZED
    g.compute(sp.scan_xyz, sp.scan_normals, sp.T_init)
    assert L.o3s_icp_get_covariance(g._h, dp) == _lib.OK and np.isfinite(buf).all() and buf.any()
    with pytest.raises(Exception):   # a reading far outside maxDist: no matches, an ordinary error return
        g.compute(sp.scan_xyz + np.float32(50.0), sp.scan_normals, sp.T_init)
    assert L.o3s_icp_get_covariance(g._h, dp) == _lib.ERR_NOT_INITIALIZED
    with pytest.raises(RuntimeError):
        g.get_covariance()
    with pytest.raises(ValueError) as e:   # BAD_CONFIG: the sharded mode
        g.shard_configure(len(sp.scan_xyz), 0, 1, lambda *a: None)
    assert f"[{_lib.ERR_BAD_CONFIG}]" in str(e.value) and "sharded" in str(e.value)
    g.compute(sp.scan_xyz, sp.scan_normals, sp.T_init)   # ... and the handle is as it was
    assert L.o3s_icp_get_covariance(g._h, dp) == _lib.OK
    for bad in (dict(sensor_std_dev=-1.0), dict(sensor_std_dev=float("nan"))):
        with pytest.raises(ValueError):
            ICP(IcpConfig(error_minimizer=COV, **bad))
    c = IcpConfig().to_c()
    c.error_minimizer = 2
    h = _lib.C.c_void_p()
    assert L.o3s_icp_create(_lib.C.byref(c), 0, _lib.C.byref(h)) == _lib.ERR_BAD_CONFIG


# ---- 6. C++ shim and the mapper --------------------------------------------------------------------------------------------------------
def test_cpp_shim_returns_the_same_covariance(tmp_path):
    from open3d_slam_advanced_rss_2024_public_amd.icp import as_xyzw

    exe = tmp_path / "cov_roundtrip"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKG, "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "cov_roundtrip.cpp"), "-L" + PKG, "-lo3dslam_icp_hip", "-Wl,-rpath," + PKG,
                           "-o", str(exe)])
    sp = syn.make_scan_pair(6000, 50000, 0.1, seed=8)
    files = {}
    for name, arr in (("ref", as_xyzw(sp.map_xyz)), ("refn", sp.map_normals.astype(np.float32)), ("scan", as_xyzw(sp.scan_xyz)),
                      ("scann", sp.scan_normals.astype(np.float32)), ("T0", np.ascontiguousarray(sp.T_init.astype(np.float32).T))):
        files[name] = str(tmp_path / f"{name}.f32")
        np.ascontiguousarray(arr, np.float32).tofile(files[name])
    out = subprocess.run([str(exe), files["ref"], files["refn"], str(sp.map_xyz.shape[0]), files["scan"], files["scann"],
                          str(sp.scan_xyz.shape[0]), files["T0"], "0.02"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    assert lines["none"] == "runtime_error"
    cov_cpp = np.array([int(w, 16) for w in lines["cov"].split()], np.uint64).view(np.float64).reshape(6, 6).T
    g, T = run(IcpConfig(error_minimizer=COV, sensor_std_dev=0.02), sp=sp)
    assert np.array_equal(np.array(lines["T"].split(), np.float32).reshape(4, 4).T, T)
    assert np.array_equal(cov_cpp, g.get_covariance()) and np.isfinite(cov_cpp).all()


def test_the_mapper_keeps_the_covariance_of_its_latest_registration():
    import odometry_ref as orf
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
    from open3d_slam_advanced_rss_2024_public_amd.mapper import Mapper
    from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection

    col = SubmapCollection(1.0e9, 5, 10 ** 12, 3, 0.2, ("MaxRadius", 30.0))
    m = Mapper(ICP(IcpConfig(error_minimizer=COV)), col, co.croppingVolumeFactory("MaxRadius", 30.0), co.croppingVolumeFactory("MaxRadius", 20.0),
               0.2, 0.25, 0.0)
    m.set_calibration(np.eye(4))
    assert np.isnan(m.last_covariance).all()
    for k in range(5):
        p, n = orf.sweep(k)
        assert m.add(p, n, 0.1 * k)
        if k == 0:   # the first sweep founds the map: nothing was registered
            assert np.isnan(m.last_covariance).all()
            continue
        assert m.flags[2] == 0
        c = m.last_covariance
        assert c.shape == (6, 6) and np.isfinite(c).all() and np.all(np.diag(c) > 0)
        assert np.array_equal(c, m.icp.get_covariance())
        _, bound = check_own_elements(m.icp)
        assert cref.rel_distance(c.T, c) <= bound
