"""The pose covariance of the scan-to-map ICP (PointToPlaneWithCovErrorMinimizer): the numpy restatement against itself, and the
configuration surface.  No GPU.

Tolerance of every comparison of two evaluations of the contract (here and in tests/test_gpu_icp_covariance.py):
    |delta_ij| / sqrt(c_ii c_jj) <= 256 * 2^-52 * cond_2(H_ref)
(icp_covariance_ref.bound).  The fixtures are room-like pairs with normals spread over three axes; each asserts cond_2(H) < 1e6, so
the bound can never grow loose enough to hide an error.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import icp_covariance_ref as cref
from open3d_slam_advanced_rss_2024_public_amd import _lib, icp

SIZES = [6, 65, 513, 5000, 140000]
SIGMA = 0.01


@functools.lru_cache(maxsize=None)
def fixture(K, deg=3.0):
    p, q, n = cref.room_pairs(K, seed=K % 97)
    T = cref.rot_step(deg) if deg else cref.rot_step(0.0, t=None)
    cov, H = cref.covariance(p, q, n, T, SIGMA, "fsum")
    cond = float(np.linalg.cond(H, 2))
    assert cond < 1e6, cond
    assert np.isfinite(cov).all()
    for a in (p, q, n, cov, H):
        a.setflags(write=False)
    return p, q, n, T, cov, H


@pytest.mark.parametrize("K", SIZES[:4])
def test_two_transcriptions_agree(K):
    """The explicit 6 x 2K d2J_dZdX matrix and its product, as the source writes it, against the accumulated sum (u u^T + v v^T)."""
    p, q, n, T, cov, H = fixture(K)
    other = cref.covariance_matrix_form(p, q, n, T, SIGMA)
    d = cref.rel_distance(other, cov)
    print(f"K {K}: cond {np.linalg.cond(H, 2):.1f} bound {cref.bound(H):.3e} distance {d:.3e}")
    assert d <= cref.bound(H)


@pytest.mark.parametrize("K", SIZES)
def test_summation_orders_agree(K):
    p, q, n, T, cov, H = fixture(K)
    for mode in ("seq", "pairwise"):
        c, _ = cref.covariance(p, q, n, T, SIGMA, mode)
        d = cref.rel_distance(c, cov)
        print(f"K {K} {mode}: bound {cref.bound(H):.3e} distance {d:.3e}")
        assert d <= cref.bound(H)


@pytest.mark.parametrize("K", SIZES[:4])
def test_symmetric_positive_semidefinite(K):
    _, _, _, _, cov, H = fixture(K)
    assert cref.rel_distance(cov.T, cov) <= cref.bound(H)
    scale = np.sqrt(np.diag(cov))
    w = np.linalg.eigvalsh((cov + cov.T) / 2 / np.outer(scale, scale))
    assert w.min() >= -cref.bound(H), w


@pytest.mark.parametrize("K", [65, 5000])
def test_scales_with_sigma_squared(K):
    p, q, n, T, cov, H = fixture(K)
    c2, _ = cref.covariance(p, q, n, T, 0.02, "fsum")
    ratio = cref.sigma2(0.02) / cref.sigma2(SIGMA)
    assert cref.rel_distance(c2 / ratio, cov) <= cref.bound(H)
    assert abs(ratio - 4.0) < 1e-6   # fl32(sigma * sigma), promoted


@pytest.mark.parametrize("K", [65, 513, 5000])
def test_permuting_the_pairs_stays_inside_the_bound(K):
    p, q, n, T, cov, H = fixture(K)
    perm = np.random.default_rng(K).permutation(K)
    c, _ = cref.covariance(p[perm], q[perm], n[perm], T, SIGMA, "seq")
    assert cref.rel_distance(c, cov) <= cref.bound(H)


def test_identity_step():
    p, q, n, T, cov, H = fixture(513, 0.0)
    assert cref.angles(T)[:3] == (0.0, 0.0, 0.0)
    assert cref.rel_distance(cref.covariance_matrix_form(p, q, n, T, SIGMA), cov) <= cref.bound(H)


@pytest.mark.parametrize("K", SIZES[:4])
def test_fp32_variant_is_finite(K):
    """Sequential fp32 sums and an fp32 inverse, the reference's number format: its distance to the contract is recorded (DESIGN),
    not asserted."""
    p, q, n, T, cov, H = fixture(K)
    c = cref.covariance_fp32(p, q, n, T, SIGMA)
    assert np.isfinite(c).all()
    print(f"K {K}: fp32 variant at relative distance {cref.rel_distance(c, cov):.3e} of the contract (bound {cref.bound(H):.3e})")


def test_singular_hessian_gives_nan():
    p, q, n = cref.room_pairs(65)
    n = np.zeros_like(n)
    n[:, 2] = 1.0    # one wall only: H has no rank in x, y
    cov, _ = cref.covariance(p * np.float32([1, 1, 0]), q, n, cref.rot_step(0.0, t=None), SIGMA)
    assert np.isnan(cov).all()   # a zero pivot: 36 NaN, as the library reports it


YAML = """
matcher:
  KDTreeMatcher:
    knn: 1
    maxDist: 0.5
    epsilon: 0.01
outlierFilters:
  - TrimmedDistOutlierFilter:
     ratio: 0.90
  - SurfaceNormalOutlierFilter:
     maxAngle: 1.57
errorMinimizer:
  PointToPlaneWithCovErrorMinimizer:
    sensorStdDev: 0.02%s
transformationCheckers:
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.001
      minDiffTransErr: 0.01
      smoothLength: 3
  - CounterTransformationChecker:
      maxIterationCount: 15
"""


def test_yaml_accepts_the_covariance_minimiser():
    cfg = icp.IcpConfig.from_yaml(YAML % "")
    assert cfg == icp.IcpConfig(error_minimizer="PointToPlaneWithCovErrorMinimizer", sensor_std_dev=0.02)
    c = cfg.to_c()
    assert c.error_minimizer == 1 and c.sensor_std_dev == np.float32(0.02)
    plain = icp.IcpConfig.from_yaml((YAML % "").replace("PointToPlaneWithCovErrorMinimizer:\n    sensorStdDev: 0.02", "PointToPlaneErrorMinimizer"))
    assert plain == icp.IcpConfig() and plain.to_c().error_minimizer == 0
    assert icp.IcpConfig.from_yaml("errorMinimizer:\n  PointToPlaneWithCovErrorMinimizer\n").sensor_std_dev == 0.01


def test_yaml_refuses_force2d():
    with pytest.raises(icp.InvalidModuleType):
        icp.IcpConfig.from_yaml(YAML % "\n    force2D: 1")
    with pytest.raises(icp.InvalidModuleType):
        icp.IcpConfig.from_yaml("errorMinimizer:\n  PointToPlaneErrorMinimizer:\n    force2D: 1\n")
    with pytest.raises(icp.InvalidModuleType):
        icp.IcpConfig.from_yaml("errorMinimizer:\n  PointToPointWithCovErrorMinimizer\n")


def test_defaults_round_trip_through_to_c():
    c = _lib.IcpConfigC()
    _lib.lib().o3s_icp_default_config(C.byref(c))
    assert c.error_minimizer == 0 and c.sensor_std_dev == np.float32(0.01) and list(c.reserved) == [0, 0]
    py = icp.IcpConfig().to_c()
    assert (py.error_minimizer, py.sensor_std_dev) == (c.error_minimizer, c.sensor_std_dev)
    assert C.sizeof(_lib.IcpConfigC) == 20 * 4   # the struct keeps its size: the two fields took two of the four reserved words
    with pytest.raises(icp.InvalidModuleType):
        icp.IcpConfig(error_minimizer="PointToPointErrorMinimizer").to_c()
