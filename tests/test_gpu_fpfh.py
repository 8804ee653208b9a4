"""FPFH features on host buffers (include/o3s_cloud_ops.h o3s_compute_fpfh; csrc/fpfh_dev.h) against the numpy restatement of
tests/fpfh_ref.py.  MI355X only.  Staged, so that one stage's ambiguity cannot hide the next one's error:

  1. neighbour lists bit-equal to the reference for every max_nn / radius of the grid below;
  2. SPFH bit-equal on every point outside the reference's rounding-sensitive set;
  3. FPFH bit-equal to the reference's second stage applied to the DEVICE's own SPFH and lists — every point, no exception;
  4. end to end: FPFH bit-equal on every point that neither is sensitive nor lists a sensitive point;
  5. degenerate inputs and run-to-run identity.

The sensitive set is a cap, not a measurement: at most 1 % of the points, and stage 4 leaves out at most 25 %, both asserted on
the reference's own output before anything is compared."""
import numpy as np
import pytest

import fpfh_ref as fr
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

pytestmark = pytest.mark.gpu

_DEV = {}


def device(noise, radius, knn):
    key = (noise, radius, knn)
    if key not in _DEV:
        p, n, _ = fr.sparse_cloud(noise=noise)
        _DEV[key] = co.computeFPFHFeature(p, n, radius, knn, want_spfh=True, want_neighbours=True)
    return _DEV[key]


_REF = {}


def reference(noise, radius, knn):
    key = (noise, radius, knn)
    if key not in _REF:
        p, n, _ = fr.sparse_cloud(noise=noise)
        _REF[key] = fr.compute_fpfh(p, n, radius, knn)
    return _REF[key]


@pytest.mark.parametrize("radius", [0.3, 2.5, 50.0])
@pytest.mark.parametrize("knn", [1, 2, 33, 100, 128])
def test_stage1_neighbour_lists(radius, knn):
    for noise in (0.01, 0.0):
        p, n, _ = fr.sparse_cloud(noise=noise)
        _, nn = co.computeFPFHFeature(p, n, radius, knn, want_neighbours=True)
        ref = fr.normals_ref.neighbour_lists(p, radius, knn)
        assert nn.shape == ref.shape and np.array_equal(nn, ref), (noise, int((nn != ref).any(axis=1).sum()))


@pytest.mark.parametrize("radius,knn", [(2.5, 100), (1.5, 33)])
def test_stage2_spfh(radius, knn):
    r = reference(0.01, radius, knn)
    print(f"sensitive {int(r.sensitive.sum())} of {len(r.sensitive)}")
    assert r.sensitive.mean() <= 0.01
    _, spfh, nn = device(0.01, radius, knn)
    assert np.array_equal(nn, r.nn)
    keep = ~r.sensitive
    assert np.array_equal(spfh[keep], r.spfh[keep])


@pytest.mark.parametrize("noise,radius,knn", [(0.01, 2.5, 100), (0.0, 2.5, 100), (0.01, 1.5, 33), (0.0, 50.0, 128)])
def test_stage3_fpfh_from_the_devices_own_spfh(noise, radius, knn):
    p, _, _ = fr.sparse_cloud(noise=noise)
    f, spfh, nn = device(noise, radius, knn)
    want = fr.fpfh_from_spfh(spfh, nn, fr.list_d2(p, nn))
    assert np.array_equal(f, want)


@pytest.mark.parametrize("radius,knn", [(2.5, 100), (1.5, 33)])
def test_stage4_end_to_end(radius, knn):
    r = reference(0.01, radius, knn)
    print(f"sensitive {int(r.sensitive.sum())}, left out {int(r.tainted.sum())} of {len(r.tainted)}")
    assert r.sensitive.mean() <= 0.01 and r.tainted.mean() <= 0.25
    f, _, _ = device(0.01, radius, knn)
    keep = ~r.tainted
    assert np.array_equal(f[keep], r.fpfh[keep])
    ok = (r.nn >= 0).sum(axis=1) > 1
    assert np.abs(f[ok].reshape(-1, 3, 11).sum(axis=2) - 200.0).max() <= 1e-9


def test_stage5_degenerate_inputs():
    z = np.array([[0.0, 0.0, 1.0]])
    # N = 0, 1, 2
    f = co.computeFPFHFeature(np.zeros((0, 3)), np.zeros((0, 3)), 2.5, 100)
    assert f.shape == (0, 33)
    f, s, nn = co.computeFPFHFeature(np.array([[1.0, 2.0, 3.0]]), z, 2.5, 100, want_spfh=True, want_neighbours=True)
    assert not f.any() and not s.any() and nn[0, 0] == 0 and (nn[0, 1:] == -1).all()
    p2 = np.array([[0.0, 0.0, 0.0], [0.0, 3.0, 4.0]])
    n2 = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    f, s, nn = co.computeFPFHFeature(p2, n2, 10.0, 5, want_spfh=True, want_neighbours=True)
    r = fr.compute_fpfh(p2, n2, 10.0, 5)
    assert np.array_equal(nn, r.nn) and np.array_equal(s, r.spfh) and np.array_equal(f, r.fpfh)
    assert s[0, 8] == 100.0 and s[0, 16] == 100.0 and s[0, 31] == 100.0 and f[0].sum() == 600.0
    # duplicates, a point alone in its ball, NaN normals
    p, n, _ = fr.sparse_cloud(noise=0.01)
    p, n = p[:3000].copy(), n[:3000].copy()
    p[100:110] = p[100]                       # ten copies of one point
    p[200] = p[200] + np.array([0.0, 0.0, 500.0])  # far from everything
    n[300:305] = np.nan
    r = fr.compute_fpfh(p, n, 2.5, 100)
    assert r.sensitive.mean() <= 0.01
    f, s, nn = co.computeFPFHFeature(p, n, 2.5, 100, want_spfh=True, want_neighbours=True)
    assert np.array_equal(nn, r.nn)
    assert np.isfinite(s).all() and np.isfinite(f).all()     # a NaN normal only moves counts to bin 0
    assert np.array_equal(s[~r.sensitive], r.spfh[~r.sensitive])
    assert np.array_equal(f, fr.fpfh_from_spfh(s, nn, fr.list_d2(p, nn)))
    assert np.array_equal(f[~r.tainted], r.fpfh[~r.tainted])
    assert not f[200].any() and nn[200, 0] == 200 and nn[200, 1] == -1
    assert (nn[100, :10] == np.arange(100, 110)).all()      # equal distances: ascending index
    f2, s2, nn2 = co.computeFPFHFeature(p, n, 2.5, 100, want_spfh=True, want_neighbours=True)
    assert np.array_equal(f, f2) and np.array_equal(s, s2) and np.array_equal(nn, nn2)      # run to run
    for bad in (0, 129, -3):
        with pytest.raises(RuntimeError, match="o3s_status 11"):
            co.computeFPFHFeature(p, n, 2.5, bad)
    with pytest.raises(RuntimeError, match="o3s_status 11"):
        co.computeFPFHFeature(p, n, 0.0, 100)
