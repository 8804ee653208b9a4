"""The input builders of tests/cloud_edge_cases.py give what their names say — asserted on the CPU oracle alone (no GPU): the GPU tests
(tests/test_gpu_cloud_edges.py) then compare the library with the oracle on exactly these clouds."""
import numpy as np
import pytest

from oracle import oracle as orc

import cloud_edge_cases as ce

I32_MIN = np.iinfo(np.int32).min


@pytest.mark.parametrize("case", ce.SURFACE_CASES, ids=ce.case_id)
def test_near_surface_cloud_splits_on_the_surface(case):
    """Of the near-surface part the oracle keeps at least a quarter and drops at least a quarter, points a few ulps apart fall on both
    sides, and (spheres) some points lie exactly on the surface: inside for `<= r` and for `>= r` alike."""
    kind, params = case
    p, n_near = ce.near_surface_cloud(kind, params)
    assert n_near >= 4000 and len(p) - n_near >= 200 and np.isfinite(p).all()
    m = orc.crop_mask(orc.make_cropper(kind, *params, centre=ce.CENTRE), p)[:n_near]
    assert 0.25 <= m.mean() <= 0.75, m.mean()
    mi = orc.crop_mask(orc.make_cropper(kind, *params, centre=ce.CENTRE, invert=True), p)[:n_near]
    assert np.array_equal(mi, ~m)
    # every near point is within 1e-12 of a surface: a volume grown or shrunk by that much takes all of them or none
    eps = 1e-12
    if kind in ("MaxRadius", "MinRadius", "MinMaxRadius"):
        for r in params:
            on = (orc.crop_mask(orc.make_cropper("MaxRadius", r, centre=ce.CENTRE), p)[:n_near]
                  & orc.crop_mask(orc.make_cropper("MinRadius", r, centre=ce.CENTRE), p)[:n_near])
            assert on.sum() >= 10, on.sum()                      # exactly on the surface
        near = np.zeros(n_near, bool)
        for r in params:
            near |= (orc.crop_mask(orc.make_cropper("MinMaxRadius", r - eps, r + eps, centre=ce.CENTRE), p)[:n_near])
        assert near.all()
    else:
        r, z0, z1 = params
        side = orc.crop_mask(orc.make_cropper("Cylinder", r + eps, -1e9, 1e9, centre=ce.CENTRE), p)[:n_near] \
            & ~orc.crop_mask(orc.make_cropper("Cylinder", r - eps, -1e9, 1e9, centre=ce.CENTRE), p)[:n_near]
        planes = np.zeros(n_near, bool)
        for z in (z0, z1):
            planes |= orc.crop_mask(orc.make_cropper("Cylinder", r, z - eps, z + eps, centre=ce.CENTRE), p)[:n_near]
        assert (side | planes).all()
        for sel in (side, planes):                               # the side and the planes each decide both ways
            assert sel.sum() >= 1000 and 0.25 <= m[sel].mean() <= 0.75, (sel.sum(), m[sel].mean())


def _mask_from(kind, params, p, squares):
    """isWithinVolume restated in numpy, with the distance compared as it is (sqrt) or as squares"""
    d = p - np.asarray(ce.CENTRE)
    x = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + (0.0 if kind == "Cylinder" else d[:, 2] * d[:, 2])
    dist = x if squares else np.sqrt(x)
    r = [v * v if squares else v for v in params]
    if kind == "MaxRadius":
        return dist <= r[0]
    if kind == "MinRadius":
        return dist >= r[0]
    if kind == "MinMaxRadius":
        return (dist <= r[1]) & (dist >= r[0])
    return (p[:, 2] >= params[1]) & (p[:, 2] <= params[2]) & (dist <= r[0])


@pytest.mark.parametrize("case", ce.SURFACE_CASES, ids=ce.case_id)
def test_near_surface_cloud_tells_the_square_root_from_squares(case):
    """The oracle's mask is numpy's sqrt((dx^2 + dy^2) + dz^2) against the radius, and every kind has a case whose cloud holds points
    that d^2 against r^2 decides differently (none can with 15.0, whose square is exact; 5.3 tells only for `>=`, 11.3 for both)."""
    kind, params = case
    p, n_near = ce.near_surface_cloud(kind, params)
    m = orc.crop_mask(orc.make_cropper(kind, *params, centre=ce.CENTRE), p)
    assert np.array_equal(m, _mask_from(kind, params, p, squares=False))
    differ = int((m != _mask_from(kind, params, p, squares=True)).sum())
    tells = case in [("MaxRadius", (11.3,)), ("MinRadius", (5.3,)), ("MinMaxRadius", (5.3, 15.0)), ("MinMaxRadius", (5.3, 11.3)),
                     ("Cylinder", (11.3, -3.1, 4.2))]
    assert (differ >= 20) if tells else (differ == 0), differ


def test_non_finite_points_are_what_they_say():
    q = ce.non_finite_points()
    assert np.array_equal(q[0], ce.CENTRE) and not np.isfinite(q[1:]).all(axis=1).any()
    m = orc.crop_mask(orc.make_cropper("MaxRadius", 15.0, centre=ce.CENTRE), q)
    assert m[0] and not m[1:].any()                              # a NaN or infinite distance is not <= r
    m = orc.crop_mask(orc.make_cropper("MinRadius", 15.0, centre=ce.CENTRE), q)
    assert not m[0] and m[1:].any() and not m[1:].all()          # infinite: outside the radius; NaN: neither


def _vox0(p, n):
    c = orc.make_cropper(*ce.DEGENERATE_VOLUME, centre=ce.CENTRE)
    op, on, oi = orc.voxelize_within_crop(c, ce.DEGENERATE_VOXEL, p, n)
    k = int((oi[:, 0] == I32_MIN).sum())
    assert (oi[:k] == I32_MIN).all() and (oi[k:] != I32_MIN).all()
    return op, on, oi, k


@pytest.mark.parametrize("n", [7, 257, 3000])
def test_degenerate_clouds_are_degenerate(n):
    v = ce.DEGENERATE_VOXEL
    p, nrm = ce.degenerate_cloud("one_voxel", n)
    op, on, oi, k = _vox0(p, nrm)
    assert k == 0 and len(op) == 1
    assert len(orc.voxel_downsample_o3d(v, p, nrm)[0]) == 1      # and one voxel on Open3D's grid, anchored at the cloud's minimum

    p, nrm = ce.degenerate_cloud("own_voxel", n)
    op, on, oi, k = _vox0(p, nrm)
    assert k == 0 and len(op) == n and len(np.unique(oi, axis=0)) == n
    assert len(orc.voxel_downsample_o3d(v, p, nrm)[0]) == n

    p, nrm = ce.degenerate_cloud("all_outside", n)
    op, on, oi, k = _vox0(p, nrm)
    assert k == n and len(op) == n and np.array_equal(op, p)     # nothing voxelised: n pass-through points, in order
    assert not orc.crop_mask(orc.make_cropper(*ce.DEGENERATE_VOLUME, centre=ce.CENTRE), p).any()

    p, nrm = ce.degenerate_cloud("one_inside", n)
    op, on, oi, k = _vox0(p, nrm)
    assert k == n - 1 and len(op) == n and np.array_equal(op[-1], p[n // 2])
    m = orc.crop_mask(orc.make_cropper(*ce.DEGENERATE_VOLUME, centre=ce.CENTRE), p)
    assert m.sum() == 1 and m[n // 2]

    p, nrm = ce.degenerate_cloud("nan_normal_voxel", n)
    op, on, oi, k = _vox0(p, nrm)
    row = np.flatnonzero(np.all(oi == ce.nan_voxel_index(), axis=1))
    assert len(row) == 1
    members = np.all(orc.voxel_idx(p, v) == ce.nan_voxel_index(), axis=1)
    assert members.sum() >= max(2, n // 10) and np.isnan(nrm[members]).any(axis=1).all()
    assert np.array_equal(on[row[0]], np.zeros(3))               # every normal skipped: a sum of zero, not normalised
    others = np.delete(np.arange(len(on)), row[0])[k:]
    assert np.isfinite(on[others]).all()


@pytest.mark.parametrize("n", [1, 2, 5, 6, 7, 63, 257, 70001])
def test_generic_cloud_is_mostly_inside(n):
    p, nrm = ce.generic_cloud(n)
    assert p.shape == nrm.shape == (n, 3)
    m = orc.crop_mask(orc.make_cropper(*ce.DEGENERATE_VOLUME, centre=ce.CENTRE), p)
    assert m.sum() >= 1 and (n < 63 or (0.5 < m.mean() < 1.0))
    if n >= 257:
        assert np.isnan(nrm).any() and not np.isnan(nrm).all(axis=1).any()


@pytest.mark.parametrize("abc", [(1, 1, 1), (4, 4, 4), (10, 10, 11)], ids=lambda t: "x".join(map(str, t)))
def test_pow2_range_fills_an_exact_power_of_two(abc):
    """The measured extents are exactly the three powers of two, both corner cells are occupied and the pass-through block stays apart
    from the highest-corner voxel (on the device its key is the largest packed key, the pass key the next power of two)."""
    p, nrm, (kind, radius, centre), lo, hi = ce.pow2_range(*abc)
    op, on, oi = orc.voxelize_within_crop(orc.make_cropper(kind, radius, centre=centre), 1.0, p, nrm)
    k = int((oi[:, 0] == I32_MIN).sum())
    outside = ~orc.crop_mask(orc.make_cropper(kind, radius, centre=centre), p)
    assert k == outside.sum() == 40 and outside[0] and outside[-1] and np.array_equal(op[:k], p[outside])
    vi = oi[k:]
    assert (vi != I32_MIN).all()
    assert np.array_equal(vi.min(axis=0), lo) and np.array_equal(vi.max(axis=0), hi)
    assert np.array_equal(hi.astype(np.int64) - lo + 1, [1 << abc[0], 1 << abc[1], 1 << abc[2]])
    for corner in (lo, hi):
        row = np.flatnonzero(np.all(vi == corner, axis=1))
        assert len(row) == 1
        members = p[np.all(orc.voxel_idx(p, 1.0) == corner, axis=1) & ~outside]
        assert len(members) >= 1 and np.all(np.floor(op[k + row[0]]) == corner)      # the mean of its own members only
        assert np.allclose(op[k + row[0]], members.mean(axis=0), rtol=0, atol=1e-9)


def test_far_from_origin_indices():
    p, nrm = ce.far_from_origin()
    idx = orc.voxel_idx(p, ce.FAR_VOXEL)
    assert idx[:, 0].min() > 3_900_000 and idx[:, 1].max() < -2_900_000 and idx[:, 2].max() < 0
    c = orc.make_cropper(*ce.DEGENERATE_VOLUME, centre=ce.FAR_ORIGIN)
    op, on, oi = orc.voxelize_within_crop(c, ce.FAR_VOXEL, p, nrm)
    k = int((oi[:, 0] == I32_MIN).sum())
    assert 0 < k < len(op) < len(p)                              # pass-through points, and voxels that hold several points


def test_unpackable_cloud_exceeds_63_key_bits():
    p = ce.unpackable_cloud()
    idx = orc.voxel_idx(p, 0.1).astype(np.int64)
    ext = idx.max(axis=0) - idx.min(axis=0) + 1
    assert float(ext[0]) * float(ext[1]) * float(ext[2]) >= 9e18
    assert np.abs(idx).max() < 2 ** 31 - 1                       # the indices themselves are representable


def test_ulp_steps():
    x = np.array([1.0, -1.0, 15.0, 4.0])
    y = ce.ulp_steps(x, np.array([1, 1, -2, 0]))
    assert y[0] == np.nextafter(1.0, 2.0) and y[1] == np.nextafter(-1.0, 0.0) and y[3] == 4.0
    assert y[2] == np.nextafter(np.nextafter(15.0, 0.0), 0.0)
