"""The crop and voxel pipelines of csrc/cloud_dev.h at their size, surface and key edges, bit for bit against the CPU oracle or numpy.
MI355X only.  The inputs come from tests/cloud_edge_cases.py; tests/test_cloud_edge_cases.py shows on the oracle alone that they are
what their names say.

  * the flag scan in isolation (k_heads + scan_flags, with the producer's per-block counts and through rocPRIM) across the sizes at
    which k_scan_flags_blk's prefix loop takes a second round (block 257: n >= 65 793);
  * points on and within a few ulps of every cropper surface, through the plain crop and through the fused crops of the resident
    pre-processing;
  * tiny, block-edge and degenerate selections through every host entry, the resident pre-processing and the submap insert;
  * index ranges that fill an exact power of two, indices far from the origin, and the refusal of a range that does not pack;
  * the merge insert into a map of some hundred thousand voxel points.
The oracle's voxel output order is unspecified: it is compared after a lexsort by voxel index, and the library's own order must be
ascending (z, y, x)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan, Submap
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as ops
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn

import cloud_edge_cases as ce
from test_gpu_submap import oracle_insert

pytestmark = pytest.mark.gpu

I32_MIN = np.iinfo(np.int32).min


@pytest.fixture(params=["hinted", "measured", "hint_miss"])
def index_range_path(request, monkeypatch):
    """As in tests/test_gpu_submap.py: the voxel index range hinted by the cropping volume on the PRODUCT library, and twice on the
    test-hook build: measured on the device (O3S_NO_HINT), and with a hint nothing fits in (O3S_HINT_MISS), so that the device's
    status word trips and the call is repeated on the measuring path.  Same bits."""
    from open3d_slam_advanced_rss_2024_public_amd import _lib

    monkeypatch.delenv("O3S_NO_HINT", raising=False)
    monkeypatch.delenv("O3S_HINT_MISS", raising=False)
    if request.param == "hinted":
        yield request.param
        return
    monkeypatch.setenv("O3S_NO_HINT" if request.param == "measured" else "O3S_HINT_MISS", "1")
    with _lib.variant("hooks"):
        yield request.param


# ---------------------------------------------------------------------------------------------------------------
# the flag scan in isolation
# ---------------------------------------------------------------------------------------------------------------
PASS_KEY = np.uint64(1) << np.uint64(40)


def _scan_patterns(n, rng):
    """run identifiers of n sorted keys, by pattern; None: every key is the pass key"""
    i = np.arange(n, dtype=np.uint64)
    last = np.zeros(n, np.uint64)
    last[-1] = 1
    short = np.cumsum(rng.random(n) < 0.5).astype(np.uint64)
    return {
        "all_one_key": np.zeros(n, np.uint64),
        "all_distinct": i,
        "all_pass_key": None,
        "only_the_last_differs": last,
        "head_at_the_last_lane_of_every_block": (i + np.uint64(1)) // np.uint64(256),
        "runs_of_mean_length_2": short,
        "runs_of_mean_length_100": np.cumsum(rng.random(n) < 0.01).astype(np.uint64),
        "pass_key_tail": short,
    }


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 65535, 65536, 65537, 65792, 65793, 131073, 300000])
def test_flag_scan_equals_numpy_with_block_counts_and_through_rocprim(hooks_lib, monkeypatch, n):
    """k_heads + scan_flags as the voxelisers chain them (hook o3s_test_scan_flags): with the producer's per-block counts
    (put_block_count + k_scan_flags_blk, one launch) and without (rocPRIM's scan + k_scan_total), the count posted and, under
    O3S_NO_MAILBOX, copied.  head[i] = key[i] != pass_key and (i == 0 or key[i-1] >> s != key[i] >> s); off = its exclusive sum;
    off[n] == count == head.sum().  65 793 is the first size whose last block (257) adds up the counts before it in two rounds."""
    f = hooks_lib.o3s_test_scan_flags
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    rng = np.random.default_rng(n)
    for name, ids in _scan_patterns(n, rng).items():
        if ids is None:
            keys = np.full(n, PASS_KEY)
        else:
            keys = (ids << np.uint64(2)) | rng.integers(1, 3, n).astype(np.uint64)     # two low bits: the merge insert's source rank
            if name == "pass_key_tail":
                keys[n - max(1, n // 3):] = PASS_KEY
        for shift in (0, 2):
            group = keys >> np.uint64(shift)
            head = keys != PASS_KEY
            head[1:] &= group[1:] != group[:-1]
            want_head = head.astype(np.uint32)
            want_off = np.concatenate([[0], np.cumsum(want_head)]).astype(np.uint32)
            for mailbox in (True, False):
                if mailbox:
                    monkeypatch.delenv("O3S_NO_MAILBOX", raising=False)
                else:
                    monkeypatch.setenv("O3S_NO_MAILBOX", "1")
                for with_blk in (1, 0):
                    got_head, got_off, count = np.full(n, 7, np.uint32), np.full(n + 1, 7, np.uint32), C.c_int64(-1)
                    assert f(0, keys.ctypes.data, n, int(PASS_KEY), shift, with_blk, got_head.ctypes.data, got_off.ctypes.data, C.byref(count)) == 0
                    what = (name, shift, "posted" if mailbox else "copied", "block counts" if with_blk else "rocPRIM")
                    assert np.array_equal(got_head, want_head), what
                    bad = np.flatnonzero(got_off != want_off)
                    assert bad.size == 0, (what, bad[:4], got_off[bad[:4]], want_off[bad[:4]])
                    assert count.value == int(want_off[n]) == int(want_head.sum()), what


# ---------------------------------------------------------------------------------------------------------------
# cropper surfaces
# ---------------------------------------------------------------------------------------------------------------
def _attributes(n, seed):
    rng = np.random.default_rng(seed)
    col = rng.uniform(0, 1, (n, 3))
    A = rng.normal(size=(n, 3, 3))
    return col, np.einsum("nij,nkj->nik", A, A).reshape(n, 9)


def _both_croppers(kind, params, centre, invert=False):
    a = list(params) + [0.0] * (3 - len(params))
    return ops.croppingVolumeFactory(kind, *a, centre=centre, invert=invert), orc.make_cropper(kind, *a, centre=centre, invert=invert)


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("case", ce.SURFACE_CASES, ids=ce.case_id)
def test_plain_crop_draws_every_surface_where_the_oracle_does(case, invert):
    """ops.crop / crop_attr (k_mask) over points on and within 4 ulps of every surface of the volume — sqrt((dx^2 + dy^2) + dz^2)
    against the radius, the cylinder's z against its planes — plus a point at the centre and points with a NaN or an infinite coordinate."""
    kind, params = case
    p, n_near = ce.near_surface_cloud(kind, params)
    g, o = _both_croppers(kind, params, ce.CENTRE, invert)
    assert 0.25 <= orc.crop_mask(o, p[:n_near]).mean() <= 0.75
    p = np.concatenate([p[: n_near // 2], ce.non_finite_points(), p[n_near // 2:]])
    nrm = ce.unit_normals(len(p), seed=1)
    col, cov = _attributes(len(p), 2)
    m = orc.crop_mask(o, p)
    gp, gn = ops.crop(g, p, nrm)
    assert gp.shape == p[m].shape and np.array_equal(gp, p[m], equal_nan=True) and np.array_equal(gn, nrm[m])
    gp, gn, gc, gv = ops.crop_attr(g, p, nrm, col, cov)
    assert np.array_equal(gp, p[m], equal_nan=True) and np.array_equal(gn, nrm[m]) and np.array_equal(gc, col[m]) and np.array_equal(gv, cov[m])


def _oracle_preprocess(sp, sn, wide, voxel, narrow):
    m = orc.crop_mask(wide, sp)
    p, n = sp[m], sn[m]
    if voxel > 0 and len(p):
        p, n, idx = orc.voxel_downsample_o3d(voxel, p, n)
        order = np.lexsort((idx[:, 0], idx[:, 1], idx[:, 2]))   # canonical voxel order (Open3D's is unspecified)
        p, n = p[order], n[order]
    m2 = orc.crop_mask(narrow, p)
    return (p, n), (p[m2], n[m2])


def _check_preprocess(ps, wide, voxel, narrow, sp, sn, want):
    n_merge, n_match = ps.preprocess(wide, voxel, narrow, sp, sn)
    (mp, mn), (np_, nn) = want
    gp, gn = ps.merge
    assert n_merge == len(mp) and np.array_equal(gp, mp) and np.array_equal(gn, mn, equal_nan=True)
    hp, hn = ps.match
    assert n_match == len(np_) and np.array_equal(hp, np_) and np.array_equal(hn, nn, equal_nan=True)


SURROUNDING = ("MaxRadius", (40.0,))          # holds every point of a near-surface cloud
ORDINARY_NARROW = ("Cylinder", (12.0, -2.0, 3.0))


@functools.lru_cache(maxsize=None)
def _surface_preprocess_case(case, voxel, role):
    kind, params = case
    p, n_near = ce.near_surface_cloud(kind, params)
    nrm = ce.unit_normals(len(p), seed=3, nan_every=97)
    wide, narrow = ((kind, params), ORDINARY_NARROW) if role == "wide" else (SURROUNDING, (kind, params))
    want = _oracle_preprocess(p, nrm, _both_croppers(*wide, ce.CENTRE)[1], voxel, _both_croppers(*narrow, ce.CENTRE)[1])
    for a in want[0] + want[1]:
        a.setflags(write=False)
    return p, nrm, wide, narrow, want, n_near


@pytest.mark.parametrize("role", ["wide", "narrow"])
@pytest.mark.parametrize("voxel", [0.0, 0.12])
@pytest.mark.parametrize("case", ce.SURFACE_CASES, ids=ce.case_id)
def test_resident_preprocess_draws_every_surface_where_the_plain_crop_does(case, voxel, role, index_range_path):
    """ProcessedScan.preprocess with the near-surface cloud's volume as the wide volume (the crop fused into k_min_part and
    k_vox_key_direct on the hinted path, k_mask otherwise) and as the narrow one (k_mask_cnt / k_mask over the down-sampled cloud, whose
    voxels mostly hold one point: the point itself comes back)."""
    p, nrm, wide, narrow, want, n_near = _surface_preprocess_case(case, voxel, role)
    n_sel = len(want[0][0]) if role == "wide" else len(want[1][0])
    assert 0.2 * n_near < n_sel < len(p)                        # the surface decides both ways on this path too
    _check_preprocess(ProcessedScan(), _both_croppers(*wide, ce.CENTRE)[0], voxel, _both_croppers(*narrow, ce.CENTRE)[0], p, nrm, want)


# ---------------------------------------------------------------------------------------------------------------
# sizes and degenerate selections through every pipeline
# ---------------------------------------------------------------------------------------------------------------
VOLUME = (ce.DEGENERATE_VOLUME[0], tuple(ce.DEGENERATE_VOLUME[1:]))     # (kind, parameters)
SIZES = [1, 2, 5, 6, 7, 63, 64, 65, 255, 256, 257, 70001, 140001]
CLOUDS = [("generic", n) for n in SIZES] + [(name, n) for name in ce.DEGENERATE_KINDS for n in (7, 257, 3000)]


def _cloud_id(c):
    return f"{c[0]}-{c[1]}"


def _cloud(which, centre=ce.CENTRE, seed=0):
    name, n = which
    return ce.generic_cloud(n, centre, seed=seed) if name == "generic" else ce.degenerate_cloud(name, n, centre, seed=seed)


def _canonical(oi):
    """the oracle's output order -> [pass-through block in input order | voxels ascending in (z, y, x)]"""
    k = int((oi[:, 0] == I32_MIN).sum())
    assert (oi[:k] == I32_MIN).all() and (oi[k:, 0] != I32_MIN).all()
    return np.concatenate([np.arange(k), np.lexsort((oi[k:, 0], oi[k:, 1], oi[k:, 2])) + k]).astype(np.int64), k


def _check_host_entries(p, nrm, col, cov, volume, centre, voxel):
    """the four voxelising host entries (they always measure the index range) against the oracle"""
    g, o = _both_croppers(*volume, centre)
    op, on, oi = orc.voxelize_within_crop(o, voxel, p, nrm)
    ocol, ocov = orc.voxelize_attrs(0, o, voxel, p, col, cov)
    order, k = _canonical(oi)
    gp, gn, gi = ops.voxelizeWithinCroppingVolume(voxel, g, p, nrm)
    assert len(gp) == len(op) and np.array_equal(gi, oi[order]) and np.array_equal(gp, op[order]) and np.array_equal(gn, on[order], equal_nan=True)
    assert np.array_equal(np.lexsort((gi[k:, 0], gi[k:, 1], gi[k:, 2])), np.arange(len(gi) - k))     # the library's own order
    gp, gn, gc, gv, gi = ops.voxelizeWithinCroppingVolume_attr(voxel, g, p, nrm, col, cov)
    assert np.array_equal(gi, oi[order]) and np.array_equal(gp, op[order]) and np.array_equal(gn, on[order], equal_nan=True)
    assert np.array_equal(gc, ocol[order]) and np.array_equal(gv, ocov[order])
    op, on, oi = orc.voxel_downsample_o3d(voxel, p, nrm)
    ocol, ocov = orc.voxelize_attrs(1, None, voxel, p, col, cov)
    order, k = _canonical(oi)
    assert k == 0
    gp, gn, gi = ops.voxelize(voxel, p, nrm)
    assert len(gp) == len(op) and np.array_equal(gi, oi[order]) and np.array_equal(gp, op[order]) and np.array_equal(gn, on[order], equal_nan=True)
    assert np.array_equal(np.lexsort((gi[:, 0], gi[:, 1], gi[:, 2])), np.arange(len(gi)))
    gp, gn, gc, gv, gi = ops.voxelize_attr(voxel, p, nrm, col, cov)
    assert np.array_equal(gi, oi[order]) and np.array_equal(gp, op[order]) and np.array_equal(gn, on[order], equal_nan=True)
    assert np.array_equal(gc, ocol[order]) and np.array_equal(gv, ocov[order])
    return len(gp)


@pytest.mark.parametrize("which", CLOUDS, ids=_cloud_id)
def test_host_voxelisers_at_every_size_and_degenerate_selection(which):
    """voxelizeWithinCroppingVolume (normals; normals, colours and covariances), voxelize and voxelize_attr: one point to 140 001 (548
    blocks: k_scan_flags_blk is not on this path, rocPRIM's scan is), either side of a wave and of a block, and the selections in which
    one lane sums every point, every point is a voxel, nothing or a single point is voxelised, a voxel has no valid normal."""
    p, nrm = _cloud(which)
    col, cov = _attributes(len(p), 5)
    _check_host_entries(p, nrm, col, cov, VOLUME, ce.CENTRE, ce.DEGENERATE_VOXEL)


PRE_NARROW = ("MaxRadius", (6.0,))


@functools.lru_cache(maxsize=None)
def _preprocess_case(which):
    p, nrm = _cloud(which)
    want = _oracle_preprocess(p, nrm, _both_croppers(*VOLUME, ce.CENTRE)[1], ce.DEGENERATE_VOXEL, _both_croppers(*PRE_NARROW, ce.CENTRE)[1])
    for a in want[0] + want[1]:
        a.setflags(write=False)
    return p, nrm, want


@pytest.mark.parametrize("which", CLOUDS, ids=_cloud_id)
def test_resident_preprocess_at_every_size_and_degenerate_selection(which, index_range_path):
    """ProcessedScan.preprocess on the same clouds.  Hinted, N = 5 keeps the per-block minima in the work area's 64-slot `part` and
    N = 6 is the first size that borrows `head` for them (nb * 24 <= N * 4); 70 001 and 140 001 points take k_scan_flags_blk into its
    second round.  A scan wholly outside the wide volume gives (0, 0) and empty clouds — the anchor is folded from no point — and leaves
    the object fit for the next scan."""
    p, nrm, want = _preprocess_case(which)
    wide, narrow = _both_croppers(*VOLUME, ce.CENTRE)[0], _both_croppers(*PRE_NARROW, ce.CENTRE)[0]
    ps = ProcessedScan()
    _check_preprocess(ps, wide, ce.DEGENERATE_VOXEL, narrow, p, nrm, want)
    if which[0] == "all_outside":
        assert (ps.n_merge, ps.n_match) == (0, 0) and ps.merge[0].shape == (0, 3) and ps.match[0].shape == (0, 3)
        p2, nrm2, want2 = _preprocess_case(("generic", 257))
        assert len(want2[1][0]) > 0
        _check_preprocess(ps, wide, ce.DEGENERATE_VOXEL, narrow, p2, nrm2, want2)


def _pose(k, origin):
    return syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.2 + 0.1 * k), np.asarray(origin, np.float64) + np.array([0.5 * k, 0.0, 0.0]))


@functools.lru_cache(maxsize=None)
def _insert_case(which, origin, voxel):
    """two successive scans (built around the sensor, posed at `origin` and half a metre on) and the oracle's map after each"""
    out, mp, mn = [], None, None
    for k in range(2):
        sp, sn = _cloud(which, centre=(0.0, 0.0, 0.0), seed=k)
        T = _pose(k, origin)
        mp, mn = oracle_insert(mp, mn, sp, sn, T, voxel, ce.DEGENERATE_VOLUME[0], ce.DEGENERATE_VOLUME[1:])
        mp.setflags(write=False)
        mn.setflags(write=False)
        out.append((sp, sn, T, mp, mn))
    return out


def _check_inserts(case, voxel):
    sm = Submap(voxel, ops.croppingVolumeFactory(*ce.DEGENERATE_VOLUME))
    for sp, sn, T, mp, mn in case:
        assert sm.insertScan(sp, sn, T)
        gp, gn = sm.getMapPointCloud()
        assert len(sm) == len(mp) and np.array_equal(gp, mp) and np.array_equal(gn, mn, equal_nan=True)
    return sm


@pytest.mark.parametrize("which", CLOUDS, ids=_cloud_id)
def test_submap_insert_at_every_size_and_degenerate_selection(which, index_range_path):
    """Submap.insertScan of two successive scans of each cloud: the first through the sort-based pipeline (hinted: k_mask with block
    counts, k_scan_flags_blk), the second — where the first left voxel points — through the merge insert."""
    _check_inserts(_insert_case(which, ce.CENTRE, ce.DEGENERATE_VOXEL), ce.DEGENERATE_VOXEL)


# ---------------------------------------------------------------------------------------------------------------
# key width
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abc", [(1, 1, 1), (4, 4, 4), (10, 10, 11)], ids=lambda t: "x".join(map(str, t)))
def test_index_range_that_fills_an_exact_power_of_two(abc):
    """The measuring path gives pass-through points the key 1 << bits with bits from ex * ey * ez: here the product IS a power of two,
    the highest-corner voxel (the largest packed key) is occupied and pass-through points are present — the two must stay apart."""
    p, nrm, (kind, radius, centre), lo, hi = ce.pow2_range(*abc)
    col, cov = _attributes(len(p), 6)
    _check_host_entries(p, nrm, col, cov, (kind, (radius,)), centre, 1.0)
    gp, gn, gi = ops.voxelizeWithinCroppingVolume(1.0, ops.croppingVolumeFactory(kind, radius, centre=centre), p, nrm)
    k = int((gi[:, 0] == I32_MIN).sum())
    assert k == 40 and np.array_equal(gi[k], lo) and np.array_equal(gi[-1], hi)


def test_indices_far_from_the_origin_through_the_host_entries():
    p, nrm = ce.far_from_origin()
    col, cov = _attributes(len(p), 7)
    n_out = _check_host_entries(p, nrm, col, cov, VOLUME, ce.FAR_ORIGIN, ce.FAR_VOXEL)
    assert 0 < n_out < len(p)


def test_indices_far_from_the_origin_through_the_submap(index_range_path):
    """the volume centred at (4e5, -3e5, -50) with voxel 0.1: hinted, the range's lowest index is of magnitude 4e6 and negative on two axes"""
    _check_inserts(_insert_case(("generic", 3000), ce.FAR_ORIGIN, ce.FAR_VOXEL), ce.FAR_VOXEL)


def test_a_range_that_does_not_pack_is_refused_and_the_next_call_is_served():
    """index extents that multiply to >= 9e18 do not pack into 63 key bits: O3S_ERR_BAD_ARGUMENT (11), and nothing is left behind"""
    p = ce.unpackable_cloud()
    with pytest.raises(RuntimeError, match="o3s_status 11"):
        ops.voxelize(0.1, p)
    with pytest.raises(RuntimeError, match="o3s_status 11"):
        ops.voxelizeWithinCroppingVolume(0.1, ops.croppingVolumeFactory("MaxRadius", 1e9), p, np.ones_like(p))
    q, nrm = ce.generic_cloud(257)
    col, cov = _attributes(len(q), 8)
    _check_host_entries(q, nrm, col, cov, VOLUME, ce.CENTRE, ce.DEGENERATE_VOXEL)


# ---------------------------------------------------------------------------------------------------------------
# the merge insert at map size
# ---------------------------------------------------------------------------------------------------------------
MAP_VOLUME, MAP_VOXEL = ("MaxRadius", 12.0), 0.1


def _ball(rng, n, radius):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True) * (radius * rng.random((n, 1)) ** (1.0 / 3.0))


@functools.lru_cache(maxsize=None)
def _map_size_case():
    rng = np.random.default_rng(77)
    out, mp, mn = [], None, None
    for k, n in enumerate((300_000, 20_000, 20_000, 20_000)):
        sp = _ball(rng, n, 11.5)
        sn = rng.normal(size=(n, 3))
        sn /= np.linalg.norm(sn, axis=1, keepdims=True)
        T = _pose(k, (0.0, 0.2, 1.5))
        n_before = 0 if mp is None else len(mp)
        mp, mn = oracle_insert(mp, mn, sp, sn, T, MAP_VOXEL, MAP_VOLUME[0], MAP_VOLUME[1:])
        mp.setflags(write=False)
        mn.setflags(write=False)
        out.append((sp, sn, T, mp, mn, n_before + n))
    return out


def test_merge_insert_into_a_map_of_some_hundred_thousand_voxel_points(monkeypatch, index_range_path):
    """voxel_insert_merge_dev streams the whole map: here three 20 000-point scans, half a metre apart, into a map of more than 100 000
    voxel points, so that n_tmp > 65 793 and both flag scans of the merge (the pass-through flags over n_tmp, the heads over the merged
    keys) take k_scan_flags_blk's second round.  Equal to the oracle after every insert, merged on the hinted path, and the same bytes
    as the sort-only insert (O3S_INSERT_SORT, hooks build) and as the same inserts with rocPRIM's scan in place of k_scan_flags_blk
    (O3S_SCAN_ROCPRIM, hooks build)."""
    from open3d_slam_advanced_rss_2024_public_amd import _lib

    case = _map_size_case()
    assert len(case[0][3]) > 100_000 and all(n_tmp > 65_793 for *_, n_tmp in case)
    a = Submap(MAP_VOXEL, ops.croppingVolumeFactory(*MAP_VOLUME))
    for sp, sn, T, mp, mn, _ in case:
        assert a.insertScan(sp, sn, T)
        gp, gn = a.getMapPointCloud()
        assert len(a) == len(mp) and np.array_equal(gp, mp) and np.array_equal(gn, mn)
    if index_range_path == "hinted":
        assert a.insert_stats() == (3, 1, 0)                    # (merged, sorted, fell back)
    elif index_range_path == "measured":
        assert a.insert_stats()[0] == 0
    monkeypatch.setenv("O3S_INSERT_SORT", "1")
    with _lib.variant("hooks"):
        b = Submap(MAP_VOXEL, ops.croppingVolumeFactory(*MAP_VOLUME))
        for sp, sn, T, *_ in case:
            assert b.insertScan(sp, sn, T)
        assert b.insert_stats()[0] == 0 and b.insert_stats()[2] == 0
        pb, nb = b.getMapPointCloud()
    pa, na = a.getMapPointCloud()
    assert pa.tobytes() == pb.tobytes() and na.tobytes() == nb.tobytes()
    # and with every flag scan of the pipelines handed to rocPRIM (O3S_SCAN_ROCPRIM, hooks build) instead of k_scan_flags_blk
    monkeypatch.delenv("O3S_INSERT_SORT")
    monkeypatch.setenv("O3S_SCAN_ROCPRIM", "1")
    with _lib.variant("hooks"):
        c = Submap(MAP_VOXEL, ops.croppingVolumeFactory(*MAP_VOLUME))
        for sp, sn, T, *_ in case:
            assert c.insertScan(sp, sn, T)
        assert c.insert_stats() == a.insert_stats()
        pc, nc = c.getMapPointCloud()
    assert pa.tobytes() == pc.tobytes() and na.tobytes() == nc.tobytes()
