"""Space carving of the sparse map (o3s_submap_carve) across its parameters, subsets, launch and sort
boundaries, ray edges, non-finite input and the state it leaves behind, against the CPU oracle.  MI355X only.

Maps are planted with Submap.setMapPointCloud and the cropping volume gets its centre from the factory, so the subset the
oracle needs (orc.crop_mask) is known without an insert.  Everything compared is an integer or a bit pattern: the removed
count, the decision per map point, the survivors and their order.  No tolerance anywhere."""
import numpy as np
import pytest

from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig, Submap
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn
from test_gpu_submap import oracle_insert

pytestmark = pytest.mark.gpu

SENSOR = np.array([0.31, -0.22, 0.13])       # its 0.05-voxel (6, -5, 2) lies inside its 0.1- and 0.3-voxels
N_PLANTED = 20


def pose(pos=SENSOR, angle=1.1):
    """A pose whose rotation has no zero entry."""
    return syn.make_T(syn.rot_axis_angle([1.0, 1.0, 1.0], angle), np.asarray(pos, np.float64))


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_rays(n, seed, lo=1.0, hi=4.0):
    """n returns in the SENSOR frame, directions uniform on the sphere, lengths in [lo, hi)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(lo, hi, (n, 1))


def make_map(n_uniform, seed, with_normals, sensor=SENSOR, extent=3.0):
    """N_PLANTED points well inside the sensor's own 0.05-voxel, then n_uniform points in +-extent; unit normals, 50 of them
    zero — ten of those on planted points, which every ray's first stop reaches."""
    rng = np.random.default_rng(seed)
    centre = (np.floor(sensor / 0.05) + 0.5) * 0.05
    p = np.concatenate([centre + rng.uniform(-0.02, 0.02, (N_PLANTED, 3)), rng.uniform(-extent, extent, (n_uniform, 3))])
    if not with_normals:
        return p, None
    nr = rng.normal(size=p.shape)
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    nr[10:20] = 0.0
    if n_uniform >= 40:
        nr[N_PLANTED + rng.choice(n_uniform, 40, replace=False)] = 0.0
    return p, nr


def device_kind(kind):   # the device mirror names the pass-everything volume after the reference's base class
    return "CroppingVolume" if kind == "Base" else kind


def new_submap(map_p, map_n, crop=("MaxRadius", 10.0), centre=(0.0, 0.0, 0.0), invert=False, map_voxel=0.1):
    p = tuple(crop[1:]) + (0.0,) * (4 - len(crop))
    sm = Submap(map_voxel, co.croppingVolumeFactory(device_kind(crop[0]), *p, centre=centre, invert=invert))
    sm.setMapPointCloud(map_p, map_n)
    return sm


def oracle_carve(map_p, map_n, raw, T, crop=("MaxRadius", 10.0), centre=(0.0, 0.0, 0.0), invert=False, voxel=0.1, max_len=20.0, trunc=0.1,
                 min_dot=0.5):
    scan_map, _ = orc.transform_cloud(T, raw, None)
    p = tuple(crop[1:]) + (0.0,) * (4 - len(crop))
    subset = orc.crop_mask(orc.make_cropper(crop[0], *p, centre=centre, invert=invert), map_p)
    return orc.carve(scan_map, map_p, map_n, np.asarray(T)[:3, 3], voxel, max_len, trunc, min_dot, subset=subset), subset


def carve_equals(sm, map_p, map_n, raw, T, rm, voxel=0.1, max_len=20.0, trunc=0.1, min_dot=0.5, expect="some", what=""):
    """The one comparison every case makes: the oracle's count is non-zero (or zero where the case is built to remove nothing),
    the device removes as many, and what is left is map[~rm] bit for bit, normals included."""
    k = int(rm.sum())
    assert (k > 0) if expect == "some" else (k == 0), (what, k)
    n_removed = sm.carve(raw, T, voxel_size=voxel, max_raytracing_length=max_len, truncation_distance=trunc, min_dot_product_with_normal=min_dot)
    gp, gn = sm.getMapPointCloud()
    print(f"carve {what}: oracle removes {k} of {len(map_p)}, device {n_removed}, left {len(gp)}")
    assert n_removed == k, what
    assert len(sm) == len(map_p) - k
    assert same_bits(gp, map_p[~rm]), what
    if map_n is None:
        assert gn is None
    else:
        assert same_bits(gn, map_n[~rm]), what


def run_case(map_p, map_n, raw, T, crop=("MaxRadius", 10.0), centre=(0.0, 0.0, 0.0), invert=False, expect="some", what="", **cp):
    rm, subset = oracle_carve(map_p, map_n, raw, T, crop, centre, invert, **cp)
    sm = new_submap(map_p, map_n, crop, centre, invert)
    carve_equals(sm, map_p, map_n, raw, T, rm, expect=expect, what=what, **cp)
    return sm, rm, subset


# ---------------------------------------------------------------------------------------------------------------
# a. parameter grid
# ---------------------------------------------------------------------------------------------------------------
GRID = {
    "voxel_0.05": dict(voxel=0.05),
    "voxel_0.1": dict(voxel=0.1),
    "voxel_0.3_several_points_per_key": dict(voxel=0.3),
    "rays_cut_at_2m": dict(max_len=2.0),
    "ray_length_below_one_voxel": dict(max_len=0.05),
    "truncation_beyond_the_ray": dict(trunc=50.0),
    "min_dot_-0.1": dict(min_dot=-0.1),
    "min_dot_0.0": dict(min_dot=0.0),
    "min_dot_0.5": dict(min_dot=0.5),
    "min_dot_0.999": dict(min_dot=0.999),
    "min_dot_1.0": dict(min_dot=1.0),
}


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("row", list(GRID))
def test_parameter_grid(row, with_normals):
    cp = GRID[row]
    T = pose()
    raw = make_rays(300, 11)
    mp, mn = make_map(5000, 12, with_normals)
    if with_normals:   # five planted points face ray k exactly: |dot| is 1 up to rounding, above 0.999 for certain
        sm_, _ = orc.transform_cloud(T, raw[:5], None)
        d = sm_ - SENSOR
        mn[:5] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rm, _ = oracle_carve(mp, mn, raw, T, **cp)
    # |dot| > 1 needs a dot product that rounds above 1: the oracle decides whether this cloud has one; a map without normals
    # ignores min_dot altogether
    expect = "none" if (with_normals and row == "min_dot_1.0" and not rm.any()) else "some"
    sm = new_submap(mp, mn)
    carve_equals(sm, mp, mn, raw, T, rm, expect=expect, what=row, **cp)
    vox = cp.get("voxel", 0.1)
    in_sensor_voxel = (orc.voxel_idx(mp, vox) == orc.voxel_idx(SENSOR[None], vox)).all(axis=1)
    assert in_sensor_voxel[:N_PLANTED].all()
    if row in ("ray_length_below_one_voxel", "truncation_beyond_the_ray"):
        assert not rm[~in_sensor_voxel].any()          # a single stop, at the sensor
        if not with_normals:
            assert rm[in_sensor_voxel].all()
    if row == "voxel_0.3_several_points_per_key":
        assert int(in_sensor_voxel.sum()) >= N_PLANTED and rm.sum() > 100
    if with_normals and row.startswith("min_dot"):     # a zero normal gives a dot product of exactly 0
        assert rm[10:20].all() == (cp["min_dot"] < 0) and rm[10:20].any() == (cp["min_dot"] < 0)
    if with_normals and row == "min_dot_0.999":
        assert rm[:5].all()


# ---------------------------------------------------------------------------------------------------------------
# b. subsets
# ---------------------------------------------------------------------------------------------------------------
SUBSETS = {
    "MaxRadius": dict(crop=("MaxRadius", 2.0), centre=(0.2, 0.1, 0.0)),
    "Cylinder": dict(crop=("Cylinder", 2.0, -1.0, 1.5), centre=(0.2, 0.1, 0.0)),
    "MinRadius_unbounded": dict(crop=("MinRadius", 1.0), centre=(0.2, 0.1, 0.0)),
    "Base_unbounded": dict(crop=("Base",)),
    "MaxRadius_inverted": dict(crop=("MaxRadius", 1.5), centre=(0.2, 0.1, 0.0), invert=True),
}


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("kind", list(SUBSETS))
def test_cropper_kinds(kind, with_normals):
    mp, mn = make_map(5000, 21, with_normals)
    _, rm, subset = run_case(mp, mn, make_rays(300, 22), pose(), what=kind, **SUBSETS[kind])
    assert 0 < subset.sum() and not rm[~subset].any()
    if kind != "Base_unbounded":
        assert subset.sum() < len(mp)


def test_subset_of_exactly_one_point_and_empty_subset():
    mp, _ = make_map(5000, 23, False)
    raw, T = make_rays(300, 24), pose()
    _, rm, subset = run_case(mp, None, raw, T, crop=("MaxRadius", 1e-9), centre=tuple(mp[3]), what="one point")
    assert subset.sum() == 1 and rm.sum() == 1 and rm[3]
    sm, rm, subset = run_case(mp, None, raw, T, crop=("MaxRadius", 0.5), centre=(100.0, 100.0, 100.0), expect="none", what="empty subset")
    assert subset.sum() == 0
    assert same_bits(sm.getMapPointCloud()[0], mp)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_sensor_outside_the_index_box_rays_leave_through_every_face(sign):
    """The subset is a ball of radius 1 at the origin, its index box about +-1 m; the sensor sits outside beyond a corner and
    every ray is aimed through a point ON one of the three far faces of the box, well inside that face, and ends behind it:
    it is inside the box just before that point and leaves through that face.  The two corners together cover all six."""
    rng = np.random.default_rng(31)
    mp = rng.uniform(-3.0, 3.0, (6000, 3))
    sensor = sign * np.array([2.05, 1.95, 2.15])
    T = pose(sensor, 0.7)
    through = []
    for axis in range(3):
        q = rng.uniform(-0.6, 0.6, (40, 3))
        q[:, axis] = -sign * 0.95
        through.append(q)
    through = np.concatenate(through)
    ends = sensor + 1.4 * (through - sensor)
    raw = (ends - sensor) @ T[:3, :3]                     # R^T (end - t), row-wise
    crop = dict(crop=("MaxRadius", 1.0), centre=(0.0, 0.0, 0.0))
    rm, subset = oracle_carve(mp, None, raw, T, **crop)
    box_lo, box_hi = mp[subset].min(axis=0), mp[subset].max(axis=0)
    assert ((sensor < box_lo) | (sensor > box_hi)).all()                  # outside on every axis
    assert ((ends < box_lo) | (ends > box_hi)).any(axis=1).all()          # and every ray ends outside again
    sm = new_submap(mp, None, **crop)
    carve_equals(sm, mp, None, raw, T, rm, what=f"corner {sign:+.0f}")
    assert rm.sum() >= 10 and not rm[~subset].any()


# ---------------------------------------------------------------------------------------------------------------
# c. launch and sort boundaries
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_scan", [1, 63, 64, 65, 255, 256, 257])
def test_scan_sizes(n_scan):
    mp, _ = make_map(5000, 41, False)
    run_case(mp, None, make_rays(257, 42)[:n_scan], pose(), what=f"scan of {n_scan}")


@pytest.fixture(scope="module")
def big_map():
    return make_map(262145 - N_PLANTED, 43, True)


@pytest.mark.parametrize("n_map", [1, 255, 256, 257, 65537, 262144 + 1])
def test_map_sizes(n_map, big_map):
    """scan_flags and k_compact change their block counts along the way; at 262 144 points the whole-map sort switches to Onesweep
    (the index range of a +-3 m map needs far fewer than 40 key bits)."""
    mp = big_map[0][:n_map]
    mn = big_map[1][:n_map] if n_map >= 65537 else None     # the small maps must lose their planted points whatever the normals
    run_case(mp, mn, make_rays(300, 44), pose(), crop=("Base",), what=f"map of {n_map}")


def test_index_range_beyond_40_key_bits_stays_on_the_default_sort():
    """Two clusters a thousand kilometres apart on two axes under an unbounded volume, carving voxel 0.05: 2e7 indices per axis, 56
    key bits with the third — the same map size as the Onesweep case above, on rocPRIM's default sort."""
    n = 262144 + 1
    mp, _ = make_map(n - N_PLANTED, 45, False)
    mp[n // 2:, :2] += 1.0e6
    ext = np.ptp(np.floor(mp / 0.05), axis=0) + 1
    assert 2.0 ** 41 < ext.prod() < 9e18
    run_case(mp, None, make_rays(300, 46), pose(), crop=("Base",), voxel=0.05, what="56 key bits")


def test_index_range_that_does_not_pack_is_refused_and_the_map_untouched():
    mp, mn = make_map(4000, 47, True)
    mp[N_PLANTED:] = np.where(mp[N_PLANTED:] > 0, 1.0e5, -1.0e5) + mp[N_PLANTED:]     # clusters at +-1e5 m on all three axes
    ext = np.ptp(np.floor(mp / 0.05), axis=0) + 1
    assert ext.prod() >= 9e18
    sm = new_submap(mp, mn, crop=("Base",))
    with pytest.raises(RuntimeError, match=f"o3s_status {_lib.ERR_BAD_ARGUMENT}$"):
        sm.carve(make_rays(300, 48), pose(), voxel_size=0.05)
    gp, gn = sm.getMapPointCloud()
    assert same_bits(gp, mp) and same_bits(gn, mn)
    # the same map carves at a voxel size whose index range packs
    rm, _ = oracle_carve(mp, mn, make_rays(300, 48), pose(), crop=("Base",), voxel=0.3)
    carve_equals(sm, mp, mn, make_rays(300, 48), pose(), rm, voxel=0.3, what="after the refusal")


# ---------------------------------------------------------------------------------------------------------------
# d. ray edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_normals", [True, False])
def test_ray_edges(with_normals):
    """One scan: a zero-length ray, exact duplicates, rays along the axes from a sensor on a voxel corner (every stop is a
    nominal multiple of the voxel: the floor flips on the last bit of the repeated addition), negative coordinates, and a ray
    whose squared length overflows (direction 0: every stop is the sensor)."""
    sensor = np.array([0.3, -0.2, 0.1])
    T = syn.make_T(None, sensor)                          # axis-parallel rays stay axis-parallel
    mp, mn = make_map(30000, 51, with_normals, sensor=sensor)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    raw = np.concatenate([np.zeros((1, 3)), axes * 2.5, axes * 2.5, axes[:, [1, 2, 0]] * np.array([[0.1 * 17]]), [[1e300, 0.0, 0.0]],
                          make_rays(100, 52), [[-1.7, -2.3, -0.9], [-1.7, -2.3, -0.9]]])
    scan_map, _ = orc.transform_cloud(T, raw, None)
    with np.errstate(over="ignore"):
        assert same_bits(scan_map[0], sensor) and np.isinf(((scan_map[19] - sensor) ** 2).sum())
    _, rm, _ = run_case(mp, mn, raw, T, what="ray edges")
    only_axes, _ = oracle_carve(mp, mn, raw[1:19], T)
    assert only_axes.sum() >= 3                           # the corner rays carve on their own account


# ---------------------------------------------------------------------------------------------------------------
# e. non-finite input
# ---------------------------------------------------------------------------------------------------------------
def nonfinite_case(with_normals):
    """A sensor in the all-positive octant whose finite rays all point away from the index-0 planes, and map points planted in the
    carving voxels whose index is 0 on one, two or three axes and the sensor's on the others — the voxels a NaN coordinate that
    is converted to index 0 would name.  No finite ray comes near them."""
    sensor = np.array([1.23, 0.87, 0.64])
    T = pose(sensor)
    rng = np.random.default_rng(61)
    si = np.floor(sensor / 0.1)
    planted = []
    for mask in [(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]:
        idx = si * np.array(mask)
        planted.append((idx + 0.5) * 0.1 + rng.uniform(-0.03, 0.03, (6, 3)))
    planted = np.concatenate(planted)
    mp = np.concatenate([planted, rng.uniform(-3.0, 3.0, (5000, 3))])
    mn = None
    if with_normals:
        mn = rng.normal(size=mp.shape)
        mn /= np.linalg.norm(mn, axis=1, keepdims=True)
    d = np.abs(rng.normal(size=(200, 3))) + 0.05
    ends = sensor + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.0, 3.0, (200, 1))
    finite = (ends - sensor) @ T[:3, :3]
    return sensor, T, mp, mn, len(planted), finite


BIG = 1.79e308   # finite; the sum of two of its products with rotation entries overflows


@pytest.mark.parametrize("with_normals", [False, True])
def test_non_finite_rays_name_no_voxel(with_normals):
    """Infinite and NaN raw coordinates (the homogeneous row turns both into NaN map-frame points), and finite raw coordinates whose
    transform overflows into map-frame points with one or two INFINITE coordinates: length inf, direction NaN on those axes and 0 on
    the others.  A stop whose coordinates are not finite, or whose index does not fit int32, names no voxel: the carve equals the
    carve of the same scan with those rows left out."""
    sensor, T, mp, mn, n_planted, finite = nonfinite_case(with_normals)
    bad = np.array([[np.inf, 0.0, 0.0], [-np.inf, np.inf, 0.0], [np.nan, 1.0, 1.0],
                    [BIG, 0.0, BIG], [-BIG, 0.0, -BIG], [0.0, BIG, BIG], [BIG, BIG, 0.0], [BIG, -BIG, BIG], [-BIG, BIG, BIG], [BIG, BIG, -BIG],
                    [1e300, 1e300, 1e300], [3.0e10, -3.0e10, 3.0e10]])
    tb, _ = orc.transform_cloud(T, bad, None)
    n_inf = np.isinf(tb).sum(axis=1)
    assert np.isnan(tb[:3]).all() and (n_inf[3:10] >= 1).all() and (n_inf == 1).any() and (n_inf == 2).any() and np.isfinite(tb[10:]).all()
    where = np.array([7, 30, 31, 64, 65, 100, 128, 150, 151, 190, 198, 199])
    raw = np.insert(finite, where - np.arange(len(where)), bad, axis=0)
    assert len(raw) == 212 and same_bits(np.delete(raw, where, axis=0), finite)
    # the reference: the finite rows alone, plus the two finite rows of `bad` (an overflowing squared length; stops beyond int32)
    rm, _ = oracle_carve(mp, mn, np.concatenate([finite, bad[10:]]), T, crop=("Base",), max_len=40.0)
    assert not rm[:n_planted].any() and rm.sum() >= 10
    sm = new_submap(mp, mn, crop=("Base",))
    carve_equals(sm, mp, mn, raw, T, rm, max_len=40.0, what="non-finite rays")


@pytest.mark.parametrize("with_normals", [False, True])
def test_map_point_with_a_nan_coordinate_survives_in_place(with_normals):
    """Under an unbounded volume a map point with a NaN coordinate is in the subset and has no voxel: it survives where it is and
    changes nothing for the others — also when its finite coordinates lie in a voxel column that a ray crosses at index 0."""
    sensor, T, mp, mn, n_planted, finite = nonfinite_case(with_normals)
    # one extra ray along -x through the voxels (k, 10, 5): it crosses index 0 on x at y = 1.05, z = 0.55
    T2 = pose(np.array([2.05, 1.05, 0.55]))
    extra = (np.array([[-2.0, 1.05, 0.55]]) - T2[:3, 3]) @ T2[:3, :3]
    raw = np.concatenate([finite, extra])
    rm0, _ = oracle_carve(mp, mn, raw, T2, crop=("Base",))
    assert rm0.sum() >= 10
    probe = np.array([[0.05, 1.05, 0.55]])                 # a finite point there IS carved (no normals), so the column is crossed
    assert orc.carve(orc.transform_cloud(T2, raw, None)[0], probe, None, T2[:3, 3], 0.1, 20.0, 0.1, 0.5).all()
    nan_pts = np.array([[np.nan, 1.05, 0.55], [np.nan, np.nan, np.nan], [0.05, np.nan, 0.55], [np.inf, 1.05, 0.55], [-np.inf, 0.0, 0.0]])
    at = np.array([0, 100, 2000, 2001, len(mp)])
    mp2 = np.insert(mp, at, nan_pts, axis=0)
    mn2 = None if mn is None else np.insert(mn, at, np.tile([[-1.0, 0.0, 0.0]], (len(at), 1)), axis=0)
    sm = new_submap(mp2, mn2, crop=("Base",))
    if not same_bits(sm.getMapPointCloud()[0], mp2):
        pytest.fail("setMapPointCloud did not keep the non-finite points")
    rm = np.insert(rm0, at, False)
    carve_equals(sm, mp2, mn2, raw, T2, rm, what="NaN map points")
    only = new_submap(nan_pts, None, crop=("Base",))       # a subset in which no point has a voxel: nothing to carve, nothing refused
    assert only.carve(raw, T2) == 0 and same_bits(only.getMapPointCloud()[0], nan_pts)


# ---------------------------------------------------------------------------------------------------------------
# f. state after a carve
# ---------------------------------------------------------------------------------------------------------------
def small_trajectory(n_scans=4, n_pts=8000, seed=7):
    world = syn.make_world(9000.0, seed=seed)
    out = []
    for k in range(n_scans):
        T = syn.make_T(syn.rot_axis_angle([0.1, 0.2, 1.0], 0.3 * k + 0.1), np.array([-3.0 + 0.3 * k, 1.0 + 0.15 * k, 1.5]))
        sp, sn = syn.make_scan(world, n_pts, T, radius=7.0, sigma=0.01, seed=300 + k)
        out.append((sp.astype(np.float64), sn.astype(np.float64), T))
    return out


def carve_pose(T):
    """The pose a carve is made from: the insert's, moved, so that its rays cut through what the inserts mapped."""
    T2 = np.array(T, np.float64)
    T2[:3, 3] += np.array([0.5, -0.4, 0.2])
    return T2


def test_carve_everything_then_carve_again_then_insert():
    rng = np.random.default_rng(71)
    mp = rng.uniform(0.1, 3.0, (3000, 3))                  # all of it, and the sensor, in voxel (0, 0, 0) of a 100 m grid
    T = pose(np.array([1.0, 1.5, 0.5]))
    raw = make_rays(50, 72)
    sm, rm, _ = run_case(mp, None, raw, T, voxel=100.0, what="one fat voxel")
    assert rm.all() and len(sm) == 0
    assert sm.carve(raw, T, voxel_size=100.0) == 0 and len(sm) == 0
    sp, _, Ts = small_trajectory(1)[0]
    assert sm.insertScan(sp, None, Ts)
    op, _ = oracle_insert(None, None, sp, None, Ts, 0.1, "MaxRadius", (10.0, 0.0, 0.0))
    gp, gn = sm.getMapPointCloud()
    assert len(op) > 1000 and same_bits(gp, op) and gn is None


def test_carve_keeps_the_survivors_colours():
    voxel, kind, params = 0.15, "MaxRadius", (10.0, 0.0, 0.0)
    sm = Submap(voxel, co.croppingVolumeFactory(kind, *params))
    rng = np.random.default_rng(73)
    sp, sn, T = small_trajectory(1, 12000)[0]
    assert sm.insertScanColored(sp, sn, rng.uniform(0, 1, sp.shape), T)
    mp, mn = sm.getMapPointCloud()
    mc = sm.getMapColors()
    T2 = carve_pose(T)
    raw = sp[:3000]
    rm, _ = oracle_carve(mp, mn, raw, T2, crop=(kind,) + params, centre=tuple(T[:3, 3]), min_dot=0.2)
    carve_equals(sm, mp, mn, raw, T2, rm, min_dot=0.2, what="coloured map")
    assert rm.sum() > 20 and sm.hasColors() and same_bits(sm.getMapColors(), mc[~rm])


def test_carve_completes_a_pending_insert_first():
    """o3s_submap_insert_processed leaves the merge insert enqueued; a carve that comes next works on the map AFTER it."""
    from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan

    wide, narrow = ("MaxRadius", 10.0), ("MaxRadius", 8.0)
    traj = small_trajectory(3)
    a = Submap(0.1, co.croppingVolumeFactory(*wide))
    b = Submap(0.1, co.croppingVolumeFactory(*wide))
    ps = ProcessedScan()
    pending = []
    for k, (sp, sn, T) in enumerate(traj):
        ps.preprocess(co.croppingVolumeFactory(*wide), 0.1, co.croppingVolumeFactory(*narrow), sp, sn)
        mp_, mn_ = ps.merge
        a.insertProcessed(ps, T)
        lo, hi = a.size_bounds()                            # never waits
        pending.append(hi > lo)
        b.insertScan(mp_, mn_, T)                           # the insert that waits
        if k == 0:
            assert len(a) == len(b)
    assert pending[-1], pending                             # the last insert was still pending when the carve was issued
    mp, mn = b.getMapPointCloud()
    sp, sn, T = traj[-1]
    T2 = carve_pose(T)
    raw = sp[:3000]
    rm, _ = oracle_carve(mp, mn, raw, T2, crop=wide, centre=tuple(T[:3, 3]), min_dot=0.2)
    carve_equals(a, mp, mn, raw, T2, rm, min_dot=0.2, what="pending insert")
    assert rm.sum() > 20


@pytest.fixture(params=["hinted", "measured", "hint_miss"])
def range_path(request, monkeypatch):
    """The three index-range paths of the voxelising insert (tests/test_gpu_submap.py, index_range_path), for this test alone."""
    monkeypatch.delenv("O3S_NO_HINT", raising=False)
    monkeypatch.delenv("O3S_HINT_MISS", raising=False)
    if request.param == "hinted":
        yield request.param
        return
    monkeypatch.setenv("O3S_NO_HINT" if request.param == "measured" else "O3S_HINT_MISS", "1")
    with _lib.variant("hooks"):
        yield request.param


@pytest.mark.parametrize("with_normals", [True, False])
def test_inserts_after_a_carve_sort_once_and_then_merge_again(with_normals, range_path):
    """A carve keeps the order of the survivors but not the voxel layout the merge insert relies on: the next insert sorts, the one
    after merges again — and the map equals the oracle's after every step."""
    voxel, kind, params = 0.15, "MaxRadius", (9.0, 0.0, 0.0)
    traj = small_trajectory(5)
    sm = Submap(voxel, co.croppingVolumeFactory(kind, *params))
    mp = mn = None
    stats = []

    def insert(k):
        nonlocal mp, mn
        sp, sn, T = traj[k]
        sn = sn if with_normals else None
        assert sm.insertScan(sp, sn, T)
        mp, mn = oracle_insert(mp, mn, sp, sn, T, voxel, kind, params)
        gp, gn = sm.getMapPointCloud()
        assert same_bits(gp, mp) and (gn is None) == (mn is None) and (mn is None or same_bits(gn, mn)), k
        stats.append(sm.insert_stats())

    insert(0)
    insert(1)
    sp, sn, T = traj[2]
    T2 = carve_pose(T)
    rm, _ = oracle_carve(mp, mn, sp[:3000], T2, crop=(kind,) + params, centre=tuple(traj[1][2][:3, 3]), min_dot=0.2)
    carve_equals(sm, mp, mn, sp[:3000], T2, rm, min_dot=0.2, what="between inserts")
    mp, mn = mp[~rm], (None if mn is None else mn[~rm])
    insert(2)
    insert(3)
    insert(4)
    print("insert_stats (merged, sorted, fell_back) after each insert:", stats)
    if range_path == "hinted":
        assert stats[0] == (0, 1, 0) and stats[1] == (1, 1, 0)
        assert stats[2] == (1, 2, 0)                       # the insert after the carve sorts
        assert stats[3] == (2, 2, 0) and stats[4] == (3, 2, 0)   # and the following ones merge again
    elif range_path == "measured":
        assert stats[-1][0] == 0 and stats[-1][2] == 0


def test_set_reference_after_a_carve_equals_the_host_path_on_the_survivors():
    voxel, wide = 0.12, ("MaxRadius", 10.0)
    traj = small_trajectory(3, 15000)
    sm = Submap(voxel, co.croppingVolumeFactory(*wide))
    for sp, sn, T in traj[:2]:
        sm.insertScan(sp, sn, T)
    mp, mn = sm.getMapPointCloud()
    sp, sn, T = traj[2]
    T2 = carve_pose(T)
    rm, _ = oracle_carve(mp, mn, sp[:4000], T2, crop=wide, centre=tuple(traj[1][2][:3, 3]), min_dot=0.2)
    carve_equals(sm, mp, mn, sp[:4000], T2, rm, min_dot=0.2, what="before set_reference")
    mp, mn = mp[~rm], mn[~rm]
    cfg = IcpConfig()
    a, b = ICP(cfg), ICP(cfg)
    n_patch = sm.set_reference(co.croppingVolumeFactory("MaxRadius", 5.0), T, a)
    mask = orc.crop_mask(orc.make_cropper("MaxRadius", 5.0, centre=T[:3, 3]), mp)
    assert n_patch == int(mask.sum()) and 1000 < n_patch < len(mp)
    xyzw, n32 = orc.o3d_to_pm(mp[mask], mn[mask])
    assert b.init_reference(xyzw[:, :3], n32)
    assert np.array_equal(a.reference_mean(), b.reference_mean())
    T_init = syn.perturb_pose(T, 0.05, 1.0, seed=4)
    s32, sn32 = sp.astype(np.float32), sn.astype(np.float32)
    Ta, Tb = a.compute(s32, sn32, T_init), b.compute(s32, sn32, T_init)
    assert np.array_equal(Ta, Tb) and a.stats.iterations == b.stats.iterations
