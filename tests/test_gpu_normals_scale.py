"""Normal estimation (k_normals in csrc/normals_dev.h) at sweep and map size and across the grid search's paths, against the exact
neighbour lists of tests/normals_ref.py and the oracle's back half (oracle.normals_from_neighbours).  MI355X only.

Contract of every case: neighbour lists bit-exact; normal components within 1e-9 of the oracle's on the reference lists (acos / cos
come from different fp64 math libraries on the two sides); unit length to 1e-12; oriented towards the origin.

The hooks build prints one O3S_PRINT_NGRID line per grid build (N, extent, cell0, target rho, final cell, origin, dims, occupied
cells, re-size taken, 2^24-cap steps, known bounds) and one per launch (the k_normals<K> instantiation).  The cases are chosen so
that the lines and the reference lists show each path taken: re-size taken and not, the cap loop, every K, and kept neighbours in
ring >= 2 (inner rows), ring >= 4 (face rows longer than one batch of eight cells) and in rings clipped by the grid's edge."""
import contextlib
import os
import tempfile

import numpy as np
import pytest

import normals_ref as nr
from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-9
PARAMS = [(1.0, 10), (1.0, 5), (0.5, 10), (3.0, 20), (2.0, 20)]      # the reference's parameter files
K_SIZES = (6, 8, 10, 12, 16, 24, 32)                                  # k_normals instantiations


# ---- device runs ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _environ(values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _parse(text):
    """[(grid line as a dict, launched K)] of the O3S_PRINT_NGRID lines, in order."""
    out, grid = [], None
    for ln in text.splitlines():
        if ln.startswith("o3s ngrid:"):
            t, grid, i = ln.split()[2:], {}, 0
            while i < len(t):
                w = 3 if t[i] in ("origin", "dims") else 1
                v = [float(x) for x in t[i + 1:i + 1 + w]]
                grid[t[i]] = v if w == 3 else v[0]
                i += 1 + w
        elif ln.startswith("o3s normals:"):
            t = ln.split()
            out.append((grid, int(t[t.index("K") + 1])))
            grid = None
    return out


def device(p, radius, knn, rho=None, evidence=False):
    """(normals, lists, records): from the product library, or from the hooks build with the O3S_PRINT_NGRID line (and O3S_NRM_RHO
    when given) when evidence is asked for.  records: [(grid dict, K)] of the call (None on the product library)."""
    if rho is None and not evidence:
        gn, gi = co.estimateNormals(p, radius, knn, want_neighbours=True)
        return gn, gi, None
    env = {"O3S_PRINT_NGRID": "1"}
    if rho is not None:
        env["O3S_NRM_RHO"] = repr(float(rho))
    with tempfile.TemporaryFile() as f, _environ(env), _lib.variant("hooks"):
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            gn, gi = co.estimateNormals(p, radius, knn, want_neighbours=True)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        recs = _parse(f.read().decode())
    assert len(recs) == 1 and recs[0][0] is not None, recs
    return gn, gi, recs


# ---- references -------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(key, p, radius, knn):
    """Exact lists and the oracle's normals on them (module cache: several cases share a cloud and its parameters)."""
    if key not in _REF:
        st = nr.Stats()
        lists = nr.neighbour_lists(p, radius, knn, stats=st)
        _REF[key] = (lists, orc.normals_from_neighbours(p, lists), st.fallback)
    return _REF[key]


def check(p, gn, gi, ref_lists, ref_normals):
    assert np.array_equal(gi, ref_lists), f"{int((gi != ref_lists).any(axis=1).sum())} of {p.shape[0]} lists differ"
    err = np.abs(gn - ref_normals).max(axis=1)
    assert err.max() <= TOL, f"{int((err > TOL).sum())} points beyond {TOL}: worst {err.max():.3e} at {int(err.argmax())}"
    assert np.abs(np.linalg.norm(gn, axis=1) - 1.0).max() <= 1e-12
    assert ((gn * (-p)).sum(axis=1) >= 0.0).all()


def cell_of(p, grid):
    """The cell of every point: the expression that keyed the grid (floor((p - origin) / cell) per axis)."""
    return np.floor((p - np.asarray(grid["origin"])) / grid["cell"]).astype(np.int64)


def rings(p, lists, grid):
    """Chebyshev ring of each point's farthest kept neighbour (cells of the printed grid), and whether that ring was clipped by
    the grid's edge.  A kept neighbour in ring r proves that the kernel walked ring r."""
    c = cell_of(p, grid)
    dims = np.asarray(grid["dims"], np.int64)
    assert (c >= 0).all() and (c < dims).all()
    r = np.zeros(p.shape[0], np.int64)
    for s in range(lists.shape[1]):
        j = lists[:, s]
        ok = j >= 0
        d = np.abs(c[np.where(ok, j, 0)] - c).max(axis=1)
        r = np.maximum(r, np.where(ok, d, 0))
    clipped = ((c - r[:, None]) < 0).any(axis=1) | ((c + r[:, None]) > dims - 1).any(axis=1)
    return r, clipped & (r >= 2)


# ---- clouds -----------------------------------------------------------------------------------------------------------------
_CLOUD = {}


def _world():
    if "world" not in _CLOUD:
        _CLOUD["world"] = syn.make_world(60000.0, seed=11)
    return _CLOUD["world"]


def pose(name):
    world = _world()
    if name == "aisle":
        return syn.corridor_pose(world, 0, 0.25)
    L, W, _ = world.size      # a room corner: 0.7 m from two walls, the floor 1.5 m below
    return syn.make_T(syn.rot_axis_angle([0, 0, 1], 0.7), np.array([L / 2 - 0.7, W / 2 - 0.7, 1.5]))


def sweep(name, seed=300):
    """A full 64 x 2048 ray-cast sweep in the sensor frame (points only: the scan arrives without normals)."""
    key = ("sweep", name, seed)
    if key not in _CLOUD:
        sp, _ = syn.make_lidar_scan(_world(), pose(name), 64, 2048, max_range=60.0, sigma=0.01, seed=seed)
        _CLOUD[key] = np.ascontiguousarray(sp, np.float64)
    return _CLOUD[key]


def host_crop_voxel(sp, radius=30.0, voxel=0.15):
    """The scan pipeline's crop and voxel steps on the host: what estimation sees inside preprocess()."""
    m = orc.crop_mask(orc.make_cropper("MaxRadius", radius), sp)
    vp, _, idx = orc.voxel_downsample_o3d(voxel, sp[m], None)
    return np.ascontiguousarray(vp[np.lexsort((idx[:, 0], idx[:, 1], idx[:, 2]))])


def cloud(name, kind):
    key = ("cloud", name, kind)
    if key not in _CLOUD:
        _CLOUD[key] = sweep(name) if kind == "raw" else host_crop_voxel(sweep(name))
    return _CLOUD[key]


def lattice(n, pitch, seed, planar=False, offset=(2.0, -3.0, 0.5)):
    g = np.arange(n) * pitch
    if planar:
        x, y = np.meshgrid(g, g, indexing="ij")
        p = np.c_[x.ravel(), y.ravel(), np.zeros(x.size)] + np.array(offset)
    else:
        x, y, z = np.meshgrid(g, g, g, indexing="ij")
        p = np.c_[x.ravel(), y.ravel(), z.ravel()] + np.array(offset)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(p.shape[0])])


# ---- cases ------------------------------------------------------------------------------------------------------------------
_RUN = {}


def sweep_case(name, kind, radius, knn):
    """Product run + hooks run with the line on (same bits), checked against the reference."""
    key = ("sweep", name, kind, radius, knn)
    if key not in _RUN:
        p = cloud(name, kind)
        gn, gi, _ = device(p, radius, knn)
        hn, hi, recs = device(p, radius, knn, evidence=True)
        assert np.array_equal(hi, gi) and np.array_equal(hn.view(np.uint64), gn.view(np.uint64))   # the line changes no bit
        ref_l, ref_n, _ = reference((name, kind, radius, knn), p, radius, knn)
        check(p, gn, gi, ref_l, ref_n)
        _RUN[key] = (p, ref_l, recs)
    return _RUN[key]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name", ["aisle", "corner"])
@pytest.mark.parametrize("kind", ["raw", "cropped"])
def test_sweeps_match_the_reference(name, kind):
    for radius, knn in PARAMS:
        p, _, recs = sweep_case(name, kind, radius, knn)
        if kind == "raw":
            assert p.shape[0] > 110_000
        assert recs[0][1] == min(k for k in K_SIZES if k >= knn)


def kb_case(knn, which):
    """Every K boundary on the cropped, voxelised aisle sweep: a radius that fills most lists and one that cuts them."""
    key = ("kb", knn, which)
    if key not in _RUN:
        p = cloud("aisle", "cropped")
        radius = 3.0 if which == "fill" else 0.3
        gn, gi, recs = device(p, radius, knn, evidence=True)
        ref_l, ref_n, _ = reference(("aisle", "cropped", radius, knn), p, radius, knn)
        check(p, gn, gi, ref_l, ref_n)
        full = (ref_l >= 0).sum(axis=1) == knn
        _RUN[key] = (full.mean(), recs)
    return _RUN[key]


@pytest.mark.timeout(600)
@pytest.mark.parametrize("knn", [1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 24, 25, 32])
def test_every_k_boundary(knn):
    fill, recs = kb_case(knn, "fill")
    assert fill > 0.9 and recs[0][1] == min(k for k in K_SIZES if k >= knn)
    cut, _ = kb_case(knn, "cut")
    if knn >= 6:
        assert cut < 0.9


def lattice_case(name):
    """Power-of-two pitches: every distance and shell radius is exact, the cell edge is a multiple of the pitch and every point
    lies on its cell's closed lower faces.  O3S_NRM_RHO holds (or moves) the cell where the case needs it; the printed cell says."""
    if ("lattice", name) in _RUN:
        return _RUN[("lattice", name)]
    if name == "cube":           # cell = pitch = radius / 2: no re-size at rho 1; radius on the 2-pitch shell (the strict cut)
        p, radius, knns, rho, cell, resized = lattice(16, 0.125, seed=1), 0.25, (7, 8, 19, 20, 27, 28), 1.0, 0.125, 0
    elif name == "cube_dup":     # + six clusters of 40 copies of lattice points (on cell faces, straddled by their shells)
        base = lattice(16, 0.125, seed=2)
        dup = np.repeat(base[[5, 77, 1000, 2047, 3001, 4095]], 40, axis=0)
        p = np.concatenate([base, dup])[np.random.default_rng(3).permutation(base.shape[0] + dup.shape[0])]
        radius, knns, rho, cell, resized = 0.25, (8, 20, 32), 1.0, 0.125, 0
    elif name == "cube_ring2":   # cell0 = 2 pitches, 8 points a cell -> re-sized to 1 pitch at rho 2; the 2-pitch shell (ring 2) ties
        p, radius, knns, rho, cell, resized = lattice(16, 0.125, seed=4), 0.5, (28, 32), 2.0, 0.125, 1
    else:                        # planar, cell = pitch; shells of 4: knn on both sides, radius on the 2-pitch shell
        p, radius, knns, rho, cell, resized = lattice(48, 0.25, seed=5, planar=True), 0.5, (5, 6, 9, 10, 13, 14), 1.0, 0.25, 0
    p = np.ascontiguousarray(p)
    res = []
    for knn in knns:
        gn, gi, recs = device(p, radius, knn, rho=rho)
        g = recs[0][0]
        assert g["cell"] == cell and g["resized"] == resized, g
        assert (cell_of(p, g) * cell + np.asarray(g["origin"]) == p).all()     # on the closed faces, exactly
        ref_l, ref_n, fb = reference(("lattice", name, radius, knn), p, radius, knn)
        check(p, gn, gi, ref_l, ref_n)
        res.append((knn, p, ref_l, recs, fb))
    _RUN[("lattice", name)] = res
    return res


@pytest.mark.parametrize("name", ["cube", "cube_dup", "cube_ring2", "plane"])
def test_lattice_ties(name):
    res = lattice_case(name)
    if name == "cube_ring2":
        for knn, p, ref_l, recs, _ in res:
            r, _ = rings(p, ref_l, recs[0][0])
            assert (r >= 2).sum() > 1000      # the tied 2-pitch shell sits exactly on the row bounds of ring 2
    if name == "cube":
        knn, p, ref_l, _, _ = res[-1]         # 28: 27 points inside two pitches, the 28th exactly on the radius and cut
        assert knn == 28 and ((ref_l >= 0).sum(axis=1) == 27).sum() > 1000
    if name in ("cube", "cube_dup"):
        assert sum(fb for *_, fb in res) > 0     # ties the reference could not certify from the kd-tree's candidates alone


def rho_case(rho):
    key = ("rho", rho)
    if key not in _RUN:
        p = cloud("aisle", "raw")
        gn, gi, _ = device(p, 1.0, 10)
        hn, hi, recs = device(p, 1.0, 10, rho=rho)
        assert np.array_equal(hi, gi) and np.array_equal(hn.view(np.uint64), gn.view(np.uint64))
        _RUN[key] = (p, recs)
    return _RUN[key]


@pytest.mark.timeout(600)
def test_any_cell_size_gives_the_same_bits():
    """Any cell keeps the search exact: O3S_NRM_RHO from 0.05 to 1e4 gives the default run's lists and normals bit for bit."""
    cells = [rho_case(rho)[1][0][0]["cell"] for rho in (0.05, 1.0, 4.0, 12.0, 64.0, 1e4)]
    assert len(set(cells)) >= 4 and min(cells) < 0.25 and max(cells) == 1.0    # 1e4 is held at cell_max = the radius


def edge_case(name):
    if ("edge", name) in _RUN:
        return _RUN[("edge", name)]
    rng = np.random.default_rng(sum(map(ord, name)))
    knns, radius = (10,), 1.0
    if name == "far_clusters":   # kilometres apart: the ext / 512 floor and the ext / 1024 clamp
        a = np.c_[rng.uniform(-3, 3, (3000, 2)), rng.normal(0, 0.02, 3000)] + np.array([1.0, 2.0, 0.0])
        b = np.c_[rng.normal(0, 0.02, 3000), rng.uniform(-3, 3, (3000, 2))] + np.array([4000.0, -1500.0, 20.0])
        p = np.concatenate([a, b])
    elif name == "volume":       # a filled 30 m cube: cell0 = 0.1 m asks for 302^3 cells > 2^24
        p, radius = rng.uniform(-15.0, 15.0, (400_000, 3)), 0.2
    elif name == "plane":
        p = np.c_[rng.uniform(-5, 5, (5000, 2)), np.full(5000, 2.0)]
    elif name == "line":
        p = np.c_[rng.uniform(0, 30, 3000), np.full(3000, 1.0), np.full(3000, 2.0)]
    elif name == "identical":
        p, knns = np.tile([[1.0, 2.0, 3.0]], (500, 1)), (10, 32)
    else:
        n = int(name[1:])       # "n1", "n2", "n3"
        p, knns = np.array([[0.5, -1.0, 2.0], [0.5, -0.75, 2.0], [0.25, -1.0, 2.25]])[:n], (1, 2, 3, 10)
    p = np.ascontiguousarray(p, np.float64)
    res = []
    for knn in knns:
        gn, gi, recs = device(p, radius, knn, evidence=True)
        ref_l, ref_n, _ = reference(("edge", name, radius, knn), p, radius, knn)
        check(p, gn, gi, ref_l, ref_n)
        res.append((p, ref_l, recs))
    _RUN[("edge", name)] = res
    return res


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name", ["far_clusters", "volume", "plane", "line", "identical", "n1", "n2", "n3"])
def test_grid_edges(name):
    res = edge_case(name)
    g = res[0][2][0][0]
    if name == "far_clusters":
        assert g["cell"] >= g["ext"] / 1024 and g["cell0"] < g["ext"] / 512
    if name == "volume":
        assert g["cap_steps"] >= 1 and np.prod(g["dims"]) <= 2 ** 24
    if name == "identical":
        assert g["ext"] == 0 and (res[0][1] >= 0).all()


@pytest.mark.timeout(900)
def test_path_evidence():
    """The printed lines and the reference lists show every path of the sizing and the ring walk taken at least once."""
    seen_k, resized, cap = set(), set(), 0
    for knn in (1, 7, 9, 11, 13, 17, 25):
        seen_k.add(kb_case(knn, "fill")[1][0][1])
    for name in ("cube", "cube_ring2", "plane"):
        for *_, recs, _ in lattice_case(name):
            resized.add(int(recs[0][0]["resized"]))
    cap = max(cap, edge_case("volume")[0][2][0][0]["cap_steps"], rho_case(0.05)[1][0][0]["cap_steps"])
    max_ring, clipped, inner = 0, 0, 0
    for (name, radius, knn, rho) in [("aisle", 3.0, 20, None), ("corner", 3.0, 20, None), ("aisle", 1.0, 10, 0.05)]:
        p, ref_l, recs = sweep_case(name, "raw", radius, knn)
        if rho is not None:
            recs = rho_case(rho)[1]
        g = recs[0][0]
        resized.add(int(g["resized"]))
        r, c = rings(p, ref_l, g)
        max_ring, clipped, inner = max(max_ring, int(r.max())), clipped + int(c.sum()), inner + int((r >= 2).sum())
    print(f"normals paths: K {sorted(seen_k)} resized {sorted(resized)} cap steps {cap} max ring {max_ring} "
          f"ring>=2 {inner} clipped {clipped}")
    assert seen_k >= {6, 8, 10, 12, 16, 24, 32}
    assert resized == {0, 1}
    assert cap >= 1
    assert inner > 0 and max_ring >= 4 and clipped > 0


# ---- the scan pipeline with estimation --------------------------------------------------------------------------------------
@pytest.fixture(params=["hinted", "measured", "miss"])
def index_range_path(request, monkeypatch):
    """test_gpu_submap.py's fixture: the voxel index range hinted by the cropping volume (product library), measured on the device
    (O3S_NO_HINT) and a hint that nothing fits in (O3S_HINT_MISS: the status word trips and the call is repeated measuring)."""
    monkeypatch.delenv("O3S_NO_HINT", raising=False)
    monkeypatch.delenv("O3S_HINT_MISS", raising=False)
    if request.param == "hinted":
        yield request.param
        return
    monkeypatch.setenv("O3S_NO_HINT" if request.param == "measured" else "O3S_HINT_MISS", "1")
    with _lib.variant("hooks"):
        yield request.param


WIDE, NARROW, VOXEL = ("MaxRadius", 30.0), ("MaxRadius", 25.0), 0.15
_PATHS = {}


def preprocess(ps, sp, wide=WIDE):
    n_merge, n_match = ps.preprocess(co.croppingVolumeFactory(*wide), VOXEL, co.croppingVolumeFactory(*NARROW), sp, None)
    (mp, mn), (qp, qn) = ps.merge, ps.match
    assert mp.shape[0] == n_merge and qp.shape[0] == n_match
    return mp.copy(), mn.copy(), qp.copy(), qn.copy()


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


@pytest.mark.timeout(600)
def test_scan_preprocess_estimates_like_the_reference(index_range_path):
    sp = sweep("aisle")
    ps = ProcessedScan()
    ps.set_normal_estimation(1.0, 10)
    out = preprocess(ps, sp)
    mp, mn, qp, qn = out
    vp = host_crop_voxel(sp, WIDE[1], VOXEL)
    assert np.array_equal(mp, vp)
    ref_l, ref_n, _ = reference(("pre", 1.0, 10), vp, 1.0, 10)
    err = np.abs(mn - ref_n).max()
    assert err <= TOL and np.abs(np.linalg.norm(mn, axis=1) - 1.0).max() <= 1e-12 and ((mn * (-mp)).sum(axis=1) >= 0).all()
    m2 = orc.crop_mask(orc.make_cropper(*NARROW), vp)
    assert np.array_equal(qp, vp[m2]) and same_bits((qn,), (mn[m2],))
    first = _PATHS.setdefault("aisle", out)
    assert same_bits(out, first)          # the three index-range paths give the same bits


@pytest.mark.timeout(600)
def test_one_scan_object_over_sweeps_of_changing_size(index_range_path):
    """NormalsWork keeps grow-only buffers: one object fed 131 k, 20 k, 131 k (another crop) and 500 points gives what a fresh
    object gives, every time."""
    a, b = sweep("aisle"), sweep("corner")
    feeds = [(a, ("MaxRadius", 60.0)), (a[::6].copy(), WIDE), (b, WIDE), (a[::260][:500].copy(), WIDE)]
    ps = ProcessedScan()
    ps.set_normal_estimation(1.0, 10)
    for sp, wide in feeds:
        got = preprocess(ps, sp, wide)
        fresh = ProcessedScan()
        fresh.set_normal_estimation(1.0, 10)
        assert same_bits(got, preprocess(fresh, sp, wide))
    assert got[0].shape[0] < 600


# ---- map size -----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_merged_map_of_sweeps():
    """Sweeps merged in the map frame (0.6 - 1 M points), knn 10 within 1 m, against the fast reference."""
    world = _world()
    parts = []
    for k in range(7):
        T = syn.corridor_pose(world, 40 * k, 0.25)
        sp, _ = syn.make_lidar_scan(world, T, 64, 2048, max_range=60.0, sigma=0.01, seed=900 + k)
        parts.append(sp.astype(np.float64) @ T[:3, :3].T + T[:3, 3])
    p = np.ascontiguousarray(np.concatenate(parts))
    assert 600_000 <= p.shape[0] <= 1_000_000
    gn, gi, _ = device(p, 1.0, 10)
    ref_l, ref_n, _ = reference(("map", 1.0, 10), p, 1.0, 10)
    check(p, gn, gi, ref_l, ref_n)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_device_usable():
    p = lattice(8, 0.25, seed=9)
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[100, 1] = bad
        with pytest.raises(RuntimeError):
            co.estimateNormals(q, 0.5, 10)
    for radius, knn in ((0.5, 0), (0.5, 33), (0.0, 10), (float("nan"), 10), (-1.0, 10)):
        with pytest.raises(RuntimeError):
            co.estimateNormals(p, radius, knn)
    gn, gi, _ = device(p, 0.5, 10)
    ref_l, ref_n, _ = reference(("refusal", 0.5, 10), p, 0.5, 10)
    check(p, gn, gi, ref_l, ref_n)
