"""Input builders for the edges of the crop and voxel pipelines (csrc/cloud_dev.h): clouds on and around a cropper surface, degenerate
selections, index ranges whose packed size is an exact power of two, indices far from the origin.  Plain numpy; the properties that
give the cases their names are asserted on the oracle in tests/test_cloud_edge_cases.py, and the GPU tests (tests/test_gpu_cloud_edges.py)
run the same clouds through the library."""
import numpy as np

CENTRE = (1.0, -2.0, 0.5)

# (kind, parameters): 15.0 and its square are exactly representable, 5.3 and 11.3 are not.  Several doubles x have sqrt(x) == r, and
# where the rounded r * r lies among them decides which comparison a rewrite to d^2 <= r^2 would get wrong: for 5.3 it is the largest
# of them (only `>= r` changes: the x below it), for 11.3 the middle one (`<= r` and `>= r` both change) — so the `<=` kinds get 11.3 too.
SURFACE_CASES = [
    ("MaxRadius", (15.0,)),
    ("MaxRadius", (5.3,)),
    ("MaxRadius", (11.3,)),
    ("MinRadius", (15.0,)),
    ("MinRadius", (5.3,)),
    ("MinMaxRadius", (5.3, 15.0)),
    ("MinMaxRadius", (5.3, 11.3)),
    ("Cylinder", (15.0, -3.0, 4.0)),
    ("Cylinder", (5.3, -3.1, 4.2)),
    ("Cylinder", (11.3, -3.1, 4.2)),
]


def case_id(case):
    return case[0] + "-" + "-".join(str(a) for a in case[1])


def ulp_steps(x, k):
    """x moved by k units in the last place (k integer array, |k| small), towards +inf for k > 0."""
    x = np.array(x, np.float64)
    k = np.broadcast_to(np.asarray(k), x.shape)
    for j in range(int(np.abs(k).max(initial=0))):
        m = np.abs(k) > j
        x[m] = np.nextafter(x[m], np.where(k[m] > 0, np.inf, -np.inf))
    return x


def _unit(rng, n, dims=3):
    d = rng.normal(size=(n, dims))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _nudge_largest(p, c, rng):
    """every point moved k in [-4, 4] ulps along the coordinate in which it is farthest from the centre"""
    a = np.argmax(np.abs(p - c), axis=1)
    rows = np.arange(len(p))
    p[rows, a] = ulp_steps(p[rows, a], rng.integers(-4, 5, len(p)))
    return p


def near_surface_cloud(kind, params, centre=CENTRE, n_dir=4000, n_plain=300, seed=0):
    """(points, n_near): the first n_near points lie within a few ulps of a surface of the cropper `kind(*params)` at `centre` — random
    directions scaled onto every surface and moved -4 .. 4 ulps along their largest coordinate; for the cylinder also points whose z is
    within 4 ulps of either plane; planted points at exactly the radius (kept when numpy's sqrt((dx^2 + dy^2) + dz^2) gives the radius
    back).  The rest are ordinary points around the volume."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float64)
    parts = []
    if kind == "Cylinder":
        r, z0, z1 = params
        d = _unit(rng, n_dir, 2)
        p = np.empty((n_dir, 3))
        p[:, :2] = c[:2] + r * d
        p[:, 2] = rng.uniform(z0 + 0.1, z1 - 0.1, n_dir)          # the planes compare z itself, not z - centre
        a = np.argmax(np.abs(p[:, :2] - c[:2]), axis=1)
        rows = np.arange(n_dir)
        p[rows, a] = ulp_steps(p[rows, a], rng.integers(-4, 5, n_dir))
        parts.append(p)
        for plane in (z0, z1):                                    # inside the radius, z within 4 ulps of the plane
            q = np.empty((n_dir // 4, 3))
            q[:, :2] = c[:2] + _unit(rng, len(q), 2) * rng.uniform(0.0, 0.9 * r, (len(q), 1))
            q[:, 2] = ulp_steps(np.full(len(q), plane), rng.integers(-4, 5, len(q)))
            parts.append(q)
        radii = [r]
        exact_dirs = [np.array([3.0, 4.0, 0.0]) / 5.0]
    else:
        radii = list(params)
        for r in radii:
            parts.append(_nudge_largest(c + r * _unit(rng, n_dir), c, rng))
        exact_dirs = [np.array([3.0, 4.0, 0.0]) / 5.0, np.array([2.0, 3.0, 6.0]) / 7.0]
    for r in radii:
        for d in exact_dirs:
            for sign in (1.0, -1.0):
                q = c + sign * r * d
                if kind == "Cylinder":
                    q[2] = c[2]
                dx, dy, dz = q - c
                if np.sqrt((dx * dx + dy * dy) + (0.0 if kind == "Cylinder" else dz * dz)) == r:
                    parts.append(q[None, :])
    near = np.concatenate(parts)
    near = near[rng.permutation(len(near))]
    plain = c + rng.uniform(-20.0, 20.0, (n_plain, 3))
    return np.concatenate([near, plain]), len(near)


def non_finite_points(centre=CENTRE):
    """points no voxel index is defined for (NaN, +-inf in one coordinate or all) and the centre itself: for the plain crop only"""
    c = np.asarray(centre, np.float64)
    rows = [c.copy()]
    for a in range(3):
        for v in (np.nan, np.inf, -np.inf):
            q = c + np.array([0.25, -0.5, 0.125])
            q[a] = v
            rows.append(q)
    rows.append(np.full(3, np.nan))
    rows.append(np.array([np.inf, -np.inf, np.inf]))
    return np.array(rows)


def unit_normals(n, seed=0, nan_every=0):
    rng = np.random.default_rng(1000 + seed)
    nrm = _unit(rng, n)
    if nan_every:
        nrm[::nan_every, 1] = np.nan
    return nrm


# ---- degenerate selections: N points around a MaxRadius volume ---------------------------------------------------------------------
DEGENERATE_VOLUME = ("MaxRadius", 10.0)
DEGENERATE_VOXEL = 0.25
DEGENERATE_KINDS = ["one_voxel", "own_voxel", "all_outside", "one_inside", "nan_normal_voxel"]


def generic_cloud(n, centre=CENTRE, half=7.0, seed=0):
    """(points, normals): uniform points around `centre`, most of them inside DEGENERATE_VOLUME, some exactly on cell boundaries of
    DEGENERATE_VOXEL, a few normals with a NaN"""
    rng = np.random.default_rng(seed + 7 * n)
    p = np.asarray(centre, np.float64) + rng.uniform(-half, half, (n, 3))
    p[::11] = np.round(p[::11] * 4.0) / 4.0
    nrm = _unit(rng, n)
    nrm[3::29, rng.integers(0, 3)] = np.nan
    return p, nrm


def degenerate_cloud(name, n, centre=CENTRE, seed=0):
    """(points, normals) of n points; volume DEGENERATE_VOLUME at `centre` (whose coordinates are multiples of the voxel), voxel
    DEGENERATE_VOXEL.
    one_voxel: all points in one cell, within less than half a cell of each other (one voxel for the absolute grid and for Open3D's)
    own_voxel: one point per cell, on a lattice of every second cell
    all_outside: no point inside the volume
    one_inside: exactly one, in the middle of the cloud
    nan_normal_voxel: a generic cloud in which every point of one well-filled cell has a NaN normal"""
    rng = np.random.default_rng(seed + 13 * n)
    c = np.asarray(centre, np.float64)
    v = DEGENERATE_VOXEL
    nrm = _unit(rng, n)
    if name == "one_voxel":
        p = c + np.array([3.0, -2.0, 1.0]) * v + rng.uniform(0.3, 0.7, (n, 3)) * v
    elif name == "own_voxel":
        side = int(np.ceil(n ** (1.0 / 3.0)))
        cells = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
        cells = cells[rng.permutation(n)] - side // 2
        p = c + (2.0 * cells + rng.uniform(0.3, 0.7, (n, 3))) * v
    elif name == "all_outside":
        p = c + _unit(rng, n) * rng.uniform(10.5, 14.0, (n, 1))
    elif name == "one_inside":
        p = c + _unit(rng, n) * rng.uniform(10.5, 14.0, (n, 1))
        p[n // 2] = c + np.array([0.4, 0.3, -0.2])
    elif name == "nan_normal_voxel":
        p, nrm = generic_cloud(n, centre, seed=seed)
        k = max(2, n // 10)
        where = rng.choice(n, k, replace=False)
        p[where] = c + np.array([-5.0, 2.0, 3.0]) * v + rng.uniform(0.3, 0.7, (k, 3)) * v
        nrm[where] = rng.normal(size=(k, 3))
        nrm[where, rng.integers(0, 3, k)] = np.nan
        stray = np.all(np.floor(p * (1.0 / v)) == nan_voxel_index(centre), axis=1)      # a generic point that fell into the same cell
        stray[where] = False
        nrm[stray, 0] = np.nan
    else:
        raise ValueError(name)
    return p, nrm


def nan_voxel_index(centre=CENTRE):
    """the absolute-grid index of the cell nan_normal_voxel fills with NaN normals"""
    v = DEGENERATE_VOXEL
    return np.floor((np.asarray(centre, np.float64) + (np.array([-5.0, 2.0, 3.0]) + 0.5) * v) * (1.0 / v)).astype(np.int32)


# ---- key width -------------------------------------------------------------------------------------------------------------------
POW2_ORIGIN = (-3, 5, -2)


def pow2_range(a, b, c, n_between=300, n_pass=40, seed=0):
    """(points, normals, cropper parameters (kind, radius, centre), lowest index, highest index) with voxel 1.0: one point in the
    lowest and one in the highest corner cell of an index box of 2^a x 2^b x 2^c cells at POW2_ORIGIN, n_between points in cells
    between them, and n_pass pass-through points outside a MaxRadius volume that contains the whole box.  The pass-through points
    come first, last and in the middle of the cloud."""
    rng = np.random.default_rng(seed + 100 * a + 10 * b + c)
    e = np.array([1 << a, 1 << b, 1 << c], np.int64)
    o = np.array(POW2_ORIGIN, np.int64)
    cells = o + rng.integers(0, e, (n_between, 3))
    cells = np.concatenate([o[None, :], cells, (o + e - 1)[None, :], cells[: n_between // 3]])   # some cells hold two points
    inside = cells + rng.uniform(0.25, 0.75, cells.shape)
    centre = o + e / 2.0
    radius = float(np.ceil(np.linalg.norm(e / 2.0))) + 2.0
    outside = centre + _unit(rng, n_pass) * rng.uniform(radius + 1.0, radius + 50.0, (n_pass, 1))
    k = len(inside) // 2
    p = np.concatenate([outside[:10], inside[:k], outside[10:30], inside[k:], outside[30:]])
    return p, _unit(rng, len(p)), ("MaxRadius", radius, tuple(centre)), o.astype(np.int32), (o + e - 1).astype(np.int32)


FAR_ORIGIN = (4.0e5, -3.0e5, -50.0)
FAR_VOXEL = 0.1


def far_from_origin(n=5000, seed=0):
    """a generic cloud shifted to FAR_ORIGIN: with FAR_VOXEL the indices are of magnitude 4e6 and negative on two axes"""
    p, nrm = generic_cloud(n, centre=FAR_ORIGIN, half=7.0, seed=seed)
    return p, nrm


def unpackable_cloud():
    """three points whose index extents at voxel 0.1 multiply to 8e27: the range does not pack into 63 key bits"""
    return np.array([[-1e8, -1e8, -1e8], [0.5, 0.25, -0.75], [1e8, 1e8, 1e8]])
