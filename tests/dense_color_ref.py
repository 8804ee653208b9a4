"""Plain Python / NumPy restatement of colour on the reference's dense-map path, the expectation of
tests/test_gpu_dense_map_color.py (include/dense_map/o3s_dense_map_color.h).  O3S = open3d_slam_rsl/open3d_slam/open3d_slam.

  color_range_crop   ColorRangeCropper::crop                       O3S/src/croppers.cpp:178-244
  transform_cloud    o3d_slam::transform with colours              O3S/src/helpers.cpp:283-318
  DenseColorMap      VoxelizedPointCloud / AggregatedVoxel         O3S/src/Voxel.cpp:18-114, O3S/include/open3d_slam/Voxel.hpp:47-50
                     Submap::insertScanDenseMap                    O3S/src/Submap.cpp:98-113

A dict of voxels, sequential float64 additions in input order (Python floats are IEEE doubles and nothing here is fused), voxel
key = floor(p * (1 / voxel)) in fp64 — the rule of oracle/dense_map_oracle.cpp.  Carving does not look at colours: a test takes the
keys a carve removes from the oracle's DenseMap and hands them to remove_keys()."""
import numpy as np


def color_range_crop(points, normals=None, colors=None, covariances=None, rgb_min=None, rgb_max=None):
    """(points, normals, colors, covariances): the points with rgb_min <= colour <= rgb_max in every component (inclusive, NaN fails),
    in input order; a cloud without colours is returned unchanged."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if colors is None or p.shape[0] == 0:          # !cloud.HasColors(): "*cropped = cloud"
        return p, normals, colors, covariances
    c = np.asarray(colors, np.float64).reshape(-1, 3)
    lo = np.broadcast_to(np.asarray(0.0 if rgb_min is None else rgb_min, np.float64), (3,))
    hi = np.broadcast_to(np.asarray(1.0 if rgb_max is None else rgb_max, np.float64), (3,))
    with np.errstate(invalid="ignore"):
        keep = np.all(lo <= c, axis=1) & np.all(c <= hi, axis=1)
    take = lambda a, w: None if a is None else np.asarray(a, np.float64).reshape(-1, w)[keep]
    return p[keep], take(normals, 3), c[keep], take(covariances, 9)


def max_radius_mask(points, radius):
    """MaxRadiusCroppingVolume at the identity pose (croppers.cpp:121-129): |p| <= radius, |p| = sqrt((x^2 + y^2) + z^2)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.sqrt((x * x + y * y) + z * z) <= radius


def is_near_identity(T):
    return bool(np.abs(np.asarray(T, np.float64) - np.eye(4)).max() < 1e-4)


def transform_cloud(T, points, normals=None, colors=None):
    """(points, normals, colors).  T * (x, y, z, 1) row by row as ((T0 x + T1 y) + T2 z) + T3, divided by the fourth row; normals with
    a zero in place of the one.  A pose within 1e-4 of the identity first copies the whole cloud, so points and normals come out twice
    — and `out->colors_ = cloud.colors_` leaves K colours beside 2 K points."""
    T = np.asarray(T, np.float64)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    v = []
    for r in range(4):
        s = T[r, 0] * x
        s = s + T[r, 1] * y
        s = s + T[r, 2] * z
        s = s + T[r, 3] * 1.0
        v.append(s)
    out = np.stack([v[0] / v[3], v[1] / v[3], v[2] / v[3]], axis=1)
    outn = None
    if normals is not None:
        n = np.asarray(normals, np.float64).reshape(-1, 3)
        a, b, c = n[:, 0], n[:, 1], n[:, 2]
        w = []
        for r in range(3):
            s = T[r, 0] * a
            s = s + T[r, 1] * b
            s = s + T[r, 2] * c
            s = s + T[r, 3] * 0.0
            w.append(s)
        outn = np.stack(w, axis=1)
    if is_near_identity(T):
        out = np.concatenate([p, out])
        if outn is not None:
            outn = np.concatenate([np.asarray(normals, np.float64).reshape(-1, 3), outn])
    return out, outn, (None if colors is None else np.asarray(colors, np.float64).reshape(-1, 3))


class _Voxel:
    __slots__ = ("n", "pos", "nrm", "col")

    def __init__(self):
        self.n = 0
        self.pos = [0.0, 0.0, 0.0]
        self.nrm = [0.0, 0.0, 0.0]
        # aggregatedColor_ = Eigen::Vector3d::Constant(1, 3, 1) (Voxel.hpp:50): for a fixed-size vector the first two arguments are the
        # (ignored) shape and the third the value — every colour sum starts at ONE.  Kept as the reference has it.
        self.col = [1.0, 1.0, 1.0]


class DenseColorMap:
    def __init__(self, voxel_size):
        self.voxel_size = float(voxel_size)
        self.inv = 1.0 / self.voxel_size
        self.voxels = {}                 # (x, y, z) -> _Voxel
        self.has_normals = False         # isHasNormals_
        self.has_colors = False          # isHasColors_ (sticky)
        self.n_scans_inserted = 0        # nScansInsertedDenseMap_

    def size(self):
        return len(self.voxels)

    def keys_of(self, points):
        p = np.asarray(points, np.float64).reshape(-1, 3)
        return [tuple(k) for k in np.floor(p * self.inv).astype(np.int64).tolist()]

    def insert(self, points, normals=None, colors=None):
        """VoxelizedPointCloud::insert (Voxel.cpp:66-88).  HasNormals() / HasColors() are Open3D's: as many as points, and not none."""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        N = p.shape[0]
        has_n = normals is not None and N > 0 and len(normals) == N
        has_c = colors is not None and N > 0 and len(colors) == N
        keys = self.keys_of(p)
        pl = p.tolist()
        nl = np.asarray(normals, np.float64).reshape(-1, 3).tolist() if has_n else None
        cl = np.asarray(colors, np.float64).reshape(-1, 3).tolist() if has_c else None
        for i in range(N):
            v = self.voxels.get(keys[i])
            if v is None:
                v = self.voxels[keys[i]] = _Voxel()
            for a in range(3):
                v.pos[a] += pl[i][a]
            v.n += 1
            if has_n:
                for a in range(3):
                    v.nrm[a] += nl[i][a]
                self.has_normals = True
            if has_c:
                for a in range(3):
                    v.col[a] += cl[i][a]
                self.has_colors = True

    def insert_scan(self, raw_points, raw_normals, raw_colors, T, volume_mask, rgb_min=None, rgb_max=None, carve_every=None):
        """Submap::insertScanDenseMap (Submap.cpp:98-113) up to the carve: volume crop (the mask), colour crop, transform, insert.
        Returns whether the carving gate fires for this scan (carve_every None: isPerformCarving false); the scan is counted."""
        m = np.asarray(volume_mask, bool)
        p = np.asarray(raw_points, np.float64).reshape(-1, 3)[m]
        n = None if raw_normals is None else np.asarray(raw_normals, np.float64).reshape(-1, 3)[m]
        c = None if raw_colors is None else np.asarray(raw_colors, np.float64).reshape(-1, 3)[m]
        p, n, c, _ = color_range_crop(p, n, c, None, rgb_min, rgb_max)
        tp, tn, tc = transform_cloud(T, p, n, c)
        self.insert(tp, tn, tc)
        due = carve_every is not None and self.n_scans_inserted % carve_every == 1
        self.n_scans_inserted += 1
        return due

    def remove_keys(self, keys):
        """removeKey (VoxelHashMap.hpp:128) for every key a carve named: the voxel is gone, colour sum included."""
        for k in keys:
            self.voxels.pop(tuple(int(x) for x in k), None)

    def transform(self, T):
        """Voxel.cpp:49-64: position and normal sums as points, translation + linear * v; the colour sum is copied."""
        if not self.voxels:
            return
        T = np.asarray(T, np.float64).tolist()
        for v in self.voxels.values():
            for s in (v.pos, v.nrm):
                x, y, z = s
                s[:] = [T[r][3] + ((T[r][0] * x + T[r][1] * y) + T[r][2] * z) for r in range(3)]

    def clear(self):
        self.voxels = {}                 # VoxelHashMap::clear: the flags stay

    def to_point_cloud(self):
        """(points, normals | None, colors | None, keys, counts) in ascending (z, y, x) key order; every mean is sum / count."""
        ks = sorted(self.voxels, key=lambda k: (k[2], k[1], k[0]))
        V = len(ks)
        vs = [self.voxels[k] for k in ks]
        cnt = np.array([v.n for v in vs], np.int32)
        d = cnt.astype(np.float64).reshape(V, 1)
        with np.errstate(all="ignore"):
            pts = np.array([v.pos for v in vs], np.float64).reshape(V, 3) / d
            nrm = np.array([v.nrm for v in vs], np.float64).reshape(V, 3) / d
            col = np.array([v.col for v in vs], np.float64).reshape(V, 3) / d
        keys = np.array(ks, np.int32).reshape(V, 3)
        return pts, (nrm if self.has_normals else None), (col if self.has_colors else None), keys, cnt
