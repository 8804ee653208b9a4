"""Host-side mirror of o3d_slam::Submap's map-building calls over the device-resident submap (include/o3s_submap.h).
Method names follow the reference (open3d_slam/src/Submap.cpp, ScanToMapRegistration.cpp); the map cloud stays in HBM."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .cloud_ops import CropperC, _d
from .icp import ICP



def _L():
    L = _lib.lib()
    if _lib.needs_binding(L, __name__):  # once per loaded library (product or test-hook build)
        dp = C.POINTER(C.c_double)
        vp = C.c_void_p
        L.o3s_submap_create.argtypes = [C.c_int, C.c_double, C.POINTER(CropperC), C.POINTER(vp)]
        L.o3s_submap_destroy.argtypes = [vp]
        L.o3s_submap_destroy.restype = None
        L.o3s_submap_insert_scan.argtypes = [vp, dp, dp, C.c_int64, dp]
        L.o3s_submap_reserve.argtypes = [vp, C.c_int64]
        L.o3s_submap_size.argtypes = [vp]
        L.o3s_submap_size.restype = C.c_int64
        L.o3s_submap_size_bounds.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.o3s_submap_download.argtypes = [vp, dp, dp]
        L.o3s_submap_center.argtypes = [vp, dp]
        L.o3s_submap_upload.argtypes = [vp, dp, dp, C.c_int64]
        L.o3s_submap_set_reference.argtypes = [vp, C.POINTER(CropperC), dp, vp, C.POINTER(C.c_int64)]
        L.o3s_submap_patch_count.argtypes = [vp, C.POINTER(CropperC), dp, C.POINTER(C.c_int64)]
        L.o3s_submap_insert_processed.argtypes = [vp, vp, dp]
        L.o3s_submap_carve.argtypes = [vp, C.POINTER(CarvingParamsC), dp, C.c_int64, dp, C.POINTER(C.c_int64)]
        L.o3s_scan_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.o3s_scan_destroy.argtypes = [vp]
        L.o3s_scan_destroy.restype = None
        L.o3s_scan_preprocess.argtypes = [vp, C.POINTER(CropperC), C.c_double, C.POINTER(CropperC), dp, dp, C.c_int64,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.o3s_scan_get.argtypes = [vp, C.c_int, dp, dp]
        L.o3s_scan_get.restype = C.c_int64
        L.o3s_scan_set_reading.argtypes = [vp, vp]
        L.o3s_scan_set_normal_estimation.argtypes = [vp, C.c_double, C.c_int32]
        ip = C.POINTER(C.c_int32)
        L.o3s_submap_feature_params_default.argtypes = [C.POINTER(FeatureParamsC)]
        L.o3s_submap_feature_params_default.restype = None
        L.o3s_submap_compute_features.argtypes = [vp, C.POINTER(FeatureParamsC)]
        L.o3s_submap_features_size.argtypes = [vp]
        L.o3s_submap_features_size.restype = C.c_int64
        L.o3s_submap_download_features.argtypes = [vp, dp, dp, dp]
        L.o3s_submap_feature_correspondences.argtypes = [vp, vp, C.c_int32, C.c_int32, ip, C.POINTER(C.c_int64), ip]
        L.o3s_submap_transform.argtypes = [vp, dp]
        L.o3s_submap_build_voxel_map.argtypes = [vp, C.c_double]
        L.o3s_submap_voxel_map_size.argtypes = [vp]
        L.o3s_submap_voxel_map_size.restype = C.c_int64
        L.o3s_submap_overlap_fitness.argtypes = [vp, dp, C.c_int64, dp, C.POINTER(C.c_int64), dp]
        L.o3s_submap_overlap_fitness_scan.argtypes = [vp, vp, C.c_int, dp, C.POINTER(C.c_int64), dp]
        L.o3s_submaps_transform.argtypes = [C.c_int32, C.POINTER(vp), dp]
        L.o3s_assembled_map_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.o3s_assembled_map_destroy.argtypes = [vp]
        L.o3s_assembled_map_destroy.restype = None
        L.o3s_assembled_map_build.argtypes = [vp, C.c_int32, C.POINTER(vp), C.c_double, C.c_int32, C.POINTER(C.c_int64)]
        L.o3s_assembled_map_size.argtypes = [vp]
        L.o3s_assembled_map_size.restype = C.c_int64
        L.o3s_assembled_map_has_normals.argtypes = [vp]
        L.o3s_assembled_map_has_colors.argtypes = [vp]
        L.o3s_assembled_map_download.argtypes = [vp, dp, dp, dp]
        L.o3s_assembled_map_to_submap.argtypes = [vp, vp]
        L.o3s_assembled_map_device_bytes.argtypes = [vp]
        L.o3s_assembled_map_device_bytes.restype = C.c_int64
    return L


def _pose(T) -> np.ndarray:
    """4x4 -> Eigen::Matrix4d::data() order (column-major)."""
    return np.ascontiguousarray(np.asarray(T, np.float64).T).reshape(16)


class CarvingParamsC(C.Structure):
    _fields_ = [("voxel_size", C.c_double), ("max_raytracing_length", C.c_double), ("truncation_distance", C.c_double),
                ("min_dot_product_with_normal", C.c_double)]


class FeatureParamsC(C.Structure):
    """o3s_submap_feature_params: PlaceRecognitionParameters' feature part (parameter_structure_definitions.lua:163-167)."""
    _fields_ = [("feature_voxel_size", C.c_double), ("normal_radius", C.c_double), ("normal_knn", C.c_int32), ("feature_radius", C.c_double),
                ("feature_knn", C.c_int32)]


def featureParams(feature_voxel_size=0.5, normal_radius=2.0, normal_knn=20, feature_radius=2.5, feature_knn=100) -> FeatureParamsC:
    return FeatureParamsC(float(feature_voxel_size), float(normal_radius), int(normal_knn), float(feature_radius), int(feature_knn))


class Submap(_lib.Handle):
    """The active submap's sparse map cloud, resident on one MI355X."""

    _destroy = "o3s_submap_destroy"

    def __init__(self, map_voxel_size: float, map_builder_cropper: CropperC, device: int = 0):
        rc = self._create(_L(), "o3s_submap_create", device, float(map_voxel_size), C.byref(map_builder_cropper))
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_submap_create failed with o3s_status {rc} (no CPU fallback)")
        self.has_normals = None
        self.device = int(device)

    def _check(self, rc, what):
        if rc != _lib.OK:
            raise RuntimeError(f"{what} failed with o3s_status {rc}")

    def insertScan(self, points, normals, mapToRangeSensor) -> bool:
        """Submap::insertScan (Submap.cpp:39-96) without carving."""
        p = np.ascontiguousarray(points, np.float64)
        n = None if normals is None else np.ascontiguousarray(normals, np.float64)
        self._check(self._lib.o3s_submap_insert_scan(self._h, _d(p), _d(n), p.shape[0], _d(_pose(mapToRangeSensor))), "o3s_submap_insert_scan")
        if p.shape[0]:
            self.has_normals = n is not None
        return True

    insert_scan = insertScan

    def insertScanColored(self, points, normals, colors, mapToRangeSensor) -> bool:
        """Submap::insertScan for a coloured scan (o3s_submap_insert_scan_colored)."""
        p = np.ascontiguousarray(points, np.float64)
        n = None if normals is None else np.ascontiguousarray(normals, np.float64)
        c = np.ascontiguousarray(colors, np.float64)
        L = self._lib
        L.o3s_submap_insert_scan_colored.argtypes = None
        self._check(L.o3s_submap_insert_scan_colored(self._h, _d(p), _d(n), _d(c), C.c_int64(p.shape[0]), _d(_pose(mapToRangeSensor))),
                    "o3s_submap_insert_scan_colored")
        if p.shape[0]:
            self.has_normals = n is not None
        return True

    def hasColors(self) -> bool:
        return bool(self._lib.o3s_submap_has_colors(self._h))

    def getMapColors(self):
        out = np.zeros((len(self), 3))
        L = self._lib
        L.o3s_submap_download_colors.argtypes = None
        self._check(L.o3s_submap_download_colors(self._h, _d(out)), "o3s_submap_download_colors")
        return out

    def __len__(self) -> int:
        return int(self._lib.o3s_submap_size(self._h))

    def size_bounds(self):
        """(at_least, at_most) without waiting for an insert whose completion is pending (o3s_submap_size_bounds): equal when none is."""
        lo, hi = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.o3s_submap_size_bounds(self._h, C.byref(lo), C.byref(hi)), "o3s_submap_size_bounds")
        return int(lo.value), int(hi.value)

    def clone(self, device: int = None) -> "Submap":
        """A second submap object with a copy of the map cloud, on the same or another device (o3s_submap_clone): the snapshot a
        loop-closure worker refines while the mapper keeps inserting into the original."""
        L = self._lib
        L.o3s_submap_clone.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        other = object.__new__(Submap)
        other.has_normals = self.has_normals
        dev = int(getattr(self, "device", 0) if device is None else device)
        rc = other._create(L, "o3s_submap_clone", self._h, dev)
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_submap_clone failed with o3s_status {rc}")
        other.device = dev
        return other

    def insert_stats(self):
        """(merged, sorted, fell_back): how the voxelising inserts ran (o3s_submap_insert_stats)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        L = self._lib
        L.o3s_submap_insert_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        self._check(L.o3s_submap_insert_stats(self._h, C.byref(a), C.byref(b), C.byref(c)), "o3s_submap_insert_stats")
        return int(a.value), int(b.value), int(c.value)

    def reserve(self, n_points: int):
        """Room for n_points (SubmapParameters::maxNumPoints_ + one scan) up front: no re-allocation stall while the map grows."""
        self._check(self._lib.o3s_submap_reserve(self._h, int(n_points)), "o3s_submap_reserve")

    def trim(self):
        """o3s_submap_trim: a submap that is no longer inserted into gives everything but its map cloud back to the allocator."""
        self._lib.o3s_submap_trim.argtypes = [C.c_void_p]
        self._check(self._lib.o3s_submap_trim(self._h), "o3s_submap_trim")

    def hand_over(self, fresh: "Submap"):
        """o3s_submap_hand_over: this (closed) submap keeps its map in arrays of its own size; every other device buffer moves to the
        empty submap `fresh`."""
        self._lib.o3s_submap_hand_over.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self._lib.o3s_submap_hand_over(self._h, fresh._h), "o3s_submap_hand_over")

    def device_bytes(self) -> int:
        self._lib.o3s_submap_device_bytes.argtypes = [C.c_void_p]
        self._lib.o3s_submap_device_bytes.restype = C.c_int64
        return int(self._lib.o3s_submap_device_bytes(self._h))

    def computeSubmapCenter(self) -> np.ndarray:
        """Submap::computeSubmapCenter (Submap.cpp:282-286): open3d GetCenter() of the map cloud, summed on the device."""
        c = np.zeros(3)
        self._check(self._lib.o3s_submap_center(self._h, _d(c)), "o3s_submap_center")
        return c

    def getMapPointCloud(self):
        """(points, normals) copied to the host — for inspection / saving; the ICP never needs it."""
        n = len(self)
        pts = np.zeros((n, 3), np.float64)
        nrm = np.zeros((n, 3), np.float64) if self.has_normals else None
        self._check(self._lib.o3s_submap_download(self._h, _d(pts), _d(nrm)), "o3s_submap_download")
        return pts, nrm

    def computeFeatures(self, params: FeatureParamsC = None) -> int:
        """Submap::computeFeatures (Submap.cpp:255-275) on the resident map: voxel down-sample, normals, FPFH — all in HBM, kept in
        the submap until the next call.  Returns the number of sparse points.  The caller keeps the reference's timer
        (minSecondsBetweenFeatureComputation_)."""
        prm = featureParams() if params is None else params
        self._check(self._lib.o3s_submap_compute_features(self._h, C.byref(prm)), "o3s_submap_compute_features")
        return int(self._lib.o3s_submap_features_size(self._h))

    def features_size(self) -> int:
        """Sparse points of the resident feature set; -1 while there is none."""
        return int(self._lib.o3s_submap_features_size(self._h))

    def _download_features(self, want_cloud: bool, want_fpfh: bool):
        n = self.features_size()
        if n < 0:
            raise RuntimeError("the submap has no features: call computeFeatures first")
        pts = np.zeros((n, 3), np.float64) if want_cloud else None
        nrm = np.zeros((n, 3), np.float64) if want_cloud else None
        f = np.zeros((n, 33), np.float64) if want_fpfh else None
        self._check(self._lib.o3s_submap_download_features(self._h, _d(pts), _d(nrm), _d(f)), "o3s_submap_download_features")
        return pts, nrm, f

    def getSparseMapPointCloud(self):
        """Submap::getSparseMapPointCloud: (points, normals) of the cloud the features were computed on."""
        pts, nrm, _ = self._download_features(True, False)
        return pts, nrm

    def getFeatures(self) -> np.ndarray:
        """Submap::getFeatures: the n x 33 FPFH features (row i = Open3D's feature column i)."""
        return self._download_features(False, True)[2]

    def featureCorrespondences(self, target: "Submap", mutual_filter: bool = True, ransac_n: int = 3):
        """(pairs, used_fallback) between this submap's resident features (source) and `target`'s: registration.featureCorrespondences
        without a copy of either feature set leaving HBM."""
        n = self.features_size()
        if n < 0 or target.features_size() < 0:
            raise RuntimeError("both submaps need features: call computeFeatures first")
        pairs = np.zeros((n, 2), np.int32)
        n_out, fb = C.c_int64(0), C.c_int32(0)
        self._check(self._lib.o3s_submap_feature_correspondences(self._h, target._h, int(bool(mutual_filter)), int(ransac_n),
                                                                 pairs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_out), C.byref(fb)),
                    "o3s_submap_feature_correspondences")
        return pairs[:n_out.value].copy(), bool(fb.value)

    def ransacRegistration(self, target: "Submap", params=None, mutual_filter: bool = True):
        """RegistrationRANSACBasedOnFeatureMatching (PlaceRecognition.cpp:81-84) between this submap's resident feature set (source)
        and `target`'s: registration.RansacResult, with neither cloud nor feature set leaving HBM (o3s_submap_registration_ransac)."""
        from . import registration as reg

        reg._L()   # binds the argtypes on the library in use
        n = self.features_size()
        if n < 0 or target.features_size() < 0:
            raise RuntimeError("both submaps need features: call computeFeatures first")
        prm = reg._ransac_params(params)
        inl = np.zeros((max(n, 1), 2), np.int32)
        r, k = reg._RansacResult(), C.c_int64(0)
        self._lib.o3s_submap_registration_ransac.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(reg._RansacParams),
                                                             C.POINTER(reg._RansacResult), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        self._check(self._lib.o3s_submap_registration_ransac(self._h, target._h, int(bool(mutual_filter)), C.byref(prm), C.byref(r),
                                                             inl.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k)),
                    "o3s_submap_registration_ransac")
        return reg._ransac_result(r, inl, k.value)

    def setMapPointCloud(self, points, normals):
        p = np.ascontiguousarray(points, np.float64)
        n = None if normals is None else np.ascontiguousarray(normals, np.float64)
        self._check(self._lib.o3s_submap_upload(self._h, _d(p), _d(n), p.shape[0]), "o3s_submap_upload")
        self.has_normals = (n is not None) if p.shape[0] else None

    def transform(self, T):
        """The cloud part of Submap::transform (Submap.cpp:115-121) in place in HBM (o3s_submap_transform): Open3D's
        PointCloud::Transform on the map cloud and on the feature cloud; no almost-identity doubling."""
        rc = self._lib.o3s_submap_transform(self._h, _d(_pose(T)))
        if rc == _lib.ERR_BAD_ARGUMENT:
            raise ValueError("transform: T must be finite with a last row that is not zero")
        self._check(rc, "o3s_submap_transform")

    def buildVoxelMap(self, voxel_size: float) -> int:
        """voxelMap_.clear(); voxelMap_.insertCloud(mapCloud_) of Submap::computeFeatures (Submap.cpp:260-264) as an occupancy
        snapshot in HBM (o3s_submap_build_voxel_map); returns the number of occupied voxels.  Inserts, carving and transform() leave
        it as built — Submap::transform does not move voxelMap_ either."""
        rc = self._lib.o3s_submap_build_voxel_map(self._h, float(voxel_size))
        if rc == _lib.ERR_BAD_ARGUMENT:
            raise ValueError("buildVoxelMap: voxel_size must be positive and finite")
        self._check(rc, "o3s_submap_build_voxel_map")
        return self.voxel_map_size()

    def voxel_map_size(self) -> int:
        """Occupied voxels of the snapshot; -1 while the submap has none (o3s_submap_voxel_map_size)."""
        return int(self._lib.o3s_submap_voxel_map_size(self._h))

    def overlapFitness(self, scan, mapToRangeSensor, which: int = 0):
        """(n_overlapping, fitness): the points of `scan`, moved by mapToRangeSensor, that fall into an occupied voxel of the
        snapshot, and their share (the body of SubmapCollection::isSwitchingSubmapsConsistant, SubmapCollection.cpp:396-402).
        `scan`: (N, 3) host points, or a ProcessedScan, whose merge (which = 0) or match (1) cloud is read where it is.
        fitness is NaN for an empty scan and 0 without a snapshot, as the reference's expression."""
        k, f = C.c_int64(0), C.c_double(0.0)
        T = _d(_pose(mapToRangeSensor))
        if isinstance(scan, ProcessedScan):
            rc = self._lib.o3s_submap_overlap_fitness_scan(self._h, scan._h, int(which), T, C.byref(k), C.byref(f))
        else:
            p = np.ascontiguousarray(scan, np.float64).reshape(-1, 3)
            rc = self._lib.o3s_submap_overlap_fitness(self._h, _d(p), p.shape[0], T, C.byref(k), C.byref(f))
        if rc == _lib.ERR_BAD_ARGUMENT:
            raise ValueError("overlapFitness: bad argument (a pose that is not finite, `which` not 0 / 1, another device)")
        self._check(rc, "o3s_submap_overlap_fitness")
        return int(k.value), float(f.value)

    def carve(self, rawScan, mapToRangeSensor, voxel_size=0.1, max_raytracing_length=20.0, truncation_distance=0.1,
              min_dot_product_with_normal=0.5) -> int:
        """Submap::carve (Submap.cpp:116-130) with SpaceCarvingParameters; returns the number of removed map points.
        The caller applies the cadence (isCarvingEnabled_, carveSpaceEveryNscans_) and calls it BEFORE the insert."""
        p = np.ascontiguousarray(rawScan, np.float64)
        cp = CarvingParamsC(float(voxel_size), float(max_raytracing_length), float(truncation_distance), float(min_dot_product_with_normal))
        k = C.c_int64()
        self._check(self._lib.o3s_submap_carve(self._h, C.byref(cp), _d(p), p.shape[0], _d(_pose(mapToRangeSensor)), C.byref(k)), "o3s_submap_carve")
        return int(k.value)

    def removeOutliers(self, params):
        """The outlier filter `params` (cloud_ops.outlier_params) on the sparse map, in place -> (number of removed points, stats |
        None): bit for bit what cloud_ops.remove_*_outlier returns on the downloaded map; normals and colours follow their points.
        Like a carve it leaves the feature set, the voxel-map snapshot and an ICP reference describing the map as it was."""
        fn = self._lib.o3s_submap_remove_outliers
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        k = C.c_int64()
        st = np.zeros(4, np.float64)
        self._check(fn(self._h, C.byref(params), C.byref(k), _d(st)), "o3s_submap_remove_outliers")
        return int(k.value), (st if params.kind == 2 else None)

    def removeRadiusOutliers(self, nb_points: int, radius: float) -> int:
        """PointCloud::RemoveRadiusOutliers(nb_points, radius) on the sparse map, in place; returns the number of removed points."""
        from .cloud_ops import outlier_params
        return self.removeOutliers(outlier_params(1, nb_points, radius))[0]

    def removeStatisticalOutliers(self, nb_neighbors: int, std_ratio: float):
        """PointCloud::RemoveStatisticalOutliers(nb_neighbors, std_ratio) on the sparse map, in place -> (number of removed points,
        [mean, std, thr, valid])."""
        from .cloud_ops import outlier_params
        return self.removeOutliers(outlier_params(2, nb_neighbors, std_ratio))

    def clusterDBSCAN(self, eps: float, min_points: int):
        """PointCloud::ClusterDBSCAN(eps, min_points) of the sparse map -> (labels (size,) int32, n_clusters): what
        cloud_ops.cluster_dbscan returns on the downloaded map.  Nothing in the map changes."""
        from .cloud_ops import dbscan_params
        fn = self._lib.o3s_submap_cluster_dbscan
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        q = dbscan_params(eps, min_points, 0)
        n = len(self)   # settles a pending insert: the size the call will see
        labels = np.full(max(n, 1), -1, np.int32)
        k = C.c_int32()
        self._check(fn(self._h, C.byref(q), labels.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k)), "o3s_submap_cluster_dbscan")
        return labels[:n], int(k.value)

    def removeSmallClusters(self, params):
        """Small-cluster removal `params` (cloud_ops.dbscan_params) on the sparse map, in place -> (number of removed points,
        n_clusters): bit for bit what cloud_ops.remove_small_clusters returns on the downloaded map; normals and colours follow
        their points.  Like a carve it leaves the feature set, the voxel-map snapshot and an ICP reference describing the map as
        it was."""
        fn = self._lib.o3s_submap_remove_small_clusters
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        k, nc = C.c_int64(), C.c_int32()
        self._check(fn(self._h, C.byref(params), C.byref(k), C.byref(nc)), "o3s_submap_remove_small_clusters")
        return int(k.value), int(nc.value)

    def selectKeypoints(self, params):
        """ISS keypoints `params` (cloud_ops.iss_params) of the resident SPARSE cloud; the feature set — sparse points, normals, FPFH
        columns — is then reduced to them, in order -> (indices of the sparse points that stayed, radii = [salient, non_max] as
        used).  Correspondences, RANSAC, place recognition, clone, hand_over, trim and transform work on the reduced set; the next
        computeFeatures rebuilds the full one.  With min_neighbors 0 nothing happens and every index stays."""
        fn = self._lib.o3s_submap_select_keypoints
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        n = self.features_size()   # -1 without a feature set: the call then fails with O3S_ERR_NOT_INITIALIZED
        idx = np.arange(max(n, 1), dtype=np.int64)
        k = C.c_int64(max(n, 0))
        radii = np.zeros(2, np.float64)
        self._check(fn(self._h, C.byref(params), idx.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(k), _d(radii)), "o3s_submap_select_keypoints")
        return idx[:k.value].copy(), radii

    def featureKeypoints(self, params):
        """ISS keypoints `params` (cloud_ops.iss_params) of the resident SPARSE cloud, labels only -> (flags (features_size,) int32
        with 1 = keypoint, saliency (features_size,), radii): what cloud_ops.compute_iss_keypoints returns on the downloaded sparse
        cloud.  Nothing in the submap changes."""
        fn = self._lib.o3s_submap_feature_keypoints
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
        n = max(self.features_size(), 0)   # without a feature set the call fails with O3S_ERR_NOT_INITIALIZED
        flags = np.zeros(max(n, 1), np.int32)
        sal = np.zeros(max(n, 1), np.float64)
        k = C.c_int64(0)
        radii = np.zeros(2, np.float64)
        self._check(fn(self._h, C.byref(params), flags.ctypes.data_as(C.POINTER(C.c_int32)), _d(sal), C.byref(k), _d(radii)),
                    "o3s_submap_feature_keypoints")
        return flags[:n], sal[:n], radii

    def segmentPlanes(self, params):
        """RANSAC plane segmentation `params` (cloud_ops.plane_params) of the sparse map, where it lies -> (labels (size,) int32 with
        -1 = no plane, models (n_planes, 4), counts (n_planes,) int64): what cloud_ops.segment_planes returns on the downloaded
        map.  Nothing in the map changes."""
        fn = self._lib.o3s_submap_segment_planes
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        n = len(self)   # settles a pending insert: the size the call will see
        labels = np.full(max(n, 1), -1, np.int32)
        models, counts = np.zeros((16, 4)), np.zeros(16, np.int64)
        k = C.c_int32(0)
        self._check(fn(self._h, C.byref(params), labels.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(k), _d(models),
                       counts.ctypes.data_as(C.POINTER(C.c_int64))), "o3s_submap_segment_planes")
        return labels[:n], models[:k.value].copy(), counts[:k.value].copy()

    def removePlanes(self, params):
        """Every point a plane of `params` (cloud_ops.plane_params) took removed from the sparse map, in place -> (number of removed
        points, models (n_planes, 4)): bit for bit and in order what is left of the downloaded map without the labelled points;
        normals and colours follow their points.  Like a carve it leaves the feature set, the voxel-map snapshot and an ICP
        reference describing the map as it was."""
        fn = self._lib.o3s_submap_remove_planes
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        models = np.zeros((16, 4))
        r, k = C.c_int64(0), C.c_int32(0)
        self._check(fn(self._h, C.byref(params), C.byref(r), C.byref(k), _d(models)), "o3s_submap_remove_planes")
        return int(r.value), models[:k.value].copy()

    def insertProcessed(self, scan: "ProcessedScan", mapToRangeSensor) -> bool:
        """insertScan(rawScan, *processed.merge_, mapToRangeSensor) (Mapper.cpp:487) from the resident merge cloud."""
        self._check(self._lib.o3s_submap_insert_processed(self._h, scan._h, _d(_pose(mapToRangeSensor))), "o3s_submap_insert_processed")
        if scan.n_merge:
            self.has_normals = True
        return True

    def patch_count(self, scan_matcher_cropper: CropperC, mapToRangeSensor) -> int:
        """Size of the patch cropSubmap would return at this pose (Mapper.cpp:328), counted on the device."""
        k = C.c_int64()
        self._check(self._lib.o3s_submap_patch_count(self._h, C.byref(scan_matcher_cropper), _d(_pose(mapToRangeSensor)), C.byref(k)), "o3s_submap_patch_count")
        return int(k.value)

    def set_reference(self, scan_matcher_cropper: CropperC, mapToRangeSensor, icp: ICP) -> int:
        """cropSubmap + open3dToPointmatcher + icp.initReference (Mapper.cpp:328-366) without leaving HBM.
        Returns the patch size; raises if the patch is empty ("Map patch is empty", Mapper.cpp:330-336)."""
        k = C.c_int64()
        rc = self._lib.o3s_submap_set_reference(self._h, C.byref(scan_matcher_cropper), _d(_pose(mapToRangeSensor)), icp._h, C.byref(k))
        if rc == _lib.ERR_EMPTY_REFERENCE:
            raise RuntimeError("map patch is empty")
        if rc != _lib.OK:
            msg = icp._L.o3s_last_error(icp._h).decode()
            raise RuntimeError(f"o3s_submap_set_reference failed with o3s_status {rc}: {msg}")
        return int(k.value)


def transform_submaps(maps, Ts):
    """SubmapCollection::transform's device work in one call (o3s_submaps_transform): maps[i] gets Ts[i]; every launch on its
    submap's own stream, one wait at the end.  A repeated submap or an invalid T raises and changes no submap."""
    maps = list(maps)
    Ts = [np.asarray(T, np.float64) for T in Ts]
    if len(maps) != len(Ts):
        raise ValueError("transform_submaps: one transform per submap")
    if not maps:
        return
    L = maps[0]._lib
    if any(m._lib is not L for m in maps):
        raise ValueError("transform_submaps: the submaps belong to different builds of the library")
    hs = (C.c_void_p * len(maps))(*[m._h.value for m in maps])
    flat = np.ascontiguousarray(np.concatenate([_pose(T) for T in Ts]))
    rc = L.o3s_submaps_transform(len(maps), hs, _d(flat))
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError("transform_submaps: a repeated submap, or a T that is not finite or has a zero last row")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_submaps_transform failed with o3s_status {rc}")


class AssembledMap(_lib.Handle):
    """The map clouds of several resident submaps assembled into one cloud on the device (include/assembled_map/o3s_assembled_map.h):
    Mapper::getAssembledMapPointCloud (Mapper.cpp:506-538) and, with a voxel size, Open3D's VoxelDownSample of it — what
    SlamWrapper::saveMap writes and SlamWrapperRos::publishMaps publishes.  The result and the work area stay resident and only
    grow; nothing but the result ever crosses the bus, and only when getPointCloud() asks for it."""

    NORMALS, COLORS = 1, 2   # bits of the C call's `attrs`
    _destroy = "o3s_assembled_map_destroy"

    def __init__(self, device: int = 0):
        rc = self._create(_L(), "o3s_assembled_map_create", device)
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_assembled_map_create failed with o3s_status {rc} (no CPU fallback)")
        self.device = int(device)

    def build(self, maps, voxel_size: float = 0.0, normals: bool = True, colors: bool = True) -> int:
        """Assembles `maps` (Submap objects, or None for a NULL pointer) in the order given; voxel_size <= 0: the plain concatenation,
        > 0: VoxelDownSample of it with the per-voxel sums in concatenation order.  The result carries normals / colours iff they
        are asked for and every non-empty submap has them.  A NULL or repeated submap, a submap of another device, more than
        2^31 - 1 points or a voxel index range that does not pack raises ValueError and leaves the previous result.  Returns the size."""
        maps = list(maps)
        if any(m is not None and m._lib is not self._lib for m in maps):
            raise ValueError("AssembledMap.build: the submaps belong to another build of the library")
        hs = (C.c_void_p * max(len(maps), 1))(*[None if m is None else m._h.value for m in maps])
        k = C.c_int64(0)
        attrs = (self.NORMALS if normals else 0) | (self.COLORS if colors else 0)
        rc = self._lib.o3s_assembled_map_build(self._h, len(maps), hs, float(voxel_size), attrs, C.byref(k))
        if rc == _lib.ERR_BAD_ARGUMENT:
            raise ValueError("AssembledMap.build: a NULL or repeated submap, a submap of another device, more than 2^31 - 1 points, or a "
                             "voxel index range that does not pack into 63 bits")
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_assembled_map_build failed with o3s_status {rc}")
        return int(k.value)

    def __len__(self) -> int:
        return int(self._lib.o3s_assembled_map_size(self._h))

    @property
    def has_normals(self) -> bool:
        return bool(self._lib.o3s_assembled_map_has_normals(self._h))

    @property
    def has_colors(self) -> bool:
        return bool(self._lib.o3s_assembled_map_has_colors(self._h))

    def getPointCloud(self):
        """(points, normals | None, colors | None) copied to the host: the one transfer of the assembled map."""
        n = len(self)
        pts = np.zeros((n, 3), np.float64)
        nrm = np.zeros((n, 3), np.float64) if self.has_normals else None
        col = np.zeros((n, 3), np.float64) if self.has_colors else None
        rc = self._lib.o3s_assembled_map_download(self._h, _d(pts), _d(nrm), _d(col))
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_assembled_map_download failed with o3s_status {rc}")
        return pts, nrm, col

    def toSubmap(self, dst: "Submap"):
        """Replaces dst's map cloud with the assembled map without leaving HBM (o3s_assembled_map_to_submap): colours are kept,
        dst's voxel layout and features are dropped.  dst may then serve as an ICP reference (set_reference) or get features."""
        rc = self._lib.o3s_assembled_map_to_submap(self._h, dst._h)
        if rc == _lib.ERR_BAD_ARGUMENT:
            raise ValueError("AssembledMap.toSubmap: the submap lives on another device")
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_assembled_map_to_submap failed with o3s_status {rc}")
        dst.has_normals = self.has_normals if len(self) else None

    def device_bytes(self) -> int:
        return int(self._lib.o3s_assembled_map_device_bytes(self._h))


class ProcessedScan(_lib.Handle):
    """ScanToMapIcp::processForScanMatchingAndMerging (ScanToMapRegistration.cpp:36-69) with both result clouds resident
    in HBM: ``merge`` (wide crop, voxelised) feeds Submap.insertProcessed, ``match`` (narrow crop) feeds the ICP."""

    _destroy = "o3s_scan_destroy"

    def __init__(self, device: int = 0):
        rc = self._create(_L(), "o3s_scan_create", device)
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_scan_create failed with o3s_status {rc} (no CPU fallback)")
        self.n_merge = self.n_match = 0

    def set_normal_estimation(self, max_radius: float, knn: int):
        """icp.max_distance_knn / icp.knn of the parameter files: used only for scans that arrive without normals."""
        rc = self._lib.o3s_scan_set_normal_estimation(self._h, float(max_radius), int(knn))
        if rc != _lib.OK:
            raise ValueError("knn must be in 1..32 and max_radius > 0")

    def preprocess(self, map_builder_cropper: CropperC, voxel_size: float, scan_matcher_cropper: CropperC, points, normals):
        p = np.ascontiguousarray(points, np.float64)
        n = None if normals is None else np.ascontiguousarray(normals, np.float64)
        a, b = C.c_int64(), C.c_int64()
        rc = self._lib.o3s_scan_preprocess(self._h, C.byref(map_builder_cropper), float(voxel_size), C.byref(scan_matcher_cropper), _d(p), _d(n),
                                      p.shape[0], C.byref(a), C.byref(b))
        if rc == _lib.ERR_BAD_SHAPE:
            raise RuntimeError("the scan has no normals and set_normal_estimation() was not called")
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_scan_preprocess failed with o3s_status {rc}")
        self.n_merge, self.n_match = int(a.value), int(b.value)
        return self.n_merge, self.n_match

    def removeOutliers(self, scan_matcher_cropper: CropperC, params):
        """The outlier filter `params` (cloud_ops.outlier_params) on the merge cloud, in place; the match cloud becomes the
        scan_matcher_cropper crop of what is left.  Returns (n_merge, n_match).  kind 0 does nothing."""
        fn = self._lib.o3s_scan_remove_outliers
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(CropperC), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        a, b = C.c_int64(self.n_merge), C.c_int64(self.n_match)
        rc = fn(self._h, C.byref(scan_matcher_cropper), C.byref(params), C.byref(a), C.byref(b))
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_scan_remove_outliers failed with o3s_status {rc}")
        self.n_merge, self.n_match = int(a.value), int(b.value)
        return self.n_merge, self.n_match

    def removeSmallClusters(self, scan_matcher_cropper: CropperC, params):
        """Small-cluster removal `params` (cloud_ops.dbscan_params) on the merge cloud, in place; the match cloud becomes the
        scan_matcher_cropper crop of what is left.  Returns (n_merge, n_match).  min_points 0 does nothing."""
        fn = self._lib.o3s_scan_remove_small_clusters
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(CropperC), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        a, b = C.c_int64(self.n_merge), C.c_int64(self.n_match)
        rc = fn(self._h, C.byref(scan_matcher_cropper), C.byref(params), C.byref(a), C.byref(b))
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_scan_remove_small_clusters failed with o3s_status {rc}")
        self.n_merge, self.n_match = int(a.value), int(b.value)
        return self.n_merge, self.n_match

    def removePlanes(self, scan_matcher_cropper: CropperC, params):
        """Every point a plane of `params` (cloud_ops.plane_params) took removed from the merge cloud, in place; the match cloud
        becomes the scan_matcher_cropper crop of what is left.  Returns (n_merge, n_match, models (n_planes, 4)).
        num_iterations 0 does nothing."""
        fn = self._lib.o3s_scan_remove_planes
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(CropperC), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                       C.POINTER(C.c_double)]
        a, b, k = C.c_int64(self.n_merge), C.c_int64(self.n_match), C.c_int32(0)
        models = np.zeros((16, 4))
        rc = fn(self._h, C.byref(scan_matcher_cropper), C.byref(params), C.byref(a), C.byref(b), C.byref(k), _d(models))
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_scan_remove_planes failed with o3s_status {rc}")
        self.n_merge, self.n_match = int(a.value), int(b.value)
        return self.n_merge, self.n_match, models[:k.value].copy()

    def _get(self, which):
        n = int(self._lib.o3s_scan_get(self._h, which, None, None))
        pts, nrm = np.zeros((n, 3), np.float64), np.zeros((n, 3), np.float64)
        if n and self._lib.o3s_scan_get(self._h, which, _d(pts), _d(nrm)) != n:
            raise RuntimeError("o3s_scan_get failed")
        return pts, nrm

    @property
    def merge(self):
        return self._get(0)

    @property
    def match(self):
        return self._get(1)

    def set_reading(self, icp: ICP):
        """open3dToPointmatcher(*processed.match_) -> resident reading of `icp` (then icp.compute_resident(T_init))."""
        rc = self._lib.o3s_scan_set_reading(self._h, icp._h)
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_scan_set_reading failed with o3s_status {rc}")
