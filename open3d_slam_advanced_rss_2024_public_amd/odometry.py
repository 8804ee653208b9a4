"""Scan-to-scan LiDAR odometry and sweep de-skewing over resident scans (C ABI: include/o3s_scan.h) — the Python mirror of
cpp/o3s_odometry.hpp.  Restates, with every cloud operation on the device:

  LidarOdometry                       O3S/src/Odometry.cpp:22-134
  ConstantVelocityMotionCompensation  O3S/src/MotionCompensation.cpp:32-127
  TransformBuffer                     O3S/src/TransformInterpolationBuffer.cpp (push rules, size limit, accessors, exact lookup)
  TransformInterpolationBuffer        ... with the range-based has and the interpolating lookup (:100-149); get_transform (:189-220)
  TrajectoryMotionCompensation        the de-skew of a sweep along the odometry's trajectory (include/trajectory/o3s_trajectory.h)

Timestamps are double seconds.  No arithmetic on clouds happens here; the velocity estimate is one host function of the library
(o3s_motion_from_poses), and so are the interpolation and extrapolation of poses (o3s_transform_* / o3s_trajectory_*), so that
C++ and Python share one implementation."""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from . import registration as reg
from . import submap as sm
from .cloud_ops import CropperC, _d, croppingVolumeFactory
from .mapper import inv_iso, mul4


class MotionC(C.Structure):
    """o3s_motion"""
    _fields_ = [("linear_velocity", C.c_double * 3), ("angular_velocity_rpy", C.c_double * 3), ("scan_duration", C.c_double),
                ("is_spinning_clockwise", C.c_int32), ("reserved", C.c_int32 * 3)]


class StampedPoseC(C.Structure):
    """o3s_stamped_pose"""
    _fields_ = [("t", C.c_double), ("T", C.c_double * 16)]


class TrajectoryDeskewC(C.Structure):
    """o3s_trajectory_deskew"""
    _fields_ = [("stamp", C.c_double), ("scan_duration", C.c_double), ("calibration", C.c_double * 16), ("is_spinning_clockwise", C.c_int32),
                ("reserved", C.c_int32 * 3)]


TRAJECTORY_MAX_POSES = 2000   # O3S_TRAJECTORY_MAX_POSES


def _L():
    sm._L(), reg._L()
    L = _lib.lib()
    if _lib.needs_binding(L, __name__):  # once per loaded library (product or test-hook build)
        dp, vp = C.POINTER(C.c_double), C.c_void_p
        L.o3s_raw_scan_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.o3s_raw_scan_destroy.argtypes = [vp]
        L.o3s_raw_scan_destroy.restype = None
        L.o3s_raw_scan_upload.argtypes = [vp, dp, dp, C.c_int64]
        L.o3s_raw_scan_size.argtypes = [vp]
        L.o3s_raw_scan_size.restype = C.c_int64
        L.o3s_raw_scan_undistort.argtypes = [vp, C.POINTER(MotionC)]
        L.o3s_undistort_cloud.argtypes = [C.c_int, C.POINTER(MotionC), dp, C.c_int64, dp]
        L.o3s_motion_from_poses.argtypes = [dp, C.c_double, dp, C.c_double, C.POINTER(MotionC)]
        sp, td = C.POINTER(StampedPoseC), C.POINTER(TrajectoryDeskewC)
        L.o3s_transform_interpolate.argtypes = [sp, sp, C.c_double, sp]
        L.o3s_transform_extrapolate.argtypes = [sp, sp, C.c_double, sp]
        L.o3s_trajectory_has.argtypes = [sp, C.c_int64, C.c_double]
        L.o3s_trajectory_lookup.argtypes = [sp, C.c_int64, C.c_double, dp]
        L.o3s_trajectory_get_transform.argtypes = [sp, C.c_int64, C.c_double, dp]
        L.o3s_raw_scan_set_point_times.argtypes = [vp, dp, C.c_int64]
        L.o3s_raw_scan_undistort_trajectory.argtypes = [vp, sp, C.c_int64, td]
        L.o3s_undistort_cloud_trajectory.argtypes = [C.c_int, sp, C.c_int64, td, dp, dp, C.c_int64, dp]
        L.o3s_scan_preprocess_staged.argtypes = [vp, C.POINTER(CropperC), C.c_double, C.POINTER(CropperC), vp, C.POINTER(C.c_int64),
                                                 C.POINTER(C.c_int64)]
        L.o3s_scan_registration_icp.argtypes = [vp, C.c_int, vp, C.c_int, C.c_double, dp, C.POINTER(reg._Estimation), C.POINTER(reg._Criteria),
                                                C.POINTER(reg._Result)]
    return L


def make_motion(linear_velocity=(0.0, 0.0, 0.0), angular_velocity_rpy=(0.0, 0.0, 0.0), scan_duration=0.1, is_spinning_clockwise=True) -> MotionC:
    m = MotionC()
    for k in range(3):
        m.linear_velocity[k] = float(linear_velocity[k])
        m.angular_velocity_rpy[k] = float(angular_velocity_rpy[k])
    m.scan_duration = float(scan_duration)
    m.is_spinning_clockwise = int(bool(is_spinning_clockwise))
    return m


def motion_from_poses(T_start, t_start, T_finish, t_finish):
    """(linear velocity, angular velocity rpy) of estimateLinearAndAngularVelocity for two buffered poses (o3s_motion_from_poses)."""
    m = MotionC()
    rc = _L().o3s_motion_from_poses(_d(sm._pose(T_start)), float(t_start), _d(sm._pose(T_finish)), float(t_finish), C.byref(m))
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_motion_from_poses failed with o3s_status {rc}")
    return np.array(m.linear_velocity[:]), np.array(m.angular_velocity_rpy[:])


def undistort_cloud(points, motion: MotionC, device: int = 0, in_place: bool = False) -> np.ndarray:
    """undistortInputPointCloud on a host cloud (o3s_undistort_cloud); in_place rewrites `points` (a contiguous float64 array)."""
    p = np.ascontiguousarray(points, np.float64)
    if in_place and p is not points:
        raise ValueError("in_place needs a contiguous float64 array")
    out = p if in_place else np.empty_like(p)
    rc = _L().o3s_undistort_cloud(device, C.byref(motion), _d(p), p.shape[0], _d(out))
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError("scan_duration must be > 0")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_undistort_cloud failed with o3s_status {rc}")
    return out


def stamped_pose(t, T) -> StampedPoseC:
    p = StampedPoseC()
    p.t = float(t)
    p.T[:] = np.asarray(T, np.float64).reshape(4, 4).T.reshape(16)
    return p


def pose_table(stamps, poses):
    """A table of o3s_stamped_pose in buffer order (a ctypes array; empty tables are one unused entry long)."""
    tab = (StampedPoseC * max(len(stamps), 1))()
    for k, (t, T) in enumerate(zip(stamps, poses)):
        tab[k].t = float(t)
        tab[k].T[:] = np.asarray(T, np.float64).reshape(4, 4).T.reshape(16)
    return tab


def _mat(T16) -> np.ndarray:
    return np.array(T16[:], np.float64).reshape(4, 4).T.copy()


def _two_pose_call(fn, name, start, end, t):
    out = StampedPoseC()
    rc = fn(C.byref(stamped_pose(*start)), C.byref(stamped_pose(*end)), float(t), C.byref(out))
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError(f"{name}: the stamps do not allow it")
    if rc != _lib.OK:
        raise RuntimeError(f"{name} failed with o3s_status {rc}")
    return out.t, _mat(out.T)


def transform_interpolate(start, end, t):
    """interpolate (Transform.cpp:16-67) between two (stamp, pose) pairs: (t, pose).  ValueError where the reference throws."""
    return _two_pose_call(_L().o3s_transform_interpolate, "o3s_transform_interpolate", start, end, t)


def transform_extrapolate(start, end, t):
    """extrapolate (Transform.cpp:69-110) beyond `end`: (stamp, pose).  ValueError where the reference throws."""
    return _two_pose_call(_L().o3s_transform_extrapolate, "o3s_transform_extrapolate", start, end, t)


def make_trajectory_deskew(stamp, scan_duration=0.1, is_spinning_clockwise=True, calibration=None) -> TrajectoryDeskewC:
    p = TrajectoryDeskewC()
    p.stamp, p.scan_duration = float(stamp), float(scan_duration)
    p.calibration[:] = np.asarray(np.eye(4) if calibration is None else calibration, np.float64).reshape(4, 4).T.reshape(16)
    p.is_spinning_clockwise = int(bool(is_spinning_clockwise))
    return p


def _trajectory_status(rc, what):
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError(f"{what}: 1 .. {TRAJECTORY_MAX_POSES} poses with stamps in order, point times for every point or a scan_duration > 0")
    if rc != _lib.OK:
        raise RuntimeError(f"{what} failed with o3s_status {rc}")


def undistort_cloud_trajectory(points, table, K, params: TrajectoryDeskewC, point_times=None, device: int = 0, in_place: bool = False) -> np.ndarray:
    """The de-skew along a trajectory on a host cloud (o3s_undistort_cloud_trajectory); table: pose_table(...) of K poses."""
    p = np.ascontiguousarray(points, np.float64)
    if in_place and p is not points:
        raise ValueError("in_place needs a contiguous float64 array")
    dt = None
    if point_times is not None:
        dt = np.ascontiguousarray(point_times, np.float64)
        if dt.shape != (p.shape[0],):
            raise ValueError("point_times: one offset per point")
    out = p if in_place else np.empty_like(p)
    _trajectory_status(_L().o3s_undistort_cloud_trajectory(device, table, int(K), C.byref(params), _d(p), _d(dt), p.shape[0], _d(out)),
                       "o3s_undistort_cloud_trajectory")
    return out


class RawScan(_lib.Handle):
    """o3s_raw_scan: a sweep staged in HBM ahead of the pre-processing (and the thing a de-skew acts on)."""

    _destroy = "o3s_raw_scan_destroy"

    def __init__(self, device: int = 0):
        rc = self._create(_L(), "o3s_raw_scan_create", device)
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_raw_scan_create failed with o3s_status {rc} (no CPU fallback)")

    def __len__(self) -> int:
        return int(self._lib.o3s_raw_scan_size(self._h))

    def upload(self, points, normals=None):
        p = np.ascontiguousarray(points, np.float64)
        n = None if normals is None else np.ascontiguousarray(normals, np.float64)
        rc = self._lib.o3s_raw_scan_upload(self._h, _d(p), _d(n), p.shape[0])
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_raw_scan_upload failed with o3s_status {rc}")

    def undistort(self, motion: MotionC):
        rc = self._lib.o3s_raw_scan_undistort(self._h, C.byref(motion))
        if rc == _lib.ERR_BAD_ARGUMENT:
            raise ValueError("scan_duration must be > 0")
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_raw_scan_undistort failed with o3s_status {rc}")

    def set_point_times(self, point_times):
        """The driver's per-point time offsets (seconds after the sweep's stamp) of the staged sweep; the next upload drops them."""
        dt = np.ascontiguousarray(point_times, np.float64).reshape(-1)
        rc = self._lib.o3s_raw_scan_set_point_times(self._h, _d(dt), dt.shape[0])
        if rc == _lib.ERR_BAD_ARGUMENT:
            raise ValueError("point_times: one offset per staged point")
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_raw_scan_set_point_times failed with o3s_status {rc}")

    def undistort_trajectory(self, table, K, params: TrajectoryDeskewC):
        _trajectory_status(self._lib.o3s_raw_scan_undistort_trajectory(self._h, table, int(K), C.byref(params)), "o3s_raw_scan_undistort_trajectory")


def preprocess_staged(scan: sm.ProcessedScan, map_builder_cropper: CropperC, voxel_size: float, scan_matcher_cropper: CropperC, raw: RawScan):
    """o3s_scan_preprocess_staged: ProcessedScan.preprocess from a staged sweep."""
    a, b = C.c_int64(), C.c_int64()
    rc = _L().o3s_scan_preprocess_staged(scan._h, C.byref(map_builder_cropper), float(voxel_size), C.byref(scan_matcher_cropper), raw._h,
                                         C.byref(a), C.byref(b))
    if rc == _lib.ERR_BAD_SHAPE:
        raise RuntimeError("the scan has no normals and set_normal_estimation() was not called")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_scan_preprocess_staged failed with o3s_status {rc}")
    scan.n_merge, scan.n_match = int(a.value), int(b.value)
    return scan.n_merge, scan.n_match


def scan_registration_status(source: sm.ProcessedScan, target: sm.ProcessedScan, max_correspondence_distance, init=None,
                             registration_type="GeneralizedIcp", epsilon=1e-3, source_which=0, target_which=0, relative_fitness=1e-6,
                             relative_rmse=1e-6, max_iteration=30):
    """(o3s_status, RegistrationResult | None) of o3s_scan_registration_icp."""
    est = reg._estimation(registration_type, epsilon)
    cr = reg._Criteria(float(relative_fitness), float(relative_rmse), int(max_iteration))
    r = reg._Result()
    rc = _L().o3s_scan_registration_icp(source._h, int(source_which), target._h, int(target_which), float(max_correspondence_distance),
                                        _d(sm._pose(np.eye(4) if init is None else init)), C.byref(est), C.byref(cr), C.byref(r))
    return rc, (reg._result(r) if rc == _lib.OK else None)


def scan_registration_icp(source, target, max_correspondence_distance, init=None, registration_type="GeneralizedIcp", **kw) -> reg.RegistrationResult:
    """CloudRegistration::registerClouds between two resident pre-processed scans (neither cloud leaves HBM)."""
    rc, res = scan_registration_status(source, target, max_correspondence_distance, init, registration_type, **kw)
    if rc == _lib.ERR_EMPTY_REFERENCE:
        raise RuntimeError("one of the scans is empty")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_scan_registration_icp failed with o3s_status {rc}")
    return res


class TransformBuffer:
    """TransformInterpolationBuffer restricted to what the odometry, the motion compensation and the drivers ask of it: the push
    rules (:22-46), the size limit (:151-155, default 2000), the accessors and the lookup of an exact stamp."""

    def __init__(self, size_limit: int = 2000):
        self.size_limit = int(size_limit)
        self._t = []
        self._T = []

    def push(self, t, T):
        t = float(t)
        if self._t and (t < self._t[0] or t < self._t[-1]):   # earlier than the earliest / out of order: ignored
            return
        self._t.append(t)
        self._T.append(np.array(T, np.float64).reshape(4, 4))
        while len(self._t) > self.size_limit:
            self._t.pop(0)
            self._T.pop(0)

    def size(self) -> int:
        return len(self._t)

    __len__ = size

    def empty(self) -> bool:
        return not self._t

    def _need(self):
        if not self._t:
            raise RuntimeError("TransformBuffer: empty buffer")

    def earliest_time(self) -> float:
        self._need()
        return self._t[0]

    def latest_time(self) -> float:
        self._need()
        return self._t[-1]

    def latest_measurement(self):
        self._need()
        return self._t[-1], self._T[-1]

    def latest_offseted_measurement(self, offset: int):
        """std::prev(end, offset + 1)"""
        self._need()
        if not 0 <= offset < len(self._t):
            raise IndexError("TransformBuffer: offset beyond the buffer")
        return self._t[-1 - offset], self._T[-1 - offset]

    def has(self, t) -> bool:
        return bool(self._t) and self._t[0] <= t <= self._t[-1]

    def lookup(self, t):
        """The pose pushed with exactly this stamp (the first of equal stamps, as std::find_if meets it)."""
        for k, tk in enumerate(self._t):
            if tk == t:
                return self._T[k]
        raise RuntimeError("TransformBuffer: no pose at the requested stamp")


class TransformInterpolationBuffer(TransformBuffer):
    """TransformInterpolationBuffer as the reference has it: the push rules and accessors of TransformBuffer, has(t) over the range
    of the buffer and the lookup that interpolates between the two neighbouring poses (:100-149).  The arithmetic is the
    library's (o3s_trajectory_lookup): C++ and Python share one implementation."""

    def __init__(self, size_limit: int = 2000):
        super().__init__(size_limit)
        self._table = None

    def push(self, t, T):
        super().push(t, T)
        self._table = None

    def table(self):
        """The buffer as a table of o3s_stamped_pose (built once per change of the buffer)."""
        if self._table is None:
            self._table = pose_table(self._t, self._T)
        return self._table

    def lookup(self, t):
        out = (C.c_double * 16)()
        rc = _L().o3s_trajectory_lookup(self.table(), len(self._t), float(t), out)
        if rc == _lib.ERR_BAD_ARGUMENT:
            raise RuntimeError(f"TransformInterpolationBuffer: missing transform for {t!r}")
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_trajectory_lookup failed with o3s_status {rc}")
        return _mat(out)


def get_transform(t, buffer: TransformInterpolationBuffer):
    """getTransform(time, buffer) (:189-220): the earliest pose before the buffer, the extrapolation from the third pose from the
    end after it (the latest pose while it holds fewer than three), else the lookup."""
    buffer._need()
    out = (C.c_double * 16)()
    rc = _L().o3s_trajectory_get_transform(buffer.table(), buffer.size(), float(t), out)
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_trajectory_get_transform failed with o3s_status {rc}")
    return _mat(out)


class TrajectoryMotionCompensation:
    """The de-skew of a sweep along the trajectory an interpolating buffer holds (o3s_*_undistort_trajectory): every point is
    expressed in the sensor frame at the sweep's stamp.  Point times come from the driver (point_times), else from the azimuth as
    in ConstantVelocityMotionCompensation (scan_duration, is_spinning_clockwise)."""

    def __init__(self, buffer: TransformInterpolationBuffer, scan_duration: float = 0.1, is_spinning_clockwise: bool = True, calibration=None):
        if not scan_duration > 0.0:
            raise ValueError("scan_duration must be > 0")
        self.buffer = buffer
        self.scan_duration = float(scan_duration)
        self.is_spinning_clockwise = bool(is_spinning_clockwise)
        self.calibration = np.eye(4) if calibration is None else np.array(calibration, np.float64).reshape(4, 4)

    def params(self, stamp) -> TrajectoryDeskewC:
        return make_trajectory_deskew(stamp, self.scan_duration, self.is_spinning_clockwise, self.calibration)

    def undistort_cloud(self, points, stamp, point_times=None, device: int = 0):
        """A host cloud de-skewed; with an empty buffer the cloud as it came."""
        if self.buffer.empty():
            return np.ascontiguousarray(points, np.float64)
        return undistort_cloud_trajectory(points, self.buffer.table(), self.buffer.size(), self.params(stamp), point_times, device)

    def undistort(self, raw_scan: RawScan, stamp, point_times=None):
        """The staged sweep de-skewed in place; with an empty buffer nothing happens."""
        if point_times is not None:
            raw_scan.set_point_times(point_times)
        if not self.buffer.empty():
            raw_scan.undistort_trajectory(self.buffer.table(), self.buffer.size(), self.params(stamp))


class ConstantVelocityMotionCompensation:
    """ConstantVelocityMotionCompensation over a TransformBuffer (MotionCompensation.cpp:32-127)."""

    def __init__(self, buffer: TransformBuffer, scan_duration: float = 0.1, is_spinning_clockwise: bool = True, num_poses_vel_estimation: int = 3):
        if not scan_duration > 0.0:
            raise ValueError("scan_duration must be > 0")
        self.buffer = buffer
        self.scan_duration = float(scan_duration)
        self.is_spinning_clockwise = bool(is_spinning_clockwise)
        self.num_poses = int(num_poses_vel_estimation)

    def motion(self, stamp) -> MotionC:
        """estimateLinearAndAngularVelocity: zero while the buffer holds no more than num_poses poses or already has this stamp."""
        m = make_motion(scan_duration=self.scan_duration, is_spinning_clockwise=self.is_spinning_clockwise)
        b = self.buffer
        if b.size() <= self.num_poses or not b.latest_time() < stamp:
            return m
        t1, T1 = b.latest_measurement()
        t0, T0 = b.latest_offseted_measurement(self.num_poses)
        rc = _L().o3s_motion_from_poses(_d(sm._pose(T0)), t0, _d(sm._pose(T1)), t1, C.byref(m))
        if rc != _lib.OK:
            raise RuntimeError(f"o3s_motion_from_poses failed with o3s_status {rc}")
        return m

    def undistort(self, raw_scan: RawScan, stamp) -> MotionC:
        """undistortInputPointCloud on the staged sweep, in place; returns the motion used."""
        m = self.motion(stamp)
        raw_scan.undistort(m)
        return m


@dataclass
class OdometryParams:
    """OdometryParameters with the values of param/tutorial_1_LO.lua over the defaults."""
    voxel_size: float = 0.05                    # odometry.scan_processing.voxel_size
    downsampling_ratio: float = 1.0             # must be 1.0: RandomDownSample(1.0) keeps the set, the order is taken as the identity
    cropper: CropperC = field(default_factory=lambda: croppingVolumeFactory("MinMaxRadius", 2.0, 40.0))
    registration_type: str = "GeneralizedIcp"   # scan_matching.cloud_registration_type
    max_correspondence_distance: float = 1.0    # scan_matching.icp.max_correspondence_dist
    knn: int = 10                               # scan_matching.icp.knn
    max_distance_knn: float = 1.0               # scan_matching.icp.max_distance_knn
    max_n_iter: int = 30                        # scan_matching.icp.max_n_iter
    buffer_size: int = 2000


class LidarOdometry:
    """LidarOdometry::addRangeScan (Odometry.cpp:29-94) over two resident scans that are swapped, never copied."""

    def __init__(self, params: OdometryParams = None, device: int = 0):
        self.params = OdometryParams() if params is None else params
        if self.params.downsampling_ratio != 1.0:
            raise ValueError("downsampling_ratio must be 1.0 (o3s_status 11, BAD_ARGUMENT)")
        self.device = int(device)
        self.prev, self.next = sm.ProcessedScan(device), sm.ProcessedScan(device)
        for s in (self.prev, self.next):
            s.set_normal_estimation(self.params.max_distance_knn, self.params.knn)
        self.buffer = TransformBuffer(self.params.buffer_size)
        self.cumulative = np.eye(4)
        self.last_stamp = None
        self.initial_transform = None     # isInitialTransformSet_ / initialTransform_
        self.last_result = None
        self.last_timings = {"preprocess_ms": 0.0, "registration_ms": 0.0}   # wall clock of the last add_range_scan's two stages

    def set_initial_transform(self, T):
        """LidarOdometry::setInitialTransform (:118-134): a second call before the value was used is ignored."""
        if self.initial_transform is not None:
            return
        self.initial_transform = np.array(T, np.float64).reshape(4, 4)
        self.cumulative = self.initial_transform.copy()

    def has_processed_measurements(self) -> bool:
        return not self.buffer.empty()

    def odom_to_range_sensor(self, stamp):
        return self.buffer.lookup(stamp)

    def _preprocess(self, scan, points, normals, raw):
        p = self.params
        t0 = time.perf_counter()
        try:
            self._preprocess_call(scan, points, normals, raw, p)
        finally:
            self.last_timings = {"preprocess_ms": (time.perf_counter() - t0) * 1e3, "registration_ms": 0.0}

    @staticmethod
    def _preprocess_call(scan, points, normals, raw, p):
        if raw is not None:
            preprocess_staged(scan, p.cropper, p.voxel_size, p.cropper, raw)
        else:
            scan.preprocess(p.cropper, p.voxel_size, p.cropper, points, normals)

    def add_range_scan(self, points, normals, stamp, raw: RawScan = None) -> bool:
        """points / normals: the sweep in the sensor frame (normals None: estimated), or raw: the sweep staged (and de-skewed) in HBM."""
        stamp = float(stamp)
        if self.prev.n_merge == 0:   # cloudPrev_.IsEmpty(): the first measurement
            self._preprocess(self.prev, points, normals, raw)
            self.buffer.push(stamp, self.cumulative)
            self.last_stamp = stamp
            return True
        if stamp < self.last_stamp:
            return False
        self._preprocess(self.next, points, normals, raw)
        p = self.params
        t0 = time.perf_counter()
        rc, res = scan_registration_status(self.prev, self.next, p.max_correspondence_distance, np.eye(4), p.registration_type,
                                           max_iteration=p.max_n_iter)
        self.last_timings["registration_ms"] = (time.perf_counter() - t0) * 1e3
        if rc == _lib.ERR_EMPTY_REFERENCE:   # Open3D on an empty target: the default result (identity, fitness 0)
            res = reg.RegistrationResult(np.eye(4), 0.0, 0.0, 0, 0)
        elif rc != _lib.OK:
            raise RuntimeError(f"o3s_scan_registration_icp failed with o3s_status {rc}")
        self.last_result = res
        T = res.transformation
        if np.sqrt(T[0, 3] * T[0, 3] + T[1, 3] * T[1, 3] + T[2, 3] * T[2, 3]) > 0.8:
            return False
        if not res.fitness > 0.1:
            if self.next.n_merge:
                self.prev, self.next = self.next, self.prev
            return False
        if self.initial_transform is not None:
            self.cumulative = self.initial_transform.copy()
            self.initial_transform = None
        else:
            self.cumulative = mul4(self.cumulative, inv_iso(T))
        self.prev, self.next = self.next, self.prev
        self.buffer.push(stamp, self.cumulative)
        self.last_stamp = stamp
        return True
