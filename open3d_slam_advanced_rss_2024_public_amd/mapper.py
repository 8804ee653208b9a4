"""Python mirror of cpp/o3s_mapper.hpp (the caller glue of o3d_slam::Mapper::addRangeMeasurement, open3d_slam/src/Mapper.cpp:
168-504, over device-resident scans / submaps / the ICP handle): used by the tests to check the compiled header step by
step.  No compute here — every cloud operation is a call into the C-ABI library; the CPU tests of the control flow pass
stand-ins for the ICP, the submap collection and the cropping volumes."""
import numpy as np


def mul4(A, B):
    """4x4 product in the driver's operation order (plain k = 0..3 accumulation, no FMA)."""
    C_ = np.zeros((4, 4))
    for c in range(4):
        for r in range(4):
            s = A[r, 0] * B[0, c]
            s = s + A[r, 1] * B[1, c]
            s = s + A[r, 2] * B[2, c]
            s = s + A[r, 3] * B[3, c]
            C_[r, c] = s
    return C_


def inv_iso(T):
    R = np.eye(4)
    R[:3, :3] = T[:3, :3].T
    for r in range(3):
        s = R[r, 0] * T[0, 3]
        s = s + R[r, 1] * T[1, 3]
        s = s + R[r, 2] * T[2, 3]
        R[r, 3] = -s
    return R


class Mapper:
    """Mapper::addRangeMeasurement restated over the Python mirror (the same steps as cpp/o3s_mapper.hpp).

    icp / collection: the ICP handle and the SubmapCollection (device-backed in the GPU tests, stand-ins in the CPU tests of
    the control flow); wide / narrow: the map-builder and scan-matcher cropping volumes as objects the scan's preprocess and
    the submap's set_reference accept."""

    def __init__(self, icp, collection, wide, narrow, scan_voxel, ref_period, min_move):
        self.icp = icp
        self.col = collection
        self.wide, self.narrow, self.scan_voxel, self.ref_period, self.min_move = wide, narrow, scan_voxel, ref_period, min_move
        self.ps = None
        self.odom = {}
        self.T = np.eye(4)
        self.T_prev = np.eye(4)
        self.T_last_insert = np.eye(4)
        self.prior = np.eye(4)
        self.last_stamp = self.last_ref = None
        self.new_value = self.ignore_odom = False
        self.flags = (0, 0, 0)
        self.iters = 0
        # covariance of the latest scan-to-map registration (ICP.get_covariance: 6 x 6, [t, alpha beta gamma]; zeros under the plain
        # minimiser); NaN when that registration failed and the prior was kept (Mapper.cpp:420-422), or before the first one
        self.last_covariance = np.full((6, 6), np.nan)
        self.check = None     # set to a callable(scan inputs, state) to validate a step against the oracle
        self.calib_inv = np.eye(4)          # calibration_.inverse(); identity until set, as in the reference (Mapper.hpp) and MapperHip
        self.is_calibration_set = False     # isCalibrationSet_ (Mapper.cpp:66-85): until it is, every scan is refused (:169-174)
        self.use_initial_map = False
        self.last_localize = None           # pose_search.LocalizeResult of the last localize_initial_pose that searched
        # mapToRangeSensorBuffer_ (Mapper.cpp:190, 228, 450, 460): the registered poses; motionCompensationMap_ works over it
        # (SlamWrapper.cpp:445-447, 671).  Off by default: the sweep then reaches the pre-processing as it came.
        from .odometry import TransformBuffer
        self.pose_buffer = TransformBuffer()
        self.motion_compensation = None
        self.last_motion = None
        # the health gate of Mapper.cpp:424-431 (MapperParams of cpp/o3s_mapper.hpp): ignored by default, which is the reference as it
        # runs — its gate is commented out.  When it is not ignored, a registration whose fitness (ICP.evaluate at the pose it
        # returned) is below min_refinement_fitness gives the scan up: nothing is adopted, pushed or inserted
        self.min_refinement_fitness = 0.7
        self.ignore_min_refinement_fitness = True
        self.fitness_max_correspondence_distance = 0.0   # 0 = the ICP chain's max_dist
        self.last_fitness = None            # IcpFitness the gate read on the last scan; None: ignored, not reached, or the ICP threw
        self.last_fitness_rejected = False
        # MapperParams::isInterpolateOdometry.  Off: the odometry is the dict `odom`, read at exact stamps only.  On: the odometry
        # is odomToRangeSensorBuffer_ as the reference has it — add_odometry_pose feeds odom_buffer, and the prior is formed at
        # any stamp by getTransform (Mapper.cpp:219-224, 237-261, 268-280)
        from .odometry import TransformInterpolationBuffer
        self.interpolate_odometry = False
        self.odom_buffer = TransformInterpolationBuffer()
        self.calibration = np.eye(4)
        self.trajectory_compensation = None   # enable_trajectory_motion_compensation
        self.last_deskewed = None             # the sweep as the last trajectory de-skew handed it to the pre-processing
        # MapperParams::degeneracyPolicy (localizability.OFF / REPORT / REMAP): what to do about a registration whose scan left
        # directions of the pose unconstrained.  Off: no call at all.  Report: ICP.localizability behind the compute, kept in
        # last_localizability.  Remap: also the prior instead of the ICP's correction in the directions below remap_min_category.
        # Constrain: every ICP iteration solves its step with no component along the directions below remap_min_category
        # (ICP.set_degeneracy, mode ANALYSE, with localizability_params); the Report-style analysis still fills last_localizability.
        # localizability_params: localizability.LocalizabilityParams — its three sums have no default
        self.degeneracy_policy = "Off"
        self.localizability_params = None
        self.remap_min_category = 1
        # MapperParams::degeneracyPartial (Constrain only): a partially localizable direction (category 1) is constrained to the
        # step its strong pairs alone ask for (ICP.set_degeneracy_partial) instead of to zero or not at all
        self.degeneracy_partial = False
        self.last_localizability = None      # None: the policy is Off, that registration failed, or before the first one
        self.last_remap_replaced = 0
        self.last_registration_pose = np.eye(4)
        self._degeneracy_armed = None         # what the ICP handle was last told (Constrain): (params, min_category)
        # MapperParams::scanOutlierRemoval: an outlier filter (cloud_ops.outlier_params) on the pre-processed sweep, right behind the
        # pre-processing — stray returns then reach neither the registration nor the map.  None / kind 0: no call is made
        self.scan_outlier_removal = None
        # MapperParams::scanClusterRemoval: small-cluster removal (cloud_ops.dbscan_params) on the pre-processed sweep, right behind
        # the outlier filter — a blob of a few dozen supported points then reaches neither the registration nor the map.
        # None / min_points 0: no call is made
        self.scan_cluster_removal = None

    def set_calibration(self, C_):
        self.calibration = np.array(C_, np.float64).reshape(4, 4)
        self.calib_inv = inv_iso(self.calibration)
        self.is_calibration_set = True

    def add_odometry_pose(self, stamp, T):
        """Mapper::addOdometryPose: into the dict of exact stamps and into the interpolating buffer (the one in use is chosen by
        interpolate_odometry)."""
        T = np.array(T, np.float64).reshape(4, 4)
        self.odom[float(stamp)] = T
        self.odom_buffer.push(stamp, T)

    def enable_motion_compensation(self, scan_duration=0.1, is_spinning_clockwise=True, num_poses_vel_estimation=3):
        """motion_compensation.is_undistort_scan: every sweep is de-skewed with the velocities of the registered poses before the
        pre-processing sees it (ConstantVelocityMotionCompensation over getMapToRangeSensorBuffer())."""
        from .odometry import ConstantVelocityMotionCompensation
        if self.trajectory_compensation is not None:
            raise ValueError("the trajectory motion compensation is already enabled")
        self.motion_compensation = ConstantVelocityMotionCompensation(self.pose_buffer, scan_duration, is_spinning_clockwise,
                                                                      num_poses_vel_estimation)

    def enable_trajectory_motion_compensation(self, scan_duration=0.1, is_spinning_clockwise=True):
        """Every sweep is de-skewed along the odometry's trajectory (odom_buffer, whatever interpolate_odometry says) before the
        pre-processing sees it: each point is expressed in the sensor frame at the sweep's stamp.  Point times come from
        add(..., point_times=), else from the azimuth.  While the buffer is empty the sweep passes as it came."""
        from .odometry import TrajectoryMotionCompensation
        if self.motion_compensation is not None:
            raise ValueError("the constant-velocity motion compensation is already enabled")
        self.trajectory_compensation = TrajectoryMotionCompensation(self.odom_buffer, scan_duration, is_spinning_clockwise)

    def getMapToRangeSensor(self, stamp):
        """Mapper::getMapToRangeSensor (Mapper.cpp:113-115): getTransform over the registered poses."""
        from .odometry import get_transform
        return get_transform(stamp, self._registered())

    def getMapToOdom(self, stamp):
        """Mapper::getMapToOdom (Mapper.cpp:106-111): mapToRangeSensor(t) * odomToRangeSensor(t)^-1."""
        from .odometry import get_transform
        return mul4(get_transform(stamp, self._registered()), inv_iso(get_transform(stamp, self.odom_buffer)))

    def _registered(self):
        """pose_buffer as an interpolating buffer (the same pushes: the push rules are the same)."""
        from .odometry import TransformInterpolationBuffer
        b = TransformInterpolationBuffer(self.pose_buffer.size_limit)
        b._t, b._T = self.pose_buffer._t, self.pose_buffer._T
        return b

    def setMapToRangeSensorInitial(self, T):
        """Mapper::setMapToRangeSensorInitial (Mapper.cpp:96-118): the next scan adopts T."""
        self.T = np.array(T, np.float64).reshape(4, 4)
        self.T_prev = self.T.copy()
        self.new_value = True

    def localize_initial_pose(self, points, normals, params, min_fitness):
        """The start pose of the localisation mode, found instead of dragged (SlamMapInitializer's interactive marker): the sweep
        is pre-processed as add() would, pose_search.localize searches params' grid in the active submap's occupancy snapshot
        (the caller has built it: Submap.buildVoxelMap) and refines the winners, and an accepted pose goes through
        setMapToRangeSensorInitial.  Valid only with use_initial_map, once the map is in the active submap (Submap.setMapPointCloud:
        the initial map goes straight into it, as in cpp/o3s_mapper.hpp) and before the first measurement — no pose has been
        registered yet: otherwise, and when no candidate reaches min_fitness, nothing changes and the answer is False.  Never
        called implicitly; last_localize keeps the LocalizeResult of the last call that searched."""
        from .pose_search import localize
        if not self.use_initial_map or len(self.sm) == 0 or self.last_stamp is not None or not self.pose_buffer.empty():
            return False
        self.ps = self.col.scan_for_next()
        self.preprocess(points, normals)
        self.last_localize = localize(self.sm, self.ps, self.icp, self.narrow, params, min_fitness, self.fitness_max_correspondence_distance)
        if not self.last_localize.ok:
            return False
        self.setMapToRangeSensorInitial(self.last_localize.T)
        return True

    def loopClosureUpdate(self, loopClosureCorrection):
        """Mapper::loopClosureUpdate (Mapper.cpp:92-95).  The ICP reference is NOT renewed: until the next renewal the matcher still
        holds the patch that was cut before the correction, as in the reference."""
        dT = np.asarray(loopClosureCorrection, np.float64)
        self.T = mul4(dT, self.T)
        self.T_prev = mul4(dT, self.T_prev)

    def getAssembledMapPointCloud(self, out, voxel_size=0.0):
        """Mapper::getAssembledMapPointCloud (Mapper.cpp:506-538) into the resident `out` (submap.AssembledMap): the map clouds of
        all submaps in index order, normals and colours where every submap carries them; voxel_size > 0 also down-samples it
        (SlamWrapperRos::publishMaps).  Returns the size; out.getPointCloud() is the one copy to the host."""
        return self.col.assembleMap(out, voxel_size)

    def _odom(self, stamp):
        """getTransform(t, odomToRangeSensorBuffer_) * calibration_.inverse()   (Mapper.cpp:221-222, 270-273)"""
        if self.interpolate_odometry:
            from .odometry import get_transform
            return mul4(get_transform(stamp, self.odom_buffer), self.calib_inv)
        return mul4(self.odom[stamp], self.calib_inv)

    @property
    def sm(self):
        return self.col.maps[self.col.active]

    def preprocess(self, sp, sn, stamp=None, point_times=None):
        if self.trajectory_compensation is not None and stamp is not None:
            self.trajectory_compensation.calibration = self.calibration
            sp = self.trajectory_compensation.undistort_cloud(sp, stamp, point_times, getattr(self.icp, "device", 0))
            self.last_deskewed = sp
        if self.motion_compensation is not None and stamp is not None:   # SlamWrapper.cpp:671: undistortInputPointCloud(raw.cloud_, raw.time_)
            self.last_motion = self.motion_compensation.motion(stamp)
            from .odometry import undistort_cloud
            sp = undistort_cloud(sp, self.last_motion, getattr(self.icp, "device", 0))
        self.ps.preprocess(self.wide, self.scan_voxel, self.narrow, sp, sn)
        q = self.scan_outlier_removal
        if q is not None and q.kind != 0:   # kind 0 / None: no call at all — the loop is what it was
            self.ps.removeOutliers(self.narrow, q)
        c = self.scan_cluster_removal
        if c is not None and c.min_points != 0:   # min_points 0 / None: no call at all — the loop is what it was
            self.ps.removeSmallClusters(self.narrow, c)

    def _arm_degeneracy(self):
        """Constrain: the handle's degeneracy mode follows the policy (set again only when the policy or its parameters change)."""
        from . import localizability as loc

        want = None
        if self.degeneracy_policy == "Constrain":
            p = self.localizability_params
            want = (None if p is None else (p.filter_min, p.strong_min, p.sum_all_min, p.sum_strong_min, p.sum_partial_min), self.remap_min_category,
                    bool(self.degeneracy_partial))
        if want == self._degeneracy_armed:
            return
        if want is None:
            self.icp.set_degeneracy(loc.DEGENERACY_OFF)
            if self._degeneracy_armed is not None and self._degeneracy_armed[2]:
                self.icp.set_degeneracy_partial(False)
        else:
            self.icp.set_degeneracy(loc.DEGENERACY_ANALYSE, params=self.localizability_params or loc.LocalizabilityParams(),
                                    min_category=self.remap_min_category)
            if want[2] or (self._degeneracy_armed is not None and self._degeneracy_armed[2]):   # (a mapper that never asks makes no call)
                self.icp.set_degeneracy_partial(want[2])
        self._degeneracy_armed = want

    def add(self, sp, sn, stamp, point_times=None):
        """point_times: the driver's per-point time offsets (seconds after `stamp`), read by the trajectory motion compensation."""
        inserted = refreset = threw = 0
        self.flags = (0, 0, 0)
        self.last_fitness, self.last_fitness_rejected = None, False
        self.last_localizability, self.last_remap_replaced = None, 0
        if self.degeneracy_policy not in ("Off", "Report", "Remap", "Constrain"):
            raise ValueError("degeneracy_policy must be 'Off', 'Report', 'Remap' or 'Constrain'")
        self._arm_degeneracy()
        if not self.use_initial_map and not self.is_calibration_set:
            return False
        self.ps = self.col.scan_for_next()
        if len(self.sm) == 0:
            self.T_prev = self.T.copy()
            self.preprocess(sp, sn, stamp, point_times)
            self.col.insert(self.ps, self.T, stamp)
            self.pose_buffer.push(stamp, self.T)
            self.flags = (1, 0, 0)
            return True
        if self.last_stamp is not None and stamp <= self.last_stamp:
            latest = self.odom_buffer.latest_time() if self.interpolate_odometry else max(self.odom)
            self.T = mul4(self.T_prev, mul4(inv_iso(self._odom(self.last_stamp)), self._odom(latest)))
            self.pose_buffer.push(latest, self.T)
            self.T_prev = self.T.copy()
            return True
        est = self.T_prev.copy()
        if self.interpolate_odometry:   # isOdomOkay (Mapper.cpp:237-261); both poses come from getTransform, no further condition
            b = self.odom_buffer
            have = b.has(stamp) or (not b.empty() and (stamp - b.latest_time()) * 1e3 < 100.0)
        else:
            have = stamp in self.odom
        if have and self.last_stamp is not None and not self.new_value and not self.ignore_odom:
            est = mul4(self.T_prev, mul4(inv_iso(self._odom(self.last_stamp)), self._odom(stamp)))
        self.ignore_odom = False
        self.prior = est
        self.preprocess(sp, sn, stamp, point_times)
        prior32 = est.astype(np.float32)
        corrected32 = prior32.copy()
        reset = self.new_value or self.last_ref is None or (stamp - self.last_ref) >= self.ref_period
        state = None
        if not reset and self.sm.patch_count(self.narrow, self.T) == 0:   # cropSubmap on every scan: empty patch -> give up (:328-336)
            return False
        try:
            if reset:
                if self.check:
                    state = self.sm.getMapPointCloud()
                self.sm.set_reference(self.narrow, self.T, self.icp)
                self.last_ref = stamp
                refreset = 1
                self.ref_pose = self.T.copy()
                self.ref_state = state
            self.ps.set_reading(self.icp)
            corrected32 = self.icp.compute_resident(prior32)
            self.iters = self.icp.stats.iterations
            if hasattr(self.icp, "get_covariance"):   # (the CPU tests' stand-in handles register nothing and have none)
                self.last_covariance = self.icp.get_covariance()
            if self.degeneracy_policy != "Off":   # before the fitness: that replaces the match streams
                self.last_localizability = self.icp.localizability(self.localizability_params)
            if self.check and reset:
                self.check(self, sp, sn, prior32, corrected32)
            if not self.ignore_min_refinement_fitness:
                self.last_fitness = self.icp.evaluate(None, self.fitness_max_correspondence_distance)
        except RuntimeError:
            threw = 1
            corrected32 = prior32.copy()
            self.last_covariance = np.full((6, 6), np.nan)
            self.iters = self.icp.stats.iterations
            self.last_fitness = None
            self.last_localizability = None
        if self.last_fitness is not None and self.last_fitness.fitness < self.min_refinement_fitness:   # Mapper.cpp:425-430
            self.last_fitness_rejected = True
            self.flags = (0, refreset, threw)
            return False
        corrected = corrected32.astype(np.float64)
        self.last_registration_pose = corrected.copy()   # the ICP's own result, before any remap (the prior when it threw)
        if self.last_localizability is not None and self.degeneracy_policy == "Remap":
            from .localizability import remap_pose
            try:   # the prior is the initial guess the chain was handed (fp32); nothing replaced: the ICP's pose bit for bit
                corrected, self.last_remap_replaced = remap_pose(self.last_localizability, prior32.astype(np.float64), corrected,
                                                                 self.remap_min_category)
            except ValueError:   # a correction of pi / 2 or more is not one to linearise: the ICP's pose stays
                pass
        if self.new_value:
            self.T_prev = self.T.copy()
            self.pose_buffer.push(stamp, self.T)
            self.new_value = False
            self.ignore_odom = True
            self.flags = (0, refreset, threw)
            return True
        self.T = corrected
        self.pose_buffer.push(stamp, self.T)
        motion = mul4(inv_iso(self.T_last_insert), self.T)
        moved = np.sqrt(motion[0, 3] * motion[0, 3] + motion[1, 3] * motion[1, 3] + motion[2, 3] * motion[2, 3])
        if not (moved < self.min_move):
            self.col.insert(self.ps, self.T, stamp)
            self.T_last_insert = self.T.copy()
            inserted = 1
        self.last_stamp = stamp
        self.T_prev = self.T.copy()
        self.flags = (inserted, refreset, threw)
        return True
