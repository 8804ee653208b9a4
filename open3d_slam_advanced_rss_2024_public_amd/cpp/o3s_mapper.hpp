// o3s_mapper.hpp — header-only C++17 restatement of the caller glue around the two ICP calls:
// o3d_slam::Mapper::addRangeMeasurement (open3d_slam/src/Mapper.cpp:168-504), with every cloud operation on the device
// (o3s_scan / o3s_submap / o3s_icp over the C ABI).  It is what a catkin package would compile instead of the reference's
// Mapper.cpp body; no Eigen / Open3D / libpointmatcher headers are needed.  Line numbers below are Mapper.cpp's.
//
//   :168-174      no calibration set (and no initial map): return false
//   :176          submaps_->setMapToRangeSensor(mapToRangeSensor_)
//   :179-195      first scan: pre-process, insert at the given pose, push the pose buffers
//   :197-235      out-of-order timestamp: propagate the previous pose by the odometry motion, no registration
//   :237-262      odometry availability (a pose within 100 ms of the buffer's latest counts as available)
//   :219-224, :268-280   with MapperParams::isInterpolateOdometry the odometry poses of both stamps come from getTransform over an
//                 interpolating buffer (clamped before it, extrapolated after it), as in the reference; without it (the default)
//                 they are read at exact stamps only
//   :106-115      getMapToOdom / getMapToRangeSensor: getTransform over the registered poses and the odometry
//   :265-281      prior = mapToRangeSensorPrev_ * ((odomPrev * C^-1)^-1 * (odomNow * C^-1)), C = calibration_ (:221-222, :270-273),
//                 unless isNewValueSetMapper_ / isIgnoreOdometryPrediction_
//   :305-318, :359-376, :382-411, :481-501   the four stage stopwatches (o3d_slam::Timer): lastTimings() / meanTimings()
//   :307-309      processForScanMatchingAndMerging + open3dToPointmatcher        -> o3s_scan_preprocess + o3s_scan_set_reading
//   :323          prior cast to float (PmTfParameters)
//   :328-336      cropSubmap(activeSubmap, mapToRangeSensor_); empty patch -> return false
//   :346-366      every referenceCloudSettingPeriod_ seconds (or after a pose reset): open3dToPointmatcher(patch) +
//                 icp_.initReference                                             -> o3s_submap_set_reference
//   :393          icp_.compute(reading, {}, prior, false)                         -> o3s_icp_compute_resident
//   :420-422      catch (std::runtime_error): keep the prior
//   :424-431      the health gate (commented out in the reference, whose libpointmatcher result has no fitness_ left to test): when
//                 isIgnoreMinRefinementFitness is off, a registration whose fitness (o3s_icp_evaluate_resident at the pose it
//                 returned) is below minRefinementFitness gives the scan up: return false, nothing adopted, pushed or inserted
//   :435          result cast back to double
//   (no counterpart) degeneracyPolicy: the localizability analysis of that registration (o3s_localizability.h) behind the compute;
//                 Report keeps it for getLatestLocalizability(), Remap also replaces the pose by o3s_localizability_remap(prior, result):
//                 the ICP's correction in the directions the scan constrained, the prior in the others.  Off (the default): no call
//   :440-455      isNewValueSetMapper_: adopt the GIVEN pose, skip this scan's result and the insert, ignore odometry next time
//   :465-479      initial-map mode: no merging (or not before mapMergeDelayInSeconds_)
//   :483-489      insert the merge cloud if the sensor moved at least minMovementBetweenMappingSteps_
//   :190, 228, 450, 460   mapToRangeSensorBuffer_.push: the registered poses, which motionCompensationMap_ reads
//                 (SlamWrapper.cpp:445-447, 671: undistortInputPointCloud before the mapper sees the sweep) -> enableMotionCompensation
//   :506-538      getAssembledMapPointCloud: the map of all submaps                -> o3s_assembled_map_build (AssembledMapHip)
// 4x4 matrices are column-major doubles (Eigen::Matrix4d::data()).  Isometry products / inverses are restated as plain
// k = 0..3 accumulations (Eigen is not part of the tree: its evaluation order is not pinned).
#pragma once

#include <chrono>
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>

#include "o3s_icp.hpp"
#include "o3s_odometry.hpp"
#include "o3s_pose.hpp"
#include "o3s_pose_search.hpp"
#include "o3s_scan.h"
#include "o3s_submap_collection.hpp"
#include "outlier_removal/o3s_outlier_removal.h"
#include "clustering/o3s_clustering.h"

namespace o3s {

// o3d_slam::TransformInterpolationBuffer restricted to what the Mapper asks of it when the odometry is sampled at the
// scan stamps: has(t), latest_time(), lookup(t) of an exact stamp.  It is the odometry buffer while
// MapperParams::isInterpolateOdometry is off; the interpolating one is o3s_odometry.hpp's TransformInterpolationBuffer
class PoseBuffer {
 public:
  void push(double t, const Mat4& T) { poses_[t] = T; }
  bool has(double t) const { return poses_.count(t) != 0; }
  bool empty() const { return poses_.empty(); }
  double latest_time() const { return poses_.rbegin()->first; }
  const Mat4& lookup(double t) const {
    auto it = poses_.find(t);
    if (it == poses_.end()) throw std::runtime_error("PoseBuffer: no pose at the requested stamp");
    return it->second;
  }

 private:
  std::map<double, Mat4> poses_;
};

// The Mapper's four stopwatches (Mapper.cpp:305-318 "Auxilary time", :359-376 "Reference Cloud Re-init time", :382-411
// "Scan2Map Registration", :481-501 "Scan Insertion"), wall-clock milliseconds like o3d_slam::Timer; 0 for a stage a scan skipped
struct MapperTimings {
  double auxiliaryMs = 0.0, referenceInitMs = 0.0, registrationMs = 0.0, insertionMs = 0.0;
};

struct MapperParams {
  double scanVoxelSize = 0.1;                        // scanProcessing_.voxelSize_
  double mapVoxelSize = 0.1;                         // mapBuilder_.mapVoxelSize_
  o3s_cropper mapBuilderCropper{};                   // wide crop of the raw scan / volume the map is re-voxelised in
  o3s_cropper scanMatcherCropper{};                  // narrow crop of the scan / of the map patch
  double referenceCloudSettingPeriod = 1.0;          // scanMatcher_.icp_.referenceCloudSettingPeriod_ (Parameters.hpp:71)
  double minMovementBetweenMappingSteps = 0.0;       // Parameters.hpp
  bool isUseInitialMap = false;
  bool isMergeScansIntoMap = true;
  double mapMergeDelayInSeconds = 0.0;
  SubmapParams submaps;                              // submaps_ (Parameters.hpp:103-109): radius_, minNumRangeData_, ...
  double minRefinementFitness = 0.7;                 // scanMatcher_.minRefinementFitness_ (Parameters.hpp:151; min_refinement_fitness)
  // isIgnoreMinRefinementFitness_ (Parameters.hpp:167).  true = the reference as it runs: its flag defaults to false, but its gate is
  // commented out (Mapper.cpp:424-431), so "ignore" is what it does
  bool isIgnoreMinRefinementFitness = true;
  double fitnessMaxCorrespondenceDistance = 0.0;     // the radius the fitness counts inliers within; 0 = the ICP chain's maxDist
  // The odometry prior at ANY stamp (Mapper.cpp:219-224, 237-261, 268-280): getTransform over an interpolating buffer, which is what
  // an external odometry source needs (its poses never carry the LiDAR's stamps).  false = exact stamps only, as before
  bool isInterpolateOdometry = false;
  // What to do about a registration whose scan left directions of the pose unconstrained (a corridor, a tunnel, an open field).
  // Off: nothing, not even the analysis.  Report: run it, keep the result.  Remap: also keep the prior in the directions whose
  // category is below remapMinCategory.  `localizability`: the thresholds — its three sums have no default and must be calibrated
  // (run Report on a well-constrained recording and read sum_all / sum_strong); unset, Report and Remap throw at construction.
  // Constrain: every ICP iteration solves its step with no component along the directions whose category is below remapMinCategory
  // (IcpHip::setDegeneracy, mode ANALYSE, include/degeneracy/o3s_degeneracy.h); the analysis behind the compute is kept as for Report.
  enum class DegeneracyPolicy { Off, Report, Remap, Constrain };
  DegeneracyPolicy degeneracyPolicy = DegeneracyPolicy::Off;
  o3s_localizability_params localizability = defaultLocalizability();
  std::int32_t remapMinCategory = 1;
  // Constrain only: a partially localizable direction (category 1) is constrained to the step its strong pairs alone ask for
  // (IcpHip::setDegeneracyPartial, include/degeneracy/o3s_degeneracy_partial.h) instead of to zero (remapMinCategory 2) or not
  // at all (remapMinCategory 1)
  bool degeneracyPartial = false;
  // An outlier filter (include/outlier_removal/o3s_outlier_removal.h: Open3D's RemoveRadiusOutliers / RemoveStatisticalOutliers) on
  // every sweep the mapper pre-processes ITSELF, right behind the pre-processing: stray returns then reach neither the registration
  // nor the map.  kind 0 (the default): no call is made.  A caller that hands over an already pre-processed scan
  // (addRangeMeasurement(o3s_scan*&, ...)) filters it itself, with o3s_scan_remove_outliers and this mapper's scanMatcherCropper
  o3s_outlier_params scanOutlierRemoval{0, 0, 0.0};
  // Small-cluster removal (include/clustering/o3s_clustering.h: Open3D's ClusterDBSCAN, then every cluster below min_cluster_size
  // points and all noise dropped) on the same sweeps, right behind the outlier filter: what that filter cannot take out — the
  // supported blob a pedestrian or a dust cloud leaves.  min_points 0 (the default): no call is made.  A caller that hands over
  // an already pre-processed scan filters it itself, with o3s_scan_remove_small_clusters and this mapper's scanMatcherCropper
  o3s_dbscan_params scanClusterRemoval{0.0, 0, 0};
  static o3s_localizability_params defaultLocalizability() {
    o3s_localizability_params p;
    o3s_localizability_default_params(&p);
    return p;
  }
};

class MapperHip {
 public:
  MapperHip(const MapperParams& p, const o3s_icp_config& icpCfg, int device = 0)
      : params_(p), icp_(icpCfg, device), submaps_(p.submaps, p.mapVoxelSize, p.mapBuilderCropper, p.isUseInitialMap, device), device_(device) {
    if (p.degeneracyPolicy != MapperParams::DegeneracyPolicy::Off) {
      o3s_localizability unused;  // (a NULL handle: the parameters are checked first, nothing else is)
      if (o3s_icp_localizability(nullptr, &p.localizability, &unused) == O3S_ERR_BAD_CONFIG)
        throw std::runtime_error("MapperParams::localizability: the thresholds are unset or out of order");
      if (p.remapMinCategory != 1 && p.remapMinCategory != 2) throw std::runtime_error("MapperParams::remapMinCategory must be 1 or 2");
      if (p.degeneracyPolicy == MapperParams::DegeneracyPolicy::Constrain) {
        icp_.setDegeneracy(O3S_DEGENERACY_ANALYSE, nullptr, &p.localizability, p.remapMinCategory);
        if (p.degeneracyPartial) icp_.setDegeneracyPartial(true);
      }
    }
    lastLocalizability_.kept = -1;
  }
  ~MapperHip() { o3s_raw_scan_destroy(deskewStage_); }
  MapperHip(const MapperHip&) = delete;
  MapperHip& operator=(const MapperHip&) = delete;

  // Mapper::setMapToRangeSensorInitial / setMapToRangeSensor with a new value (Mapper.cpp:96-118): the next scan adopts it
  void setMapToRangeSensorInitial(const Mat4& T) {
    mapToRangeSensor_ = T;
    mapToRangeSensorPrev_ = T;
    isNewValueSetMapper_ = true;
  }
  void setMapToRangeSensor(const Mat4& T) { mapToRangeSensor_ = T; }  // first-scan pose (no flag: Mapper.cpp:179-195)
  // The start pose of the localisation mode, FOUND instead of dragged (SlamMapInitializer's interactive marker): the sweep is
  // pre-processed as addRangeMeasurement would, o3s::localize searches `search`'s grid in the active submap's occupancy snapshot —
  // which the caller has built: activeSubmap().buildVoxelMap — and refines the winners, and an accepted pose goes through
  // setMapToRangeSensorInitial.  Valid only with isUseInitialMap, once the map is in and before the first measurement: otherwise,
  // and when no candidate reaches minFitness, nothing of the mapper's state changes and the answer is false.  Never called
  // implicitly: a mapper that does not call it launches and allocates what it always did.
  bool localizeInitialPose(const double* rawPts, const double* rawNormals, std::int64_t N, const o3s_pose_search_params& search, double minFitness) {
    if (!params_.isUseInitialMap || submaps_.activeSubmap().empty() || haveLast_ || !mapToRangeSensorBuffer_.empty()) return false;
    scan_ = submaps_.scanForNextMeasurement();
    preprocess(Raw{rawPts, rawNormals, N, nullptr, nullptr}, 0.0);
    lastLocalize_ = localize(submaps_.activeSubmap(), scan_, icp_, params_.scanMatcherCropper, search, minFitness, params_.fitnessMaxCorrespondenceDistance);
    if (!lastLocalize_.ok) return false;
    setMapToRangeSensorInitial(lastLocalize_.T);
    return true;
  }
  const LocalizeResult& lastLocalize() const { return lastLocalize_; }  // of the last localizeInitialPose that searched
  // Mapper::loopClosureUpdate (Mapper.cpp:93-96)
  void loopClosureUpdate(const Mat4& loopClosureCorrection) {
    mapToRangeSensor_ = mul(loopClosureCorrection, mapToRangeSensor_);
    mapToRangeSensorPrev_ = mul(loopClosureCorrection, mapToRangeSensorPrev_);
  }
  void addOdometryPose(double t, const Mat4& odomToRangeSensor) {
    odomToRangeSensorBuffer_.push(t, odomToRangeSensor);
    odomInterpolationBuffer_.push(t, odomToRangeSensor);
  }
  const TransformInterpolationBuffer& getOdomToRangeSensorBuffer() const { return odomInterpolationBuffer_; }
  // Mapper::getMapToRangeSensor / getMapToOdom (Mapper.cpp:106-115)
  Mat4 getMapToRangeSensor(double t) const { return getTransform(t, mapToRangeSensorBuffer_); }
  Mat4 getMapToOdom(double t) const {
    return mul(getTransform(t, mapToRangeSensorBuffer_), inverse_isometry(getTransform(t, odomInterpolationBuffer_)));
  }
  // Mapper::setExternalOdometryFrameToCloudFrameCalibration (Mapper.cpp:66-85): the odometry poses are those of ANOTHER frame
  // (the tracking camera / IMU); every lookup is multiplied by calibration^-1 before the motion is formed (:221-222, :270-273)
  void setCalibration(const Mat4& odometryFrameToCloudFrame) {
    calibration_ = odometryFrameToCloudFrame;
    calibrationInv_ = inverse_isometry(odometryFrameToCloudFrame);
    isCalibrationSet_ = true;
  }
  bool isCalibrationSet() const { return isCalibrationSet_; }
  // motion_compensation.is_undistort_scan (off by default): every sweep handed over as host arrays is staged, de-skewed with the
  // velocities of the registered poses (ConstantVelocityMotionCompensation over getMapToRangeSensorBuffer()) and pre-processed from
  // the staged copy.  A sweep the caller has staged itself is de-skewed with undistort(staged, stamp) before it is handed over, as
  // SlamWrapper.cpp:671 does before the mapper sees the cloud; a sweep that arrives pre-processed was de-skewed before that.
  void enableMotionCompensation(double scanDuration = 0.1, bool isSpinningClockwise = true, int numPosesVelocityEstimation = 3) {
    if (trajectoryCompensation_) throw std::runtime_error("the trajectory motion compensation is already enabled");
    motionCompensation_.reset(new ConstantVelocityMotionCompensation(mapToRangeSensorBuffer_, scanDuration, isSpinningClockwise,
                                                                     numPosesVelocityEstimation));
  }
  bool isMotionCompensationEnabled() const { return (bool)motionCompensation_; }
  o3s_motion undistort(o3s_raw_scan* staged, double timestamp) {
    if (!motionCompensation_) throw std::runtime_error("undistort: motion compensation is not enabled");
    lastMotion_ = motionCompensation_->undistort(staged, timestamp);
    return lastMotion_;
  }
  const o3s_motion& lastMotion() const { return lastMotion_; }
  // The de-skew along the odometry's trajectory (off by default), the twin of the two above: every sweep handed over as host arrays
  // is staged, de-skewed along the poses addOdometryPose was given (whatever isInterpolateOdometry says) and pre-processed from the
  // staged copy; a sweep the caller has staged itself — with o3s_raw_scan_set_point_times where the driver provides point times —
  // is de-skewed with undistortAlongOdometry(staged, stamp) before it is handed over.  Host arrays carry no point times: their
  // points are timed by azimuth.
  void enableTrajectoryMotionCompensation(double scanDuration = 0.1, bool isSpinningClockwise = true) {
    if (motionCompensation_) throw std::runtime_error("the constant-velocity motion compensation is already enabled");
    trajectoryCompensation_.reset(new TrajectoryMotionCompensation(odomInterpolationBuffer_, scanDuration, isSpinningClockwise));
  }
  bool isTrajectoryMotionCompensationEnabled() const { return (bool)trajectoryCompensation_; }
  void undistortAlongOdometry(o3s_raw_scan* staged, double timestamp) {
    if (!trajectoryCompensation_) throw std::runtime_error("undistortAlongOdometry: trajectory motion compensation is not enabled");
    trajectoryCompensation_->undistort(staged, timestamp, calibration_);
  }
  const TransformBuffer& getMapToRangeSensorBuffer() const { return mapToRangeSensorBuffer_; }
  const MapperTimings& lastTimings() const { return lastTimings_; }
  MapperTimings meanTimings() const {  // Timer::getAvgMeasurementMsec over the scans that ran the stage
    MapperTimings m;
    m.auxiliaryMs = nTimed_[0] ? sumTimings_.auxiliaryMs / nTimed_[0] : 0.0;
    m.referenceInitMs = nTimed_[1] ? sumTimings_.referenceInitMs / nTimed_[1] : 0.0;
    m.registrationMs = nTimed_[2] ? sumTimings_.registrationMs / nTimed_[2] : 0.0;
    m.insertionMs = nTimed_[3] ? sumTimings_.insertionMs / nTimed_[3] : 0.0;
    return m;
  }
  // initial map for the localisation mode (isUseInitialMap_): Mapper.cpp:180-183 inserts it as the first "scan"
  SubmapHip& activeSubmap() { return submaps_.activeSubmap(); }
  SubmapCollectionHip& submaps() { return submaps_; }
  // Mapper::getAssembledMapPointCloud (Mapper.cpp:506-538) into the resident `out`: the map clouds of all submaps in index order with
  // the normals and colours every submap carries; voxelSize > 0 also down-samples it (SlamWrapperRos::publishMaps).  Returns the size;
  // out.download() is the one copy to the host.  Call it from the mapping thread.
  std::int64_t getAssembledMapPointCloud(AssembledMapHip& out, double voxelSize = 0.0) { return submaps_.assembleMap(out, voxelSize); }
  IcpHip& icp() { return icp_; }
  const Mat4& mapToRangeSensor() const { return mapToRangeSensor_; }
  const Mat4& lastPrior() const { return lastPrior_; }
  bool lastScanInserted() const { return lastInserted_; }
  bool lastReferenceReset() const { return lastReferenceReset_; }
  bool lastIcpThrew() const { return lastIcpThrew_; }
  int lastIterations() const { return lastIterations_; }
  // the fitness the health gate read on the last scan (fitness NaN: the gate is ignored, the scan never reached the registration,
  // or the ICP threw), and whether it gave the scan up
  const o3s_icp_fitness& lastFitness() const { return lastFitness_; }
  bool lastFitnessRejected() const { return lastFitnessRejected_; }
  // covariance of the latest scan-to-map registration (IcpHip::getCovariance: zeros under the plain minimiser); NaN when that
  // registration failed and the prior was kept (Mapper.cpp:420-422), or before the first one
  const std::array<double, 36>& getLatestRegistrationCovariance() const { return lastCovariance_; }
  // the localizability analysis of the latest scan-to-map registration (degeneracyPolicy Report / Remap); kept = -1 when there is
  // none: the policy is Off, that registration failed, or before the first one.  lastRemapReplaced(): the directions in which
  // Remap kept the prior on the last scan (0 under Off / Report)
  const o3s_localizability& getLatestLocalizability() const { return lastLocalizability_; }
  int lastRemapReplaced() const { return lastRemapReplaced_; }
  // the pose the ICP itself returned on the last scan, before any remap (the prior when it threw)
  const Mat4& lastRegistrationPose() const { return lastRegistrationPose_; }

  // rawScan in the sensor frame (3 x N doubles, normals nullable when normal estimation is configured on the scan object)
  bool addRangeMeasurement(const double* rawPts, const double* rawNormals, std::int64_t N, double timestamp) {
    return add(Raw{rawPts, rawNormals, N, nullptr, nullptr}, timestamp);
  }
  // The same with the raw sweep staged in HBM beforehand (o3s_raw_scan_upload, typically from the thread that receives the
  // sweeps — the reference's mapping worker is fed from a buffer too, SlamWrapper.cpp:660-709): the host-to-device copy of
  // sweep k + 1 then runs while this thread still registers sweep k.
  bool addRangeMeasurement(const o3s_raw_scan* staged, double timestamp) {
    if (!staged) throw std::runtime_error("addRangeMeasurement: no staged scan");
    return add(Raw{nullptr, nullptr, o3s_raw_scan_size(staged), staged, nullptr}, timestamp);
  }
  // The same with the sweep already PRE-PROCESSED by the receiving thread: o3s_scan_preprocess with THIS mapper's croppers and
  // scan voxel size (params()) into a scan object of the caller's, on that object's own stream, while this thread still
  // registers and inserts sweep k.  The pre-processing does not depend on the pose (both croppers sit at the sensor,
  // ScanToMapRegistration.cpp:36-69), so the result is the same bits; the "Auxilary time" stage of this call shrinks to a
  // pointer exchange.  On return `preprocessed` is a spare object to fill next (the filled one has joined the ring of
  // resident scans the submap collection keeps for its overlap buffer); when the call returns before the pre-processing
  // stage — no calibration yet, an out-of-order stamp — it is left as it was.
  bool addRangeMeasurement(o3s_scan*& preprocessed, double timestamp) {
    if (!preprocessed) throw std::runtime_error("addRangeMeasurement: no pre-processed scan");
    return add(Raw{nullptr, nullptr, 0, nullptr, &preprocessed}, timestamp);
  }
  const MapperParams& params() const { return params_; }

 private:
  struct Raw {
    const double* pts;
    const double* normals;
    std::int64_t N;
    const o3s_raw_scan* staged;
    o3s_scan** ready;  // a scan object the caller has already pre-processed this sweep into
  };
  bool add(const Raw& raw, double timestamp) {
    lastInserted_ = lastReferenceReset_ = lastIcpThrew_ = lastFitnessRejected_ = false;
    lastFitness_ = o3s_icp_fitness{};
    lastFitness_.fitness = std::numeric_limits<double>::quiet_NaN();
    bool haveFitness = false, haveLocalizability = false;
    lastLocalizability_ = o3s_localizability{};
    lastLocalizability_.kept = -1;
    lastRemapReplaced_ = 0;
    lastTimings_ = MapperTimings{};
    if (!params_.isUseInitialMap && !isCalibrationSet_) return false;  // "Calibration is not set. Returning from mapping." (:169-174)
    scan_ = submaps_.scanForNextMeasurement();  // stays ours until submaps_.insertScan takes it into its overlap buffer
    // ---- first scan (:179-195) ----
    if (submaps_.activeSubmap().empty()) {
      if (params_.isUseInitialMap) {  // the raw "scan" IS the map: inserted as is (:181-183)
        if (raw.staged || raw.ready) throw std::runtime_error("the initial map is handed over as host arrays");
        submaps_.activeSubmap().insertScan(raw.pts, raw.normals, raw.N, mapToRangeSensor_.m);
      } else {
        mapToRangeSensorPrev_ = mapToRangeSensor_;
        preprocess(raw, timestamp);
        submaps_.insertScan(scan_, mapToRangeSensor_.m, timestamp);
        mapToRangeSensorBuffer_.push(timestamp, mapToRangeSensor_);
        lastInserted_ = true;
      }
      return true;
    }
    // ---- out-of-order stamp (:197-235): propagate by the odometry motion, no registration ----
    if (haveLast_ && timestamp <= lastMeasurementTimestamp_) {
      const double latest = params_.isInterpolateOdometry ? odomInterpolationBuffer_.latest_time() : odomToRangeSensorBuffer_.latest_time();
      const Mat4 motion = mul(inverse_isometry(odomInCloudFrame(lastMeasurementTimestamp_)), odomInCloudFrame(latest));
      mapToRangeSensor_ = mul(mapToRangeSensorPrev_, motion);
      mapToRangeSensorBuffer_.push(latest, mapToRangeSensor_);
      mapToRangeSensorPrev_ = mapToRangeSensor_;
      return true;
    }
    // ---- odometry prior (:237-281) ----
    bool isOdomOkay, havePoses;
    if (params_.isInterpolateOdometry) {  // both poses come from getTransform: no further condition (:268-273)
      const TransformInterpolationBuffer& b = odomInterpolationBuffer_;
      isOdomOkay = b.has(timestamp) || (!b.empty() && (timestamp - b.latest_time()) * 1e3 < 100.0);
      havePoses = true;
    } else {
      isOdomOkay = odomToRangeSensorBuffer_.has(timestamp);
      if (!odomToRangeSensorBuffer_.empty() && (timestamp - odomToRangeSensorBuffer_.latest_time()) * 1e3 < 100.0) isOdomOkay = true;
      havePoses = odomToRangeSensorBuffer_.has(timestamp) && odomToRangeSensorBuffer_.has(lastMeasurementTimestamp_);
    }
    Mat4 estimate = mapToRangeSensorPrev_;
    if (isOdomOkay && haveLast_ && !isNewValueSetMapper_ && !isIgnoreOdometryPrediction_ && havePoses) {
      const Mat4 motion = mul(inverse_isometry(odomInCloudFrame(lastMeasurementTimestamp_)), odomInCloudFrame(timestamp));
      estimate = mul(mapToRangeSensorPrev_, motion);
    }
    isIgnoreOdometryPrediction_ = false;
    lastPrior_ = estimate;
    // ---- pre-processing on the device (:307-309), under the "Auxilary time" stopwatch (:305-312) ----
    auto t0 = Clock::now();
    preprocess(raw, timestamp);
    stamp(t0, lastTimings_.auxiliaryMs, sumTimings_.auxiliaryMs, 0);
    float prior32[16], corrected32[16];
    for (int k = 0; k < 16; ++k) corrected32[k] = prior32[k] = (float)estimate.m[k];  // :323, :338
    // ---- map patch + reference (:328-366) ----
    o3s_cropper patch = params_.scanMatcherCropper;
    for (int a = 0; a < 3; ++a) patch.centre[a] = mapToRangeSensor_(a, 3);  // cropSubmap: setPose(mapToRangeSensor_)
    const bool resetRef = isNewValueSetMapper_ || !haveRef_ || (timestamp - lastReferenceInitializationTimestamp_) >= params_.referenceCloudSettingPeriod;
    // the reference crops the submap on EVERY scan and gives the scan up when the patch is empty (:328-336) — also between two
    // renewals of the ICP reference (a patch emptied by carving or a submap switch must not be registered against a stale index).
    // On those scans the count needs the map as the previous insert left it, the registration does not (it runs against the index
    // of an earlier renewal): the chain is put on the GPU first (o3s_icp_compute_resident_launch), the patch is counted while it
    // runs — completing the pending insert —, and an empty patch gives the scan up exactly as before, the finished chain unused.
    std::int64_t nPatchNow = -1;
    try {
      if (resetRef) {  // "Reference Cloud Re-init time" (:359-370)
        t0 = Clock::now();
        std::int64_t nPatch = 0;
        if (!submaps_.activeSubmap().setReference(patch, mapToRangeSensor_.m, icp_, &nPatch)) return false;  // "Map patch is empty" / initReference failed
        lastReferenceInitializationTimestamp_ = timestamp;
        haveRef_ = true;
        lastReferenceReset_ = true;
        stamp(t0, lastTimings_.referenceInitMs, sumTimings_.referenceInitMs, 1);
      }
      t0 = Clock::now();  // "Scan2Map Registration" (:382-405)
      check(o3s_scan_set_reading(scan_, icp_.handle()), "o3s_scan_set_reading");
      o3s_icp_stats st{};
      int rc;
      if (resetRef) {
        rc = o3s_icp_compute_resident(icp_.handle(), prior32, corrected32, &st);
      } else {
        const int rl = o3s_icp_compute_resident_launch(icp_.handle(), prior32);
        try {
          nPatchNow = submaps_.activeSubmap().patchCount(patch, mapToRangeSensor_.m);
        } catch (...) {
          if (rl == O3S_OK) (void)o3s_icp_compute_resident_finish(icp_.handle(), corrected32, &st);
          throw;
        }
        rc = rl == O3S_OK ? o3s_icp_compute_resident_finish(icp_.handle(), corrected32, &st) : rl;
        if (nPatchNow == 0) {  // "Map patch is empty": the scan is given up (:333-336); nothing of the registration is kept
          (void)o3s_icp_synchronize(icp_.handle());
          return false;
        }
      }
      lastIterations_ = st.iterations;
      if (rc != O3S_OK) throw std::runtime_error(o3s_last_error(icp_.handle()));  // every libpointmatcher exception derives from it
      lastCovariance_ = icp_.getCovariance();
      if (params_.degeneracyPolicy != MapperParams::DegeneracyPolicy::Off) {  // before the fitness: that replaces the match streams
        lastLocalizability_ = icp_.localizability(params_.localizability);
        haveLocalizability = true;
      }
      if (!params_.isIgnoreMinRefinementFitness) {  // result.fitness_ of :425, inside the registration's stopwatch
        lastFitness_ = icp_.evaluate(nullptr, (float)params_.fitnessMaxCorrespondenceDistance);
        haveFitness = true;
      }
      stamp(t0, lastTimings_.registrationMs, sumTimings_.registrationMs, 2);
    } catch (const std::runtime_error&) {
      // (a scan whose reading could not even be handed over: the reference would have looked at the patch first)
      if (!resetRef && nPatchNow < 0 && submaps_.activeSubmap().patchCount(patch, mapToRangeSensor_.m) == 0) return false;
      lastIcpThrew_ = true;  // :420-422: the prior stays (corrected32 must not hold a half-written result)
      lastCovariance_.fill(std::numeric_limits<double>::quiet_NaN());
      haveLocalizability = false;
      lastLocalizability_ = o3s_localizability{};
      lastLocalizability_.kept = -1;
      for (int k = 0; k < 16; ++k) corrected32[k] = prior32[k];
      // a compute that failed before it waited for its stream may leave the asynchronous index build / the reading's hand-over in
      // flight: nothing below may rewrite the buffers they read until the handle's stream has drained
      (void)o3s_icp_synchronize(icp_.handle());
    }
    // ---- health gate (:424-431): "Skipping the refinement step" ----
    if (haveFitness && lastFitness_.fitness < params_.minRefinementFitness) {
      lastFitnessRejected_ = true;
      return false;
    }
    Mat4 corrected{};
    for (int k = 0; k < 16; ++k) corrected.m[k] = (double)corrected32[k];  // :435
    lastRegistrationPose_ = corrected;
    if (haveLocalizability && params_.degeneracyPolicy == MapperParams::DegeneracyPolicy::Remap) {
      // the prior is the initial guess the chain was handed (fp32, :323); with every direction kept the result is copied bit for bit
      Mat4 prior{}, remapped{};
      for (int k = 0; k < 16; ++k) prior.m[k] = (double)prior32[k];
      std::int32_t replaced = 0;
      if (o3s_localizability_remap(&lastLocalizability_, params_.remapMinCategory, prior.m, corrected.m, remapped.m, &replaced) == O3S_OK) {
        corrected = remapped;
        lastRemapReplaced_ = (int)replaced;
      }  // (refused: a correction of pi / 2 or more is not one to linearise — the ICP's pose stays)
    }
    // ---- pose reset (:440-455) ----
    if (isNewValueSetMapper_) {  // the GIVEN pose is adopted; lastMeasurementTimestamp_ is left as it was (:440-455)
      initTime_ = timestamp;
      mapToRangeSensorPrev_ = mapToRangeSensor_;
      mapToRangeSensorBuffer_.push(timestamp, mapToRangeSensor_);
      isNewValueSetMapper_ = false;
      isIgnoreOdometryPrediction_ = true;
      return true;
    }
    mapToRangeSensor_ = corrected;
    mapToRangeSensorBuffer_.push(timestamp, mapToRangeSensor_);
    // ---- localisation mode: no merging (:465-479) ----
    const double timeSinceInit = timestamp - initTime_;
    if ((params_.isUseInitialMap && !params_.isMergeScansIntoMap) ||
        (timeSinceInit < params_.mapMergeDelayInSeconds && params_.isUseInitialMap && params_.isMergeScansIntoMap)) {
      lastMeasurementTimestamp_ = timestamp;
      haveLast_ = true;
      mapToRangeSensorPrev_ = mapToRangeSensor_;
      return true;
    }
    // ---- insert (:483-489), under the "Scan Insertion" stopwatch (:481-495) ----
    t0 = Clock::now();
    const Mat4 motion = mul(inverse_isometry(mapToRangeSensorLastScanInsertion_), mapToRangeSensor_);
    const double moved = std::sqrt(motion(0, 3) * motion(0, 3) + motion(1, 3) * motion(1, 3) + motion(2, 3) * motion(2, 3));
    if (!(moved < params_.minMovementBetweenMappingSteps)) {
      submaps_.insertScan(scan_, mapToRangeSensor_.m, timestamp);  // :487 submaps_->insertScan(rawScan, *mergeScan, mapToRangeSensor_, timestamp)
      mapToRangeSensorLastScanInsertion_ = mapToRangeSensor_;
      lastInserted_ = true;
    }
    lastMeasurementTimestamp_ = timestamp;
    haveLast_ = true;
    mapToRangeSensorPrev_ = mapToRangeSensor_;
    stamp(t0, lastTimings_.insertionMs, sumTimings_.insertionMs, 3);
    return true;
  }

  using Clock = std::chrono::steady_clock;
  void stamp(const Clock::time_point& t0, double& last, double& sum, int which) {
    last = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    sum += last;
    nTimed_[which] += 1;
  }
  // getTransform(t, odomToRangeSensorBuffer_) * calibration_.inverse()   (:221-222, :270-273)
  Mat4 odomInCloudFrame(double t) const {
    if (params_.isInterpolateOdometry) return mul(getTransform(t, odomInterpolationBuffer_), calibrationInv_);
    return mul(odomToRangeSensorBuffer_.lookup(t), calibrationInv_);
  }
  void preprocess(const Raw& raw, double timestamp) {
    std::int64_t nMerge = 0, nMatch = 0;
    if ((motionCompensation_ || trajectoryCompensation_) && !raw.ready && !raw.staged) {  // host arrays: stage, de-skew, pre-process from the staged copy
      if (!deskewStage_) check(o3s_raw_scan_create(device_, &deskewStage_), "o3s_raw_scan_create");
      check(o3s_raw_scan_upload(deskewStage_, raw.pts, raw.normals, raw.N), "o3s_raw_scan_upload");
      if (motionCompensation_)
        lastMotion_ = motionCompensation_->undistort(deskewStage_, timestamp);
      else
        trajectoryCompensation_->undistort(deskewStage_, timestamp, calibration_);
      check(o3s_scan_preprocess_staged(scan_, &params_.mapBuilderCropper, params_.scanVoxelSize, &params_.scanMatcherCropper, deskewStage_, &nMerge,
                                       &nMatch),
            "o3s_scan_preprocess_staged");
      removeScanOutliers();
      return;
    }
    if (raw.ready) {  // pre-processed — and, where wanted, filtered — by the caller
      o3s_scan* filled = *raw.ready;
      *raw.ready = submaps_.exchangeScanForNextMeasurement(filled);
      scan_ = filled;
      return;
    }
    if (raw.staged)
      check(o3s_scan_preprocess_staged(scan_, &params_.mapBuilderCropper, params_.scanVoxelSize, &params_.scanMatcherCropper, raw.staged, &nMerge, &nMatch),
            "o3s_scan_preprocess_staged");
    else
      check(o3s_scan_preprocess(scan_, &params_.mapBuilderCropper, params_.scanVoxelSize, &params_.scanMatcherCropper, raw.pts, raw.normals, raw.N, &nMerge,
                                &nMatch),
            "o3s_scan_preprocess");
    removeScanOutliers();
  }
  // MapperParams::scanOutlierRemoval, then ::scanClusterRemoval, on the sweep just pre-processed; kind 0 / min_points 0: no call,
  // the loop is what it was
  void removeScanOutliers() {
    if (params_.scanOutlierRemoval.kind != 0)
      check(o3s_scan_remove_outliers(scan_, &params_.scanMatcherCropper, &params_.scanOutlierRemoval, nullptr, nullptr), "o3s_scan_remove_outliers");
    if (params_.scanClusterRemoval.min_points != 0)
      check(o3s_scan_remove_small_clusters(scan_, &params_.scanMatcherCropper, &params_.scanClusterRemoval, nullptr, nullptr),
            "o3s_scan_remove_small_clusters");
  }
  static void check(int rc, const char* what) {
    if (rc != O3S_OK) throw std::runtime_error(std::string(what) + " failed (status " + std::to_string(rc) + ")");
  }

  MapperParams params_;
  static std::array<double, 36> nanCovariance() {
    std::array<double, 36> c;
    c.fill(std::numeric_limits<double>::quiet_NaN());
    return c;
  }
  IcpHip icp_;
  SubmapCollectionHip submaps_;
  o3s_scan* scan_ = nullptr;  // owned by submaps_ (its ring of resident scans)
  PoseBuffer odomToRangeSensorBuffer_;                     // the odometry at exact stamps (isInterpolateOdometry off)
  TransformInterpolationBuffer odomInterpolationBuffer_;  // the odometry at any stamp (isInterpolateOdometry on; the trajectory de-skew)
  std::unique_ptr<TrajectoryMotionCompensation> trajectoryCompensation_;  // null: off
  TransformBuffer mapToRangeSensorBuffer_;  // the registered poses (Mapper::getMapToRangeSensorBuffer)
  std::unique_ptr<ConstantVelocityMotionCompensation> motionCompensation_;  // motionCompensationMap_; null: off
  o3s_raw_scan* deskewStage_ = nullptr;     // where a sweep handed over as host arrays is de-skewed
  o3s_motion lastMotion_{};
  int device_ = 0;
  Mat4 mapToRangeSensor_ = Mat4::identity(), mapToRangeSensorPrev_ = Mat4::identity(), lastPrior_ = Mat4::identity();
  Mat4 mapToRangeSensorLastScanInsertion_ = Mat4::identity(), lastRegistrationPose_ = Mat4::identity();
  double lastMeasurementTimestamp_ = 0.0, lastReferenceInitializationTimestamp_ = 0.0, initTime_ = 0.0;
  bool haveLast_ = false, haveRef_ = false;  // haveLast_: lastMeasurementTimestamp_ holds a stamp (the reference leaves it default-constructed after the first scan, whose lookup would throw: no odometry prior is formed then)
  bool isNewValueSetMapper_ = false, isIgnoreOdometryPrediction_ = false;
  bool lastInserted_ = false, lastReferenceReset_ = false, lastIcpThrew_ = false, lastFitnessRejected_ = false;
  o3s_icp_fitness lastFitness_{};
  LocalizeResult lastLocalize_;
  o3s_localizability lastLocalizability_{};
  int lastRemapReplaced_ = 0;
  std::array<double, 36> lastCovariance_ = nanCovariance();
  int lastIterations_ = 0;
  Mat4 calibration_ = Mat4::identity(), calibrationInv_ = Mat4::identity();
  bool isCalibrationSet_ = false;
  MapperTimings lastTimings_, sumTimings_;
  long long nTimed_[4] = {0, 0, 0, 0};
};

}  // namespace o3s
