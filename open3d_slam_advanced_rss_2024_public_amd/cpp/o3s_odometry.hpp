// o3s_odometry.hpp — header-only C++17 restatement of the reference's LiDAR-only front end over resident scans
// (include/o3s_scan.h), the same logic as the package's odometry.py; timestamps are double seconds.  O3S = open3d_slam/src.
//
//   TransformBuffer                      TransformInterpolationBuffer.cpp: the push rules (:22-46), the size limit (:151-155,
//                                        default 2000), size / latest_time / latest_measurement / latest_offseted_measurement /
//                                        has, and the lookup of an exact stamp
//   TransformInterpolationBuffer         the same buffer with the lookup of ANY stamp it covers (:100-149: interpolation between the
//                                        two neighbouring poses) and getTransform (:189-220: clamp before, extrapolation after);
//                                        the arithmetic is the library's (include/trajectory/o3s_trajectory.h)
//   TrajectoryMotionCompensation         the de-skew of a staged sweep along such a buffer (o3s_raw_scan_undistort_trajectory)
//   ConstantVelocityMotionCompensation   MotionCompensation.cpp:32-127: velocities from the buffer (o3s_motion_from_poses),
//                                        the de-skew on the staged sweep (o3s_raw_scan_undistort)
//   LidarOdometry                        Odometry.cpp:22-134: two o3s_scan objects that are swapped, never copied; the registration
//                                        is o3s_scan_registration_icp between the two resident merge clouds
// No Eigen / Open3D headers are needed; only the C ABI.
#pragma once

#include <cmath>
#include <cstdint>
#include <deque>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "o3s_pose.hpp"
#include "o3s_registration.h"
#include "o3s_scan.h"
#include "trajectory/o3s_trajectory.h"

namespace o3s {

struct TimestampedPose {
  double time;
  Mat4 transform;
};

class TransformBuffer {
 public:
  explicit TransformBuffer(std::size_t sizeLimit = 2000) : limit_(sizeLimit) {}
  void push(double t, const Mat4& T) {
    if (!poses_.empty() && (t < poses_.front().time || t < poses_.back().time)) return;  // earlier than the earliest / out of order
    poses_.push_back(TimestampedPose{t, T});
    while (poses_.size() > limit_) poses_.pop_front();
  }
  std::size_t size() const { return poses_.size(); }
  bool empty() const { return poses_.empty(); }
  double earliest_time() const { return need().front().time; }
  double latest_time() const { return need().back().time; }
  const TimestampedPose& latest_measurement() const { return need().back(); }
  const TimestampedPose& latest_offseted_measurement(int offset) const {  // *std::prev(end, offset + 1)
    if (offset < 0 || (std::size_t)offset >= need().size()) throw std::runtime_error("TransformBuffer: offset beyond the buffer");
    return poses_[poses_.size() - 1 - (std::size_t)offset];
  }
  bool has(double t) const { return !poses_.empty() && poses_.front().time <= t && t <= poses_.back().time; }
  const Mat4& lookup(double t) const {  // the pose pushed with exactly this stamp (the first of equal stamps)
    for (const TimestampedPose& p : poses_)
      if (p.time == t) return p.transform;
    throw std::runtime_error("TransformBuffer: no pose at the requested stamp");
  }
  std::vector<o3s_stamped_pose> table() const {  // the buffer as the library's functions take it
    std::vector<o3s_stamped_pose> tab(poses_.size());
    for (std::size_t k = 0; k < poses_.size(); ++k) {
      tab[k].t = poses_[k].time;
      for (int i = 0; i < 16; ++i) tab[k].T[i] = poses_[k].transform.m[i];
    }
    return tab;
  }

 private:
  const std::deque<TimestampedPose>& need() const {
    if (poses_.empty()) throw std::runtime_error("TransformBuffer: empty buffer");
    return poses_;
  }
  std::deque<TimestampedPose> poses_;
  std::size_t limit_;
};

// getTransform over a table of stamped poses (o3s_trajectory_get_transform)
inline Mat4 getTransform(double t, const o3s_stamped_pose* table, std::size_t K) {
  Mat4 out{};
  if (K == 0) throw std::runtime_error("getTransform: empty buffer");
  const int rc = o3s_trajectory_get_transform(table, (std::int64_t)K, t, out.m);
  if (rc != O3S_OK) throw std::runtime_error("o3s_trajectory_get_transform failed (status " + std::to_string(rc) + ")");
  return out;
}
inline Mat4 getTransform(double t, const TransformBuffer& buffer) {
  const std::vector<o3s_stamped_pose> tab = buffer.table();
  return getTransform(t, tab.data(), tab.size());
}

// The buffer kept as one table in memory, so that every lookup and every de-skew reads it in place
class TransformInterpolationBuffer {
 public:
  explicit TransformInterpolationBuffer(std::size_t sizeLimit = 2000) : limit_(sizeLimit) {}
  void push(double t, const Mat4& T) {
    if (!empty() && (t < earliest_time() || t < latest_time())) return;  // earlier than the earliest / out of order
    o3s_stamped_pose p;
    p.t = t;
    for (int i = 0; i < 16; ++i) p.T[i] = T.m[i];
    poses_.push_back(p);
    while (size() > limit_) ++head_;
    if (head_ > limit_) {  // drop the retired front now and then, not on every push
      poses_.erase(poses_.begin(), poses_.begin() + (std::ptrdiff_t)head_);
      head_ = 0;
    }
  }
  std::size_t size() const { return poses_.size() - head_; }
  bool empty() const { return size() == 0; }
  const o3s_stamped_pose* table() const { return poses_.data() + head_; }
  double earliest_time() const { return need()[0].t; }
  double latest_time() const { return need()[size() - 1].t; }
  const o3s_stamped_pose& latest_measurement() const { return need()[size() - 1]; }
  const o3s_stamped_pose& latest_offseted_measurement(int offset) const {
    if (offset < 0 || (std::size_t)offset >= size()) throw std::runtime_error("TransformInterpolationBuffer: offset beyond the buffer");
    return need()[size() - 1 - (std::size_t)offset];
  }
  bool has(double t) const { return o3s_trajectory_has(table(), (std::int64_t)size(), t) != 0; }
  Mat4 lookup(double t) const {
    Mat4 out{};
    const int rc = o3s_trajectory_lookup(table(), (std::int64_t)size(), t, out.m);
    if (rc == O3S_ERR_BAD_ARGUMENT) throw std::runtime_error("TransformInterpolationBuffer: missing transform for the requested stamp");
    if (rc != O3S_OK) throw std::runtime_error("o3s_trajectory_lookup failed (status " + std::to_string(rc) + ")");
    return out;
  }

 private:
  const o3s_stamped_pose* need() const {
    if (empty()) throw std::runtime_error("TransformInterpolationBuffer: empty buffer");
    return table();
  }
  std::vector<o3s_stamped_pose> poses_;
  std::size_t head_ = 0, limit_;
};

inline Mat4 getTransform(double t, const TransformInterpolationBuffer& buffer) { return getTransform(t, buffer.table(), buffer.size()); }

// The de-skew of a staged sweep along the trajectory the buffer holds: every point is expressed in the sensor frame at the
// sweep's stamp.  Point times come from the driver (o3s_raw_scan_set_point_times on the staged sweep), else from the azimuth as
// in ConstantVelocityMotionCompensation.  With an empty buffer the sweep stays as it came.
class TrajectoryMotionCompensation {
 public:
  TrajectoryMotionCompensation(const TransformInterpolationBuffer& buffer, double scanDuration = 0.1, bool isSpinningClockwise = true)
      : buffer_(buffer), scanDuration_(scanDuration), clockwise_(isSpinningClockwise) {
    if (!(scanDuration > 0.0)) throw std::runtime_error("lidar scanDuration_ must be > 0");
  }
  void undistort(o3s_raw_scan* staged, double stamp, const Mat4& calibration) const {
    if (buffer_.empty()) return;
    o3s_trajectory_deskew p{};
    p.stamp = stamp;
    p.scan_duration = scanDuration_;
    for (int i = 0; i < 16; ++i) p.calibration[i] = calibration.m[i];
    p.is_spinning_clockwise = clockwise_ ? 1 : 0;
    const int rc = o3s_raw_scan_undistort_trajectory(staged, buffer_.table(), (std::int64_t)buffer_.size(), &p);
    if (rc != O3S_OK) throw std::runtime_error("o3s_raw_scan_undistort_trajectory failed (status " + std::to_string(rc) + ")");
  }

 private:
  const TransformInterpolationBuffer& buffer_;
  double scanDuration_;
  bool clockwise_;
};

class ConstantVelocityMotionCompensation {
 public:
  ConstantVelocityMotionCompensation(const TransformBuffer& buffer, double scanDuration = 0.1, bool isSpinningClockwise = true,
                                     int numPosesVelocityEstimation = 3)
      : buffer_(buffer), scanDuration_(scanDuration), clockwise_(isSpinningClockwise), numPoses_(numPosesVelocityEstimation) {
    if (!(scanDuration > 0.0)) throw std::runtime_error("lidar scanDuration_ must be > 0");
  }
  // estimateLinearAndAngularVelocity: zero while the buffer holds no more than numPoses poses, or already has this stamp
  o3s_motion motion(double stamp) const {
    o3s_motion m{};
    m.scan_duration = scanDuration_;
    m.is_spinning_clockwise = clockwise_ ? 1 : 0;
    if (buffer_.size() <= (std::size_t)numPoses_ || !(buffer_.latest_time() < stamp)) return m;
    const TimestampedPose& finish = buffer_.latest_measurement();
    const TimestampedPose& start = buffer_.latest_offseted_measurement(numPoses_);
    if (o3s_motion_from_poses(start.transform.m, start.time, finish.transform.m, finish.time, &m) != O3S_OK)
      throw std::runtime_error("o3s_motion_from_poses failed");
    return m;
  }
  // undistortInputPointCloud on the staged sweep, in place; returns the motion used
  o3s_motion undistort(o3s_raw_scan* staged, double stamp) const {
    const o3s_motion m = motion(stamp);
    const int rc = o3s_raw_scan_undistort(staged, &m);
    if (rc != O3S_OK) throw std::runtime_error("o3s_raw_scan_undistort failed (status " + std::to_string(rc) + ")");
    return m;
  }

 private:
  const TransformBuffer& buffer_;
  double scanDuration_;
  bool clockwise_;
  int numPoses_;
};

// OdometryParameters with the values of param/tutorial_1_LO.lua over the defaults
struct OdometryParams {
  double voxelSize = 0.05;                 // odometry.scan_processing.voxel_size
  double downSamplingRatio = 1.0;          // must be 1.0: RandomDownSample(1.0) keeps the set; the order is taken as the identity
  o3s_cropper cropper{3, 0, 2.0, 40.0, 0.0, {0.0, 0.0, 0.0}};  // MinMaxRadius 2 .. 40 m
  o3s_o3d_estimation_type registrationType = O3S_O3D_GENERALIZED;
  double maxCorrespondenceDistance = 1.0;  // scan_matching.icp.max_correspondence_dist
  int knn = 10;                            // scan_matching.icp.knn
  double maxDistanceKnn = 1.0;             // scan_matching.icp.max_distance_knn
  int maxNumIter = 30;                     // scan_matching.icp.max_n_iter
  std::size_t bufferSize = 2000;
};

class LidarOdometry {
 public:
  explicit LidarOdometry(const OdometryParams& p = OdometryParams(), int device = 0) : params_(p), buffer_(p.bufferSize) {
    if (p.downSamplingRatio != 1.0) throw std::invalid_argument("downSamplingRatio must be 1.0 (O3S_ERR_BAD_ARGUMENT)");
    check(o3s_scan_create(device, &prev_), "o3s_scan_create");
    check(o3s_scan_create(device, &next_), "o3s_scan_create");
    check(o3s_scan_set_normal_estimation(prev_, p.maxDistanceKnn, p.knn), "o3s_scan_set_normal_estimation");
    check(o3s_scan_set_normal_estimation(next_, p.maxDistanceKnn, p.knn), "o3s_scan_set_normal_estimation");
  }
  ~LidarOdometry() {
    o3s_scan_destroy(prev_);
    o3s_scan_destroy(next_);
  }
  LidarOdometry(const LidarOdometry&) = delete;
  LidarOdometry& operator=(const LidarOdometry&) = delete;

  // LidarOdometry::setInitialTransform (:118-134): a second call before the value was used is ignored
  void setInitialTransform(const Mat4& T) {
    if (isInitialTransformSet_) return;
    initialTransform_ = T;
    cumulative_ = T;
    isInitialTransformSet_ = true;
  }
  bool hasProcessedMeasurements() const { return !buffer_.empty(); }
  const TransformBuffer& getBuffer() const { return buffer_; }
  const Mat4& cumulative() const { return cumulative_; }
  const Mat4& getOdomToRangeSensor(double t) const { return buffer_.lookup(t); }
  const o3s_scan* getPreProcessedCloud() const { return prev_; }
  const o3s_o3d_icp_result& lastResult() const { return lastResult_; }

  // the sweep in the sensor frame on the host (normals nullable: estimated) ...
  bool addRangeScan(const double* pts, const double* normals, std::int64_t N, double timestamp) {
    return add(pts, normals, N, nullptr, timestamp);
  }
  // ... or staged (and de-skewed) in HBM
  bool addRangeScan(const o3s_raw_scan* staged, double timestamp) { return add(nullptr, nullptr, 0, staged, timestamp); }

 private:
  bool add(const double* pts, const double* normals, std::int64_t N, const o3s_raw_scan* staged, double timestamp) {
    if (o3s_scan_get(prev_, 0, nullptr, nullptr) == 0) {  // cloudPrev_.IsEmpty(): the first measurement (:31-37)
      preprocess(prev_, pts, normals, N, staged);
      buffer_.push(timestamp, cumulative_);
      lastMeasurementTimestamp_ = timestamp;
      return true;
    }
    if (timestamp < lastMeasurementTimestamp_) return false;  // measurements came out of order (:45-48)
    preprocess(next_, pts, normals, N, staged);
    const Mat4 identity = Mat4::identity();
    o3s_o3d_estimation est;
    o3s_o3d_default_estimation(&est);
    est.type = params_.registrationType;
    o3s_o3d_icp_criteria cr;
    o3s_o3d_icp_default_criteria(&cr);
    cr.max_iteration = params_.maxNumIter;
    o3s_o3d_icp_result res{};
    const int rc = o3s_scan_registration_icp(prev_, 0, next_, 0, params_.maxCorrespondenceDistance, identity.m, &est, &cr, &res);
    if (rc == O3S_ERR_EMPTY_REFERENCE) {  // an empty target: the default result (identity, fitness 0)
      res = o3s_o3d_icp_result{};
      for (int k = 0; k < 16; ++k) res.transformation[k] = identity.m[k];
    } else {
      check(rc, "o3s_scan_registration_icp");
    }
    lastResult_ = res;
    const double* T = res.transformation;
    if (std::sqrt(T[12] * T[12] + T[13] * T[13] + T[14] * T[14]) > 0.8) return false;  // "jumped more than 80cm" (:58-63): cloudPrev_ stays
    if (!(res.fitness > 0.1)) {                                                          // "Odometry failed" (:66-82)
      if (o3s_scan_get(next_, 0, nullptr, nullptr) != 0) std::swap(prev_, next_);
      return false;
    }
    if (isInitialTransformSet_) {  // :83-88
      cumulative_ = initialTransform_;
      isInitialTransformSet_ = false;
    } else {
      Mat4 R;
      for (int k = 0; k < 16; ++k) R.m[k] = T[k];
      cumulative_ = mul(cumulative_, inverse_isometry(R));
    }
    std::swap(prev_, next_);  // cloudPrev_ = std::move(*preProcessed): handles, not clouds
    buffer_.push(timestamp, cumulative_);
    lastMeasurementTimestamp_ = timestamp;
    return true;
  }
  // LidarOdometry::preprocess (:22-27): the merge cloud of o3s_scan_preprocess with the odometry's cropper in both places
  void preprocess(o3s_scan* s, const double* pts, const double* normals, std::int64_t N, const o3s_raw_scan* staged) {
    if (staged)
      check(o3s_scan_preprocess_staged(s, &params_.cropper, params_.voxelSize, &params_.cropper, staged, nullptr, nullptr), "o3s_scan_preprocess_staged");
    else
      check(o3s_scan_preprocess(s, &params_.cropper, params_.voxelSize, &params_.cropper, pts, normals, N, nullptr, nullptr), "o3s_scan_preprocess");
  }
  static void check(int rc, const char* what) {
    if (rc != O3S_OK) throw std::runtime_error(std::string(what) + " failed (status " + std::to_string(rc) + ")");
  }

  OdometryParams params_;
  TransformBuffer buffer_;
  o3s_scan* prev_ = nullptr;
  o3s_scan* next_ = nullptr;
  Mat4 cumulative_ = Mat4::identity(), initialTransform_ = Mat4::identity();
  bool isInitialTransformSet_ = false;
  double lastMeasurementTimestamp_ = 0.0;
  o3s_o3d_icp_result lastResult_{};
};

}  // namespace o3s
