// o3s_icp.hpp — header-only C++17 shim over the C ABI (include/o3s_icp.h) for host code that stays C++/catkin.
//
// It gives open3d_slam the same two calls it makes on its public `PM::ICP icp_` member
// (open3d_slam/include/open3d_slam/Mapper.hpp:70-72):
//     icp_.initReference(referenceDataPoints)                     Mapper.cpp:363
//     icp_.compute(reading, {}, T_init, false)                    Mapper.cpp:393
// and rethrows the library's status codes as the exceptions libpointmatcher would have thrown, so the Mapper's existing
// `catch (const std::runtime_error&)` (Mapper.cpp:420-422) keeps working unchanged.
// No Eigen / libpointmatcher headers are needed: matrices are passed as raw column-major float pointers, which is what
// `PM::Matrix::data()` returns.  See INTEGRATION.md for the exact patch.
#pragma once

#include <array>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "o3s_icp.h"
#include "o3s_dense_map.h"
#include "dense_map/o3s_dense_map_color.h"
#include "o3s_submap.h"
#include "degeneracy/o3s_degeneracy.h"
#include "degeneracy/o3s_degeneracy_partial.h"
#include "localizability/o3s_localizability.h"
#include "outlier_removal/o3s_outlier_removal.h"
#include "clustering/o3s_clustering.h"
#include "plane_segmentation/o3s_plane_segmentation.h"
#include "keypoints/o3s_keypoints.h"

namespace o3s {

// PointMatcher<T>::ConvergenceError derives from std::runtime_error (PointMatcher.h:142-147); so does TransformationError.
struct ConvergenceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct TransformationError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

class IcpHip {
 public:
  // cfg mirrors param/icp.yaml; o3s_icp_default_config gives the shipped values
  explicit IcpHip(int device = 0) {
    o3s_icp_config cfg;
    o3s_icp_default_config(&cfg);
    create(cfg, device);
  }
  IcpHip(const o3s_icp_config& cfg, int device) { create(cfg, device); }
  ~IcpHip() { o3s_icp_destroy(h_); }
  IcpHip(const IcpHip&) = delete;
  IcpHip& operator=(const IcpHip&) = delete;

  // ICP::initReference(referenceIn): features = referenceIn.features.data() (4 x M), normals =
  // referenceIn.getDescriptorViewByName("normals").data() (3 x M).  Returns false for an empty cloud (ICP.cpp:295-298).
  bool initReference(const float* features4xM, const float* normals3xM, std::int64_t M) {
    const int rc = o3s_icp_init_reference(h_, features4xM, normals3xM, M);
    if (rc == O3S_ERR_EMPTY_REFERENCE) return false;
    raise(rc);
    return true;
  }

  // ICP::compute(readingIn, {}, T_refIn_readIn, false): T_init / T_out are 4x4 column-major (PM::TransformationParameters::data()).
  void compute(const float* features4xN, const float* normals3xN, std::int64_t N, const float* T_init, float* T_out) {
    raise(o3s_icp_compute(h_, features4xN, normals3xN, N, T_init, T_out, &stats_));
  }

  bool getMaxNumIterationsReached() const { return stats_.max_iters_reached != 0; }  // PointMatcher.h:786
  const o3s_icp_stats& stats() const { return stats_; }
  // icp.errorMinimizer->getCovariance() (PointToPlaneWithCov.cpp:164-168): 6 x 6 column-major, parameters [t_x t_y t_z alpha beta gamma],
  // of the last successful compute on this handle; all zeros under the plain minimiser (ErrorMinimizer.cpp:266-270).  Throws
  // std::runtime_error before any compute or after a failed one.  Eigen::Map<const Eigen::Matrix<double, 6, 6>>(c.data()) reads it.
  std::array<double, 36> getCovariance() const {
    std::array<double, 36> c{};
    const int rc = o3s_icp_get_covariance(h_, c.data());
    if (rc != O3S_OK) throw std::runtime_error("o3s_icp_get_covariance: no successful compute on this handle (status " + std::to_string(rc) + ")");
    return c;
  }
  // Open3D's RegistrationResult (fitness_, inlier_rmse_) of the resident reading over the chain's own matcher
  // (o3s_icp_evaluate_resident): T == nullptr evaluates where the last successful compute left the reading, a 4x4 column-major T what
  // iteration 0 of a compute from it matches; maxCorrespondenceDistance 0 = the chain's maxDist.  What the health gate of
  // Mapper.cpp:424-431 reads as result.fitness_.
  o3s_icp_fitness evaluate(const float* T = nullptr, float maxCorrespondenceDistance = 0.f) {
    o3s_icp_fitness f{};
    raise(o3s_icp_evaluate_resident(h_, T, maxCorrespondenceDistance, &f));
    return f;
  }
  // Which directions of the pose the kept pairs of the last successful compute constrained (o3s_icp_localizability: four launches
  // behind the chain, one round trip).  params: the three sums have no default (o3s_localizability_default_params leaves them NaN).
  // Call it before evaluate(): the fitness replaces the match streams the analysis reads.
  o3s_localizability localizability(const o3s_localizability_params& params) {
    o3s_localizability out{};
    raise(o3s_icp_localizability(h_, &params, &out));
    return out;
  }
  // How the later computes treat directions the scan does not constrain (o3s_icp_set_degeneracy): O3S_DEGENERACY_OFF, _FIXED with
  // `fixedSet` (the same set in every iteration) or _ANALYSE with `params` (every iteration analyses its own kept pairs and
  // constrains the directions of category < minCategory).  One launch more per iteration (FIXED) or four (ANALYSE); none when OFF.
  void setDegeneracy(std::int32_t mode, const o3s_degeneracy_set* fixedSet = nullptr, const o3s_localizability_params* params = nullptr,
                     std::int32_t minCategory = 2) {
    raise(o3s_icp_set_degeneracy(h_, mode, fixedSet, params, minCategory));
  }
  // One 6-bit mask per iteration of the last successful compute: the directions that iteration constrained (o3s_icp_degeneracy_trace)
  std::vector<std::int32_t> degeneracyTrace() {
    std::vector<std::int32_t> masks(4096);
    masks.resize((size_t)o3s_icp_degeneracy_trace(h_, masks.data(), (std::int32_t)masks.size()));
    return masks;
  }
  // With the flag set, the ANALYSE chain constrains a partially localizable direction (category 1) to the step its strong pairs
  // alone ask for, instead of to zero or not at all (o3s_icp_set_degeneracy_partial).  No launch more; FIXED and OFF ignore it.
  void setDegeneracyPartial(bool enable) { raise(o3s_icp_set_degeneracy_partial(h_, enable ? 1 : 0)); }
  // One record per iteration of the last successful compute: the directions of category 1 and the six values the rows carried
  // (o3s_icp_degeneracy_partial_trace); empty when the flag is off
  struct DegeneracyPartialTrace {
    std::vector<std::int32_t> partialMasks;
    std::vector<double> values;  // [n][6]
  };
  DegeneracyPartialTrace degeneracyPartialTrace() {
    DegeneracyPartialTrace t;
    t.partialMasks.resize(4096);
    t.values.resize(4096 * 6);
    const size_t n = (size_t)o3s_icp_degeneracy_partial_trace(h_, t.partialMasks.data(), t.values.data(), (std::int32_t)t.partialMasks.size());
    t.partialMasks.resize(n);
    t.values.resize(n * 6);
    return t;
  }
  o3s_icp* handle() { return h_; }

 private:
  void create(const o3s_icp_config& cfg, int device) {
    const int rc = o3s_icp_create(&cfg, device, &h_);
    if (rc != O3S_OK) throw std::runtime_error(std::string("o3s_icp_create: ") + o3s_last_error(nullptr));
  }
  void raise(int rc) const {
    if (rc == O3S_OK) return;
    const std::string msg = o3s_last_error(h_);
    switch (rc) {
      case O3S_ERR_NO_MATCHES:
      case O3S_ERR_NO_POINTS:
      case O3S_ERR_NAN: throw ConvergenceError(msg);
      case O3S_ERR_NOT_RIGID: throw TransformationError(msg);
      default: throw std::runtime_error(msg);
    }
  }
  o3s_icp* h_ = nullptr;
  o3s_icp_stats stats_{};
};

// Device-resident map cloud of the active submap (include/o3s_submap.h).  Mirrors the two places the reference walks
// the whole map on the host for every scan:
//     Submap::insertScan(raw, preProcessed, mapToRangeSensor, time, carve)        Submap.cpp:39-96
//     ScanToMapIcp::cropSubmap + open3dToPointmatcher + icp_.initReference        Mapper.cpp:328-366
// points / normals: std::vector<Eigen::Vector3d>::data() cast to double*; poses: Eigen::Matrix4d::data().
class SubmapHip {
 public:
  SubmapHip(double mapVoxelSize, const o3s_cropper& mapBuilderCropper, int device = 0) {
    const int rc = o3s_submap_create(device, mapVoxelSize, &mapBuilderCropper, &m_);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_create failed (status " + std::to_string(rc) + ")");
  }
  ~SubmapHip() { o3s_submap_destroy(m_); }
  SubmapHip(const SubmapHip&) = delete;
  SubmapHip& operator=(const SubmapHip&) = delete;

  bool insertScan(const double* points3xN, const double* normals3xN, std::int64_t N, const double* mapToRangeSensor4x4) {
    const int rc = o3s_submap_insert_scan(m_, points3xN, normals3xN, N, mapToRangeSensor4x4);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_insert_scan failed (status " + std::to_string(rc) + ")");
    return true;
  }
  // Submap::carve (Submap.cpp:116-130) on the raw scan; call before insertScan on the scans the cadence selects
  std::int64_t carve(const o3s_carving_params& p, const double* rawPoints3xN, std::int64_t N, const double* mapToRangeSensor4x4) {
    std::int64_t removed = 0;
    if (o3s_submap_carve(m_, &p, rawPoints3xN, N, mapToRangeSensor4x4, &removed) != O3S_OK) throw std::runtime_error("o3s_submap_carve failed");
    return removed;
  }
  // Open3D's outlier filters on the sparse map, in place (outlier_removal/o3s_outlier_removal.h); returns the number of removed
  // points.  stats4 (nullable, statistical): mean, std, thr, valid
  std::int64_t removeOutliers(const o3s_outlier_params& p, double* stats4 = nullptr) {
    std::int64_t removed = 0;
    const int rc = o3s_submap_remove_outliers(m_, &p, &removed, stats4);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_remove_outliers failed (status " + std::to_string(rc) + ")");
    return removed;
  }
  std::int64_t removeRadiusOutliers(std::int32_t nbPoints, double searchRadius) { return removeOutliers(o3s_outlier_params{1, nbPoints, searchRadius}); }
  std::int64_t removeStatisticalOutliers(std::int32_t nbNeighbors, double stdRatio, double* stats4 = nullptr) {
    return removeOutliers(o3s_outlier_params{2, nbNeighbors, stdRatio}, stats4);
  }
  // Open3D's ClusterDBSCAN(eps, minPoints) of the sparse map (clustering/o3s_clustering.h): one label per map point, -1 = noise;
  // returns the number of clusters.  Nothing in the map changes
  std::int32_t clusterDBSCAN(double eps, std::int32_t minPoints, std::vector<std::int32_t>& labels) {
    const o3s_dbscan_params p{eps, minPoints, 0};
    labels.assign(static_cast<std::size_t>(o3s_submap_size(m_)), -1);
    std::int32_t n = 0;
    const int rc = o3s_submap_cluster_dbscan(m_, &p, labels.data(), &n);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_cluster_dbscan failed (status " + std::to_string(rc) + ")");
    return n;
  }
  // ... and the removal of every point without a cluster or in a cluster below p.min_cluster_size points, in place; returns the
  // number of removed points.  nClusters nullable
  std::int64_t removeSmallClusters(const o3s_dbscan_params& p, std::int32_t* nClusters = nullptr) {
    std::int64_t removed = 0;
    const int rc = o3s_submap_remove_small_clusters(m_, &p, &removed, nClusters);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_remove_small_clusters failed (status " + std::to_string(rc) + ")");
    return removed;
  }
  // ISS keypoints of the resident SPARSE cloud (keypoints/o3s_keypoints.h; o3s_submap_compute_features must have run), then the
  // feature set — sparse points, normals, FPFH columns — reduced to them, in order: correspondences, RANSAC and place recognition
  // then search the keypoints alone.  indices (nullable): which sparse points stayed; radii2 (nullable): the radii used.  Returns
  // the number of keypoints (the feature set's size when p.min_neighbors is 0: nothing happens then)
  std::int64_t selectKeypoints(const o3s_iss_params& p, std::vector<std::int64_t>* indices = nullptr, double* radii2 = nullptr) {
    const std::int64_t before = o3s_submap_features_size(m_);
    std::int64_t n = before > 0 ? before : 0;
    std::vector<std::int64_t> idx(static_cast<std::size_t>(n));
    for (std::size_t k = 0; k < idx.size(); ++k) idx[k] = static_cast<std::int64_t>(k);
    const int rc = o3s_submap_select_keypoints(m_, &p, idx.data(), &n, radii2);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_select_keypoints failed (status " + std::to_string(rc) + ")");
    idx.resize(static_cast<std::size_t>(n));
    if (indices) *indices = idx;
    return n;
  }
  // ... labels only: one flag (1 = keypoint) and one saliency per sparse point; nothing in the submap changes.  saliency, radii2
  // nullable; returns the number of keypoints
  std::int64_t featureKeypoints(const o3s_iss_params& p, std::vector<std::int32_t>& flags, std::vector<double>* saliency = nullptr, double* radii2 = nullptr) {
    const std::int64_t nf = o3s_submap_features_size(m_);
    flags.assign(static_cast<std::size_t>(nf > 0 ? nf : 0), 0);
    std::vector<double> sal(flags.size(), 0.0);
    std::int64_t n = 0;
    const int rc = o3s_submap_feature_keypoints(m_, &p, flags.data(), sal.data(), &n, radii2);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_feature_keypoints failed (status " + std::to_string(rc) + ")");
    if (saliency) *saliency = sal;
    return n;
  }
  // RANSAC plane segmentation of the sparse map where it lies (plane_segmentation/o3s_plane_segmentation.h): one label per map
  // point, -1 = no plane; models gets 4 doubles per reported plane, counts (nullable) its inliers; returns the number of planes.
  // Nothing in the map changes
  std::int32_t segmentPlanes(const o3s_plane_params& p, std::vector<std::int32_t>& labels, std::vector<double>& models,
                             std::vector<std::int64_t>* counts = nullptr) {
    labels.assign(static_cast<std::size_t>(o3s_submap_size(m_)), -1);
    models.assign(16 * 4, 0.0);
    std::vector<std::int64_t> c(16, 0);
    std::int32_t n = 0;
    const int rc = o3s_submap_segment_planes(m_, &p, labels.data(), &n, models.data(), c.data());
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_segment_planes failed (status " + std::to_string(rc) + ")");
    models.resize(static_cast<std::size_t>(n) * 4);
    c.resize(static_cast<std::size_t>(n));
    if (counts) *counts = c;
    return n;
  }
  // ... and every point a reported plane took removed, in place; returns the number of removed points.  models nullable
  std::int64_t removePlanes(const o3s_plane_params& p, std::vector<double>* models = nullptr) {
    std::int64_t removed = 0;
    std::int32_t n = 0;
    double m[16 * 4] = {0.0};
    const int rc = o3s_submap_remove_planes(m_, &p, &removed, &n, m);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_remove_planes failed (status " + std::to_string(rc) + ")");
    if (models) models->assign(m, m + static_cast<std::size_t>(n) * 4);
    return removed;
  }
  std::int64_t size() const { return o3s_submap_size(m_); }
  // the two questions the per-scan loop asks about the size, answered without waiting for an insert whose completion is pending
  // (o3s_submap_size_bounds) whenever the bounds decide them
  bool empty() const {
    std::int64_t lo = 0, hi = 0;
    if (o3s_submap_size_bounds(m_, &lo, &hi) != O3S_OK) throw std::runtime_error("o3s_submap_size_bounds failed");
    return hi == 0 || (lo == 0 && size() == 0);
  }
  bool largerThan(std::int64_t n) const {
    std::int64_t lo = 0, hi = 0;
    if (o3s_submap_size_bounds(m_, &lo, &hi) != O3S_OK) throw std::runtime_error("o3s_submap_size_bounds failed");
    if (hi <= n) return false;
    if (lo > n) return true;
    return size() > n;
  }
  // a copy of the map on `device` (o3s_submap_clone): the snapshot a loop-closure worker refines while this submap is inserted into
  o3s_submap* cloneHandle(int device) const {
    o3s_submap* c = nullptr;
    if (o3s_submap_clone(m_, device, &c) != O3S_OK) throw std::runtime_error("o3s_submap_clone failed");
    return c;
  }
  // room for nPoints up front (SubmapParameters::maxNumPoints_ + one scan): no re-allocation stalls while the map grows
  void reserve(std::int64_t nPoints) {
    if (o3s_submap_reserve(m_, nPoints) != O3S_OK) throw std::runtime_error("o3s_submap_reserve failed");
  }
  // this submap is closed, `fresh` (empty) takes over: the map stays here in arrays of its own size, every other device buffer
  // moves to `fresh` (o3s_submap_hand_over: no hipFree / hipMalloc of the large arrays)
  void handOverTo(SubmapHip& fresh) {
    if (o3s_submap_hand_over(m_, fresh.m_) != O3S_OK) throw std::runtime_error("o3s_submap_hand_over failed");
  }
  // a submap that is no longer inserted into gives everything but its map cloud back to the allocator (o3s_submap_trim)
  void trim() { (void)o3s_submap_trim(m_); }
  // false = "Map patch is empty" (Mapper.cpp:330-336) or an empty reference (ICP.cpp:295-298)
  bool setReference(const o3s_cropper& scanMatcherCropper, const double* mapToRangeSensor4x4, IcpHip& icp, std::int64_t* nPatch = nullptr) {
    const int rc = o3s_submap_set_reference(m_, &scanMatcherCropper, mapToRangeSensor4x4, icp.handle(), nPatch);
    if (rc == O3S_ERR_EMPTY_REFERENCE) return false;
    if (rc != O3S_OK) throw std::runtime_error(std::string("o3s_submap_set_reference: ") + o3s_last_error(icp.handle()));
    return true;
  }
  // size of the patch cropSubmap would return at this pose (Mapper.cpp:328): the reference looks at it on EVERY scan
  std::int64_t patchCount(const o3s_cropper& scanMatcherCropper, const double* mapToRangeSensor4x4) {
    std::int64_t n = 0;
    if (o3s_submap_patch_count(m_, &scanMatcherCropper, mapToRangeSensor4x4, &n) != O3S_OK) throw std::runtime_error("o3s_submap_patch_count failed");
    return n;
  }
  void download(double* points3xN, double* normals3xN) const {
    if (o3s_submap_download(m_, points3xN, normals3xN) != O3S_OK) throw std::runtime_error("o3s_submap_download failed");
  }
  // voxelMap_.clear(); voxelMap_.insertCloud(mapCloud_) (Submap.cpp:260-264) as an occupancy snapshot in HBM; returns its size
  std::int64_t buildVoxelMap(double voxelSize) {
    if (o3s_submap_build_voxel_map(m_, voxelSize) != O3S_OK) throw std::runtime_error("o3s_submap_build_voxel_map failed");
    return o3s_submap_voxel_map_size(m_);
  }
  std::int64_t voxelMapSize() const { return o3s_submap_voxel_map_size(m_); }  // -1: never built
  // the share of a resident scan's points (which: 0 merge cloud, 1 match cloud), moved by mapToRangeSensor, that fall into an
  // occupied voxel of the snapshot (SubmapCollection.cpp:396-402); NaN for an empty scan, 0 without a snapshot
  double overlapFitness(const o3s_scan* scan, int which, const double* mapToRangeSensor4x4, std::int64_t* nOverlapping = nullptr) const {
    std::int64_t n = 0;
    double f = 0.0;
    if (o3s_submap_overlap_fitness_scan(m_, scan, which, mapToRangeSensor4x4, &n, &f) != O3S_OK) throw std::runtime_error("o3s_submap_overlap_fitness_scan failed");
    if (nOverlapping) *nOverlapping = n;
    return f;
  }
  o3s_submap* handle() { return m_; }

 private:
  o3s_submap* m_ = nullptr;
};

// Device-resident stand-in for Submap::denseMap_ (o3d_slam::VoxelizedPointCloud) and the calls Submap makes on it:
//     Submap::insertScanDenseMap(rawScan, mapToRangeSensor, time, isPerformCarving)   Submap.cpp:97-113
//     Submap::carve(scan, sensorPosition, param, &denseMap_)                          Submap.cpp:146-157
//     VoxelizedPointCloud::insert / toPointCloud / transform                          Voxel.cpp:49-114
class DenseMapHip {
 public:
  explicit DenseMapHip(double denseMapVoxelSize, int device = 0) {
    const int rc = o3s_dense_map_create(device, denseMapVoxelSize, &m_);
    if (rc != O3S_OK) throw std::runtime_error("o3s_dense_map_create failed (status " + std::to_string(rc) + ")");
  }
  ~DenseMapHip() { o3s_dense_map_destroy(m_); }
  DenseMapHip(const DenseMapHip&) = delete;
  DenseMapHip& operator=(const DenseMapHip&) = delete;

  void insert(const double* points3xN, const double* normals3xN, std::int64_t N) {
    check(o3s_dense_map_insert(m_, points3xN, normals3xN, N), "o3s_dense_map_insert");
  }
  // carving == nullptr <=> isPerformCarving == false; returns the number of voxels carved away
  std::int64_t insertScanDenseMap(const o3s_cropper& denseMapCropper, const double* rawPoints3xN, const double* rawNormals3xN, std::int64_t N,
                                  const double* mapToRangeSensor4x4, const o3s_dense_carving_params* carving = nullptr) {
    std::int64_t removed = 0;
    check(o3s_dense_map_insert_scan(m_, &denseMapCropper, rawPoints3xN, rawNormals3xN, N, mapToRangeSensor4x4, carving, &removed),
          "o3s_dense_map_insert_scan");
    return removed;
  }
  // The coloured forms (include/dense_map/o3s_dense_map_color.h).  colors3xN == nullptr: the calls above.  rgbMin3 / rgbMax3 are the
  // bounds of the reference's colorCropper_ (nullptr: its defaults 0 / 1)
  void insert(const double* points3xN, const double* normals3xN, const double* colors3xN, std::int64_t N) {
    check(o3s_dense_map_insert_colored(m_, points3xN, normals3xN, colors3xN, N), "o3s_dense_map_insert_colored");
  }
  std::int64_t insertScanDenseMap(const o3s_cropper& denseMapCropper, const double* rawPoints3xN, const double* rawNormals3xN,
                                  const double* rawColors3xN, std::int64_t N, const double* mapToRangeSensor4x4,
                                  const o3s_dense_carving_params* carving = nullptr, const double* rgbMin3 = nullptr,
                                  const double* rgbMax3 = nullptr) {
    std::int64_t removed = 0;
    check(o3s_dense_map_insert_scan_colored(m_, &denseMapCropper, rgbMin3, rgbMax3, rawPoints3xN, rawNormals3xN, rawColors3xN, N,
                                            mapToRangeSensor4x4, carving, &removed),
          "o3s_dense_map_insert_scan_colored");
    return removed;
  }
  // points and normals from the scan o3s_scan_preprocess left in HBM; one colour per raw point of it, from the host
  std::int64_t insertResidentScanDenseMap(const o3s_cropper& denseMapCropper, const o3s_scan* scan, const double* rawColors3xN,
                                          std::int64_t nColors, const double* mapToRangeSensor4x4,
                                          const o3s_dense_carving_params* carving = nullptr, const double* rgbMin3 = nullptr,
                                          const double* rgbMax3 = nullptr) {
    std::int64_t removed = 0;
    check(o3s_dense_map_insert_resident_scan_colored(m_, &denseMapCropper, rgbMin3, rgbMax3, scan, rawColors3xN, nColors, mapToRangeSensor4x4,
                                                     carving, &removed),
          "o3s_dense_map_insert_resident_scan_colored");
    return removed;
  }
  std::int64_t carve(const o3s_dense_carving_params& p, const double* scanPoints3xN, std::int64_t N, const double* sensorPosition3) {
    std::int64_t removed = 0;
    check(o3s_dense_map_carve(m_, &p, scanPoints3xN, N, sensorPosition3, &removed), "o3s_dense_map_carve");
    return removed;
  }
  void transform(const double* T4x4) { check(o3s_dense_map_transform(m_, T4x4), "o3s_dense_map_transform"); }
  std::int64_t size() const { return o3s_dense_map_size(m_); }
  bool empty() const { return size() == 0; }
  bool hasNormals() const { return o3s_dense_map_has_normals(m_) != 0; }
  bool hasColors() const { return o3s_dense_map_has_colors(m_) != 0; }
  // buffers sized by size(); returns the number of voxels written
  std::int64_t toPointCloud(double* points3xV, double* normals3xV) const {
    std::int64_t n = 0;
    check(o3s_dense_map_to_point_cloud(m_, points3xV, normals3xV, nullptr, nullptr, &n), "o3s_dense_map_to_point_cloud");
    return n;
  }
  // colors3xV: only while hasColors() (sum / count of every voxel; the sum starts at (1, 1, 1), see the header)
  std::int64_t toPointCloud(double* points3xV, double* normals3xV, double* colors3xV) const {
    std::int64_t n = 0;
    check(o3s_dense_map_to_point_cloud_colored(m_, points3xV, normals3xV, colors3xV, nullptr, nullptr, &n), "o3s_dense_map_to_point_cloud_colored");
    return n;
  }
  o3s_dense_map* handle() { return m_; }

 private:
  static void check(int rc, const char* what) {
    if (rc != O3S_OK) throw std::runtime_error(std::string(what) + " failed (status " + std::to_string(rc) + ")");
  }
  o3s_dense_map* m_ = nullptr;
};

// RANSAC plane segmentation of host arrays (plane_segmentation/o3s_plane_segmentation.h).  points3xN: std::vector<Eigen::Vector3d>::data()
// cast to double*.  Open3D's SegmentPlane returns (plane_model, inliers); bestIteration / estK / evaluated are what the search did.
struct PlaneSegmentation {
  std::array<double, 4> model{};
  std::vector<std::int64_t> inliers;
  std::int64_t bestIteration = -1, estK = 0, evaluated = 0;
};
inline PlaneSegmentation segmentPlane(const double* points3xN, std::int64_t N, const o3s_plane_params& p, int device = 0) {
  PlaneSegmentation r;
  r.inliers.resize(static_cast<std::size_t>(N > 0 ? N : 1));
  std::int64_t n = 0;
  const int rc = o3s_segment_plane(device, &p, points3xN, N, nullptr, 0, r.model.data(), r.inliers.data(), &n, &r.bestIteration, &r.estK, &r.evaluated);
  if (rc != O3S_OK) throw std::runtime_error("o3s_segment_plane failed (status " + std::to_string(rc) + ")");
  r.inliers.resize(static_cast<std::size_t>(n));
  return r;
}
// ... and the peel: one label per point (-1 = no plane), 4 doubles per reported plane, counts nullable; returns the number of planes
inline std::int32_t segmentPlanes(const double* points3xN, std::int64_t N, const o3s_plane_params& p, std::vector<std::int32_t>& labels,
                                  std::vector<double>& models, std::vector<std::int64_t>* counts = nullptr, int device = 0) {
  labels.assign(static_cast<std::size_t>(N > 0 ? N : 0), -1);
  models.assign(16 * 4, 0.0);
  std::vector<std::int64_t> c(16, 0);
  std::int32_t n = 0;
  const int rc = o3s_segment_planes(device, &p, points3xN, N, labels.data(), &n, models.data(), c.data());
  if (rc != O3S_OK) throw std::runtime_error("o3s_segment_planes failed (status " + std::to_string(rc) + ")");
  models.resize(static_cast<std::size_t>(n) * 4);
  c.resize(static_cast<std::size_t>(n));
  if (counts) *counts = c;
  return n;
}

// ISS keypoints of host arrays (keypoints/o3s_keypoints.h; Open3D's geometry::keypoint::ComputeISSKeypoints).  indices: the
// keypoints as ascending input indices; saliency: one value per INPUT point; radii: the salient and the non-max radius used.
struct IssKeypoints {
  std::vector<std::int64_t> indices;
  std::vector<double> points, saliency;  // 3 x indices.size(); N
  std::array<double, 2> radii{};
};
inline IssKeypoints computeIssKeypoints(const double* points3xN, std::int64_t N, const o3s_iss_params& p, int device = 0) {
  IssKeypoints r;
  const std::size_t n0 = static_cast<std::size_t>(N > 0 ? N : 0);
  r.indices.resize(n0);
  r.points.resize(3 * n0);
  r.saliency.assign(n0, 0.0);
  std::int64_t n = 0;
  const int rc = o3s_iss_keypoints(device, &p, points3xN, nullptr, N, r.points.data(), nullptr, r.indices.data(), &n, r.saliency.data(), r.radii.data());
  if (rc != O3S_OK) throw std::runtime_error("o3s_iss_keypoints failed (status " + std::to_string(rc) + ")");
  r.indices.resize(static_cast<std::size_t>(n));
  r.points.resize(3 * static_cast<std::size_t>(n));
  return r;
}

}  // namespace o3s
