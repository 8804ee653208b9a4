// o3s_submap_collection.hpp — header-only C++17 restatement of the submap bookkeeping that sits between the Mapper and the
// map clouds: o3d_slam::SubmapCollection (open3d_slam/src/SubmapCollection.cpp), with every submap resident on the device
// (o3s_submap over the C ABI).  Line numbers below are SubmapCollection.cpp's.
//
//   :28-32     constructor: one empty submap, scan buffer of 5 (setParameters: numScansOverlap_, :255-256)
//   :86-92     insertBufferedScans: the buffered (pre-processed) scans go into the new active submap at their own poses
//   :94-148    updateActiveSubmap: forced creation; minNumRangeData_ gate; localisation mode never switches; closest submap by
//              centre; maxNumPoints_ forces a new submap at the NEXT scan; another submap within radius_: stay / switch when
//              adjacent and isSwitchingSubmapsConsistant (:392-407: the reference's body is commented out and returns true — here
//              it is the written body when SubmapParams::isCheckSwitchingConsistency is on, true otherwise) / create when the
//              active one is left behind; nobody within radius_: create
//   :150-162   createNewSubmap (id, parent, origin)
//   :164-174   findClosestSubmap (first minimum of the centre distances)
//   :193-247   insertScan: buffer the scan; on a switch the scan
//              still goes into the PREVIOUS submap, whose centre is then computed (Submap::computeSubmapCenter, Submap.cpp:
//              282-286), it is queued as finished, an adjacency edge is added, the buffer is replayed into the new one
//   computeFeatures(idx): Submap::computeFeatures (Submap.cpp:255-275) of a submap on the device (o3s_submap_compute_features),
//              and with it the occupancy snapshot voxelMap_ (:260-264) at 2.5 x mapVoxelSize (Submap.cpp:239-240, magic.hpp:16);
//              the caller keeps the reference's timer (minSecondsBetweenFeatureComputation_) and decides when to call it.
//   :257-289   computeFeatures(finishedSubmapIds): the features of every finished submap, each pushed to the loop-closure candidates,
//              and the odometry constraints (parent -> finished) of all of them in ONE device call into odometryConstraints_
//              (o3s_constraint_builders.hpp), one after the other on the caller; getOdometryConstraints, popLoopClosureCandidates
//   :324-375   transform: which increment goes to which submap (planSubmapTransforms, o3s_pose_graph.hpp), applied to all resident
//              submaps by ONE o3s_submaps_transform call; per submap mapToRangeSensor_ * T, T * submapCenter_, the dense map where the
//              driver keeps one (Submap.cpp:115-128); the overlap buffer is flushed
//   :75-81     updateAdjacencyMatrix: the submaps of a loop-closure constraint become adjacent
//   :69-73     getTotalNumPoints; assembleMap: the loop of Mapper::getAssembledMapPointCloud (Mapper.cpp:524-535) over the resident
//              submaps as ONE o3s_assembled_map_build call into an AssembledMapHip (the map of all submaps, optionally down-sampled)
// Place recognition of a finished submap against the collection — candidate selection, the one-to-many RANSAC, the consistency
//              gates, the batched refinement — is PlaceRecognitionHip (o3s_place_recognition.hpp); the RANSAC between two submaps
//              is o3s_submap_registration_ransac (o3s_submap.h) on their feature sets.
// The scans the buffer keeps are resident o3s_scan objects: the caller hands over the scan it has just pre-processed and
// gets another one to fill next (a ring of numScansOverlap_ + 1 handles, nothing is copied).
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <deque>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "assembled_map/o3s_assembled_map.h"
#include "o3s_constraint_builders.hpp"
#include "o3s_icp.hpp"
#include "o3s_pose_graph.hpp"
#include "o3s_scan.h"

namespace o3s {

struct SubmapParams {            // o3d_slam::SubmapParameters (Parameters.hpp:103-109)
  double radius = 20.0;
  int minNumRangeData = 5;
  std::int64_t maxNumPoints = 400000;
  int numScansOverlap = 3;
  // adjacency_based_revisiting_min_fitness (Parameters.hpp:108; 0.5 in the shipped lua files): what the share of scan points inside
  // occupied voxels of the candidate submap must exceed before the active submap switches back to it
  double adjacencyBasedRevisitingMinFitness = 0.4;
  // off = the reference as it runs (isSwitchingSubmapsConsistant returns true); on = the body written at SubmapCollection.cpp:396-404
  bool isCheckSwitchingConsistency = false;
};

// o3d_slam::AdjacencyMatrix (AdjacencyMatrix.cpp:16-71): the edges updateActiveSubmap asks about, and the loop-closure flags
// getLoopClosureCandidatesIdxs asks about (o3s_place_recognition.hpp)
class AdjacencyHip {
 public:
  void addEdge(std::size_t a, std::size_t b) {  // :16-21: BOTH ends lose their loop-closure flag
    adj_[a].insert(b);
    adj_[b].insert(a);
    isLoopClosureSubmap_[a] = false;
    isLoopClosureSubmap_[b] = false;
  }
  bool isAdjacent(std::size_t a, std::size_t b) const {
    if (a == b) return true;
    const auto it = adj_.find(a);
    return it != adj_.end() && it->second.count(b) != 0;
  }
  void markAsLoopClosureSubmap(std::size_t id) { isLoopClosureSubmap_.at(id) = true; }  // :57-59 (std::out_of_range for an id no edge names)
  // :23-55 as written: INT_MAX while no edge has been added; else a breadth-first walk from `id` that stops at the first flagged
  // submap it takes from the queue — or, when none is reachable, at the LAST submap it visits — and returns max(0, hops - 1)
  int getDistanceToNearestLoopClosureSubmap(std::size_t id) const {
    if (isLoopClosureSubmap_.empty()) return std::numeric_limits<int>::max();
    std::deque<std::size_t> toProcess;
    std::set<std::size_t> visited;
    std::map<std::size_t, std::size_t> parents;
    std::size_t v = id;
    visited.insert(id);
    toProcess.push_back(id);
    while (!toProcess.empty()) {
      v = toProcess.front();
      toProcess.pop_front();
      if (isLoopClosureSubmap_.at(v)) break;
      for (const std::size_t adj : adj_.at(v))
        if (visited.insert(adj).second) {
          toProcess.push_back(adj);
          parents.insert({adj, v});
        }
    }
    int distance = 0;
    while (v != id) {
      v = parents.at(v);
      ++distance;
    }
    return std::max(0, distance - 1);
  }
  const std::map<std::size_t, std::set<std::size_t>>& edges() const { return adj_; }

 private:
  std::map<std::size_t, std::set<std::size_t>> adj_;
  std::map<std::size_t, bool> isLoopClosureSubmap_;
};

// The map of all submaps, resident on the device (assembled_map/o3s_assembled_map.h): the result of
// SubmapCollectionHip::assembleMap / MapperHip::getAssembledMapPointCloud.  Keep ONE object for the life of the mapper: its arrays
// only grow, so the periodic caller (SlamWrapperRos::publishMaps, every 250 ms) neither frees nor allocates in steady state.
class AssembledMapHip {
 public:
  explicit AssembledMapHip(int device = 0) {
    const int rc = o3s_assembled_map_create(device, &a_);
    if (rc != O3S_OK) throw std::runtime_error("o3s_assembled_map_create failed (status " + std::to_string(rc) + ")");
  }
  ~AssembledMapHip() { o3s_assembled_map_destroy(a_); }
  AssembledMapHip(const AssembledMapHip&) = delete;
  AssembledMapHip& operator=(const AssembledMapHip&) = delete;

  std::int64_t size() const { return o3s_assembled_map_size(a_); }
  bool hasNormals() const { return o3s_assembled_map_has_normals(a_) != 0; }
  bool hasColors() const { return o3s_assembled_map_has_colors(a_) != 0; }
  // 3 x size() doubles each (std::vector<Eigen::Vector3d>::data()); normals / colors nullable, refused when the map carries none
  void download(double* points3xN, double* normals3xN = nullptr, double* colors3xN = nullptr) const {
    const int rc = o3s_assembled_map_download(a_, points3xN, normals3xN, colors3xN);
    if (rc == O3S_ERR_BAD_SHAPE) throw std::invalid_argument("AssembledMapHip::download: the map carries no such attribute");
    if (rc != O3S_OK) throw std::runtime_error("o3s_assembled_map_download failed (status " + std::to_string(rc) + ")");
  }
  // the assembled map becomes dst's map cloud without leaving HBM (an ICP reference over the whole map, features of the whole map)
  void toSubmap(SubmapHip& dst) const {
    if (o3s_assembled_map_to_submap(a_, dst.handle()) != O3S_OK) throw std::runtime_error("o3s_assembled_map_to_submap failed");
  }
  std::int64_t deviceBytes() const { return o3s_assembled_map_device_bytes(a_); }
  o3s_assembled_map* handle() { return a_; }

 private:
  o3s_assembled_map* a_ = nullptr;
};

class SubmapCollectionHip {
 public:
  struct Entry {
    std::unique_ptr<SubmapHip> map;
    std::size_t id = 0, parentId = 0;
    double origin[3] = {0, 0, 0};   // mapToSubmap_.translation()
    double center[3] = {0, 0, 0};   // submapCenter_ once computed
    bool isCenterComputed = false;
    Mat4 mapToRangeSensor = Mat4::identity();  // Submap::mapToRangeSensor_: the pose of the last scan that went in (Submap.cpp:45)
    const double* mapToSubmapCenter() const { return isCenterComputed ? center : origin; }  // Submap.cpp:203-205
  };

  SubmapCollectionHip(const SubmapParams& sp, double mapVoxelSize, const o3s_cropper& mapBuilderCropper, bool isUseInitialMap, int device = 0)
      : params_(sp), voxel_(mapVoxelSize), cropper_(mapBuilderCropper), isUseInitialMap_(isUseInitialMap), device_(device) {
    if (sp.numScansOverlap <= 0) throw std::invalid_argument("Num scan overlap has to be > 0");  // :255
    const double eye[3] = {0, 0, 0};
    createNewSubmap(eye);  // :30, at the default-constructed (identity) pose
    for (int k = 0; k < sp.numScansOverlap + 1; ++k) {
      o3s_scan* sc = nullptr;
      if (o3s_scan_create(device, &sc) != O3S_OK) throw std::runtime_error("o3s_scan_create failed");
      free_.push_back(sc);
    }
  }
  ~SubmapCollectionHip() {
    for (auto& b : buffer_) o3s_scan_destroy(b.scan);
    for (o3s_scan* sc : free_) o3s_scan_destroy(sc);
  }
  SubmapCollectionHip(const SubmapCollectionHip&) = delete;
  SubmapCollectionHip& operator=(const SubmapCollectionHip&) = delete;

  // a scan object to pre-process the next scan into (handed back through insertScan)
  o3s_scan* scanForNextMeasurement() {
    if (free_.empty()) throw std::logic_error("the previous scan was not handed back");
    return free_.back();
  }
  // The same when the caller has pre-processed the next scan into an object of its OWN (another thread, the object's own
  // stream): `filled` takes the place of the ring's free object, which is handed out in exchange — nothing is copied, the ring
  // keeps its size, and the caller owns (and eventually destroys, or fills next) what it gets back.
  o3s_scan* exchangeScanForNextMeasurement(o3s_scan* filled) {
    if (free_.empty()) throw std::logic_error("the previous scan was not handed back");
    if (!filled) throw std::invalid_argument("exchangeScanForNextMeasurement: no scan");
    o3s_scan* spare = free_.back();
    free_.back() = filled;
    return spare;
  }
  // CloudRegistrationParameters::maxRadiusNormalEstimation_ / knnNormalEstimation_ for sweeps that arrive without normals: set on
  // every scan object of the ring (objects handed in through exchangeScanForNextMeasurement are the caller's to configure)
  void setScanNormalEstimation(double maxRadius, int knn) {
    for (auto& b : buffer_)
      if (o3s_scan_set_normal_estimation(b.scan, maxRadius, knn) != O3S_OK) throw std::invalid_argument("o3s_scan_set_normal_estimation");
    for (o3s_scan* sc : free_)
      if (o3s_scan_set_normal_estimation(sc, maxRadius, knn) != O3S_OK) throw std::invalid_argument("o3s_scan_set_normal_estimation");
  }
  std::size_t numSubmaps() const { return submaps_.size(); }
  std::size_t activeSubmapIdx() const { return activeIdx_; }
  SubmapHip& activeSubmap() { return *submaps_[activeIdx_].map; }
  // Submap::computeFeatures of submap `idx` (sparse cloud, normals, FPFH stay resident in it); returns the number of sparse points.
  // keypoints (nullable = off): ISS keypoint selection right behind the features (SubmapHip::selectKeypoints) — the feature set
  // place recognition searches is then the keypoints' alone, and the number returned is theirs
  std::int64_t computeFeatures(std::size_t idx, const o3s_submap_feature_params* params = nullptr, const o3s_iss_params* keypoints = nullptr) {
    o3s_submap_feature_params p;
    o3s_submap_feature_params_default(&p);
    if (params) p = *params;
    if (o3s_submap_compute_features(submaps_.at(idx).map->handle(), &p) != O3S_OK) throw std::runtime_error("o3s_submap_compute_features failed");
    if (keypoints) submaps_.at(idx).map->selectKeypoints(*keypoints);
    if (voxel_ > 0.0) submaps_.at(idx).map->buildVoxelMap(kVoxelExpansionFactorAdjacencyBasedRevisiting * voxel_);  // Submap.cpp:260-264
    return o3s_submap_features_size(submaps_.at(idx).map->handle());
  }
  // SubmapCollection::computeFeatures(finishedSubmapIds) (:257-281): the features of every finished submap, each pushed to the
  // loop-closure candidates, and the odometry constraints of the finished submaps into the collection's own list (one device call:
  // o3s_constraint_builders.hpp).  The reference runs the features on a second thread; here the two steps run one after the other on
  // the caller (both settle and use the streams of the same submaps).
  void computeFeatures(const std::vector<std::pair<std::size_t, double>>& finishedSubmapIds, const o3s_submap_feature_params* params = nullptr,
                       const o3s_iss_params* keypoints = nullptr) {
    for (const auto& id : finishedSubmapIds) {
      computeFeatures(id.first, params, keypoints);
      loopClosureCandidates_.push_back(id);
    }
    computeOdometryConstraints(*this, finishedSubmapIds, &odometryConstraints_);
  }
  const Constraints& getOdometryConstraints() const { return odometryConstraints_; }  // :287-289
  std::vector<std::pair<std::size_t, double>> popLoopClosureCandidates() {                // loopClosureCandidatesIdxs_.popAllElements()
    std::vector<std::pair<std::size_t, double>> out;
    out.swap(loopClosureCandidates_);
    return out;
  }
  const o3s_submap* submapHandle(std::size_t i) { return submaps_.at(i).map->handle(); }
  double mapVoxelSize() const { return voxel_; }
  bool isRefineOdometryConstraintsBetweenSubmaps() const { return isRefineOdometryConstraints_; }  // Parameters.hpp:177; every parameter file: false
  void setRefineOdometryConstraintsBetweenSubmaps(bool on) { isRefineOdometryConstraints_ = on; }
  // SubmapCollection::isSwitchingSubmapsConsistant (:392-407) as written in its commented body, over the resident merge cloud of
  // `scan` (what insertScan passes as preProcessedScan).  A candidate without a snapshot has fitness 0; an empty scan NaN: both false.
  bool isSwitchingSubmapsConsistant(const o3s_scan* scan, std::size_t newActiveSubmapCandidate, const double mapToRangeSensor[16]) {
    lastSwitchFitness_ = submaps_.at(newActiveSubmapCandidate).map->overlapFitness(scan, 0, mapToRangeSensor);
    return lastSwitchFitness_ > params_.adjacencyBasedRevisitingMinFitness;
  }
  // fitness of the last consistency check (NaN: none was made by the last insertScan)
  double lastSwitchFitness() const { return lastSwitchFitness_; }
  const Entry& submap(std::size_t i) const { return submaps_.at(i); }
  SubmapHip& submapMap(std::size_t i) { return *submaps_.at(i).map; }
  const AdjacencyHip& adjacency() const { return adjacency_; }
  void forceNewSubmapCreationAtNextScan() { isForceNewSubmapCreation_ = true; }
  // SubmapCollection::updateAdjacencyMatrix (:72-78): a loop-closure constraint makes its two submaps adjacent
  void addLoopClosureEdge(std::size_t idA, std::size_t idB) { adjacency_.addEdge(idA, idB); }
  // SubmapCollection::popFinishedSubmapIds (:53-55)
  std::vector<std::pair<std::size_t, double>> popFinishedSubmapIds() {
    std::vector<std::pair<std::size_t, double>> out(finished_.begin(), finished_.end());
    finished_.clear();
    return out;
  }
  // SubmapCollection::updateAdjacencyMatrix (:75-81)
  void updateAdjacencyMatrix(const Constraints& loopClosureConstraints) {
    for (const auto& c : loopClosureConstraints) {
      adjacency_.addEdge(c.sourceSubmapIdx, c.targetSubmapIdx);
      adjacency_.markAsLoopClosureSubmap(c.sourceSubmapIdx);
      adjacency_.markAsLoopClosureSubmap(c.targetSubmapIdx);
    }
  }
  // the dense map the driver keeps for submap `idx` (Submap::denseMap_): transform() moves it with the submap; not owned
  void setDenseMap(std::size_t idx, DenseMapHip* dense) { denseMaps_[idx] = dense; }
  // SubmapCollection::transform (:324-375).  A submap that more than one increment names is refused (the reference would move it
  // twice; the batched device call takes every submap once).
  void transform(const OptimizedTransforms& transformIncrements) {
    std::vector<std::size_t> parents;
    for (const Entry& e : submaps_) parents.push_back(e.parentId);
    const auto plan = planSubmapTransforms(parents, transformIncrements);
    std::vector<o3s_submap*> maps;
    std::vector<double> Ts;
    for (const auto& p : plan) {
      maps.push_back(submaps_.at(p.first).map->handle());
      Ts.insert(Ts.end(), p.second.m, p.second.m + 16);
    }
    if (!plan.empty()) {  // all device work: one call, one wait
      const int rc = o3s_submaps_transform((std::int32_t)maps.size(), maps.data(), Ts.data());
      if (rc == O3S_ERR_BAD_ARGUMENT) throw std::invalid_argument("SubmapCollection::transform: a submap named twice, or an invalid transform");
      if (rc != O3S_OK) throw std::runtime_error("o3s_submaps_transform failed (status " + std::to_string(rc) + ")");
    }
    for (const auto& p : plan) {
      Entry& e = submaps_[p.first];
      const Mat4& T = p.second;
      e.mapToRangeSensor = mul(e.mapToRangeSensor, T);  // Submap.cpp:126, a right-multiplication
      if (e.isCenterComputed) {                         // :127 (submapCenter_ is zero until it is computed; nobody reads it before)
        double v[3];
        for (int r = 0; r < 3; ++r) v[r] = ((T(r, 0) * e.center[0] + T(r, 1) * e.center[1]) + T(r, 2) * e.center[2]) + T(r, 3);
        for (int r = 0; r < 3; ++r) e.center[r] = v[r];
      }
      const auto it = denseMaps_.find(p.first);
      if (it != denseMaps_.end() && it->second) it->second->transform(T.m);
    }
    while (!buffer_.empty()) {  // :374 overlapScansBuffer_.clear(): the scan objects are free again
      free_.push_back(buffer_.front().scan);
      buffer_.pop_front();
    }
  }
  // SubmapCollection::getTotalNumPoints (:69-73); completes pending inserts (o3s_submap_size)
  std::size_t getTotalNumPoints() const {
    std::size_t sum = 0;
    for (const Entry& e : submaps_) sum += (std::size_t)e.map->size();
    return sum;
  }
  // The loop of Mapper::getAssembledMapPointCloud (Mapper.cpp:524-535) as one device call: every submap in index order — the active
  // one is not special — into `out`.  voxelSize <= 0: the plain concatenation (what saveMap writes); > 0: Open3D VoxelDownSample of it
  // (publishMaps).  attrs: O3S_ASSEMBLE_NORMALS | O3S_ASSEMBLE_COLORS; an attribute not every non-empty submap carries is dropped.
  // Call it from the thread that inserts (the rule of o3s_submap_clone).  Returns the size of the result.
  std::int64_t assembleMap(AssembledMapHip& out, double voxelSize = 0.0, int attrs = O3S_ASSEMBLE_NORMALS | O3S_ASSEMBLE_COLORS) {
    std::vector<o3s_submap*> maps;
    for (Entry& e : submaps_) maps.push_back(e.map->handle());
    std::int64_t n = 0;
    const int rc = o3s_assembled_map_build(out.handle(), (std::int32_t)maps.size(), maps.data(), voxelSize, (std::int32_t)attrs, &n);
    if (rc == O3S_ERR_BAD_ARGUMENT) throw std::invalid_argument("SubmapCollection::assembleMap: too many points, or a voxel size the map's extent does not pack with");
    if (rc != O3S_OK) throw std::runtime_error("o3s_assembled_map_build failed (status " + std::to_string(rc) + ")");
    return n;
  }
  bool lastInsertSwitchedSubmaps() const { return lastSwitched_; }
  // where the last switch of submaps spent its time, ms: creating the new object | the closing scan into the previous submap | its
  // centre | retiring it (hand-over / trim) | the buffered scans into the new one
  const double* lastSwitchMs() const { return lastSwitchMs_; }

  // SubmapCollection::insertScan (:193-247).  `scan` is the object returned by scanForNextMeasurement(), pre-processed
  // (its merge cloud is what Submap::insertScan receives as preProcessedScan).  The initial map of the localisation mode
  // (Mapper.cpp:180-183) goes straight into activeSubmap(): that mode never switches submaps, so the buffer is never replayed.
  bool insertScan(o3s_scan* scan, const double mapToRangeSensor[16], double timestamp) {
    lastSwitched_ = false;
    lastSwitchFitness_ = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 16; ++k) mapToRangeSensor_[k] = mapToRangeSensor[k];
    const std::size_t prevActive = activeIdx_;
    // ":201 if (submaps_.empty())" never holds — the constructor has created submap 0 — so the first scan takes the general
    // path like every other: buffered, no switch before minNumRangeData_ scans, inserted into the active submap
    addScanToBuffer(scan, mapToRangeSensor, timestamp);  // :210
    updateActiveSubmap(scan);                            // :213
    if (prevActive != activeIdx_) {                      // :216-239
      lastSwitched_ = true;
      const auto t0 = std::chrono::steady_clock::now();
      insertInto(prevActive, scan, mapToRangeSensor);
      const auto t1 = std::chrono::steady_clock::now();
      computeSubmapCenter(prevActive);
      const auto t2 = std::chrono::steady_clock::now();
      retire(prevActive);  // only now: the closing scan has gone in, the previous submap is no longer inserted into
      const auto t3 = std::chrono::steady_clock::now();
      finished_.emplace_back(prevActive, timestamp);
      numScansMergedInActiveSubmap_ = 0;
      adjacency_.addEdge(submaps_[prevActive].id, submaps_[activeIdx_].id);
      insertBufferedScans(activeIdx_);
      const auto t4 = std::chrono::steady_clock::now();
      auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
      lastSwitchMs_[0] = lastCreateMs_;
      lastSwitchMs_[1] = ms(t0, t1);
      lastSwitchMs_[2] = ms(t1, t2);
      lastSwitchMs_[3] = ms(t2, t3);
      lastSwitchMs_[4] = ms(t3, t4);
      if (submaps_[activeIdx_].map->size() == 0) throw std::logic_error("submap should not be empty after switching");
    } else {
      insertInto(activeIdx_, scan, mapToRangeSensor);  // :243
    }
    ++numScansMergedInActiveSubmap_;
    return true;
  }

 private:
  struct Buffered {
    o3s_scan* scan;
    double T[16];
    double time;
  };

  void insertInto(std::size_t idx, o3s_scan* scan, const double T[16]) {
    for (int k = 0; k < 16; ++k) submaps_[idx].mapToRangeSensor.m[k] = T[k];
    const int rc = o3s_submap_insert_processed(submaps_[idx].map->handle(), scan, T);
    if (rc != O3S_OK) throw std::runtime_error("o3s_submap_insert_processed failed (status " + std::to_string(rc) + ")");
  }
  // CircularBuffer::push with a size limit (:82-84): the oldest entry falls out and its scan object becomes free again
  void addScanToBuffer(o3s_scan* scan, const double T[16], double time) {
    if (free_.empty() || free_.back() != scan) throw std::logic_error("insertScan expects the object of scanForNextMeasurement()");
    free_.pop_back();
    Buffered b{scan, {}, time};
    for (int k = 0; k < 16; ++k) b.T[k] = T[k];
    buffer_.push_back(b);
    while ((int)buffer_.size() > params_.numScansOverlap) {
      free_.push_back(buffer_.front().scan);
      buffer_.pop_front();
    }
    if (free_.empty()) throw std::logic_error("scan ring exhausted");
  }
  void insertBufferedScans(std::size_t idx) {  // :86-92 (pops everything, oldest first)
    while (!buffer_.empty()) {
      insertInto(idx, buffer_.front().scan, buffer_.front().T);
      free_.push_back(buffer_.front().scan);
      buffer_.pop_front();
    }
  }
  void computeSubmapCenter(std::size_t idx) {
    Entry& e = submaps_[idx];
    if (o3s_submap_center(e.map->handle(), e.center) != O3S_OK) throw std::runtime_error("o3s_submap_center failed");
    e.isCenterComputed = true;
  }
  static double dist3(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
  }
  // A submap that stops being the active one keeps its map cloud and nothing else: the closed submaps of a long run do not hold a
  // spare array and a work area each (~120 MB per submap at the default limits).  What it held goes to its successor — AFTER the
  // closing scan, which insertScan still puts into it (:216-239; round 4 trimmed it before that insert, which allocated most of it
  // again).  A brand-new successor takes the buffers over as they are (o3s_submap_hand_over: pointers change hands, no hipFree /
  // hipMalloc of the large arrays — 5 - 6 ms on the mapping thread per created submap before); an older submap that is
  // re-activated holds a map already: the previous one is trimmed and the re-activated one sized again (rare: a revisit).
  void retire(std::size_t prev) {
    if (prev >= submaps_.size() || prev == activeIdx_) return;
    SubmapHip& closed = *submaps_[prev].map;
    SubmapHip& next = *submaps_[activeIdx_].map;
    if (next.size() == 0) {
      closed.handOverTo(next);
    } else {
      closed.trim();
      reserveFor(next);
    }
  }
  void reserveFor(SubmapHip& m) {
    // a submap is closed at the scan after it passes maxNumPoints_ (:118-120): with a finite limit its arrays are sized once
    if (params_.maxNumPoints > 0 && params_.maxNumPoints <= kReserveLimit) m.reserve(params_.maxNumPoints + kReserveScanPoints);
  }
  void createNewSubmap(const double origin[3]) {  // :150-162
    const auto c0 = std::chrono::steady_clock::now();
    Entry e;
    e.map = std::make_unique<SubmapHip>(voxel_, cropper_, device_);
    if (submaps_.empty()) reserveFor(*e.map);  // the first submap; every later one inherits its predecessor's buffers (retire)
    e.id = submapId_++;
    e.parentId = activeIdx_;
    for (int a = 0; a < 3; ++a) e.origin[a] = origin[a];
    submaps_.push_back(std::move(e));
    activeIdx_ = submaps_.size() - 1;
    numScansMergedInActiveSubmap_ = 0;
    lastCreateMs_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c0).count();
  }
  std::size_t findClosestSubmap(const double p0[3]) const {  // :164-174, std::min_element: the first minimum
    std::size_t best = 0;
    for (std::size_t i = 1; i < submaps_.size(); ++i)
      if (dist3(p0, submaps_[i].mapToSubmapCenter()) < dist3(p0, submaps_[best].mapToSubmapCenter())) best = i;
    return best;
  }
  void updateActiveSubmap(const o3s_scan* scan) {  // :94-148
    const double* p0 = mapToRangeSensor_ + 12;
    if (isForceNewSubmapCreation_) {
      createNewSubmap(p0);
      isForceNewSubmapCreation_ = false;
      return;
    }
    if (numScansMergedInActiveSubmap_ < params_.minNumRangeData) return;
    if (isUseInitialMap_) return;
    const std::size_t closest = findClosestSubmap(p0);
    const std::size_t active = activeIdx_;
    if (submaps_[active].map->largerThan((std::int64_t)params_.maxNumPoints)) isForceNewSubmapCreation_ = true;  // (size() > maxNumPoints_, :118-120)
    const bool isAnotherSubmapWithinRange = dist3(p0, submaps_[closest].mapToSubmapCenter()) < params_.radius;
    if (isAnotherSubmapWithinRange) {
      if (closest == active) return;
      if (adjacency_.isAdjacent(submaps_[closest].id, submaps_[active].id) &&
          (!params_.isCheckSwitchingConsistency || isSwitchingSubmapsConsistant(scan, closest, mapToRangeSensor_))) {  // :132-133
        activeIdx_ = closest;  // (insertScan retires the previous one once the closing scan is in)
      } else {
        const bool isTraveledSufficientDistance = dist3(p0, submaps_[active].mapToSubmapCenter()) > params_.radius;
        if (isTraveledSufficientDistance) createNewSubmap(p0);
      }
    } else {
      createNewSubmap(p0);
    }
  }

  static constexpr double kVoxelExpansionFactorAdjacencyBasedRevisiting = 2.5;  // magic.hpp:16
  static constexpr std::int64_t kReserveLimit = 8000000;      // larger limits mean "no limit": the arrays then double as the map grows
  static constexpr std::int64_t kReserveScanPoints = 262144;  // the scan that takes the map over the limit (2 x a 64 x 2048 sweep)
  SubmapParams params_;
  double voxel_;
  o3s_cropper cropper_;
  bool isUseInitialMap_;
  int device_;
  std::vector<Entry> submaps_;
  std::size_t activeIdx_ = 0, submapId_ = 0;
  int numScansMergedInActiveSubmap_ = 0;
  bool isForceNewSubmapCreation_ = false, lastSwitched_ = false;
  double lastSwitchMs_[5] = {0, 0, 0, 0, 0}, lastCreateMs_ = 0.0;
  double lastSwitchFitness_ = std::numeric_limits<double>::quiet_NaN();
  double mapToRangeSensor_[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::deque<Buffered> buffer_;
  std::vector<o3s_scan*> free_;
  std::deque<std::pair<std::size_t, double>> finished_;
  std::vector<std::pair<std::size_t, double>> loopClosureCandidates_;  // loopClosureCandidatesIdxs_
  Constraints odometryConstraints_;
  bool isRefineOdometryConstraints_ = false;
  AdjacencyHip adjacency_;
  std::map<std::size_t, DenseMapHip*> denseMaps_;
};

}  // namespace o3s
