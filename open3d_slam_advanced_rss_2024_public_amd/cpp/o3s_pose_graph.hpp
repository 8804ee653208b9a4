// o3s_pose_graph.hpp — header-only C++17 restatement of the back end of a loop closure: o3d_slam::Constraint (Constraint.hpp),
// OptimizationProblem (open3d_slam/src/OptimizationProblem.cpp; line numbers below are its own) and the plan of
// SubmapCollection::transform (SubmapCollection.cpp:324-375) over the C ABI.  pose_graph.py is its Python mirror: same logic,
// same bits.
//
//   :25-44     solve: GlobalOptimization(poseGraph_, LevenbergMarquardt, default criteria, the four option fields) —
//              o3s_global_optimization (pose_graph/o3s_pose_graph.h), host arithmetic in the library
//   :50-62     buildOptimizationProblem: only the EDGES are cleared; the nodes stay and are extended
//   :64-99     odometry edges (certain; source < target) and the new nodes, chained from the last OPTIMISED node
//              (numOdometryEdgesPrev_, poseGraphOptimized_.nodes_.back().pose_.inverse())
//   :101-121   loop-closure edges (uncertain; source > target; the information matrix must be valid)
//   :151-189   the constraint lists; insertLoopClosureConstraints drops a (source, target) pair that is already there
//   :191-202   getOptimizedTransformIncrements: dT_ is the optimised node pose ITSELF (:197)
// Deviation: the std::sort comparator at :66-67 sets a source against a target and is not a strict weak order; the odometry
// constraints are sorted stably by source index here.  Matrix inverses are isometry inverses (o3s_pose.hpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "o3s_pose.hpp"
#include "pose_graph/o3s_pose_graph.h"

namespace o3s {

struct Constraint {  // Constraint.hpp:14-22
  Mat4 sourceToTarget = Mat4::identity();
  std::size_t sourceSubmapIdx = 0, targetSubmapIdx = 0;
  double informationMatrix[36] = {1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1};  // column-major
  bool isInformationMatrixValid = false;
  bool isOdometryConstraint = true;
  double timestamp = 0.0;
};
using Constraints = std::vector<Constraint>;

struct OptimizedTransform {
  Mat4 dT;
  std::size_t submapId;
};
using OptimizedTransforms = std::vector<OptimizedTransform>;

struct GlobalOptimizationParams {  // Parameters.hpp:142-146 (the parameter files set maxCorrespondenceDistance = 1000.0)
  double maxCorrespondenceDistance = 10.0;
  double loopClosurePreference = 2.0;
  double edgePruneThreshold = 0.2;
  int referenceNode = 0;
};

struct PoseGraphHip {  // registration::PoseGraph
  std::vector<Mat4> nodes;
  std::vector<o3s_pose_graph_edge> edges;
};

class OptimizationProblemHip {
 public:
  explicit OptimizationProblemHip(const GlobalOptimizationParams& p = GlobalOptimizationParams()) : params_(p) {}

  void clearOdometryConstraints() { odometryConstraints_.clear(); }
  void clearLoopClosureConstraints() { loopClosureConstraints_.clear(); }
  void addOdometryConstraint(const Constraint& c) { odometryConstraints_.push_back(c); }
  void addLoopClosureConstraint(const Constraint& c) { loopClosureConstraints_.push_back(c); }
  void insertOdometryConstraints(const Constraints& cs) { odometryConstraints_.insert(odometryConstraints_.end(), cs.begin(), cs.end()); }
  void insertLoopClosureConstraints(const Constraints& cs) {  // :177-189
    for (const auto& c : cs) {
      const auto it = std::find_if(loopClosureConstraints_.begin(), loopClosureConstraints_.end(), [&c](const Constraint& c2) {
        return c.sourceSubmapIdx == c2.sourceSubmapIdx && c.targetSubmapIdx == c2.targetSubmapIdx;
      });
      if (it == loopClosureConstraints_.end()) loopClosureConstraints_.push_back(c);
    }
  }
  const Constraints& getLoopClosureConstraints() const { return loopClosureConstraints_; }
  void updateLoopClosureConstraint(std::size_t idx, const Constraint& c) { loopClosureConstraints_.at(idx) = c; }

  void buildOptimizationProblem() {  // :50-62
    poseGraph_.edges.clear();
    setupOdometryEdgesAndPoseGraphNodes();
    setupLoopClosureEdges();
  }

  void solve() {  // :25-44
    o3s_global_optimization_criteria criteria;
    o3s_global_optimization_option option;
    o3s_global_optimization_defaults(&criteria, &option);
    option.max_correspondence_distance = params_.maxCorrespondenceDistance;
    option.reference_node = params_.referenceNode;
    option.edge_prune_threshold = params_.edgePruneThreshold;
    option.preference_loop_closure = params_.loopClosurePreference;
    poseGraphNonOptimized_ = poseGraph_;
    std::int32_t nOut = 0;
    static_assert(sizeof(Mat4) == 16 * sizeof(double), "Mat4 is 16 doubles");
    const int rc = o3s_global_optimization((std::int32_t)poseGraph_.nodes.size(), poseGraph_.nodes.empty() ? nullptr : poseGraph_.nodes[0].m,
                                           (std::int32_t)poseGraph_.edges.size(), poseGraph_.edges.data(), &nOut, &criteria, &option, &lastStats_);
    if (rc != O3S_OK) throw std::runtime_error("o3s_global_optimization failed (status " + std::to_string(rc) + ")");
    poseGraph_.edges.resize((std::size_t)nOut);
    poseGraphOptimized_ = poseGraph_;
  }

  OptimizedTransforms getOptimizedTransformIncrements() const {  // :191-202
    if (poseGraphOptimized_.nodes.size() != poseGraph_.nodes.size()) throw std::logic_error("Graphs are not of same size, did you run the optimization?");
    OptimizedTransforms out;
    for (std::size_t i = 0; i < poseGraph_.nodes.size(); ++i) out.push_back(OptimizedTransform{poseGraphOptimized_.nodes[i], i});  // :197 deltaT = tNew
    return out;
  }

  const PoseGraphHip& poseGraph() const { return poseGraph_; }
  const PoseGraphHip& poseGraphOptimized() const { return poseGraphOptimized_; }
  const o3s_global_optimization_stats& lastStats() const { return lastStats_; }

 private:
  static o3s_pose_graph_edge makeEdge(const Constraint& c, bool uncertain) {
    o3s_pose_graph_edge e{};
    e.source = (std::int32_t)c.sourceSubmapIdx;
    e.target = (std::int32_t)c.targetSubmapIdx;
    e.uncertain = uncertain ? 1 : 0;
    for (int k = 0; k < 16; ++k) e.transformation[k] = c.sourceToTarget.m[k];
    for (int k = 0; k < 36; ++k) e.information[k] = c.informationMatrix[k];
    e.confidence = 1.0;
    return e;
  }
  void setupOdometryEdgesAndPoseGraphNodes() {  // :64-99
    std::stable_sort(odometryConstraints_.begin(), odometryConstraints_.end(),
                     [](const Constraint& a, const Constraint& b) { return a.sourceSubmapIdx < b.sourceSubmapIdx; });
    for (const auto& c : odometryConstraints_) {
      if (!(c.targetSubmapIdx > c.sourceSubmapIdx)) throw std::logic_error("id_source should always be less than id_target for the odometry constraints");
      poseGraph_.edges.push_back(makeEdge(c, false));
    }
    Mat4 odometry = Mat4::identity();
    if (!poseGraphOptimized_.edges.empty()) {
      odometry = inverse_isometry(poseGraphOptimized_.nodes.back());  // :87
    } else {
      poseGraph_.nodes.push_back(Mat4::identity());  // :89 (again on every build until a solve has left edges)
    }
    for (std::size_t i = numOdometryEdgesPrev_; i < odometryConstraints_.size(); ++i) {
      odometry = mul(odometryConstraints_[i].sourceToTarget, odometry);
      poseGraph_.nodes.push_back(inverse_isometry(odometry));
    }
    numOdometryEdgesPrev_ = odometryConstraints_.size();
  }
  void setupLoopClosureEdges() {  // :101-121
    numLoopClosuresPrev_ = loopClosureConstraints_.size();
    for (const auto& c : loopClosureConstraints_) {
      if (!c.isInformationMatrixValid)
        throw std::logic_error("Invalid information matrix between: " + std::to_string(c.sourceSubmapIdx) + " and " + std::to_string(c.targetSubmapIdx));
      if (!(c.sourceSubmapIdx > c.targetSubmapIdx)) throw std::logic_error("Optimization problem, loop closure constraints: source should be greater than target");
      poseGraph_.edges.push_back(makeEdge(c, true));
    }
  }

  GlobalOptimizationParams params_;
  PoseGraphHip poseGraph_, poseGraphOptimized_, poseGraphNonOptimized_;
  Constraints odometryConstraints_, loopClosureConstraints_;
  std::size_t numOdometryEdgesPrev_ = 0, numLoopClosuresPrev_ = 0;
  o3s_global_optimization_stats lastStats_{};
};

// Which transform goes to which submap (SubmapCollection.cpp:324-371), in the reference's order of application: the submaps an
// increment names get theirs; every other submap walks up its parents until one is not among the unnamed submaps and takes
// increments.at(parent) — a POSITIONAL lookup, as written (:362).  parents[i]: Submap::getParentId() of submap i.
inline std::vector<std::pair<std::size_t, Mat4>> planSubmapTransforms(const std::vector<std::size_t>& parents, const OptimizedTransforms& increments) {
  const std::size_t n = parents.size();
  std::vector<std::pair<std::size_t, Mat4>> plan;
  std::vector<bool> named(n, false);
  for (const auto& u : increments)
    if (u.submapId < n) {  // (else: "trying to update submap ... but there are only ...", :337 — reported and skipped)
      plan.emplace_back(u.submapId, u.dT);
      named[u.submapId] = true;
    }
  for (std::size_t idx = 0; idx < n; ++idx) {
    if (named[idx]) continue;
    std::size_t current = idx;
    while (!increments.empty()) {  // "while (true && !transformIncrements.empty())"
      current = parents.at(current);
      if (named.at(current)) {  // the parent is in the pose graph
        plan.emplace_back(idx, increments.at(current).dT);
        break;
      }
      if (current == parents.at(current)) throw std::runtime_error("Stuck in a loop, this should not happen");
    }
  }
  return plan;
}

// SlamWrapper::updateSubmapsAndTrajectory (SlamWrapper.cpp:1105-1140).  Collection: transform(const OptimizedTransforms&) and
// updateAdjacencyMatrix(const Constraints&) (SubmapCollectionHip); Mapper: loopClosureUpdate(const Mat4&) (MapperHip).
template <class Collection, class Mapper>
OptimizedTransforms updateSubmapsAndTrajectory(OptimizationProblemHip& problem, Collection& collection, Mapper& mapper, const Constraints& lastConstraints) {
  const OptimizedTransforms increments = problem.getOptimizedTransformIncrements();
  collection.transform(increments);
  if (lastConstraints.empty()) throw std::logic_error("updateSubmapsAndTrajectory: no loop-closure constraint");
  const Constraint latest = *std::max_element(lastConstraints.begin(), lastConstraints.end(),
                                              [](const Constraint& a, const Constraint& b) { return a.timestamp < b.timestamp; });
  if (!(latest.sourceSubmapIdx > latest.targetSubmapIdx)) throw std::logic_error("update submaps and trajectory: the source of a loop closure is the later submap");
  mapper.loopClosureUpdate(increments.at(latest.sourceSubmapIdx).dT);
  Constraints cs = problem.getLoopClosureConstraints();
  for (std::size_t i = 0; i < cs.size(); ++i) {
    cs[i].sourceToTarget = Mat4::identity();
    problem.updateLoopClosureConstraint(i, cs[i]);
  }
  collection.updateAdjacencyMatrix(cs);
  return increments;
}

}  // namespace o3s
