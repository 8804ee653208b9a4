// o3s_constraint_builders.hpp — header-only C++17 restatement of open3d_slam/src/constraint_builders.cpp (line numbers below are
// its own) over resident submaps and the C ABI, and of the body of SlamWrapper::loopClosureWorker (SlamWrapper.cpp:1068-1099).
// constraint_builders.py / pose_graph.loop_closure_step are its Python mirror: same logic, same bits.
//
//   :23-30     hasConstraint
//   :33-41     buildOdometryConstraint: magic.hpp's factors (overlap voxel 20 x, correspondence distance 1.5 x the map voxel size,
//              getMapVoxelSize's value-if-zero 0.04), refinement skipped unless isRefineOdometryConstraintsBetweenSubmaps
//   :43-90     buildConstraint.  Refinement skipped (every parameter file of the reference): overlap selection and Open3D's
//              information matrix at the identity — o3s_submaps_odometry_constraints (constraints/o3s_constraints.h), ALL the pairs
//              of one invocation in ONE call.  Refinement on: o3s_o3d_registration_icp_submaps_overlap per pair (point-to-plane,
//              100 iterations, information matrix at the result; the target needs normals, as in the reference)
//   :92-118    computeOdometryConstraints, both overloads: the candidates overload skips submapId < 1, the pair is
//              (parent(target), target); the all-submaps overload also skips pairs whose source or target is the active submap
// Kept where it looks odd: a pair whose overlap is empty STILL yields its constraint, with the zero information matrix (the reference
// emits it, and hasConstraint — every later invocation — depends on it being there).  Only the form buildConstraint's one caller
// asks for is built: overlap selection and information matrix both on.
// Collection: numSubmaps(), activeSubmapIdx(), submap(i) with .id and .parentId, submapHandle(i), mapVoxelSize(),
// isRefineOdometryConstraintsBetweenSubmaps(), getOdometryConstraints() (SubmapCollectionHip).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "constraints/o3s_constraints.h"
#include "o3s_pose_graph.hpp"
#include "o3s_registration.h"

namespace o3s {

namespace magic {  // magic.hpp:12-15
constexpr double voxelSizeCorrespondenceSearchIfMapVoxelSizeIsZero = 0.04;
constexpr int icpRunUntilConvergenceNumberOfIterations = 100;
constexpr double voxelExpansionFactorOverlapComputation = 20.0;
constexpr double voxelExpansionFactorIcpCorrespondenceDistance = 1.5;
}  // namespace magic

inline double getMapVoxelSize(double mapVoxelSize, double valueIfZero) {  // helpers.cpp:356-358
  return std::fabs(mapVoxelSize) <= 1e-3 ? valueIfZero : mapVoxelSize;
}

inline bool hasConstraint(std::size_t sourceIdx, std::size_t targetIdx, const Constraints& constraints) {  // :23-30
  for (const auto& c : constraints)
    if (c.sourceSubmapIdx == sourceIdx && c.targetSubmapIdx == targetIdx) return true;
  return false;
}

// The two device calls behind the builders; tests of the rules put stand-ins here.
struct ConstraintDeviceCalls {
  // n pairs at the identity: infos n x 36 (column-major), statuses n; returns the call's o3s_status
  std::function<int(std::int32_t, const o3s_submap* const*, const o3s_submap* const*, double overlapVoxel, std::int64_t minPoints, double maxDist,
                    double* infos, std::int32_t* statuses)>
      constraints = [](std::int32_t n, const o3s_submap* const* s, const o3s_submap* const* t, double voxel, std::int64_t minPoints, double maxDist,
                       double* infos, std::int32_t* statuses) {
        return o3s_submaps_odometry_constraints(n, s, t, nullptr, voxel, minPoints, maxDist, infos, nullptr, nullptr, statuses);
      };
  // one pair refined from the identity: T and info (column-major) out; returns o3s_status (O3S_ERR_EMPTY_REFERENCE: empty overlap)
  std::function<int(const o3s_submap*, const o3s_submap*, double maxDist, double overlapVoxel, std::int64_t minPoints, int maxIteration, double* T,
                    double* info)>
      refine = [](const o3s_submap* s, const o3s_submap* t, double maxDist, double voxel, std::int64_t minPoints, int maxIteration, double* T, double* info) {
        o3s_o3d_icp_criteria cr;
        o3s_o3d_icp_default_criteria(&cr);
        cr.max_iteration = maxIteration;
        o3s_o3d_icp_result r{};
        const Mat4 eye = Mat4::identity();
        const int rc = o3s_o3d_registration_icp_submaps_overlap(s, t, maxDist, eye.m, &cr, voxel, minPoints, &r, info, nullptr);
        if (rc == O3S_OK)
          for (int k = 0; k < 16; ++k) T[k] = r.transformation[k];
        return rc;
      };
};

using SubmapPairs = std::vector<std::pair<std::size_t, std::size_t>>;  // (source index, target index)

// buildConstraint (:43-90) for several pairs: one device call for all of them when the refinement is skipped
template <class Collection>
Constraints buildConstraints(const SubmapPairs& pairs, Collection& collection, bool isComputeOverlap, double icpMaxCorrespondenceDistance,
                             double voxelSizeOverlapCompute, bool isEstimateInformationMatrix, bool isSkipIcpRefinement,
                             const ConstraintDeviceCalls& calls = ConstraintDeviceCalls()) {
  if (!isComputeOverlap || !isEstimateInformationMatrix)
    throw std::invalid_argument("buildConstraint: only the overlap-selected constraint with an information matrix is built (its one caller's form)");
  Constraints out;
  if (pairs.empty()) return out;
  const std::int64_t minNumPointsPerVoxel = 1;
  std::vector<const o3s_submap*> src, tgt;
  for (const auto& p : pairs) {
    src.push_back(collection.submapHandle(p.first));
    tgt.push_back(collection.submapHandle(p.second));
  }
  for (const auto& p : pairs) {
    Constraint c;
    c.sourceSubmapIdx = p.first;
    c.targetSubmapIdx = p.second;
    c.isOdometryConstraint = true;
    c.isInformationMatrixValid = isEstimateInformationMatrix;
    c.sourceToTarget = Mat4::identity();
    for (double& v : c.informationMatrix) v = 0.0;
    out.push_back(c);
  }
  if (isSkipIcpRefinement) {
    std::vector<double> infos(36 * pairs.size(), 0.0);
    std::vector<std::int32_t> statuses(pairs.size(), 0);
    const int rc = calls.constraints((std::int32_t)pairs.size(), src.data(), tgt.data(), voxelSizeOverlapCompute, minNumPointsPerVoxel,
                                     icpMaxCorrespondenceDistance, infos.data(), statuses.data());
    if (rc != O3S_OK) throw std::runtime_error("o3s_submaps_odometry_constraints failed (status " + std::to_string(rc) + ")");
    for (std::size_t k = 0; k < pairs.size(); ++k) {
      if (statuses[k] != O3S_OK && statuses[k] != O3S_ERR_EMPTY_REFERENCE)
        throw std::runtime_error("odometry constraint " + std::to_string(pairs[k].first) + " -> " + std::to_string(pairs[k].second) + ": o3s_status " +
                                 std::to_string(statuses[k]));
      for (int e = 0; e < 36; ++e) out[k].informationMatrix[e] = infos[36 * k + (std::size_t)e];
    }
    return out;
  }
  for (std::size_t k = 0; k < pairs.size(); ++k) {
    double T[16], info[36];
    const int rc = calls.refine(src[k], tgt[k], icpMaxCorrespondenceDistance, voxelSizeOverlapCompute, minNumPointsPerVoxel,
                                magic::icpRunUntilConvergenceNumberOfIterations, T, info);
    if (rc == O3S_ERR_EMPTY_REFERENCE) continue;  // identity and the zero matrix
    if (rc == O3S_ERR_BAD_SHAPE) throw std::runtime_error("TransformationEstimationPointToPlane requires target normals");
    if (rc != O3S_OK) throw std::runtime_error("o3s_o3d_registration_icp_submaps_overlap failed (status " + std::to_string(rc) + ")");
    for (int e = 0; e < 16; ++e) out[k].sourceToTarget.m[e] = T[e];
    for (int e = 0; e < 36; ++e) out[k].informationMatrix[e] = info[e];
  }
  return out;
}

template <class Collection>
Constraint buildConstraint(std::size_t sourceIdx, std::size_t targetIdx, Collection& collection, bool isComputeOverlap, double icpMaxCorrespondenceDistance,
                           double voxelSizeOverlapCompute, bool isEstimateInformationMatrix, bool isSkipIcpRefinement,
                           const ConstraintDeviceCalls& calls = ConstraintDeviceCalls()) {
  return buildConstraints({{sourceIdx, targetIdx}}, collection, isComputeOverlap, icpMaxCorrespondenceDistance, voxelSizeOverlapCompute,
                          isEstimateInformationMatrix, isSkipIcpRefinement, calls)[0];
}

// buildOdometryConstraint (:33-41) for several pairs
template <class Collection>
Constraints buildOdometryConstraints(const SubmapPairs& pairs, Collection& collection, const ConstraintDeviceCalls& calls = ConstraintDeviceCalls()) {
  const double mapVoxelSize = getMapVoxelSize(collection.mapVoxelSize(), magic::voxelSizeCorrespondenceSearchIfMapVoxelSizeIsZero);
  Constraints cs = buildConstraints(pairs, collection, true, magic::voxelExpansionFactorIcpCorrespondenceDistance * mapVoxelSize,
                                    magic::voxelExpansionFactorOverlapComputation * mapVoxelSize, true,
                                    !collection.isRefineOdometryConstraintsBetweenSubmaps(), calls);
  for (auto& c : cs) c.isOdometryConstraint = true;
  return cs;
}

template <class Collection>
Constraint buildOdometryConstraint(std::size_t sourceIdx, std::size_t targetIdx, Collection& collection,
                                   const ConstraintDeviceCalls& calls = ConstraintDeviceCalls()) {
  return buildOdometryConstraints({{sourceIdx, targetIdx}}, collection, calls)[0];
}

namespace detail {
// hasConstraint against the list as it grows: a pair named twice in one invocation is built once
template <class Collection>
void appendMissingOdometryConstraints(const SubmapPairs& pairs, Collection& collection, Constraints* constraints, const ConstraintDeviceCalls& calls) {
  SubmapPairs todo;
  for (const auto& p : pairs) {
    bool listed = hasConstraint(p.first, p.second, *constraints);
    for (const auto& q : todo) listed = listed || q == p;
    if (!listed) todo.push_back(p);
  }
  const Constraints built = buildOdometryConstraints(todo, collection, calls);
  constraints->insert(constraints->end(), built.begin(), built.end());
}
}  // namespace detail

// :92-105  candidates: (submap id, time stamp) of finished submaps
template <class Collection>
void computeOdometryConstraints(Collection& collection, const std::vector<std::pair<std::size_t, double>>& candidates, Constraints* constraints,
                                const ConstraintDeviceCalls& calls = ConstraintDeviceCalls()) {
  SubmapPairs pairs;
  for (const auto& candidate : candidates) {
    if (candidate.first < 1) continue;
    const std::size_t targetCandidate = candidate.first;
    pairs.emplace_back(collection.submap(targetCandidate).parentId, targetCandidate);
  }
  detail::appendMissingOdometryConstraints(pairs, collection, constraints, calls);
}

// :107-118  every submap from 1 on
template <class Collection>
void computeOdometryConstraints(Collection& collection, Constraints* constraints, const ConstraintDeviceCalls& calls = ConstraintDeviceCalls()) {
  const std::size_t activeSubmapIdx = collection.submap(collection.activeSubmapIdx()).id;
  SubmapPairs pairs;
  for (std::size_t submapIdx = 1; submapIdx < collection.numSubmaps(); ++submapIdx) {
    const std::size_t targetIdx = submapIdx, sourceIdx = collection.submap(targetIdx).parentId;
    if (sourceIdx != activeSubmapIdx && targetIdx != activeSubmapIdx) pairs.emplace_back(sourceIdx, targetIdx);
  }
  detail::appendMissingOdometryConstraints(pairs, collection, constraints, calls);
}

// The body of SlamWrapper::loopClosureWorker (SlamWrapper.cpp:1068-1099), once: the loop-closure constraints of the candidates; none:
// return and leave the problem alone; else a COPY of the collection's odometry constraints completed with the all-submaps overload,
// the problem's odometry constraints cleared, both kinds inserted, the problem built and solved.  Returns the loop-closure
// constraints: what updateSubmapsAndTrajectory then takes.  Place: buildLoopClosureConstraints(mapToRangeSensor, collection,
// lastFinishedSubmapIdx, activeSubmapIdx, timestamp) (PlaceRecognitionHip).
template <class Collection, class Place>
Constraints loopClosureStep(Collection& collection, Place& placeRecognition, OptimizationProblemHip& problem,
                            const std::vector<std::pair<std::size_t, double>>& candidates, const ConstraintDeviceCalls& calls = ConstraintDeviceCalls()) {
  Constraints loopClosureConstraints;
  for (const auto& id : candidates) {  // SubmapCollection::buildLoopClosureConstraints (:291-299)
    const Constraints cs = placeRecognition.buildLoopClosureConstraints(collection.submap(collection.activeSubmapIdx()).mapToRangeSensor, collection, id.first,
                                                                        collection.activeSubmapIdx(), id.second);
    loopClosureConstraints.insert(loopClosureConstraints.end(), cs.begin(), cs.end());
  }
  if (loopClosureConstraints.empty()) return loopClosureConstraints;
  Constraints odometryConstraints = collection.getOdometryConstraints();
  computeOdometryConstraints(collection, &odometryConstraints, calls);
  problem.clearOdometryConstraints();
  problem.insertLoopClosureConstraints(loopClosureConstraints);
  problem.insertOdometryConstraints(odometryConstraints);
  problem.buildOptimizationProblem();
  problem.solve();
  return loopClosureConstraints;
}

}  // namespace o3s
