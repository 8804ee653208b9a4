// Drives cpp/o3s_pose_graph.hpp from a script on stdin so that tests/test_pose_graph.py can compare it bit for bit with the Python
// mirror (pose_graph.py, submap_collection.py).  Numbers travel as C99 hex floats.  Commands, one per line:
//   odom s t <16 T> <36 info>            addOdometryConstraint
//   loop s t valid <16 T> <36 info>      insertLoopClosureConstraints({c})
//   clear_odom | build | solve
//   nodes | edges | increments           print the pose graph's nodes / edges / the optimised increments
//   plan n p0 .. pn-1 k then k lines "id <16 T>"    planSubmapTransforms
// Also pulls in o3s_submap_collection.hpp so that SubmapCollectionHip::transform is compiled by plain g++.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "o3s_pose_graph.hpp"
#include "o3s_submap_collection.hpp"

static double rd(std::istream& in) {
  std::string w;
  in >> w;
  return std::strtod(w.c_str(), nullptr);
}
static void print_mat(const o3s::Mat4& T) {
  for (int k = 0; k < 16; ++k) std::printf(" %a", T.m[k]);
  std::printf("\n");
}
static o3s::Constraint read_constraint(std::istream& in, bool loop) {
  o3s::Constraint c;
  in >> c.sourceSubmapIdx >> c.targetSubmapIdx;
  if (loop) {
    int v = 0;
    in >> v;
    c.isInformationMatrixValid = v != 0;
    c.isOdometryConstraint = false;
  }
  for (int k = 0; k < 16; ++k) c.sourceToTarget.m[k] = rd(in);
  for (int k = 0; k < 36; ++k) c.informationMatrix[k] = rd(in);
  return c;
}

int main() {
  auto keep = &o3s::SubmapCollectionHip::transform;  // instantiates nothing on the device: the member only has to compile and link
  (void)keep;
  o3s::OptimizationProblemHip problem;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    try {
      if (cmd == "odom") problem.addOdometryConstraint(read_constraint(in, false));
      else if (cmd == "loop") problem.insertLoopClosureConstraints({read_constraint(in, true)});
      else if (cmd == "clear_odom") problem.clearOdometryConstraints();
      else if (cmd == "build") problem.buildOptimizationProblem();
      else if (cmd == "solve") problem.solve();
      else if (cmd == "nodes") {
        std::printf("nodes %zu\n", problem.poseGraph().nodes.size());
        for (const auto& T : problem.poseGraph().nodes) print_mat(T);
      } else if (cmd == "edges") {
        std::printf("edges %zu\n", problem.poseGraph().edges.size());
        for (const auto& e : problem.poseGraph().edges) std::printf(" %d %d %d %a\n", e.source, e.target, e.uncertain, e.confidence);
      } else if (cmd == "increments") {
        const auto inc = problem.getOptimizedTransformIncrements();
        std::printf("increments %zu\n", inc.size());
        for (const auto& u : inc) {
          std::printf(" %zu", u.submapId);
          print_mat(u.dT);
        }
      } else if (cmd == "plan") {
        std::size_t n = 0, k = 0;
        in >> n;
        std::vector<std::size_t> parents(n);
        for (auto& p : parents) in >> p;
        in >> k;
        o3s::OptimizedTransforms inc(k);
        for (auto& u : inc) {
          std::getline(std::cin, line);
          std::istringstream li(line);
          li >> u.submapId;
          for (int q = 0; q < 16; ++q) u.dT.m[q] = rd(li);
        }
        const auto plan = o3s::planSubmapTransforms(parents, inc);
        std::printf("plan %zu\n", plan.size());
        for (const auto& p : plan) {
          std::printf(" %zu", p.first);
          print_mat(p.second);
        }
      } else if (!cmd.empty()) {
        std::printf("error: unknown command %s\n", cmd.c_str());
      }
    } catch (const std::exception& e) {
      std::printf("error: %s\n", e.what());
    }
  }
  return 0;
}
