// Drives cpp/o3s_place_recognition.hpp and AdjacencyHip (cpp/o3s_submap_collection.hpp) on the CPU for
// tests/test_place_recognition_logic.py: the host policy only, no device call.  stdin, one command per line:
//   edge a b | mark id | dist id                      AdjacencyHip; `dist` prints the distance
//   submap id cx cy cz                                appends a submap of the stand-in collection
//   candidates finished active radius minBetween      prints the candidate indices
//   pose <16 hex doubles, column-major>               prints isRegistrationConsistent under the default limits, then roll pitch yaw
// With the argument `device` (tests/test_gpu_place_recognition_cpp.py) the same stdin builds a collection of RESIDENT submaps instead:
//   cloud <file of 3 x N doubles | -> cx cy cz features   appends a submap (uploaded, with a feature set when features = 1)
//   edge a b
//   closures finished active overlapVoxel registrationType seed maxDriftYaw
//                                                     PlaceRecognitionHip::buildLoopClosureConstraints: prints every candidate, then every constraint
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "o3s_place_recognition.hpp"

struct FakeEntry {
  std::size_t id;
  double c[3];
  const double* mapToSubmapCenter() const { return c; }
};
struct FakeCollection {
  std::vector<FakeEntry> entries;
  o3s::AdjacencyHip adj;
  std::size_t numSubmaps() const { return entries.size(); }
  const FakeEntry& submap(std::size_t i) const { return entries.at(i); }
  const o3s::AdjacencyHip& adjacency() const { return adj; }
};

// compiled, never called: PlaceRecognitionHip::buildLoopClosureConstraints against SubmapCollectionHip itself
o3s::Constraints closures_of(o3s::PlaceRecognitionHip& place, o3s::SubmapCollectionHip& collection, std::size_t finished, double stamp) {
  return place.buildLoopClosureConstraints(o3s::Mat4::identity(), collection, finished, collection.activeSubmapIdx(), stamp);
}

// resident submaps the test uploads itself (SubmapCollectionHip only fills its submaps from scans)
struct DeviceCollection {
  std::vector<FakeEntry> entries;
  std::vector<std::unique_ptr<o3s::SubmapHip>> maps;
  o3s::AdjacencyHip adj;
  std::size_t numSubmaps() const { return entries.size(); }
  const FakeEntry& submap(std::size_t i) const { return entries.at(i); }
  const o3s::AdjacencyHip& adjacency() const { return adj; }
  o3s::SubmapHip& submapMap(std::size_t i) { return *maps.at(i); }
};

static void print_hex(const double* v, int n) {
  for (int k = 0; k < n; ++k) std::printf(" %a", v[k]);
}

static int device_main() {
  DeviceCollection col;
  o3s_cropper big{};
  big.kind = 1;  // MaxRadius
  big.p0 = 1000.0;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "cloud") {
      std::string path;
      FakeEntry e;
      int features = 0;
      in >> path >> e.c[0] >> e.c[1] >> e.c[2] >> features;
      e.id = col.entries.size();
      col.entries.push_back(e);
      col.maps.push_back(std::make_unique<o3s::SubmapHip>(0.1, big, 0));
      if (path != "-") {
        std::ifstream f(path, std::ios::binary | std::ios::ate);
        const std::streamsize bytes = f.tellg();
        f.seekg(0);
        std::vector<double> pts((std::size_t)bytes / 8);
        f.read(reinterpret_cast<char*>(pts.data()), bytes);
        if (o3s_submap_upload(col.maps.back()->handle(), pts.data(), nullptr, (std::int64_t)(pts.size() / 3)) != O3S_OK) return 2;
      }
      if (features) {
        o3s_submap_feature_params fp;
        o3s_submap_feature_params_default(&fp);
        if (o3s_submap_compute_features(col.maps.back()->handle(), &fp) != O3S_OK) return 3;
      }
    } else if (cmd == "edge") {
      std::size_t a, b;
      in >> a >> b;
      col.adj.addEdge(a, b);
    } else if (cmd == "closures") {
      std::size_t finished, active;
      unsigned long long seed;
      o3s::PlaceRecognitionParams p;
      in >> finished >> active >> p.overlapVoxelSize >> p.registrationType >> seed >> p.consistencyCheck.maxDriftYaw;
      p.ransac.seed = seed;
      o3s::PlaceRecognitionHip place(p);
      const o3s::Constraints cs = place.buildLoopClosureConstraints(o3s::Mat4::identity(), col, finished, active, 42.0);
      for (const auto& c : place.lastCandidates()) {
        std::printf("candidate %zu %d %lld %lld", c.targetSubmapIdx, (int)c.rejected, (long long)c.numCorrespondences, (long long)c.ransac.correspondences);
        print_hex(c.ransac.transformation, 16);
        std::printf("\n");
      }
      for (const auto& c : cs) {
        std::printf("constraint %zu %zu %d %d %a", c.sourceSubmapIdx, c.targetSubmapIdx, (int)c.isInformationMatrixValid, (int)c.isOdometryConstraint, c.timestamp);
        print_hex(c.sourceToTarget.m, 16);
        print_hex(c.informationMatrix, 36);
        std::printf("\n");
      }
      std::printf("end\n");
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "device") == 0) return device_main();
  FakeCollection col;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "edge") {
      std::size_t a, b;
      in >> a >> b;
      col.adj.addEdge(a, b);
    } else if (cmd == "mark") {
      std::size_t a;
      in >> a;
      try {
        col.adj.markAsLoopClosureSubmap(a);
      } catch (const std::out_of_range&) {
        std::printf("out_of_range\n");
      }
    } else if (cmd == "dist") {
      std::size_t a;
      in >> a;
      std::printf("%d\n", col.adj.getDistanceToNearestLoopClosureSubmap(a));
    } else if (cmd == "submap") {
      FakeEntry e;
      in >> e.id >> e.c[0] >> e.c[1] >> e.c[2];
      col.entries.push_back(e);
    } else if (cmd == "candidates") {
      std::size_t finished, active;
      o3s::PlaceRecognitionParams p;
      in >> finished >> active >> p.loopClosureSearchRadius >> p.minSubmapsBetweenLoopClosures;
      std::printf("candidates");
      for (std::size_t i : o3s::getLoopClosureCandidatesIdxs(col, finished, active, p)) std::printf(" %zu", i);
      std::printf("\n");
    } else if (cmd == "pose") {
      o3s::Mat4 T;
      for (int k = 0; k < 16; ++k) {
        std::string w;
        in >> w;
        T.m[k] = std::strtod(w.c_str(), nullptr);
      }
      double rpy[3];
      o3s::toRPY(T, rpy);
      std::printf("%d %a %a %a\n", o3s::isRegistrationConsistent(T, o3s::ConsistencyCheckParams()) ? 1 : 0, rpy[0], rpy[1], rpy[2]);
    }
  }
  return 0;
}
