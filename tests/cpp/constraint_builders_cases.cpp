// Drives cpp/o3s_constraint_builders.hpp for tests/test_constraint_builders_cpp.py.  stdin, one command per line:
//   submap parent [file of 3 x N doubles]      appends a submap (its id is its index); with the argument `device` the file is uploaded
//   voxel v | active i | refine 0|1            mapVoxelSize(), activeSubmapIdx(), isRefineOdometryConstraintsBetweenSubmaps()
//   have s t                                   a constraint (s, t) that is already in the list
//   empty s t                                  (stand-in calls) the pair's overlap is empty
//   candidates id ...                          the candidates overload of computeOdometryConstraints
//   all                                        the all-submaps overload
//   clear                                      empties the list
// Every call of a stand-in prints `call ...` / `refine ...`; after `candidates` / `all` every constraint of the list is printed with
// the bits of its matrices, then `end`.  Without `device` the two device calls are stand-ins and no submap handle is real.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "o3s_submap_collection.hpp"

// compiled, never called: the builders and the worker's body against SubmapCollectionHip and PlaceRecognitionHip themselves
#include "o3s_place_recognition.hpp"
o3s::Constraints step_of(o3s::SubmapCollectionHip& collection, o3s::PlaceRecognitionHip& place, o3s::OptimizationProblemHip& problem) {
  collection.computeFeatures(collection.popFinishedSubmapIds());
  return o3s::loopClosureStep(collection, place, problem, collection.popLoopClosureCandidates());
}

struct Entry {
  std::size_t id, parentId;
};
struct Collection {
  std::vector<Entry> entries;
  std::vector<std::unique_ptr<o3s::SubmapHip>> maps;  // `device` only
  std::size_t active = 0;
  double voxel = 0.1;
  bool refineFlag = false;
  std::size_t numSubmaps() const { return entries.size(); }
  std::size_t activeSubmapIdx() const { return active; }
  const Entry& submap(std::size_t i) const { return entries.at(i); }
  const o3s_submap* submapHandle(std::size_t i) {
    return maps.empty() ? reinterpret_cast<const o3s_submap*>(i + 1) : maps.at(i)->handle();  // stand-in: the index, never dereferenced
  }
  double mapVoxelSize() const { return voxel; }
  bool isRefineOdometryConstraintsBetweenSubmaps() const { return refineFlag; }
};

int main(int argc, char** argv) {
  const bool device = argc > 1 && std::strcmp(argv[1], "device") == 0;
  Collection col;
  o3s::Constraints list;
  std::set<std::pair<std::size_t, std::size_t>> emptyPairs;
  auto index = [](const o3s_submap* h) { return (std::size_t)reinterpret_cast<std::uintptr_t>(h) - 1; };
  o3s::ConstraintDeviceCalls calls;
  if (!device) {
    calls.constraints = [&](std::int32_t n, const o3s_submap* const* s, const o3s_submap* const* t, double voxel, std::int64_t minPoints, double maxDist,
                            double* infos, std::int32_t* statuses) {
      std::printf("call %d %a %a %lld", (int)n, voxel, maxDist, (long long)minPoints);
      for (std::int32_t k = 0; k < n; ++k) {
        std::printf(" %zu:%zu", index(s[k]), index(t[k]));
        const bool none = emptyPairs.count({index(s[k]), index(t[k])}) != 0;
        statuses[k] = none ? O3S_ERR_EMPTY_REFERENCE : O3S_OK;
        for (int e = 0; e < 36; ++e) infos[36 * k + e] = none ? 0.0 : (double)(k + 1);
      }
      std::printf("\n");
      return (int)O3S_OK;
    };
    calls.refine = [&](const o3s_submap* s, const o3s_submap* t, double maxDist, double voxel, std::int64_t minPoints, int maxIteration, double* T,
                       double* info) {
      std::printf("refine %zu %zu %a %a %lld %d\n", index(s), index(t), maxDist, voxel, (long long)minPoints, maxIteration);
      if (emptyPairs.count({index(s), index(t)})) return (int)O3S_ERR_EMPTY_REFERENCE;
      for (int e = 0; e < 16; ++e) T[e] = e % 5 == 0 ? 1.0 : 0.0;
      T[12] = 0.5;
      for (int e = 0; e < 36; ++e) info[e] = 3.0;
      return (int)O3S_OK;
    };
  }
  o3s_cropper big{};
  big.kind = 1;  // MaxRadius
  big.p0 = 1.0e6;
  auto print = [&]() {
    for (const auto& c : list) {
      std::printf("constraint %zu %zu %d %d", c.sourceSubmapIdx, c.targetSubmapIdx, (int)c.isInformationMatrixValid, (int)c.isOdometryConstraint);
      for (double v : c.sourceToTarget.m) std::printf(" %a", v);
      for (double v : c.informationMatrix) std::printf(" %a", v);
      std::printf("\n");
    }
    std::printf("end\n");
  };
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "submap") {
      Entry e;
      std::string path;
      in >> e.parentId >> path;
      e.id = col.entries.size();
      col.entries.push_back(e);
      if (device) {
        col.maps.push_back(std::make_unique<o3s::SubmapHip>(0.0, big, 0));
        std::ifstream f(path, std::ios::binary | std::ios::ate);
        const std::streamsize bytes = f.tellg();
        f.seekg(0);
        std::vector<double> pts((std::size_t)bytes / 8);
        f.read(reinterpret_cast<char*>(pts.data()), bytes);
        if (o3s_submap_upload(col.maps.back()->handle(), pts.data(), nullptr, (std::int64_t)(pts.size() / 3)) != O3S_OK) return 2;
      }
    } else if (cmd == "voxel") {
      in >> col.voxel;
    } else if (cmd == "active") {
      in >> col.active;
    } else if (cmd == "refine") {
      int on = 0;
      in >> on;
      col.refineFlag = on != 0;
    } else if (cmd == "have" || cmd == "empty") {
      std::size_t s, t;
      in >> s >> t;
      if (cmd == "empty") {
        emptyPairs.insert({s, t});
      } else {
        o3s::Constraint c;
        c.sourceSubmapIdx = s;
        c.targetSubmapIdx = t;
        list.push_back(c);
      }
    } else if (cmd == "clear") {
      list.clear();
    } else if (cmd == "candidates") {
      std::vector<std::pair<std::size_t, double>> cand;
      std::size_t id;
      while (in >> id) cand.emplace_back(id, 0.0);
      o3s::computeOdometryConstraints(col, cand, &list, calls);
      print();
    } else if (cmd == "all") {
      o3s::computeOdometryConstraints(col, &list, calls);
      print();
    }
  }
  return 0;
}
