// Drives the two registration health gates of the compiled drivers (cpp/o3s_mapper.hpp, cpp/o3s_submap_collection.hpp) over a
// recorded scene: plain g++, only libo3dslam_icp_hip.so at link time.
//
//   health_gates <scene.bin> <out.txt>
// scene.bin (little endian):
//   int64   mode (0: MapperHip, the fitness gate; 1: SubmapCollectionHip alone, the revisit check), K
//   double  scan_voxel, map_voxel, wide_radius, narrow_radius, ref_period, min_movement
//   double  submap_radius;  int64 min_num_range_data, max_num_points, num_scans_overlap
//   double  min_refinement_fitness, fitness_max_correspondence_distance;  int64 ignore_min_refinement_fitness
//   double  adjacency_based_revisiting_min_fitness;  int64 check_switching_consistency
//   double  first_pose[16]                                         (column-major; mode 0: the pose the first scan is inserted at)
//   K x { double stamp; double pose[16]; int64 N; double pts[3N]; double normals[3N] }     (pose: mode 1 only, mapToRangeSensor)
// out.txt, one line per scan:
//   mode 0  "k ok inserted ref_reset icp_threw rejected n_corr n_points map_size  fitness(%a) rmse(%a)  T(16, %a)"
//   mode 1  "k active n_submaps switched snapshot_sizes...  fitness(%a)"     (after the scan; every finished submap has had its
//           features — and with them its occupancy snapshot — computed, as the reference's feature thread would)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "o3s_mapper.hpp"

template <typename T>
static T rd(std::ifstream& f) {
  T v;
  f.read(reinterpret_cast<char*>(&v), sizeof(T));
  if (!f) {
    std::fprintf(stderr, "scene truncated\n");
    std::exit(2);
  }
  return v;
}
static o3s::Mat4 rd_mat(std::ifstream& f) {
  o3s::Mat4 m;
  f.read(reinterpret_cast<char*>(m.m), sizeof(m.m));
  return m;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  if (!f) return 2;
  const std::int64_t mode = rd<std::int64_t>(f), K = rd<std::int64_t>(f);
  o3s::MapperParams p;
  p.scanVoxelSize = rd<double>(f);
  p.mapVoxelSize = rd<double>(f);
  p.mapBuilderCropper.kind = 1;  // MaxRadius
  p.mapBuilderCropper.p0 = rd<double>(f);
  p.scanMatcherCropper.kind = 1;
  p.scanMatcherCropper.p0 = rd<double>(f);
  p.referenceCloudSettingPeriod = rd<double>(f);
  p.minMovementBetweenMappingSteps = rd<double>(f);
  p.submaps.radius = rd<double>(f);
  p.submaps.minNumRangeData = (int)rd<std::int64_t>(f);
  p.submaps.maxNumPoints = rd<std::int64_t>(f);
  p.submaps.numScansOverlap = (int)rd<std::int64_t>(f);
  p.minRefinementFitness = rd<double>(f);
  p.fitnessMaxCorrespondenceDistance = rd<double>(f);
  p.isIgnoreMinRefinementFitness = rd<std::int64_t>(f) != 0;
  p.submaps.adjacencyBasedRevisitingMinFitness = rd<double>(f);
  p.submaps.isCheckSwitchingConsistency = rd<std::int64_t>(f) != 0;
  const o3s::Mat4 first_pose = rd_mat(f);
  FILE* out = std::fopen(argv[2], "w");
  if (!out) return 2;
  try {
    o3s_icp_config cfg;
    o3s_icp_default_config(&cfg);  // icp.yaml
    std::unique_ptr<o3s::MapperHip> mapper;
    std::unique_ptr<o3s::SubmapCollectionHip> col;
    if (mode == 0) {
      mapper.reset(new o3s::MapperHip(p, cfg, 0));
      mapper->setCalibration(o3s::Mat4::identity());
      mapper->setMapToRangeSensor(first_pose);
    } else {
      col.reset(new o3s::SubmapCollectionHip(p.submaps, p.mapVoxelSize, p.mapBuilderCropper, false, 0));
    }
    for (std::int64_t k = 0; k < K; ++k) {
      const double stamp = rd<double>(f);
      const o3s::Mat4 pose = rd_mat(f);
      const std::int64_t N = rd<std::int64_t>(f);
      std::vector<double> pts((size_t)N * 3), nrm((size_t)N * 3);
      f.read(reinterpret_cast<char*>(pts.data()), (std::streamsize)(pts.size() * 8));
      f.read(reinterpret_cast<char*>(nrm.data()), (std::streamsize)(nrm.size() * 8));
      if (!f) throw std::runtime_error("scene truncated");
      if (mode == 0) {
        const bool ok = mapper->addRangeMeasurement(pts.data(), nrm.data(), N, stamp);
        const o3s_icp_fitness& fit = mapper->lastFitness();
        std::fprintf(out, "%lld %d %d %d %d %d %lld %lld %lld  %a %a ", (long long)k, ok ? 1 : 0, mapper->lastScanInserted() ? 1 : 0,
                     mapper->lastReferenceReset() ? 1 : 0, mapper->lastIcpThrew() ? 1 : 0, mapper->lastFitnessRejected() ? 1 : 0,
                     (long long)fit.n_correspondences, (long long)fit.n_points, (long long)mapper->activeSubmap().size(), fit.fitness, fit.inlier_rmse);
        for (int i = 0; i < 16; ++i) std::fprintf(out, " %a", mapper->mapToRangeSensor().m[i]);
        std::fprintf(out, "\n");
      } else {
        o3s_scan* scan = col->scanForNextMeasurement();
        std::int64_t n_merge = 0, n_match = 0;
        if (o3s_scan_preprocess(scan, &p.mapBuilderCropper, p.scanVoxelSize, &p.scanMatcherCropper, pts.data(), nrm.data(), N, &n_merge, &n_match) != O3S_OK)
          throw std::runtime_error("o3s_scan_preprocess failed");
        col->insertScan(scan, pose.m, stamp);
        const double fitness = col->lastSwitchFitness();
        for (const auto& fin : col->popFinishedSubmapIds()) col->computeFeatures(fin.first);
        std::fprintf(out, "%lld %zu %zu %d", (long long)k, col->activeSubmapIdx(), col->numSubmaps(), col->lastInsertSwitchedSubmaps() ? 1 : 0);
        for (std::size_t i = 0; i < col->numSubmaps(); ++i) std::fprintf(out, " %lld", (long long)col->submapMap(i).voxelMapSize());
        std::fprintf(out, "  %a\n", fitness);
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(out, "exception %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
