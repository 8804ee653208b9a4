// The assembled map through the compiled headers a catkin package would include (cpp/o3s_submap_collection.hpp, cpp/o3s_mapper.hpp):
// plain g++, only libo3dslam_icp_hip.so at link time.
//
//   assembled_map_case <scans.bin>
// scans.bin (little endian):
//   double  scan_voxel, map_voxel, wide_radius, narrow_radius, assemble_voxel
//   int64   K
//   K x { int64 force_new_submap; double pose[16] (column-major); int64 N; double pts[3N]; double normals[3N] }
// Every scan is pre-processed into the collection's scan object and inserted (SubmapCollectionHip::insertScan); a scan with
// force_new_submap != 0 is preceded by forceNewSubmapCreationAtNextScan().  Then SubmapCollectionHip::assembleMap runs for voxel 0
// and for assemble_voxel into ONE AssembledMapHip.  stdout:
//   submaps <n> total <getTotalNumPoints>
//   plain <size> <has_normals> <has_colors> <fnv64 of the point bytes> <fnv64 of the normal bytes>
//   voxel <size> <has_normals> <has_colors> <fnv64 of the point bytes> <fnv64 of the normal bytes>
//   again <the voxel line's fields once more, from a second build: the same bytes without a new allocation> <device bytes equal: 0 / 1>
#include <cinttypes>
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
    std::fprintf(stderr, "input truncated\n");
    std::exit(2);
  }
  return v;
}

static std::uint64_t fnv64(const std::vector<double>& v) {
  std::uint64_t h = 1469598103934665603ull;
  const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
  for (std::size_t i = 0; i < v.size() * sizeof(double); ++i) {
    h ^= b[i];
    h *= 1099511628211ull;
  }
  return h;
}

static void report(const char* tag, o3s::AssembledMapHip& a, const char* tail = "") {
  const std::size_t n = (std::size_t)a.size();
  std::vector<double> p(3 * n), q(a.hasNormals() ? 3 * n : 0);
  a.download(p.data(), a.hasNormals() ? q.data() : nullptr, nullptr);
  std::printf("%s %zu %d %d %016" PRIx64 " %016" PRIx64 "%s\n", tag, n, (int)a.hasNormals(), (int)a.hasColors(), fnv64(p), fnv64(q), tail);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  const double scanVoxel = rd<double>(f), mapVoxel = rd<double>(f), wideR = rd<double>(f), narrowR = rd<double>(f), assembleVoxel = rd<double>(f);
  const std::int64_t K = rd<std::int64_t>(f);
  try {
    o3s_cropper wide{}, narrow{};
    wide.kind = narrow.kind = 1;  // MaxRadius
    wide.p0 = wideR;
    narrow.p0 = narrowR;
    o3s::SubmapParams sp;
    sp.radius = 1.0e9;  // nothing switches by itself
    sp.minNumRangeData = 1000000;
    sp.maxNumPoints = 1000000000000ll;
    sp.numScansOverlap = 1;
    o3s::SubmapCollectionHip col(sp, mapVoxel, wide, false, 0);
    for (std::int64_t k = 0; k < K; ++k) {
      const std::int64_t force = rd<std::int64_t>(f);
      double T[16];
      for (double& v : T) v = rd<double>(f);
      const std::int64_t N = rd<std::int64_t>(f);
      std::vector<double> pts(3 * (std::size_t)N), nrm(3 * (std::size_t)N);
      f.read(reinterpret_cast<char*>(pts.data()), (std::streamsize)(pts.size() * sizeof(double)));
      f.read(reinterpret_cast<char*>(nrm.data()), (std::streamsize)(nrm.size() * sizeof(double)));
      if (!f) return 2;
      if (force) col.forceNewSubmapCreationAtNextScan();
      o3s_scan* sc = col.scanForNextMeasurement();
      std::int64_t nMerge = 0, nMatch = 0;
      if (o3s_scan_preprocess(sc, &wide, scanVoxel, &narrow, pts.data(), nrm.data(), N, &nMerge, &nMatch) != O3S_OK) return 3;
      col.insertScan(sc, T, 0.1 * (double)k);
    }
    std::printf("submaps %zu total %zu\n", col.numSubmaps(), col.getTotalNumPoints());
    o3s::AssembledMapHip map(0);
    col.assembleMap(map, 0.0);
    report("plain", map);
    col.assembleMap(map, assembleVoxel);
    report("voxel", map);
    const std::int64_t held = map.deviceBytes();
    col.assembleMap(map, assembleVoxel, O3S_ASSEMBLE_NORMALS);
    report("again", map, map.deviceBytes() == held ? " 1" : " 0");
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  return 0;
}
