// plane_segmentation_case.cpp — plane segmentation as COMPILED host code: SubmapHip::segmentPlanes / removePlanes and the free
// functions of cpp/o3s_icp.hpp, plain g++, linking only the C-ABI library.  tests/test_gpu_plane_segmentation_cpp.py writes the
// case and compares what is printed here with the Python path over the same library: integers exactly, doubles bit for bit.
//
// argv[1]: the case — int64 N, seed, num_iterations, ransac_n, max_planes, min_inliers; doubles distance_threshold, confidence,
// map voxel size, cropper radius; points (3 x N doubles), normals (3 x N).  The cloud is uploaded as the submap's map.
// Output: "size n"; "host_one best est_k evaluated n_inliers" + 4 x %a; "host_peel n_planes" + a count and 4 x %a per plane;
// "submap_peel n_planes checksum" (sum of (label + 2) * (index + 1)) + a count and 4 x %a per plane; "removed n size n";
// "first" / "last" + 6 x %a (point and normal of the first and last survivor).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "o3s_icp.hpp"

namespace {
template <class T>
bool rd(std::FILE* f, T* p, std::size_t n) {
  return std::fread(p, sizeof(T), n, f) == n;
}
void row(const char* tag, const double* v, int n) {
  std::printf("%s", tag);
  for (int k = 0; k < n; ++k) std::printf(" %a", v[k]);
  std::printf("\n");
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::int64_t q[6];
  double d[4];
  if (!rd(f, q, 6) || !rd(f, d, 4)) return 2;
  const std::int64_t N = q[0];
  std::vector<double> pts((std::size_t)N * 3), nrm((std::size_t)N * 3);
  if (!rd(f, pts.data(), pts.size()) || !rd(f, nrm.data(), nrm.size())) return 2;
  std::fclose(f);
  try {
    o3s_plane_params p;
    o3s_plane_default_params(&p);
    p.distance_threshold = d[0];
    p.confidence = d[1];
    p.seed = (std::uint64_t)q[1];
    p.num_iterations = (std::int32_t)q[2];
    p.ransac_n = (std::int32_t)q[3];
    p.max_planes = (std::int32_t)q[4];
    p.min_inliers = (std::int32_t)q[5];
    o3s_cropper c{};
    c.kind = 1;
    c.p0 = d[3];
    o3s::SubmapHip sm(d[2], c, 0);
    if (o3s_submap_upload(sm.handle(), pts.data(), nrm.data(), N) != O3S_OK) return 3;
    std::printf("size %lld\n", (long long)sm.size());

    o3s_plane_params one = p;
    one.max_planes = 1;
    const o3s::PlaneSegmentation r = o3s::segmentPlane(pts.data(), N, one);
    std::printf("host_one %lld %lld %lld %zu", (long long)r.bestIteration, (long long)r.estK, (long long)r.evaluated, r.inliers.size());
    row("", r.model.data(), 4);

    std::vector<std::int32_t> labels;
    std::vector<double> models;
    std::vector<std::int64_t> counts;
    std::int32_t n = o3s::segmentPlanes(pts.data(), N, p, labels, models, &counts);
    std::printf("host_peel %d\n", (int)n);
    for (std::int32_t k = 0; k < n; ++k) {
      std::printf("plane %lld", (long long)counts[(std::size_t)k]);
      row("", models.data() + 4 * k, 4);
    }

    n = sm.segmentPlanes(p, labels, models, &counts);
    long long sum = 0;
    for (std::size_t i = 0; i < labels.size(); ++i) sum += (long long)(labels[i] + 2) * (long long)(i + 1);
    std::printf("submap_peel %d %lld\n", (int)n, sum);
    for (std::int32_t k = 0; k < n; ++k) {
      std::printf("plane %lld", (long long)counts[(std::size_t)k]);
      row("", models.data() + 4 * k, 4);
    }

    const std::int64_t removed = sm.removePlanes(p, &models);
    const std::int64_t left = sm.size();
    std::printf("removed %lld size %lld\n", (long long)removed, (long long)left);
    std::vector<double> op((std::size_t)left * 3), on((std::size_t)left * 3);
    sm.download(op.data(), on.data());
    if (left > 0) {
      const double a[6] = {op[0], op[1], op[2], on[0], on[1], on[2]};
      const std::size_t e = (std::size_t)(left - 1) * 3;
      const double b[6] = {op[e], op[e + 1], op[e + 2], on[e], on[e + 1], on[e + 2]};
      row("first", a, 6);
      row("last", b, 6);
    }
  } catch (const std::exception& e) {
    std::printf("exception %s\n", e.what());
    return 1;
  }
  return 0;
}
