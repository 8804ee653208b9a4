// outlier_dev.h — Open3D's two outlier filters on device arrays (part of the cloud_ops.hip translation unit):
//   PointCloud::RemoveRadiusOutliers(nb_points, search_radius), PointCloud::RemoveStatisticalOutliers(nb_neighbors, std_ratio)
// (Open3D v0.15.1, geometry/PointCloud.cpp; the contract is restated in include/outlier_removal/o3s_outlier_removal.h).  The kd-tree
// is replaced by the grid index of normals_dev.h — the same bounds, keys, cell-sorted copy and per-cell ranges — so the neighbour
// sets are exact for any cell size.  fp64 throughout, no FMA contraction, no floating-point atomics.
#pragma once
#include "normals_dev.h"

namespace {
namespace o3s_cloud {

constexpr int kOrMaxParts = 1024;  // blocks of the two cloud-wide sums (they stride over the cloud)

__device__ __forceinline__ bool finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// flag = 1 for a point whose three coordinates are finite (the points the grid is built over), with the per-block counts for the
// one-launch scan; avg (nullable, statistical) starts at -1 = "no neighbours"
__global__ void __launch_bounds__(kB) k_or_finite(const double* __restrict__ pts, int64_t N, uint32_t* __restrict__ flag, uint32_t* __restrict__ blk_cnt,
                                                  double* __restrict__ avg) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  uint32_t f = 0u;
  if (i < N) {
    f = finite3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]) ? 1u : 0u;
    flag[i] = f;
    if (avg) avg[i] = -1.0;
  }
  put_block_count(f, blk_cnt);
}

// finite-subset ordinal -> input index
__global__ void __launch_bounds__(kB) k_or_fmap(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off, int64_t N, uint32_t* __restrict__ fmap) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i < N && flag[i]) fmap[off[i]] = (uint32_t)i;
}

// The 3 x 3 x 3 block of cells around the point (qx, qy, qz) as nine runs of the cell-sorted copy: the three cells of a row are
// consecutive keys, so their points are one run.  The 27 cell headers go out as one batch of independent loads.  The cell is
// found by the expression that built the keys (k_grid_keys).  Row 4 is the query's own row.
__device__ __forceinline__ void block_runs(double qx, double qy, double qz, const NGrid& g, const uint32_t* __restrict__ cbeg,
                                           const uint32_t* __restrict__ cend, uint32_t (&lo)[9], uint32_t (&hi)[9]) {
  const int cx = (int)floor((qx - g.ox) / g.cell), cy = (int)floor((qy - g.oy) / g.cell), cz = (int)floor((qz - g.oz) / g.cell);
  uint32_t cb[27], ce[27];
#pragma unroll
  for (int u = 0; u < 27; ++u) {
    const int z = cz + u / 9 - 1, y = cy + (u / 3) % 3 - 1, x = cx + u % 3 - 1;
    const bool in = z >= 0 && z < g.nz && y >= 0 && y < g.ny && x >= 0 && x < g.nx;
    const size_t c = in ? ((size_t)z * (size_t)g.ny + (size_t)y) * (size_t)g.nx + (size_t)x : 0;
    const uint32_t b0 = cbeg[c], e0 = cend[c];
    cb[u] = in ? b0 : 0u;
    ce[u] = in ? e0 : 0u;
  }
#pragma unroll
  for (int row = 0; row < 9; ++row) {
    uint32_t l = 0xffffffffu, h = 0u;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int q = row * 3 + u;
      if (ce[q] > cb[q]) {  // empty cells carry begin = end = 0
        l = min(l, cb[q]);
        h = max(h, ce[q]);
      }
    }
    lo[row] = h > l ? l : 0u;
    hi[row] = h > l ? h : 0u;
  }
}

// The walk over those runs, the own row first (it holds the query itself and its nearest neighbours), in batches of kWalkBatch
// candidates whose loads go out together: hits(j0, m) for every batch with a candidate at d2 < r2 — bit u of m: candidate j0 + u
// (an index into the cell-sorted copy) passed; done() is asked before every batch and ends the walk.
constexpr int kWalkBatch = 8;
template <class Hits, class Done>
__device__ __forceinline__ void walk_block(const double* __restrict__ sp, const uint32_t (&lo)[9], const uint32_t (&hi)[9], double qx, double qy, double qz,
                                           double r2, Hits hits, Done done) {
  constexpr int kNb = kWalkBatch;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int row = k == 0 ? 4 : (k <= 4 ? k - 1 : k);
    const uint32_t jb = lo[row], je = hi[row];
    for (uint32_t j0 = jb; j0 < je && !done(); j0 += kNb) {
      double px[kNb], py[kNb], pz[kNb];
#pragma unroll
      for (int u = 0; u < kNb; ++u) {
        const size_t j = (size_t)min(j0 + (uint32_t)u, je - 1u);
        px[u] = sp[3 * j];
        py[u] = sp[3 * j + 1];
        pz[u] = sp[3 * j + 2];
      }
      uint32_t m = 0u;
#pragma unroll
      for (int u = 0; u < kNb; ++u)
        if (j0 + (uint32_t)u < je && dist2(qx, qy, qz, px[u], py[u], pz[u]) < r2) m |= 1u << u;
      if (m) hits(j0, m);
    }
  }
}

// Radius filter.  The grid's cell edge is at least the radius, so every point at d2 < r2 lies in the 3 x 3 x 3 block around the
// query's cell.  One query per lane (cell-sorted order: neighbouring lanes walk the same cells).  A lane stops at the first batch
// that takes its count above nb: in a dense map (0.1 m voxels, 0.5 m radius) that is after a few dozen candidates of the several
// hundred in the block.  keep[input index] = count > nb (the array is zeroed beforehand: non-finite points stay 0).
__global__ void __launch_bounds__(kB) k_or_count(const double* __restrict__ sp, const uint32_t* __restrict__ vals, int64_t N, NGrid g,
                                                 const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend, int nb, double r2,
                                                 const uint32_t* __restrict__ fmap /*nullable: identity*/, uint32_t* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= N) return;
  const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
  uint32_t lo[9], hi[9];
  block_runs(qx, qy, qz, g, cbeg, cend, lo, hi);
  int count = 0;
  walk_block(sp, lo, hi, qx, qy, qz, r2, [&](uint32_t, uint32_t m) { count += __popc(m); }, [&]() { return count > nb; });
  const uint32_t f = vals[t];
  keep[fmap ? fmap[f] : f] = count > nb ? 1u : 0u;
}

// Statistical filter, step 1: the exact nb nearest points by the ring search the normals use (no radius cut: r2 = +inf, so a far,
// isolated point walks rings to the grid's extent), then avg = (sum of sqrt(d2), ascending) / k into avg[input index].
template <int K>
__global__ void __launch_bounds__(kB) k_or_knn_mean(const double* __restrict__ sp, const uint32_t* __restrict__ vals, int64_t N, NGrid g,
                                                    const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend, int nb,
                                                    const uint32_t* __restrict__ fmap /*nullable: identity*/, double* __restrict__ avg) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= N) return;
  const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
  double D[K];
  int32_t J[K];
  knn_grid_search<K>(sp, vals, qx, qy, qz, g, cbeg, cend, nb, __builtin_huge_val(), D, J);
  int k = 0;
  double sum = 0.0;
#pragma unroll
  for (int s = 0; s < K; ++s)
    if (s < nb && J[s] != 0x7fffffff) {
      sum += sqrt(D[s]);
      k = s + 1;
    }
  const uint32_t f = vals[t];
  avg[fmap ? fmap[f] : f] = sum / (double)k;  // k >= 1: the query finds itself
}

// fixed-order sum of a block's kB values (a tree over LDS: halves first); the total is thread 0's
__device__ __forceinline__ double block_sum_fixed(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int m = kB / 2; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m) sh[threadIdx.x] += sh[threadIdx.x + m];
    __syncthreads();
  }
  return sh[0];
}

// Statistical filter, step 2: the two cloud-wide sums.  kPass 1: valid = #{avg >= 0} and the sum of the avg > 0; kPass 2: the sum
// of (avg - mean)^2 over the avg > 0.  Every block strides over the cloud and leaves one fp64 partial (and one count); the grid
// depends on N alone.
template <int kPass>
__global__ void __launch_bounds__(kB) k_or_stats_part(const double* __restrict__ avg, int64_t N, const double* __restrict__ stats, double* __restrict__ part,
                                                      uint32_t* __restrict__ part_cnt) {
  __shared__ double sh[kB];
  const double mean = kPass == 2 ? stats[0] : 0.0;
  double acc = 0.0;
  uint32_t cnt = 0u;
  for (int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x; i < N; i += (int64_t)gridDim.x * kB) {
    const double a = avg[i];
    if (kPass == 1) {
      if (a >= 0.0) ++cnt;
      if (a > 0.0) acc += a;
    } else if (a > 0.0) {
      const double d = a - mean;
      acc += d * d;
    }
  }
  const double tot = block_sum_fixed(acc, sh);
  if (kPass == 1) {
    __shared__ uint32_t sc[kB / 64];
    const uint32_t w = wave_sum_u32(cnt);
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t n = 0u;
      for (int k = 0; k < kB / 64; ++k) n += sc[k];
      part_cnt[blockIdx.x] = n;
    }
  }
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// ... folded in block order by one block (thread 0 adds the partials as they lie in LDS).  kPass 1 leaves stats[0] = mean and
// stats[3] = valid; kPass 2 leaves stats[1] = std and stats[2] = thr = mean + ratio * std, where k_or_mask reads it: no host trip.
template <int kPass>
__global__ void __launch_bounds__(kB) k_or_stats_fold(const double* __restrict__ part, const uint32_t* __restrict__ part_cnt, int n_part, double ratio,
                                                      double* __restrict__ stats) {
  __shared__ double sh[kOrMaxParts];
  __shared__ uint32_t sc[kOrMaxParts];
  if (blockIdx.x != 0) return;
  for (int k = threadIdx.x; k < n_part; k += kB) {
    sh[k] = part[k];
    sc[k] = kPass == 1 ? part_cnt[k] : 0u;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  uint64_t cnt = 0;
  for (int k = 0; k < n_part; ++k) {
    sum += sh[k];
    cnt += sc[k];
  }
  if (kPass == 1) {
    stats[0] = sum / (double)cnt;
    stats[3] = (double)cnt;
  } else {
    const double sd = sqrt(sum / (stats[3] - 1.0));
    stats[1] = sd;
    stats[2] = stats[0] + ratio * sd;
  }
}

// Statistical filter, step 3: keep = avg > 0 && avg < thr (a NaN threshold keeps nothing), with the per-block counts for the scan
__global__ void __launch_bounds__(kB) k_or_mask(const double* __restrict__ avg, int64_t N, const double* __restrict__ stats, uint32_t* __restrict__ keep,
                                                uint32_t* __restrict__ blk_cnt) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  uint32_t f = 0u;
  if (i < N) {
    const double a = avg[i], thr = stats[2];
    f = (a > 0.0 && a < thr) ? 1u : 0u;
    keep[i] = f;
  }
  put_block_count(f, blk_cnt);
}

// the kept input indices, ascending
__global__ void __launch_bounds__(kB) k_or_kept_idx(const uint32_t* __restrict__ keep, const uint32_t* __restrict__ off, int64_t N, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (i < N && keep[i]) out[off[i]] = i;
}

// work area of one filter call over n points (the grid index has its own: NormalsWork)
struct OutlierArea {
  static constexpr size_t kSlack = 4096;
  unsigned long long* d_bb;
  uint32_t *fin, *keep, *off, *fmap, *part_cnt;
  double *fpts, *avg, *part, *stats;
  char* tmp;
  template <class A>
  void lay(A& a, size_t n, size_t tb_scan, bool statistical) {
    take(a, d_bb, kBoundsWords);
    take(a, fin, n);
    take(a, keep, n);
    take(a, off, n + 1);
    take(a, fmap, n);
    take(a, fpts, n * 3);
    take(a, avg, statistical ? n : 0);
    take(a, part, kOrMaxParts);
    take(a, part_cnt, kOrMaxParts);
    take(a, stats, 4);
    take(a, tmp, tb_scan);
  }
};

struct OutlierWork {  // grow-only, leased per call from the device's pool
  NormalsWork grid;
  Arena arena;
  DevMem out_p, out_n, out_i;  // where the host-array entry compacts to before it copies out
};

struct OutlierResult {
  const uint32_t *keep, *off;  // keep flags of the N input points and their exclusive scan (off[N] = n_keep), in the work area
  int64_t n_keep;
  const double* avg;    // statistical: N averages (device); radius: null
  double stats[4];      // statistical: mean, std, thr, valid
};

// the cap on the grid's dense cell arrays: a constant in the product; the hooks build reads it per call (the coarser-cell path at test sizes)
inline size_t outlier_max_cells() {
  if (const char* e = O3S_HOOK_ENV("O3S_OR_MAX_CELLS")) {
    const long long v = atoll(e);
    if (v >= 8) return (size_t)v;
  }
  return kGridMaxCells;
}

// kind 1 / 2 of o3s_outlier_params on d_pts (3 x N doubles on the device, N > 0, parameters checked by the caller).  Returns with
// the flags and their scan in the work area and the count on the host; the caller compacts what rides along.
inline int outlier_flags_dev(OutlierWork& w, int kind, int nb, double value, const double* d_pts, int64_t N, OutlierResult* out, hipStream_t s) {
  if (N <= 0 || N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  const bool stat = kind == 2;
  const size_t tb = scan_temp_bytes(N);
  OutlierArea a;
  CK(lay_out(w.arena, a, (size_t)N, tb, stat));
  uint32_t* blk = reinterpret_cast<uint32_t*>(a.tmp);
  out->keep = a.keep;
  out->off = a.off;
  out->n_keep = 0;
  out->avg = stat ? a.avg : nullptr;
  for (int k = 0; k < 4; ++k) out->stats[k] = 0.0;
  // the finite points: the grid is built over them alone
  hipLaunchKernelGGL(k_or_finite, dim3(nblk(N)), dim3(kB), 0, s, d_pts, N, a.fin, blk, stat ? a.avg : (double*)nullptr);
  int64_t Nf = 0;
  int rc = scan_flags(a.fin, a.off, N, a.tmp, tb, &Nf, s, blk);
  if (rc != O3S_OK) return rc;
  const double* fp = d_pts;
  const uint32_t* fmap = nullptr;
  if (Nf < N && Nf > 0) {
    hipLaunchKernelGGL(k_compact, dim3(nblk(N)), dim3(kB), 0, s, d_pts, (const double*)nullptr, N, a.fin, a.off, a.fpts, (double*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(k_or_fmap, dim3(nblk(N)), dim3(kB), 0, s, a.fin, a.off, N, a.fmap);
    fp = a.fpts;
    fmap = a.fmap;
  }
  if (!stat) CK(hipMemsetAsync(a.keep, 0, (size_t)N * 4, s));
  if (Nf > 0) {
    GridIndex gi;
    if (!stat) {
      // cell = the radius, a hair above: floor((p - o) / cell) of two points closer than the radius then differs by one at most,
      // whatever the division rounds to.  The build only ever makes the cell coarser (extent / 512, the cap on the cell arrays).
      rc = build_grid_index(w.grid, fp, Nf, value * (1.0 + 1e-6), 0.0, 0.0, &gi, s, nullptr, /*keep_cell=*/true, outlier_max_cells());
      if (rc != O3S_OK) return rc;
      hipLaunchKernelGGL(k_or_count, dim3(nblk(Nf)), dim3(kB), 0, s, gi.sp, gi.vals, Nf, gi.g, gi.cbeg, gi.cend, nb, value * value, fmap, a.keep);
    } else {
      // no radius to size the cell by: a first guess from the bounds and the count — a surface-like cloud of extent e has about
      // rho points per cell at e sqrt(rho / Nf) — which the build then re-sizes once from the occupancy it measures, to
      // rho = 0.8 nb points per occupied cell (between 4 and 12), as the normals' search has it
      unsigned long long bb[6];
      rc = cloud_bounds(FlatPoints{fp}, Nf, a.d_bb, s, bb);
      if (rc != O3S_OK) return rc;
      double ext = 0.0;
      for (int k = 0; k < 3; ++k) ext = std::max(ext, from_ordered_bits(bb[3 + k]) - from_ordered_bits(bb[k]));
      const double rho = std::min(12.0, std::max(4.0, 0.8 * (double)nb));
      const double cell0 = ext * std::sqrt(rho / (double)Nf);
      rc = build_grid_index(w.grid, fp, Nf, cell0, rho, std::numeric_limits<double>::max(), &gi, s, bb, /*keep_cell=*/false, outlier_max_cells());
      if (rc != O3S_OK) return rc;
#define O3S_OR_LAUNCH(KK) \
  hipLaunchKernelGGL(k_or_knn_mean<KK>, dim3(nblk(Nf)), dim3(kB), 0, s, gi.sp, gi.vals, Nf, gi.g, gi.cbeg, gi.cend, nb, fmap, a.avg)
      if (nb <= 8) O3S_OR_LAUNCH(8);
      else if (nb <= 16) O3S_OR_LAUNCH(16);
      else if (nb <= 24) O3S_OR_LAUNCH(24);
      else O3S_OR_LAUNCH(32);
#undef O3S_OR_LAUNCH
    }
    CK(hipGetLastError());
  }
  if (stat) {
    const int n_part = (int)std::min<unsigned>(nblk(N), (unsigned)kOrMaxParts);
    hipLaunchKernelGGL(k_or_stats_part<1>, dim3(n_part), dim3(kB), 0, s, a.avg, N, a.stats, a.part, a.part_cnt);
    hipLaunchKernelGGL(k_or_stats_fold<1>, dim3(1), dim3(kB), 0, s, a.part, a.part_cnt, n_part, value, a.stats);
    hipLaunchKernelGGL(k_or_stats_part<2>, dim3(n_part), dim3(kB), 0, s, a.avg, N, a.stats, a.part, a.part_cnt);
    hipLaunchKernelGGL(k_or_stats_fold<2>, dim3(1), dim3(kB), 0, s, a.part, a.part_cnt, n_part, value, a.stats);
    hipLaunchKernelGGL(k_or_mask, dim3(nblk(N)), dim3(kB), 0, s, a.avg, N, a.stats, a.keep, blk);
    CK(hipGetLastError());
    rc = scan_flags(a.keep, a.off, N, a.tmp, tb, &out->n_keep, s, blk);
    if (rc != O3S_OK) return rc;
    CK(hipMemcpyAsync(out->stats, a.stats, 32, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
  } else {
    rc = scan_flags(a.keep, a.off, N, a.tmp, tb, &out->n_keep, s);
    if (rc != O3S_OK) return rc;
  }
  return O3S_OK;
}

}  // namespace o3s_cloud
}  // namespace
