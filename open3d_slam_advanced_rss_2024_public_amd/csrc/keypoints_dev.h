// keypoints_dev.h — Open3D's geometry::keypoint::ComputeISSKeypoints on device arrays (part of the cloud_ops.hip translation unit;
// Open3D v0.15.1, geometry/Keypoint.cpp; Zhong 2009).  The contract is restated in include/keypoints/o3s_keypoints.h.
// The neighbour search is the radius filter's (outlier_dev.h: grid over the finite points with cell >= the larger radius, the
// 3 x 3 x 3 block as nine runs); the cloud's resolution comes from the normals' ring search with k = 2 and the statistical filter's
// fixed-order sum.  fp64 throughout, no FMA contraction, no floating-point atomics.
#pragma once
#include "outlier_dev.h"

namespace {
namespace o3s_cloud {

constexpr int kIssMaxSweeps = 16;  // the Jacobi's bound (it converges quadratically: a 3 x 3 needs 4-6)

// one Jacobi rotation of the pair (p, q) of a symmetric 3 x 3; r is the third index (the rotation of localizability_dev.h
// without the eigenvectors nobody reads here)
__device__ __forceinline__ void iss_rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
  if (!(apq != 0.0)) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double at = fabs(theta) + sqrt(theta * theta + 1.0);
  const double t = theta < 0.0 ? -1.0 / at : 1.0 / at;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
}

// eigenvalues l1 >= l2 >= l3 of a finite symmetric 3 x 3 by cyclic Jacobi.  Not the closed form of the normals (fast_eigen3x3):
// its smallest eigenvalue carries an absolute error of order eps * l1, and the smallest eigenvalue is what is ranked here.
__device__ __forceinline__ void iss_eigvals3(double a00, double a01, double a02, double a11, double a12, double a22, double& l1, double& l2, double& l3) {
  for (int sweep = 0; sweep < kIssMaxSweeps; ++sweep) {
    const double off = (fabs(a01) + fabs(a02)) + fabs(a12);
    const double diag = (fabs(a00) + fabs(a11)) + fabs(a22);
    if (!(off > 8.470329472543003e-22 /*2^-70*/ * diag)) break;  // (a NaN ends the loop as well)
    iss_rotate(a00, a11, a01, a02, a12);  // (0, 1), third index 2
    iss_rotate(a00, a22, a02, a01, a12);  // (0, 2), third index 1
    iss_rotate(a11, a22, a12, a01, a02);  // (1, 2), third index 0
  }
  double t;
  if (a00 < a11) t = a00, a00 = a11, a11 = t;
  if (a11 < a22) t = a11, a11 = a22, a22 = t;
  if (a00 < a11) t = a00, a00 = a11, a11 = t;
  l1 = a00, l2 = a11, l3 = a22;
}

// Resolution, step 1: d[input index] = sqrt(d2 to the nearest other finite point) by the exact 2-nearest search (the query finds
// itself at 0, or two coincident points in its place: the second entry is the nearest other point either way).  d starts at -1
// (k_or_finite): the statistical filter's sums then count the finite points and add their distances (k_or_stats_part<1>).
__global__ void __launch_bounds__(kB) k_iss_nn_dist(const double* __restrict__ sp, const uint32_t* __restrict__ vals, int64_t N, NGrid g,
                                                    const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend,
                                                    const uint32_t* __restrict__ fmap /*nullable: identity*/, double* __restrict__ d) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= N) return;
  const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
  double D[2];
  int32_t J[2];
  knn_grid_search<2>(sp, vals, qx, qy, qz, g, cbeg, cend, 2, __builtin_huge_val(), D, J);
  const uint32_t f = vals[t];
  d[fmap ? fmap[f] : f] = sqrt(D[1]);  // N >= 2: the second entry exists
}

// Saliency.  One query per lane in cell-sorted order; the whole block at salient^2, no early exit: the count and the six sums of
// the scatter matrix about the query, in the walk's order — the same order for two coincident queries, since they share the cell,
// the runs and every distance.  Then the eigenvalues and the two ratio tests.  sal_s[t] lies beside the cell-sorted coordinates
// for k_iss_nms; sal_in[input index] is what the caller sees (zeroed beforehand: non-finite points stay 0).
__global__ void __launch_bounds__(kB) k_iss_scatter(const double* __restrict__ sp, const uint32_t* __restrict__ vals, int64_t N, NGrid g,
                                                    const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend, int min_nb, double r2, double gamma_21,
                                                    double gamma_32, const uint32_t* __restrict__ fmap /*nullable: identity*/, double* __restrict__ sal_s,
                                                    double* __restrict__ sal_in) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= N) return;
  const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
  uint32_t lo[9], hi[9];
  block_runs(qx, qy, qz, g, cbeg, cend, lo, hi);
  int count = 0;
  double sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  walk_block(
      sp, lo, hi, qx, qy, qz, r2,
      [&](uint32_t j0, uint32_t m) {
        count += __popc(m);
        double dx[kWalkBatch], dy[kWalkBatch], dz[kWalkBatch];
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u) {  // the batch's hits again (they are in cache), as independent loads
          const bool on = (m >> u) & 1u;
          const size_t j = on ? (size_t)(j0 + (uint32_t)u) : (size_t)t;
          dx[u] = sp[3 * j] - qx;
          dy[u] = sp[3 * j + 1] - qy;
          dz[u] = sp[3 * j + 2] - qz;
        }
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u)
          if ((m >> u) & 1u) {
            sxx += dx[u] * dx[u];
            sxy += dx[u] * dy[u];
            sxz += dx[u] * dz[u];
            syy += dy[u] * dy[u];
            syz += dy[u] * dz[u];
            szz += dz[u] * dz[u];
          }
      },
      [&]() { return false; });
  double sal = 0.0;
  const bool zero = sxx == 0.0 && sxy == 0.0 && sxz == 0.0 && syy == 0.0 && syz == 0.0 && szz == 0.0;
  if (count >= min_nb && !zero) {
    double l1, l2, l3;
    iss_eigvals3(sxx, sxy, sxz, syy, syz, szz, l1, l2, l3);
    if (l2 / l1 < gamma_21 && l3 / l2 < gamma_32) sal = l3;
  }
  sal_s[t] = sal;
  const uint32_t f = vals[t];
  sal_in[fmap ? fmap[f] : f] = sal;
}

// Non-maximum suppression.  One query per lane in cell-sorted order: a point with sal > 0 walks the block at non_max^2, counts,
// and compares its saliency with every neighbour's; the walk ends at the first larger one.  keep[input index] = 1 for a keypoint
// (the array is zeroed beforehand: non-finite points stay 0).
__global__ void __launch_bounds__(kB) k_iss_nms(const double* __restrict__ sp, const uint32_t* __restrict__ vals, int64_t N, NGrid g,
                                                const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend, int min_nb, double r2,
                                                const double* __restrict__ sal_s, const uint32_t* __restrict__ fmap /*nullable: identity*/,
                                                uint32_t* __restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (t >= N) return;
  const double mine = sal_s[t];
  if (!(mine > 0.0)) return;
  const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
  uint32_t lo[9], hi[9];
  block_runs(qx, qy, qz, g, cbeg, cend, lo, hi);
  int count = 0;
  bool larger = false;
  walk_block(
      sp, lo, hi, qx, qy, qz, r2,
      [&](uint32_t j0, uint32_t m) {
        count += __popc(m);
        double v[kWalkBatch];
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u) v[u] = (m >> u) & 1u ? sal_s[j0 + (uint32_t)u] : 0.0;
#pragma unroll
        for (int u = 0; u < kWalkBatch; ++u) larger = larger || v[u] > mine;
      },
      [&]() { return larger; });
  if (larger || count < min_nb) return;
  const uint32_t f = vals[t];
  keep[fmap ? fmap[f] : f] = 1u;
}

// The feature set restricted to the kept sparse points idx[0 .. n_keep), ascending: 39 doubles per point — 3 coordinates, 3 normal
// components, the 33 of the FPFH column — one per thread, so a column's loads are one batch of a wave and every store is coalesced.
constexpr int kIssRow = 3 + 3 + 33;
__global__ void __launch_bounds__(kB) k_iss_gather_feat(const int64_t* __restrict__ idx, int64_t n_keep, const double* __restrict__ p, const double* __restrict__ n,
                                                        const double* __restrict__ f, double* __restrict__ out_p, double* __restrict__ out_n,
                                                        double* __restrict__ out_f) {
  const int64_t e = (int64_t)blockIdx.x * kB + threadIdx.x;
  if (e >= n_keep * kIssRow) return;
  const int64_t o = e / kIssRow;
  const int c = (int)(e - o * kIssRow);
  const int64_t i = idx[o];
  if (c < 3) out_p[3 * o + c] = p[3 * i + c];
  else if (c < 6) out_n[3 * o + (c - 3)] = n[3 * i + (c - 3)];
  else out_f[33 * o + (c - 6)] = f[33 * i + (c - 6)];
}

// work area of one keypoint call over n points (the grid index has its own: NormalsWork)
struct IssArea {
  static constexpr size_t kSlack = 4096;
  unsigned long long* d_bb;
  uint32_t *fin, *keep, *off, *fmap, *part_cnt;
  double *fpts, *nn, *part, *stats, *sal_s, *sal_in;
  char* tmp;
  template <class A>
  void lay(A& a, size_t n, size_t tb_scan) {
    take(a, d_bb, kBoundsWords);
    take(a, fin, n);
    take(a, keep, n);
    take(a, off, n + 1);
    take(a, fmap, n);
    take(a, fpts, n * 3);
    take(a, nn, n);
    take(a, part, kOrMaxParts);
    take(a, part_cnt, kOrMaxParts);
    take(a, stats, 4);
    take(a, sal_s, n);
    take(a, sal_in, n);
    take(a, tmp, tb_scan);
  }
};

struct IssWork {  // grow-only, leased per call from the device's pool
  NormalsWork grid;
  Arena arena;
  DevMem out_p, out_n, out_i, out_f;  // where the entries compact to: the host-array one copies out, the resident one swaps
};

struct IssResult {
  const uint32_t *keep, *off;  // keypoint flags of the N input points and their exclusive scan (off[N] = n_keep), in the work area
  int64_t n_keep;
  const double* sal;  // N saliencies by input index (device)
  double radii[2];    // the salient and the non-max radius used
};

// ISS keypoints of d_pts (3 x N doubles on the device, N > 0, parameters checked by the caller).  Returns with the flags, their
// scan and the saliencies in the work area and the count on the host; the caller compacts what rides along.
inline int iss_flags_dev(IssWork& w, double salient, double non_max, double gamma_21, double gamma_32, int min_nb, const double* d_pts, int64_t N, IssResult* out,
                         hipStream_t s) {
  if (N <= 0 || N > (int64_t)0x7fffffff) return O3S_ERR_BAD_ARGUMENT;
  const bool from_res = salient == 0.0 || non_max == 0.0;
  const size_t tb = scan_temp_bytes(N);
  IssArea a;
  CK(lay_out(w.arena, a, (size_t)N, tb));
  uint32_t* blk = reinterpret_cast<uint32_t*>(a.tmp);
  out->keep = a.keep;
  out->off = a.off;
  out->n_keep = 0;
  out->sal = a.sal_in;
  // the finite points: the grids are built over them alone
  hipLaunchKernelGGL(k_or_finite, dim3(nblk(N)), dim3(kB), 0, s, d_pts, N, a.fin, blk, from_res ? a.nn : (double*)nullptr);
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
  CK(hipMemsetAsync(a.keep, 0, (size_t)N * 4, s));
  CK(hipMemsetAsync(a.sal_in, 0, (size_t)N * 8, s));
  if (from_res) {
    double res = 0.0;
    if (Nf >= 2) {
      // no radius to size the cell by: the statistical filter's first guess (outlier_flags_dev), re-sized once by the build to
      // about four points per occupied cell
      unsigned long long bb[6];
      rc = cloud_bounds(FlatPoints{fp}, Nf, a.d_bb, s, bb);
      if (rc != O3S_OK) return rc;
      double ext = 0.0;
      for (int k = 0; k < 3; ++k) ext = std::max(ext, from_ordered_bits(bb[3 + k]) - from_ordered_bits(bb[k]));
      const double rho = 4.0;
      GridIndex gi;
      rc = build_grid_index(w.grid, fp, Nf, ext * std::sqrt(rho / (double)Nf), rho, std::numeric_limits<double>::max(), &gi, s, bb, /*keep_cell=*/false,
                            outlier_max_cells());
      if (rc != O3S_OK) return rc;
      hipLaunchKernelGGL(k_iss_nn_dist, dim3(nblk(Nf)), dim3(kB), 0, s, gi.sp, gi.vals, Nf, gi.g, gi.cbeg, gi.cend, fmap, a.nn);
      const int n_part = (int)std::min<unsigned>(nblk(N), (unsigned)kOrMaxParts);
      hipLaunchKernelGGL(k_or_stats_part<1>, dim3(n_part), dim3(kB), 0, s, a.nn, N, a.stats, a.part, a.part_cnt);
      hipLaunchKernelGGL(k_or_stats_fold<1>, dim3(1), dim3(kB), 0, s, a.part, a.part_cnt, n_part, 0.0, a.stats);
      CK(hipGetLastError());
      double st[4];
      CK(hipMemcpyAsync(st, a.stats, 32, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      res = st[0];  // (sum of the distances) / (number of finite points)
    }
    salient = 6.0 * res;
    non_max = 4.0 * res;
  }
  out->radii[0] = salient;
  out->radii[1] = non_max;
  const double rmax = std::max(salient, non_max);
  if (Nf > 0 && rmax > 0.0 && std::isfinite(rmax)) {
    // cell = the larger radius, a hair above (see outlier_flags_dev): every neighbour of either search lies in the 3 x 3 x 3 block,
    // also when the build made the cell coarser
    GridIndex gi;
    rc = build_grid_index(w.grid, fp, Nf, rmax * (1.0 + 1e-6), 0.0, 0.0, &gi, s, nullptr, /*keep_cell=*/true, outlier_max_cells());
    if (rc != O3S_OK) return rc;
    const dim3 gr(nblk(Nf)), bl(kB);
    hipLaunchKernelGGL(k_iss_scatter, gr, bl, 0, s, gi.sp, gi.vals, Nf, gi.g, gi.cbeg, gi.cend, min_nb, salient * salient, gamma_21, gamma_32, fmap, a.sal_s, a.sal_in);
    hipLaunchKernelGGL(k_iss_nms, gr, bl, 0, s, gi.sp, gi.vals, Nf, gi.g, gi.cbeg, gi.cend, min_nb, non_max * non_max, (const double*)a.sal_s, fmap, a.keep);
    CK(hipGetLastError());
  }
  return scan_flags(a.keep, a.off, N, a.tmp, tb, &out->n_keep, s);
}

}  // namespace o3s_cloud
}  // namespace
