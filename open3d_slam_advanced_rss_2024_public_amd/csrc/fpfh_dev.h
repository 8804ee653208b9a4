// fpfh_dev.h — FPFH features and feature correspondences on device arrays (part of the cloud_ops.hip translation unit).
//
// The front of a loop closure (O3S/src/Submap.cpp:255-275, the head of O3S/src/PlaceRecognition.cpp:81-84):
//     feature = registration::ComputeFPFHFeature(sparse, KDTreeSearchParamHybrid(radius, max_nn));
//     RegistrationRANSACBasedOnFeatureMatching(...)  =  feature correspondences + RANSAC over them (the RANSAC stays on the host)
// Open3D v0.15.1 is not part of the reference tree; the contract is restated in include/o3s_cloud_ops.h (o3s_compute_fpfh) and DESIGN.md 9b, and
// tests/fpfh_ref.py is written from the same text.  fp64 throughout, no FMA contraction.
//
//   k_fpfh_lists     one wave per query: the max_nn (<= 128) nearest points with d2 < radius^2, ascending (d2, index), kept in HBM
//   k_spfh           one wave per point: pair features of the list, three 11-bin histograms counted in LDS, replayed as additions
//   k_fpfh           a lane per (point, group of 11 rows): distance-weighted sum of the neighbours' SPFH in list order
//   k_feat_nn        brute-force 1-NN in feature space, target columns tiled through LDS, one partial winner per target chunk
//   k_feat_nn_fold   folds the chunks' winners (ties to the lower index)
//   k_feat_nn_fwd_multi / k_feat_nn_fwd_fold / k_feat_nn_bwd_multi   the same search of ONE source against up to 16 targets read through a
//                    table (FeatSegs): all targets in one launch per direction, chunks snapped to the targets' boundaries
//   k_place_count / k_place_flags / k_place_scatter   mutual filter, per-target fall-back and order-preserving compaction on the device
#pragma once
#include "normals_dev.h"

namespace {
namespace o3s_cloud {

constexpr int kFpfhNnMax = 128;  // largest max_nn served (the reference's feature_knn is 100)
constexpr int kFpfhBuf = 256;    // candidate keys a wave parks in LDS between two selections (>= kFpfhNnMax + 2 x 64)
constexpr int kFpfhDim = 33;
constexpr unsigned long long kKeyInfD = ~0ull;
constexpr int32_t kKeyInfJ = 0x7fffffff;

// Ascending bitonic sort of n2 (a power of two, 64 .. kFpfhBuf) keys (d2 bits, index) by the one wave of the block.  d2 >= 0 and
// never NaN here, so the order of the bit patterns is the order of the values.
__device__ __forceinline__ void wave_sort_keys(unsigned long long* kd, int32_t* kj, int n2, int lane) {
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = lane; t < (n2 >> 1); t += 64) {
        const int i = 2 * t - (t & (j - 1));  // bit j of i is clear
        const int p = i + j;
        const bool up = (i & k) == 0;
        const unsigned long long a = kd[i], b = kd[p];
        const int32_t ja = kj[i], jb = kj[p];
        const bool gt = a > b || (a == b && ja > jb);
        if (gt == up) {
          kd[i] = b;
          kd[p] = a;
          kj[i] = jb;
          kj[p] = ja;
        }
      }
      __syncthreads();  // one wave per block: orders the LDS traffic of consecutive stages
    }
}

// KDTreeFlann::SearchHybrid(p, radius, max_nn) for every point of the cloud, one wave (= one block) per query, queries in cell order.
// The lanes first find, one row of cells each, the run of cell-sorted points the ball's bounding box covers in that row (cells of a
// row are consecutive keys, so their points are one run); the wave then streams the runs 64 candidates at a time.  A candidate
// with d2 < r2 that beats the current max_nn-th best is appended to the LDS buffer (ballot + prefix count, no atomics); when fewer
// than 64 slots are left the buffer is sorted and cut to the max_nn best, whose last key becomes the bar for what follows.  The
// result does not depend on the order candidates arrive in, nor on the cell size: any ball, however many points it holds, is exact.
__global__ void __launch_bounds__(64) k_fpfh_lists(const double* __restrict__ sp /*cell-sorted points*/, const uint32_t* __restrict__ vals /*sorted -> original*/,
                                                   int64_t N, NGrid g, const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend, int max_nn,
                                                   double radius, double r2, int32_t* __restrict__ out_idx /*N x max_nn*/,
                                                   double* __restrict__ out_d2 /*N x max_nn*/) {
  static_assert(kFpfhBuf >= kFpfhNnMax + 128 && (kFpfhBuf & (kFpfhBuf - 1)) == 0, "room for one batch after a cut, power of two for the sort");
  __shared__ unsigned long long s_d[kFpfhBuf];
  __shared__ int32_t s_j[kFpfhBuf];
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= N) return;
  const double qx = sp[3 * t], qy = sp[3 * t + 1], qz = sp[3 * t + 2];
  const int64_t self = vals[t];
  // cells the ball can touch, per axis: one millionth of a cell of slack covers the rounding of the two divisions
  auto cell_lo = [&](double q, double o, int n) {
    const double v = floor((q - radius - o) / g.cell - 1e-6);
    return v < 0.0 ? 0 : (v > (double)(n - 1) ? n - 1 : (int)v);
  };
  auto cell_hi = [&](double q, double o, int n) {
    const double v = floor((q + radius - o) / g.cell + 1e-6);
    return v < 0.0 ? 0 : (v > (double)(n - 1) ? n - 1 : (int)v);
  };
  const int x0 = cell_lo(qx, g.ox, g.nx), x1 = cell_hi(qx, g.ox, g.nx);
  const int y0 = cell_lo(qy, g.oy, g.ny), y1 = cell_hi(qy, g.oy, g.ny);
  const int z0 = cell_lo(qz, g.oz, g.nz), z1 = cell_hi(qz, g.oz, g.nz);
  const int nyr = y1 - y0 + 1, nrows = nyr * (z1 - z0 + 1);
  int cnt = 0;
  unsigned long long thr_d = kKeyInfD;
  int32_t thr_j = kKeyInfJ;
  auto select = [&]() {  // sort what is parked, keep the max_nn best
    const int n2 = cnt <= 64 ? 64 : (cnt <= 128 ? 128 : kFpfhBuf);
    for (int i = cnt + lane; i < n2; i += 64) {
      s_d[i] = kKeyInfD;
      s_j[i] = kKeyInfJ;
    }
    __syncthreads();
    wave_sort_keys(s_d, s_j, n2, lane);
    if (cnt >= max_nn) {
      cnt = max_nn;
      thr_d = s_d[max_nn - 1];
      thr_j = s_j[max_nn - 1];
    }
    __syncthreads();
  };
  for (int rb = 0; rb < nrows; rb += 64) {
    const int r = rb + lane;
    uint32_t lo = 0u, hi = 0u;
    if (r < nrows) {
      const int z = z0 + r / nyr, y = y0 + r % nyr;
      const size_t row0 = ((size_t)z * (size_t)g.ny + (size_t)y) * (size_t)g.nx;
      bool any = false;
      for (int x = x0; x <= x1; ++x) {
        const uint32_t b = cbeg[row0 + (size_t)x], e = cend[row0 + (size_t)x];
        if (e > b) {  // empty cells carry begin = end = 0
          lo = any ? lo : b;
          hi = e;
          any = true;
        }
      }
    }
    unsigned long long have = __ballot(hi > lo);
    while (have) {
      const int rr = __ffsll((long long)have) - 1;
      have &= have - 1ull;
      const uint32_t rlo = __shfl(lo, rr, 64), rhi = __shfl(hi, rr, 64);
      for (uint32_t j0 = rlo; j0 < rhi; j0 += 64u) {
        const uint32_t j = j0 + (uint32_t)lane;
        bool pass = false;
        unsigned long long db = 0ull;
        int32_t id = 0;
        if (j < rhi) {
          const double ddx = qx - sp[3 * (size_t)j], ddy = qy - sp[3 * (size_t)j + 1], ddz = qz - sp[3 * (size_t)j + 2];
          double d = ddx * ddx;
          d = d + ddy * ddy;
          d = d + ddz * ddz;
          db = (unsigned long long)__double_as_longlong(d);
          id = (int32_t)vals[j];
          pass = d < r2 && (db < thr_d || (db == thr_d && id < thr_j));
        }
        const unsigned long long mask = __ballot(pass);
        if (mask) {
          if (pass) {
            const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
            s_d[pos] = db;
            s_j[pos] = id;
          }
          cnt += __popcll(mask);
          if (cnt > kFpfhBuf - 64) select();
        }
      }
    }
  }
  select();
  const int k = cnt < max_nn ? cnt : max_nn;
  for (int s = lane; s < max_nn; s += 64) {
    out_idx[(size_t)self * (size_t)max_nn + (size_t)s] = s < k ? s_j[s] : -1;
    out_d2[(size_t)self * (size_t)max_nn + (size_t)s] = s < k ? __longlong_as_double((long long)s_d[s]) : 0.0;
  }
}

// Pair feature of (p1, n1) and (p2, n2): include/o3s_cloud_ops.h.  Returns the three histogram coordinates (f3 is not binned).
__device__ __forceinline__ void pair_feature(const D3& p1, const D3& n1, const D3& p2, const D3& n2, double& f0, double& f1, double& f2) {
  f0 = f1 = f2 = 0.0;
  D3 dp{p2.x - p1.x, p2.y - p1.y, p2.z - p1.z};
  const double f3 = sqrt(dot3(dp, dp));
  if (f3 == 0.0) return;
  const double a1 = dot3(n1, dp) / f3, a2 = dot3(n2, dp) / f3;
  D3 na = n1, nb = n2;
  double g2;
  if (acos(fabs(a1)) > acos(fabs(a2))) {
    na = n2;
    nb = n1;
    dp = {-dp.x, -dp.y, -dp.z};
    g2 = -a2;
  } else {
    g2 = a1;
  }
  D3 v = cross3(dp, na);
  const double vn = sqrt(dot3(v, v));
  if (vn == 0.0) return;
  v = {v.x / vn, v.y / vn, v.z / vn};
  const D3 w = cross3(na, v);
  f2 = g2;
  f1 = dot3(v, nb);
  f0 = atan2(dot3(w, nb), dot3(na, nb));
}
// (int)floor(x) clamped to 0 .. 10; a NaN coordinate (NaN normal) falls in bin 0
__device__ __forceinline__ int bin11(double x) {
  const double fl = floor(x);
  return fl >= 10.0 ? 10 : (fl >= 1.0 ? (int)fl : 0);
}

__device__ __forceinline__ int list_length(const int32_t* __restrict__ row, int max_nn, int lane) {
  int len = 0;
  for (int s0 = 0; s0 < max_nn; s0 += 64) {
    const int s = s0 + lane;
    len += __popcll(__ballot(s < max_nn && row[s] >= 0));
  }
  return len;
}

// SPFH of every point: one wave per point, a lane per list entry; a bin's value is `inc` added count times, so the counts go to LDS
// (integer atomics) and lanes 0..32 replay the additions.  Column-major 33 x N: spfh[33 i + row].
__global__ void __launch_bounds__(64) k_spfh(const double* __restrict__ pts, const double* __restrict__ nrm, int64_t N, int max_nn,
                                             const int32_t* __restrict__ nn_idx, double* __restrict__ spfh) {
  __shared__ int s_cnt[kFpfhDim];
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  if (i >= N) return;
  if (lane < kFpfhDim) s_cnt[lane] = 0;
  __syncthreads();
  const int32_t* row = nn_idx + (size_t)i * (size_t)max_nn;
  const int len = list_length(row, max_nn, lane);
  if (len > 1) {
    const D3 p1{pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]}, n1{nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
    for (int k = 1 + lane; k < len; k += 64) {
      const size_t j = (size_t)row[k];
      const D3 p2{pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]}, n2{nrm[3 * j], nrm[3 * j + 1], nrm[3 * j + 2]};
      double f0, f1, f2;
      pair_feature(p1, n1, p2, n2, f0, f1, f2);
      const double kPi = 3.14159265358979323846;
      atomicAdd(&s_cnt[bin11(11.0 * (f0 + kPi) / (2.0 * kPi))], 1);
      atomicAdd(&s_cnt[11 + bin11(11.0 * (f1 + 1.0) * 0.5)], 1);
      atomicAdd(&s_cnt[22 + bin11(11.0 * (f2 + 1.0) * 0.5)], 1);
    }
  }
  __syncthreads();
  if (lane < kFpfhDim) {
    double v = 0.0;
    if (len > 1) {
      const double inc = 100.0 / (double)(len - 1);
      const int c = s_cnt[lane];
      for (int u = 0; u < c; ++u) v += inc;
    }
    spfh[(size_t)i * kFpfhDim + lane] = v;
  }
}

// FPFH of every point.  What the definition fixes is the order of the three group sums: each takes every val of its 11 rows in row
// order, neighbour after neighbour.  A lane therefore owns one (point, group) chain — 21 points per wave — and does all of its work
// alone: per neighbour it gathers its 11 SPFH values (88 contiguous bytes), divides each by d2, adds it to the group sum in row
// order and to its own output row.  Nothing crosses lanes, so there is neither a shuffle nor a barrier; list entries and gathers
// are fetched kFpfhAhead neighbours at a time.  An entry at distance 0 contributes val = +0.0, which changes no bit.
// (One wave per point, lane = row, the sums read through shuffles: 0.78 - 0.82 ms at 36.8 k points with or without prefetching —
// 22 LDS-path permutes per neighbour on an LDS shared by four SIMDs.  21 points per wave with the vals exchanged through LDS and
// two barriers per neighbour: 0.90 ms, a chain of dependent loads on too few waves.)
constexpr int kFpfhPts = 21;
constexpr int kFpfhAhead = 4;
__global__ void __launch_bounds__(64) k_fpfh(const double* __restrict__ spfh, int64_t N, int max_nn, const int32_t* __restrict__ nn_idx,
                                             const double* __restrict__ nn_d2, double* __restrict__ fpfh) {
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kFpfhPts + lane / 3;
  if (lane >= 3 * kFpfhPts || i >= N) return;
  const int g0 = (lane % 3) * 11;
  const int32_t* row = nn_idx + (size_t)i * (size_t)max_nn;
  const double* drow = nn_d2 + (size_t)i * (size_t)max_nn;
  int len = 0;
  {  // list length: the -1 padding is a suffix, so the first negative entry is found by bisection
    int lo = 0, hi = max_nn;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (row[mid] >= 0) lo = mid + 1;
      else hi = mid;
    }
    len = lo;
  }
  double out[11];
#pragma unroll
  for (int w = 0; w < 11; ++w) out[w] = 0.0;
  double* dst = fpfh + (size_t)i * kFpfhDim + g0;
  if (len > 1) {
    double sum = 0.0;
    for (int k0 = 1; k0 < len; k0 += kFpfhAhead) {
      double sv[kFpfhAhead][11], dv[kFpfhAhead];
#pragma unroll
      for (int u = 0; u < kFpfhAhead; ++u) {
        const int k = k0 + u < len ? k0 + u : len - 1;  // past the end: the last entry again, then ignored
        dv[u] = k0 + u < len ? drow[k] : 0.0;
        const double* src = spfh + (size_t)row[k] * kFpfhDim + g0;
#pragma unroll
        for (int w = 0; w < 11; ++w) sv[u][w] = src[w];
      }
#pragma unroll
      for (int u = 0; u < kFpfhAhead; ++u) {
        const bool use = dv[u] != 0.0;  // an entry at distance 0 is skipped
        const double d = use ? dv[u] : 1.0;
#pragma unroll
        for (int w = 0; w < 11; ++w) {
          const double val = use ? sv[u][w] / d : 0.0;
          sum += val;
          out[w] += val;
        }
      }
    }
    if (sum != 0.0) sum = 100.0 / sum;
    const double* own = spfh + (size_t)i * kFpfhDim + g0;
#pragma unroll
    for (int w = 0; w < 11; ++w) {
      out[w] = out[w] * sum;
      out[w] = out[w] + own[w];
    }
  }
#pragma unroll
  for (int w = 0; w < 11; ++w) dst[w] = out[w];
}

struct FpfhWork {  // grow-only buffers of the feature computation (owned by the caller's object)
  NormalsWork grid;
  DevMem idx, d2, spfh;  // neighbour lists (N x max_nn int32 + d2) and SPFH (33 x N): in HBM between the stages
  void release() {
    grid.release();
    idx.release();
    d2.release();
    spfh.release();
  }
};

// d_pts, d_nrm (3 x N doubles, device) -> d_fpfh (33 x N doubles); the lists and the SPFH stay in w (w.idx, w.d2, w.spfh)
inline int fpfh_dev(FpfhWork& w, const double* d_pts, const double* d_nrm, int64_t N, double radius, int max_nn, double* d_fpfh, hipStream_t s) {
  if (N == 0) return O3S_OK;
  if (N > (int64_t)0x7fffffff || max_nn < 1 || max_nn > kFpfhNnMax || !(radius > 0.0) || !std::isfinite(radius)) return O3S_ERR_BAD_ARGUMENT;
  const size_t n = (size_t)N;
  CK(w.idx.alloc(n * (size_t)max_nn * 4));
  CK(w.d2.alloc(n * (size_t)max_nn * 8));
  CK(w.spfh.alloc(n * kFpfhDim * 8));
  GridIndex gi;
  // cells of half a radius, never re-sized (the density target is out of reach on purpose): the ball's box is at most 6 cells wide,
  // so a query has at most 36 rows — one per lane — and the runs hold 1.5 - 2 x the ball's points
  const int rc = build_grid_index(w.grid, d_pts, N, radius * 0.5, 1e30, radius * 0.5, &gi, s);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_fpfh_lists, dim3((unsigned)N), dim3(64), 0, s, gi.sp, gi.vals, N, gi.g, gi.cbeg, gi.cend, max_nn, radius, radius * radius,
                     w.idx.as<int32_t>(), w.d2.as<double>());
  hipLaunchKernelGGL(k_spfh, dim3((unsigned)N), dim3(64), 0, s, d_pts, d_nrm, N, max_nn, (const int32_t*)w.idx.as<int32_t>(), w.spfh.as<double>());
  hipLaunchKernelGGL(k_fpfh, dim3((unsigned)((N + kFpfhPts - 1) / kFpfhPts)), dim3(64), 0, s, (const double*)w.spfh.as<double>(), N, max_nn, (const int32_t*)w.idx.as<int32_t>(),
                     (const double*)w.d2.as<double>(), d_fpfh);
  CK(hipGetLastError());
  return O3S_OK;
}

// ---- feature correspondences -------------------------------------------------------------------------------------------------
constexpr int kFcBlock = 256;
constexpr int kFcTileDoubles = 2112;  // 64 target columns of 33 rows (16.5 KiB of LDS)
constexpr int kFcDimMax = 264;        // a tile holds at least 8 columns

// Nearest target column of every source column within one chunk of the targets: squared L2 as the running sum of squared
// differences in row order (never |a|^2 + |b|^2 - 2 a.b: it cancels).  A thread owns a source column (in registers at DIM = 33),
// the block stages `tile` target columns in LDS and every lane reads the same word (a broadcast).  Strict `<` while walking the
// targets upwards keeps the lowest index among equals.
template <int DIM>
__global__ void __launch_bounds__(kFcBlock) k_feat_nn(const double* __restrict__ src, int64_t n, const double* __restrict__ tgt, int64_t m, int dim_rt,
                                                      int64_t chunk, double* __restrict__ part_d /*[chunks][n]*/, int32_t* __restrict__ part_j) {
  __shared__ double s_t[kFcTileDoubles];
  const int dim = DIM > 0 ? DIM : dim_rt;
  const int tile = kFcTileDoubles / dim;
  const int64_t i = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.y * chunk, t1 = t0 + chunk < m ? t0 + chunk : m;
  const double* a_g = src + (size_t)(i < n ? i : 0) * (size_t)dim;
  double a[DIM > 0 ? DIM : 1];
  if (DIM > 0) {
#pragma unroll
    for (int j = 0; j < DIM; ++j) a[j] = a_g[j];
  }
  double best = __builtin_huge_val();
  int32_t bj = -1;
  for (int64_t tb = t0; tb < t1; tb += tile) {
    const int nt = (int)(t1 - tb < (int64_t)tile ? t1 - tb : (int64_t)tile);
    __syncthreads();
    for (int e = threadIdx.x; e < nt * dim; e += kFcBlock) s_t[e] = tgt[(size_t)tb * (size_t)dim + (size_t)e];
    __syncthreads();
    for (int u = 0; u < nt; ++u) {
      double d = 0.0;
      if (DIM > 0) {
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
          const double df = a[j] - s_t[u * DIM + j];
          d = d + df * df;
        }
      } else {
        for (int j = 0; j < dim; ++j) {
          const double df = a_g[j] - s_t[u * dim + j];
          d = d + df * df;
        }
      }
      if (d < best) {
        best = d;
        bj = (int32_t)(tb + u);
      }
    }
  }
  if (i < n) {
    part_d[(size_t)blockIdx.y * (size_t)n + (size_t)i] = best;
    part_j[(size_t)blockIdx.y * (size_t)n + (size_t)i] = bj;
  }
}
__global__ void __launch_bounds__(kFcBlock) k_feat_nn_fold(const double* __restrict__ part_d, const int32_t* __restrict__ part_j, int64_t n, int chunks,
                                                           int32_t* __restrict__ out_j) {
  const int64_t i = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
  if (i >= n) return;
  double best = __builtin_huge_val();
  int32_t bj = -1;
  for (int c = 0; c < chunks; ++c) {  // chunks in ascending target order: strict `<` keeps the lower index
    const double d = part_d[(size_t)c * (size_t)n + (size_t)i];
    if (d < best) {
      best = d;
      bj = part_j[(size_t)c * (size_t)n + (size_t)i];
    }
  }
  out_j[i] = bj;
}

struct FeatNnWork {
  DevMem part_d, part_j, ij, ji;
};

// out_j[i] = the column of b nearest to column i of a (device arrays, dim x n / dim x m)
inline int feat_nn_dev(DevMem& part_d, DevMem& part_j, const double* d_a, int64_t n, const double* d_b, int64_t m, int dim, int32_t* d_out_j, hipStream_t s) {
  const unsigned bx = (unsigned)((n + kFcBlock - 1) / kFcBlock);
  const int64_t tile = kFcTileDoubles / dim;
  // about 2048 blocks in all (8 per CU), chunks a whole number of tiles
  int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((m + tile - 1) / tile, 2048 / (int64_t)bx));
  int64_t chunk = ((m + chunks - 1) / chunks + tile - 1) / tile * tile;
  chunks = (m + chunk - 1) / chunk;
  CK(part_d.alloc((size_t)chunks * (size_t)n * 8));
  CK(part_j.alloc((size_t)chunks * (size_t)n * 4));
  if (dim == kFpfhDim)
    hipLaunchKernelGGL(k_feat_nn<kFpfhDim>, dim3(bx, (unsigned)chunks), dim3(kFcBlock), 0, s, d_a, n, d_b, m, dim, chunk, part_d.as<double>(), part_j.as<int32_t>());
  else
    hipLaunchKernelGGL(k_feat_nn<0>, dim3(bx, (unsigned)chunks), dim3(kFcBlock), 0, s, d_a, n, d_b, m, dim, chunk, part_d.as<double>(), part_j.as<int32_t>());
  hipLaunchKernelGGL(k_feat_nn_fold, dim3(bx), dim3(kFcBlock), 0, s, (const double*)part_d.as<double>(), (const int32_t*)part_j.as<int32_t>(), n, (int)chunks,
                     d_out_j);
  CK(hipGetLastError());
  return O3S_OK;
}

// The head of RegistrationRANSACBasedOnFeatureMatching on device feature arrays: ij, with mutual_filter also ji and the pairs
// (i, ij[i]) with ji[ij[i]] == i in ascending i; fewer than 3 ransac_n of those -> all (i, ij[i]).  The two index arrays come to
// the host (4 (n + m) bytes) and the filter runs there.
inline int feature_correspondences_dev(FeatNnWork& w, const double* d_src, int64_t n_src, const double* d_tgt, int64_t n_tgt, int dim, int mutual_filter,
                                       int ransac_n, int32_t* out_pairs, int64_t* n_out, int* used_fallback, hipStream_t s) {
  *n_out = 0;
  if (used_fallback) *used_fallback = 0;
  if (n_src == 0 || n_tgt == 0) return O3S_OK;
  if (n_src > (int64_t)0x7fffffff || n_tgt > (int64_t)0x7fffffff || dim < 1 || dim > kFcDimMax || ransac_n < 0) return O3S_ERR_BAD_ARGUMENT;
  std::vector<int32_t> ij((size_t)n_src), ji;
  CK(w.ij.alloc((size_t)n_src * 4));
  int rc = feat_nn_dev(w.part_d, w.part_j, d_src, n_src, d_tgt, n_tgt, dim, w.ij.as<int32_t>(), s);
  if (rc != O3S_OK) return rc;
  CK(hipMemcpyAsync(ij.data(), w.ij.p, (size_t)n_src * 4, hipMemcpyDeviceToHost, s));
  if (mutual_filter) {
    ji.resize((size_t)n_tgt);
    CK(w.ji.alloc((size_t)n_tgt * 4));
    CK(hipStreamSynchronize(s));  // the partial winners are re-used by the second direction
    rc = feat_nn_dev(w.part_d, w.part_j, d_tgt, n_tgt, d_src, n_src, dim, w.ji.as<int32_t>(), s);
    if (rc != O3S_OK) return rc;
    CK(hipMemcpyAsync(ji.data(), w.ji.p, (size_t)n_tgt * 4, hipMemcpyDeviceToHost, s));
  }
  CK(hipStreamSynchronize(s));
  int64_t k = 0;
  if (mutual_filter) {
    for (int64_t i = 0; i < n_src; ++i) {
      const int32_t j = ij[(size_t)i];
      if (j >= 0 && ji[(size_t)j] == (int32_t)i) {
        out_pairs[2 * k] = (int32_t)i;
        out_pairs[2 * k + 1] = j;
        ++k;
      }
    }
    if (k >= (int64_t)3 * ransac_n) {
      *n_out = k;
      return O3S_OK;
    }
    if (used_fallback) *used_fallback = 1;
    k = 0;
  }
  for (int64_t i = 0; i < n_src; ++i) {  // a column of NaNs has no nearest column and makes no pair
    const int32_t j = ij[(size_t)i];
    if (j >= 0) {
      out_pairs[2 * k] = (int32_t)i;
      out_pairs[2 * k + 1] = j;
      ++k;
    }
  }
  *n_out = k;
  return O3S_OK;
}

// ---- one source against several targets (include/place_recognition/o3s_place_recognition.h) -----------------------------------
// The feature arrays of up to kPlaceMaxTargets targets as a table passed by value: nothing is concatenated or copied.  beg[k] is
// the first column of target k in the concatenated column space, beg[K] the number of columns of all targets; cbeg[k] the first
// chunk of target k in the forward search, whose chunks all hold `chunk` columns (a whole number of tiles) and never straddle
// two targets.  The arithmetic is k_feat_nn's: per-segment results do not depend on the partition.
constexpr int kPlaceMaxTargets = 16;
struct FeatSegs {
  const double* f[kPlaceMaxTargets];
  int64_t beg[kPlaceMaxTargets + 1];
  int32_t cbeg[kPlaceMaxTargets + 1];
  int32_t K;
  int64_t chunk;
};
// the segment that holds element g of a table of begins (statically indexed: the table stays in scalar registers)
template <class T>
__device__ __forceinline__ int seg_of(const T (&beg)[kPlaceMaxTargets + 1], int K, T g) {
  int k = 0;
#pragma unroll
  for (int q = 1; q < kPlaceMaxTargets; ++q)
    if (q < K && g >= beg[q]) k = q;
  return k;
}
template <class T>
__device__ __forceinline__ T seg_pick(const T (&v)[kPlaceMaxTargets], int k) {
  T r = v[0];
#pragma unroll
  for (int q = 1; q < kPlaceMaxTargets; ++q)
    if (q == k) r = v[q];
  return r;
}
template <class T>
__device__ __forceinline__ T seg_pick1(const T (&v)[kPlaceMaxTargets + 1], int k) {
  T r = v[0];
#pragma unroll
  for (int q = 1; q <= kPlaceMaxTargets; ++q)
    if (q == k) r = v[q];
  return r;
}

// Forward: nearest column of every target for every source column, one launch.  blockIdx.y is a chunk of ONE target; the winner's
// index is local to that target.
template <int DIM>
__global__ void __launch_bounds__(kFcBlock) k_feat_nn_fwd_multi(const double* __restrict__ src, int64_t n, FeatSegs sg, int dim_rt,
                                                                double* __restrict__ part_d /*[chunks][n]*/, int32_t* __restrict__ part_j) {
  __shared__ double s_t[kFcTileDoubles];
  const int dim = DIM > 0 ? DIM : dim_rt;
  const int tile = kFcTileDoubles / dim;
  const int64_t i = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
  const int k = seg_of(sg.cbeg, sg.K, (int32_t)blockIdx.y);
  const double* __restrict__ tgt = seg_pick(sg.f, k);
  const int64_t m = seg_pick1(sg.beg, k + 1) - seg_pick1(sg.beg, k);
  const int64_t t0 = (int64_t)((int32_t)blockIdx.y - seg_pick1(sg.cbeg, k)) * sg.chunk, t1 = t0 + sg.chunk < m ? t0 + sg.chunk : m;
  const double* a_g = src + (size_t)(i < n ? i : 0) * (size_t)dim;
  double a[DIM > 0 ? DIM : 1];
  if (DIM > 0) {
#pragma unroll
    for (int j = 0; j < DIM; ++j) a[j] = a_g[j];
  }
  double best = __builtin_huge_val();
  int32_t bj = -1;
  for (int64_t tb = t0; tb < t1; tb += tile) {
    const int nt = (int)(t1 - tb < (int64_t)tile ? t1 - tb : (int64_t)tile);
    __syncthreads();
    for (int e = threadIdx.x; e < nt * dim; e += kFcBlock) s_t[e] = tgt[(size_t)tb * (size_t)dim + (size_t)e];
    __syncthreads();
    for (int u = 0; u < nt; ++u) {
      double d = 0.0;
      if (DIM > 0) {
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
          const double df = a[j] - s_t[u * DIM + j];
          d = d + df * df;
        }
      } else {
        for (int j = 0; j < dim; ++j) {
          const double df = a_g[j] - s_t[u * dim + j];
          d = d + df * df;
        }
      }
      if (d < best) {
        best = d;
        bj = (int32_t)(tb + u);
      }
    }
  }
  if (i < n) {
    part_d[(size_t)blockIdx.y * (size_t)n + (size_t)i] = best;
    part_j[(size_t)blockIdx.y * (size_t)n + (size_t)i] = bj;
  }
}
// ij[k][i]: the chunks of target k in ascending order (blockIdx.y = k); a target without columns has no chunk and gives -1
__global__ void __launch_bounds__(kFcBlock) k_feat_nn_fwd_fold(const double* __restrict__ part_d, const int32_t* __restrict__ part_j, int64_t n, FeatSegs sg,
                                                               int32_t* __restrict__ ij /*[K][n]*/) {
  const int64_t i = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
  if (i >= n) return;
  const int k = (int)blockIdx.y;
  const int c0 = seg_pick1(sg.cbeg, k), c1 = seg_pick1(sg.cbeg, k + 1);
  double best = __builtin_huge_val();
  int32_t bj = -1;
  for (int c = c0; c < c1; ++c) {
    const double d = part_d[(size_t)c * (size_t)n + (size_t)i];
    if (d < best) {
      best = d;
      bj = part_j[(size_t)c * (size_t)n + (size_t)i];
    }
  }
  ij[(size_t)k * (size_t)n + (size_t)i] = bj;
}

// Backward: nearest source column of every column of every target, one launch.  A thread owns column g of the concatenated
// targets, read through the table; the block stages tiles of the source, blockIdx.y walks chunks of it.
template <int DIM>
__global__ void __launch_bounds__(kFcBlock) k_feat_nn_bwd_multi(FeatSegs sg, const double* __restrict__ src, int64_t n, int dim_rt, int64_t chunk,
                                                                double* __restrict__ part_d /*[chunks][M]*/, int32_t* __restrict__ part_j) {
  __shared__ double s_t[kFcTileDoubles];
  const int dim = DIM > 0 ? DIM : dim_rt;
  const int tile = kFcTileDoubles / dim;
  const int64_t M = seg_pick1(sg.beg, sg.K);
  const int64_t g = (int64_t)blockIdx.x * kFcBlock + threadIdx.x, gc = g < M ? g : 0;
  const int k = seg_of(sg.beg, sg.K, gc);
  const double* a_g = seg_pick(sg.f, k) + (size_t)(gc - seg_pick1(sg.beg, k)) * (size_t)dim;
  const int64_t t0 = (int64_t)blockIdx.y * chunk, t1 = t0 + chunk < n ? t0 + chunk : n;
  double a[DIM > 0 ? DIM : 1];
  if (DIM > 0) {
#pragma unroll
    for (int j = 0; j < DIM; ++j) a[j] = a_g[j];
  }
  double best = __builtin_huge_val();
  int32_t bj = -1;
  for (int64_t tb = t0; tb < t1; tb += tile) {
    const int nt = (int)(t1 - tb < (int64_t)tile ? t1 - tb : (int64_t)tile);
    __syncthreads();
    for (int e = threadIdx.x; e < nt * dim; e += kFcBlock) s_t[e] = src[(size_t)tb * (size_t)dim + (size_t)e];
    __syncthreads();
    for (int u = 0; u < nt; ++u) {
      double d = 0.0;
      if (DIM > 0) {
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
          const double df = a[j] - s_t[u * DIM + j];
          d = d + df * df;
        }
      } else {
        for (int j = 0; j < dim; ++j) {
          const double df = a_g[j] - s_t[u * dim + j];
          d = d + df * df;
        }
      }
      if (d < best) {
        best = d;
        bj = (int32_t)(tb + u);
      }
    }
  }
  if (g < M) {
    part_d[(size_t)blockIdx.y * (size_t)M + (size_t)g] = best;
    part_j[(size_t)blockIdx.y * (size_t)M + (size_t)g] = bj;
  }
}

// The head of a place-recognition call, kPlaceHeadWords u32 per target: [0] mutual pairs counted, [1] used_fallback, [2] n_pairs
constexpr int kPlaceHeadWords = 4;
// mutual pairs of every target: one integer atomic per wave (the count does not depend on their order)
__global__ void __launch_bounds__(kFcBlock) k_place_count(const int32_t* __restrict__ ij, const int32_t* __restrict__ ji, int64_t n, FeatSegs sg,
                                                          uint32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
  const int k = (int)blockIdx.y;
  bool f = false;
  if (i < n) {
    const int32_t j = ij[(size_t)k * (size_t)n + (size_t)i];
    f = j >= 0 && ji[(size_t)(seg_pick1(sg.beg, k) + j)] == (int32_t)i;
  }
  const unsigned long long b = __ballot(f);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&head[k * kPlaceHeadWords], (uint32_t)__popcll(b));
}
// flag[k][i] of the pair (i, ij[k][i]): mutual, or — no mutual filter, or fewer than 3 ransac_n mutual pairs in THIS target —
// every source column that has a nearest column.  Thread 0 of each target's first block records the decision.
__global__ void __launch_bounds__(kFcBlock) k_place_flags(const int32_t* __restrict__ ij, const int32_t* __restrict__ ji, int64_t n, FeatSegs sg, int mutual,
                                                          uint32_t min_mutual, uint32_t* __restrict__ head, uint32_t* __restrict__ flag /*[K * n + 1]*/) {
  const int64_t i = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
  const int k = (int)blockIdx.y;
  const int64_t b0 = seg_pick1(sg.beg, k), m = seg_pick1(sg.beg, k + 1) - b0;
  const bool fallback = mutual && m > 0 && head[k * kPlaceHeadWords] < min_mutual;
  if (i == 0) head[k * kPlaceHeadWords + 1] = fallback ? 1u : 0u;
  if (i == 0 && k == 0) flag[(size_t)sg.K * (size_t)n] = 0u;  // the scan's last offset is then the number of all pairs
  if (i >= n) return;
  const int32_t j = ij[(size_t)k * (size_t)n + (size_t)i];
  bool f = j >= 0;
  if (f && mutual && !fallback) f = ji[(size_t)(b0 + j)] == (int32_t)i;
  flag[(size_t)k * (size_t)n + (size_t)i] = f ? 1u : 0u;
}
// order-preserving compaction into target k's slice (n pairs wide) of the pair buffer, and the slice's length
__global__ void __launch_bounds__(kFcBlock) k_place_scatter(const int32_t* __restrict__ ij, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off,
                                                            int64_t n, uint32_t* __restrict__ head, int32_t* __restrict__ pairs /*[K][n][2]*/) {
  const int64_t i = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
  const int k = (int)blockIdx.y;
  const size_t r0 = (size_t)k * (size_t)n;
  const uint32_t o0 = off[r0];
  if (i == 0) head[k * kPlaceHeadWords + 2] = off[r0 + (size_t)n] - o0;
  if (i >= n || !flag[r0 + (size_t)i]) return;
  const size_t at = r0 + (size_t)(off[r0 + (size_t)i] - o0);
  pairs[2 * at] = (int32_t)i;
  pairs[2 * at + 1] = ij[r0 + (size_t)i];
}

// Blocks a search launch aims at.  The 33-row search holds 85 VGPRs: 5 waves per SIMD, 5 blocks per CU, 1280 resident blocks on the
// 256 CUs; a launch of 8 x 1280 blocks of equal work leaves at most an eighth of the last round idle (feat_nn_dev's 2048 blocks are
// 1.6 rounds, and a one-to-many launch has K times the columns to cut finer).  Measured at closure size, K = 4: 2048 -> 31.2 ms,
// 5120 -> 26.2, 10240 -> 25.7, 40960 -> 24.9 against 30 ms for the loop of per-pair calls; the partial winners grow with
// it (12 bytes per source column and chunk).  The hooks build reads it per call, so that one test can run several partitions of the
// same targets.
constexpr int kPlaceBlocks = 10240;
inline int64_t place_blocks() {
  if (const char* e = O3S_HOOK_ENV("O3S_PLACE_BLOCKS")) {
    const long v = atol(e);
    if (v >= 1 && v <= (1 << 20)) return (int64_t)v;
  }
  return kPlaceBlocks;
}

// grow-only work area of a one-to-many call (part of the leased RANSAC area, ransac_impl.h)
struct PlaceWork {
  DevMem part_d, part_j, ij, ji, flag, off, head, pairs, scan_tmp;
};

// Correspondences of one source feature array against K targets (device arrays): w.pairs holds K slices of n_src pairs, slice k
// the pairs of target k in ascending source index; n_out[k], used_fallback[k] come to the host in ONE small copy, behind which the
// stream is drained.  The arguments were checked by the caller: 1 <= K <= kPlaceMaxTargets, n_src >= 1, K n_src < 2^31, all
// targets' columns together < 2^31, 1 <= dim <= kFcDimMax, ransac_n >= 0.
inline int place_correspondences_dev(PlaceWork& w, const double* d_src, int64_t n, const double* const* d_tgt, const int64_t* n_tgt, int K, int dim,
                                     int mutual_filter, int ransac_n, int64_t* n_out, int32_t* used_fallback, hipStream_t s) {
  const int64_t tile = kFcTileDoubles / dim;
  const unsigned bx = (unsigned)((n + kFcBlock - 1) / kFcBlock);
  FeatSegs sg;
  memset(&sg, 0, sizeof(sg));
  sg.K = K;
  int64_t M = 0;
  for (int k = 0; k < K; ++k) {
    sg.f[k] = d_tgt[k];
    sg.beg[k] = M;
    M += n_tgt[k];
  }
  for (int k = K; k <= kPlaceMaxTargets; ++k) sg.beg[k] = M;
  // about kPlaceBlocks blocks in all; one chunk size for every target, a whole number of tiles
  const int64_t blocks = place_blocks();
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>((M + tile - 1) / tile, blocks / (int64_t)bx));
  sg.chunk = std::max<int64_t>(tile, ((M + want - 1) / want + tile - 1) / tile * tile);
  int32_t chunks = 0;
  for (int k = 0; k < K; ++k) {
    sg.cbeg[k] = chunks;
    chunks += (int32_t)((n_tgt[k] + sg.chunk - 1) / sg.chunk);
  }
  for (int k = K; k <= kPlaceMaxTargets; ++k) sg.cbeg[k] = chunks;
  const size_t rows = (size_t)K * (size_t)n;
  CK(w.ij.alloc(rows * 4));
  CK(w.flag.alloc((rows + 1) * 4));
  CK(w.off.alloc((rows + 2) * 4));
  CK(w.pairs.alloc(rows * 8));
  CK(w.head.alloc((size_t)kPlaceMaxTargets * kPlaceHeadWords * 4));
  const size_t scan_bytes = scan_temp_bytes((int64_t)rows + 1);
  CK(w.scan_tmp.alloc(scan_bytes));
  // backward chunks over the source
  const unsigned by = (unsigned)((M + kFcBlock - 1) / kFcBlock);
  int64_t bchunks = std::max<int64_t>(1, std::min<int64_t>((n + tile - 1) / tile, blocks / (int64_t)std::max(by, 1u)));
  const int64_t bchunk = ((n + bchunks - 1) / bchunks + tile - 1) / tile * tile;
  bchunks = (n + bchunk - 1) / bchunk;
  const bool back = mutual_filter && M > 0;
  CK(w.part_d.alloc(std::max((size_t)chunks * (size_t)n, back ? (size_t)bchunks * (size_t)M : (size_t)0) * 8));
  CK(w.part_j.alloc(std::max((size_t)chunks * (size_t)n, back ? (size_t)bchunks * (size_t)M : (size_t)0) * 4));
  CK(hipMemsetAsync(w.head.p, 0, (size_t)kPlaceMaxTargets * kPlaceHeadWords * 4, s));
  if (chunks > 0) {
    if (dim == kFpfhDim)
      hipLaunchKernelGGL(k_feat_nn_fwd_multi<kFpfhDim>, dim3(bx, (unsigned)chunks), dim3(kFcBlock), 0, s, d_src, n, sg, dim, w.part_d.as<double>(),
                         w.part_j.as<int32_t>());
    else
      hipLaunchKernelGGL(k_feat_nn_fwd_multi<0>, dim3(bx, (unsigned)chunks), dim3(kFcBlock), 0, s, d_src, n, sg, dim, w.part_d.as<double>(),
                         w.part_j.as<int32_t>());
  }
  hipLaunchKernelGGL(k_feat_nn_fwd_fold, dim3(bx, (unsigned)K), dim3(kFcBlock), 0, s, (const double*)w.part_d.as<double>(), (const int32_t*)w.part_j.as<int32_t>(), n,
                     sg, w.ij.as<int32_t>());
  if (back) {  // in stream order behind the fold, which was the last reader of the forward partial winners
    CK(w.ji.alloc((size_t)M * 4));
    if (dim == kFpfhDim)
      hipLaunchKernelGGL(k_feat_nn_bwd_multi<kFpfhDim>, dim3(by, (unsigned)bchunks), dim3(kFcBlock), 0, s, sg, d_src, n, dim, bchunk, w.part_d.as<double>(),
                         w.part_j.as<int32_t>());
    else
      hipLaunchKernelGGL(k_feat_nn_bwd_multi<0>, dim3(by, (unsigned)bchunks), dim3(kFcBlock), 0, s, sg, d_src, n, dim, bchunk, w.part_d.as<double>(),
                         w.part_j.as<int32_t>());
    hipLaunchKernelGGL(k_feat_nn_fold, dim3(by), dim3(kFcBlock), 0, s, (const double*)w.part_d.as<double>(), (const int32_t*)w.part_j.as<int32_t>(), M, (int)bchunks,
                       w.ji.as<int32_t>());
    hipLaunchKernelGGL(k_place_count, dim3(bx, (unsigned)K), dim3(kFcBlock), 0, s, (const int32_t*)w.ij.as<int32_t>(), (const int32_t*)w.ji.as<int32_t>(), n, sg,
                       w.head.as<uint32_t>());
  }
  hipLaunchKernelGGL(k_place_flags, dim3(bx, (unsigned)K), dim3(kFcBlock), 0, s, (const int32_t*)w.ij.as<int32_t>(), (const int32_t*)w.ji.as<int32_t>(), n, sg,
                     back ? 1 : 0, (uint32_t)std::min<int64_t>((int64_t)3 * ransac_n, (int64_t)0xffffffff), w.head.as<uint32_t>(), w.flag.as<uint32_t>());
  CK(hipGetLastError());
  const int rc = scan_flags_dev(w.flag.as<uint32_t>(), w.off.as<uint32_t>(), (int64_t)rows + 1, w.scan_tmp.p, scan_bytes, s);
  if (rc != O3S_OK) return rc;
  hipLaunchKernelGGL(k_place_scatter, dim3(bx, (unsigned)K), dim3(kFcBlock), 0, s, (const int32_t*)w.ij.as<int32_t>(), (const uint32_t*)w.flag.as<uint32_t>(),
                     (const uint32_t*)w.off.as<uint32_t>(), n, w.head.as<uint32_t>(), w.pairs.as<int32_t>());
  CK(hipGetLastError());
  uint32_t head[kPlaceMaxTargets * kPlaceHeadWords];
  CK(hipMemcpyAsync(head, w.head.p, sizeof(head), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  for (int k = 0; k < K; ++k) {
    n_out[k] = (int64_t)head[k * kPlaceHeadWords + 2];
    if (used_fallback) used_fallback[k] = (int32_t)head[k * kPlaceHeadWords + 1];
  }
  return O3S_OK;
}

}  // namespace o3s_cloud
}  // namespace
