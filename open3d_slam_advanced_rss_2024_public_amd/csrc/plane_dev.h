// plane_dev.h — device side of PointCloud::SegmentPlane (contract: include/plane_segmentation/o3s_plane_segmentation.h; Open3D
// v0.15.1, geometry/PointCloudSegmentation.cpp; Fischler & Bolles 1981).  Part of the cloud_ops.hip translation unit.
// Iteration `itr` is a pure function of (seed, itr, plane number): a lane of k_pl_hyp draws (or reads) its sample and forms the plane
// of its first three points; k_pl_eval scores a batch of hypotheses over all M points (one lane per hypothesis, its four
// coefficients in registers, one chunk of kPlChunk points per block staged in LDS and read at the same address by every lane: a
// broadcast), k_pl_fold adds a hypothesis' chunks up in ascending order and one wave applies the serial selection rule to the
// device-resident header (k_pl_select).  A hypothesis that does not PASS is scored like the others and skipped by the fold and
// the rule: at the design shapes fewer than one in ten thousand is, and compacting the batch would cost three launches more.
// The winner's inliers are flagged, scanned and gathered, and GetPlaneFromPoints runs over that list in chunks of kPlChunk.
// fp64, no FMA contraction, integer atomics only — and none at all in the scoring path: no result depends on an arrival order.
#pragma once
#include "ransac_dev.h"  // philox4x32_10: one definition of the sample stream

#include "../../include/plane_segmentation/o3s_plane_segmentation.h"

#pragma clang fp contract(off)

namespace {
namespace o3s_cloud {

constexpr int kPlNMax = 8;
constexpr int kPlBatch = 1024;    // iterations per batch; the hooks build reads O3S_PLANE_BATCH per call
constexpr int kPlChunk = 512;     // points per evaluation chunk: part of the contract (the order of the err sum)
constexpr int kPlEvalBlock = 64;  // hypotheses per block of k_pl_eval for a batch below kPlEvalBlockMax, else kPlEvalBlockMax;
constexpr int kPlEvalBlockMax = 256;  // the hooks build reads O3S_PLANE_EVAL_BLOCK (64, 128, 256)
constexpr int kPlFoldBlock = 64;
constexpr int kPlFoldAhead = 8;   // chunk sums loaded together in front of their adds
constexpr int kPlLook = 8;        // with confidence < 1 the host reads est_k back every kPlLook batches

struct PlaneHeader {  // device resident: the best so far, the serial rule's est_k, then the inlier list's length and the refit
  long long est_k, best_itr, evaluated, n_in, n_list;
  double err, fitness, rmse;
  double plane[4];  // the winning sample's
  double cen[3];    // centroid of the inlier list
  double model[4];  // GetPlaneFromPoints of the inlier list
};
struct PlaneArgs {
  int n;
  uint32_t k;  // plane number of the peel: the last counter word
  double thr, confidence;
  unsigned long long seed;
  long long M;
};

__global__ void k_pl_init(PlaneHeader* __restrict__ h, long long n_iter) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  h->est_k = n_iter;
  h->best_itr = -1;
  h->evaluated = h->n_in = h->n_list = 0;
  h->err = h->fitness = h->rmse = 0.0;
  for (int k = 0; k < 4; ++k) h->plane[k] = h->model[k] = 0.0;
  for (int k = 0; k < 3; ++k) h->cen[k] = 0.0;
}

__device__ __forceinline__ double pl_dist(double a, double b, double c, double d, double x, double y, double z) {
  return fabs(((a * x + b * y) + c * z) + d);
}

// One lane per iteration of the batch [itr0, itr0 + count): outcome and plane (a, b, c, d; zeros unless PASS) at slot itr - itr0.
__global__ void __launch_bounds__(kB) k_pl_hyp(PlaneArgs a, const double* __restrict__ pts, const int32_t* __restrict__ table, long long itr0, int count,
                                               const PlaneHeader* __restrict__ hdr, int32_t* __restrict__ outcome, double* __restrict__ planes) {
  if (hdr && itr0 >= hdr->est_k) return;  // the serial loop has ended in front of this batch
  const int slot = blockIdx.x * kB + threadIdx.x;
  if (slot >= count) return;
  const long long itr = itr0 + slot;
  const int n = a.n;
  int idx[kPlNMax];
  if (table) {
#pragma unroll
    for (int j = 0; j < kPlNMax; ++j) idx[j] = j < n ? table[itr * n + j] : -1 - j;
  } else {
#pragma unroll
    for (int q = 0; q < kPlNMax / 4; ++q) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (q * 4 < n) philox4x32_10((uint32_t)itr, (uint32_t)((unsigned long long)itr >> 32), (uint32_t)q, a.k, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
#pragma unroll
      for (int u = 0; u < 4; ++u) idx[q * 4 + u] = q * 4 + u < n ? (int)(((unsigned long long)w[u] * (unsigned long long)a.M) >> 32) : -1 - (q * 4 + u);
    }
  }
  int out = O3S_PLANE_PASS;
#pragma unroll
  for (int p = 0; p < kPlNMax; ++p) {
    if (p < n && (idx[p] < 0 || (long long)idx[p] >= a.M)) out = O3S_PLANE_REPEATED;  // (the entries refuse such a table; nothing is read out of range)
#pragma unroll
    for (int q = p + 1; q < kPlNMax; ++q)
      if (q < n && idx[p] == idx[q]) out = O3S_PLANE_REPEATED;
  }
  double pl[4] = {0.0, 0.0, 0.0, 0.0};
  if (out == O3S_PLANE_PASS) {
    double p[9];
    bool fin = true;
#pragma unroll
    for (int v = 0; v < 3; ++v)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[3 * v + c] = pts[3 * (size_t)idx[v] + c];
        fin = fin && isfinite(p[3 * v + c]);
      }
    if (!fin) {
      out = O3S_PLANE_NONFINITE;
    } else {
      const double e0x = p[3] - p[0], e0y = p[4] - p[1], e0z = p[5] - p[2];
      const double e1x = p[6] - p[0], e1y = p[7] - p[1], e1z = p[8] - p[2];
      const double nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
      const double norm = sqrt((nx * nx + ny * ny) + nz * nz);
      if (norm == 0.0) {
        out = O3S_PLANE_DEGENERATE;
      } else if (!isfinite(norm)) {
        out = O3S_PLANE_NONFINITE;  // finite points whose cross product overflows: no plane either
      } else {
        pl[0] = nx / norm, pl[1] = ny / norm, pl[2] = nz / norm;
        pl[3] = -((pl[0] * p[0] + pl[1] * p[1]) + pl[2] * p[2]);
      }
    }
  }
  outcome[slot] = out;
#pragma unroll
  for (int k = 0; k < 4; ++k) planes[(size_t)slot * 4 + k] = pl[k];
}

// Block (x, y): points of chunk x (the long axis of the grid), hypotheses blockDim.x * y .. + blockDim.x - 1 of the batch.  n_in and err
// accumulate in point order.
__global__ void __launch_bounds__(kPlEvalBlockMax) k_pl_eval(const double* __restrict__ pts, long long M, double thr, long long itr0,
                                                             const PlaneHeader* __restrict__ hdr, int count, const double* __restrict__ planes,
                                                             uint32_t* __restrict__ part_n /*[chunks][count]*/, double* __restrict__ part_e) {
  __shared__ double s_p[kPlChunk * 3];
  if (hdr && itr0 >= hdr->est_k) return;  // uniform: in front of the barrier
  const int slot = blockIdx.y * blockDim.x + threadIdx.x;
  const double4 pl = reinterpret_cast<const double4*>(planes)[slot < count ? slot : count - 1];
  const long long k0 = (long long)blockIdx.x * kPlChunk;
  const int nk = (int)(M - k0 < (long long)kPlChunk ? M - k0 : (long long)kPlChunk);
  for (int e = threadIdx.x; e < nk * 3; e += blockDim.x) s_p[e] = pts[(size_t)k0 * 3 + e];
  __syncthreads();
  uint32_t cnt = 0u;
  double acc = 0.0;
#pragma unroll 8
  for (int u = 0; u < nk; ++u) {
    const double d = pl_dist(pl.x, pl.y, pl.z, pl.w, s_p[3 * u], s_p[3 * u + 1], s_p[3 * u + 2]);
    if (d < thr) {
      cnt += 1u;
      acc = acc + d;
    }
  }
  if (slot < count) {
    part_n[(size_t)blockIdx.x * count + slot] = cnt;
    part_e[(size_t)blockIdx.x * count + slot] = acc;
  }
}

// the chunks of a hypothesis added up in ascending order: the documented order of the err sum.  Zeros where the outcome is not PASS.
// The loads of kPlFoldAhead chunks go out together, then their adds run in order: the chain is as long as before, the waiting is not
__global__ void __launch_bounds__(kPlFoldBlock) k_pl_fold(long long itr0, const PlaneHeader* __restrict__ hdr, int count, int chunks,
                                                          const int32_t* __restrict__ outcome, const uint32_t* __restrict__ part_n,
                                                          const double* __restrict__ part_e, uint32_t* __restrict__ sv_n, double* __restrict__ sv_e) {
  if (hdr && itr0 >= hdr->est_k) return;
  const int i = blockIdx.x * kPlFoldBlock + threadIdx.x;
  if (i >= count) return;
  uint32_t n = 0u;
  double e = 0.0;
  if (outcome[i] == O3S_PLANE_PASS) {
    int c = 0;
    for (; c + kPlFoldAhead <= chunks; c += kPlFoldAhead) {
      uint32_t pn[kPlFoldAhead];
      double pe[kPlFoldAhead];
#pragma unroll
      for (int u = 0; u < kPlFoldAhead; ++u) {
        pn[u] = part_n[(size_t)(c + u) * count + i];
        pe[u] = part_e[(size_t)(c + u) * count + i];
      }
#pragma unroll
      for (int u = 0; u < kPlFoldAhead; ++u) {
        n += pn[u];
        e = e + pe[u];
      }
    }
    for (; c < chunks; ++c) {
      n += part_n[(size_t)c * count + i];
      e = e + part_e[(size_t)c * count + i];
    }
  }
  sv_n[i] = n;
  sv_e[i] = e;
}

// One wave: the selection rule over the batch's PASS slots in itr order, on the header (k_ransac_select's walk; fitness = n / M,
// rmse = err / sqrt(n)).
__global__ void __launch_bounds__(64) k_pl_select(PlaneArgs a, PlaneHeader* __restrict__ hdr, long long itr0, int count, const int32_t* __restrict__ outcome,
                                                  const uint32_t* __restrict__ sv_n, const double* __restrict__ sv_e, const double* __restrict__ planes) {
  const int lane = threadIdx.x;
  long long est_k = hdr->est_k;
  if (itr0 >= est_k) return;
  double best_fit = hdr->fitness, best_rmse = hdr->rmse, best_e = hdr->err;
  long long best_n = hdr->n_in, best_itr = hdr->best_itr, evaluated = hdr->evaluated;
  int best_slot = -1;
  bool done = false;
  for (int base = 0; base < count && !done; base += 64) {
    const int slot = base + lane;
    const bool in_batch = slot < count;
    const bool valid = in_batch && outcome[slot] == O3S_PLANE_PASS;
    const long long itr = itr0 + slot;
    const uint32_t n = valid ? sv_n[slot] : 0u;
    const double e = valid ? sv_e[slot] : 0.0;
    const double fit = (double)n / (double)a.M;
    const double rmse = n ? e / sqrt((double)n) : 0.0;
    int pos = 0;
    for (;;) {
      const bool in_range = valid && lane >= pos && itr < est_k;
      const bool better = in_range && (fit > best_fit || (fit == best_fit && rmse < best_rmse));
      const unsigned long long m_better = __ballot(better), m_range = __ballot(in_range);
      if (m_better == 0ull) {
        evaluated += __popcll(m_range);
        if (__ballot(in_batch && lane >= pos && !(itr < est_k)) != 0ull) done = true;  // the first itr >= est_k ends the loop
        break;
      }
      const int l = __ffsll((long long)m_better) - 1;
      evaluated += __popcll(m_range & ((2ull << l) - 1ull));
      best_fit = __shfl(fit, l, 64);
      best_rmse = __shfl(rmse, l, 64);
      best_e = __shfl(e, l, 64);
      best_n = (long long)__shfl((int)n, l, 64);
      best_itr = __shfl(itr, l, 64);
      best_slot = __shfl(slot, l, 64);
      double p = best_fit;
      for (int j = 1; j < a.n; ++j) p = p * best_fit;
      const double ek = log(1.0 - a.confidence) / log(1.0 - p);
      if (ek < (double)est_k) est_k = (long long)ceil(ek);
      pos = l + 1;
    }
  }
  if (lane == 0) {
    hdr->est_k = est_k;
    hdr->best_itr = best_itr;
    hdr->evaluated = evaluated;
    hdr->n_in = best_n;
    hdr->err = best_e;
    hdr->fitness = best_fit;
    hdr->rmse = best_rmse;
  }
  if (best_slot >= 0 && lane < 4) hdr->plane[lane] = planes[(size_t)best_slot * 4 + lane];
}

// the winner's inliers: flags in point order (the arithmetic of k_pl_eval), with the per-block counts for the one-launch scan
__global__ void __launch_bounds__(kB) k_pl_inlier_flags(const double* __restrict__ pts, long long M, double thr, const PlaneHeader* __restrict__ hdr,
                                                        uint32_t* __restrict__ flag, uint32_t* __restrict__ blk_cnt) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  uint32_t f = 0u;
  if (i < M) {
    f = (hdr->best_itr >= 0 && pl_dist(hdr->plane[0], hdr->plane[1], hdr->plane[2], hdr->plane[3], pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]) < thr) ? 1u : 0u;
    flag[i] = f;
  }
  put_block_count(f, blk_cnt);
}
// off[M] and the header's n_list = the length of the inlier list, whichever scan ran
__global__ void k_pl_list_total(const uint32_t* __restrict__ flag, uint32_t* __restrict__ off, long long M, PlaneHeader* __restrict__ hdr) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t total = off[M - 1] + flag[M - 1];
  off[M] = total;
  hdr->n_list = (long long)total;
}

// GetPlaneFromPoints, first half: block c stages chunk c of the inlier list (lp: the list's points, compacted) in LDS, then lane v sums
// component v of the chunk sequentially from 0.0 — kCov false: the three coordinates (part: [chunk][3]); true: the six products
// xx, xy, xz, yy, yz, zz of r = p - centroid (part: [chunk][6]).  The grid covers the cloud; blocks past the list return at once
template <bool kCov>
__global__ void __launch_bounds__(64) k_pl_refit_part(const double* __restrict__ lp, const PlaneHeader* __restrict__ hdr, double* __restrict__ part) {
  __shared__ double s_q[kPlChunk * 3];
  const long long L = hdr->n_list;
  const long long c = blockIdx.x;
  const long long k0 = c * kPlChunk;
  if (k0 >= L) return;  // uniform: in front of the barrier
  const int nk = (int)(L - k0 < (long long)kPlChunk ? L - k0 : (long long)kPlChunk);
  for (int e = threadIdx.x; e < nk * 3; e += 64) s_q[e] = lp[3 * (size_t)k0 + e];
  __syncthreads();
  const int v = threadIdx.x;
  if (v >= (kCov ? 6 : 3)) return;
  double s = 0.0;
  if (!kCov) {
#pragma unroll 8
    for (int u = 0; u < nk; ++u) s = s + s_q[3 * u + v];
    part[3 * c + v] = s;
  } else {
    const int i = v < 3 ? 0 : (v < 5 ? 1 : 2), j = v < 3 ? v : (v < 5 ? v - 2 : 2);
    const double ci = hdr->cen[i], cj = hdr->cen[j];
#pragma unroll 8
    for (int u = 0; u < nk; ++u) s = s + (s_q[3 * u + i] - ci) * (s_q[3 * u + j] - cj);
    part[6 * c + v] = s;
  }
}
// ... second half: one wave, lane v < 3 (or 6) adds component v of the chunk sums up in ascending chunk order; then the centroid,
// or the model from the six sums
template <bool kCov>
__global__ void __launch_bounds__(64) k_pl_refit_fold(const double* __restrict__ part, PlaneHeader* __restrict__ hdr) {
  const long long L = hdr->n_list;
  if (L <= 0 || hdr->best_itr < 0) return;  // (uniform)
  const long long chunks = (L + kPlChunk - 1) / kPlChunk;
  const int lane = threadIdx.x, nv = kCov ? 6 : 3;
  double s = 0.0;
  if (lane < nv) {
    long long c = 0;
    for (; c + kPlFoldAhead <= chunks; c += kPlFoldAhead) {
      double pv[kPlFoldAhead];
#pragma unroll
      for (int u = 0; u < kPlFoldAhead; ++u) pv[u] = part[(size_t)nv * (c + u) + lane];
#pragma unroll
      for (int u = 0; u < kPlFoldAhead; ++u) s = s + pv[u];
    }
    for (; c < chunks; ++c) s = s + part[(size_t)nv * c + lane];
  }
  if (!kCov) {
    if (lane < 3) hdr->cen[lane] = s / (double)L;
    return;
  }
  const double xx = __shfl(s, 0, 64), xy = __shfl(s, 1, 64), xz = __shfl(s, 2, 64), yy = __shfl(s, 3, 64), yz = __shfl(s, 4, 64), zz = __shfl(s, 5, 64);
  if (lane != 0) return;
  const double det_x = yy * zz - yz * yz, det_y = xx * zz - xz * xz, det_z = xx * yy - xy * xy;
  double a, b, c;
  if (det_x > det_y && det_x > det_z) {
    a = det_x, b = xz * yz - xy * zz, c = xy * yz - xz * yy;
  } else if (det_y > det_z) {
    a = xz * yz - xy * zz, b = det_y, c = xy * xz - yz * xx;
  } else {
    a = xy * yz - xz * yy, b = xy * xz - yz * xx, c = det_z;
  }
  const double norm = sqrt((a * a + b * b) + c * c);
  if (norm == 0.0) {
    hdr->model[0] = hdr->model[1] = hdr->model[2] = hdr->model[3] = 0.0;
    return;
  }
  a = a / norm, b = b / norm, c = c / norm;
  hdr->model[0] = a, hdr->model[1] = b, hdr->model[2] = c;
  hdr->model[3] = -((a * hdr->cen[0] + b * hdr->cen[1]) + c * hdr->cen[2]);
}

// The peel between two planes: a point of the list gets the plane's number at its input index; the others move up, in order, into
// the next cloud with their input indices (orig null: the cloud is still the input, index = position).
__global__ void __launch_bounds__(kB) k_pl_peel(const double* __restrict__ pts, const uint32_t* __restrict__ orig, long long M, const uint32_t* __restrict__ flag,
                                                const uint32_t* __restrict__ off, int32_t plane, int32_t* __restrict__ labels, double* __restrict__ next_pts,
                                                uint32_t* __restrict__ next_orig) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  if (i >= M) return;
  const uint32_t o = orig ? orig[i] : (uint32_t)i;
  if (flag[i]) {
    if (labels) labels[o] = plane;
    return;
  }
  if (!next_pts) return;  // the last plane: nothing follows
  const size_t r = (size_t)i - off[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) next_pts[3 * r + c] = pts[3 * i + c];
  next_orig[r] = o;
}

// keep = no plane took the point, in input order, with the per-block counts for the one-launch scan
__global__ void __launch_bounds__(kB) k_pl_keep(const int32_t* __restrict__ labels, long long N, uint32_t* __restrict__ keep, uint32_t* __restrict__ blk_cnt) {
  const long long i = (long long)blockIdx.x * kB + threadIdx.x;
  uint32_t f = 0u;
  if (i < N) {
    f = labels[i] < 0 ? 1u : 0u;
    keep[i] = f;
  }
  put_block_count(f, blk_cnt);
}

}  // namespace o3s_cloud
}  // namespace
