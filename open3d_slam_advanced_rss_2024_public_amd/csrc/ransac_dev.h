// ransac_dev.h — device side of RegistrationRANSACBasedOnCorrespondence (contract: include/o3s_registration.h, "RANSAC").
// Iteration `itr` is a pure function of (seed, itr): a lane of k_ransac_hyp draws (or reads) its sample, runs the edge-length
// check, Eigen::umeyama on the sample and the distance check; the survivors of a batch are compacted in itr order, evaluated
// over all K correspondences (k_ransac_eval: T in registers, the pair records through LDS as a broadcast, sums in
// correspondence order per chunk of kRansacChunk pairs), folded chunk by chunk in ascending order, and one wave applies the
// serial selection rule to the device-resident header.  fp64, no FMA contraction, no float atomics.
#pragma once
#include "cloud_dev.h"

#pragma clang fp contract(off)

namespace {
namespace o3s_cloud {

constexpr int kRansacNMax = 8;
constexpr int kRansacBatch = 16384;  // iterations per batch; the hooks build reads O3S_RANSAC_BATCH per call
constexpr int kRansacChunk = 512;    // correspondences per evaluation chunk: part of the contract (the order of the err2 sum)
constexpr int kRansacEvalBlock = 64;
constexpr int kRansacAhead = 4;      // batches issued ahead of the last est_k the host has seen
constexpr int kRansacSlotWords = 8;  // one post slot of the common layout per batch in flight

enum { kRansacPass = 0, kRansacRepeated = 1, kRansacEdge = 2, kRansacDistance = 3 };

struct RansacHeader {  // device resident: the best so far and the serial rule's est_k
  long long est_k, best_itr, evaluated, n_in;
  double err2, fitness, rmse;
  double T[12];  // rows of [R | t]
  uint32_t bad;  // a correspondence named a point that does not exist
  uint32_t pad;
};
struct RansacArgs {
  int n, check_edge, check_dist;
  double sim, thr, max_dist, confidence;
  unsigned long long seed;
  long long K;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * (unsigned long long)c0, p1 = 0xCD9E8D57ull * (unsigned long long)c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0, c1 = n1, c2 = n2, c3 = n3;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// d = |T s - t| with the products and sums in this order; the pair is an inlier when d < max_dist and adds d * d
__device__ __forceinline__ double ransac_dist(const double T[12], const double* r) {
  const double px = ((T[0] * r[0] + T[1] * r[1]) + T[2] * r[2]) + T[3];
  const double py = ((T[4] * r[0] + T[5] * r[1]) + T[6] * r[2]) + T[7];
  const double pz = ((T[8] * r[0] + T[9] * r[1]) + T[10] * r[2]) + T[11];
  const double dx = px - r[3], dy = py - r[4], dz = pz - r[5];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

__global__ void k_ransac_init(RansacHeader* __restrict__ h, long long max_iteration) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  h->est_k = max_iteration;
  h->best_itr = -1;
  h->evaluated = 0;
  h->n_in = 0;
  h->err2 = h->fitness = h->rmse = 0.0;
  for (int k = 0; k < 12; ++k) h->T[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
  h->bad = 0u;
}

// the K correspondences as (s, t) coordinate records: nothing chases an index afterwards
__global__ void __launch_bounds__(kB) k_ransac_gather(const double* __restrict__ src, long long ns, const double* __restrict__ tgt, long long nt,
                                                      const int32_t* __restrict__ pairs, long long K, double* __restrict__ rec,
                                                      RansacHeader* __restrict__ h) {
  const long long k = (long long)blockIdx.x * kB + threadIdx.x;
  if (k >= K) return;
  const long long i = pairs[2 * k], j = pairs[2 * k + 1];
  const bool ok = i >= 0 && i < ns && j >= 0 && j < nt;
  if (!ok) atomicOr(&h->bad, 1u);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    rec[6 * k + a] = ok ? src[3 * i + a] : 0.0;
    rec[6 * k + 3 + a] = ok ? tgt[3 * j + a] : 0.0;
  }
}

// One lane per iteration of the batch [itr0, itr0 + count): flag (1: passed), outcome and T (12 doubles) at slot itr - itr0.
__global__ void __launch_bounds__(kB) k_ransac_hyp(RansacArgs a, const double* __restrict__ rec, const int32_t* __restrict__ table, long long itr0,
                                                   int count, const RansacHeader* __restrict__ hdr, uint32_t* __restrict__ flag,
                                                   int32_t* __restrict__ outcome, double* __restrict__ Tout) {
  if (hdr && itr0 >= hdr->est_k) return;  // the serial loop has ended in front of this batch
  const int slot = blockIdx.x * kB + threadIdx.x;
  if (slot >= count) return;
  const long long itr = itr0 + slot;
  const int n = a.n;
  int idx[kRansacNMax];
  if (table) {
#pragma unroll
    for (int j = 0; j < kRansacNMax; ++j) idx[j] = j < n ? table[itr * n + j] : -1 - j;
  } else {
#pragma unroll
    for (int q = 0; q < kRansacNMax / 4; ++q) {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (q * 4 < n) philox4x32_10((uint32_t)itr, (uint32_t)((unsigned long long)itr >> 32), (uint32_t)q, 0u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32), w);
#pragma unroll
      for (int u = 0; u < 4; ++u) idx[q * 4 + u] = q * 4 + u < n ? (int)(((unsigned long long)w[u] * (unsigned long long)a.K) >> 32) : -1 - (q * 4 + u);
    }
  }
  int out = kRansacPass;
#pragma unroll
  for (int p = 0; p < kRansacNMax; ++p) {
    if (p < n && (idx[p] < 0 || (long long)idx[p] >= a.K)) out = kRansacRepeated;  // a row that names no correspondence defines no motion either
#pragma unroll
    for (int q = p + 1; q < kRansacNMax; ++q)
      if (q < n && idx[p] == idx[q]) out = kRansacRepeated;
  }
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = 0.0;
  if (out == kRansacPass && a.check_edge) {
#pragma unroll
    for (int p = 0; p < kRansacNMax; ++p) {
      if (p >= n) continue;
      const double* rp = rec + 6 * (size_t)idx[p];
#pragma unroll
      for (int q = p + 1; q < kRansacNMax; ++q) {
        if (q >= n) continue;
        const double* rq = rec + 6 * (size_t)idx[q];
        const double sx = rp[0] - rq[0], sy = rp[1] - rq[1], sz = rp[2] - rq[2];
        const double tx = rp[3] - rq[3], ty = rp[4] - rq[4], tz = rp[5] - rq[5];
        const double ds = sqrt((sx * sx + sy * sy) + sz * sz), dt = sqrt((tx * tx + ty * ty) + tz * tz);
        if (ds < dt * a.sim || dt < ds * a.sim) out = kRansacEdge;
      }
    }
  }
  if (out == kRansacPass) {
    // Eigen::umeyama(source sample, target sample, false): means, sigma = (1/n) sum (t - mt)(s - ms)^T, R = U S V^T, t = mt - R ms
    const double inv_n = 1.0 / (double)n;
    double ms[3] = {0, 0, 0}, mt[3] = {0, 0, 0};
#pragma unroll
    for (int p = 0; p < kRansacNMax; ++p) {
      if (p >= n) continue;
      const double* rp = rec + 6 * (size_t)idx[p];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ms[c] += rp[c];
        mt[c] += rp[3 + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ms[c] *= inv_n;
      mt[c] *= inv_n;
    }
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
    for (int p = 0; p < kRansacNMax; ++p) {
      if (p >= n) continue;
      const double* rp = rec + 6 * (size_t)idx[p];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r][c] += (rp[3 + r] - mt[r]) * (rp[c] - ms[c]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) A[r][c] *= inv_n;
    // one-sided (Hestenes) Jacobi on the columns of sigma, as h_svd3 (o3d_icp_impl.h): A -> U diag(sv), V accumulates the rotations
    for (int sweep = 0; sweep < 64; ++sweep) {
      bool rotated = false;
#pragma unroll
      for (int pq = 0; pq < 3; ++pq) {
        const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
        double al = 0, be = 0, ga = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          al += A[i][p] * A[i][p];
          be += A[i][q] * A[i][q];
          ga += A[i][p] * A[i][q];
        }
        if (ga == 0.0 || !(fabs(ga) > 1e-15 * sqrt(al * be))) continue;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        if (t == 0.0) continue;
        rotated = true;
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double ap = A[i][p], aq = A[i][q];
          A[i][p] = cs * ap - sn * aq;
          A[i][q] = sn * ap + cs * aq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = cs * vp - sn * vq;
          V[i][q] = sn * vp + cs * vq;
        }
      }
      if (!rotated) break;
    }
    double nrm[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nrm[c] = sqrt((A[0][c] * A[0][c] + A[1][c] * A[1][c]) + A[2][c] * A[2][c]);
    // singular values descending: a three-element network on the columns (strict `<`: equal columns keep their order)
#pragma unroll
    for (int st = 0; st < 3; ++st) {
      const int p = st == 1 ? 1 : 0, q = st == 1 ? 2 : 1;
      if (nrm[p] < nrm[q]) {
        double x = nrm[p];
        nrm[p] = nrm[q];
        nrm[q] = x;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          x = A[i][p], A[i][p] = A[i][q], A[i][q] = x;
          x = V[i][p], V[i][p] = V[i][q], V[i][q] = x;
        }
      }
    }
    // U's third column is u0 x u1 and S = diag(1, 1, sign det V): the same R as Eigen's U S V^T with S(2) = sign(det U det V) whenever
    // sigma has rank >= 2 — and a sample of three points never has rank 3, so the third column of A is never divided by its norm
    double u0[3], u1[3], u2[3];
    if (nrm[0] > 0.0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) u0[i] = A[i][0] / nrm[0];
    } else {
      u0[0] = 1.0, u0[1] = 0.0, u0[2] = 0.0;
    }
    if (nrm[1] > 0.0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) u1[i] = A[i][1] / nrm[1];
    } else {  // rank <= 1 (a flagged sample): a unit axis not along u0, made orthogonal to it
      const bool first = fabs(u0[0]) < 0.9;
      const double e[3] = {first ? 1.0 : 0.0, first ? 0.0 : 1.0, 0.0};
      const double dt = first ? u0[0] : u0[1];
      double l = 0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        u1[i] = e[i] - dt * u0[i];
        l += u1[i] * u1[i];
      }
      l = sqrt(l);
#pragma unroll
      for (int i = 0; i < 3; ++i) u1[i] /= l;
    }
    u2[0] = u0[1] * u1[2] - u0[2] * u1[1];
    u2[1] = u0[2] * u1[0] - u0[0] * u1[2];
    u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
    const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                        V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
    const double sg = detV < 0 ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) T[4 * r + c] = (u0[r] * V[c][0] + u1[r] * V[c][1]) + sg * u2[r] * V[c][2];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) T[4 * r + 3] = mt[r] - ((T[4 * r] * ms[0] + T[4 * r + 1] * ms[1]) + T[4 * r + 2] * ms[2]);
    if (a.check_dist) {
#pragma unroll
      for (int p = 0; p < kRansacNMax; ++p) {
        if (p >= n) continue;
        if (ransac_dist(T, rec + 6 * (size_t)idx[p]) > a.thr) out = kRansacDistance;
      }
    }
  }
  flag[slot] = out == kRansacPass ? 1u : 0u;
  outcome[slot] = out;
#pragma unroll
  for (int k = 0; k < 12; ++k) Tout[(size_t)slot * 12 + k] = T[k];
}

// the batch's survivors in itr order (off: the exclusive scan of flag over count + 1 words, off[count] = their number)
__global__ void __launch_bounds__(kB) k_ransac_scatter(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off, int count, long long itr0,
                                                       const RansacHeader* __restrict__ hdr, int32_t* __restrict__ surv) {
  if (hdr && itr0 >= hdr->est_k) return;
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i < count && flag[i]) surv[off[i]] = i;
}

// Block (x, y): survivors 64 x .. 64 x + 63, correspondences of chunk y.  A lane keeps its hypothesis' T in registers, the chunk's
// records sit in LDS and every lane reads the same word; n_in and err2 accumulate in correspondence order.
__global__ void __launch_bounds__(kRansacEvalBlock) k_ransac_eval(const double* __restrict__ rec, long long K, double max_dist, long long itr0,
                                                                  const RansacHeader* __restrict__ hdr, const uint32_t* __restrict__ off, int count,
                                                                  const int32_t* __restrict__ surv, const double* __restrict__ Tin,
                                                                  uint32_t* __restrict__ part_n /*[chunks][count]*/, double* __restrict__ part_e) {
  __shared__ double s_rec[kRansacChunk * 6];
  if (hdr && itr0 >= hdr->est_k) return;
  const uint32_t n_surv = off[count];
  if ((uint32_t)blockIdx.x * kRansacEvalBlock >= n_surv) return;  // uniform: in front of every barrier
  const uint32_t i = blockIdx.x * kRansacEvalBlock + threadIdx.x;
  const int slot = surv[i < n_surv ? i : n_surv - 1];
  double T[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) T[k] = Tin[(size_t)slot * 12 + k];
  const long long k0 = (long long)blockIdx.y * kRansacChunk;
  const int nk = (int)(K - k0 < (long long)kRansacChunk ? K - k0 : (long long)kRansacChunk);
  for (int e = threadIdx.x; e < nk * 6; e += kRansacEvalBlock) s_rec[e] = rec[(size_t)k0 * 6 + e];
  __syncthreads();
  uint32_t cnt = 0u;
  double acc = 0.0;
  for (int u = 0; u < nk; ++u) {
    const double d = ransac_dist(T, s_rec + 6 * u);
    if (d < max_dist) {
      cnt += 1u;
      acc = acc + d * d;
    }
  }
  if (i < n_surv) {
    part_n[(size_t)blockIdx.y * count + i] = cnt;
    part_e[(size_t)blockIdx.y * count + i] = acc;
  }
}

// the chunks of a survivor added up in ascending order: the documented order of the err2 sum
__global__ void __launch_bounds__(kB) k_ransac_fold(long long itr0, const RansacHeader* __restrict__ hdr, const uint32_t* __restrict__ off, int count,
                                                    int chunks, const int32_t* __restrict__ surv, const uint32_t* __restrict__ part_n,
                                                    const double* __restrict__ part_e, uint32_t* __restrict__ sv_n, double* __restrict__ sv_e,
                                                    long long* __restrict__ slot_n /*nullable*/, double* __restrict__ slot_e) {
  if (hdr && itr0 >= hdr->est_k) return;
  const uint32_t i = blockIdx.x * kB + threadIdx.x;
  if (i >= off[count]) return;
  uint32_t n = 0u;
  double e = 0.0;
  for (int c = 0; c < chunks; ++c) {
    n += part_n[(size_t)c * count + i];
    e = e + part_e[(size_t)c * count + i];
  }
  sv_n[i] = n;
  sv_e[i] = e;
  if (slot_n) {
    slot_n[surv[i]] = (long long)n;
    slot_e[surv[i]] = e;
  }
}

// One wave: rule 6 over the batch's survivors in itr order, on the header; then (est_k) goes to the host through the post.
__global__ void __launch_bounds__(64) k_ransac_select(RansacArgs a, RansacHeader* __restrict__ hdr, long long itr0, const uint32_t* __restrict__ off,
                                                      int count, const int32_t* __restrict__ surv, const uint32_t* __restrict__ sv_n,
                                                      const double* __restrict__ sv_e, const double* __restrict__ Tin, uint32_t* __restrict__ mailbox,
                                                      uint32_t seq) {
  const int lane = threadIdx.x;
  long long est_k = hdr->est_k;
  if (itr0 < est_k) {
    const uint32_t n_surv = off[count];
    double best_fit = hdr->fitness, best_rmse = hdr->rmse, best_e = hdr->err2;
    long long best_n = hdr->n_in, best_itr = hdr->best_itr, evaluated = hdr->evaluated;
    int best_slot = -1;
    bool done = false;
    for (uint32_t base = 0; base < n_surv && !done; base += 64) {
      const uint32_t i = base + lane;
      const bool valid = i < n_surv;
      const int slot = valid ? surv[i] : 0;
      const long long itr = itr0 + slot;
      const uint32_t n = valid ? sv_n[i] : 0u;
      const double e = valid ? sv_e[i] : 0.0;
      const double fit = (double)n / (double)a.K;
      const double rmse = n ? sqrt(e / (double)n) : 0.0;
      int pos = 0;
      for (;;) {
        const bool in_range = valid && lane >= pos && itr < est_k;
        const bool better = in_range && (fit > best_fit || (fit == best_fit && rmse < best_rmse));
        const unsigned long long m_better = __ballot(better), m_range = __ballot(in_range);
        if (m_better == 0ull) {
          evaluated += __popcll(m_range);
          if (__ballot(valid && lane >= pos && !(itr < est_k)) != 0ull) done = true;  // the first itr >= est_k ends the loop
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
      hdr->err2 = best_e;
      hdr->fitness = best_fit;
      hdr->rmse = best_rmse;
    }
    if (best_slot >= 0 && lane < 12) hdr->T[lane] = Tin[(size_t)best_slot * 12 + lane];
  }
  if (mailbox && lane == 0) {
    const unsigned long long v[1] = {(unsigned long long)est_k};
    post(mailbox, seq, kPostVals, v);
  }
}

// the winner's inliers: flags in correspondence order (the arithmetic of k_ransac_eval), then a scan and a scatter
__global__ void __launch_bounds__(kB) k_ransac_inlier_flags(const double* __restrict__ rec, long long K, double max_dist, const RansacHeader* __restrict__ hdr,
                                                            uint32_t* __restrict__ flag) {
  const long long k = (long long)blockIdx.x * kB + threadIdx.x;
  if (k >= K) return;
  double T[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) T[j] = hdr->T[j];
  flag[k] = (hdr->best_itr >= 0 && ransac_dist(T, rec + 6 * k) < max_dist) ? 1u : 0u;
}
__global__ void __launch_bounds__(kB) k_ransac_inlier_scatter(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ off, long long K,
                                                              const int32_t* __restrict__ pairs, int32_t* __restrict__ out) {
  const long long k = (long long)blockIdx.x * kB + threadIdx.x;
  if (k >= K || !flag[k]) return;
  out[2 * (size_t)off[k]] = pairs[2 * k];
  out[2 * (size_t)off[k] + 1] = pairs[2 * k + 1];
}

}  // namespace o3s_cloud
}  // namespace
