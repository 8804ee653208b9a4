// localizability_dev.h — the four kernels of the localizability analysis (include/localizability/o3s_localizability.h holds the
// arithmetic contract).  They hang behind the iteration that ended the chain the way k_cov does: the same kept-pair predicate, the
// same matched-normal stream, the same points per lane, the same two sources of pairs
//   chain   (ext_p == null) the state the chain ended with: p = T_prev * reading - mp, n = matched normal
//   module  (ext_p != null) two 3 x K arrays of pairs that are already centred (o3s_localizability_estimate)
//   k_loc_hessian   12 fp64 partial sums per block: the upper triangles of A_t = sum n n^T and A_r = sum c c^T
//   k_loc_eig       one block: folds them, two lanes (one per 3 x 3 block, in two waves) run the Jacobis and leave the six directions in
//                   device memory
//   k_loc_contrib   the second pass: 12 fp64 sums and 7 counts per block (six n_strong, the pairs taken); k_loc_contrib_partial is
//                   the same body with the strong-pair sums of include/degeneracy/o3s_degeneracy_partial.h beside them
//   k_loc_post      one block: folds them, applies the categories, stamps the clock and posts (host_post.h)
// Nothing per pair is stored: pass 2 forms the centred pair again exactly as pass 1 did.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "icp_kernels.h"

#pragma clang fp contract(off)

namespace o3s {
namespace kern {

constexpr int kLocTri = 6;                // upper triangle of a 3 x 3
constexpr int kLocSums = 2 * kLocTri;     // pass 1: A_t then A_r;  pass 2: sum_all[6] then sum_strong[6]
constexpr int kLocCounts = 7;             // pass 2: n_strong[6], then the pairs taken
constexpr int kLocDirs = 6 + 18;          // k_loc_eig's output: eval[6], evec[6][3]
constexpr int kLocMaxSweeps = 16;         // the Jacobi's bound (it converges quadratically: a 3 x 3 needs 4-6)
// what k_loc_post posts, 8-byte values: eval[6] evec[18] sum_all[6] sum_strong[6] n_strong[6] category[6] kept centre[3] and the
// two wall_clock64 stamps of the pass (k_loc_hessian's start, k_loc_post's end); integers as bit patterns
constexpr int kLocPostVals = kLocDirs + kLocSums + 6 + 6 + 1 + 3 + 2;

struct LocThresholds {
  double filter_min, strong_min, sum_all_min, sum_strong_min, sum_partial_min;
};

// the slot's pair as both passes see it; false: the slot is not a kept pair
__device__ __forceinline__ bool loc_pair(bool chain, int i, const float* __restrict__ rx, const float* __restrict__ ry, const float* __restrict__ rz,
                                         const float4* __restrict__ mn, const int32_t* __restrict__ pos, const float* __restrict__ d2, float limit,
                                         float max_out_r2, const float* T, float mpx, float mpy, float mpz, const float* __restrict__ ext_p,
                                         const float* __restrict__ ext_n, float (&p)[3], float (&n)[3]) {
  if (chain) {
    if (!kept_pair(pos[i], d2[i], limit, max_out_r2)) return false;
    const float4 nn = mn[i];
    const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);
    float q[3];  // (the centred reference point: not used here, and not loaded)
    cov_chain_pair(T, rx[i], ry[i], rz[i], none, mpx, mpy, mpz, 0.f, 0.f, 0.f, p, q);
    n[0] = nn.x, n[1] = nn.y, n[2] = nn.z;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[c] = ext_p[3 * (size_t)i + c];
      n[c] = ext_n[3 * (size_t)i + c];
    }
  }
  return true;
}
// c = p x n, fp32, left to right (the translation unit is compiled without FMA contraction)
__device__ __forceinline__ void loc_cross(const float (&p)[3], const float (&n)[3], float (&c)[3]) {
  c[0] = p[1] * n[2] - p[2] * n[1];
  c[1] = p[2] * n[0] - p[0] * n[2];
  c[2] = p[0] * n[1] - p[1] * n[0];
}
// the chain's state as k_cov reads it.  live (the degeneracy-aware chain, degeneracy_dev.h): the kernel runs INSIDE an iteration, in
// front of k_solve, so the pose its pairs were formed under is still T_iter (the header) — k_solve moves those very words to
// T_prev, which is what the pass behind the chain reads: the same bits either way.  false: the chain has ended, or an earlier
// kernel of this iteration failed it, and the caller returns at once
__device__ __forceinline__ bool loc_chain_state(bool chain, int live, const IcpState* __restrict__ st, float (&T)[16], float& limit, float& mpx,
                                                float& mpy, float& mpz) {
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
  limit = kInfF, mpx = mpy = mpz = 0.f;
  if (chain) {
    const float hv = hdr_load(st);
    if (live) {  // uniform
      if (hdr_i(hv, H_DONE) || hdr_i(hv, H_STATUS)) return false;
#pragma unroll
      for (int k = 0; k < 16; ++k) T[k] = hdr_f(hv, k);
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) T[k] = st->T_prev[k];
    }
    limit = hdr_f(hv, H_LIMIT);
    mpx = hdr_f(hv, H_MP), mpy = hdr_f(hv, H_MP + 1), mpz = hdr_f(hv, H_MP + 2);
  }
  return true;
}

__global__ void __launch_bounds__(kBlock) k_loc_hessian(const float* __restrict__ rx, const float* __restrict__ ry, const float* __restrict__ rz, int N,
                                                        const float4* __restrict__ mn, const int32_t* __restrict__ pos, const float* __restrict__ d2,
                                                        float max_out_r2, const IcpState* __restrict__ st, const float* __restrict__ ext_p,
                                                        const float* __restrict__ ext_n, double* __restrict__ part /*[12][grid]*/,
                                                        unsigned long long* __restrict__ t_start /*wall_clock64 of block 0's start*/,
                                                        int live /*inside an iteration: loc_chain_state*/) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *t_start = wall_clock64();
  using Sum = BlockSum<kLocTri, kBlock>;  // two passes of six
  __shared__ double s_a[Sum::kWordsA];
  __shared__ double s_b[Sum::kWordsB];
  const bool chain = ext_p == nullptr;  // uniform
  float T[16], limit, mpx, mpy, mpz;
  if (!loc_chain_state(chain, live, st, T, limit, mpx, mpy, mpz)) return;
  double accT[kLocTri], accR[kLocTri];
#pragma unroll
  for (int c = 0; c < kLocTri; ++c) accT[c] = accR[c] = 0.0;
  for (int base = blockIdx.x * (kBlock * kNePPT) + threadIdx.x; base < N; base += gridDim.x * (kBlock * kNePPT)) {
#pragma unroll
    for (int u = 0; u < kNePPT; ++u) {
      const int i = base + u * kBlock;
      if (i >= N) continue;
      float p[3], n[3], c[3];
      if (!loc_pair(chain, i, rx, ry, rz, mn, pos, d2, limit, max_out_r2, T, mpx, mpy, mpz, ext_p, ext_n, p, n)) continue;
      loc_cross(p, n, c);
      int t = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = a; b < 3; ++b) {
          accT[t] += (double)n[a] * (double)n[b];  // products of promoted fp32 values: exact
          accR[t] += (double)c[a] * (double)c[b];
          ++t;
        }
      }
    }
  }
  Sum::run(accT, s_a, s_b);
  if (threadIdx.x < kLocTri) part[threadIdx.x * gridDim.x + blockIdx.x] = Sum::total(s_b, threadIdx.x);
  Sum::run(accR, s_a, s_b);  // (its first barrier stands between the totals above and the new segment sums)
  if (threadIdx.x < kLocTri) part[(kLocTri + threadIdx.x) * gridDim.x + blockIdx.x] = Sum::total(s_b, threadIdx.x);
}

// ---- the 3 x 3 eigen step: every element a scalar of its own (compile-time subscripts only: the matrix lives in registers; a
// run-time subscript would put it into scratch, see the note at the top of solve_device.h) -------------------------------------------
struct Sym3 {
  double a00, a01, a02, a11, a12, a22;
};
struct Mat3 {
  double v00, v01, v02, v10, v11, v12, v20, v21, v22;  // v[row][column]; column j is the direction of eigenvalue j
};
// one Jacobi rotation of the pair (p, q); r is the third index: app, aqq, apq the pair's elements, arp, arq the third row's, and
// the pair's two columns of V
__device__ __forceinline__ void loc_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p,
                                           double& v1q, double& v2p, double& v2q) {
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
  const double x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;
  v0p = c * x0 - s * y0, v0q = s * x0 + c * y0;
  v1p = c * x1 - s * y1, v1q = s * x1 + c * y1;
  v2p = c * x2 - s * y2, v2q = s * x2 + c * y2;
}
__device__ __forceinline__ void loc_swap_cols(double& ea, double& eb, double& a0, double& b0, double& a1, double& b1, double& a2, double& b2) {
  if (!(ea > eb)) return;  // strictly greater: the sort is stable
  double t;
  t = ea, ea = eb, eb = t;
  t = a0, a0 = b0, b0 = t;
  t = a1, a1 = b1, b1 = t;
  t = a2, a2 = b2, b2 = t;
}
// unit length, the component of largest magnitude positive (a tie: the lowest index)
__device__ __forceinline__ void loc_orient(double& x, double& y, double& z) {
  const double len = sqrt((x * x + y * y) + z * z);
  x = x / len, y = y / len, z = z / len;
  const double ax = fabs(x), ay = fabs(y), az = fabs(z);
  const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
  if (lead < 0.0) x = -x, y = -y, z = -z;
}
// A (upper triangle 00 01 02 11 12 22) -> eval[3] ascending, evec[3][3] (evec[j] the direction of eval[j])
__device__ __forceinline__ void loc_eig3(const double* __restrict__ tri, double* __restrict__ eval, double* __restrict__ evec) {
  Sym3 A{tri[0], tri[1], tri[2], tri[3], tri[4], tri[5]};
  const double total = ((((fabs(A.a00) + fabs(A.a01)) + fabs(A.a02)) + fabs(A.a11)) + fabs(A.a12)) + fabs(A.a22);
  if (!(total < __builtin_huge_val())) {  // a non-finite sum (NaN fails the comparison too): no Jacobi
    const double nan = __builtin_nan("");
#pragma unroll
    for (int k = 0; k < 3; ++k) eval[k] = nan;
#pragma unroll
    for (int k = 0; k < 9; ++k) evec[k] = nan;
    return;
  }
  Mat3 V{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < kLocMaxSweeps; ++sweep) {
    const double off = (fabs(A.a01) + fabs(A.a02)) + fabs(A.a12);
    const double diag = (fabs(A.a00) + fabs(A.a11)) + fabs(A.a22);
    if (!(off > 8.470329472543003e-22 /*2^-70*/ * diag)) break;  // (a NaN ends the loop as well)
    loc_rotate(A.a00, A.a11, A.a01, A.a02, A.a12, V.v00, V.v01, V.v10, V.v11, V.v20, V.v21);  // (0, 1), third index 2
    loc_rotate(A.a00, A.a22, A.a02, A.a01, A.a12, V.v00, V.v02, V.v10, V.v12, V.v20, V.v22);  // (0, 2), third index 1
    loc_rotate(A.a11, A.a22, A.a12, A.a01, A.a02, V.v01, V.v02, V.v11, V.v12, V.v21, V.v22);  // (1, 2), third index 0
  }
  double e0 = A.a00, e1 = A.a11, e2 = A.a22;
  loc_swap_cols(e0, e1, V.v00, V.v01, V.v10, V.v11, V.v20, V.v21);
  loc_swap_cols(e1, e2, V.v01, V.v02, V.v11, V.v12, V.v21, V.v22);
  loc_swap_cols(e0, e1, V.v00, V.v01, V.v10, V.v11, V.v20, V.v21);
  loc_orient(V.v00, V.v10, V.v20);
  loc_orient(V.v01, V.v11, V.v21);
  loc_orient(V.v02, V.v12, V.v22);
  eval[0] = e0, eval[1] = e1, eval[2] = e2;
  evec[0] = V.v00, evec[1] = V.v10, evec[2] = V.v20;
  evec[3] = V.v01, evec[4] = V.v11, evec[5] = V.v21;
  evec[6] = V.v02, evec[7] = V.v12, evec[8] = V.v22;
}

// The fold of twelve sums (k_loc_eig, k_loc_post, degeneracy_dev.h): component c is folded by wave c % 4 — lane l adds the partials
// of blocks l, l + 64, ... in order, then the wave's DPP tree — so the order is a function of the number of blocks alone (k_cov_post).
__device__ __forceinline__ void loc_fold12(const double* __restrict__ part /*[12][nb]*/, int nb, double* __restrict__ out /*LDS*/) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int c = w; c < kLocSums; c += kBlock / 64) {
    double s = 0.0;
    for (int b = l; b < nb; b += 64) s += part[(size_t)c * nb + b];
    s = wave_sum(s);
    if (l == 0) out[c] = s;
  }
}

// One block: loc_fold12, then the two eigen-decompositions.
__global__ void __launch_bounds__(kBlock) k_loc_eig(const double* __restrict__ part /*[12][nb]*/, int nb, double* __restrict__ dirs /*eval[6], evec[6][3]*/,
                                                    const IcpState* __restrict__ st_live /*non-null: inside an iteration*/) {
  __shared__ double s_sum[kLocSums];
  if (st_live) {  // uniform
    const float hv = hdr_load(st_live);
    if (hdr_i(hv, H_DONE) || hdr_i(hv, H_STATUS)) return;
  }
  loc_fold12(part, nb, s_sum);
  __syncthreads();
  // the two blocks are independent serial chains of fp64 divisions and square roots: one lane each, in two waves, side by side
  if (threadIdx.x == 0) loc_eig3(s_sum, dirs, dirs + 6);
  if (threadIdx.x == 64) loc_eig3(s_sum + kLocTri, dirs + 3, dirs + 6 + 9);
}

// What the flagged instantiation of pass 2 reads and writes on top (include/degeneracy/o3s_degeneracy_partial.h): the matched points
// (chain: the matcher's stream and the centroid mq of the header; module: a third 3 x K array) and a partial region of its own.
struct LocNoPartialIo {};  // the unflagged instantiation carries nothing
struct LocPartialIo {
  const float4* mq;      // chain
  const float* ext_q;    // module
  double* part;          // [12][grid]: num[6] then den[6]
};
// kPartial: the strong-pair sums num_j, den_j of the partially localizable directions, twelve accumulators beside pass 2's own
// (which keep their accumulators, their order and their partial region: the unflagged instantiation is the source it was and gives
// the bits it gave).  Chain sources are live only: the centroid mq is read where k_normal_eq reads it.
template <bool kPartial, class Pio>
__device__ __forceinline__ void loc_contrib_body(const float* __restrict__ rx, const float* __restrict__ ry, const float* __restrict__ rz, int N,
                                                 const float4* __restrict__ mn, const int32_t* __restrict__ pos, const float* __restrict__ d2,
                                                 float max_out_r2, const IcpState* __restrict__ st, const float* __restrict__ ext_p,
                                                 const float* __restrict__ ext_n, const double* __restrict__ dirs, double filter_min,
                                                 double strong_min, double* __restrict__ part /*[12][grid]*/,
                                                 unsigned long long* __restrict__ part_cnt /*[7][grid]*/, int live, const Pio pio) {
  using Sum = BlockSum<kLocTri, kBlock>;
  __shared__ double s_a[Sum::kWordsA];
  __shared__ double s_b[Sum::kWordsB];
  __shared__ uint32_t s_cnt[kLocCounts][kBlock / 64];
  const bool chain = ext_p == nullptr;  // uniform
  float T[16], limit, mpx, mpy, mpz;
  if (!loc_chain_state(chain, live, st, T, limit, mpx, mpy, mpz)) return;
  double dir[6][3];  // uniform: fully unrolled subscripts below, so registers
#pragma unroll
  for (int j = 0; j < 6; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) dir[j][c] = dirs[6 + 3 * j + c];
  double accA[6], accS[6];
  uint32_t cnt[kLocCounts];
#pragma unroll
  for (int j = 0; j < 6; ++j) accA[j] = accS[j] = 0.0;
  double accN[kPartial ? 6 : 1], accD[kPartial ? 6 : 1];
  float mqx = 0.f, mqy = 0.f, mqz = 0.f;
  if constexpr (kPartial) {
#pragma unroll
    for (int j = 0; j < 6; ++j) accN[j] = accD[j] = 0.0;
    if (chain) {  // uniform
      const float hv = hdr_load(st);
      mqx = hdr_f(hv, H_MQ), mqy = hdr_f(hv, H_MQ + 1), mqz = hdr_f(hv, H_MQ + 2);
    }
  }
#pragma unroll
  for (int j = 0; j < kLocCounts; ++j) cnt[j] = 0u;
  for (int base = blockIdx.x * (kBlock * kNePPT) + threadIdx.x; base < N; base += gridDim.x * (kBlock * kNePPT)) {
#pragma unroll
    for (int u = 0; u < kNePPT; ++u) {
      const int i = base + u * kBlock;
      if (i >= N) continue;
      float p[3], n[3], c[3];
      if (!loc_pair(chain, i, rx, ry, rz, mn, pos, d2, limit, max_out_r2, T, mpx, mpy, mpz, ext_p, ext_n, p, n)) continue;
      loc_cross(p, n, c);
      const float r = sqrtf((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);  // the correctly rounded ones, as in cov_terms
      float tau[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) tau[k] = r > 0.f ? c[k] / r : 0.f;
      cnt[6] += 1u;
      float h = 0.f;  // kPartial: the pair's residual as k_normal_eq forms it
      if constexpr (kPartial) {
        float q[3];
        if (chain) {
          const float4 qq = pio.mq[i];
          q[0] = qq.x - mqx, q[1] = qq.y - mqy, q[2] = qq.z - mqz;
        } else {
#pragma unroll
          for (int k = 0; k < 3; ++k) q[k] = pio.ext_q[3 * (size_t)i + k];
        }
        const float ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
        h = h + ex * n[0];
        h = h + ey * n[1];
        h = h + ez * n[2];
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const float* g = j < 3 ? n : tau;
        const double a = fabs(((double)g[0] * dir[j][0] + (double)g[1] * dir[j][1]) + (double)g[2] * dir[j][2]);
        if (a >= filter_min) accA[j] += a;
        if (a >= strong_min) {
          accS[j] += a;
          cnt[j] += 1u;
        }
        if constexpr (kPartial) {
          const float* gr = j < 3 ? n : c;  // the minimiser's own row: the rotation part unnormalised
          const double s = ((double)gr[0] * dir[j][0] + (double)gr[1] * dir[j][1]) + (double)gr[2] * dir[j][2];
          if (a >= strong_min) {
            accN[j] += s * (double)h;
            accD[j] += s * s;
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < kLocCounts; ++j) {
    const uint32_t s = wave_sum_u32(cnt[j]);
    if ((threadIdx.x & 63) == 0) s_cnt[j][threadIdx.x >> 6] = s;
  }
  Sum::run(accA, s_a, s_b);  // (its barriers also publish s_cnt)
  if (threadIdx.x < 6) part[threadIdx.x * gridDim.x + blockIdx.x] = Sum::total(s_b, threadIdx.x);
  if (threadIdx.x < kLocCounts) {
    unsigned long long c = 0ull;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) c += s_cnt[threadIdx.x][w];
    part_cnt[threadIdx.x * gridDim.x + blockIdx.x] = c;
  }
  Sum::run(accS, s_a, s_b);
  if (threadIdx.x < 6) part[(6 + threadIdx.x) * gridDim.x + blockIdx.x] = Sum::total(s_b, threadIdx.x);
  if constexpr (kPartial) {
    Sum::run(accN, s_a, s_b);  // (its first barrier stands between the totals above and the new segment sums)
    if (threadIdx.x < 6) pio.part[threadIdx.x * gridDim.x + blockIdx.x] = Sum::total(s_b, threadIdx.x);
    Sum::run(accD, s_a, s_b);
    if (threadIdx.x < 6) pio.part[(6 + threadIdx.x) * gridDim.x + blockIdx.x] = Sum::total(s_b, threadIdx.x);
  }
}

__global__ void __launch_bounds__(kBlock) k_loc_contrib(const float* __restrict__ rx, const float* __restrict__ ry, const float* __restrict__ rz, int N,
                                                        const float4* __restrict__ mn, const int32_t* __restrict__ pos, const float* __restrict__ d2,
                                                        float max_out_r2, const IcpState* __restrict__ st, const float* __restrict__ ext_p,
                                                        const float* __restrict__ ext_n, const double* __restrict__ dirs, double filter_min,
                                                        double strong_min, double* __restrict__ part /*[12][grid]*/,
                                                        unsigned long long* __restrict__ part_cnt /*[7][grid]*/, int live) {
  loc_contrib_body<false>(rx, ry, rz, N, mn, pos, d2, max_out_r2, st, ext_p, ext_n, dirs, filter_min, strong_min, part, part_cnt, live, LocNoPartialIo{});
}
__global__ void __launch_bounds__(kBlock) k_loc_contrib_partial(const float* __restrict__ rx, const float* __restrict__ ry, const float* __restrict__ rz,
                                                                int N, const float4* __restrict__ mn, const int32_t* __restrict__ pos,
                                                                const float* __restrict__ d2, float max_out_r2, const IcpState* __restrict__ st,
                                                                const float* __restrict__ ext_p, const float* __restrict__ ext_n,
                                                                const double* __restrict__ dirs, double filter_min, double strong_min,
                                                                double* __restrict__ part /*[12][grid]*/,
                                                                unsigned long long* __restrict__ part_cnt /*[7][grid]*/, int live, LocPartialIo pio) {
  loc_contrib_body<true>(rx, ry, rz, N, mn, pos, d2, max_out_r2, st, ext_p, ext_n, dirs, filter_min, strong_min, part, part_cnt, live, pio);
}

// One block: the 12 sums folded as in k_loc_eig, the 7 counts by waves 0..3 in turn (lane l adds blocks l, l + 64, ...: integers,
// any order gives the same).  Thread 0 applies the categories and posts, and leaves the values in `out` for a host whose posts are
// switched off.
__global__ void __launch_bounds__(kBlock) k_loc_post(const double* __restrict__ part /*[12][nb]*/, const unsigned long long* __restrict__ part_cnt /*[7][nb]*/,
                                                     int nb, const double* __restrict__ dirs, LocThresholds th, const IcpState* __restrict__ st /*null: module*/,
                                                     const unsigned long long* __restrict__ t_start, double* __restrict__ out /*[kLocPostVals]*/,
                                                     uint32_t* __restrict__ mailbox, uint32_t seq) {
  __shared__ double s_sum[kLocSums];
  __shared__ unsigned long long s_cnt[kLocCounts];
  loc_fold12(part, nb, s_sum);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  for (int c = w; c < kLocCounts; c += kBlock / 64) {
    unsigned long long s = 0ull;
    for (int b = l; b < nb; b += 64) s += part_cnt[(size_t)c * nb + b];
    s = wave_sum_u64(s);
    if (l == 0) s_cnt[c] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double v[kLocPostVals];
#pragma unroll
    for (int k = 0; k < kLocDirs; ++k) v[k] = dirs[k];
#pragma unroll
    for (int k = 0; k < kLocSums; ++k) v[kLocDirs + k] = s_sum[k];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double all = s_sum[j], strong = s_sum[6 + j];
      const long long cat = (all >= th.sum_all_min || strong >= th.sum_strong_min) ? 2 : (strong >= th.sum_partial_min ? 1 : 0);
      v[kLocDirs + kLocSums + j] = __longlong_as_double((long long)s_cnt[j]);
      v[kLocDirs + kLocSums + 6 + j] = __longlong_as_double(cat);
    }
    constexpr int kTail = kLocDirs + kLocSums + 12;
    v[kTail] = __longlong_as_double((long long)s_cnt[6]);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[kTail + 1 + c] = st ? (double)st->mp[c] : 0.0;
    v[kTail + 4] = __longlong_as_double((long long)*t_start);
    v[kTail + 5] = __longlong_as_double((long long)wall_clock64());
#pragma unroll
    for (int k = 0; k < kLocPostVals; ++k) out[k] = v[k];
    host_post::post(mailbox, seq, host_post::kPostVals, v);
  }
}

}  // namespace kern

// the work area, in doubles: pass 1's partials [12][blocks], the six directions, pass 2's partials [12][blocks] and counts
// [7][blocks], what k_loc_post posts, k_loc_hessian's start stamp.  (Here, not in localizability_impl.h: the degeneracy-aware chain
// launches the first three kernels from the issue loop, which stands in front of that header.)
constexpr size_t kLocOffDirs = (size_t)kMaxPartialBlocks * kern::kLocSums;
constexpr size_t kLocOffPart2 = kLocOffDirs + kern::kLocDirs;
constexpr size_t kLocOffCnt = kLocOffPart2 + (size_t)kMaxPartialBlocks * kern::kLocSums;
constexpr size_t kLocOffOut = kLocOffCnt + (size_t)kMaxPartialBlocks * kern::kLocCounts;
constexpr size_t kLocOffStart = kLocOffOut + kern::kLocPostVals;
constexpr size_t kLocBufBytes = (kLocOffStart + 1) * sizeof(double);
// the grid of both passes (k_cov's)
inline int loc_blocks(int n) { return std::max(1, std::min(kMaxPartialBlocks, (n + kern::kBlock * kern::kNePPT - 1) / (kern::kBlock * kern::kNePPT))); }
}  // namespace o3s
