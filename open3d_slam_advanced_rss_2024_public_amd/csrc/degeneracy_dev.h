// degeneracy_dev.h — k_constrain, the one kernel of the degeneracy-aware step (include/degeneracy/o3s_degeneracy.h holds the
// arithmetic contract): it stands between the normal equations (k_sel_ne / k_normal_eq) and k_solve and rewrites the [27][nb] block
// partials in d_ne into the system constrained to C x = 0, so that k_solve runs unchanged on it.
//   FIXED    the set arrives by value with the launch
//   ANALYSE  k_loc_hessian, k_loc_eig and k_loc_contrib (localizability_dev.h, live) have run on this iteration's kept pairs; the
//            kernel folds pass 2 as k_loc_post does, applies the categories (k_loc_decide, fused in here: one launch less per
//            iteration) and takes the directions of category < min_category
// One block of kBlock threads.  Every small matrix lives in LDS and is indexed there (a run-time subscript into registers would put
// it into scratch, see the note at the top of solve_device.h); the 36 entries are formed by 36 lanes side by side, each a serial
// left-to-right fp64 sum, so the order of operations is the header's whatever the lane count.
// k_constrain_values (include/degeneracy/o3s_degeneracy_partial.h) is the same body with values for the rows, C x = d: the caller's
// (FIXED, the module-level minimiser), or in ANALYSE mode -num / den of the strong-pair sums k_loc_contrib_partial left, for the
// rows of category 1.  The instantiation without values is the kernel it was before the values existed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_kernels.h"
#include "localizability_dev.h"

#pragma clang fp contract(off)

namespace o3s {
namespace kern {

// what the last constrained iteration used, for o3s_icp_get_degeneracy: dirs in the mask's order (translation 0..2, rotation 3..5)
struct DegLast {
  double dir[6][3];
  uint32_t mask;
  uint32_t pad;
};
struct DegFixed {  // the caller's set, by value: rows in the mask's order (translation 0..2, rotation 3..5), mask of the rows present
  double dir[6][3];
  uint32_t mask;
};
struct DegLds {
  double s_a[BlockSum<kNeComps, kBlock>::kWordsA];
  double s_b[BlockSum<kNeComps, kBlock>::kWordsB];
  double s_sum[kNeComps];
  double loc[kLocSums];  // ANALYSE: pass 2's folded sums
  double C[6][6];        // the rows of C: rotation directions first, then translation
  double A[6][6], P[6][6], M[6][6], F[2][6][6];
  double mu[2];
  int n_rot, n_rows;
  uint32_t mask;
};

// ---- values for the rows (o3s_degeneracy_partial.h) ------------------------------------------------------------------------------------
// o3s_degeneracy_partial, as the device leaves it (the host copies it out as it stands)
struct DegPartialLast {
  double num[6], den[6], value[6];
  int32_t category[6];
  uint32_t partial_mask, constrained_mask;
};
struct DegValuesIo {
  const double* pp_part;  // ANALYSE: [12][nbl] of k_loc_contrib_partial (num[6] then den[6]); null: the caller's values below
  double fixed_vals[6];   // the caller's values, in the mask's order
  DegPartialLast* last;   // nullable (the module-level minimiser leaves no record)
  uint32_t* pmasks;       // the per-iteration trace, nullable: the partial mask ...
  double* values;         // ... and the six values the rows carried [cap][6]
};
struct DegValLds {
  double pp[kLocSums];  // the folded strong-pair sums: num[6], den[6]
  double quot[6];       // -num / den of every direction
  double val[6];        // what the direction's row carries (0 outside the partial mask)
  double d[6];          // ... in the order of the rows of C
  double xc[6], rs[6], ts[6], g2[6];
  int32_t cat[6];
  uint32_t pmask;
};
// -num / den, +0.0 when den is 0 or the quotient is not finite
__device__ __forceinline__ double deg_quotient(double num, double den) {
  if (den == 0.0) return 0.0;
  const double q = -num / den;
  return fabs(q) < __builtin_huge_val() ? q : 0.0;  // (a NaN fails the comparison)
}

template <bool kValues>
__device__ __forceinline__ void constrain_body(double* __restrict__ part /*[27][nb]*/, int nb, const IcpState* __restrict__ st, const DegFixed& fixed,
                                               const double* __restrict__ loc_part /*null: FIXED; [12][nbl] of k_loc_contrib*/, int nbl,
                                               const double* __restrict__ loc_dirs, const LocThresholds& th, int min_category,
                                               DegLast* __restrict__ last, uint32_t* __restrict__ masks /*nullable*/, int mask_cap,
                                               const DegValuesIo& io) {
  __shared__ DegLds L;
  __shared__ DegValLds V;  // (kValues only: the other instantiation never touches it, and it is not allocated there)
  const float hv = hdr_load(st);
  if (hdr_i(hv, H_DONE) || hdr_i(hv, H_STATUS)) return;  // the chain has ended (or this iteration has failed: k_solve closes it)
  const int t = threadIdx.x;
  const int it = hdr_i(hv, H_ITER);
  const bool analyse = loc_part != nullptr;  // uniform
  if (analyse) {  // k_loc_post's fold (loc_fold12, localizability_dev.h)
    loc_fold12(loc_part, nbl, L.loc);
    if constexpr (kValues) loc_fold12(io.pp_part, nbl, V.pp);
  }
  if (t < 36) L.C[t / 6][t % 6] = 0.0;
  __syncthreads();
  if (t == 0) {  // the set: mask, and the rows of C (rotation first)
    uint32_t mask = 0u;
    if (analyse) {
      uint32_t pmask = 0u;
      for (int j = 0; j < 6; ++j) {
        const double all = L.loc[j], strong = L.loc[6 + j];
        const int cat = (all >= th.sum_all_min || strong >= th.sum_strong_min) ? 2 : (strong >= th.sum_partial_min ? 1 : 0);
        if (cat < min_category) mask |= 1u << j;
        if constexpr (kValues) {
          if (cat == 1) mask |= 1u << j, pmask |= 1u << j;
          V.cat[j] = cat;
          V.quot[j] = deg_quotient(V.pp[j], V.pp[6 + j]);
          V.val[j] = cat == 1 ? V.quot[j] : 0.0;
        }
      }
      if constexpr (kValues) V.pmask = pmask;
    } else {
      mask = fixed.mask;
      if constexpr (kValues) {
        for (int j = 0; j < 6; ++j) V.val[j] = (mask & (1u << j)) ? io.fixed_vals[j] : 0.0;
      }
    }
    int row = 0;
    for (int j = 3; j < 6; ++j)
      if (mask & (1u << j)) {
        for (int c = 0; c < 3; ++c) L.C[row][c] = analyse ? loc_dirs[6 + 3 * j + c] : fixed.dir[j][c];
        if constexpr (kValues) V.d[row] = V.val[j];
        ++row;
      }
    L.n_rot = row;
    for (int j = 0; j < 3; ++j)
      if (mask & (1u << j)) {
        for (int c = 0; c < 3; ++c) L.C[row][3 + c] = analyse ? loc_dirs[6 + 3 * j + c] : fixed.dir[j][c];
        if constexpr (kValues) V.d[row] = V.val[j];
        ++row;
      }
    L.n_rows = row;
    L.mask = mask;
    if (masks && it < mask_cap) masks[it] = mask;
    if constexpr (kValues) {
      if (analyse && io.pmasks && it < mask_cap) {
        io.pmasks[it] = V.pmask;
        for (int j = 0; j < 6; ++j) io.values[(size_t)it * 6 + j] = V.val[j];
      }
    }
  }
  __syncthreads();
  const uint32_t mask = L.mask;
  if (mask == 0u) return;  // uniform.  The empty set: the partials stay as they are, bit for bit
  if (t < 18) {  // the set this iteration used, in the mask's order
    const int j = t / 3, c = t % 3;
    double v = 0.0;
    if (mask & (1u << j)) v = analyse ? loc_dirs[6 + 3 * j + c] : fixed.dir[j][c];
    last->dir[j][c] = v;
  } else if (t == 18) {
    last->mask = mask;
  }
  if constexpr (kValues) {
    if (analyse && io.last) {  // uniform
      if (t >= 64 && t < 70) {
        const int j = t - 64;
        io.last->num[j] = V.pp[j], io.last->den[j] = V.pp[6 + j], io.last->value[j] = V.quot[j], io.last->category[j] = V.cat[j];
      } else if (t == 70) {
        io.last->partial_mask = V.pmask, io.last->constrained_mask = mask;
      }
    }
  }
  ne_fold(part, nb, L.s_a, L.s_b, L.s_sum);
  __syncthreads();
  const int n_rot = L.n_rot, n_rows = L.n_rows;
  const int a = t / 6, c = t % 6;  // (t < 36)
  if (t < 36) {
    const int lo = a < c ? a : c, hi = a < c ? c : a;
    L.A[a][c] = L.s_sum[lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)];  // the row-major upper triangle, mirrored
    double d = 0.0, fr = 0.0, ft = 0.0;
    for (int j = 0; j < n_rows; ++j) d += L.C[j][a] * L.C[j][c];
    for (int j = 0; j < n_rot; ++j) fr += L.C[j][a] * L.C[j][c];
    for (int j = n_rot; j < n_rows; ++j) ft += L.C[j][a] * L.C[j][c];
    L.P[a][c] = (a == c ? 1.0 : 0.0) - d;
    L.F[0][a][c] = fr;
    L.F[1][a][c] = ft;
  } else if (t == 64 || t == 65) {  // mu_r, mu_t: the next wave, beside the 36 lanes
    const int o = t == 64 ? 0 : 3;
    const double d0 = L.s_sum[o * 6 - (o * (o - 1)) / 2], d1 = L.s_sum[(o + 1) * 6 - ((o + 1) * o) / 2], d2 = L.s_sum[(o + 2) * 6 - ((o + 2) * (o + 1)) / 2];
    double mu = ((d0 + d1) + d2) / 3.0;
    if (!(fabs(mu) < __builtin_huge_val()) || mu == 0.0) mu = 1.0;  // zero or not finite (a NaN fails the comparison)
    L.mu[t - 64] = mu;
  } else if (kValues && t >= 128 && t < 134) {  // xc = C^T d and its two halves: the third wave
    const int k = t - 128;
    double x = 0.0, r = 0.0, s = 0.0;
    for (int j = 0; j < n_rows; ++j) x += L.C[j][k] * V.d[j];
    for (int j = 0; j < n_rot; ++j) r += L.C[j][k] * V.d[j];
    for (int j = n_rot; j < n_rows; ++j) s += L.C[j][k] * V.d[j];
    V.xc[k] = x, V.rs[k] = r, V.ts[k] = s;
  }
  __syncthreads();
  if (t < 36) {
    double m = 0.0;
    for (int k = 0; k < 6; ++k) m += L.A[a][k] * L.P[k][c];
    L.M[a][c] = m;
  } else if (kValues && t >= 64 && t < 70) {  // g'' = g + A xc
    const int k = t - 64;
    double s = 0.0;
    for (int m = 0; m < 6; ++m) s += L.A[k][m] * V.xc[m];
    V.g2[k] = L.s_sum[21 + k] + s;
  }
  __syncthreads();
  if (t < 36 && a <= c) {
    double v = 0.0;
    for (int k = 0; k < 6; ++k) v += L.P[a][k] * L.M[k][c];
    v = (v + L.mu[0] * L.F[0][a][c]) + L.mu[1] * L.F[1][a][c];
    part[(size_t)(a * 6 - (a * (a - 1)) / 2 + (c - a)) * nb] = v;
  } else if (t >= 64 && t < 70) {
    const int r = t - 64;
    double g = 0.0;
    if constexpr (kValues) {
      for (int k = 0; k < 6; ++k) g += L.P[r][k] * V.g2[k];
      g = (g - L.mu[0] * V.rs[r]) - L.mu[1] * V.ts[r];
    } else {
      for (int k = 0; k < 6; ++k) g += L.P[r][k] * L.s_sum[21 + k];
    }
    part[(size_t)(21 + r) * nb] = g;
  }
  // the other nb - 1 columns: +0.0, whose fold is exact (every thread read its share of them in ne_fold, in front of two barriers)
  for (int k = t; k < kNeComps * (nb - 1); k += kBlock) part[(size_t)(k / (nb - 1)) * nb + 1 + k % (nb - 1)] = 0.0;
}

__global__ void __launch_bounds__(kBlock) k_constrain(double* __restrict__ part /*[27][nb]*/, int nb, const IcpState* __restrict__ st, DegFixed fixed,
                                                      const double* __restrict__ loc_part /*null: FIXED; [12][nbl] of k_loc_contrib*/, int nbl,
                                                      const double* __restrict__ loc_dirs, LocThresholds th, int min_category,
                                                      DegLast* __restrict__ last, uint32_t* __restrict__ masks /*nullable*/, int mask_cap) {
  constrain_body<false>(part, nb, st, fixed, loc_part, nbl, loc_dirs, th, min_category, last, masks, mask_cap, DegValuesIo{});
}
__global__ void __launch_bounds__(kBlock) k_constrain_values(double* __restrict__ part /*[27][nb]*/, int nb, const IcpState* __restrict__ st, DegFixed fixed,
                                                             const double* __restrict__ loc_part, int nbl, const double* __restrict__ loc_dirs,
                                                             LocThresholds th, int min_category, DegLast* __restrict__ last,
                                                             uint32_t* __restrict__ masks /*nullable*/, int mask_cap, DegValuesIo io) {
  constrain_body<true>(part, nb, st, fixed, loc_part, nbl, loc_dirs, th, min_category, last, masks, mask_cap, io);
}

// The module-level estimate (o3s_degen_partial_estimate) behind k_loc_post: one block folds the strong-pair sums as k_constrain_values
// does and leaves the record; the categories are the ones k_loc_post left in `loc_out` (bit patterns of integers).
__global__ void __launch_bounds__(kBlock) k_deg_partial_post(const double* __restrict__ pp_part /*[12][nbl]*/, int nbl,
                                                             const double* __restrict__ loc_out /*k_loc_post's values*/,
                                                             DegPartialLast* __restrict__ out) {
  __shared__ double s_pp[kLocSums];
  loc_fold12(pp_part, nbl, s_pp);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t pmask = 0u, cmask = 0u;
    for (int j = 0; j < 6; ++j) {
      const int cat = (int)__double_as_longlong(loc_out[kLocDirs + kLocSums + 6 + j]);
      out->num[j] = s_pp[j], out->den[j] = s_pp[6 + j], out->value[j] = deg_quotient(s_pp[j], s_pp[6 + j]), out->category[j] = cat;
      if (cat == 1) pmask |= 1u << j;
      if (cat < 2) cmask |= 1u << j;
    }
    out->partial_mask = pmask, out->constrained_mask = cmask;
  }
}

}  // namespace kern
}  // namespace o3s
