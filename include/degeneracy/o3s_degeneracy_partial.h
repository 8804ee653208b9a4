/*
 * o3s_degeneracy_partial.h — C ABI of the partial-direction treatment of the degeneracy-aware ICP step (same shared library,
 * libo3dslam_icp_hip.so; o3s_degeneracy.h holds the step itself).  A direction of category 1 (partially localizable,
 * ../localizability/o3s_localizability.h) is seen by a few strong pairs only: a door frame in a corridor, a pole in a tunnel.
 * Constrained to zero it loses what those pairs say; left to the full solve it is decided by the many weak pairs.  With the flag of
 * this header set, every iteration of the ANALYSE chain constrains such a direction to the value d_j that its strong pairs alone ask
 * for: C x = d instead of C x = 0.  Off by default; with it off the chain launches, allocates and computes what it does without this
 * header, bit for bit.  No launch more per iteration: the flagged instantiation of k_loc_contrib forms the sums, k_constrain folds
 * them and applies the values; k_solve is untouched.
 *
 * Arithmetic contract.
 *  Per kept pair of the iteration, exactly as k_normal_eq / k_sel_ne form them (fp32, no FMA contraction, left to right):
 *    p = the centred reading point, q = the centred matched point, n = the matched normal
 *    c = p x n (o3s_localizability.h),  e = p - q component-wise,  h = ((0 + ex nx) + ey ny) + ez nz
 *  a_j = the pair's pass-2 contribution of o3s_localizability.h in direction j (the mask's order: j < 3 translation direction v_j,
 *  j >= 3 rotation direction w_j-3):  |n . v_j|  or  |tau . w_j|.
 *  Strong-pair sums, fp64, for all six directions, over the pairs with a_j >= strong_min:
 *    s = (g0 d0 + g1 d1) + g2 d2      g = n (translation) or g = c (rotation; unnormalised: the minimiser's own row), promoted to
 *                                     fp64, d = the direction
 *    num_j += s * (double)h,   den_j += s * s
 *  Order of every sum: per-block partials folded in block order as the sums of pass 2 are; no floating-point atomics; the same input
 *  gives the same bits from call to call.  Pass 2's own sums keep their accumulators and their order: o3s_icp_localizability after a
 *  flagged compute still reports the last iteration's bits.
 *  value_j = -num_j / den_j, and +0.0 when den_j is 0 or the quotient is not finite: the step along e_j that minimises the
 *  point-to-plane error of the strong pairs alone, in the iteration's own parameterisation about its centroids.  (In steady state
 *  it cancels the centroid shift mq - mp along the direction, which C x = 0 does not.)
 *
 *  k_constrain with values d for the rows of C (rotation rows first, then translation rows, as in o3s_degeneracy.h; fp64, no FMA
 *  contraction, every sum left to right from 0; S, A, g, P, M, F_r, F_t, mu_r, mu_t, A' as defined there):
 *    xc[a]  = sum over the rows j of C, in order, of C[j][a] d_j                              (C^T d)
 *    g''[k] = g[k] + (sum over m = 0..5 of A[k][m] xc[m])                                     (g + A xc)
 *    r[a]   = sum over the rotation rows of C[j][a] d_j,  t[a] likewise over the translation rows
 *    g'[a]  = ((sum over k = 0..5 of P[a][k] g''[k]) - mu_r r[a]) - mu_t t[a]
 *  A' is exactly the A' of o3s_degeneracy.h.  The solution of A' x = -g' has e_j . x = d_j and minimises the same quadratic over that
 *  affine set.  A set whose values are all +0.0 gives the bits of C x = 0.
 *
 * Which rows carry a value.  In mode O3S_DEGENERACY_ANALYSE with the flag set, the set of an iteration is
 * {category < min_category} u {category == 1}; the rows of category 1 carry value_j, the others 0.  o3s_icp_degeneracy_trace reports
 * the whole set.  The modes FIXED and OFF ignore the flag.  The sharded mode refuses as it does without the flag.
 *
 * Link names.  The exported names abbreviate "degeneracy" to "degen": the set of exported symbols that spell the word out is the
 * ABI of o3s_degeneracy.h and is checked as such (tests/test_abi_degeneracy.py).  The macros at the end give every call its long
 * name as well.
 * Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_DEGENERACY_PARTIAL_H
#define O3S_DEGENERACY_PARTIAL_H

#include <stdint.h>

#include "o3s_degeneracy.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct o3s_degeneracy_partial {
  double num[6], den[6]; /* the strong-pair sums, in the mask's order (translation 0..2, rotation 3..5)   */
  double value[6];       /* -num / den of every direction (0 where den is 0 or the quotient is not finite) */
  int32_t category[6];   /* 2 localizable, 1 partially, 0 not                                              */
  int32_t partial_mask;     /* the directions of category 1: their rows carried value[j]                   */
  int32_t constrained_mask; /* the whole set of the iteration (o3s_icp_degeneracy_trace's mask)            */
} o3s_degeneracy_partial;

/* The flag of the handle's later computes (0 or 1).  A change invalidates the captured graph of the chain.  Setting it allocates
 * the work area here, not inside a compute.  h NULL or enable outside {0, 1}: O3S_ERR_BAD_ARGUMENT before any device work. */
int o3s_icp_set_degen_partial(o3s_icp* h, int32_t enable);

/* The flag (nullable out), and in *last (nullable) what the last constrained iteration of the last successful compute used: its
 * sums, values, categories and masks (all zeros when the flag is off, the mode is not ANALYSE, no iteration of that compute had a
 * set or nothing has been computed since the flag was set). */
int o3s_icp_get_degen_partial(o3s_icp* h, int32_t* enabled, o3s_degeneracy_partial* last);

/* One record per iteration of the last successful compute, at most cap of them: the partial mask and the six values the rows
 * carried (0 for the directions outside the partial mask).  Returns their number (o3s_icp_degeneracy_trace's); 0 when the flag is
 * off, the mode is not ANALYSE, there is nothing to report or an argument is NULL. */
int32_t o3s_icp_degen_partial_trace(o3s_icp* h, int32_t* partial_masks, double* values /*[cap][6]*/, int32_t cap);

/* The same kernels at module level, beside o3s_localizability_estimate: three 3 x K host arrays of pairs that are ALREADY centred
 * (AoS [x y z] per pair).  *loc (nullable) is o3s_localizability_estimate's result, bit for bit; out->value holds -num / den of
 * all six directions, partial_mask the directions of category 1 and constrained_mask the directions of category < 2.
 * K <= 0: O3S_ERR_NO_POINTS.  NULL pointers (but loc): O3S_ERR_BAD_ARGUMENT; parameters out of order or unset: O3S_ERR_BAD_CONFIG —
 * both before any device work, on a NULL handle too, outputs untouched. */
int o3s_degen_partial_estimate(o3s_icp* h, const float* reading_c, const float* reference_c, const float* normals, int64_t K,
                               const o3s_localizability_params* params, o3s_localizability* loc, o3s_degeneracy_partial* out);

/* o3s_icp_minimize_degeneracy with values for the rows of the set: the step of the caller's weighted pairs under C x = d.
 * rot_values[j] belongs to set->rot[j], trans_values[j] to set->trans[j] (entries beyond the counts are ignored); one array NULL
 * means zeros; both NULL gives o3s_icp_minimize_degeneracy's bits.  A bad set or a non-finite value: O3S_ERR_BAD_ARGUMENT before
 * any device work, on a NULL handle too, outputs untouched. */
int o3s_icp_minimize_degen_values(o3s_icp* h, const float* reading_xyzw, const int32_t* ids, const float* dists2, const float* weights,
                                  int64_t N, const o3s_degeneracy_set* set, const double rot_values[3], const double trans_values[3],
                                  float T_out[16], float A_out[36], float b_out[6], float x_out[6]);

#ifdef __cplusplus
}
#endif

#define o3s_icp_set_degeneracy_partial o3s_icp_set_degen_partial
#define o3s_icp_get_degeneracy_partial o3s_icp_get_degen_partial
#define o3s_icp_degeneracy_partial_trace o3s_icp_degen_partial_trace
#define o3s_degeneracy_partial_estimate o3s_degen_partial_estimate
#define o3s_icp_minimize_degeneracy_values o3s_icp_minimize_degen_values

#endif /* O3S_DEGENERACY_PARTIAL_H */
