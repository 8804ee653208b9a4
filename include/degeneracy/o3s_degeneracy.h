/*
 * o3s_degeneracy.h — C ABI of the degeneracy-aware ICP step (same shared library, libo3dslam_icp_hip.so): every iteration of the
 * scan-to-map chain solves its step under the equality constraints C x = 0 in the directions the scan does not constrain, instead of
 * having o3s_localizability_remap (../localizability/o3s_localizability.h) take the correction back after the chain has slid along
 * them.  One kernel, k_constrain, between the normal equations (k_sel_ne / k_normal_eq) and k_solve rewrites the block partials of
 * the normal equations into the constrained system; k_solve itself is what it is without the feature.  Nothing goes to the host
 * per iteration.  With the mode OFF the chain launches exactly what it launches without this header.
 *
 * The set of an iteration: n_rot <= 3 unit rotation directions w_j and n_trans <= 3 unit translation directions v_j, each group
 * mutually orthogonal; as 6-vectors of the minimiser's x = [rot; trans] (o3s_icp_minimize): e = [w; 0] or e = [0; v].  The rows of C
 * are the rotation directions in their order, then the translation directions in theirs.
 *
 * Arithmetic contract (k_constrain, one block; fp64 throughout, no FMA contraction, every sum left to right from 0).
 *  S[27] = the block partials [27][nb] of the normal equations folded exactly as k_solve folds them (the same routine): the row-major
 *  upper triangle of A (21) and the six sums g = sum G h; k_solve's b is -g.  A is S mirrored to the full symmetric 6 x 6.
 *    D[a][c]  = sum over the rows j of C, in order, of C[j][a] C[j][c]                      (C^T C)
 *    P[a][c]  = (a == c ? 1 : 0) - D[a][c]
 *    M[a][c]  = sum over k = 0..5 of A[a][k] P[k][c]                                       (A P)
 *    F_r[a][c] = sum over the rotation rows of C[j][a] C[j][c],  F_t likewise over the translation rows
 *    mu_r = ((A00 + A11) + A22) / 3,  mu_t = ((A33 + A44) + A55) / 3, each replaced by 1.0 when it is zero or not finite
 *    A'[a][c] = ((sum over k = 0..5 of P[a][k] M[k][c]) + mu_r F_r[a][c]) + mu_t F_t[a][c]    for a <= c (the upper triangle only:
 *               k_solve mirrors it)
 *    g'[a]    = sum over k = 0..5 of P[a][k] g[k]                                           (b' = P b = -g')
 *  A', g' become the partial of block 0 and the other nb - 1 columns become +0.0, whose fold is exact; k_solve then rounds each sum
 *  to fp32 once, as always.  The solution of A' x = b' minimises the same quadratic over C x = 0; mu keeps the filled-in directions
 *  at the scale of A, so that k_solve's rank branches see a full-rank system.
 *  An iteration whose set is empty writes nothing to the partials: that iteration is bit-identical to the unconstrained one.
 *  An iteration that finds the chain ended, or failed by an earlier kernel of the iteration, writes nothing at all.
 *
 * Where the set comes from (per handle; not a field of o3s_icp_config):
 *  O3S_DEGENERACY_OFF      nothing is launched, allocated or captured (the default)
 *  O3S_DEGENERACY_FIXED    the caller's set in every iteration, in each iteration's own parameterisation (about that iteration's
 *                          centroid).  One launch more per iteration: k_constrain.
 *  O3S_DEGENERACY_ANALYSE  every iteration runs the localizability analysis (k_loc_hessian, k_loc_eig, k_loc_contrib: the arithmetic
 *                          contract of o3s_localizability.h, on the kept pairs of THAT iteration under the pose they were formed at) in
 *                          front of k_constrain, which folds pass 2 as k_loc_post does, applies the categories and constrains every
 *                          direction whose category < min_category.  Four launches more per iteration.  Partially localizable
 *                          directions get no treatment of their own unless o3s_degeneracy_partial.h's flag is set.
 *  Mask of an iteration (o3s_icp_degeneracy_trace): bit j < 3 translation direction j, bit 3 + j rotation direction j; in ANALYSE
 *  mode j is the analysis' index (eval ascending), in FIXED mode the index in the caller's set.
 *  After a constrained compute in ANALYSE mode, o3s_icp_localizability with the same parameters reports for the last iteration the
 *  very directions and categories that iteration used: same kernels, same pairs, same pose, same bits.
 *
 * A change of mode, set or parameters invalidates the captured graph of the chain.  Eager, replayed, profiled and
 * o3s_icp_compute_batch chains give the same bits.  The sharded mode refuses a compute with a mode other than OFF:
 * O3S_ERR_BAD_CONFIG.  Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_DEGENERACY_H
#define O3S_DEGENERACY_H

#include <stdint.h>

#include "../localizability/o3s_localizability.h"
#include "../o3s_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { O3S_DEGENERACY_OFF = 0, O3S_DEGENERACY_FIXED = 1, O3S_DEGENERACY_ANALYSE = 2 };

typedef struct o3s_degeneracy_set {
  int32_t n_rot, n_trans; /* 0..3 each                                                   */
  double rot[3][3];       /* w_j, unit and mutually orthogonal to 1e-9; rows >= n_rot are ignored  */
  double trans[3][3];     /* v_j likewise                                                */
} o3s_degeneracy_set;

typedef struct o3s_degeneracy_config {
  int32_t mode;                         /* O3S_DEGENERACY_*                                             */
  int32_t min_category;                 /* ANALYSE: directions of category < min_category (1 or 2) are constrained */
  o3s_degeneracy_set fixed_set;         /* FIXED                                                        */
  o3s_localizability_params loc_params; /* ANALYSE                                                      */
} o3s_degeneracy_config;

/* mode OFF, min_category 2, the empty set, o3s_localizability_default_params (its three sums NaN: they have no default) */
void o3s_degeneracy_default_config(o3s_degeneracy_config* c);

/* Sets the mode of the handle's later computes.  FIXED reads fixed_set only, ANALYSE reads loc_params and min_category only, OFF
 * reads neither (all three may be NULL then).  Refused before any device work, on a NULL handle too (the arguments are checked
 * first), with the handle's mode as it was:
 *   O3S_ERR_BAD_ARGUMENT  a mode outside the enum; FIXED with fixed_set NULL, a count outside 0..3, a non-finite direction, a
 *                         direction whose squared length differs from 1 by more than 1e-9 or two directions of a group whose dot
 *                         product exceeds 1e-9 in magnitude; ANALYSE with loc_params NULL or min_category outside {1, 2}; h NULL
 *   O3S_ERR_BAD_CONFIG    ANALYSE with thresholds out of order or unset (o3s_localizability.h)
 * ANALYSE allocates the localizability work area here, not inside a compute. */
int o3s_icp_set_degeneracy(o3s_icp* h, int32_t mode, const o3s_degeneracy_set* fixed_set, const o3s_localizability_params* loc_params,
                           int32_t min_category);

/* What o3s_icp_set_degeneracy left (nullable out), and in *last_set (nullable) the set the last constrained iteration of the last
 * successful compute used, in the mask's order (all zeros when the mode is OFF or nothing has been computed since the mode was set). */
int o3s_icp_get_degeneracy(o3s_icp* h, o3s_degeneracy_config* out, o3s_degeneracy_set* last_set);

/* One mask per iteration of the last successful compute, at most cap of them; returns their number (the iterations of
 * o3s_icp_get_trace), 0 when the mode was OFF, there is nothing to report or an argument is NULL. */
int32_t o3s_icp_degeneracy_trace(o3s_icp* h, int32_t* masks, int32_t cap);

/* o3s_icp_minimize with k_constrain in front of k_solve: the step of the caller's weighted pairs under C x = 0.  A_out, b_out
 * (nullable, as there) are the constrained system A', b' as k_solve rounded it to fp32.  An empty set gives o3s_icp_minimize's bits.
 * A bad set: O3S_ERR_BAD_ARGUMENT before any device work, on a NULL handle too, outputs untouched. */
int o3s_icp_minimize_degeneracy(o3s_icp* h, const float* reading_xyzw, const int32_t* ids, const float* dists2, const float* weights, int64_t N,
                                const o3s_degeneracy_set* set, float T_out[16], float A_out[36], float b_out[6], float x_out[6]);

#ifdef __cplusplus
}
#endif
#endif /* O3S_DEGENERACY_H */
