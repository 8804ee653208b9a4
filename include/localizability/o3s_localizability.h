/*
 * o3s_localizability.h — C ABI of the localizability analysis of the scan-to-map ICP (same shared library, libo3dslam_icp_hip.so):
 * which directions of the pose the kept pairs of the LAST iteration of a compute actually constrained, and a pose that takes the
 * ICP's correction in those directions only.  The pose covariance (o3s_icp_get_covariance) says in hindsight that a registration
 * was ill-conditioned; this says which directions were, per translation and per rotation direction, and o3s_localizability_remap
 * keeps the prior there.  The analysis is two more passes over the resident pairs behind the iteration that ended the chain
 * (csrc/localizability_dev.h); the chain itself — launches, graph, pose, trace, stats, covariance — is the same with and without
 * it, and nothing is launched unless the call is made.
 *
 * Arithmetic contract.
 *  Inputs: the inputs of the covariance pass (o3s_icp.h, "pose covariance"): for every kept pair of the last iteration, in
 *  processing-slot order, p = the centred fp32 reading point (S - mp), n = the matched fp32 normal.
 *  Per pair, fp32, no FMA contraction, left to right:
 *    c = p x n:  cx = py nz - pz ny, cy = pz nx - px nz, cz = px ny - py nx
 *    r = sqrt((px^2 + py^2) + pz^2);   tau = c / r component-wise when r > 0, else 0
 *  Pass 1, fp64 sums of exact products of the promoted fp32 values, six upper-triangle sums each (00 01 02 11 12 22):
 *    A_t = sum n n^T,  A_r = sum c c^T     (the translation and rotation diagonal blocks of the Hessian of the minimiser's
 *    x = [rot; trans], o3s_icp_minimize)
 *  Eigen step, fp64, on each 3 x 3 block: cyclic Jacobi, pairs (0,1) (0,2) (1,2) per sweep, at most 16 sweeps, ended when
 *  NOT (|a01| + |a02| + |a12| > 2^-70 (|a00| + |a11| + |a22|)); a rotation of pair (p,q) with a_pq != 0 is
 *    theta = (a_qq - a_pp) / (2 a_pq);  t = sign(theta) / (|theta| + sqrt(theta^2 + 1)) (sign(0) = +1);  c = 1 / sqrt(t^2 + 1);  s = t c
 *    a_pp -= t a_pq;  a_qq += t a_pq;  a_pq = 0;  (a_rp, a_rq) <- (c a_rp - s a_rq, s a_rp + c a_rq);  columns p, q of V likewise
 *  Eigenvalues ascending (a stable three-element sort), each eigenvector divided by sqrt((x^2 + y^2) + z^2), then its component
 *  of largest magnitude made positive (a tie: the lowest index).  A block with a non-finite sum gives NaN eigenvalues and NaN
 *  eigenvectors (no Jacobi is run on it).
 *  Pass 2, fp64 on the promoted fp32 values, per pair and direction:
 *    translation direction v:  a = |(nx v0 + ny v1) + nz v2|       rotation direction w:  a = |(taux w0 + tauy w1) + tauz w2|
 *    sum_all = sum a [a >= filter_min],  sum_strong = sum a [a >= strong_min],  n_strong = sum [a >= strong_min]
 *  (a NaN contribution fails both comparisons).
 *  Category per direction: 2 (localizable) if sum_all >= sum_all_min or sum_strong >= sum_strong_min; else 1 (partially) if
 *  sum_strong >= sum_partial_min; else 0 (not).
 *  Order of every sum: per-block partials folded in block order, as the covariance pass does; no floating-point atomics; the
 *  counts are integer partials.  The same input gives the same bits from call to call.
 *
 * Launches: k_loc_hessian, k_loc_eig, k_loc_contrib, k_loc_post on the handle's stream, one host round trip (the post of
 * k_loc_post).  The work area is allocated by the first call and never again.
 *
 * (The header lives in a directory of its own: include/ itself holds the headers of the first device-side ABI, one list.)
 * Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_LOCALIZABILITY_H
#define O3S_LOCALIZABILITY_H

#include <stdint.h>

#include "../o3s_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct o3s_localizability_params {
  double filter_min;      /* kappa_f: contributions below it are ignored            0 <= kappa_f <= kappa_s <= 1 */
  double strong_min;      /* kappa_s: contributions at or above it count as strong                               */
  double sum_all_min;     /* kappa_1 >= kappa_2 >= kappa_3 >= 0, all finite: absolute sums, they scale with the  */
  double sum_strong_min;  /* kappa_2   number of kept pairs, so there is NO default: default_params leaves the   */
  double sum_partial_min; /* kappa_3   three NaN and an unset threshold is O3S_ERR_BAD_CONFIG                    */
} o3s_localizability_params;

typedef struct o3s_localizability {
  double eval[6];        /* [0..2] translation block, ascending; [3..5] rotation block, ascending */
  double evec[6][3];     /* unit direction of eval[j]                                             */
  double sum_all[6], sum_strong[6];
  int64_t n_strong[6];
  int32_t category[6];   /* 2 localizable, 1 partially, 0 not                                     */
  int64_t kept;          /* pairs the passes took                                                 */
  double centre[3];      /* mp of the last iteration, in the reference cloud's own frame          */
  float gpu_ms;          /* start of k_loc_hessian -> end of k_loc_post, the device's clock       */
  int32_t reserved;
} o3s_localizability;

/* kappa_f = cos 80 deg, kappa_s = cos 35 deg, the three sums NaN (they have to be calibrated: run the analysis on a
 * well-constrained recording and read sum_all / sum_strong). */
void o3s_localizability_default_params(o3s_localizability_params* p);

/* The analysis of the last successful compute on this handle (any compute entry point, o3s_icp_compute_batch included, either
 * minimiser).  It disturbs neither o3s_icp_get_covariance, o3s_icp_get_error_elements nor the next compute, and two calls give
 * the same bits.  kept = 0 (nothing to analyse) gives all zeros, categories 0 and O3S_OK.
 * NULL pointers: O3S_ERR_BAD_ARGUMENT; parameters out of order or unset: O3S_ERR_BAD_CONFIG — both before any device work and
 * with *out untouched.  The sharded mode: O3S_ERR_BAD_CONFIG.  Before any compute, after a failed one, or after the handle has
 * been given other work that replaced the chain's buffers: O3S_ERR_NOT_INITIALIZED. */
int o3s_icp_localizability(o3s_icp* h, const o3s_localizability_params* params, o3s_localizability* out);

/* The same kernels at module level, beside o3s_icp_estimate_covariance: two 3 x K host arrays of pairs that are ALREADY centred
 * (AoS [x y z] per pair).  Needs no reference and touches no state of a compute; centre is 0.  K <= 0: O3S_ERR_NO_POINTS.
 * Non-finite input gives non-finite eigen output, categories 0 and O3S_OK. */
int o3s_localizability_estimate(o3s_icp* h, const float* reading_c, const float* normals, int64_t K,
                                const o3s_localizability_params* params, o3s_localizability* out);

/* A pose that takes the ICP's correction only in the directions of category >= min_category (1 or 2).  Host arithmetic, fp64,
 * column-major 4 x 4 matrices; no device, no handle.
 *   dT = T_icp . T_prior^-1 (the inverse of the affine [A, t] itself: a prior that went through fp32 is orthonormal to 1e-7 only),
 *   m = centre,  R = the rotation block of dT,
 *   u = dT(m) - m,  a = 1/2 (R21 - R12, R02 - R20, R10 - R01) (row, column),  theta = atan2(|a|, (tr R - 1) / 2),
 *   r = (theta / |a|) a when |a| > 0, else 0
 *   u' = sum over j < 3 with category[j] >= min_category of (v_j . u) v_j,   r' = the same over j >= 3 with w_j and r
 *   T_out = [x -> exp(r')(x - m) + m + u'] . T_prior, exp by Rodrigues' formula
 * *n_replaced (nullable) = the number of directions with category < min_category; when it is 0, T_out is T_icp copied bit for
 * bit, whatever the correction is.  Otherwise theta >= pi / 2 (not a correction one may linearise) or a singular T_prior is
 * O3S_ERR_BAD_ARGUMENT; so are, always, a non-finite matrix, min_category outside {1, 2} and a NULL pointer.  A refused call leaves
 * T_out and *n_replaced untouched. */
int o3s_localizability_remap(const o3s_localizability* loc, int32_t min_category, const double T_prior[16],
                             const double T_icp[16], double T_out[16], int32_t* n_replaced);

#ifdef __cplusplus
}
#endif
#endif /* O3S_LOCALIZABILITY_H */
