/*
 * o3s_registration.h — C ABI of the Open3D-semantics ICP the reference uses OUTSIDE the scan-to-map path: loop-closure
 * refinement and odometry constraints between submaps (same shared library, libo3dslam_icp_hip.so).
 * Paths: O3S = open3d_slam_rsl/open3d_slam/open3d_slam.
 *
 *   o3s_o3d_registration_icp     open3d::pipelines::registration::RegistrationICP(source, target, max_dist, init,
 *                                TransformationEstimationPointToPlane(), criteria)
 *                                  O3S/src/CloudRegistration.cpp:57-61 (registerClouds), O3S/src/PlaceRecognition.cpp:111,
 *                                  O3S/src/constraint_builders.cpp:60-68
 *   o3s_o3d_information_matrix   open3d::pipelines::registration::GetInformationMatrixFromPointClouds
 *                                  O3S/src/PlaceRecognition.cpp:144-145, O3S/src/constraint_builders.cpp:71-74
 *
 * fp64 like Open3D (this is a different arithmetic from the fp32 libpointmatcher chain of o3s_icp.h): the source cloud
 * is transformed incrementally by every update, correspondences are the nearest target point with squared distance
 * < max_dist^2 (exact: uniform grid + ring search; ties to the lower index), the 6x6 system J^T J x = -J^T r is solved
 * with Eigen's pivoted LDLT restated on the host, the update is Rz * Ry * Rx through quaternions, and the loop stops when
 * both |d fitness| < relative_fitness and |d rmse| < relative_rmse, or after max_iteration updates.
 * Open3D v0.15.1 is not part of the reference tree: parity is against the oracle's restatement of its published source;
 * correspondences, fitness and iteration counts agree exactly, poses to 1e-9 (the sums run in a different order).
 * Points / normals: 3 x N column-major doubles (host); poses: Eigen::Matrix4d::data() order.  Return: o3s_status.
 */
#ifndef O3S_REGISTRATION_H
#define O3S_REGISTRATION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct o3s_o3d_icp_criteria { /* open3d ICPConvergenceCriteria; defaults 1e-6, 1e-6, 30 */
  double relative_fitness;
  double relative_rmse;
  int32_t max_iteration;
} o3s_o3d_icp_criteria;

typedef struct o3s_o3d_icp_result { /* open3d RegistrationResult */
  double transformation[16];
  double fitness;          /* correspondences / source points */
  double inlier_rmse;      /* sqrt(sum d2 / correspondences) */
  int64_t correspondences; /* correspondence_set_.size() */
  int32_t iterations;      /* updates applied */
} o3s_o3d_icp_result;

void o3s_o3d_icp_default_criteria(o3s_o3d_icp_criteria* c);
int o3s_o3d_registration_icp(int device, const double* source, int64_t Ns, const double* target,
                             const double* target_normals, int64_t Nt, double max_correspondence_distance,
                             const double init[16], const o3s_o3d_icp_criteria* criteria, o3s_o3d_icp_result* result);
/* The estimation of a registration: CloudRegistrationType (O3S/include/open3d_slam/Parameters.hpp:37-45), the three branches
 * of cloudRegistrationFactory (O3S/src/CloudRegistration.cpp:16-21, 57-61, 88-101).  Every parameter set the reference ships
 * selects GeneralizedIcp for the loop-closure refinement (scan_to_map_refinement_type).
 *   O3S_O3D_POINT_TO_PLANE  TransformationEstimationPointToPlane()                      (what o3s_o3d_registration_icp runs)
 *   O3S_O3D_POINT_TO_POINT  TransformationEstimationPointToPoint(with_scaling = false)   (Eigen::umeyama over the correspondences)
 *   O3S_O3D_GENERALIZED     RegistrationGeneralizedICP(..., TransformationEstimationForGeneralizedICP(gicp_epsilon), ...):
 *                           per-point covariances C = Rx diag(eps, 1, 1) Rx^T from the normals as given
 *                           (InitializePointCloudForGeneralizedICP, GeneralizedICP.cpp) unless covariances are passed;
 *                           the source's covariances turn with the source (C <- R C R^T at init and at every update). */
typedef enum o3s_o3d_estimation_type {
  O3S_O3D_POINT_TO_PLANE = 0,
  O3S_O3D_POINT_TO_POINT = 1,
  O3S_O3D_GENERALIZED = 2
} o3s_o3d_estimation_type;
typedef struct o3s_o3d_estimation {
  int32_t type;        /* o3s_o3d_estimation_type */
  double gicp_epsilon; /* TransformationEstimationForGeneralizedICP::epsilon_ (1e-3); must be > 0 for every type */
  int32_t reserved[4];
} o3s_o3d_estimation;
/* GENERALIZED with epsilon 1e-3: what the reference's parameters select. */
void o3s_o3d_default_estimation(o3s_o3d_estimation* e);
/* RegistrationICP with the estimation `est` (o3s_o3d_registration_icp with est->type == O3S_O3D_POINT_TO_PLANE returns the same
 * bits).  Normals: 3 x N doubles, covariances: 9 x N doubles (a column-major 3 x 3 per point, Open3D's Matrix3d; symmetric: the
 * upper triangle is read), all nullable.  GENERALIZED needs normals or covariances on each cloud (covariances win, as in Open3D;
 * Open3D's KNN(20) normal estimation for a cloud with neither is not restated: O3S_ERR_BAD_SHAPE); POINT_TO_PLANE needs target
 * normals (O3S_ERR_BAD_SHAPE); POINT_TO_POINT needs neither.  An unknown type, gicp_epsilon <= 0 or a NULL cloud / pose / result /
 * est is O3S_ERR_BAD_ARGUMENT before any device call.
 * Degenerate correspondence sets.  POINT_TO_PLANE and GENERALIZED solve J^T J x = -J^T r as Eigen's LDLT does (largest-diagonal
 * pivoting, D^-1 a pseudo-inverse): an unknown whose row, column and right-hand side are exactly zero comes back exactly 0.0 (a
 * plane z = c with normals e3 under an identity init leaves the pose's x and y exactly where they were); on a system that is
 * rank-deficient only to rounding, x solves it to rounding and its component in the system's range is the minimum-norm
 * solution's, while the component along the unobserved directions is rounding noise divided by rounding-sized pivots — as with
 * Eigen, it is not specified.  POINT_TO_POINT: the update is always a proper rotation (R^T R = I, det R = +1) that attains the
 * optimum of Umeyama's objective tr(R sigma^T) and t = mean(t) - R mean(s).  Where the centred cross-covariance sigma has rank >= 2
 * (and, when det sigma < 0, a simple smallest singular value) that rotation is unique and is Eigen::umeyama's; at rank <= 1 — one
 * or two correspondences, collinear ones, copies of one pair — Open3D defines none and WHICH of the optimal rotations comes back
 * is not specified (one exact pair gives R = I). */
int o3s_o3d_registration_icp_ex(int device, const double* source, const double* source_normals, const double* source_cov,
                                int64_t Ns, const double* target, const double* target_normals, const double* target_cov,
                                int64_t Nt, double max_correspondence_distance, const double init[16],
                                const o3s_o3d_estimation* est, const o3s_o3d_icp_criteria* criteria,
                                o3s_o3d_icp_result* result);
/* info: 6 x 6, column-major (symmetric). */
int o3s_o3d_information_matrix(int device, const double* source, int64_t Ns, const double* target, int64_t Nt,
                               double max_correspondence_distance, const double T[16], double info[36]);


/* One candidate pair of a batch (host pointers; target_normals must not be NULL; init: 4x4 column-major). */
typedef struct o3s_o3d_pair {
  const double* source;
  int64_t n_source;
  const double* target;
  const double* target_normals;
  int64_t n_target;
  double init[16];
} o3s_o3d_pair;
/* RegistrationICP over independent candidate pairs — the loop-closure candidates of
 * PlaceRecognition::buildLoopClosureConstraints (O3S/src/PlaceRecognition.cpp:70-150, a serial loop in the reference)
 * or the odometry constraints between adjacent submaps (O3S/src/constraint_builders.cpp:55-75) — run concurrently on one
 * device, each pair on its own HIP stream.  Every pair gives exactly the result of o3s_o3d_registration_icp on it.
 * infos (nullable): n_pairs x 36 doubles, GetInformationMatrixFromPointClouds at each pair's final transformation
 * (PlaceRecognition.cpp:144-145), computed on the pair's registration index (the correspondences of o3s_o3d_information_matrix,
 * its sums in another order: equal to 1e-12 relative).  status: n_pairs o3s_status values; the return value is the first one that is not OK. */
int o3s_o3d_registration_icp_batch(int device, int32_t n_pairs, const o3s_o3d_pair* pairs,
                                   double max_correspondence_distance, const o3s_o3d_icp_criteria* criteria,
                                   o3s_o3d_icp_result* results, double* infos, int32_t* status);

/* computeIndicesOfOverlappingPoints (O3S/src/helpers.cpp:319-345, called at O3S/src/PlaceRecognition.cpp:103 in front of
 * the loop-closure ICP): the points of `source` (moved by source_to_target, Open3D PointCloud::Transform) and of `target`
 * that fall into voxels of edge voxel_size (getVoxelIdx, reciprocal form, VoxelHashMap.hpp:43-51) holding at least
 * min_points_per_voxel points of BOTH clouds.  The reference emits them in its unordered_map's iteration order
 * (unspecified); here: ascending index order.  idx_source / idx_target hold up to Ns / Nt entries (size_t in the
 * reference).  Points whose voxel index leaves +-2^20 (or NaN) are refused with O3S_ERR_BAD_ARGUMENT. */
int o3s_overlap_indices(int device, const double* source, int64_t Ns, const double* target, int64_t Nt,
                        const double source_to_target[16], double voxel_size, int64_t min_points_per_voxel,
                        int64_t* idx_source, int64_t* n_source, int64_t* idx_target, int64_t* n_target);

/* Work memory of the registrations above and of o3s_o3d_registration_icp_submaps[_overlap] (o3s_submap.h).  Open3D allocates its
 * KD-tree and correspondence sets per call (Registration.cpp RegistrationICP); on the device an allocation stalls every stream for
 * milliseconds, so the library keeps its work areas per device and hands them out per call.  o3s_o3d_registration_reserve sizes
 * one area for clouds of up to max_source_points / max_target_points ahead of time (a mapper calls it once with its submaps'
 * maxNumPoints, O3S param MapBuilderParameters): no registration up to those sizes allocates afterwards.  Without it the areas
 * grow on demand.  o3s_o3d_registration_release returns the idle areas of the device to the allocator. */
int o3s_o3d_registration_reserve(int device, int64_t max_source_points, int64_t max_target_points);
/* `count` areas of that size (the lanes of o3s_o3d_registration_icp_submaps_overlap_batch / o3s_o3d_registration_icp_batch: up to four). */
int o3s_o3d_registration_reserve_n(int device, int64_t max_source_points, int64_t max_target_points, int32_t count);
int o3s_o3d_registration_release(int device);

/* ---- RANSAC ---------------------------------------------------------------------------------------------------------------
 * RegistrationRANSACBasedOnCorrespondence / RegistrationRANSACBasedOnFeatureMatching (O3S/src/PlaceRecognition.cpp:81-84) with
 * TransformationEstimationPointToPoint(false), CorrespondenceCheckerBasedOnEdgeLength and CorrespondenceCheckerBasedOnDistance,
 * restated from Open3D's published source and made DETERMINISTIC: a counter-based sample stream and serial-order semantics, so the
 * result does not depend on how the device batches the work.  fp64, no FMA contraction.
 *
 * Inputs: source 3 x Ns, target 3 x Nt, correspondences 2 x K int32 (source index, target index), o3s_ransac_params.  An empty
 * result (identity, fitness 0, rmse 0, best_iteration -1) comes back when ransac_n < 3, K < ransac_n or
 * max_correspondence_distance <= 0, as in Open3D.  ransac_n > 8 is O3S_ERR_BAD_ARGUMENT.
 *
 * Iteration itr (0-based) is fully defined by (seed, itr):
 *  1. Sample.  ransac_n correspondence indices from Philox4x32-10: key (seed low word, seed high word), counter (itr low, itr
 *     high, j / 4, 0), index j = (word[j mod 4] * K) >> 32.  With an explicit sample table (H x ransac_n int32, row-major) row itr
 *     is used instead and the loop runs over min(max_iteration, H) iterations.  A sample with a repeated index is SKIPPED: the one
 *     deliberate deviation from Open3D, which draws with replacement — such a sample defines no rigid motion, and umeyama on it
 *     returns a rotation that depends on the SVD implementation.
 *  2. Edge-length check.  For every pair a < b of the sample, ds = |s_a - s_b|, dt = |t_a - t_b|: ds >= dt * similarity and
 *     dt >= ds * similarity.  It does not depend on T and runs before the estimation.
 *  3. Estimate.  T = Eigen::umeyama(source sample, target sample, false): the means, sigma = (1/n) sum (t - mt)(s - ms)^T, its SVD
 *     U S V^T, S(2) = -1 when det U det V < 0, R = U S V^T, t = mt - R ms.
 *  4. Distance check.  |T s_j - t_j| <= distance_threshold for every pair of the sample.
 *  5. Evaluate, over all K correspondences in ascending index: p = R s + t with each row as ((r0 sx + r1 sy) + r2 sz) + t,
 *     d = sqrt((dx dx + dy dy) + dz dz); the pair is an inlier when d < max_correspondence_distance; n_in counts them.  err2 sums
 *     d * d over the inliers in this fixed order: within each chunk of 512 consecutive correspondences ([0, 512), [512, 1024), ...)
 *     sequentially from 0.0 in ascending index, then the chunk sums added sequentially from 0.0 in ascending chunk order.
 *     fitness = n_in / K, rmse = sqrt(err2 / n_in), 0 when n_in is 0.
 *  6. Select with serial semantics.  est_k = max_iteration and an empty best (fitness 0, rmse 0) to start with; iterations are
 *     considered in ascending itr and the loop ends at the first itr >= est_k.  An iteration that passed the checkers replaces the
 *     best when its fitness is larger, or equal with a smaller rmse; on replacement e = log(1 - confidence) /
 *     log(1 - r^ransac_n) with r = n_in / K and r^n = ((r r) r) ..., and est_k = ceil(e) if e < est_k.  confidence = 1.0 never stops
 *     early, r = 1 stops at once.  This is what Open3D computes on one thread; the device returns exactly this for any batch size and
 *     any number of batches in flight.
 *  7. Result: the winner's transformation, fitness, rmse, its inlier pairs in ascending order (optional), the winning itr, the final
 *     est_k and the number of hypotheses evaluated (checker-passing iterations the serial loop reached). */
typedef struct o3s_ransac_params {
  double max_correspondence_distance; /* 0.75  ransac_max_correspondence_dist */
  int32_t ransac_n;                   /* 3     ransac_model_size (3 .. 8) */
  double distance_threshold;          /* 0.8   CorrespondenceCheckerBasedOnDistance */
  double edge_length_similarity;      /* 0.6   CorrespondenceCheckerBasedOnEdgeLength */
  int32_t check_distance;             /* 1; 0 switches the checker off */
  int32_t check_edge_length;          /* 1; 0 switches the checker off */
  int32_t max_iteration;              /* 10 000 000  ransac_num_iter */
  double confidence;                  /* 0.999       ransac_probability (0 .. 1) */
  uint64_t seed;                      /* 0 */
} o3s_ransac_params;
typedef struct o3s_ransac_result {
  double transformation[16]; /* Eigen::Matrix4d::data() order */
  double fitness;
  double inlier_rmse;
  int64_t correspondences; /* n_in of the winner = correspondence_set_.size() */
  int64_t best_iteration;  /* the winning itr; -1: the empty result */
  int64_t est_k;           /* the final est_k */
  int64_t evaluated;       /* hypotheses evaluated */
} o3s_ransac_result;
void o3s_ransac_default_params(o3s_ransac_params* p);
/* samples (nullable): n_samples x ransac_n int32, each in [0, K).  inlier_correspondences (nullable): 2 x K int32. */
int o3s_registration_ransac_correspondence(int device, const double* source, int64_t Ns, const double* target, int64_t Nt,
                                           const int32_t* correspondences, int64_t K, const o3s_ransac_params* params,
                                           const int32_t* samples, int64_t n_samples, o3s_ransac_result* result,
                                           int32_t* inlier_correspondences);
/* o3s_feature_correspondences (dim x N features, o3s_cloud_ops.h) chained into the above.  inlier_correspondences (nullable):
 * 2 x Ns int32; n_correspondences (nullable): K, the size of the correspondence set. */
int o3s_registration_ransac_feature_matching(int device, const double* source, int64_t Ns, const double* target, int64_t Nt,
                                             const double* source_feature, const double* target_feature, int32_t dim,
                                             int32_t mutual_filter, const o3s_ransac_params* params, o3s_ransac_result* result,
                                             int32_t* inlier_correspondences, int64_t* n_correspondences);
/* Steps 1 - 5 for H hypotheses, nothing selected: rows 0 .. H - 1 of `samples`, or (samples NULL) the Philox draws of iterations
 * first_iteration .. first_iteration + H - 1.  Per hypothesis: outcome (0 passed, 1 repeated index, 2 edge-length check failed,
 * 3 distance check failed), the transformation (16 doubles, Eigen order; estimated for outcomes 0 and 3, else zero rotation),
 * and for outcome 0 n_in and err2 (0 otherwise).  transformations, n_in, err2 are nullable. */
int o3s_ransac_evaluate_samples(int device, const double* source, int64_t Ns, const double* target, int64_t Nt,
                                const int32_t* correspondences, int64_t K, const o3s_ransac_params* params, const int32_t* samples,
                                int64_t first_iteration, int64_t H, int32_t* outcome, double* transformations, int64_t* n_in,
                                double* err2);
/* The work area of the RANSAC entries (o3s_submap_registration_ransac included): leased per call from a pool per device and grown on
 * demand; o3s_ransac_reserve sizes one for up to max_correspondences ahead of time, so that repeated closures do not allocate;
 * o3s_ransac_release returns the device's idle areas to the allocator. */
int o3s_ransac_reserve(int device, int64_t max_correspondences);
int o3s_ransac_release(int device);

#ifdef __cplusplus
}
#endif
#endif /* O3S_REGISTRATION_H */
