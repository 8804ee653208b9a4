/*
 * o3s_keypoints.h — C ABI of Intrinsic Shape Signatures keypoints on device clouds (same shared library,
 * libo3dslam_icp_hip.so):
 *   geometry::keypoint::ComputeISSKeypoints(cloud, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)
 *                                                        (Open3D v0.15.1, geometry/Keypoint.cpp; Zhong 2009)
 * on host arrays and on the resident feature set of a submap, where it reduces the sparse cloud, its normals and its FPFH
 * columns to the keypoints, so that the place-recognition search runs on salient points only.  Open3D is not part of the
 * reference tree; parity is against a numpy restatement written from this contract (tests/iss_ref.py).  All arithmetic is
 * IEEE fp64 without FMA contraction.
 *
 * Contract (the rules in the order they apply)
 *  distance     d2(i, j) = ((dx dx + dy dy) + dz dz), the squared distance of o3s_estimate_normals, o3s_remove_outliers and
 *               o3s_cluster_dbscan: the code base has one definition.  j is a neighbour of i at radius r iff d2(i, j) < r * r.
 *               The comparison is strict; i is its own neighbour.  The search is exact (uniform grid); which grid cell it
 *               uses never shows in a neighbour set.
 *  non-finite   a point with a NaN or infinite coordinate is no one's neighbour, has saliency 0 and is never a keypoint.
 *  resolution   if salient_radius == 0 || non_max_radius == 0, BOTH are replaced as in Open3D: res = (sum over the finite
 *               points of sqrt(d2 to the nearest other finite point)) / (number of finite points), salient = 6 res,
 *               non_max = 4 res.  The sum is formed from fp64 block partials folded in block order: it depends on N alone,
 *               not on a launch.  Fewer than two finite points: res = 0 and no keypoints.  The radii actually used are
 *               returned (radii2).
 *  saliency     n_i = #{ j : d2(i, j) < salient^2 }.  n_i < min_neighbors: sal_i = 0.  Otherwise
 *               S_i = sum_j (p_j - p_i)(p_j - p_i)^T, unnormalised and centred on the query, not on the mean (Open3D's
 *               ComputeScatterMatrix).  S_i all zero: sal_i = 0.  Otherwise, with the eigenvalues l1 >= l2 >= l3 of S_i,
 *               sal_i = l3 if l2 / l1 < gamma_21 && l3 / l2 < gamma_32, else 0.
 *  non-maximum  i is a keypoint iff sal_i > 0, #{ j : d2(i, j) < non_max^2 } >= min_neighbors, and no j of that set has
 *               sal_j > sal_i.  The comparison is strict: exact ties keep both (Open3D's IsLocalMaxima).
 *  order        keypoints are reported as ascending input indices; payloads (normals, FPFH columns) follow their points.
 *  bits         S_i is summed in the order of the grid walk, which depends on the grid cell: the bits of sal_i are not part
 *               of the contract beyond the bound tests/iss_ref.py states.  Two calls on the same cloud with the same
 *               parameters on the same build give the same bits; the host-array and the resident entry give the same bits on
 *               the same points; two coincident points get the same saliency bits and the same flag.
 *  off          min_neighbors == 0 (the zeroed struct): O3S_OK, nothing is read, written or launched, and no device is
 *               needed; the other fields mean nothing then.
 *  bad          min_neighbors < 0, a negative, NaN or infinite radius, a gamma that is NaN or <= 0, N < 0 or N >= 2^31:
 *               O3S_ERR_BAD_ARGUMENT before any device work, outputs untouched.
 *  N == 0       O3S_OK with n_keypoints = 0.
 * The resident entries check the parameters before they look at the handle.  Work memory comes from a per-device pool: a
 * second call of the same size allocates nothing.
 *
 * (The header lives in a directory of its own: include/ itself holds the headers of the first device-side ABI, one list.)
 * Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_KEYPOINTS_H
#define O3S_KEYPOINTS_H

#include <stdint.h>

#include "../o3s_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct o3s_iss_params {
  double salient_radius; /* 0 = from the cloud's resolution */
  double non_max_radius; /* 0 = from the cloud's resolution */
  double gamma_21;       /* Open3D default 0.975 */
  double gamma_32;       /* Open3D default 0.975 */
  int32_t min_neighbors; /* Open3D default 5; 0 = off */
  int32_t reserved;
} o3s_iss_params;

/* Host arrays.  pts: 3 x N doubles.  normals nullable (then out_normals is not written); they ride along.  out_pts /
 * out_normals / out_indices (nullable): room for N; *n_keypoints are written.  saliency (nullable, N): sal_i of every INPUT
 * point.  radii2 (nullable): the salient and the non-max radius used. */
int o3s_iss_keypoints(int device, const o3s_iss_params* p, const double* pts, const double* normals, int64_t N,
                      double* out_pts, double* out_normals, int64_t* out_indices, int64_t* n_keypoints, double* saliency,
                      double radii2[2]);

/* The resident feature set of a submap (o3s_submap_compute_features must have run, else O3S_ERR_NOT_INITIALIZED): the
 * keypoints of the SPARSE cloud, then the sparse points, the sparse normals and the 33-double FPFH columns compacted to
 * the keypoints, in order; o3s_submap_features_size shrinks to *n_keypoints.  The descriptors were computed on the full
 * sparse cloud (an FPFH needs its whole neighbourhood); a second o3s_submap_compute_features rebuilds the full set.
 * out_indices (nullable, room for the old features_size): which sparse points stayed.  The map cloud, the voxel-map
 * snapshot and an ICP reference are untouched.  n_keypoints, radii2 nullable. */
int o3s_submap_select_keypoints(o3s_submap* m, const o3s_iss_params* p, int64_t* out_indices, int64_t* n_keypoints,
                                double radii2[2]);

/* Labels only, nothing moves: flags (nullable, one int32 per sparse point: 1 = keypoint, 0 = not) and saliency (nullable,
 * one double per sparse point) of the resident sparse cloud — what o3s_iss_keypoints returns on the downloaded cloud, bit
 * for bit.  n_keypoints, radii2 nullable. */
int o3s_submap_feature_keypoints(const o3s_submap* m, const o3s_iss_params* p, int32_t* flags, double* saliency,
                                 int64_t* n_keypoints, double radii2[2]);

#ifdef __cplusplus
}
#endif
#endif /* O3S_KEYPOINTS_H */
