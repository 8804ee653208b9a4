/*
 * o3s_plane_segmentation.h — C ABI of RANSAC plane segmentation on device clouds (same shared library, libo3dslam_icp_hip.so):
 *   PointCloud::SegmentPlane(distance_threshold, ransac_n, num_iterations)
 *       (Open3D v0.15.1, geometry/PointCloudSegmentation.cpp, TriangleMesh::ComputeTrianglePlane, GetPlaneFromPoints;
 *        Fischler & Bolles)
 * on host arrays, on a resident submap's sparse map and on a resident pre-processed scan, plus a peel of several planes one
 * after another.  Open3D is not part of the reference tree; parity is against a restatement of its published source in closed
 * form (tests/plane_ref.py), made deterministic the way the registration RANSAC was (o3s_registration.h, "RANSAC"): a
 * counter-based sample stream and a serial-order selection rule, so that no batch size, launch order or arrival order of an
 * atomic shows in a result.  All arithmetic is IEEE fp64 with +, -, x, / and sqrt in the order written below, without FMA
 * contraction: every comparison against the restatement is exact.
 *
 * Contract: ONE SEGMENTATION of a cloud of M points in a given order
 *  sample       of iteration itr (0-based): ransac_n indices from Philox4x32-10 exactly as the registration RANSAC draws them:
 *               key = (seed low, seed high), counter = (itr low, itr high, j / 4, k), index j = (word[j mod 4] * M) >> 32.  The
 *               last counter word k is the plane number of the peel (0 for a single plane: the stream the registration RANSAC
 *               reads).  With an explicit sample table (H x ransac_n int32) row itr is used and the loop runs over
 *               min(num_iterations, H) iterations; a table is allowed only with max_planes == 1.
 *  outcome      of a sample, decided in this order:
 *                 O3S_PLANE_REPEATED    two equal indices among the ransac_n (Open3D draws without replacement: the deliberate
 *                                       deviation, the registration RANSAC's)
 *                 O3S_PLANE_NONFINITE   one of the FIRST THREE points has a NaN or infinite coordinate
 *                 O3S_PLANE_DEGENERATE  the normal n below has norm exactly 0
 *                 O3S_PLANE_PASS        everything else; only a PASS is evaluated
 *  plane        the first three indices define it, as in Open3D: e0 = p1 - p0, e1 = p2 - p0, n = e0 x e1 with every component
 *               a*b - c*d, norm = sqrt((nx nx + ny ny) + nz nz), (a, b, c) = n / norm, d = -((a p0x + b p0y) + c p0z).
 *  evaluation   over all M points in ascending index: dist_i = |((a x + b y) + c z) + d|; point i is an inlier iff
 *               dist_i < distance_threshold (strict; false for a non-finite point).  n_in counts the inliers; err sums dist_i —
 *               NOT its square: Open3D 0.15.1 has `error += distance` — in the code base's fixed order: within each chunk of
 *               512 consecutive points sequentially from 0.0 in ascending index, then the chunk sums sequentially from 0.0 in
 *               ascending chunk order.  fitness = n_in / M; rmse = err / sqrt(n_in), 0 when n_in is 0.
 *  selection    rule 6 of the registration RANSAC: est_k = num_iterations, best empty; iterations in ascending order, ending at
 *               the first itr >= est_k; a PASS replaces the best when its fitness is larger, or equal with a smaller rmse; on a
 *               replacement e = log(1 - confidence) / log(1 - r^ransac_n) with r = n_in / M and r^n = ((r r) r) ..., and
 *               est_k = ceil(e) if e < est_k.  confidence 1.0 never stops early (Open3D 0.15.1 has no early stop).
 *  inliers      the ascending indices with dist_i < distance_threshold under the WINNING SAMPLE's plane.
 *  refit        GetPlaneFromPoints over the inlier list: centroid c = the three coordinate sums / the inlier count; with
 *               r = p - c the six sums xx, xy, xz, yy, yz, zz of products; every sum in the chunk-of-512 order, chunks counted
 *               along the inlier list.  det_x = yy zz - yz yz, det_y = xx zz - xz xz, det_z = xx yy - xy xy;
 *                 det_x > det_y and det_x > det_z:  normal = (det_x, xz yz - xy zz, xy yz - xz yy)
 *                 else det_y > det_z:               normal = (xz yz - xy zz, det_y, xy xz - yz xx)
 *                 else:                             normal = (xy yz - xz yy, xy xz - yz xx, det_z)
 *               normalised by sqrt((a a + b b) + c c) — a zero norm gives the model (0, 0, 0, 0) — and
 *               d = -((a cx + b cy) + c cz).  The sign is what comes out.  The returned inliers stay those of the winning
 *               sample's plane, not of the refit (Open3D does the same).
 *  result       model[4], the inlier indices, n_inliers, best_iteration, the final est_k and `evaluated` = the number of PASS
 *               iterations the serial loop reached.  No PASS, or M < ransac_n: model (0, 0, 0, 0), no inliers,
 *               best_iteration -1, est_k = the iterations asked for, O3S_OK.
 * Contract: THE PEEL (max_planes > 1)
 *               plane k is one segmentation of the remaining cloud: the points no earlier plane took, non-finite ones included,
 *               in input order; M, the sample indices and the chunks are those of that compacted cloud.  The peel ends before
 *               reporting plane k if its final inlier count is below min_inliers, if nothing passed or if M < ransac_n.
 *               labels[i] = the plane that took point i, else -1; n_planes, models[n_planes][4], counts[n_planes].
 *  off          num_iterations == 0 (the zeroed struct): O3S_OK, nothing is read, written or launched, no device is needed and no
 *               pointer is dereferenced; the other fields mean nothing then.
 *  bad          distance_threshold not > 0 or not finite, confidence outside (0, 1], num_iterations < 0, ransac_n outside 3..8,
 *               max_planes outside 1..16, min_inliers < 0, N < 0 or N >= 2^31, a sample table together with max_planes > 1, a
 *               table index outside [0, N): O3S_ERR_BAD_ARGUMENT before any device work, outputs untouched.
 *  N == 0       O3S_OK with empty results.
 * The resident entries check the parameters before they look at the handle's device.  Work memory is leased per call from a
 * per-device pool: a second call of the same size allocates nothing (o3s_plane_reserve sizes an area ahead of time).
 *
 * Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_PLANE_SEGMENTATION_H
#define O3S_PLANE_SEGMENTATION_H

#include <stdint.h>

#include "../o3s_scan.h"
#include "../o3s_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { O3S_PLANE_PASS = 0, O3S_PLANE_REPEATED = 1, O3S_PLANE_NONFINITE = 2, O3S_PLANE_DEGENERATE = 3 };

typedef struct o3s_plane_params {
  double distance_threshold; /* [m]; a point is an inlier iff dist < distance_threshold (strict) */
  double confidence;         /* (0, 1]; 1.0 never stops early (Open3D 0.15.1's behaviour) */
  uint64_t seed;
  int32_t num_iterations;    /* 0 = off (the zeroed struct): O3S_OK, nothing read, written or launched */
  int32_t ransac_n;          /* 3 .. 8; the first three indices of a sample define the plane, as in Open3D */
  int32_t max_planes;        /* 1 .. 16; planes peeled one after another */
  int32_t min_inliers;       /* a plane with fewer final inliers ends the peel and is not reported */
} o3s_plane_params;          /* 40 bytes */

/* confidence 1.0, ransac_n 3, num_iterations 100, max_planes 1, min_inliers 3, seed 0; distance_threshold 0: the caller's */
void o3s_plane_default_params(o3s_plane_params* p);

/* Host arrays, the first plane only (max_planes and min_inliers are checked and otherwise unused).  pts: 3 x N doubles.
 * samples (nullable): n_samples x ransac_n int32.  model: 4 doubles.  inlier_indices (nullable, room for N): the first *n_inliers
 * are written, ascending.  n_inliers, best_iteration, est_k, evaluated: nullable. */
int o3s_segment_plane(int device, const o3s_plane_params* p, const double* pts, int64_t N, const int32_t* samples,
                      int64_t n_samples, double model[4], int64_t* inlier_indices, int64_t* n_inliers, int64_t* best_iteration,
                      int64_t* est_k, int64_t* evaluated);

/* Host arrays, the peel.  labels: N.  models (room for max_planes x 4) and counts (nullable, room for max_planes): the first
 * *n_planes rows are written. */
int o3s_segment_planes(int device, const o3s_plane_params* p, const double* pts, int64_t N, int32_t* labels, int32_t* n_planes,
                       double* models, int64_t* counts);

/* The stages of one segmentation, nothing selected: iterations first_iteration .. first_iteration + count - 1 of the stream, or
 * rows 0 .. count - 1 of `samples` (then first_iteration must be 0).  outcome: count; planes (nullable): count x 4 — zeros where
 * the outcome is not PASS; n_in, err (nullable): count, zeros where not PASS.  confidence, num_iterations (unless 0: off),
 * max_planes and min_inliers are checked and otherwise unused; N >= ransac_n. */
int o3s_plane_evaluate_samples(int device, const o3s_plane_params* p, const double* pts, int64_t N, const int32_t* samples,
                               int64_t first_iteration, int64_t count, int32_t* outcome, double* planes, int64_t* n_in, double* err);

/* The sparse map of a resident submap, where it lies: what o3s_segment_planes returns on the downloaded cloud.  labels: host,
 * room for o3s_submap_size(m) points.  A pending insert is completed first; nothing in the map changes. */
int o3s_submap_segment_planes(o3s_submap* m, const o3s_plane_params* p, int32_t* labels, int32_t* n_planes, double* models,
                              int64_t* counts);

/* ... and every point a reported plane took removed, in place: the survivors are compacted by the path o3s_submap_carve and
 * o3s_submap_remove_small_clusters use (order kept, normals and colours follow), and what a carve leaves stale is left stale
 * here: the feature set, the voxel-map snapshot and an ICP reference taken from the map describe the map as it was.
 * n_removed, n_planes, models (room for max_planes x 4): nullable. */
int o3s_submap_remove_planes(o3s_submap* m, const o3s_plane_params* p, int64_t* n_removed, int32_t* n_planes, double* models);

/* A resident pre-processed scan, in place, on the terms of o3s_scan_remove_small_clusters: the merge cloud loses the points the
 * reported planes took, then the match cloud is rebuilt as the scan_matcher_cropper crop (identity pose) of the filtered merge
 * cloud.  n_merge / n_match (nullable): the new sizes; n_planes, models (room for max_planes x 4): nullable. */
int o3s_scan_remove_planes(o3s_scan* s, const o3s_cropper* scan_matcher_cropper, const o3s_plane_params* p, int64_t* n_merge,
                           int64_t* n_match, int32_t* n_planes, double* models);

/* A work area for clouds of up to max_points points and num_iterations iterations, made ahead of time in the device's pool; and
 * the idle areas of the device given back to the allocator. */
int o3s_plane_reserve(int device, int64_t max_points, int32_t num_iterations);
int o3s_plane_release(int device);
/* The device memory held by the work area that served the last call on `device` (0 before any, and after a release): the
 * steady state shows as a number that stops changing. */
int64_t o3s_plane_device_bytes(int device);

#ifdef __cplusplus
}
#endif
#endif /* O3S_PLANE_SEGMENTATION_H */
