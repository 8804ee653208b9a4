/*
 * o3s_outlier_removal.h — C ABI of the two Open3D outlier filters on device clouds (same shared library, libo3dslam_icp_hip.so):
 *   PointCloud::RemoveRadiusOutliers(nb_points, search_radius)          (Open3D v0.15.1, geometry/PointCloud.cpp)
 *   PointCloud::RemoveStatisticalOutliers(nb_neighbors, std_ratio)      (Rusu et al.)
 * on host arrays, on a resident submap's sparse map (in place) and on a resident pre-processed scan (in place).  Open3D is not
 * part of the reference tree; parity is against a restatement of its published source (tests/outlier_ref.py) written from the
 * contract below.  All arithmetic is IEEE fp64 without FMA contraction.
 *
 * Contract
 *  distance     d2(i, j) = ((dx dx + dy dy) + dz dz) with dx = x_i - x_j, ... : the squared distance of o3s_estimate_normals
 *               (o3s_cloud_ops.h); the code base has one definition.  The neighbour sets are exact (uniform grid, ring search);
 *               which grid cell the search uses never shows in a result.
 *  non-finite   a point with a NaN or infinite coordinate is no one's neighbour, has no neighbours and is always removed.
 *  order        kept points stay in input order; normals (and, on a submap, colours) follow their points.
 *  radius       (kind 1)  point i is kept iff #{ j : d2(i, j) < value * value } > nb.  The count includes i itself; the comparison
 *               on the squared distance is strict.  nb < 1 or value <= 0 (or NaN): O3S_ERR_BAD_ARGUMENT.
 *  statistical  (kind 2)  per point k = min(nb, number of finite points); the k nearest points, itself included, ascending
 *               (d2, index); avg_i = (sum of sqrt(d2)) / k, the sqrt correctly rounded, the sum sequential from 0.0 in that order.
 *               A non-finite point has avg_i = -1.  valid = number of points with at least one neighbour (= the finite points).
 *               mean = (sum over avg > 0 of avg) / valid;  std = sqrt((sum over avg > 0 of (avg - mean)^2) / (valid - 1)) — for
 *               valid == 1 that is 0 / 0 = NaN;  thr = mean + value * std.  Point i is kept iff avg_i > 0 && avg_i < thr: a NaN
 *               threshold keeps nothing, and a cloud of coincident points keeps nothing.  The two cloud-wide sums are fp64 block
 *               partials folded in block order: an order that depends on N alone (no floating-point atomics), so two calls give
 *               the same bits; against a sequential sum they differ by at most N 2^-52 times the sum of the terms' magnitudes.
 *               nb < 1, nb > 32 (the bound o3s_estimate_normals serves) or value <= 0 (or NaN): O3S_ERR_BAD_ARGUMENT.
 *  kind 0       O3S_OK: nothing is touched and nothing is launched (no device is needed).  Any other kind: O3S_ERR_BAD_ARGUMENT.
 *  N == 0       O3S_OK with n_out == 0.  N >= 2^31: O3S_ERR_BAD_ARGUMENT.
 * Argument checks come before any device work.  Work memory comes from a per-device pool: a second call of the same size
 * allocates nothing.
 *
 * (The header lives in a directory of its own: include/ itself holds the headers of the first device-side ABI, one list.)
 * Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_OUTLIER_REMOVAL_H
#define O3S_OUTLIER_REMOVAL_H

#include <stdint.h>

#include "../o3s_scan.h"
#include "../o3s_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct o3s_outlier_params {
  int32_t kind;  /* 0 = none, 1 = radius, 2 = statistical */
  int32_t nb;    /* radius: nb_points; statistical: nb_neighbors */
  double value;  /* radius: search_radius [m]; statistical: std_ratio */
} o3s_outlier_params;

/* Host arrays.  pts: 3 x N doubles; normals nullable (then out_normals is not written).  out_pts / out_normals: room for N
 * points; *n_out are written.  out_indices (nullable, N): the kept input indices, ascending.  avg_dist (nullable, N): avg_i of
 * every input point, statistical only (left alone by the radius filter).  stats4 (nullable): mean, std, thr, valid —
 * statistical only.  With kind 0 nothing is written, *n_out included. */
int o3s_remove_outliers(int device, const o3s_outlier_params* p, const double* pts, const double* normals, int64_t N,
                        double* out_pts, double* out_normals, int64_t* out_indices, int64_t* n_out, double* avg_dist,
                        double stats4[4]);

/* The sparse map of a resident submap, in place: bit for bit and in order what o3s_remove_outliers returns on the downloaded
 * cloud.  A pending insert is completed first; the survivors are compacted by the path o3s_submap_carve uses (normals and colours
 * follow), and what a carve leaves behind is what this call leaves behind: the feature set, the voxel-map snapshot and an ICP
 * reference taken from the map describe the map as it was.  n_removed, stats4 nullable. */
int o3s_submap_remove_outliers(o3s_submap* m, const o3s_outlier_params* p, int64_t* n_removed, double stats4[4]);

/* A resident pre-processed scan, in place: the merge cloud is filtered, then the match cloud is rebuilt as the
 * scan_matcher_cropper crop (identity pose, as o3s_scan_preprocess applies it) of the filtered merge cloud.  Voxel order is kept
 * (the compaction preserves order); the reading in the ICP layout is rebuilt by the next o3s_scan_set_reading.  n_merge / n_match
 * (nullable): the new sizes. */
int o3s_scan_remove_outliers(o3s_scan* s, const o3s_cropper* scan_matcher_cropper, const o3s_outlier_params* p,
                             int64_t* n_merge, int64_t* n_match);

#ifdef __cplusplus
}
#endif
#endif /* O3S_OUTLIER_REMOVAL_H */
