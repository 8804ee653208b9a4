/*
 * o3s_clustering.h — C ABI of DBSCAN clustering and small-cluster removal on device clouds (same shared library,
 * libo3dslam_icp_hip.so):
 *   PointCloud::ClusterDBSCAN(eps, min_points)          (Open3D v0.15.1, geometry/PointCloudCluster.cpp; Ester et al.)
 * and "drop every cluster below n points", on host arrays, on a resident submap's sparse map and on a resident pre-processed
 * scan.  Open3D is not part of the reference tree; parity is against a restatement of its published source
 * (tests/dbscan_ref.py), which holds both Open3D's sequential loop and the closed form below and shows that they agree.  Every
 * result is an integer: there is no tolerance anywhere, and no launch order, grid cell size or arrival order of an atomic shows.
 *
 * Contract
 *  distance     d2(i, j) = ((dx dx + dy dy) + dz dz) with dx = x_i - x_j, ... in IEEE fp64 without FMA contraction: the squared
 *               distance of o3s_estimate_normals and o3s_remove_outliers; the code base has one definition.
 *  neighbours   j is a neighbour of i iff both are finite and d2(i, j) < eps * eps.  The comparison is strict; i is its own
 *               neighbour.  The search is exact (uniform grid); which grid cell it uses never shows in a result.
 *  non-finite   a point with a NaN or infinite coordinate is no one's neighbour, has none, and has label -1.
 *  core         count_i = number of neighbours of i, itself included; i is core iff count_i >= min_points.
 *  clusters     the connected components of the graph on the core points with an edge between core i and core j iff they are
 *               neighbours.  The id of a cluster is the rank, ascending from 0, of its smallest core index among all clusters'
 *               smallest core indices.  (Open3D's loop over ascending idx opens a cluster at the first unlabelled core point,
 *               and the expansion labels the whole component.)
 *  border       a finite non-core point with at least one core neighbour gets the minimum cluster id over its core neighbours.
 *               (Open3D expands clusters in label order and never relabels a point whose label is >= 0.)
 *  noise        every other point: -1.
 *  outputs      n_clusters, and size[c] = the number of points, border included, with label c.
 *  removal      point i is kept iff label_i >= 0 and size[label_i] >= min_cluster_size; with min_cluster_size <= 1 only noise
 *               goes.  Kept points stay in input order; normals (and, on a submap, colours) follow their points.
 *  off          min_points == 0 (the zeroed struct): O3S_OK, nothing is read, written or launched, and no device is needed;
 *               the other fields mean nothing then.
 *  bad          min_points < 0, eps not > 0 or not finite, min_cluster_size < 0, N < 0 or N >= 2^31: O3S_ERR_BAD_ARGUMENT
 *               before any device work, outputs untouched.
 *  N == 0       O3S_OK with n_clusters = 0 and n_out = 0.
 * The resident entries check the parameters before they look at the handle's device.  Work memory comes from a per-device
 * pool: a second call of the same size allocates nothing.
 *
 * (The header lives in a directory of its own: include/ itself holds the headers of the first device-side ABI, one list.)
 * Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_CLUSTERING_H
#define O3S_CLUSTERING_H

#include <stdint.h>

#include "../o3s_scan.h"
#include "../o3s_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct o3s_dbscan_params {
  double eps;               /* neighbourhood radius [m] */
  int32_t min_points;       /* 0 = off; a point with at least this many neighbours, itself included, is core */
  int32_t min_cluster_size; /* removal only: clusters with fewer points go (0 and 1: only noise goes) */
} o3s_dbscan_params;

/* Host arrays.  pts: 3 x N doubles.  labels: N; *n_clusters; cluster_sizes (nullable, room for N): the first *n_clusters are
 * written.  min_cluster_size is checked and otherwise unused. */
int o3s_cluster_dbscan(int device, const o3s_dbscan_params* p, const double* pts, int64_t N, int32_t* labels,
                       int32_t* n_clusters, int32_t* cluster_sizes);

/* Host arrays, removal.  normals nullable (then out_normals is not written).  out_pts / out_normals: room for N points; *n_out are
 * written.  out_indices (nullable, N): the kept input indices, ascending.  labels (nullable, N): the labels of the INPUT points.
 * n_clusters nullable. */
int o3s_remove_small_clusters(int device, const o3s_dbscan_params* p, const double* pts, const double* normals, int64_t N,
                              double* out_pts, double* out_normals, int64_t* out_indices, int64_t* n_out, int32_t* labels,
                              int32_t* n_clusters);

/* The sparse map of a resident submap, clustered: labels (host, room for o3s_submap_size(m) points) are what
 * o3s_cluster_dbscan returns on the downloaded cloud.  A pending insert is completed first; nothing in the map changes. */
int o3s_submap_cluster_dbscan(o3s_submap* m, const o3s_dbscan_params* p, int32_t* labels, int32_t* n_clusters);

/* The sparse map of a resident submap, in place: bit for bit and in order what o3s_remove_small_clusters returns on the
 * downloaded cloud.  A pending insert is completed first; the survivors are compacted by the path o3s_submap_carve uses (normals
 * and colours follow), and what a carve leaves behind is what this call leaves behind: the feature set, the voxel-map snapshot
 * and an ICP reference taken from the map describe the map as it was.  n_removed, n_clusters nullable. */
int o3s_submap_remove_small_clusters(o3s_submap* m, const o3s_dbscan_params* p, int64_t* n_removed, int32_t* n_clusters);

/* A resident pre-processed scan, in place: the merge cloud is filtered, then the match cloud is rebuilt as the
 * scan_matcher_cropper crop (identity pose, as o3s_scan_preprocess applies it) of the filtered merge cloud.  Order is kept; the
 * reading in the ICP layout is rebuilt by the next o3s_scan_set_reading.  n_merge / n_match (nullable): the new sizes. */
int o3s_scan_remove_small_clusters(o3s_scan* s, const o3s_cropper* scan_matcher_cropper, const o3s_dbscan_params* p,
                                   int64_t* n_merge, int64_t* n_match);

#ifdef __cplusplus
}
#endif
#endif /* O3S_CLUSTERING_H */
