/*
 * o3s_constraints.h — C ABI of the odometry constraints between RESIDENT submaps (same shared library, libo3dslam_icp_hip.so):
 * buildConstraint(source, target, isComputeOverlap = true, ..., isSkipIcpRefinement = true) of O3S/src/constraint_builders.cpp:43-90
 * for n pairs in one call — the overlap selection at T_k (computeIndicesOfOverlappingPoints), then Open3D's
 * GetInformationMatrixFromPointClouds on the two selections at T_k.  No ICP runs: that is the path every shipped configuration
 * takes (isRefineOdometryConstraintsBetweenSubmaps = false); the refinement itself is o3s_o3d_registration_icp_submaps_overlap.
 *
 * Contract, pair by pair:
 *  selection       exactly o3s_overlap_indices (o3s_cloud_ops.h) on the two map clouds at T_k: getVoxelIdx in its reciprocal form, a
 *                  voxel counts when it holds at least min_points_per_voxel points of BOTH clouds, ascending index order.
 *  correspondences for every selected source point q = T_k . p (Open3D's PointCloud::Transform, skipped for an identity) the nearest
 *                  selected target point t with d2 = ((qx - tx)^2 + (qy - ty)^2) + (qz - tz)^2 < max_correspondence_distance^2
 *                  (strict); among equals the lowest target index.  The arithmetic is that of o3s_o3d_information_matrix.
 *  matrix          Open3D's G^T G over the correspondences, G's three rows built from the TARGET point; fp64 sums in a fixed order
 *                  that depends on the pair alone: pair k's 36 doubles are the same bits from run to run, alone or in a batch of
 *                  any composition, at any position.
 *  inputs          the maps are read where they lie (no copy, no normals needed); a pending insert is completed first; the submaps
 *                  are left as they are; a submap may appear in several pairs, as source and as target.
 *  statuses[k]     O3S_OK; O3S_ERR_EMPTY_REFERENCE for an empty submap or an empty selection; O3S_ERR_BAD_ARGUMENT for a non-finite
 *                  coordinate or a voxel index beyond +-2^20 (as o3s_overlap_indices), or a pair of 2^31 points or more.  Both give
 *                  a zero matrix and zero counts, neither stops the other pairs and neither is an error of the call.
 * The call itself fails with O3S_ERR_BAD_ARGUMENT, before any device work and without touching an output, on: n < 0; a NULL
 * sources / targets / infos / statuses array or a NULL submap with n > 0; a voxel size or a radius that is not positive and
 * finite; a radius below overlap_voxel_size * 2^-20 (the search grid's cells are numbered in 64 bits); min_points_per_voxel < 1;
 * submaps on more than one device; a non-finite T.  n == 0 is O3S_OK.  There is no cap on n.
 *
 * All pairs are enqueued together on one stream (pair tables on the device, no host thread); the host waits once.  Work memory
 * comes from the per-device registration pool (o3s_o3d_registration_reserve): a second call of the same sizes allocates nothing.
 *
 * (The header lives in a directory of its own: include/ itself holds the headers of the first device-side ABI, one list.)
 * Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_CONSTRAINTS_H
#define O3S_CONSTRAINTS_H

#include <stdint.h>

#include "../o3s_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Ts: n x 16 doubles (column-major 4 x 4 each), NULL: every pair at the identity.  infos: n x 36 doubles, column-major 6 x 6.
 * n_overlaps (nullable): n x 2, the sizes of the source's and the target's selection.  n_correspondences (nullable): n. */
int o3s_submaps_odometry_constraints(int32_t n, const o3s_submap* const* sources, const o3s_submap* const* targets,
                                     const double* Ts, double overlap_voxel_size, int64_t min_points_per_voxel,
                                     double max_correspondence_distance, double* infos, int64_t* n_overlaps,
                                     int64_t* n_correspondences, int32_t* statuses);

#ifdef __cplusplus
}
#endif
#endif /* O3S_CONSTRAINTS_H */
