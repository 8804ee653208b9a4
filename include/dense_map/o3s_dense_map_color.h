/*
 * o3s_dense_map_color.h — colour in the device-resident dense map (same shared library, same handle as
 * o3s_dense_map.h): the reference's ColorRangeCropper and the colour sum of o3d_slam::AggregatedVoxel.
 * Paths: O3S = open3d_slam_rsl/open3d_slam/open3d_slam.
 *
 *   o3s_color_range_crop                        ColorRangeCropper::crop          O3S/src/croppers.cpp:178-244
 *   o3s_dense_map_insert_colored                VoxelizedPointCloud::insert      O3S/src/Voxel.cpp:66-88
 *   o3s_dense_map_insert_scan_colored           Submap::insertScanDenseMap       O3S/src/Submap.cpp:98-113
 *   o3s_dense_map_insert_resident_scan_colored  the same, scan already in HBM
 *   o3s_dense_map_to_point_cloud_colored        VoxelizedPointCloud::toPointCloud O3S/src/Voxel.cpp:90-114
 *   o3s_dense_map_has_colors                    VoxelizedPointCloud::hasColors   O3S/src/Voxel.cpp:42-44
 *
 * Colours are 3 x N doubles (point-major, r g b), as open3d::geometry::PointCloud::colors_ holds them.  What the
 * reference does, kept to the bit:
 *
 *  - The colour sum of a fresh voxel starts at (1, 1, 1), NOT at zero.  The reference's initialiser is
 *    `aggregatedColor_ = Eigen::Vector3d::Constant(1, 3, 1)` (O3S/include/open3d_slam/Voxel.hpp:50): for a fixed-size
 *    type, Constant(rows, cols, value) ignores rows and cols in the assertion-free build the reference ships and gives
 *    `value` in every component.  One white point therefore gives the colour (2, 2, 2).  This is restated on purpose.
 *  - The colour of a voxel is its sum divided by the number of ALL points aggregated into it, coloured or not
 *    (getAggregatedColor, Voxel.cpp:24-26): clouds without colours dilute it, and it may exceed 1.
 *  - has_colors is sticky (isHasColors_): once a coloured cloud has been aggregated, every live voxel reports a colour,
 *    (1, 1, 1) / n for a voxel that never saw one.  o3s_dense_map_clear leaves it as it leaves has_normals.
 *  - A carved voxel is destroyed (removeKey); a later point in that cell starts from (1, 1, 1) again.
 *  - o3s_dense_map_transform leaves the colour sums alone (the voxel is copied, Voxel.cpp:57).
 *  - o3d_slam::transform assigns the colours once (`out->colors_ = cloud.colors_`, O3S/src/helpers.cpp:291), after its
 *    near-identity branch has copied the whole cloud: for a pose within 1e-4 of the identity the cloud holds 2 K
 *    points, 2 K normals and K colours, no longer "HasColors()", and that scan adds no colour and does not set
 *    has_colors.  Its 2 K points and normals are aggregated as before.
 *  - The carving cadence and the carve with the RAW scan do not depend on colours: a scan whose points are all
 *    rejected by colour inserts nothing, still counts, and still carves.
 *
 * A map that never meets a colour holds no colour sums and does exactly the device work it did before this header.
 * Every entry with its colour argument NULL is its counterpart of o3s_dense_map.h.  Return: o3s_status.
 */
#ifndef O3S_DENSE_MAP_COLOR_H
#define O3S_DENSE_MAP_COLOR_H

#include <stdint.h>

#include "../o3s_dense_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ColorRangeCropper::crop: keeps, in input order, the points whose colour c satisfies rgb_min <= c <= rgb_max in every
 * component (inclusive; a NaN component fails), with their colours, normals and covariances (9 doubles per point).
 * rgb_min / rgb_max NULL: the reference's defaults (0, 0, 0) / (1, 1, 1).  colors NULL: a cloud without colours is
 * returned unchanged — everything is copied.  normals, covariances: nullable, with their outputs.  Output buffers hold
 * N entries; *n_out = points kept. */
int o3s_color_range_crop(int device, const double rgb_min[3], const double rgb_max[3], const double* pts,
                         const double* normals, const double* colors, const double* covariances, int64_t N,
                         double* out_pts, double* out_normals, double* out_colors, double* out_covariances,
                         int64_t* n_out);

/* 1 once a cloud with colours has been aggregated (isHasColors_). */
int o3s_dense_map_has_colors(const o3s_dense_map* m);

/* Slots of the voxel table (a power of two, at least twice the voxels and tombstones it holds; 0 for an empty map):
 * grows when an insert re-hashes.  Tests and memory accounting. */
int64_t o3s_dense_map_capacity(const o3s_dense_map* m);

/* o3s_dense_map_insert with colours.  colors NULL: exactly o3s_dense_map_insert.  A refused insert (a voxel index out
 * of range: O3S_ERR_BAD_ARGUMENT) leaves the map, colour sums and flags included, as it was. */
int o3s_dense_map_insert_colored(o3s_dense_map* m, const double* pts, const double* normals, const double* colors,
                                 int64_t N);

/* o3s_dense_map_insert_scan with the colour crop between the volume crop and the transform (Submap.cpp:100-102) and
 * the near-identity rule above.  raw_colors NULL: exactly o3s_dense_map_insert_scan (the bounds are not looked at). */
int o3s_dense_map_insert_scan_colored(o3s_dense_map* m, const o3s_cropper* dense_map_cropper, const double rgb_min[3],
                                      const double rgb_max[3], const double* raw_pts, const double* raw_normals,
                                      const double* raw_colors, int64_t N, const double T_map_sensor[16],
                                      const o3s_dense_carving_params* carving, int64_t* n_removed);

/* The same with the raw scan that o3s_scan_preprocess left in HBM: points and normals are read where they are, only
 * the colours (host, 3 x n_colors) are uploaded.  n_colors must be the number of raw points of the scan, else
 * O3S_ERR_BAD_SHAPE and the map is untouched.  raw_colors NULL: exactly o3s_dense_map_insert_resident_scan. */
int o3s_dense_map_insert_resident_scan_colored(o3s_dense_map* m, const o3s_cropper* dense_map_cropper,
                                               const double rgb_min[3], const double rgb_max[3], const o3s_scan* scan,
                                               const double* raw_colors, int64_t n_colors,
                                               const double T_map_sensor[16], const o3s_dense_carving_params* carving,
                                               int64_t* n_removed);

/* o3s_dense_map_to_point_cloud plus the colour of every voxel (sum / count): same order, and the same bits in
 * everything that entry returns.  colors: nullable; asking for them on a map whose has_colors is 0 returns
 * O3S_ERR_BAD_SHAPE (as o3s_submap_download_colors does). */
int o3s_dense_map_to_point_cloud_colored(const o3s_dense_map* m, double* pts, double* normals, double* colors,
                                         int32_t* keys, int32_t* counts, int64_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* O3S_DENSE_MAP_COLOR_H */
