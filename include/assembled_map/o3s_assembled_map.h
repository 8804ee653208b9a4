/*
 * o3s_assembled_map.h — C ABI of the assembled map: the map clouds of several device-resident submaps read as ONE cloud, on the
 * device (same shared library, libo3dslam_icp_hip.so).  Plain C99.
 * Paths: O3S = open3d_slam_rsl/open3d_slam/open3d_slam, ROS = open3d_slam_rsl/ros/open3d_slam_ros.
 *
 *   o3s_assembled_map_build, voxel_size <= 0   Mapper::getAssembledMapPointCloud          O3S/src/Mapper.cpp:506-538
 *                                              (what SlamWrapper::saveMap writes,          O3S/src/SlamWrapper.cpp:545-568)
 *   o3s_assembled_map_build, voxel_size > 0    + Open3D v0.15.1 VoxelDownSample on it      O3S/src/helpers.cpp:108-115
 *                                              (SlamWrapperRos::publishMaps, every         ROS/src/SlamWrapperRos.cpp:420-442,
 *                                              visualizeEveryNmsec_ = 250 ms, at           O3S/include/open3d_slam/Parameters.hpp:188-190)
 *                                              assembledMapVoxelSize_ = 0.1 and again at
 *                                              submapVoxelSize_ for the `submaps` topic)
 *
 * In the reference each getMapPointCloudCopy takes the submap's map mutex (O3S/src/Submap.cpp:210-214) and the concatenation and
 * the down-sampling are host loops over a cloud that only grows.  Here the submaps stay where they are: a segment table (one
 * entry per non-empty submap: its point / normal / colour arrays and the ordinal of its first point in the concatenation) is
 * written to the device and the kernels read the K arrays as one cloud; nothing crosses the bus but that table and, when asked
 * for, the result.
 *
 * Conventions are those of o3s_submap.h: points / normals / colours are 3 x N column-major doubles, fp64 arithmetic without FMA
 * contraction.  Return: o3s_status.  Not here: the PCD writer (host I/O), the per-submap palette colours of
 * assembleColoredPointCloud (that branch is dead in the reference: cloud->HasColors() on a fresh cloud is false,
 * ROS/src/helpers_ros.cpp:60, so the `submaps` topic is points only — attrs = 0 here), the dense maps.
 */
#ifndef O3S_ASSEMBLED_MAP_H
#define O3S_ASSEMBLED_MAP_H

#include <stdint.h>

#include "../o3s_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The result cloud and the work area of its builds, resident on `device`.  Every array is grow-only: a caller that builds
 * periodically neither frees nor allocates once the object has seen its largest input (each hipFree waits for the whole device:
 * o3s_submap_hand_over).  destroy(NULL) is a no-op. */
typedef struct o3s_assembled_map o3s_assembled_map;
int o3s_assembled_map_create(int device, o3s_assembled_map** out);
void o3s_assembled_map_destroy(o3s_assembled_map* a);

/* attrs of o3s_assembled_map_build */
#define O3S_ASSEMBLE_NORMALS 1 /* bit 0: normals wanted */
#define O3S_ASSEMBLE_COLORS 2  /* bit 1: colours wanted */

/* Builds the map of maps[0] .. maps[n - 1]; *n_out (nullable) = its size.
 *
 * Input.  The virtual input is the concatenation of the submaps' map clouds in the order given, each in its current point order
 * (Mapper.cpp:524-535).  Pending inserts (o3s_submap_insert_processed) are completed first.  The submaps are only READ: after
 * the call every submap holds the same bits, the same size and the same voxel layout / merge state — the next insert into the
 * active submap still takes the merge path (o3s_submap_insert_stats).
 *
 * voxel_size <= 0: the result is exactly that concatenation (getAssembledMapPointCloud).  One launch.
 *
 * voxel_size > 0: the result is Open3D v0.15.1 VoxelDownSample of that concatenation, exactly as o3s_voxel_downsample_attr
 * (o3s_cloud_ops.h) defines it: anchor = min bound over ALL submaps - voxel_size / 2, voxel index floor((p - anchor) / voxel_size),
 * one point per voxel = the mean of its points, the mean of their normals (NOT renormalised), the mean of their colours, voxels in
 * ascending (z, y, x) index order.  The per-voxel fp64 sums run in the input order of the concatenation — submap order, then
 * point order — so a voxel that holds points of several submaps has the bits of the sequential loop over the concatenated
 * cloud, and the result depends on the ORDER of maps.
 *
 * Attributes.  The result carries normals (colours) iff bit 0 (bit 1) of attrs is set AND every non-empty submap carries them.
 * The reference appends an attribute only for the submaps that have it (Mapper.cpp:528-533); Open3D's HasNormals() / HasColors()
 * is then false for the mixed cloud, so VoxelDownSample and the PCD writer drop it.  For the plain concatenation the reference
 * returns that inconsistent cloud (fewer normals than points); here the attribute is dropped in both forms.
 *
 * Empty input.  n == 0 (maps may then be NULL), or every submap empty: O3S_OK and a result of size 0 (Mapper.cpp:509-512).
 *
 * Bad arguments.  Everything is checked before the first launch, and on O3S_ERR_BAD_ARGUMENT the object keeps its previous
 * result: a NULL object, n < 0, maps == NULL with n > 0, a NULL or repeated submap pointer, a submap on a device other than
 * the object's, more than 2^31 - 1 points in total, and — found from the bounds of the input, before any key is formed — a voxel
 * index range that does not fit 31 bits per axis or whose product does not pack into 63 bits (the rule of the other voxelisers).
 * A failure of the runtime (O3S_ERR_HIP) once the result arrays are being rewritten leaves a result of size 0.
 *
 * Streams.  The call creates no stream.  Each distinct stream of the submaps is drained once (as in o3s_submaps_transform),
 * everything is enqueued on maps[0]'s stream, and the call returns when the result is complete.
 *
 * Threading.  The rule of o3s_submap_clone: call it from the thread that inserts into the submaps, or pass clones. */
int o3s_assembled_map_build(o3s_assembled_map* a, int32_t n, o3s_submap* const* maps, double voxel_size, int32_t attrs,
                            int64_t* n_out);
int64_t o3s_assembled_map_size(const o3s_assembled_map* a);
int o3s_assembled_map_has_normals(const o3s_assembled_map* a);
int o3s_assembled_map_has_colors(const o3s_assembled_map* a);
/* Copies the result to the host: 3 x size doubles each; normals / colors nullable.  Asking for an attribute the result does not
 * carry is O3S_ERR_BAD_SHAPE (nothing is copied). */
int o3s_assembled_map_download(const o3s_assembled_map* a, double* pts, double* normals, double* colors);
/* Replaces dst's map cloud with the result without leaving HBM: what o3s_submap_upload does with a host cloud, except that
 * colours are kept when the result has them.  dst's voxel layout becomes invalid (its next insert sorts) and its feature set is
 * dropped; a pending insert of dst is completed first.  dst must live on the object's device (O3S_ERR_BAD_ARGUMENT otherwise).
 * dst MAY be one of the submaps of the last build — the result is a copy, no longer tied to them; the only rule is that of every
 * call that rewrites a submap: nothing else may read dst concurrently.  This is what lets the whole map become an ICP reference
 * (o3s_submap_set_reference) or get features (o3s_submap_compute_features) without a round trip. */
int o3s_assembled_map_to_submap(const o3s_assembled_map* a, o3s_submap* dst);
/* device memory the object holds: result arrays, work area, segment table */
int64_t o3s_assembled_map_device_bytes(const o3s_assembled_map* a);

#ifdef __cplusplus
}
#endif
#endif /* O3S_ASSEMBLED_MAP_H */
