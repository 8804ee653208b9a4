/*
 * o3s_pose_search.h — C ABI of the initial pose search in a resident map (same shared library, libo3dslam_icp_hip.so): the
 * device counterpart of the manual alignment of SlamMapInitializer (ros/open3d_slam_ros/src/SlamMapInitializer.cpp:50-130),
 * where a person drags an interactive marker until the scan lies on the loaded map.  Here a grid of candidate poses around a
 * prior is scored against the occupancy snapshot of the submap (o3s_submap_build_voxel_map) in one device call and the best
 * local maxima come back; refining and accepting one of them is host policy over the existing entries (pose_search.py,
 * cpp/o3s_pose_search.hpp).
 *
 * Pose grid.  Axis a in {x, y, z} has 2 n_a + 1 cells, cell i at offset (i - n_a) * step; the yaw axis has n_yaw cells,
 * psi_l = yaw0 + l * step_yaw.  Pose index p = ((l * (2 n_z + 1) + k) * (2 n_y + 1) + j) * (2 n_x + 1) + i: x runs fastest.
 * Pose of index p — fp64, no FMA, in this order: c = cos(psi_l), s = sin(psi_l) (libm, on the host); R = Rz(psi_l) R_c element
 * by element: row 0 = (c * Rc0) - (s * Rc1), row 1 = (s * Rc0) + (c * Rc1), row 2 = Rc2 — a yaw about the MAP's z axis, roll and
 * pitch are the prior's; t = (t_c.x + (double)(i - n_x) * step_xy, t_c.y + (double)(j - n_y) * step_xy,
 * t_c.z + (double)(k - n_z) * step_z).  o3s_pose_search_pose returns exactly that matrix.
 *
 * Score of pose p: the integer n_overlapping that o3s_submap_overlap_fitness(m, pts, N, T_p, ...) returns for the scan points
 * i with i % point_stride == 0 — the contract written down at that function in o3s_submap.h (isometry product, voxel key,
 * lookup; a point whose key does not pack, or is not a number, counts as not overlapping and is no error).
 *
 * Selection.  Pose p is a local maximum when no neighbour q beats it: the neighbours are the index offsets in {-1, 0, 1}^4
 * without 0, inside the grid — the yaw axis wraps when yaw_ring is set and n_yaw >= 3 —, and q beats p when
 * score[q] > score[p], or score[q] == score[p] and q < p (a plateau keeps its lowest index).  Eligible: score >= min_score, and
 * a local maximum when local_maxima is set.  The result is the first top_k eligible poses ordered by (score descending, index
 * ascending).  All of it is integer work on the device; the result does not depend on any run-time order.
 *
 * (The header lives in a directory of its own, like include/place_recognition/.)  Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_POSE_SEARCH_H
#define O3S_POSE_SEARCH_H

#include <stdint.h>

#include "../o3s_submap.h"

#ifdef __cplusplus
extern "C" {
#endif

#define O3S_POSE_SEARCH_MAX_TOP_K 64
#define O3S_POSE_SEARCH_MAX_HALF_WIDTH 4096 /* n_x, n_y, n_z: 0 .. this */
#define O3S_POSE_SEARCH_MAX_YAWS 65536      /* n_yaw: 1 .. this */

typedef struct o3s_pose_search_params {
  double  center[16];   /* prior T_map_sensor, column-major; only the rotation block R_c and translation t_c are read */
  double  step_xy, step_z, step_yaw;   /* m, m, rad */
  double  yaw0;         /* rad */
  int32_t n_x, n_y, n_z;/* half widths: the axis has 2 n + 1 cells, offset (i - n) * step, i = 0 .. 2 n */
  int32_t n_yaw;        /* number of yaws >= 1: psi_l = yaw0 + l * step_yaw, l = 0 .. n_yaw - 1 */
  int32_t yaw_ring;     /* 1: the yaw axis closes on itself (neighbours wrap) for the local-maximum rule */
  int32_t point_stride; /* >= 1: only scan points i with i % point_stride == 0 are counted */
  int32_t local_maxima; /* 1: select among local maxima only; 0: among all poses */
  int32_t top_k;        /* 1 .. 64 */
  int64_t min_score;    /* poses with a smaller score are never selected */
} o3s_pose_search_params;

typedef struct o3s_pose_search_result {
  int64_t n_poses;          /* P */
  int32_t n_found;          /* winners: 0 .. top_k */
  int32_t reserved;
  int64_t index[64];        /* pose indices of the winners, best first; entries from n_found on are -1 */
  int64_t score[64];        /* their scores; entries from n_found on are 0 */
  int64_t n_points_counted; /* ceil(N / point_stride) */
  float   gpu_ms;           /* device time of the call (wall_clock64 stamps of its first and last kernel) */
  int32_t reserved2;
} o3s_pose_search_result;

/* identity centre, steps 0.5 m / 0.5 m / 5 degrees, yaw0 0, n 8 / 8 / 0, 72 yaws as a ring, stride 1, local maxima, top_k 8,
 * min_score 1 */
void o3s_pose_search_default_params(o3s_pose_search_params* p);
/* P = (2 n_x + 1)(2 n_y + 1)(2 n_z + 1) n_yaw, or -1 for parameters the search refuses (below).  No device. */
int64_t o3s_pose_search_count(const o3s_pose_search_params* p);
/* T_out (column-major) = the pose of `index` as defined above.  O3S_ERR_BAD_ARGUMENT: NULL, refused parameters, or an index
 * outside 0 .. P - 1.  No device. */
int o3s_pose_search_pose(const o3s_pose_search_params* p, int64_t index, double T_out[16]);

/* Scores every pose of the grid against m's snapshot and selects.  pts: 3 x N host doubles in the sensor frame.
 * scores_out (nullable): P words, the score of every pose — the only other thing that crosses the bus is the result.
 * Refusals, all decided before any device work, outputs untouched —
 *   O3S_ERR_BAD_ARGUMENT: a NULL argument (pts may be NULL when N == 0); N < 0; a center, yaw0 or step that is not finite; a
 *     step <= 0 on an axis with more than one cell; n_x, n_y, n_z outside 0 .. O3S_POSE_SEARCH_MAX_HALF_WIDTH, n_yaw outside
 *     1 .. O3S_POSE_SEARCH_MAX_YAWS, point_stride < 1, top_k outside 1 .. 64, yaw_ring or local_maxima other than 0 / 1;
 *     P > 2^26, N > 2^20, or P * ceil(N / point_stride) > 2^34 (a guard that keeps one call short, not a performance claim);
 *     for the _scan form: `which` other than 0 / 1, or a scan on another device than the submap;
 *   O3S_ERR_NOT_INITIALIZED: the submap has no snapshot.
 * N == 0 is O3S_OK with every score 0.  The call blocks, runs on the submap's stream and leaves the submap, its snapshot and the
 * scan as they were; like the overlap count it may run from several threads against one snapshot (each call works in an area
 * of its own). */
int o3s_submap_pose_search(const o3s_submap* m, const double* pts, int64_t N, const o3s_pose_search_params* p,
                           o3s_pose_search_result* result, uint32_t* scores_out);
/* The same over a RESIDENT pre-processed scan of the same device (o3s_scan.h); which: 0 = merge cloud, 1 = match cloud. */
struct o3s_scan;
int o3s_submap_pose_search_scan(const o3s_submap* m, const struct o3s_scan* scan, int which,
                                const o3s_pose_search_params* p, o3s_pose_search_result* result, uint32_t* scores_out);

#ifdef __cplusplus
}
#endif
#endif /* O3S_POSE_SEARCH_H */
