/*
 * o3s_pose_graph.h — C ABI of the pose-graph solver (same shared library, libo3dslam_icp_hip.so): what
 * OptimizationProblem::solve (O3S/src/OptimizationProblem.cpp:25-44) asks of Open3D —
 * open3d::pipelines::registration::GlobalOptimization with GlobalOptimizationLevenbergMarquardt: the line-process pose graph of
 * Choi, Zhou, Koltun, "Robust Reconstruction of Indoor Scenes" (CVPR 2015), minimised by Levenberg-Marquardt.
 * Host arithmetic: it opens no device and works on a machine without a GPU (o3s_motion_from_poses set the precedent).  The
 * contract — residual, Jacobians, linear system, update, line process, LM loop, pruning driver — is written out in DESIGN.md
 * section 9d; it was restated from the published method and Open3D's documented interface and could not be compared with
 * Open3D's source.  All arithmetic is fp64, edges are visited in index order, every sum is taken in a fixed order: results are
 * run-to-run identical.  6n x 6n dense LDLT: one node per submap, tens of them.
 *
 * (The header lives in a directory of its own: include/ itself holds the headers of the device-side ABI, one list.)
 * Conventions: poses / transformations are 4x4 doubles in column-major order, information matrices 6x6 column-major in
 * Open3D's order (rotation x, y, z, then translation).  Return: o3s_status (o3s_icp.h).
 */
#ifndef O3S_POSE_GRAPH_H
#define O3S_POSE_GRAPH_H

#include <stdint.h>

#include "../o3s_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* registration::PoseGraphEdge: transformation = X with X = pose_target^-1 pose_source when the edge is satisfied */
typedef struct o3s_pose_graph_edge {
  int32_t source, target, uncertain;
  double transformation[16];
  double information[36];
  double confidence; /* the line process l in [0, 1]; exactly 1.0 for an edge that is not uncertain */
} o3s_pose_graph_edge;

/* registration::GlobalOptimizationOption */
typedef struct o3s_global_optimization_option {
  double max_correspondence_distance; /* 0.075 */
  double edge_prune_threshold;        /* 0.25  */
  double preference_loop_closure;     /* 1.0   */
  int32_t reference_node;             /* -1: no compensation */
} o3s_global_optimization_option;

/* registration::GlobalOptimizationConvergenceCriteria */
typedef struct o3s_global_optimization_criteria {
  int32_t max_iteration;    /* 100 */
  int32_t max_iteration_lm; /* 20  */
  double min_relative_increment;          /* 1e-6 */
  double min_relative_residual_increment; /* 1e-6 */
  double min_right_term;                  /* 1e-6 */
  double min_residual;                    /* 1e-6 */
  double upper_scale_factor;              /* 2/3  */
  double lower_scale_factor;              /* 1/3  */
} o3s_global_optimization_criteria;

/* which rule ended a pass */
enum {
  O3S_PG_STOP_NONE = 0,
  O3S_PG_STOP_RIGHT_TERM = 1,         /* max(b) < min_right_term */
  O3S_PG_STOP_INCREMENT = 2,          /* |delta| < min_relative_increment (|x| + min_relative_increment) */
  O3S_PG_STOP_RESIDUAL_INCREMENT = 3, /* F - F_new < min_relative_residual_increment F */
  O3S_PG_STOP_RESIDUAL = 4,           /* F < min_residual */
  O3S_PG_STOP_MAX_ITERATION = 5,
  O3S_PG_STOP_MAX_ITERATION_LM = 6
};

typedef struct o3s_global_optimization_pass {
  int32_t iterations; /* outer iterations begun */
  int32_t lm_trials;  /* linear solves */
  int32_t accepted;   /* steps taken (rho > 0) */
  int32_t stop_rule;
  int32_t n_edges;
  int32_t reserved;
  double residual_before, residual_after; /* the objective F */
  double line_process_weight;
} o3s_global_optimization_pass;

/* pass[0]: the whole graph; pass[1]: the graph without the pruned edges */
typedef struct o3s_global_optimization_stats {
  o3s_global_optimization_pass pass[2];
} o3s_global_optimization_stats;

void o3s_global_optimization_defaults(o3s_global_optimization_criteria* criteria, o3s_global_optimization_option* option);

/* GlobalOptimization(pose_graph, GlobalOptimizationLevenbergMarquardt(), criteria, option).  poses: n_nodes x 16, in / out.
 * edges: in / out — the survivors of the pruning, with their confidences, are compacted to the front in their original order
 * and *n_edges_out (nullable) is their number.  stats: nullable.  n_nodes <= 0, an edge id out of range, an edge that is not
 * uncertain with confidence != 1.0 or a NULL argument: O3S_ERR_BAD_ARGUMENT, and nothing is changed. */
int o3s_global_optimization(int32_t n_nodes, double* poses, int32_t n_edges, o3s_pose_graph_edge* edges, int32_t* n_edges_out,
                            const o3s_global_optimization_criteria* criteria, const o3s_global_optimization_option* option,
                            o3s_global_optimization_stats* stats);

/* The solver's own linearisation at (poses, edge confidences), for checking a restatement step by step: per edge the residual e
 * (6), Js and Jt (6 x 6, column-major); the system H (6n x 6n, column-major) and b (6n) that an LM trial at this state solves;
 * the objective F and the line-process weight w under `option`.  Every output is nullable.  Same validation as above. */
int o3s_pose_graph_linearize(int32_t n_nodes, const double* poses, int32_t n_edges, const o3s_pose_graph_edge* edges,
                             const o3s_global_optimization_option* option, double* e, double* Js, double* Jt, double* H,
                             double* b, double* objective, double* line_process_weight);

#ifdef __cplusplus
}
#endif
#endif /* O3S_POSE_GRAPH_H */
