"""The back end of a loop closure: the pose-graph solver of the library (include/pose_graph/o3s_pose_graph.h — Open3D's
GlobalOptimization with Levenberg-Marquardt, host arithmetic, no device) and the reference's bookkeeping around it —
o3d_slam::Constraint (Constraint.hpp), OptimizationProblem (OptimizationProblem.cpp:25-121, 151-210) and
SlamWrapper::updateSubmapsAndTrajectory (SlamWrapper.cpp:1105-1140).  Python mirror of cpp/o3s_pose_graph.hpp: the same logic,
the compiled header is checked against it."""
from __future__ import annotations

import copy
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .mapper import inv_iso, mul4


class PoseGraphEdgeC(C.Structure):
    """o3s_pose_graph_edge"""
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("uncertain", C.c_int32), ("transformation", C.c_double * 16),
                ("information", C.c_double * 36), ("confidence", C.c_double)]


class OptionC(C.Structure):
    """o3s_global_optimization_option"""
    _fields_ = [("max_correspondence_distance", C.c_double), ("edge_prune_threshold", C.c_double), ("preference_loop_closure", C.c_double),
                ("reference_node", C.c_int32)]


class CriteriaC(C.Structure):
    """o3s_global_optimization_criteria"""
    _fields_ = [("max_iteration", C.c_int32), ("max_iteration_lm", C.c_int32), ("min_relative_increment", C.c_double),
                ("min_relative_residual_increment", C.c_double), ("min_right_term", C.c_double), ("min_residual", C.c_double),
                ("upper_scale_factor", C.c_double), ("lower_scale_factor", C.c_double)]


class PassC(C.Structure):
    """o3s_global_optimization_pass"""
    _fields_ = [("iterations", C.c_int32), ("lm_trials", C.c_int32), ("accepted", C.c_int32), ("stop_rule", C.c_int32), ("n_edges", C.c_int32),
                ("reserved", C.c_int32), ("residual_before", C.c_double), ("residual_after", C.c_double), ("line_process_weight", C.c_double)]


class StatsC(C.Structure):
    """o3s_global_optimization_stats"""
    _fields_ = [("passes", PassC * 2)]


STOP_NONE, STOP_RIGHT_TERM, STOP_INCREMENT, STOP_RESIDUAL_INCREMENT, STOP_RESIDUAL, STOP_MAX_ITERATION, STOP_MAX_ITERATION_LM = range(7)


def _L():
    L = _lib.lib()
    if _lib.needs_binding(L, __name__):
        dp, ep = C.POINTER(C.c_double), C.POINTER(PoseGraphEdgeC)
        L.o3s_global_optimization_defaults.argtypes = [C.POINTER(CriteriaC), C.POINTER(OptionC)]
        L.o3s_global_optimization_defaults.restype = None
        L.o3s_global_optimization.argtypes = [C.c_int32, dp, C.c_int32, ep, C.POINTER(C.c_int32), C.POINTER(CriteriaC), C.POINTER(OptionC),
                                              C.POINTER(StatsC)]
        L.o3s_pose_graph_linearize.argtypes = [C.c_int32, dp, C.c_int32, ep, C.POINTER(OptionC), dp, dp, dp, dp, dp, dp, dp]
    return L


def _d(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


@dataclass
class PoseGraphEdge:
    """registration::PoseGraphEdge.  transformation: 4x4, information: 6x6 (rotation x, y, z, then translation)."""
    source: int
    target: int
    transformation: np.ndarray = field(default_factory=lambda: np.eye(4))
    information: np.ndarray = field(default_factory=lambda: np.eye(6))
    uncertain: bool = False
    confidence: float = 1.0


@dataclass
class PoseGraph:
    """registration::PoseGraph: nodes are 4x4 poses."""
    nodes: list = field(default_factory=list)
    edges: list = field(default_factory=list)


def default_criteria() -> CriteriaC:
    c = CriteriaC()
    _L().o3s_global_optimization_defaults(C.byref(c), None)
    return c


def default_option() -> OptionC:
    o = OptionC()
    _L().o3s_global_optimization_defaults(None, C.byref(o))
    return o


def _pack(graph: PoseGraph):
    n = len(graph.nodes)
    poses = np.zeros((max(n, 1), 16))
    for i, T in enumerate(graph.nodes):
        poses[i] = np.asarray(T, np.float64).T.reshape(16)   # column-major
    edges = (PoseGraphEdgeC * max(len(graph.edges), 1))()
    for k, e in enumerate(graph.edges):
        edges[k].source, edges[k].target, edges[k].uncertain = int(e.source), int(e.target), int(bool(e.uncertain))
        edges[k].transformation[:] = list(np.asarray(e.transformation, np.float64).T.reshape(16))
        edges[k].information[:] = list(np.asarray(e.information, np.float64).T.reshape(36))
        edges[k].confidence = float(e.confidence)
    return poses, edges


def _unpack_edge(e: PoseGraphEdgeC) -> PoseGraphEdge:
    return PoseGraphEdge(int(e.source), int(e.target), np.array(e.transformation[:]).reshape(4, 4).T.copy(),
                         np.array(e.information[:]).reshape(6, 6).T.copy(), bool(e.uncertain), float(e.confidence))


def global_optimization(graph: PoseGraph, criteria: CriteriaC = None, option: OptionC = None):
    """GlobalOptimization(pose_graph, GlobalOptimizationLevenbergMarquardt(), criteria, option) on a copy: returns
    (optimised PoseGraph — the pruned edges gone, the survivors in their order —, StatsC).  Raises ValueError on a graph the library
    refuses (no node, an edge id out of range, a certain edge whose confidence is not 1)."""
    L = _L()
    cr = default_criteria() if criteria is None else criteria
    op = default_option() if option is None else option
    poses, edges = _pack(graph)
    n_out, st = C.c_int32(0), StatsC()
    rc = L.o3s_global_optimization(len(graph.nodes), _d(poses), len(graph.edges), edges, C.byref(n_out), C.byref(cr), C.byref(op), C.byref(st))
    if rc == _lib.ERR_BAD_ARGUMENT:
        raise ValueError("o3s_global_optimization refused the graph")
    if rc != _lib.OK:
        raise RuntimeError(f"o3s_global_optimization failed with o3s_status {rc}")
    out = PoseGraph([poses[i].reshape(4, 4).T.copy() for i in range(len(graph.nodes))], [_unpack_edge(edges[k]) for k in range(n_out.value)])
    return out, st


def linearize(graph: PoseGraph, option: OptionC = None):
    """The solver's own linearisation at the graph's poses and confidences (o3s_pose_graph_linearize): dict with e (E x 6), Js, Jt
    (E x 6 x 6), H (6n x 6n), b (6n), objective, line_process_weight."""
    L = _L()
    op = default_option() if option is None else option
    poses, edges = _pack(graph)
    n, E = len(graph.nodes), len(graph.edges)
    e, Js, Jt = np.zeros((max(E, 1), 6)), np.zeros((max(E, 1), 36)), np.zeros((max(E, 1), 36))
    H, b, F, w = np.zeros((6 * n, 6 * n)), np.zeros(6 * n), C.c_double(0), C.c_double(0)
    rc = L.o3s_pose_graph_linearize(n, _d(poses), E, edges, C.byref(op), _d(e), _d(Js), _d(Jt), _d(H), _d(b),
                                    C.cast(C.byref(F), C.POINTER(C.c_double)), C.cast(C.byref(w), C.POINTER(C.c_double)))
    if rc != _lib.OK:
        raise ValueError(f"o3s_pose_graph_linearize failed with o3s_status {rc}")
    return dict(e=e[:E], Js=Js[:E].reshape(E, 6, 6).transpose(0, 2, 1).copy(), Jt=Jt[:E].reshape(E, 6, 6).transpose(0, 2, 1).copy(), H=H.T.copy(), b=b,
                objective=F.value, line_process_weight=w.value)


# ---- o3d_slam::Constraint, OptimizationProblem ------------------------------------------------------------------------

@dataclass
class Constraint:
    """o3d_slam::Constraint (Constraint.hpp:14-22).  registration.loop_closure_constraint and the odometry-constraint calls produce
    source_to_target and information_matrix; the ids and the time stamp are the caller's."""
    source_to_target: np.ndarray = field(default_factory=lambda: np.eye(4))
    source_submap_idx: int = 0
    target_submap_idx: int = 0
    information_matrix: np.ndarray = field(default_factory=lambda: np.eye(6))
    is_information_matrix_valid: bool = False
    is_odometry_constraint: bool = True
    timestamp: float = 0.0


@dataclass
class OptimizedTransform:
    """o3d_slam::OptimizedTransform"""
    dT: np.ndarray
    submap_id: int


@dataclass
class GlobalOptimizationParameters:
    """Parameters.hpp:142-146 (the parameter files set max_correspondence_distance = 1000.0)"""
    max_correspondence_distance: float = 10.0
    loop_closure_preference: float = 2.0
    edge_prune_threshold: float = 0.2
    reference_node: int = 0


class OptimizationProblem:
    """OptimizationProblem.cpp:46-121, 151-210 line by line; solve() (:25-44) is the library's o3s_global_optimization."""

    def __init__(self, params: GlobalOptimizationParameters = None):
        self.params = params or GlobalOptimizationParameters()
        self.pose_graph, self.pose_graph_optimized, self.pose_graph_non_optimized = PoseGraph(), PoseGraph(), PoseGraph()
        self.odometry_constraints, self.loop_closure_constraints = [], []
        self.num_odometry_edges_prev = 0
        self.num_loop_closures_prev = 0
        self.last_stats = None

    # :151-189
    def clear_odometry_constraints(self):
        self.odometry_constraints = []

    def clear_loop_closure_constraints(self):
        self.loop_closure_constraints = []

    def add_odometry_constraint(self, c: Constraint):
        self.odometry_constraints.append(c)

    def add_loop_closure_constraint(self, c: Constraint):
        self.loop_closure_constraints.append(c)

    def insert_odometry_constraints(self, cs):
        self.odometry_constraints.extend(cs)

    def insert_loop_closure_constraints(self, cs):
        """:177-189: a constraint between a (source, target) pair that is already there is dropped"""
        for c in cs:
            if not any(c.source_submap_idx == c2.source_submap_idx and c.target_submap_idx == c2.target_submap_idx
                       for c2 in self.loop_closure_constraints):
                self.loop_closure_constraints.append(c)

    # :50-121
    def build_optimization_problem(self):
        self.pose_graph.edges = []          # :56 only the edges: the nodes stay and are extended
        self._setup_odometry_edges_and_pose_graph_nodes()
        self._setup_loop_closure_edges()

    def _setup_odometry_edges_and_pose_graph_nodes(self):
        # :66-67 sorts with a comparator that sets a source against a target (not a strict weak order); here: stable, by source
        self.odometry_constraints.sort(key=lambda c: c.source_submap_idx)
        for c in self.odometry_constraints:
            if not c.target_submap_idx > c.source_submap_idx:
                raise AssertionError("id_source should always be less than id_target for the odometry constraints")
            self.pose_graph.edges.append(PoseGraphEdge(c.source_submap_idx, c.target_submap_idx, np.array(c.source_to_target, np.float64),
                                                       np.array(c.information_matrix, np.float64), False, 1.0))
        n_existing_edges = len(self.pose_graph_optimized.edges)
        if n_existing_edges > 0:
            odometry = inv_iso(self.pose_graph_optimized.nodes[-1])      # :87
        else:
            self.pose_graph.nodes.append(np.eye(4))                        # :89 (again on every build until a solve has left edges)
            odometry = np.eye(4)
        for i in range(self.num_odometry_edges_prev, len(self.odometry_constraints)):
            odometry = mul4(np.asarray(self.odometry_constraints[i].source_to_target, np.float64), odometry)
            self.pose_graph.nodes.append(inv_iso(odometry))
        self.num_odometry_edges_prev = len(self.odometry_constraints)

    def _setup_loop_closure_edges(self):
        self.num_loop_closures_prev = len(self.loop_closure_constraints)
        for c in self.loop_closure_constraints:
            if not c.is_information_matrix_valid:
                raise AssertionError(f"Invalid information matrix between: {c.source_submap_idx} and {c.target_submap_idx}")
            if not c.source_submap_idx > c.target_submap_idx:
                raise AssertionError("Optimization problem, loop closure constraints: source should be greater than target")
            self.pose_graph.edges.append(PoseGraphEdge(c.source_submap_idx, c.target_submap_idx, np.array(c.source_to_target, np.float64),
                                                       np.array(c.information_matrix, np.float64), True, 1.0))

    # :25-44
    def solve(self):
        p = self.params
        option = OptionC(float(p.max_correspondence_distance), float(p.edge_prune_threshold), float(p.loop_closure_preference), int(p.reference_node))
        self.pose_graph_non_optimized = copy.deepcopy(self.pose_graph)
        self.pose_graph, self.last_stats = global_optimization(self.pose_graph, default_criteria(), option)
        self.pose_graph_optimized = copy.deepcopy(self.pose_graph)

    # :191-202
    def get_optimized_transform_increments(self):
        if len(self.pose_graph_optimized.nodes) != len(self.pose_graph.nodes):
            raise AssertionError("Graphs are not of same size, did you run the optimization?")
        # :197 `deltaT = tNew`: the increment IS the optimised node pose (the old pose is read and not used)
        return [OptimizedTransform(self.pose_graph_optimized.nodes[i].copy(), i) for i in range(len(self.pose_graph.nodes))]

    def get_loop_closure_constraints(self):
        return self.loop_closure_constraints

    def update_loop_closure_constraint(self, idx: int, c: Constraint):
        self.loop_closure_constraints[idx] = c       # .at(idx): IndexError out of range


def update_submaps_and_trajectory(problem: OptimizationProblem, collection, mapper, last_constraints):
    """SlamWrapper::updateSubmapsAndTrajectory (SlamWrapper.cpp:1105-1140): the collection is transformed by the optimised
    increments, the mapper's poses by the increment of the latest loop-closure constraint's source, every loop-closure constraint's
    transform is reset to identity, and the constraints' submaps become adjacent.  Returns the increments."""
    increments = problem.get_optimized_transform_increments()
    collection.transform(increments)
    latest = last_constraints[0]                     # std::max_element: the first of the largest time stamps
    for c in last_constraints[1:]:
        if latest.timestamp < c.timestamp:
            latest = c
    if not latest.source_submap_idx > latest.target_submap_idx:
        raise AssertionError("update submaps and trajectory: the source of a loop closure is the later submap")
    dT = increments[latest.source_submap_idx]        # .at(): positional
    mapper.loopClosureUpdate(dT.dT)
    cs = list(problem.get_loop_closure_constraints())
    for i, old in enumerate(cs):
        c = copy.copy(old)
        c.source_to_target = np.eye(4)
        problem.update_loop_closure_constraint(i, c)
        cs[i] = c
    collection.update_adjacency_matrix(cs)
    return increments


def loop_closure_step(collection, place_recognition, problem: OptimizationProblem, candidates, device_call=None, refine_call=None):
    """The body of SlamWrapper::loopClosureWorker (SlamWrapper.cpp:1068-1099), once: the loop-closure constraints of the candidates
    ((submap id, time stamp), SubmapCollection::buildLoopClosureConstraints :291-299); none: return [] and leave the problem alone;
    else a COPY of the collection's odometry constraints completed with the all-submaps overload of computeOdometryConstraints,
    the problem's odometry constraints cleared, both kinds inserted, the problem built and solved.  Returns the loop-closure
    constraints: what update_submaps_and_trajectory then takes as last_constraints."""
    from .constraint_builders import compute_odometry_constraints

    loop_closure_constraints = []
    for submap_id, stamp in candidates:
        loop_closure_constraints.extend(place_recognition.buildLoopClosureConstraints(
            collection.range_sensor_poses[collection.active], collection, int(submap_id), collection.active, stamp))
    if not loop_closure_constraints:
        return []
    odometry_constraints = list(collection.getOdometryConstraints())
    compute_odometry_constraints(collection, odometry_constraints, None, device_call or getattr(collection, "_odometry_call", None),
                                 refine_call or getattr(collection, "_refine_call", None))
    problem.clear_odometry_constraints()
    problem.insert_loop_closure_constraints(loop_closure_constraints)
    problem.insert_odometry_constraints(odometry_constraints)
    problem.build_optimization_problem()
    problem.solve()
    return loop_closure_constraints
