"""The loop-closure back end on the CPU: the pose-graph solver of the library (include/pose_graph/o3s_pose_graph.h; host
arithmetic, no device is opened), the reference's bookkeeping around it (pose_graph.py, cpp/o3s_pose_graph.hpp) and
SubmapCollection.transform with stand-in submaps.  The yardsticks are the numpy restatement of the contract
(tests/pose_graph_ref.py) and scipy's minimiser, never the library's own earlier output.

Tolerances (measured with the graphs below, 10 x margin):
  two-node graph, |pose_t^-1 pose_s - X|   measured 3.5e-7 (the pass stops on F < min_residual = 1e-6)    bound 3.5e-6
  reference node kept                       measured 5.6e-16 (one product with the compensation)         bound 5.6e-15
  objective above scipy's optimum, ring     measured 7.7e-11 relative                                     bound 7.7e-10
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_graph_ref as ref
from open3d_slam_advanced_rss_2024_public_amd import _lib
from open3d_slam_advanced_rss_2024_public_amd import pose_graph as pg
from open3d_slam_advanced_rss_2024_public_amd.mapper import Mapper
from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection
from test_submap_collection_logic import FakeScan, FakeSubmap, drive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MCD = 0.5            # max_correspondence_distance of the ring tests: w = 1.0 * 0.25 * 400 = 100
GAP = 7.7e-10        # relative objective gap to scipy's optimum (see above)


def ring_option(reference_node=0):
    op = pg.default_option()
    op.max_correspondence_distance, op.reference_node = MCD, reference_node
    return op


@pytest.fixture(scope="module")
def ring():
    """The eight-node ring of tests 2 - 4 and its optimum by scipy (computed once, left unchanged)."""
    g, truth = ref.ring_graph(pg.PoseGraph, pg.PoseGraphEdge)
    w = ref.line_process_weight(g.edges, MCD, 1.0)
    nodes_opt, F_opt = ref.least_squares_optimum(g.nodes, g.edges, w, fixed=0)
    return dict(graph=g, truth=truth, w=w, nodes_opt=nodes_opt, F_opt=F_opt)


def test_the_solvers_header_is_plain_c(tmp_path):
    """include/pose_graph/o3s_pose_graph.h under the check tests/test_abi.py applies to the headers of include/: C99, pedantic."""
    src = tmp_path / "c_abi.c"
    src.write_text('#include "pose_graph/o3s_pose_graph.h"\n'
                   "int main(void) { o3s_global_optimization_criteria c; o3s_global_optimization_option o;"
                   " o3s_global_optimization_defaults(&c, &o); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "c_abi.o")])


def test_the_library_exports_the_solver_and_the_transform_on_both_builds():
    _lib.build()
    for L in (_lib.lib(), _lib.load("hooks")):
        for name in ("o3s_global_optimization", "o3s_global_optimization_defaults", "o3s_pose_graph_linearize", "o3s_submap_transform",
                     "o3s_submaps_transform"):
            assert hasattr(L, name), name


# ---- 1. known answers ----------------------------------------------------------------------------------------------------

def test_defaults_are_open3ds():
    c, o = pg.default_criteria(), pg.default_option()
    assert (c.max_iteration, c.max_iteration_lm) == (100, 20)
    assert (c.min_relative_increment, c.min_relative_residual_increment, c.min_right_term, c.min_residual) == (1e-6, 1e-6, 1e-6, 1e-6)
    assert (c.upper_scale_factor, c.lower_scale_factor) == (2.0 / 3.0, 1.0 / 3.0)
    assert (o.max_correspondence_distance, o.edge_prune_threshold, o.preference_loop_closure, o.reference_node) == (0.075, 0.25, 1.0, -1)


def test_a_consistent_graph_is_returned_unchanged_on_the_right_term_rule():
    g, _ = ref.ring_graph(pg.PoseGraph, pg.PoseGraphEdge)
    for e in g.edges:
        e.transformation = np.linalg.inv(g.nodes[e.target]) @ g.nodes[e.source]
    out, st = pg.global_optimization(g, None, pg.default_option())
    assert all(np.array_equal(a, b) for a, b in zip(out.nodes, g.nodes))
    assert len(out.edges) == len(g.edges)
    for p in st.passes:
        assert (p.stop_rule, p.iterations, p.lm_trials, p.accepted) == (pg.STOP_RIGHT_TERM, 0, 0, 0)


@pytest.mark.parametrize("reference_node", [0, 1])
def test_two_nodes_one_edge(reference_node):
    X = ref.exp6(np.array([0.1, -0.2, 0.3, 1.0, 2.0, -0.5]))
    A = ref.exp6(np.array([0.3, 0.1, -0.4, 3.0, -1.0, 0.7]))
    B = ref.exp6(np.array([0.05, 0.02, -0.03, 0.2, -0.1, 0.1])) @ A @ np.linalg.inv(X)       # the target node, perturbed
    g = pg.PoseGraph([A.copy(), B.copy()], [pg.PoseGraphEdge(0, 1, X, np.eye(6) * 100.0, False, 1.0)])
    op = pg.default_option()
    op.reference_node = reference_node
    out, st = pg.global_optimization(g, None, op)
    err = np.abs(np.linalg.inv(out.nodes[1]) @ out.nodes[0] - X).max()
    kept = np.abs(out.nodes[reference_node] - g.nodes[reference_node]).max()
    print(f"two nodes: |Tt^-1 Ts - X| = {err:.3e}, reference node moved by {kept:.3e}")
    assert err < 3.5e-6
    assert kept < 5.6e-15
    assert st.passes[0].accepted >= 1 and st.passes[0].residual_after < st.passes[0].residual_before


# ---- 2. against an independent minimiser -----------------------------------------------------------------------------------

def test_ring_reaches_scipys_optimum(ring):
    g = ring["graph"]
    out, st = pg.global_optimization(g, None, ring_option())
    assert len(out.edges) == len(g.edges)
    F_lib = ref.objective_eliminated(out.nodes, g.edges, ring["w"])
    gap = (F_lib - ring["F_opt"]) / ring["F_opt"]
    print(f"ring: library {F_lib:.12g}, scipy {ring['F_opt']:.12g}, relative gap {gap:.3e}; passes "
          f"{[(p.iterations, p.lm_trials, p.accepted, p.stop_rule) for p in st.passes]}")
    assert gap < GAP
    assert np.abs(out.nodes[0] - g.nodes[0]).max() < 5.6e-15          # the gauge: node 0 stays
    # every uncertain edge carries the closed-form line process of the returned poses' predecessor step: in (0, 1], near 1 here
    assert all(0.99 < e.confidence <= 1.0 for e in out.edges if e.uncertain)
    assert all(e.confidence == 1.0 for e in out.edges if not e.uncertain)


# ---- 3. pruning ------------------------------------------------------------------------------------------------------------

def test_a_false_closure_is_pruned(ring):
    """The ring plus one false closure 5 -> 1 (half of exp6(0.3, -0.2, 1.0, 4, -3, 1) off the truth).  Its closed-form l at the
    optimum of the ring without it is ~1e-5 < edge_prune_threshold = 0.25, every true closure's is > 0.999 (checked below with the
    numpy restatement).  Other false closures tried with this ring are pruned as well but end 1e-8 .. 5e-7 above scipy's optimum:
    the second pass then stops on the residual-increment rule at 1e-6; a full-size one (a metre-scale error at l = 1 in the first
    steps) can pull the ring into another basin where true closures are switched off — the line process is no global method."""
    g, truth = ref.ring_graph(pg.PoseGraph, pg.PoseGraphEdge)
    bad = ref.exp6(0.5 * np.array([0.3, -0.2, 1.0, 4.0, -3.0, 1.0]))
    g.edges.append(pg.PoseGraphEdge(5, 1, bad @ np.linalg.inv(truth[1]) @ truth[5], g.edges[0].information.copy(), True, 1.0))
    w = ref.line_process_weight(g.edges, MCD, 1.0)
    assert w == ring["w"]                                               # same information(5, 5) on every uncertain edge
    ls = [ref.closed_form_confidence(ring["nodes_opt"], e, w) for e in g.edges if e.uncertain]
    assert ls[-1] < 0.25 and all(l > 0.25 for l in ls[:-1]), ls
    out, st = pg.global_optimization(g, None, ring_option())
    assert len(out.edges) == len(g.edges) - 1
    assert [(e.source, e.target, e.uncertain) for e in out.edges] == [(e.source, e.target, e.uncertain) for e in g.edges[:-1]]
    assert all(np.array_equal(a.transformation, b.transformation) for a, b in zip(out.edges, g.edges[:-1]))
    assert (st.passes[0].n_edges, st.passes[1].n_edges) == (len(g.edges), len(g.edges) - 1)
    F_lib = ref.objective_eliminated(out.nodes, ring["graph"].edges, ring["w"])
    gap = (F_lib - ring["F_opt"]) / ring["F_opt"]
    print(f"pruned ring: relative gap to the optimum without the false edge {gap:.3e}")
    assert gap < GAP


# ---- 4. the restatement, step by step ----------------------------------------------------------------------------------------

def test_first_step_linearisation_equals_the_restatement(ring):
    """e, Js, Jt, H, b of the first LM step (the linearisation at the initial poses and confidences, which every trial up to the
    first accepted one solves) against numpy, 1e-12 relative to the largest entry of each."""
    g = ring["graph"]
    lz = pg.linearize(g, ring_option())
    H, b = ref.linear_system(g.nodes, g.edges)

    def rel(a, r):
        return np.abs(a - r).max() / np.abs(r).max()

    # (the odometry edges of this ring are satisfied by its nodes — their e is rounding noise — so each quantity is compared over
    # all edges at once, relative to its largest entry)
    terms = [ref.edge_terms(g.nodes, ed) for ed in g.edges]
    for k, name in enumerate(["e", "Js", "Jt"]):
        assert rel(lz[name], np.stack([t[k] for t in terms])) < 1e-12, name
    assert rel(lz["H"], H) < 1e-12 and rel(lz["b"], b) < 1e-12
    assert np.array_equal(lz["H"], lz["H"].T) or rel(lz["H"], lz["H"].T) < 1e-15
    assert lz["line_process_weight"] == ref.line_process_weight(g.edges, MCD, 1.0)
    assert abs(lz["objective"] - ref.objective(g.nodes, g.edges, ring["w"])) < 1e-12 * lz["objective"]
    _, st = pg.global_optimization(g, None, ring_option())
    assert st.passes[0].residual_before == lz["objective"] and st.passes[0].accepted >= 1


# ---- 5. validation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["edge_id", "certain_confidence", "no_nodes"])
def test_bad_graphs_are_refused_and_left_alone(what, ring):
    g = ring["graph"]
    poses, edges = pg._pack(g)
    n_nodes = len(g.nodes)
    if what == "edge_id":
        edges[3].target = n_nodes
    elif what == "certain_confidence":
        edges[2].confidence = 0.5
    else:
        n_nodes = 0
    before_p, before_e = poses.copy(), bytes(edges)
    n_out, st = C.c_int32(-7), pg.StatsC()
    cr, op = pg.default_criteria(), ring_option()
    rc = pg._L().o3s_global_optimization(n_nodes, pg._d(poses), len(g.edges), edges, C.byref(n_out), C.byref(cr), C.byref(op), C.byref(st))
    assert rc == _lib.ERR_BAD_ARGUMENT
    assert np.array_equal(poses, before_p) and bytes(edges) == before_e and n_out.value == -7


# ---- 6. OptimizationProblem -----------------------------------------------------------------------------------------------

def _constraints():
    """A chain 0 -> 1 -> 2 -> 3 (odometry, handed over out of order) and a closure 3 -> 0."""
    rng = np.random.default_rng(11)
    info = np.diag([2.0, 2.0, 2.0, 1.0, 1.0, 1.0]) * 300.0 + 0.5
    steps = [ref.exp6(np.array([0.01 * k, -0.02, 0.4, 2.0 + k, 0.3, 0.05])) for k in range(4)]
    odom = [pg.Constraint(np.linalg.inv(steps[k]), k, k + 1, info.copy(), True, True, 1.0 + k) for k in range(3)]
    total = steps[0] @ steps[1] @ steps[2]                    # pose_0^-1 pose_3 along the odometry
    drifted = ref.exp6(np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.1, 3)])) @ total
    loop = pg.Constraint(drifted, 3, 0, info.copy(), True, False, 9.0)
    extra = pg.Constraint(np.linalg.inv(steps[3]), 3, 4, info.copy(), True, True, 5.0)
    return odom, loop, extra


def test_optimization_problem_bookkeeping():
    odom, loop, extra = _constraints()
    pr = pg.OptimizationProblem()
    assert (pr.params.max_correspondence_distance, pr.params.loop_closure_preference, pr.params.edge_prune_threshold, pr.params.reference_node) == \
        (10.0, 2.0, 0.2, 0)
    pr.insert_odometry_constraints([odom[2], odom[0], odom[1]])
    dup = pg.Constraint(np.eye(4), 3, 0, np.eye(6), True, False, 10.0)
    pr.insert_loop_closure_constraints([loop, dup])
    pr.insert_loop_closure_constraints([dup])
    assert len(pr.loop_closure_constraints) == 1 and pr.loop_closure_constraints[0] is loop          # dedup on (source, target)
    pr.build_optimization_problem()
    assert [(e.source, e.target, e.uncertain, e.confidence) for e in pr.pose_graph.edges] == \
        [(0, 1, False, 1.0), (1, 2, False, 1.0), (2, 3, False, 1.0), (3, 0, True, 1.0)]              # sorted by source; flags
    assert len(pr.pose_graph.nodes) == 4 and np.array_equal(pr.pose_graph.nodes[0], np.eye(4))
    chain = np.eye(4)
    for k in range(3):                                                                                # node k + 1 = (X_k ... X_0)^-1
        chain = odom[k].source_to_target @ chain
        assert np.allclose(pr.pose_graph.nodes[k + 1], np.linalg.inv(chain), atol=1e-12)
    with pytest.raises(AssertionError):
        pr.get_optimized_transform_increments()                                                       # "did you run the optimization?"
    pr.solve()
    inc = pr.get_optimized_transform_increments()
    assert [u.submap_id for u in inc] == [0, 1, 2, 3]
    assert all(np.array_equal(u.dT, T) for u, T in zip(inc, pr.pose_graph_optimized.nodes))          # the increment IS the node pose
    assert np.abs(inc[0].dT - np.eye(4)).max() < 5.6e-15                                             # reference node 0
    # second round, as SlamWrapper::loopClosureWorker drives it: the odometry list is cleared and handed over whole again
    last = pr.pose_graph_optimized.nodes[-1].copy()
    pr.clear_odometry_constraints()
    pr.insert_odometry_constraints(odom + [extra])
    pr.build_optimization_problem()
    assert len(pr.pose_graph.nodes) == 5 and len(pr.pose_graph.edges) == 5
    assert all(np.array_equal(a, b) for a, b in zip(pr.pose_graph.nodes[:4], pr.pose_graph_optimized.nodes))   # the nodes stayed
    assert np.allclose(pr.pose_graph.nodes[4], np.linalg.inv(extra.source_to_target @ np.linalg.inv(last)), atol=1e-12)   # chained from the last OPTIMISED node


def test_optimization_problem_asserts():
    odom, loop, _ = _constraints()
    pr = pg.OptimizationProblem()
    pr.add_odometry_constraint(pg.Constraint(np.eye(4), 2, 1, np.eye(6), True, True, 0.0))
    with pytest.raises(AssertionError):
        pr.build_optimization_problem()                       # odometry: source < target
    pr = pg.OptimizationProblem()
    pr.insert_odometry_constraints(odom)
    pr.add_loop_closure_constraint(pg.Constraint(np.eye(4), 0, 3, np.eye(6), True, False, 0.0))
    with pytest.raises(AssertionError):
        pr.build_optimization_problem()                       # loop closure: source > target
    pr = pg.OptimizationProblem()
    pr.insert_odometry_constraints(odom)
    pr.add_loop_closure_constraint(pg.Constraint(np.eye(4), 3, 0, np.eye(6), False, False, 0.0))
    with pytest.raises(AssertionError):
        pr.build_optimization_problem()                       # invalid information matrix


# ---- 7. SubmapCollection.transform ---------------------------------------------------------------------------------------

class Increment:
    def __init__(self, dT, submap_id):
        self.dT, self.submap_id = dT, submap_id


def _collection():
    calls = []
    col = SubmapCollection(10.0, 1, 10 ** 9, 2, 0.1, ("MaxRadius", 30.0), submap_factory=FakeSubmap, scan_factory=FakeScan,
                           transform_maps=lambda maps, Ts: calls.append((list(maps), [np.array(T) for T in Ts])))
    drive(col, [0, 12, 24, 24, 12], [0, 0, 0, 12, 12])       # five submaps, parents 0 0 1 2 3 (the logic test's loop)
    drive(col, [13], [12])                                     # one more scan into the active submap: the overlap buffer holds it
    assert len(col.maps) == 5 and col.parents == [0, 0, 1, 2, 3] and len(col.buffer) == 1
    return col, calls


def _T(k):
    return ref.exp6(np.array([0.01 * k, 0.02, -0.03 * k, 1.0 + k, -2.0, 0.5 * k]))


def test_collection_transform_parent_walk_and_positional_lookup():
    col, calls = _collection()
    centers = [None if c is None else c.copy() for c in col.centers]
    poses = [T.copy() for T in col.range_sensor_poses]
    assert len(col.buffer) > 0
    n_ring = len(col.buffer) + len(col.free)
    # increments name submaps 1 and 0, in that order: position 0 holds submap 1's, position 1 holds submap 0's
    inc = [Increment(_T(1), 1), Increment(_T(2), 0)]
    col.transform(inc)
    assert len(calls) == 1                                            # ONE batched device call
    maps, Ts = calls[0]
    # named ones first, in the increments' order; then 2, 3, 4: submap 2's parent is 1 (named) -> increments.at(1) = _T(2), the
    # POSITIONAL lookup; 3 walks 2 (revisited: unnamed) -> 1; 4 walks 3 -> 2 -> 1
    assert [col.maps.index(m) for m in maps] == [1, 0, 2, 3, 4]
    for T, k in zip(Ts, [1, 2, 2, 2, 2]):
        assert np.array_equal(T, _T(k))
    used = dict(zip([1, 0, 2, 3, 4], Ts))
    for i in range(5):
        assert np.array_equal(col.range_sensor_poses[i], np.asarray(pg.mul4(poses[i], used[i])))     # origin pose right-multiplied
        if centers[i] is None:
            assert col.centers[i] is None
        else:
            assert np.allclose(col.centers[i], (used[i] @ np.append(centers[i], 1.0))[:3], rtol=0, atol=1e-12)   # centre left-multiplied
            assert not np.array_equal(col.centers[i], centers[i])
    assert col.buffer == [] and len(col.free) == n_ring               # flushed: the scan objects are back in the ring


def test_collection_transform_empty_list_and_errors():
    col, calls = _collection()
    poses = [T.copy() for T in col.range_sensor_poses]
    n_buf = len(col.buffer)
    col.transform([])
    assert calls == [] and all(np.array_equal(a, b) for a, b in zip(col.range_sensor_poses, poses))
    assert col.buffer == [] and n_buf > 0                             # (:374 clears the buffer whatever the list holds)
    col, calls = _collection()
    with pytest.raises(IndexError):
        col.transform([Increment(_T(1), 0), Increment(_T(2), 3)])     # 4's parent 3 is named: increments.at(3) with two entries
    assert calls == []
    col, calls = _collection()
    col.transform([Increment(_T(1), 0), Increment(_T(2), 7)])         # an id beyond the collection is reported and skipped
    assert len(calls) == 1 and len(calls[0][0]) == 5 and all(np.array_equal(T, _T(1)) for T in calls[0][1])
    # submap 0 is its own parent and unnamed: the reference's "stuck in a loop"
    col, calls = _collection()
    with pytest.raises(RuntimeError, match="Stuck in a loop"):
        col.transform([Increment(_T(1), 2), Increment(_T(2), 3)])
    assert calls == []
    col, calls = _collection()
    with pytest.raises(ValueError):
        col.transform([Increment(_T(1), 0), Increment(_T(2), 0)])
    assert calls == []


def test_collection_transform_moves_the_dense_map_kept_for_a_submap():
    col, calls = _collection()

    class Dense:
        def __init__(self):
            self.Ts = []

        def transform(self, T):
            self.Ts.append(np.array(T))

    col.dense_maps[0] = d = Dense()
    col.transform([Increment(_T(1), 0), Increment(_T(2), 1)])
    assert len(d.Ts) == 1 and np.array_equal(d.Ts[0], _T(1))


# ---- 8. update_submaps_and_trajectory ------------------------------------------------------------------------------------

def test_update_submaps_and_trajectory():
    odom, loop, _ = _constraints()
    pr = pg.OptimizationProblem()
    pr.insert_odometry_constraints(odom)
    loop2 = pg.Constraint(np.linalg.inv(odom[1].source_to_target @ odom[0].source_to_target), 2, 0, loop.information_matrix.copy(), True, False, 4.0)
    pr.insert_loop_closure_constraints([loop, loop2])
    pr.build_optimization_problem()
    pr.solve()

    class Col:
        def __init__(self):
            self.log = []

        def transform(self, inc):
            self.log.append(("transform", [u.submap_id for u in inc]))

        def update_adjacency_matrix(self, cs):
            self.log.append(("adjacency", [(c.source_submap_idx, c.target_submap_idx) for c in cs]))

    col = Col()
    mapper = Mapper(None, None, None, None, 0.1, 1.0, 0.0)
    mapper.T, mapper.T_prev = _T(3), _T(4)
    # the latest constraint by time stamp is `loop` (9.0 > 4.0), whatever its place in the list: its source is submap 3
    inc = pg.update_submaps_and_trajectory(pr, col, mapper, [loop2, loop])
    assert col.log[0] == ("transform", [0, 1, 2, 3])
    assert np.array_equal(mapper.T, pg.mul4(inc[3].dT, _T(3))) and np.array_equal(mapper.T_prev, pg.mul4(inc[3].dT, _T(4)))   # left-multiplied
    assert all(np.array_equal(c.source_to_target, np.eye(4)) for c in pr.get_loop_closure_constraints())
    assert not np.array_equal(loop.source_to_target, np.eye(4))       # the caller's objects are copies' originals: untouched
    assert col.log[1] == ("adjacency", [(3, 0), (2, 0)])


# ---- 9. the compiled header ------------------------------------------------------------------------------------------------

def _hex(a):
    return " ".join(float(v).hex() for v in np.asarray(a, np.float64).T.reshape(-1))


def _mats(lines):
    return [np.array([float.fromhex(w) for w in ln.split()[-16:]]).reshape(4, 4).T for ln in lines]


def test_cpp_header_returns_pythons_bits(tmp_path):
    """cpp/o3s_pose_graph.hpp (and SubmapCollectionHip::transform, compiled with it) with plain g++ against the C ABI: the cases
    of tests 6 and 7 return the bits of the Python mirror."""
    _lib.build()
    pkg = os.path.join(ROOT, "open3d_slam_advanced_rss_2024_public_amd")
    exe = tmp_path / "pose_graph_cases"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "pose_graph_cases.cpp"), "-L" + pkg, "-lo3dslam_icp_hip", "-Wl,-rpath," + pkg, "-o", str(exe)])
    odom, loop, extra = _constraints()

    def cline(c, is_loop):
        head = f"loop {c.source_submap_idx} {c.target_submap_idx} {int(c.is_information_matrix_valid)}" if is_loop else \
            f"odom {c.source_submap_idx} {c.target_submap_idx}"
        return f"{head} {_hex(c.source_to_target)} {_hex(c.information_matrix)}"

    col, calls = _collection()
    inc = [Increment(_T(1), 1), Increment(_T(2), 0)]
    script = [cline(odom[2], False), cline(odom[0], False), cline(odom[1], False), cline(loop, True), cline(loop, True), "build", "nodes", "edges",
              "increments", "solve", "increments", "edges", "clear_odom"] + [cline(c, False) for c in odom + [extra]] + ["build", "nodes", "solve", "increments",
              "plan 5 " + " ".join(str(p) for p in col.parents) + " 2"] + [f"{u.submap_id} {_hex(u.dT)}" for u in inc] + \
             ["plan 5 0 0 1 2 3 2", f"2 {_hex(_T(1))}", f"3 {_hex(_T(2))}"]
    out = subprocess.run([str(exe)], input="\n".join(script) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()

    def block(start, n):
        return lines[start + 1:start + 1 + n]

    # the Python mirror through the same steps
    pr = pg.OptimizationProblem()
    pr.insert_odometry_constraints([odom[2], odom[0], odom[1]])
    pr.insert_loop_closure_constraints([loop])
    pr.insert_loop_closure_constraints([loop])
    pr.build_optimization_problem()
    at = 0
    assert lines[at] == "nodes 4"
    assert all(np.array_equal(a, b) for a, b in zip(_mats(block(at, 4)), pr.pose_graph.nodes))
    at += 5
    assert lines[at] == "edges 4" and [tuple(int(v) for v in ln.split()[:3]) for ln in block(at, 4)] == [(0, 1, 0), (1, 2, 0), (2, 3, 0), (3, 0, 1)]
    at += 5
    assert lines[at].startswith("error: Graphs are not of same size")
    at += 1
    pr.solve()
    assert lines[at] == "increments 4"
    assert all(np.array_equal(a, u.dT) for a, u in zip(_mats(block(at, 4)), pr.get_optimized_transform_increments()))
    at += 5
    n_e = len(pr.pose_graph.edges)
    assert lines[at] == f"edges {n_e}"
    assert [float.fromhex(ln.split()[3]) for ln in block(at, n_e)] == [e.confidence for e in pr.pose_graph.edges]
    at += 1 + n_e
    pr.clear_odometry_constraints()
    pr.insert_odometry_constraints(odom + [extra])
    pr.build_optimization_problem()
    assert lines[at] == "nodes 5"
    assert all(np.array_equal(a, b) for a, b in zip(_mats(block(at, 5)), pr.pose_graph.nodes))
    at += 6
    pr.solve()
    assert lines[at] == "increments 5"
    assert all(np.array_equal(a, u.dT) for a, u in zip(_mats(block(at, 5)), pr.get_optimized_transform_increments()))
    at += 6
    col.transform(inc)
    maps, Ts = calls[0]
    assert lines[at] == "plan 5"
    assert [int(ln.split()[0]) for ln in block(at, 5)] == [col.maps.index(m) for m in maps]
    assert all(np.array_equal(a, b) for a, b in zip(_mats(block(at, 5)), Ts))
    at += 6
    assert lines[at].startswith("error: Stuck in a loop")
