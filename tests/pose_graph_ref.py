"""numpy restatement of the pose-graph solver's contract (include/pose_graph/o3s_pose_graph.h): the
line-process pose graph of Choi, Zhou, Koltun 2015 as Open3D's GlobalOptimization poses it — residual, Jacobians, linear
system, objective, the closed-form line process — and what the tests build their graphs from.  Written from the statement
with numpy's own matrix products and inverses, not from the library's code; the library is compared with it, never with its
own earlier output."""
import numpy as np


def generators():
    G = np.zeros((6, 4, 4))
    G[0, 1, 2], G[0, 2, 1] = -1.0, 1.0
    G[1, 2, 0], G[1, 0, 2] = -1.0, 1.0
    G[2, 0, 1], G[2, 1, 0] = -1.0, 1.0
    G[3, 0, 3] = G[4, 1, 3] = G[5, 2, 3] = 1.0
    return G


def lin(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2, M[0, 3], M[1, 3], M[2, 3]])


def exp6(v):
    """TransformVector6dToMatrix4d: [Rz(v2) Ry(v1) Rx(v0), (v3, v4, v5)]"""
    a, b, g = v[0], v[1], v[2]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = v[3:]
    return T


def log6(T):
    """TransformMatrix4dToVector6d"""
    sy = np.sqrt(T[0, 0] * T[0, 0] + T[1, 0] * T[1, 0])
    if sy >= 1e-6:
        r = (np.arctan2(T[2, 1], T[2, 2]), np.arctan2(-T[2, 0], sy), np.arctan2(T[1, 0], T[0, 0]))
    else:
        r = (np.arctan2(-T[1, 2], T[1, 1]), np.arctan2(-T[2, 0], sy), 0.0)
    return np.array([r[0], r[1], r[2], T[0, 3], T[1, 3], T[2, 3]])


def edge_terms(nodes, edge):
    """(e, Js, Jt) of one edge: e = lin(X^-1 Tt^-1 Ts), column i of Js = lin(X^-1 Tt^-1 G_i Ts), of Jt = lin(X^-1 Tt^-1 (-G_i) Ts)"""
    A = np.linalg.inv(edge.transformation) @ np.linalg.inv(nodes[edge.target])
    Ts = nodes[edge.source]
    e = lin(A @ Ts)
    Js, Jt = np.zeros((6, 6)), np.zeros((6, 6))
    for i, G in enumerate(generators()):
        Js[:, i] = lin(A @ G @ Ts)
        Jt[:, i] = lin(A @ (-G) @ Ts)
    return e, Js, Jt


def r2(nodes, edge):
    e = edge_terms(nodes, edge)[0]
    return float(e @ edge.information @ e)


def line_process_weight(edges, max_correspondence_distance, preference_loop_closure):
    unc = [e.information[5, 5] for e in edges if e.uncertain]
    return preference_loop_closure * max_correspondence_distance ** 2 * float(np.mean(unc)) if unc else 0.0


def linear_system(nodes, edges):
    n = len(nodes)
    H, b = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    for ed in edges:
        e, Js, Jt = edge_terms(nodes, ed)
        s, t, l, L = 6 * ed.source, 6 * ed.target, ed.confidence, ed.information
        H[s:s + 6, s:s + 6] += l * Js.T @ L @ Js
        H[s:s + 6, t:t + 6] += l * Js.T @ L @ Jt
        H[t:t + 6, s:s + 6] += l * Jt.T @ L @ Js
        H[t:t + 6, t:t + 6] += l * Jt.T @ L @ Jt
        b[s:s + 6] -= l * Js.T @ L @ e
        b[t:t + 6] -= l * Jt.T @ L @ e
    return H, b


def objective(nodes, edges, w):
    """sum over edges of l e^T Lambda e + w (sqrt(l) - 1)^2 at the edges' confidences"""
    return sum(ed.confidence * r2(nodes, ed) + w * (np.sqrt(ed.confidence) - 1.0) ** 2 for ed in edges)


def objective_eliminated(nodes, edges, w):
    """the same objective with every uncertain edge's line process at its optimum l = (w / (w + r^2))^2: w r^2 / (w + r^2)"""
    F = 0.0
    for ed in edges:
        q = r2(nodes, ed)
        F += w * q / (w + q) if ed.uncertain else q
    return F


def closed_form_confidence(nodes, edge, w):
    return (w / (w + r2(nodes, edge))) ** 2


def least_squares_optimum(nodes0, edges, w, fixed=0):
    """The minimiser of objective_eliminated by scipy.optimize.least_squares (xtol = ftol = gtol = 1e-14), node `fixed` held at its
    pose (the gauge); every other node i is Exp6(v_i) nodes0[i].  Returns (nodes, objective)."""
    from scipy.optimize import least_squares

    n = len(nodes0)
    free = [i for i in range(n) if i != fixed]
    chol = [np.linalg.cholesky(ed.information).T for ed in edges]   # r^2 = |C e|^2

    def nodes_of(v):
        out = [T.copy() for T in nodes0]
        for k, i in enumerate(free):
            out[i] = exp6(v[6 * k:6 * k + 6]) @ nodes0[i]
        return out

    def fun(v):
        ns = nodes_of(v)
        res = []
        for ed, Cm in zip(edges, chol):
            r = Cm @ edge_terms(ns, ed)[0]
            if ed.uncertain:   # |r|^2 -> w |r|^2 / (w + |r|^2): scale the residual vector
                r = r * np.sqrt(w / (w + r @ r))
            res.append(r)
        return np.concatenate(res)

    sol = least_squares(fun, np.zeros(6 * len(free)), xtol=1e-14, ftol=1e-14, gtol=1e-14, method="trf", x_scale=1.0, max_nfev=2000)
    ns = nodes_of(sol.x)
    return ns, objective_eliminated(ns, edges, w)


# ---- the graphs of the tests ---------------------------------------------------------------------------------------------

def ring_graph(PoseGraph, PoseGraphEdge, n=8, seed=3, radius=10.0, odom_sigma=(0.004, 0.03), closures=((4, 0), (6, 1), (7, 2)),
               info_scale=400.0, false_closure=None):
    """n nodes on a circle.  Certain odometry edges i -> i + 1 with noise (sigma: rotation rad, translation m); the node poses are the
    chained noisy odometry (drift); uncertain closures between true poses; optionally one gross false closure (source, target)."""
    rng = np.random.default_rng(seed)
    truth = []
    for i in range(n):
        a = 2 * np.pi * i / n
        truth.append(exp6(np.array([0.02 * np.sin(a), 0.03 * np.cos(a), a, radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(2 * a)])))
    info = np.diag([2.0, 2.0, 2.0, 1.0, 1.0, 1.0]) * info_scale
    edges, nodes = [], [truth[0].copy()]
    for i in range(n - 1):
        noise = exp6(np.concatenate([rng.normal(0, odom_sigma[0], 3), rng.normal(0, odom_sigma[1], 3)]))
        X = noise @ np.linalg.inv(truth[i + 1]) @ truth[i]           # target = i + 1, source = i
        edges.append(PoseGraphEdge(i, i + 1, X, info.copy(), False, 1.0))
        nodes.append(nodes[i] @ np.linalg.inv(X))                    # pose_t = pose_s X^-1
    for s, t in closures:
        noise = exp6(np.concatenate([rng.normal(0, 0.001, 3), rng.normal(0, 0.005, 3)]))
        edges.append(PoseGraphEdge(s, t, noise @ np.linalg.inv(truth[t]) @ truth[s], info.copy(), True, 1.0))
    if false_closure is not None:
        s, t = false_closure
        bad = exp6(np.array([0.3, -0.2, 1.0, 4.0, -3.0, 1.0]))
        edges.append(PoseGraphEdge(s, t, bad @ np.linalg.inv(truth[t]) @ truth[s], info.copy(), True, 1.0))
    return PoseGraph(nodes, edges), truth
