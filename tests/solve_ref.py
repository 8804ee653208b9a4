"""Scenes for the 6x6 point-to-plane solve and a plain float64 reference of it.  numpy only.

A scene is (ref, ref_normals, reading, weights) with ids[i] = i: N points p ~ U[-1,1]^3 shaped into a surface, its normals, the same
points under a small rigid motion, and 0/1 weights.  What a scene is for is the 6x6 system A x = b its pairs add up to
(PointToPlane.cpp:185-238): the surfaces below leave A with rank 6, 5 or 3, well or badly conditioned, and `tilted` slides the
condition number of a degenerate surface continuously through the solver's decisions (fast path / rank threshold / fp64 fallback).
"""
import numpy as np

N = 400
EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
RCOND32 = 6 * EPS32   # FullPivHouseholderQR's threshold (6 eps of the largest pivot): branches 0 and 1
RCOND64 = 6 * EPS64   # the double JacobiSVD's: branch 2

ORDINARY = ((0.01, -0.02, 0.015), (0.05, -0.03, 0.08))
# motions along the scene's weak directions only: b then lies (almost) wholly in the direction a rank decision drops
IN_NULL = {
    "plane": ((0.0, 0.0, 0.02), (0.05, -0.03, 0.0)),
    "corridor": ((0.0, 0.0, 0.0), (0.05, 0.0, 0.0)),
    "cylinder": ((0.0, 0.0, 0.02), (0.0, 0.0, 0.05)),
}
SEEDS = {"generic": 101, "plane": 102, "corridor": 103, "cylinder": 104, "sphere": 105}
TILT_SEED = 211


def rodrigues_f64(rv):
    """exp([rv]x) in float64: the rotation build_step forms from x[:3] (AngleAxis(|rv|, rv / |rv|).toRotationMatrix())."""
    rv = np.asarray(rv, np.float64)
    th = float(np.sqrt((rv * rv).sum()))
    if th == 0.0:
        return np.eye(3)
    a = rv / th
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def move(p, motion):
    rv, t = motion
    return (np.asarray(p, np.float64) @ rodrigues_f64(rv).T + np.asarray(t, np.float64)).astype(np.float32)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def surface(kind, n=N):
    """(points, normals) in float64 of the named surface, from the scene's fixed seed."""
    u = np.random.default_rng(SEEDS[kind]).uniform(-1.0, 1.0, (n, 3))
    if kind == "generic":
        nrm = _unit(np.random.default_rng(SEEDS[kind] + 1000).normal(size=(n, 3)))
        return u, nrm
    if kind == "plane":
        p = u.copy()
        p[:, 2] = 0.0
        return p, np.tile([0.0, 0.0, 1.0], (n, 1))
    if kind == "corridor":   # floor z = -1 (normal +z) and wall y = 1 (normal -y): nothing sees x
        p = u.copy()
        nrm = np.zeros((n, 3))
        h = n // 2
        p[:h, 2] = -1.0
        nrm[:h, 2] = 1.0
        p[h:, 1] = 1.0
        nrm[h:, 1] = -1.0
        return p, nrm
    if kind == "cylinder":   # radius 1.5 about z: nothing sees z, and the turn about z only through the reading's offset
        th = np.pi * u[:, 0]
        nrm = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1)
        p = 1.5 * nrm
        p[:, 2] = u[:, 2]
        return p, nrm
    if kind == "sphere":     # radius 2: the three rotations are seen only at second order of the motion
        nrm = _unit(u)
        return 2.0 * nrm, nrm
    raise ValueError(kind)


def _scene(p, nrm, motion, weights=None):
    n = p.shape[0]
    w = np.ones(n, np.float32) if weights is None else weights
    return p.astype(np.float32), nrm.astype(np.float32), move(p, motion), w


def generic(n=N, motion=ORDINARY):
    return _scene(*surface("generic", n), motion)


def plane(n=N, motion=ORDINARY):
    return _scene(*surface("plane", n), motion)


def corridor(n=N, motion=ORDINARY):
    return _scene(*surface("corridor", n), motion)


def cylinder(n=N, motion=ORDINARY):
    return _scene(*surface("cylinder", n), motion)


def sphere(n=N, motion=ORDINARY):
    return _scene(*surface("sphere", n), motion)


def no_normals(n=N, motion=ORDINARY):
    """The generic scene with every reference normal zero: A = 0 and b = 0, the solver's rank-0 return (x = 0)."""
    p, nrm = surface("generic", n)
    return _scene(p, np.zeros_like(nrm), motion)


def pairs(K, n=N, motion=ORDINARY):
    """The generic scene with exactly K pairs kept: rank K for K <= 5 (K = 1: b = 0, x = 0, a pure translation step)."""
    w = np.zeros(n, np.float32)
    w[np.random.default_rng(300 + K).choice(n, K, replace=False)] = 1.0
    return _scene(*surface("generic", n), motion, w)


def tilted(kind, eps, motion=ORDINARY, n=N):
    """plane / corridor / cylinder with eps * N(0,1) added to every normal before normalising; one noise draw for every eps, so
    that kappa_2(A) is a continuous function of eps."""
    p, nrm = surface(kind, n)
    noise = np.random.default_rng(TILT_SEED).normal(size=(n, 3))
    return _scene(p, _unit(nrm + float(eps) * noise), motion)


EXACT_RANK = {"plane": 3, "corridor": 5, "cylinder": 5}
SWEEP_ORDINARY = ("plane", np.logspace(-1, -6, 21))
SWEEP_IN_NULL = np.logspace(-2.5, -3.7, 49)


def all_cases():
    """Every system of the solver tests, as (name, scene-thunk, kind): kind 'fixed' for the named scenes, 'sweep' for the tilted ones."""
    out = [("generic", generic, "fixed"), ("plane", plane, "fixed"), ("corridor", corridor, "fixed"), ("cylinder", cylinder, "fixed"),
           ("sphere", sphere, "fixed"), ("no_normals", no_normals, "fixed")]
    for K in range(1, 7):
        out.append((f"pairs{K}", (lambda K=K: pairs(K)), "fixed"))
    kind, epss = SWEEP_ORDINARY
    for e in epss:
        out.append((f"tilted-{kind}-ordinary-{e:.3e}", (lambda e=e: tilted(kind, e)), "sweep"))
    for kind in ("plane", "corridor", "cylinder"):
        for e in SWEEP_IN_NULL:
            out.append((f"tilted-{kind}-innull-{e:.3e}", (lambda kind=kind, e=e: tilted(kind, e, IN_NULL[kind])), "sweep"))
    return out


def minimize_inputs(scene, reference_mean):
    """(reading in the centred frame, ids, squared distances, weights): what ICP.minimize / OracleIcp.p2plane_step take after
    init_reference(ref, ref_normals) returned `reference_mean`."""
    ref, _, reading, w = scene
    m = np.asarray(reference_mean, np.float32)
    q = reading - m
    d = q - (ref - m)
    d2 = (d * d).sum(axis=1).astype(np.float32)
    return q, np.arange(ref.shape[0], dtype=np.int32), d2, w


FLAT = dict(max_dist=float("inf"), trim_ratio=None, max_normal_angle=None)   # every pair kept: the weights alone decide


def oracle_system(orc, scene):
    """(OracleIcp with the scene's reference, minimize inputs, T, A, b, x, branch) of one scene; `orc` is the oracle module (this
    file imports numpy only)."""
    o = orc.OracleIcp(orc.OracleConfig(max_dist=float("inf"), trim_ratio=-1.0, max_normal_angle=-1.0), threads=1)
    assert o.init_reference(scene[0], scene[1]) == orc.OK
    inputs = minimize_inputs(scene, o.reference_mean())
    T, A, b, x = o.p2plane_step(*inputs)
    x6, branch = orc.solve6(A, b)
    assert np.array_equal(x6.view(np.uint32), x.view(np.uint32))
    return o, inputs, T, A, b, x, branch


KAPPA_FAST = 600.0      # below: the fast path is certainly taken   (cond_F bound <= 1.01 * 6 sqrt(6) * kappa_2 < 1e4)
KAPPA_GENERAL = 1.0e4   # from here on it is certainly refused      (cond_F >= kappa_2)


def reach(records):
    """records: (branch, kappa_2) of the sweep points -> the four counts both test files assert on."""
    return {"fast": sum(1 for br, k in records if k < KAPPA_FAST),
            "general_rank6": sum(1 for br, k in records if br == 0 and k >= KAPPA_GENERAL),
            "min_norm": sum(1 for br, k in records if br == 1),
            "fp64": sum(1 for br, k in records if br == 2)}


REACH_MIN = {"fast": 3, "general_rank6": 3, "min_norm": 3, "fp64": 10}


def well_separated(kind, branch, kappa):
    """Is the system away from the rank decision, so that a float64 SVD with the branch's threshold must agree with the solver?
    The fixed scenes are by construction; a sweep point is with kappa_2 <= 5e5 or >= 1e7 (the QR decides near 1 / (6 eps) = 1.4e6);
    the fp64 fallback makes no decision of its own in that range (its threshold is 6 * 2^-52)."""
    return kind == "fixed" or branch == 2 or kappa <= 5.0e5 or kappa >= 1.0e7


X_F64_BOUND = 1.0e-4    # |x - x_f64| / |x_f64|: see tests/test_solve_ref.py for the measured maxima this stands 30 times above


def kappa2(A):
    s = np.linalg.svd(np.asarray(A, np.float64), compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else float("inf")


def rank_f64(A, rcond=RCOND32):
    s = np.linalg.svd(np.asarray(A, np.float64), compute_uv=False)
    return int((s > rcond * s[0]).sum())


def min_norm_f64(A, b, rcond):
    """Minimum-norm least-squares solution of the symmetric system in float64: singular values <= rcond * s_max are dropped."""
    A = np.asarray(A, np.float64)
    A = 0.5 * (A + A.T)
    U, s, Vt = np.linalg.svd(A)
    keep = s > rcond * s[0]
    if s[0] == 0.0:
        return np.zeros(6)
    c = (U.T @ np.asarray(b, np.float64))[keep] / s[keep]
    return Vt[keep].T @ c


def rel_err(x, x_ref):
    x = np.asarray(x, np.float64)
    x_ref = np.asarray(x_ref, np.float64)
    den = np.linalg.norm(x_ref)
    return float(np.linalg.norm(x - x_ref) / den) if den > 0 else float(np.linalg.norm(x))
