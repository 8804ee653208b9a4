"""Numpy restatement of the localizability analysis, written from the arithmetic contract in
include/localizability/o3s_localizability.h: fp32 per-pair terms, fp64 sums, the same cyclic Jacobi, the same sign rule — and the
scenes the tests run it on.  Nothing here calls the library."""
import math

import numpy as np

KAPPA_F = math.cos(math.radians(80.0))
KAPPA_S = math.cos(math.radians(35.0))
MAX_SWEEPS = 16
F32 = np.float32


# ---- per-pair terms, fp32, left to right -------------------------------------------------------------------------------------------
def pair_terms(p, n):
    """(c, tau) of (K, 3) fp32 centred points and normals: c = p x n, tau = c / |p| (0 where |p| = 0)."""
    p = np.ascontiguousarray(p, F32)
    n = np.ascontiguousarray(n, F32)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        c = np.stack([F32(py * nz) - F32(pz * ny), F32(pz * nx) - F32(px * nz), F32(px * ny) - F32(py * nx)], axis=1).astype(F32)
        r = np.sqrt(F32(F32(F32(px * px) + F32(py * py)) + F32(pz * pz))).astype(F32)
        tau = np.where((r > 0)[:, None], c / np.where(r > 0, r, F32(1))[:, None], F32(0)).astype(F32)
    return c, tau


def hessian_blocks(p, n, fsum=True):
    """(A_t, A_r): 3 x 3 fp64, sums of exact products of the promoted fp32 values (math.fsum: the correctly rounded sum)."""
    c, _ = pair_terms(p, n)
    out = []
    for g in (np.asarray(n, F32).astype(np.float64), c.astype(np.float64)):
        A = np.zeros((3, 3))
        for a in range(3):
            for b in range(a, 3):
                prod = g[:, a] * g[:, b]
                with np.errstate(all="ignore"):
                    A[a, b] = A[b, a] = math.fsum(prod) if (fsum and np.isfinite(prod).all()) else prod.sum()
        out.append(A)
    return out[0], out[1]


# ---- the eigen step ------------------------------------------------------------------------------------------------------------------
def jacobi3(A):
    """(eval[3] ascending, evec[3][3] with evec[j] the unit direction of eval[j]) of a symmetric 3 x 3, as the contract states it."""
    A = np.array(A, np.float64)
    if not np.isfinite(A).all():
        return np.full(3, np.nan), np.full((3, 3), np.nan)
    a = A.copy()
    V = np.eye(3)
    for _ in range(MAX_SWEEPS):
        off = (abs(a[0, 1]) + abs(a[0, 2])) + abs(a[1, 2])
        diag = (abs(a[0, 0]) + abs(a[1, 1])) + abs(a[2, 2])
        if not (off > 2.0 ** -70 * diag):
            break
        for p, q in ((0, 1), (0, 2), (1, 2)):
            r = 3 - p - q
            apq = a[p, q]
            if not (apq != 0.0):
                continue
            with np.errstate(all="ignore"):
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                at = abs(theta) + math.sqrt(theta * theta + 1.0)
            t = -1.0 / at if theta < 0.0 else 1.0 / at
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            a[p, p] = a[p, p] - t * apq
            a[q, q] = a[q, q] + t * apq
            a[p, q] = a[q, p] = 0.0
            rp, rq = a[r, p], a[r, q]
            a[r, p] = a[p, r] = c * rp - s * rq
            a[r, q] = a[q, r] = s * rp + c * rq
            vp, vq = V[:, p].copy(), V[:, q].copy()
            V[:, p] = c * vp - s * vq
            V[:, q] = s * vp + c * vq
    e = [a[0, 0], a[1, 1], a[2, 2]]
    cols = [V[:, 0].copy(), V[:, 1].copy(), V[:, 2].copy()]
    for i, j in ((0, 1), (1, 2), (0, 1)):   # the stable three-element sort
        if e[i] > e[j]:
            e[i], e[j] = e[j], e[i]
            cols[i], cols[j] = cols[j], cols[i]
    out = np.zeros((3, 3))
    for j in range(3):
        x, y, z = cols[j]
        ln = math.sqrt((x * x + y * y) + z * z)
        v = np.array([x / ln, y / ln, z / ln])
        ax, ay, az = abs(v[0]), abs(v[1]), abs(v[2])
        lead = v[0] if (ax >= ay and ax >= az) else (v[1] if ay >= az else v[2])
        out[j] = -v if lead < 0.0 else v
    return np.array(e), out


# ---- pass 2 ------------------------------------------------------------------------------------------------------------------------------
def contributions(p, n, evec):
    """(K, 6) fp64: |g . d_j| with g the normal (j < 3) or tau (j >= 3), promoted, left to right."""
    _, tau = pair_terms(p, n)
    n64, t64 = np.asarray(n, F32).astype(np.float64), tau.astype(np.float64)
    out = np.zeros((len(n64), 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            g, d = (n64 if j < 3 else t64), evec[j]
            out[:, j] = np.abs((g[:, 0] * d[0] + g[:, 1] * d[1]) + g[:, 2] * d[2])
    return out


def sums(contrib, kappa_f=KAPPA_F, kappa_s=KAPPA_S):
    """(sum_all[6], sum_strong[6], n_strong[6], abs_all[6], abs_strong[6]): correctly rounded sums (a NaN contribution fails both
    comparisons); abs_* = the sums of the magnitudes taken, i.e. the same numbers: kept for the reordering bound."""
    sa, ss, ns = np.zeros(6), np.zeros(6), np.zeros(6, np.int64)
    with np.errstate(all="ignore"):
        for j in range(6):
            a = contrib[:, j]
            sa[j] = math.fsum(a[a >= kappa_f])
            ss[j] = math.fsum(a[a >= kappa_s])
            ns[j] = int((a >= kappa_s).sum())
    return sa, ss, ns


def categories(sum_all, sum_strong, k1, k2, k3):
    return np.array([2 if (sum_all[j] >= k1 or sum_strong[j] >= k2) else (1 if sum_strong[j] >= k3 else 0) for j in range(6)], np.int32)


def analyse(p, n, k1, k2, k3, kappa_f=KAPPA_F, kappa_s=KAPPA_S, evec=None):
    """The whole analysis as a dict; evec: directions to use in pass 2 instead of the restatement's own (6, 3)."""
    At, Ar = hessian_blocks(p, n)
    et, vt = jacobi3(At)
    er, vr = jacobi3(Ar)
    own = np.concatenate([vt, vr])
    d = own if evec is None else np.asarray(evec, np.float64)
    con = contributions(p, n, d)
    sa, ss, ns = sums(con, kappa_f, kappa_s)
    return dict(A_t=At, A_r=Ar, eval=np.concatenate([et, er]), evec=own, contrib=con, sum_all=sa, sum_strong=ss, n_strong=ns,
                category=categories(sa, ss, k1, k2, k3), kept=len(np.asarray(p)))


# ---- remap (fp64), for the property tests' expectations ------------------------------------------------------------------------------
def correction(T_prior, T, centre):
    """(u, r) of dT = T . T_prior^-1 about `centre`: the translation of the centre and the rotation vector."""
    dT = np.asarray(T, np.float64) @ np.linalg.inv(np.asarray(T_prior, np.float64))
    R = dT[:3, :3]
    m = np.asarray(centre, np.float64)
    u = R @ m + dT[:3, 3] - m
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    na = np.linalg.norm(a)
    th = math.atan2(na, (np.trace(R) - 1.0) / 2.0)
    return u, (th / na) * a if na > 0 else np.zeros(3)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def _jitter(normals, rng, rad=1e-3):
    """Analytic unit normals turned by about `rad`: no exact zeros, no tied eigenvalues."""
    n = normals + rng.normal(0.0, rad, normals.shape)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _planes(K, rng, planes, weights):
    """planes: (axis, offset, half extents of the two other axes); points uniform on each, normals +-e_axis pointing inwards."""
    counts = np.floor(np.asarray(weights, np.float64) / np.sum(weights) * K).astype(int)
    counts[0] += K - counts.sum()
    P, Nn = [], []
    for (axis, off, ext), c in zip(planes, counts):
        pts = np.zeros((c, 3))
        others = [a for a in range(3) if a != axis]
        for a, e in zip(others, ext):
            pts[:, a] = rng.uniform(-e, e, c)
        pts[:, axis] = off
        nn = np.zeros((c, 3))
        nn[:, axis] = -np.sign(off) if off != 0 else 1.0
        P.append(pts)
        Nn.append(nn)
    P, Nn = np.concatenate(P), np.concatenate(Nn)
    order = rng.permutation(len(P))
    return P[order], Nn[order]


def room(K, seed=0):
    """Three unequal pairs of planes: a 10 x 7 x 3 m box seen from inside."""
    rng = np.random.default_rng(seed)
    planes = [(0, -5.0, (3.5, 1.5)), (0, 5.0, (3.5, 1.5)), (1, -3.5, (5.0, 1.5)), (1, 3.5, (5.0, 1.5)), (2, -1.5, (5.0, 3.5)), (2, 1.5, (5.0, 3.5))]
    P, Nn = _planes(K, rng, planes, [3, 3, 4, 4, 5, 5])
    return P, _jitter(Nn, rng)


def corridor(K, seed=0):
    """Floor and ceiling 60 %, walls 40 %, open along x: 40 m long, 3 m wide, 2.5 m high."""
    rng = np.random.default_rng(seed)
    planes = [(2, -1.25, (20.0, 1.5)), (2, 1.25, (20.0, 1.5)), (1, -1.5, (20.0, 1.25)), (1, 1.5, (20.0, 1.25))]
    P, Nn = _planes(K, rng, planes, [3, 3, 2, 2])
    return P, _jitter(Nn, rng)


def plane(K, seed=0, jitter=True):
    """One 20 x 20 m plane z = 0, normals e_z."""
    rng = np.random.default_rng(seed)
    P, Nn = _planes(K, rng, [(2, 0.0, (10.0, 10.0))], [1])
    return P, (_jitter(Nn, rng) if jitter else Nn)


def tunnel(K, seed=0):
    """A cylinder of radius 2 m about x, 40 m long, normals pointing at the axis."""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(0.0, 2.0 * math.pi, K)
    P = np.stack([rng.uniform(-20.0, 20.0, K), 2.0 * np.cos(phi), 2.0 * np.sin(phi)], axis=1)
    Nn = np.stack([np.zeros(K), -np.cos(phi), -np.sin(phi)], axis=1)
    return P, _jitter(Nn, rng)


SCENES = {"room": room, "corridor": corridor, "plane": plane, "tunnel": tunnel}
# the directions each scene leaves free, as (block, axis): block 0 translation, 1 rotation
FREE = {"room": [], "corridor": [(0, 0)], "plane": [(0, 0), (0, 1), (1, 2)], "tunnel": [(0, 0), (1, 0)]}


def centred_pairs(scene, K, seed=0):
    """(p, n) fp32 of a scene: the points centred on their fp64 mean, as the chain hands them to the analysis."""
    P, Nn = SCENES[scene](K, seed)
    p = (P - P.mean(0)).astype(F32)
    return p, Nn.astype(F32)


def make_T(rvec, t):
    """4 x 4 from a rotation vector and a translation."""
    rvec = np.asarray(rvec, np.float64)
    th = float(np.linalg.norm(rvec))
    T = np.eye(4)
    if th > 0:
        k = rvec / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx
    T[:3, 3] = t
    return T


def scan_pair(scene, n_scan=3000, n_map=12000, seed=0, sigma=0.002):
    """A reference cloud of the scene and a reading of it taken from a pose T_true (reading -> reference frame), with T_init a
    little off T_true: (map_xyz, map_normals, scan_xyz, scan_normals, T_true, T_init), clouds fp32."""
    rng = np.random.default_rng(1000 + seed)
    M, Mn = SCENES[scene](n_map, 2 * seed)
    S, Sn = SCENES[scene](n_scan, 2 * seed + 1)
    S = S + rng.normal(0.0, sigma, S.shape)
    T_true = make_T([0.01, -0.02, 0.3], [0.5, -0.2, 0.1])
    Ti = np.linalg.inv(T_true)
    scan = S @ Ti[:3, :3].T + Ti[:3, 3]
    scan_n = Sn @ Ti[:3, :3].T
    T_init = make_T([0.004, 0.003, -0.005], [0.03, -0.02, 0.015]) @ T_true
    return M.astype(F32), Mn.astype(F32), scan.astype(F32), scan_n.astype(F32), T_true, T_init


# ---- sweeps for the mapper: a sensor moving along x through a scene, the odometry a little off ---------------------------------------
SWEEP_RADIUS = 6.0


def sweeps(scene, n_sweeps=12, n_points=8000, step=0.25, odom_offset=(0.02, 0.0, 0.0), seed=0):
    """dict(poses, scans [(points, normals) in the sensor frame, float64], stamps, odom): the sensor moves by `step` along x per
    sweep, every sweep sees the surfaces within SWEEP_RADIUS, and the odometry carries the true motion plus `odom_offset` per sweep."""
    poses, scans, odom = [], [], []
    for k in range(n_sweeps):
        T = make_T([0, 0, 0], [step * k, 0.05, 0.1])
        rng = np.random.default_rng(5000 + 97 * seed + k)
        P, Nn = SCENES[scene](6 * n_points, 7000 + 97 * seed + k)
        local = P - T[:3, 3]
        near = np.flatnonzero(np.linalg.norm(local, axis=1) < SWEEP_RADIUS)[:n_points]
        sp = local[near] + rng.normal(0.0, 0.002, (len(near), 3))
        poses.append(T)
        scans.append((sp.astype(np.float64), Nn[near].astype(np.float64)))
        odom.append(make_T([0, 0, 0], T[:3, 3] + k * np.asarray(odom_offset, np.float64)))
    return dict(poses=poses, scans=scans, stamps=[0.1 * k for k in range(n_sweeps)], odom=odom)


def free_mask(scene, evec):
    """Which of the six returned directions are the scene's free ones: those lying in the span of the block's free axes (the
    plane's two free translations form one eigenspace: its directions are any basis of the x-y plane)."""
    m = np.zeros(6, bool)
    for block in (0, 1):
        axes = [a for b, a in FREE[scene] if b == block]
        for j in range(3):
            d = np.asarray(evec[3 * block + j], np.float64)
            m[3 * block + j] = bool(axes) and math.sqrt(sum(d[a] * d[a] for a in axes)) > 0.9
    return m


def thresholds(scene, res):
    """(k1, k2, k3) from an analysis `res` of the scene, as the tests derive them: k3 = 4 x the largest sum in a free direction,
    k1 = half the smallest sum_all in a constrained one, k2 between them (the geometric mean, at most k1)."""
    free = free_mask(scene, res["evec"])
    big_free = max([0.0] + [max(res["sum_all"][j], res["sum_strong"][j]) for j in range(6) if free[j]])
    small_con = min(res["sum_all"][j] for j in range(6) if not free[j])
    k3 = 4.0 * big_free if big_free > 0 else 1e-3 * small_con
    k1 = 0.5 * small_con
    k2 = min(k1, math.sqrt(k1 * k3))
    return k1, k2, k3, free
