"""Numpy restatement of the partial-direction treatment of the degeneracy-aware ICP step, written from the arithmetic contract in
include/degeneracy/o3s_degeneracy_partial.h: the strong-pair sums (math.fsum: correctly rounded), the projection of the normal
equations onto C x = d in fp64, left to right, and the constrained chain with values built on the helpers of tests/degeneracy_ref.py
and tests/localizability_ref.py.  Nothing here calls the library under test."""
import math

import numpy as np

import degeneracy_ref as dref
import localizability_ref as lref

F32 = np.float32
EPS64 = 2.0 ** -53


# ---- the strong-pair sums ------------------------------------------------------------------------------------------------------------
def residuals(p, q, n):
    """h (K,) fp32 of centred pairs: e = p - q, h = ((0 + ex nx) + ey ny) + ez nz, no FMA, left to right."""
    p, q, n = (np.ascontiguousarray(a, F32) for a in (p, q, n))
    with np.errstate(all="ignore"):
        e = (p - q).astype(F32)
        h = F32(0) + F32(e[:, 0] * n[:, 0])
        h = F32(h + F32(e[:, 1] * n[:, 1]))
        h = F32(h + F32(e[:, 2] * n[:, 2]))
    return h.astype(F32)


def strong_sums(p, q, n, evec, contrib=None, kappa_s=lref.KAPPA_S):
    """dict(num[6], den[6], abs_num[6], abs_den[6], value[6]): over the pairs with a_j >= kappa_s, s = (g0 d0 + g1 d1) + g2 d2 with
    g = n (j < 3) or c = p x n (j >= 3) promoted to fp64, num = sum s h, den = sum s s; abs_* = the sums of the magnitudes of the
    terms, for the reordering bound."""
    c, _ = lref.pair_terms(p, n)
    if contrib is None:
        contrib = lref.contributions(p, n, np.asarray(evec, np.float64))
    h = residuals(p, q, n).astype(np.float64)
    n64, c64 = np.asarray(n, F32).astype(np.float64), c.astype(np.float64)
    num, den, anum, aden = np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6)
    with np.errstate(all="ignore"):
        for j in range(6):
            g, d = (n64 if j < 3 else c64), np.asarray(evec[j], np.float64)
            s = (g[:, 0] * d[0] + g[:, 1] * d[1]) + g[:, 2] * d[2]
            take = contrib[:, j] >= kappa_s
            tn, td = (s * h)[take], (s * s)[take]
            num[j], den[j] = math.fsum(tn), math.fsum(td)
            anum[j], aden[j] = math.fsum(np.abs(tn)), math.fsum(td)
    return dict(num=num, den=den, abs_num=anum, abs_den=aden, value=np.array([quotient(num[j], den[j]) for j in range(6)]))


def quotient(num, den):
    """-num / den; 0 when den is 0 or the quotient is not finite."""
    if den == 0.0:
        return 0.0
    with np.errstate(all="ignore"):
        v = -np.float64(num) / np.float64(den)
    return float(v) if math.isfinite(v) else 0.0


def sum_bounds(sums, K):
    """(bound of num[6], bound of den[6]): (K + 8) 2^-53 times the sum of the magnitudes of the terms — K additions in any order
    and the roundings of the products."""
    return (K + 8) * EPS64 * sums["abs_num"], (K + 8) * EPS64 * sums["abs_den"]


def value_bound(sums, K, j, dir_err=0.0):
    """The sums' bounds propagated through the quotient -num / den, and one rounding of the division.  dir_err: a bound of the
    error of the direction itself (two eigen solvers): |delta s| <= |g| dir_err, and a strong pair has |s| >= KAPPA_S |g| (for a
    rotation row g = c = r tau), so the terms move by at most dir_err / KAPPA_S (num) and twice that (den) of their magnitudes."""
    bn, bd = sum_bounds(sums, K)
    bn = bn + dir_err / lref.KAPPA_S * sums["abs_num"]
    bd = bd + 2.0 * dir_err / lref.KAPPA_S * sums["abs_den"]
    den = sums["den"][j]
    if not den > bd[j]:
        return math.inf
    v = abs(sums["value"][j])
    return (bn[j] + v * bd[j]) / (den - bd[j]) + 2 * EPS64 * v


# ---- the projection onto C x = d -----------------------------------------------------------------------------------------------------
def project_values(A, b, rot, trans, d):
    """(A', b') of the contract for a symmetric 6 x 6 A, b (= -g) and the values d of the rows of C (rotation rows first), fp64,
    every sum left to right from 0.  A' is degeneracy_ref.project's.  The empty set returns the input itself."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    C, n_rot = dref.rows_of(rot, trans)
    if len(C) == 0:
        return A, b
    d = np.asarray(d, np.float64).reshape(-1)
    assert len(d) == len(C)
    Ap, _ = dref.project(A, b, rot, trans)
    D = np.zeros((6, 6))
    for a in range(6):
        for c in range(6):
            for j in range(len(C)):
                D[a, c] += C[j, a] * C[j, c]
    P = np.eye(6) - D
    g = -b
    xc, rs, ts = np.zeros(6), np.zeros(6), np.zeros(6)
    for a in range(6):
        for j in range(len(C)):
            xc[a] += C[j, a] * d[j]
            if j < n_rot:
                rs[a] += C[j, a] * d[j]
            else:
                ts[a] += C[j, a] * d[j]
    g2 = np.zeros(6)
    for k in range(6):
        s = 0.0
        for m in range(6):
            s += A[k, m] * xc[m]
        g2[k] = g[k] + s
    mu_r, mu_t = dref._mu(A, 0), dref._mu(A, 3)
    gp = np.zeros(6)
    for a in range(6):
        v = 0.0
        for k in range(6):
            v += P[a, k] * g2[k]
        gp[a] = (v - mu_r * rs[a]) - mu_t * ts[a]
    return Ap, -gp


def value_leakage(x, rot, trans, d):
    """max |e_j . x - d_j| over the rows of C."""
    C, _ = dref.rows_of(rot, trans)
    return float(np.abs(C @ np.asarray(x, np.float64) - np.asarray(d, np.float64).reshape(-1)).max()) if len(C) else 0.0


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------
def door(K, seed=0):
    """lref.corridor with a 1.0 x 0.8 m panel across it at x = 3 (2 % of the points): the one thing that sees the axis."""
    kp = int(0.02 * K)
    P, Nn = lref.corridor(K - kp, seed)
    rng = np.random.default_rng(90000 + seed)
    panel = np.stack([np.full(kp, 3.0), rng.uniform(-0.5, 0.5, kp), rng.uniform(-0.4, 0.4, kp)], axis=1)
    pn = lref._jitter(np.tile(np.array([-1.0, 0.0, 0.0]), (kp, 1)), rng)
    P, Nn = np.concatenate([P, panel]), np.concatenate([Nn, pn])
    order = rng.permutation(len(P))
    return P[order], Nn[order]


def door_pair(n_scan=3000, n_map=12000, seed=0, sigma=0.002):
    """lref.scan_pair on the door scene: (map_xyz, map_normals, scan_xyz, scan_normals, T_true, T_init), clouds fp32."""
    rng = np.random.default_rng(1000 + seed)
    M, Mn = door(n_map, 2 * seed)
    S, Sn = door(n_scan, 2 * seed + 1)
    S = S + rng.normal(0.0, sigma, S.shape)
    T_true = lref.make_T([0.01, -0.02, 0.3], [0.5, -0.2, 0.1])
    Ti = np.linalg.inv(T_true)
    scan = S @ Ti[:3, :3].T + Ti[:3, 3]
    scan_n = Sn @ Ti[:3, :3].T
    T_init = lref.make_T([0.004, 0.003, -0.005], [0.03, -0.02, 0.015]) @ T_true
    return M.astype(F32), Mn.astype(F32), scan.astype(F32), scan_n.astype(F32), T_true, T_init


def door_sweeps(n_sweeps=6, n_points=8000, step=0.25, odom_offset=(0.005, 0.02, 0.015), seed=0):
    """lref.sweeps on the door scene: the sensor moves towards the panel along x, the odometry a little off in all three directions,
    along the axis by the least."""
    poses, scans, odom = [], [], []
    for k in range(n_sweeps):
        T = lref.make_T([0, 0, 0], [step * k, 0.05, 0.1])
        rng = np.random.default_rng(5000 + 97 * seed + k)
        P, Nn = door(6 * n_points, 7000 + 97 * seed + k)
        local = P - T[:3, 3]
        near = np.flatnonzero(np.linalg.norm(local, axis=1) < lref.SWEEP_RADIUS)[:n_points]
        sp = local[near] + rng.normal(0.0, 0.002, (len(near), 3))
        poses.append(T)
        scans.append((sp.astype(np.float64), Nn[near].astype(np.float64)))
        odom.append(lref.make_T([0, 0, 0], T[:3, 3] + k * np.asarray(odom_offset, np.float64)))
    return dict(poses=poses, scans=scans, stamps=[0.1 * k for k in range(n_sweeps)], odom=odom)


def door_thresholds(res):
    """(k1, k2, k3) from the first iteration's analysis: the axis (direction 0) falls between k3 and k2, every other direction
    above k1."""
    k1 = 0.5 * min(res["sum_all"][1:6])
    k3 = 0.25 * res["sum_strong"][0]
    k2 = min(k1, 4.0 * res["sum_strong"][0])
    return k1, k2, k3


# ---- the constrained chain with values ---------------------------------------------------------------------------------------------------
def prepare(orc, o, ref_xyz, ref_normals, scan, scan_normals, T_init):
    """What every iteration of a chain starts from, as degeneracy_ref.constrained_chain forms it: the centred reference, the reading
    under T_refMean_readMean, that transformation and the reference's mean."""
    mean = o.reference_mean().astype(F32)
    ref_c = (np.asarray(ref_xyz, F32) - mean).astype(F32)
    T0 = np.asarray(T_init, F32).copy()
    T0[:3, 3] = T0[:3, 3] - mean
    read, read_n = orc.rigid_transform(T0, np.asarray(scan, F32), np.asarray(scan_normals, F32))
    return dict(mean=mean, ref_c=ref_c, ref_n=np.asarray(ref_normals, F32), T0=T0, read=read[:, :3], read_n=read_n[:, :3])


def iteration(orc, o, prep, T_iter, ks):
    """One iteration's pairs under the pose T_iter (fp32, the reference's centred frame) from the oracle's module calls, their
    analysis and their strong-pair sums: dict(A, b, mp, mq, res, sums, kept)."""
    step, step_n = orc.rigid_transform(np.asarray(T_iter, F32), prep["read"], prep["read_n"])
    step, step_n = np.ascontiguousarray(step[:, :3]), np.ascontiguousarray(step_n[:, :3])
    ids, d2 = o.find_closests(step)
    w = o.outlier_weights(step_n, ids, d2)
    _, A, b, _ = o.p2plane_step(step, ids, d2, w)
    keep = w > 0
    mp = step[keep].astype(np.float64).mean(0).astype(F32)
    mq = prep["ref_c"][ids[keep]].astype(np.float64).mean(0).astype(F32)
    p = (step[keep] - mp).astype(F32)
    q = (prep["ref_c"][ids[keep]] - mq).astype(F32)
    n = prep["ref_n"][ids[keep]]
    res = lref.analyse(p, n, *ks)
    return dict(A=A, b=b, mp=mp, mq=mq, res=res, sums=strong_sums(p, q, n, res["evec"], res["contrib"]), kept=int(keep.sum()))


def iteration_set(it, min_category=2, partial=True):
    """(in_set[6], part[6], val[6]) of an iteration: the set {category < min_category} u {category == 1}, the rows that carry a
    value and the values (0 elsewhere)."""
    cat = it["res"]["category"]
    part = (cat == 1) & partial
    return (cat < min_category) | part, part, np.where(part, it["sums"]["value"], 0.0)


def constrained_chain(orc, o, ref_xyz, ref_normals, scan, scan_normals, T_init, iters, ks, min_category=2, partial=True):
    """degeneracy_ref.constrained_chain in ANALYSE mode with the flag: per iteration the set {category < min_category} u
    {category == 1}, the rows of category 1 carrying -num / den of their strong pairs.  partial=False is the chain of
    degeneracy_ref.  Returns dict(T, masks, pmasks, values [iters][6], analyses, sums, leaks, kept)."""
    prep = prepare(orc, o, ref_xyz, ref_normals, scan, scan_normals, T_init)
    T_iter = np.eye(4, dtype=F32)
    out = dict(masks=[], pmasks=[], values=[], analyses=[], sums=[], leaks=[], kept=[])
    for _ in range(iters):
        it = iteration(orc, o, prep, T_iter, ks)
        res = it["res"]
        in_set, part, val = iteration_set(it, min_category, partial)
        trans, rot = res["evec"][:3][in_set[:3]], res["evec"][3:][in_set[3:]]
        d = np.concatenate([val[3:][in_set[3:]], val[:3][in_set[:3]]])          # rotation rows first
        Ap, bp = project_values(it["A"], it["b"], rot, trans, d)
        x, _ = orc.solve6(Ap.astype(F32), bp.astype(F32))
        T_iter = (dref.step_from_x(x, it["mp"], it["mq"]).astype(F32) @ T_iter).astype(F32)
        out["masks"].append(int(sum(1 << j for j in range(6) if in_set[j])))
        out["pmasks"].append(int(sum(1 << j for j in range(6) if part[j])))
        out["values"].append(val)
        out["analyses"].append(res)
        out["sums"].append(it["sums"])
        out["leaks"].append(value_leakage(x, rot, trans, d))
        out["kept"].append(it["kept"])
    T = (T_iter @ prep["T0"]).astype(F32)
    T[:3, 3] = T[:3, 3] + prep["mean"]
    out["T"] = T
    return out


def axis_error(T, T_true):
    """|translation error along x| of a pose against the truth, metres."""
    return abs(float(np.asarray(T, np.float64)[0, 3] - np.asarray(T_true, np.float64)[0, 3]))
