"""Numpy restatement of the degeneracy-aware ICP step, written from the arithmetic contract in include/degeneracy/o3s_degeneracy.h:
the projection of the normal equations onto C x = 0 in fp64, left to right, and the constrained chain built from the oracle's module
calls, the localizability restatement (tests/localizability_ref.py) and that projection.  Nothing here calls the library under test."""
import math

import numpy as np

import localizability_ref as lref

F32 = np.float32


def rows_of(rot, trans):
    """C: the rotation directions [w; 0] in their order, then the translation directions [0; v]."""
    rot = np.asarray(rot, np.float64).reshape(-1, 3)
    trans = np.asarray(trans, np.float64).reshape(-1, 3)
    C = np.zeros((len(rot) + len(trans), 6))
    C[:len(rot), :3] = rot
    C[len(rot):, 3:] = trans
    return C, len(rot)


def _mu(A, o):
    mu = ((A[o, o] + A[o + 1, o + 1]) + A[o + 2, o + 2]) / 3.0
    return 1.0 if (not math.isfinite(mu) or mu == 0.0) else mu


def project(A, b, rot, trans):
    """(A', b') of the contract for a symmetric 6 x 6 A and b, fp64, every sum left to right from 0; A' is the upper triangle
    mirrored, as k_solve takes it.  The empty set returns the input itself."""
    A = np.array(A, np.float64)
    b = np.array(b, np.float64)
    C, n_rot = rows_of(rot, trans)
    if len(C) == 0:
        return A, b
    D = np.zeros((6, 6))
    F = np.zeros((2, 6, 6))
    for a in range(6):
        for c in range(6):
            for j in range(len(C)):
                D[a, c] += C[j, a] * C[j, c]
                F[0 if j < n_rot else 1, a, c] += C[j, a] * C[j, c]
    P = np.eye(6) - D
    M = np.zeros((6, 6))
    for a in range(6):
        for c in range(6):
            for k in range(6):
                M[a, c] += A[a, k] * P[k, c]
    mu_r, mu_t = _mu(A, 0), _mu(A, 3)
    Ap = np.zeros((6, 6))
    bp = np.zeros(6)
    for a in range(6):
        for c in range(a, 6):
            v = 0.0
            for k in range(6):
                v += P[a, k] * M[k, c]
            Ap[a, c] = Ap[c, a] = (v + mu_r * F[0, a, c]) + mu_t * F[1, a, c]
        for k in range(6):
            bp[a] += P[a, k] * b[k]
    return Ap, bp


def leakage(x, rot, trans):
    """max |e . x| over the rows of C."""
    C, _ = rows_of(rot, trans)
    return float(np.abs(C @ np.asarray(x, np.float64)).max()) if len(C) else 0.0


# ---- the step from x, as PointToPlane.cpp forms it (fp32, left to right) -------------------------------------------------------------
def step_from_x(x, mp, mq):
    """T (4 x 4 fp32) = [R(x[0:3]) | R (-mp) + (x[3:6] + mq)]: the angle-axis rotation about the kept reading centroid."""
    x = np.asarray(x, F32)
    mp = np.asarray(mp, F32)
    mq = np.asarray(mq, F32)
    n2 = F32(F32(F32(x[0] * x[0]) + F32(x[1] * x[1])) + F32(x[2] * x[2]))
    ang = F32(np.sqrt(n2))
    ax = x[:3].copy()
    wmax = F32(max(abs(x[0]), abs(x[1]), abs(x[2])))
    with np.errstate(all="ignore"):
        a = (x[:3] / wmax).astype(F32)
        z = F32(F32(F32(a[0] * a[0]) + F32(a[1] * a[1])) + F32(a[2] * a[2]))
        if z > 0:
            ax = (x[:3] / F32(F32(np.sqrt(z)) * wmax)).astype(F32)
    s, c = F32(math.sin(float(ang))), F32(math.cos(float(ang)))
    sv = (s * ax).astype(F32)
    cv = (F32(F32(1) - c) * ax).astype(F32)
    R = np.zeros((3, 3), F32)
    t = F32(cv[0] * ax[1]); R[0, 1] = t - sv[2]; R[1, 0] = t + sv[2]
    t = F32(cv[0] * ax[2]); R[0, 2] = t + sv[1]; R[2, 0] = t - sv[1]
    t = F32(cv[1] * ax[2]); R[1, 2] = t - sv[0]; R[2, 1] = t + sv[0]
    for k in range(3):
        R[k, k] = F32(F32(cv[k] * ax[k]) + c)
    T = np.eye(4, dtype=F32)
    T[:3, :3] = R
    for r in range(3):
        v = F32(R[r, 0] * -mp[0])
        v = F32(v + F32(R[r, 1] * -mp[1]))
        v = F32(v + F32(R[r, 2] * -mp[2]))
        T[r, 3] = F32(v + F32(x[3 + r] + mq[r]))
    return T


# ---- the constrained chain -------------------------------------------------------------------------------------------------------------
def constrained_chain(orc, o, ref_xyz, ref_normals, scan, scan_normals, T_init, iters, ks=None, min_category=2, fixed=None):
    """The chain of `iters` iterations (no Differential checker) restated from the oracle's module calls: per iteration
    find_closests / outlier_weights / p2plane_step (for A, b), the set (`fixed` = (rot, trans), else localizability_ref with the
    thresholds `ks` on the kept pairs), the projection, solve6 and the step.  `o`: an OracleIcp whose reference is initialised.
    Returns dict(T, masks, sets, analyses): the pose in the reference's own frame, and per iteration the 6-bit mask (bit j < 3
    translation direction j, bit 3 + j rotation direction j), the set used and the analysis (None with a fixed set)."""
    mean = o.reference_mean().astype(F32)
    ref_c = (np.asarray(ref_xyz, F32) - mean).astype(F32)
    ref_n = np.asarray(ref_normals, F32)
    T0 = np.asarray(T_init, F32).copy()
    T0[:3, 3] = T0[:3, 3] - mean                                  # T_refMean_readMean (the reading's mean is forced to 0)
    read, read_n = orc.rigid_transform(T0, np.asarray(scan, F32), np.asarray(scan_normals, F32))
    read, read_n = read[:, :3], read_n[:, :3]
    T_iter = np.eye(4, dtype=F32)
    masks, sets, analyses = [], [], []
    for _ in range(iters):
        step, step_n = orc.rigid_transform(T_iter, read, read_n)
        step, step_n = np.ascontiguousarray(step[:, :3]), np.ascontiguousarray(step_n[:, :3])
        ids, d2 = o.find_closests(step)
        w = o.outlier_weights(step_n, ids, d2)
        _, A, b, _ = o.p2plane_step(step, ids, d2, w)
        keep = w > 0
        mp = step[keep].astype(np.float64).mean(0).astype(F32)
        mq = ref_c[ids[keep]].astype(np.float64).mean(0).astype(F32)
        if fixed is not None:
            rot, trans = fixed
            mask = sum(1 << j for j in range(len(trans))) | sum(8 << j for j in range(len(rot)))
            res = None
        else:
            p = (step[keep] - mp).astype(F32)
            res = lref.analyse(p, ref_n[ids[keep]], *ks)
            low = res["category"] < min_category
            trans, rot = res["evec"][:3][low[:3]], res["evec"][3:][low[3:]]
            mask = int(sum(1 << j for j in range(6) if low[j]))
        Ap, bp = project(A, b, rot, trans)
        x, _ = orc.solve6(Ap.astype(F32), bp.astype(F32))
        T_iter = (step_from_x(x, mp, mq).astype(F32) @ T_iter).astype(F32)
        masks.append(mask)
        sets.append((np.array(rot), np.array(trans)))
        analyses.append(res)
    out = (T_iter @ T0).astype(F32)
    out[:3, 3] = out[:3, 3] + mean
    return dict(T=out, masks=masks, sets=sets, analyses=analyses)


def threshold_margins(res, ks):
    """The smallest relative distance of the restatement's sums from the thresholds that decide a category: sum_all against k1,
    sum_strong against k2 and k3."""
    k1, k2, k3 = ks
    gaps = [abs(s - k1) / k1 for s in res["sum_all"]] + [abs(s - k) / k for s in res["sum_strong"] for k in (k2, k3)]
    return min(gaps)
