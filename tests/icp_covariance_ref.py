"""Restatement of PointToPlaneWithCovErrorMinimizer::estimateCovariance (libpointmatcher, ErrorMinimizers/PointToPlaneWithCov.cpp)
in numpy (test infrastructure), written from the arithmetic contract of include/o3s_icp.h ("pose covariance") — the same text the
kernel k_cov of csrc/icp_kernels.h is written from.

The per-pair terms are fp32 in the contract's left-to-right order (numpy evaluates one operation per ufunc call and never contracts
a * b + c; sqrt and / are correctly rounded).  The 42 sums are fp64 sums of exact products of promoted fp32 values, in one of three
orders (`mode`): "fsum" (math.fsum: the correctly rounded sum), "seq" (one running sum) and "pairwise" (numpy's blocked pairwise
sum).  The inverse is LAPACK's partial-pivot LU in fp64.

Parameter order of the 6 x 6 result: [t_x, t_y, t_z, alpha, beta, gamma] — translation first.
"""
import math

import numpy as np

F = np.float32
TRI = [(a, c) for a in range(6) for c in range(a, 6)]   # row-major upper triangle: the order of the library's 21 + 21 sums


def angles(T):
    """(alpha, beta, gamma, tx, ty, tz) of the 4x4 step: fp64 asin / atan2 / cos on the promoted fp32 entries, each rounded once."""
    T = np.asarray(T, F)
    beta = F(-math.asin(float(T[2, 0])))
    alpha = F(math.atan2(float(T[2, 1]), float(T[2, 2])))
    cb = math.cos(float(beta))
    gamma = F(math.atan2(float(T[1, 0]) / cb, float(T[0, 0]) / cb))
    return alpha, beta, gamma, F(T[0, 3]), F(T[1, 3]), F(T[2, 3])


def pair_terms(p, q, n, T):
    """h, u, v of every pair: (K, 6) fp32 each."""
    p, q, n = (np.ascontiguousarray(x, F).reshape(-1, 3) for x in (p, q, n))
    al, be, ga, tx, ty, tz = angles(T)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        r = np.sqrt((px * px + py * py) + pz * pz)
        dx, dy, dz = px / r, py / r, pz / r
        s = np.sqrt((qx * qx + qy * qy) + qz * qz)
        ex, ey, ez = qx / s, qy / s, qz / s
        na = nz * dy - ny * dz
        nb = nx * dz - nz * dx
        ng = ny * dx - nx * dy
        E = nx * ((((px - ga * py) + be * pz) + tx) - qx)
        E = E + ny * ((((ga * px + py) - al * pz) + ty) - qy)
        E = E + nz * (((((-be) * px + al * py) + pz) + tz) - qz)
        Nr = nx * ((dx - ga * dy) + be * dz)
        Nr = Nr + ny * ((ga * dx + dy) - al * dz)
        Nr = Nr + nz * (((-be) * dx + al * dy) + dz)
        Nq = -((nx * ex + ny * ey) + nz * ez)
        w = E + r * Nr
        h = np.stack([nx, ny, nz, r * na, r * nb, r * ng], axis=1)
        u = np.stack([nx * Nr, ny * Nr, nz * Nr, na * w, nb * w, ng * w], axis=1)
        v = np.stack([nx * Nq, ny * Nq, nz * Nq, (s * na) * Nq, (s * nb) * Nq, (s * ng) * Nq], axis=1)
    for x in (h, u, v):
        assert x.dtype == F
    return h, u, v


def _sum(cols, mode):
    """cols: list of (K,) fp64 arrays whose elements are all summed."""
    if mode == "fsum":
        return math.fsum(x for c in cols for x in c.tolist())
    if mode == "seq":
        acc = 0.0
        for c in cols:
            acc = float(np.cumsum(np.concatenate([[acc], c]))[-1])   # cumsum is one running sum
        return acc
    if mode == "pairwise":
        return float(sum(np.sum(np.ascontiguousarray(c)) for c in cols))
    raise ValueError(mode)


def sums(h, u, v, mode="fsum"):
    """H = sum h h^T and M = sum (u u^T + v v^T), 6 x 6 fp64, from exact products of the promoted fp32 terms."""
    h, u, v = (x.astype(np.float64) for x in (h, u, v))
    H = np.zeros((6, 6))
    M = np.zeros((6, 6))
    for a, c in TRI:
        H[a, c] = H[c, a] = _sum([h[:, a] * h[:, c]], mode)
        M[a, c] = M[c, a] = _sum([u[:, a] * u[:, c], v[:, a] * v[:, c]], mode)
    return H, M


def sigma2(sensor_std_dev):
    return float(F(sensor_std_dev) * F(sensor_std_dev))


def finish(H, M, sensor_std_dev):
    """sigma2 * H^-1 * M * H^-1 in fp64; NaN when H is singular or not finite."""
    if not (np.isfinite(H).all() and np.isfinite(M).all()):
        return np.full((6, 6), np.nan)
    try:
        Hi = np.linalg.inv(H)
    except np.linalg.LinAlgError:
        return np.full((6, 6), np.nan)
    return sigma2(sensor_std_dev) * (Hi @ M @ Hi)


def covariance(p, q, n, T, sensor_std_dev, mode="fsum"):
    """(cov, H): the contract, with the sums taken in order `mode`."""
    h, u, v = pair_terms(p, q, n, T)
    H, M = sums(h, u, v, mode)
    return finish(H, M, sensor_std_dev), H


def covariance_matrix_form(p, q, n, T, sensor_std_dev):
    """The second transcription, as the source writes it: the explicit 6 x 2K matrix d2J_dZdX = [d2J_dReadingdX | d2J_dReferencedX]
    and its product with its transpose; J_hessian as a product as well.  fp64 products of the fp32 per-pair terms."""
    h, u, v = pair_terms(p, q, n, T)
    d2J_dZdX = np.concatenate([u.astype(np.float64).T, v.astype(np.float64).T], axis=1)   # 6 x 2K
    J_hessian = h.astype(np.float64).T @ h.astype(np.float64)
    inv_J = np.linalg.inv(J_hessian)
    return sigma2(sensor_std_dev) * (inv_J @ (d2J_dZdX @ d2J_dZdX.T) @ inv_J)


def covariance_fp32(p, q, n, T, sensor_std_dev):
    """A bit-faithful-in-spirit fp32 evaluation: sequential fp32 sums of fp32 products, fp32 inverse and products.  Recorded in
    DESIGN beside the contract; never asserted tighter than finiteness."""
    h, u, v = pair_terms(p, q, n, T)
    H = np.zeros((6, 6), F)
    M = np.zeros((6, 6), F)
    for a in range(6):
        for c in range(6):
            H[a, c] = np.cumsum(h[:, a] * h[:, c], dtype=F)[-1]
            M[a, c] = np.cumsum(np.concatenate([u[:, a] * u[:, c], v[:, a] * v[:, c]]), dtype=F)[-1]
    Hi = np.linalg.inv(H).astype(F)
    return (F(sensor_std_dev) * F(sensor_std_dev)) * ((Hi @ M).astype(F) @ Hi).astype(F)


def bound(H):
    """The tolerance of the CPU and GPU tests on |delta_ij| / sqrt(c_ii c_jj): 256 * 2^-52 * cond_2(H).  256 covers the product of
    three factors, about 204: at most 17 levels of an fp64 summation tree, two applications of H^-1, six-term inner products."""
    return 256.0 * 2.0 ** -52 * float(np.linalg.cond(H, 2))


def rel_distance(c, c_ref):
    """max |c_ij - ref_ij| / sqrt(ref_ii ref_jj)."""
    d = np.sqrt(np.abs(np.diag(c_ref)))
    return float(np.max(np.abs(np.asarray(c, np.float64) - c_ref) / np.outer(d, d)))


def rot_step(deg, axis=(0.3, -0.5, 0.8), t=(0.02, -0.01, 0.005)):
    """A 4x4 fp32 step: rotation by `deg` about `axis` and a small translation; deg = 0 and t = None give the identity."""
    T = np.eye(4)
    if deg:
        a = np.asarray(axis, np.float64)
        a = a / np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        th = math.radians(deg)
        T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    if t is not None:
        T[:3, 3] = t
    return T.astype(F)


def room_pairs(K, seed=0, noise=0.01):
    """K centred pairs (p, q, n), (K, 3) fp32, of a room: points on the six faces of a 10 x 8 x 3 m box with slightly perturbed
    face normals — well spread over three axes, so H is well conditioned — the reading a noisy, slightly shifted copy."""
    rng = np.random.default_rng(4242 + seed)
    half = np.array([5.0, 4.0, 1.5])
    face = rng.integers(0, 6, K)
    face[:6] = np.arange(6)[:min(K, 6)]      # every face is present from K = 6 on
    ax, sign = face // 2, 1.0 - 2.0 * (face % 2)
    q = rng.uniform(-1, 1, (K, 3)) * half
    q[np.arange(K), ax] = sign * half[ax]
    n = rng.normal(0, 0.05, (K, 3))
    n[np.arange(K), ax] = -sign
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    p = q + rng.normal(0, noise, (K, 3)) + np.array([0.03, -0.02, 0.01])
    p32, q32 = p.astype(F), q.astype(F)
    mp = (p32.astype(np.float64).sum(0) / K).astype(F)
    mq = (q32.astype(np.float64).sum(0) / K).astype(F)
    return p32 - mp, q32 - mq, n.astype(F)
