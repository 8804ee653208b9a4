"""References that can judge the host arithmetic and the first pass of the loop-closure ICP (include/o3s_registration.h) where
tests/o3d_registration_ref.py cannot: rank-deficient and badly conditioned 6 x 6 systems, degenerate Umeyama inputs, the 30 sums of
one pass with an a-priori bound, GICP covariances near their branch.  Written from the published algorithms (Eigen's LDLT.h and
Umeyama.h, Open3D v0.15.1's GeneralizedICP.cpp / TransformationEstimation.cpp / Eigen.cpp), with mpmath at 60 digits where a
judge is needed and fp64 where the thing judged is "another fp64 implementation of the same algorithm".  Pinned on the CPU by
tests/test_o3d_solve_ref.py.

The layout of the 30 sums (one pass of GetRegistrationResultAndCorrespondences + the next ComputeTransformation):
  point-to-plane, GICP: [0..20] the upper triangle of J^T J row by row, [21..26] J^T r, [27] sum r^2;
  point-to-point:       [0..2] sum (s - c), [3..5] sum (t - c), [6..14] sum (t - c)(s - c)^T row-major, c a fixed shift;
  every type:           [28] sum d^2, [29] the number of correspondences.

The bound B_k of first_pass_sums
--------------------------------
u = 2^-53.  Component k of the sums is sum_i term_ik over the n correspondences.  An fp64 implementation differs from the exact
sum in two ways, and B_k = S_k + P_k is the sum of a bound for each; both are functions of the input alone.

 S_k = (n + 8) u sum_i |term_ik|: n - 1 rounded additions in ANY order (sequential, tree, per-lane partials folded later) are off
   by at most gamma_(n-1) sum |term| (Higham, Accuracy and Stability, 4.2); the 8 covers the second-order part and the fact
   that the terms added are the rounded ones.
 P_k = sum_i p_ik, the rounding inside one term, counted with the magnitudes a_ik that the term's own products reach (absolute
   values taken inside every difference, so that cancellation cannot hide an error):
   every type, [28]: d^2 = ((dx dx) + (dy dy)) + dz dz with dx = qx - tx: each square goes through (1 + u)^5 at most: p = 6 u d^2.
   point-to-plane: J = [q x n ; n], r = (q - t) . n.  A cross component is two products and a difference: within 2 u of
     aJ = |q_b n_c| + |q_c n_b| (the three n components are exact, aJ = |n|); r goes through (1 + u)^4: within 4 u of
     ar = sum |e_a n_a|.  J_a J_b: (2 + 2 + 1) u -> p = 6 u aJ_a aJ_b; J_a r: (2 + 4 + 1) u -> p = 8 u aJ_a ar; r^2: 9 u -> p = 10 u ar^2.
   point-to-point: s - c and t - c are one rounding each: p = 2 u |s - c|; their product adds one: p = 4 u |t_a - c_a| |s_b - c_b|.
   GICP: the term is G^T A G, G^T A d, d^T A d with A = M^-1, M = Ct + Cs, G = [-[q]x | I], d = q - t.  The library inverts M
     through its cofactors; a cofactor (two products, a difference of entries <= ||M||) is off by <= 4 u ||M||^2, the determinant
     (three more products, two additions) by <= 30 u ||M||^3, the sum M itself (Cs is turned by a rotation first) by <= 19 u ||M||
     per entry, which moves A by <= 57 u kappa ||A||.  Relative to det M = l1 l2 l3 these are multiples of
         rho = ||M||^3 / det M = l1^2 / (l2 l3)   (>= kappa(M) = l1 / l3, equal when the two large eigenvalues coincide, as
                                                   they do for covariances made from one normal each),
     so every entry of the computed A is within (57 + 4 + 30 + 2) u rho ||A|| <= 93 u rho ||A||.  An entry of the term multiplies A
     by two columns of G whose 1-norms are <= sqrt 2 g_a (g_a: the 2-norm of column a: sqrt(q_b^2 + q_c^2), or 1), and adds a few
     roundings of its own: p = 256 u rho_i ||A_i|| g_a g_b, with ||d||_1 in the place of g for every d.
   The reference forms the terms in np.longdouble (x86 80-bit: 2^-64) and, for GICP, A in mpmath; it adds them with math.fsum
   (exact, rounded once): its own error is 2^-11 of S_k + P_k and is not counted.

Scenes
------
edge_scene: small seeded clouds on the dyadic lattice 2^-10 inside a box of a few metres; every squared distance is then an exact
fp64 number, the placed source is exact under the poses of lattice_init (a quarter turn and a dyadic shift), so nearest
neighbours, ties and the radius test are decided exactly and `fragile` is a condition, not a measurement."""
import math

import mpmath as mp
import numpy as np

U = 2.0 ** -53
DPS = 60
LD = np.longdouble
DBL_MIN = np.finfo(np.float64).tiny
KINDS = ("PointToPlaneIcp", "PointToPointIcp", "GeneralizedIcp")
TYPE_ID = {"PointToPlaneIcp": 0, "PointToPointIcp": 1, "GeneralizedIcp": 2}   # o3s_o3d_estimation_type


# ---- Eigen LDLT<Matrix6d> in fp64 ------------------------------------------------------------------------------------------
def ldlt_solve6(A, b):
    """Eigen::LDLT<Matrix6d>(A).solve(b), fp64 (Eigen/src/Cholesky/LDLT.h, ldlt_inplace<Lower>::unblocked and _solve_impl): only the
    lower triangle is read; at step k the largest |diagonal| of the trailing block is brought to k by a symmetric transposition;
    the solve is P^T L^-T D^+ L^-1 P b with D^+ zero where |d| <= DBL_MIN."""
    m = np.tril(np.array(A, np.float64))
    n = m.shape[0]
    tr = np.zeros(n, np.int64)
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(m)[k:])))          # the first of equal maxima, as maxCoeff
        tr[k] = p
        if p != k:
            s = n - p - 1
            m[[k, p], :k] = m[[p, k], :k]                        # rows k and p left of the block
            if s:
                m[p + 1:, [k, p]] = m[p + 1:, [p, k]]            # columns k and p below p
            m[k, k], m[p, p] = m[p, p], m[k, k]
            for i in range(k + 1, p):                            # the part of row p / column k in between, transposed
                m[i, k], m[p, i] = m[p, i], m[i, k]
        if k > 0:
            temp = np.diag(m)[:k] * m[k, :k]
            m[k, k] -= float(np.dot(m[k, :k], temp))
            if k + 1 < n:
                m[k + 1:, k] -= m[k + 1:, :k] @ temp
        akk = m[k, k]
        if k == 0 and not abs(akk) > 0:                          # the whole diagonal is zero: nothing more to factor
            tr[:] = np.arange(n)
            break
        if abs(akk) > 0 and k + 1 < n:
            m[k + 1:, k] /= akk
    y = np.array(b, np.float64)
    for k in range(n):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    for i in range(n):
        y[i] -= float(np.dot(m[i, :i], y[:i]))
    d = np.diag(m)
    y = np.array([y[i] / d[i] if abs(d[i]) > DBL_MIN else 0.0 for i in range(n)])
    for i in range(n - 1, -1, -1):
        y[i] -= float(np.dot(m[i + 1:, i], y[i + 1:]))
    for k in range(n - 1, -1, -1):
        y[k], y[tr[k]] = y[tr[k]], y[k]
    return y


def _mpm(a):
    a = np.asarray(a, np.float64)
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in a]) if a.ndim == 2 else mp.matrix([mp.mpf(float(v)) for v in a])


def _np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def solve_mp(A, b, rank=None):
    """The judge of a 6 x 6 solve, mpmath at 60 digits, A symmetric (as given, not symmetrised).
    rank None / n: (x, I, eigenvalues) with A x = b exactly (LU).  rank < n — the rank the SCENE has, not one estimated from the
    data: (A^+ b, P, the `rank` largest eigenvalues) with P the orthogonal projector onto range(A), both from the eigenvectors of the
    `rank` largest |eigenvalues|.  Everything is rounded to fp64 once, at the end."""
    with mp.workdps(DPS):
        Am, bm = _mpm(A), _mpm(b)
        n = Am.rows
        E, Q = mp.eigsy(Am)
        lam = [E[i] for i in range(n)]
        if rank is None or rank == n:
            x = mp.lu_solve(Am, bm)
            return np.array([float(v) for v in x]), np.eye(n), np.array(sorted((float(v) for v in lam), reverse=True))
        keep = sorted(range(n), key=lambda i: -abs(lam[i]))[:rank]
        x = mp.zeros(n, 1)
        P = mp.zeros(n, n)
        for i in keep:
            q = Q[:, i]
            x += q * ((q.T * bm)[0] / lam[i])
            P += q * q.T
        return np.array([float(v) for v in x]), _np(P), np.array([float(lam[i]) for i in keep])


# ---- TransformVector6dToMatrix4d -------------------------------------------------------------------------------------------
def vec6_to_T_mp(x):
    """utility::TransformVector6dToMatrix4d at 60 digits: Rz(x2) Ry(x1) Rx(x0), translation x[3:]; rounded once."""
    with mp.workdps(DPS):
        a, b, g = (mp.mpf(float(v)) for v in x[:3])
        Rx = mp.matrix([[1, 0, 0], [0, mp.cos(a), -mp.sin(a)], [0, mp.sin(a), mp.cos(a)]])
        Ry = mp.matrix([[mp.cos(b), 0, mp.sin(b)], [0, 1, 0], [-mp.sin(b), 0, mp.cos(b)]])
        Rz = mp.matrix([[mp.cos(g), -mp.sin(g), 0], [mp.sin(g), mp.cos(g), 0], [0, 0, 1]])
        T = np.eye(4)
        T[:3, :3] = _np(Rz * Ry * Rx)
        T[:3, 3] = np.asarray(x[3:], np.float64)
        return T


def vec6_to_T_quat(x):
    """The same in fp64 the way Eigen does it: the three AngleAxis factors as quaternions, their product, Quaternion::toRotationMatrix."""
    def q(ang, ax):
        v = [math.cos(0.5 * ang), 0.0, 0.0, 0.0]
        v[1 + ax] = math.sin(0.5 * ang)
        return v

    def mul(a, b):
        return [a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]]

    w, qx, qy, qz = mul(mul(q(x[2], 2), q(x[1], 1)), q(x[0], 0))
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    T = np.eye(4)
    T[:3, :3] = [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]
    T[:3, 3] = x[3:]
    return T


# ---- Eigen::umeyama --------------------------------------------------------------------------------------------------------
def umeyama_mp(src, dst, rank):
    """Eigen::umeyama(src, dst, with_scaling = false) judged at 60 digits (Umeyama 1991; Eigen/src/Geometry/Umeyama.h): centred on
    the two means, sigma = (1/n) sum (d - md)(s - ms)^T.  `rank`: the rank of sigma the scene has by construction; singular values
    beyond it are exact zeros.  Returns a dict:
      sv        the singular values (descending, zeros beyond the rank),
      sigma     sigma rounded to fp64, ms, md the means,
      sign      -1 if rank 3 and det sigma < 0, else +1,
      optimum   max over proper rotations of tr(R sigma^T) = sv0 + sv1 + sign sv2,
      unique    the maximiser is unique: rank >= 2 and, for sign < 0, sv2 < sv1 (a simple smallest singular value),
      gap       what R's conditioning hangs on: sv1 + sign sv2 (the smallest sum of two signed singular values),
      R, t      the maximiser and t = md - R ms when unique, else None."""
    with mp.workdps(DPS):
        S, D = _mpm(np.asarray(src, np.float64)), _mpm(np.asarray(dst, np.float64))
        n = S.rows
        ms = mp.matrix([sum(S[i, a] for i in range(n)) / n for a in range(3)])
        md = mp.matrix([sum(D[i, a] for i in range(n)) / n for a in range(3)])
        sg = mp.zeros(3, 3)
        for i in range(n):
            ds = mp.matrix([S[i, a] - ms[a] for a in range(3)])
            dd = mp.matrix([D[i, a] - md[a] for a in range(3)])
            sg += dd * ds.T
        sg /= n
        Um, sv, Vt = mp.svd_r(sg)
        sv = [sv[i] if i < rank else mp.mpf(0) for i in range(3)]
        sign = -1 if (rank == 3 and mp.det(sg) < 0) else 1
        out = {"sv": np.array([float(v) for v in sv]), "sigma": _np(sg), "ms": np.array([float(v) for v in ms]),
               "md": np.array([float(v) for v in md]), "sign": sign, "optimum": float(sv[0] + sv[1] + sign * sv[2]),
               "gap": float(sv[1] + sign * sv[2]), "R": None, "t": None}
        out["unique"] = bool(rank >= 2 and (sign > 0 or sv[2] < sv[1] * (1 - mp.mpf(10) ** -30)))
        if out["unique"]:
            Vm = Vt.T
            if rank == 2:   # the third columns: the proper completion of the first two (any sign of either gives the same R below)
                for M_ in (Um, Vm):
                    a, b = M_[:, 0], M_[:, 1]
                    M_[0, 2], M_[1, 2], M_[2, 2] = a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]
            s3 = -1 if mp.det(Um) * mp.det(Vm) < 0 else 1
            R = Um * mp.diag([1, 1, s3]) * Vm.T
            t = md - R * ms
            out["R"], out["t"] = _np(R), np.array([float(v) for v in t])
        return out


# ---- InitializePointCloudForGeneralizedICP, one point ---------------------------------------------------------------------
def covariance_mp(n, eps):
    """C = Rx diag(eps, 1, 1) Rx^T with Rx = GetRotationFromE1ToX(n) (GeneralizedICP.cpp): v = e1 x n, c = e1 . n; Rx = I when
    c < -0.99, else I + [v]x + [v]x^2 / (1 + c).  The normal as given (not normalised), exact at 60 digits, rounded once.
    Returns (C, bound): bound_ab = 24 u (|Rx| D |Rx|^T)_ab with |Rx| = |I + [v]x| + |[v]x|^2 / (1 + c) built from absolute values: an
    fp64 evaluation gets every entry of Rx within 8 u of that (three products and two additions in [v]x^2, the factor's division
    and product, two additions), and each entry of C adds (8 + 8 + 4) u of sum_k |Rx_ak| d_k |Rx_bk|.  c = -1 (factor 1 / 0) has no
    finite reference and is not asked for."""
    n = [float(v) for v in n]
    with mp.workdps(DPS):
        c = mp.mpf(n[0])
        D = mp.diag([mp.mpf(float(eps)), 1, 1])
        if c < mp.mpf(-0.99):
            R = mp.eye(3)
            Ra = mp.eye(3)
        else:
            v = [mp.mpf(0), -mp.mpf(n[2]), mp.mpf(n[1])]
            S = mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
            f = 1 / (1 + c)
            R = mp.eye(3) + S + (S * S) * f
            Sa = S.apply(abs)
            Ra = mp.eye(3) + Sa + (Sa * Sa) * abs(f)
        return _np(R * D * R.T), 24 * U * _np(Ra * D * Ra.T)


# ---- the 30 sums of one pass -------------------------------------------------------------------------------------------------
def _two(x):
    """an mpf as a longdouble (hi + lo of two doubles: 106 bits in, 64 kept)"""
    hi = float(x)
    return LD(hi) + LD(float(x - mp.mpf(hi)))


def _fsum_ld(col):
    """the exact sum of longdoubles, rounded once to fp64: each is split into two doubles, math.fsum adds them exactly"""
    hi = col.astype(np.float64)
    lo = (col - hi.astype(LD)).astype(np.float64)
    return math.fsum(list(hi) + list(lo))


def _skew_neg(q):
    """-[q]x for each row of q: [[0, z, -y], [-z, 0, x], [y, -x, 0]]"""
    n = len(q)
    S = np.zeros((n, 3, 3), q.dtype)
    S[:, 0, 1], S[:, 0, 2] = q[:, 2], -q[:, 1]
    S[:, 1, 0], S[:, 1, 2] = -q[:, 2], q[:, 0]
    S[:, 2, 0], S[:, 2, 1] = q[:, 1], -q[:, 0]
    return S


def pass_terms(kind, q, t, tn=None, cs=None, ct=None, shift=None, dtype=np.float64, A=None):
    """The n x 30 terms of one pass over the pairs (q_i, t_i) in `dtype` arithmetic — q the source points AS PLACED, t their target
    points, tn the targets' normals, cs the source's covariances as placed (turned), ct the targets', shift the point-to-point c.
    A (GICP): the inverses (Ct + Cs)^-1 if the caller has better ones than np.linalg.inv in fp64."""
    q, t = np.asarray(q, dtype), np.asarray(t, dtype)
    n = len(q)
    T = np.zeros((n, 30), dtype)
    d = q - t
    T[:, 28] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    T[:, 29] = 1
    iu = np.triu_indices(6)
    if kind == "PointToPlaneIcp":
        nn = np.asarray(tn, dtype)
        r = (d[:, 0] * nn[:, 0] + d[:, 1] * nn[:, 1]) + d[:, 2] * nn[:, 2]
        J = np.concatenate([np.cross(q, nn), nn], axis=1)
        T[:, :21] = (J[:, :, None] * J[:, None, :])[:, iu[0], iu[1]]
        T[:, 21:27] = J * r[:, None]
        T[:, 27] = r * r
    elif kind == "PointToPointIcp":
        c = np.asarray(shift, dtype)
        s3, t3 = q - c, t - c
        T[:, 0:3], T[:, 3:6] = s3, t3
        T[:, 6:15] = (t3[:, :, None] * s3[:, None, :]).reshape(n, 9)
    else:
        if A is None:
            A = np.linalg.inv(np.asarray(ct, np.float64) + np.asarray(cs, np.float64))
        A = np.asarray(A, dtype)
        G = np.concatenate([_skew_neg(q), np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3))], axis=2)   # n x 3 x 6
        AG = A @ G
        H = np.transpose(G, (0, 2, 1)) @ AG
        Ad = (A @ d[:, :, None])[:, :, 0]
        T[:, :21] = H[:, iu[0], iu[1]]
        T[:, 21:27] = (np.transpose(G, (0, 2, 1)) @ Ad[:, :, None])[:, :, 0]
        T[:, 27] = (d * Ad).sum(axis=1)
    return T


def first_pass_sums(kind, q, t, tn=None, cs=None, ct=None, shift=None):
    """(sums[30], B[30]): the exact sums of one pass over the given pairs, rounded once, and the bound of the module docstring.  An
    empty pair list gives zeros."""
    q64, t64 = np.asarray(q, np.float64).reshape(-1, 3), np.asarray(t, np.float64).reshape(-1, 3)
    n = len(q64)
    if n == 0:
        return np.zeros(30), np.zeros(30)
    A = None
    if kind == "GeneralizedIcp":
        M = np.asarray(ct, np.float64) + np.asarray(cs, np.float64)   # (used for the bound only; the reference adds exactly below)
        A = np.zeros((n, 3, 3), LD)
        with mp.workdps(DPS):
            for i in range(n):
                Ai = (_mpm(np.asarray(ct[i], np.float64)) + _mpm(np.asarray(cs[i], np.float64))) ** -1
                for a in range(3):
                    for b in range(3):
                        A[i, a, b] = _two(Ai[a, b])
    terms = pass_terms(kind, q64, t64, tn, cs, ct, shift, dtype=LD, A=A)
    sums = np.array([_fsum_ld(terms[:, k]) for k in range(30)])
    absum = np.abs(terms).astype(np.float64).sum(axis=0)
    # the per-term part
    P = np.zeros(30)
    d = np.abs(q64 - t64)
    P[28] = 6 * U * float((d * d).sum())
    iu = np.triu_indices(6)
    if kind == "PointToPlaneIcp":
        nn = np.abs(np.asarray(tn, np.float64))
        aq = np.abs(q64)
        aJ = np.concatenate([np.stack([aq[:, 1] * nn[:, 2] + aq[:, 2] * nn[:, 1], aq[:, 2] * nn[:, 0] + aq[:, 0] * nn[:, 2],
                                       aq[:, 0] * nn[:, 1] + aq[:, 1] * nn[:, 0]], axis=1), nn], axis=1)
        ar = (d * nn).sum(axis=1)
        P[:21] = 6 * U * (aJ[:, :, None] * aJ[:, None, :])[:, iu[0], iu[1]].sum(axis=0)
        P[21:27] = 8 * U * (aJ * ar[:, None]).sum(axis=0)
        P[27] = 10 * U * float((ar * ar).sum())
    elif kind == "PointToPointIcp":
        c = np.asarray(shift, np.float64)
        s3, t3 = np.abs(q64 - c), np.abs(t64 - c)
        P[0:3], P[3:6] = 2 * U * s3.sum(axis=0), 2 * U * t3.sum(axis=0)
        P[6:15] = 4 * U * (t3[:, :, None] * s3[:, None, :]).reshape(n, 9).sum(axis=0)
    else:
        lam = np.linalg.eigvalsh(M)                       # ascending
        rho = lam[:, 2] ** 2 / (lam[:, 0] * lam[:, 1])
        nA = 1.0 / lam[:, 0]
        g = np.concatenate([np.sqrt(np.stack([q64[:, 1] ** 2 + q64[:, 2] ** 2, q64[:, 0] ** 2 + q64[:, 2] ** 2, q64[:, 0] ** 2 + q64[:, 1] ** 2], axis=1)),
                            np.ones((n, 3))], axis=1)
        d1 = d.sum(axis=1)
        w = 256 * U * rho * nA
        P[:21] = (w[:, None] * (g[:, :, None] * g[:, None, :])[:, iu[0], iu[1]]).sum(axis=0)
        P[21:27] = (w[:, None] * g * d1[:, None]).sum(axis=0)
        P[27] = float((w * d1 * d1).sum())
    B = (n + 8) * U * absum + P
    B[29] = 0.0
    return sums, B


def sums_to_system(sums):
    """(J^T J, -J^T r) of the sums of a point-to-plane / GICP pass: the system SolveJacobianSystemAndObtainExtrinsicMatrix solves"""
    A = np.zeros((6, 6))
    iu = np.triu_indices(6)
    A[iu] = sums[:21]
    A = A + np.triu(A, 1).T
    return A, -np.asarray(sums[21:27], np.float64)


def umeyama_from_sums(sums, shift):
    """h-side Umeyama as a numpy-SVD restatement, from the point-to-point sums: returns (T, sigma)"""
    n = sums[29]
    ms, mt = sums[0:3] / n, sums[3:6] / n
    sigma = sums[6:15].reshape(3, 3) / n - np.outer(mt, ms)
    Um, _, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(Um) * np.linalg.det(Vt.T) < 0:
        S[2] = -1.0
    T = np.eye(4)
    T[:3, :3] = Um @ np.diag(S) @ Vt
    T[:3, 3] = (mt + shift) - T[:3, :3] @ (ms + shift)
    return T, sigma


# ---- scenes --------------------------------------------------------------------------------------------------------------------
LAT = 2.0 ** -10


def lattice(rng, n, lo, hi):
    """n x 3 points on the dyadic lattice 2^-10 inside [lo, hi)^3"""
    return rng.integers(int(lo / LAT), int(hi / LAT), size=(n, 3)).astype(np.float64) * LAT


def lattice_init(which):
    """poses under which a lattice point stays a lattice point and every product is exact: the identity, or a quarter turn about z
    with a dyadic shift"""
    T = np.eye(4)
    if which == "quarter":
        T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
        T[:3, 3] = [0.5, -0.25, 0.125]
    return T


SPECIAL_NORMALS = [
    [1.0, 0.0, 0.0],                                    # e1: v = 0, Rx = I through the formula
    [-1.0, 0.0, 0.0],                                   # -e1: c < -0.99, the identity branch
    [-0.99, 0.0, math.sqrt(1 - 0.99 ** 2)],             # c exactly -0.99: the formula, factor 100
    [np.nextafter(-0.99, -1.0), 0.1, 0.0],              # one ulp below: the identity branch
    [0.0, 0.0, 0.0],                                    # the zero vector: c = 0, v = 0: Rx = I
    [0.6, 0.5, 0.1],                                    # not unit: used as it is
]
LONG_NORMAL = [600.0, -700.0, 380.0]                    # length ~1e3: a covariance with entries ~1e6 (rho of the module docstring ~1e12)


def special_normals(rng, n, long_normal=False):
    """n normals: the special ones first (as many as fit), random unit normals after them.  long_normal: LONG_NORMAL among the special
    ones — for the covariance tests; in a sum it would make the honest bound of its one pair swamp everyone else's."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    sp = SPECIAL_NORMALS + ([LONG_NORMAL] if long_normal else [])
    k = min(n, len(sp))
    v[:k] = np.array(sp, np.float64)[:k]
    return v


def edge_scene(ns, nt, seed, init="identity", max_dist=0.25, far=True, nonfinite=True, long_normal=False):
    """A seeded lattice scene: nt target points in a box, ns source points that — placed by `init` — lie within 1/16 of a target
    point each, except (when the flags ask and ns allows) every 7th, which lies ~100 m away, and every 11th, which has a NaN or an
    infinity in one coordinate.  Returns a dict: src, src_n, tgt, tgt_n, init, max_dist, placed (init . src, exact), corr (the
    nearest target index of each source index or -1, decided on exact squared distances), fragile (the source indices whose nearest
    neighbour is tied or whose d^2 lies within a relative 1e-9 of r^2: must be empty)."""
    rng = np.random.default_rng(seed)
    side = 1.0 if nt <= 2 else (2.0 if nt <= 300 else 4.0)
    tgt = lattice(rng, nt, 0.0, side)
    if nt > 1:   # no two target points coincide
        while len(np.unique(tgt, axis=0)) < nt:
            tgt = lattice(rng, nt, 0.0, side)
    pick = rng.integers(0, nt, size=ns)
    placed = tgt[pick] + rng.integers(-64, 65, size=(ns, 3)).astype(np.float64) * LAT
    idx = np.arange(ns)
    if far and ns >= 8:
        placed[idx % 7 == 3] += 100.0
    T = lattice_init(init)
    src = (placed - T[:3, 3]) @ T[:3, :3]      # T^-1: exact on the lattice
    bad = np.zeros(ns, bool)
    if nonfinite and ns >= 12:
        bad = idx % 11 == 5
        vals = np.array([np.nan, np.inf, -np.inf])
        src[bad, idx[bad] % 3] = vals[(idx[bad] // 11) % 3]
    with np.errstate(invalid="ignore"):
        placed = src @ T[:3, :3].T + T[:3, 3]
    corr = np.full(ns, -1, np.int32)
    fragile = []
    r2 = max_dist * max_dist
    for i in np.nonzero(~bad)[0]:
        d = placed[i] - tgt
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]     # exact: lattice coordinates below 2^8
        j = int(np.argmin(d2))
        if nt > 1 and np.partition(d2, 1)[1] == d2[j]:
            fragile.append(int(i))
        if abs(d2[j] - r2) <= 1e-9 * r2:
            fragile.append(int(i))
        if d2[j] < r2:
            corr[i] = j
    return {"src": src, "src_n": special_normals(rng, ns, long_normal), "tgt": tgt, "tgt_n": special_normals(rng, nt, long_normal), "init": T,
            "max_dist": max_dist, "placed": placed, "corr": corr, "fragile": fragile}


# (Ns, Nt, init) of the first-pass tests: Ns in {1, 2, 3, 63, 64, 65, 255, 256, 257, 1000} against Nt in {1, 2, 65, 257, 1000} — the
# diagonal, every Ns against the largest target, the largest source against every Nt; the two poses alternate, and the sizes at
# which a block, a wave or a partial fills exactly are run under both
_SIZES = ([(1, 1), (2, 2), (3, 2), (63, 65), (64, 65), (65, 65), (255, 257), (256, 257), (257, 257), (1000, 1000)] +
          [(n, 1000) for n in (1, 2, 3, 63, 64, 65, 255, 256, 257)] + [(1000, n) for n in (1, 2, 65, 257)])
EDGE_CASES = [(ns, nt, "identity" if k % 2 == 0 else "quarter") for k, (ns, nt) in enumerate(_SIZES)] + \
             [(64, 65, "quarter"), (256, 257, "quarter"), (1000, 1000, "quarter"), (65, 65, "identity"), (257, 257, "identity")]
_SCENES = {}


def edge_case(ns, nt, init, long_normal=False):
    """edge_scene of one of EDGE_CASES, made once per process (the seed is a function of the sizes)"""
    key = (ns, nt, init, long_normal)
    if key not in _SCENES:
        _SCENES[key] = edge_scene(ns, nt, 1000 + 7 * ns + nt, init, long_normal=long_normal)
    return _SCENES[key]


def fragile_pairs(placed, tgt, r):
    """For scenes off the lattice: the finite source points whose two nearest target points are within a relative 1e-9 of each other
    in d^2, or whose nearest d^2 is within a relative 1e-9 of r^2 (cKDTree, then d^2 recomputed)."""
    from scipy.spatial import cKDTree

    fin = np.isfinite(placed).all(axis=1)
    idx = np.nonzero(fin)[0]
    k = min(2, len(tgt))
    _, j = cKDTree(tgt).query(placed[fin], k=k)
    j = j.reshape(len(idx), k)
    d2 = ((placed[idx][:, None, :] - tgt[j]) ** 2).sum(axis=2)
    out = np.abs(d2[:, 0] - r * r) <= 1e-9 * r * r
    if k == 2:
        out |= np.abs(d2[:, 1] - d2[:, 0]) <= 1e-9 * np.maximum(d2[:, 1], 1e-300)
    return idx[out]


def tilted_frame(axis=(0.36, 0.48, 0.8)):
    """an orthonormal frame (u, v, n) with n along `axis`"""
    n = np.asarray(axis, np.float64)
    n = n / np.linalg.norm(n)
    a = np.array([1.0, 0.0, 0.0]) if abs(n[0]) < 0.9 else np.array([0.0, 1.0, 0.0])
    u = a - n * (a @ n)
    u /= np.linalg.norm(u)
    return u, np.cross(n, u), n


def degenerate_pairs(name, n=200, seed=0, resid=0.01):
    """Correspondence lists (q, t, tn, rank) of the degenerate scenes, for the host solve: q the source points, t their targets,
    tn the targets' normals, rank the rank of the point-to-plane system J^T J the scene has by construction.
      plane_z     dyadic points on z = 0, normal e3, source lifted by a dyadic residual         rank 3 (rx, ry, tz)
      two_planes  z = 0 with e3 and x = 0 with e1                                              rank 5 (ty dead)
      line        dyadic points on the x axis, one normal e3                                   rank 2 (ry, tz)
      tilted_plane / tilted_corridor / tilted_cylinder: the same kinds of surface in a tilted frame, generic coordinates:
                  rank 3 / 5 / 4 (a corridor leaves the shift along it free; a cylinder the turn about and the shift along its axis)"""
    rng = np.random.default_rng(seed)
    e1, e2, e3 = np.eye(3)
    if name == "plane_z":
        t = np.concatenate([lattice(rng, n, -2.0, 2.0)[:, :2], np.zeros((n, 1))], axis=1)
        tn = np.tile(e3, (n, 1))
        return t + 2.0 ** -7 * e3, t, tn, 3
    if name == "two_planes":
        h = n // 2
        a = np.concatenate([lattice(rng, h, -2.0, 2.0)[:, :2], np.zeros((h, 1))], axis=1)
        b = np.concatenate([np.zeros((n - h, 1)), lattice(rng, n - h, -2.0, 2.0)[:, :2]], axis=1)
        t = np.concatenate([a, b])
        tn = np.concatenate([np.tile(e3, (h, 1)), np.tile(e1, (n - h, 1))])
        return t + 2.0 ** -7 * tn, t, tn, 5
    if name == "line":
        t = np.concatenate([(rng.choice(4096, n, replace=False)[:, None] - 2048.0) * LAT, np.zeros((n, 2))], axis=1)   # no point twice
        tn = np.tile(e3, (n, 1))
        return t + 2.0 ** -7 * e3, t, tn, 2
    u, v, w = tilted_frame()
    org = np.array([0.7, -0.4, 1.1])
    if name == "tilted_plane":
        ab = rng.uniform(-2.0, 2.0, size=(n, 2))
        t = org + ab[:, :1] * u + ab[:, 1:] * v
        tn = np.tile(w, (n, 1))
        return t + resid * tn, t, tn, 3
    if name == "tilted_corridor":   # two parallel walls (normal w) and a floor (normal v): nothing constrains the shift along u
        ab = rng.uniform(-2.0, 2.0, size=(n, 2))
        k = np.arange(n) % 3
        t = np.where((k == 0)[:, None], org + ab[:, :1] * u + ab[:, 1:] * v + 1.5 * w,
                     np.where((k == 1)[:, None], org + ab[:, :1] * u + ab[:, 1:] * v - 1.5 * w, org + ab[:, :1] * u + ab[:, 1:] * w - 2.0 * v))
        tn = np.where((k == 2)[:, None], v, w) * np.ones((n, 1))
        return t + resid * tn, t, tn, 5
    if name == "tilted_cylinder":   # radius 1.5 about the axis org + s u: the turn about and the shift along the axis are free
        s, th = rng.uniform(-2.0, 2.0, size=n), rng.uniform(0.0, 2.0 * np.pi, size=n)
        rad = np.cos(th)[:, None] * v + np.sin(th)[:, None] * w
        t = org + s[:, None] * u + 1.5 * rad
        return t + resid * rad, t, rad, 4
    raise ValueError(name)
