"""NumPy / SciPy fp64 restatement of Open3D v0.15.1 RegistrationICP (pipelines/registration/Registration.cpp) with its three
estimation types, for the tests of include/o3s_registration.h:

  "PointToPlaneIcp"  TransformationEstimationPointToPlane        (TransformationEstimation.cpp)
  "PointToPointIcp"  TransformationEstimationPointToPoint(false)  (Eigen::umeyama over the correspondences)
  "GeneralizedIcp"   RegistrationGeneralizedICP with TransformationEstimationForGeneralizedICP(epsilon) (GeneralizedICP.cpp)

Written from Open3D's published source, independently of the library: exact nearest neighbours (cKDTree, eps 0) with the
radius test d2 < r2, Open3D's W = (M^-1)^(1/2) form of the GICP term (the library sums G^T M^-1 G), the source's covariances
turned with the source at init and at every update (PointCloud::Transform -> TransformCovariances), numpy's SVD for umeyama.

`workers` goes to every cKDTree.query (the answers do not depend on it); `bounded` gives each query distance_upper_bound
r (1 + 1e-9), which only prunes candidates the exact d2 < r2 test would drop anyway."""
import numpy as np
from scipy.spatial import cKDTree

TYPES = ("PointToPlaneIcp", "PointToPointIcp", "GeneralizedIcp")


def is_identity(T, prec=1e-12):
    """Eigen isIdentity(prec): |diag - 1| <= prec * min(|diag|, 1), |off-diagonal| <= prec."""
    T = np.asarray(T, np.float64)
    for r in range(4):
        for c in range(4):
            v = T[r, c]
            if r == c:
                if not abs(v - 1.0) <= prec * min(abs(v), 1.0):
                    return False
            elif not abs(v) <= prec:
                return False
    return True


def transform_points(T, p):
    """PointCloud::Transform on the points: (T [p 1]).head<3>() / w."""
    v = p @ T[:3, :3].T + T[:3, 3]
    w = p @ T[3, :3] + T[3, 3]
    return v / w[:, None]


def rotation_e1_to(n):
    """GetRotationFromE1ToX (GeneralizedICP.cpp) for each row of n (as given: not normalised)."""
    n = np.asarray(n, np.float64)
    m = len(n)
    v = np.stack([np.zeros(m), -n[:, 2], n[:, 1]], axis=1)  # e1 x n
    c = n[:, 0]                                               # e1 . n
    sv = np.zeros((m, 3, 3))
    sv[:, 0, 1], sv[:, 0, 2] = -v[:, 2], v[:, 1]
    sv[:, 1, 0], sv[:, 1, 2] = v[:, 2], -v[:, 0]
    sv[:, 2, 0], sv[:, 2, 1] = -v[:, 1], v[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        factor = 1.0 / (1.0 + c)
    R = np.eye(3)[None] + sv + (sv @ sv) * factor[:, None, None]
    R[c < -0.99] = np.eye(3)  # "x and e1 are in the same direction" (the opposite one, in fact): Open3D's branch kept
    return R


def covariances_from_normals(n, epsilon=1e-3):
    """InitializePointCloudForGeneralizedICP for a cloud with normals: C_i = Rx diag(eps, 1, 1) Rx^T."""
    R = rotation_e1_to(n)
    return R @ np.diag([epsilon, 1.0, 1.0])[None] @ np.transpose(R, (0, 2, 1))


def correspondences(pcd, tree, tgt, r, workers=1, bounded=False):
    """GetRegistrationResultAndCorrespondences: (source index, target index) pairs, fitness, inlier_rmse."""
    ns = len(pcd)
    fin = np.isfinite(pcd).all(axis=1)
    src_idx = np.nonzero(fin)[0]
    if bounded:
        _, j = tree.query(pcd[fin], k=1, eps=0.0, distance_upper_bound=r * (1.0 + 1e-9), workers=workers)
        found = j < len(tgt)           # a miss comes back as index len(tgt)
        src_idx, j = src_idx[found], j[found]
    else:
        _, j = tree.query(pcd[fin], k=1, eps=0.0, workers=workers)
    d = pcd[src_idx] - tgt[j]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    hit = d2 < r * r
    src_idx, j, d2 = src_idx[hit], j[hit], d2[hit]
    count = len(src_idx)
    fitness = count / ns if count else 0.0
    rmse = float(np.sqrt(d2.sum() / count)) if count else 0.0
    return src_idx, j, fitness, rmse


def vec6_to_T(x):
    """TransformVector6dToMatrix4d: Rz(x2) Ry(x1) Rx(x0), translation x[3:]."""
    a, b, g = x[:3]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(g), -np.sin(g), 0], [np.sin(g), np.cos(g), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:]
    return T


def solve_jtj(JTJ, JTr, solver=None):
    """SolveJacobianSystemAndObtainExtrinsicMatrix: JTJ x = -JTr (Open3D: Eigen LDLT), then vec6_to_T.  solver(A, b) -> x: what
    solves the system (default np.linalg.solve, which raises on a singular one; tests/o3d_solve_ref.py has Eigen's LDLT)."""
    return vec6_to_T((solver or np.linalg.solve)(JTJ, -JTr))


def skew(v):
    S = np.zeros((len(v), 3, 3))
    S[:, 0, 1], S[:, 0, 2] = -v[:, 2], v[:, 1]
    S[:, 1, 0], S[:, 1, 2] = v[:, 2], -v[:, 0]
    S[:, 2, 0], S[:, 2, 1] = -v[:, 1], v[:, 0]
    return S


def inv_sqrt_spd(M):
    """M^-1.sqrt() (Eigen's MatrixSquareRoot of the inverse) for symmetric positive definite M: the principal square root of M^-1,
    formed from M^-1's eigen decomposition (equal to scipy.linalg.sqrtm(inv(M)); batched)."""
    Mi = np.linalg.inv(M)
    Mi = 0.5 * (Mi + np.transpose(Mi, (0, 2, 1)))
    lam, V = np.linalg.eigh(Mi)
    return (V * np.sqrt(lam)[:, None, :]) @ np.transpose(V, (0, 2, 1))


def update_point_to_plane(pcd, tgt, tn, si, tj, solver=None):
    vs, vt, nt = pcd[si], tgt[tj], tn[tj]
    r = ((vs - vt) * nt).sum(axis=1)
    J = np.concatenate([np.cross(vs, nt), nt], axis=1)
    return solve_jtj(J.T @ J, J.T @ r, solver)


def update_generalized(pcd, tgt, cs, ct, si, tj, solver=None):
    """TransformationEstimationForGeneralizedICP::ComputeTransformation in Open3D's own form: W = (Ct + Cs)^-1.sqrt(),
    J = W [-[vs]x | I], r = W d; JTJ += J^T J, JTr += J^T r over the three rows of every correspondence."""
    vs, vt = pcd[si], tgt[tj]
    d = vs - vt
    W = inv_sqrt_spd(ct[tj] + cs[si])
    G = np.concatenate([-skew(vs), np.broadcast_to(np.eye(3), (len(si), 3, 3))], axis=2)
    J = W @ G                              # n x 3 x 6
    r = (W @ d[:, :, None])[:, :, 0]       # n x 3
    JTJ = np.einsum("nka,nkb->ab", J, J)
    JTr = np.einsum("nka,nk->a", J, r)
    return solve_jtj(JTJ, JTr, solver)


def umeyama(src, dst):
    """Eigen::umeyama(src, dst, with_scaling = false) on row-point arrays."""
    n = len(src)
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    sigma = (dst - md).T @ (src - ms) / n
    U, _, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt.T) < 0:
        S[2] = -1.0
    T = np.eye(4)
    T[:3, :3] = U @ np.diag(S) @ Vt
    T[:3, 3] = md - T[:3, :3] @ ms
    return T


def registration_icp(source, target, max_correspondence_distance, init=None, registration_type="PointToPlaneIcp", target_normals=None,
                     source_normals=None, source_covariances=None, target_covariances=None, epsilon=1e-3, relative_fitness=1e-6,
                     relative_rmse=1e-6, max_iteration=30, workers=1, bounded=False, solver=None):
    """RegistrationICP(source, target, max_dist, init, <estimation>, criteria); GeneralizedIcp: RegistrationGeneralizedICP (the
    covariances of InitializePointCloudForGeneralizedICP first).  Returns the fields of RegistrationResult as a dict.
    solver: see solve_jtj."""
    assert registration_type in TYPES
    src = np.asarray(source, np.float64)
    tgt = np.ascontiguousarray(target, np.float64)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    cs = ct = None
    if registration_type == "GeneralizedIcp":
        cs = (np.asarray(source_covariances, np.float64).reshape(-1, 3, 3).copy() if source_covariances is not None
              else covariances_from_normals(source_normals, epsilon))
        ct = (np.asarray(target_covariances, np.float64).reshape(-1, 3, 3) if target_covariances is not None
              else covariances_from_normals(target_normals, epsilon))
    tn = None if target_normals is None else np.asarray(target_normals, np.float64)
    pcd = src.copy()
    if not is_identity(T):
        pcd = transform_points(T, pcd)
        if cs is not None:
            R = T[:3, :3]
            cs = R[None] @ cs @ R.T[None]
    tree = cKDTree(tgt)
    r = float(max_correspondence_distance)
    si, tj, fitness, rmse = correspondences(pcd, tree, tgt, r, workers, bounded)
    it = 0
    for _ in range(int(max_iteration)):
        if len(si) == 0:
            update = np.eye(4)
        elif registration_type == "PointToPlaneIcp":
            update = update_point_to_plane(pcd, tgt, tn, si, tj, solver)
        elif registration_type == "PointToPointIcp":
            update = umeyama(pcd[si], tgt[tj])
        else:
            update = update_generalized(pcd, tgt, cs, ct, si, tj, solver)
        T = update @ T
        pcd = transform_points(update, pcd)
        if cs is not None:
            R = update[:3, :3]
            cs = R[None] @ cs @ R.T[None]
        f0, e0 = fitness, rmse
        si, tj, fitness, rmse = correspondences(pcd, tree, tgt, r, workers, bounded)
        it += 1
        if abs(f0 - fitness) < relative_fitness and abs(e0 - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fitness, "inlier_rmse": rmse, "correspondences": len(si), "iterations": it}


def information_matrix(source, target, max_correspondence_distance, transformation, workers=1, bounded=False):
    """GetInformationMatrixFromPointClouds (pipelines/registration/Registration.cpp): the source placed by T, its nearest target
    point within the radius, and for each correspondence the three rows G = [[0, z, -y, 1, 0, 0], [-z, 0, x, 0, 1, 0],
    [y, -x, 0, 0, 0, 1]] of the TARGET point (x, y, z); returns the 6 x 6 sum of G^T G."""
    src = np.asarray(source, np.float64)
    tgt = np.ascontiguousarray(target, np.float64)
    T = np.asarray(transformation, np.float64)
    pcd = src if is_identity(T) else transform_points(T, src)
    _, tj, _, _ = correspondences(pcd, cKDTree(tgt), tgt, float(max_correspondence_distance), workers, bounded)
    x, y, z = tgt[tj, 0], tgt[tj, 1], tgt[tj, 2]
    n = len(tj)
    G = np.zeros((n, 3, 6))
    G[:, 0, 1], G[:, 0, 2], G[:, 0, 3] = z, -y, 1.0
    G[:, 1, 0], G[:, 1, 2], G[:, 1, 4] = -z, x, 1.0
    G[:, 2, 0], G[:, 2, 1], G[:, 2, 5] = y, -x, 1.0
    return np.einsum("nka,nkb->ab", G, G)
