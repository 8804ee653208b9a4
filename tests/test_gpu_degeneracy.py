"""The degeneracy-aware ICP step (include/degeneracy/o3s_degeneracy.h) on the GPU against the numpy restatement
(tests/degeneracy_ref.py).  MI355X only.

Bounds, from the contract and the number formats:
  A', b'    |delta| <= 64 * 2^-24 * max|A| against the restated projection (fp64) of the device's own unconstrained A, b (o3s_icp_minimize):
            the outputs are fp32 and each entry combines at most 36 entries with coefficients <= 1.  b' is also held to the same
            multiple of max|b| (it combines six entries of b).
  x         bit-equal to orc.solve6 on the device's own A', b' (the rule of tests/test_gpu_solver_branches.py).
  C x = 0   |e . x| <= 8 x the restatement's own leakage (solve6 on the restated A', b'), floor 4 * 2^-24 |x|.
  chain     pose within the 1e-4 m / 1e-4 rad tests/test_gpu_parity.py allows between chain and oracle, given that in every iteration
            the restatement's sums stay 10 % away from each threshold (asserted on the restatement alone).
The normal equations have at most kMaxPartialBlocks = 512 block partials: the size that would give 513 runs with the clamp's 512.
Comparisons between two ways of issuing the same chain are bit for bit."""
import functools

import numpy as np
import pytest

import degeneracy_ref as dref
import localizability_ref as lref
import solve_ref as sr
from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig, _lib
from open3d_slam_advanced_rss_2024_public_amd import localizability as loc
from open3d_slam_advanced_rss_2024_public_amd.icp import compute_batch
from test_gpu_localizability import ONE_BLOCK, assert_same_snapshot, params_of, same_bits, snapshot
from test_gpu_parity import assert_pose_close

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
COV = "PointToPlaneWithCovErrorMinimizer"
ITERS = 6
FIXED_CHAIN = dict(use_differential=False, max_iters=ITERS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_result(a, b):
    """Two snapshots without the traces: compute_batch leaves them on the device."""
    assert np.array_equal(a["T"], b["T"]) and np.array_equal(a["cov"], b["cov"], equal_nan=True) and a["scalars"] == b["scalars"]


def basis(seed, n):
    """n orthonormal directions (to the last bits of fp64: a QR of a seeded matrix)."""
    q = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))[0]
    return q.T[:n].copy()


# ---- 1. the module-level entry ------------------------------------------------------------------------------------------------------------
NB_SIZES = [(1, ONE_BLOCK - 3), (2, ONE_BLOCK + 1), (256, 256 * ONE_BLOCK), (257, 256 * ONE_BLOCK + 1), (513, 512 * ONE_BLOCK + 1)]
SETS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 3), (3, 2), (3, 3)]


@functools.lru_cache(maxsize=None)
def minimize_case(kind, n):
    """A handle with the scene's reference, the minimize inputs (every seventh weight 0) and the unconstrained result."""
    scene = (sr.generic if kind == "generic" else sr.corridor)(n)
    g = ICP(IcpConfig(**sr.FLAT))
    assert g.init_reference(scene[0], scene[1])
    q, ids, d2, w = sr.minimize_inputs(scene, g.reference_mean())
    w = w.copy()
    w[::7] = 0.0
    inputs = (q, ids, d2, w)
    return g, inputs, g.minimize(*inputs)


@pytest.mark.parametrize("nb,n", NB_SIZES)
@pytest.mark.parametrize("kind", ["generic", "corridor"])
def test_minimize_degeneracy_matches_the_restated_projection(kind, nb, n):
    g, inputs, (T0, A0, b0, x0) = minimize_case(kind, n)
    tolA = 64 * EPS32 * np.abs(A0).max()
    tolb = 64 * EPS32 * min(np.abs(A0).max(), np.abs(b0).max())
    for k, (n_rot, n_trans) in enumerate(SETS):
        rot, trans = basis(100 * nb + k, n_rot), basis(200 * nb + k, n_trans)
        if kind == "corridor" and n_trans == 1:
            trans = np.array([[1.0, 0.0, 0.0]])                   # the axis nothing sees: the constraint the feature is for
        T, A, b, x = g.minimize_degeneracy(*inputs, loc.DegeneracySet(rot, trans))
        if n_rot + n_trans == 0:                                  # the empty set: o3s_icp_minimize's bits
            for got, want in ((T, T0), (A, A0), (b, b0), (x, x0)):
                assert np.array_equal(bits(got), bits(want))
            continue
        Ar, br = dref.project(A0, b0, rot, trans)
        dA, db = np.abs(A - Ar).max(), np.abs(b - br).max()
        x6, _ = orc.solve6(A, b)
        xr, _ = orc.solve6(Ar.astype(np.float32), br.astype(np.float32))
        leak, leak_ref = dref.leakage(x, rot, trans), dref.leakage(xr, rot, trans)
        bound = max(8.0 * leak_ref, 4 * EPS32 * float(np.linalg.norm(x)))
        print(f"{kind} nb {nb} N {n} set {n_rot}+{n_trans}: |dA| {dA:.3e} (tol {tolA:.3e})  |db| {db:.3e} (tol {tolb:.3e})  "
              f"leak {leak:.3e} (restatement {leak_ref:.3e}, bound {bound:.3e})")
        assert np.array_equal(bits(A), bits(A.T))
        assert dA <= tolA and db <= tolb
        assert np.array_equal(bits(x), bits(x6)), (x, x6)
        assert leak <= bound
        again = g.minimize_degeneracy(*inputs, loc.DegeneracySet(rot, trans))
        assert all(np.array_equal(bits(u), bits(v)) for u, v in zip((T, A, b, x), again))


def test_minimize_degeneracy_refuses_a_bad_set_with_the_handle():
    g, inputs, _ = minimize_case("generic", ONE_BLOCK - 3)
    with pytest.raises(ValueError) as e:
        g.minimize_degeneracy(*inputs, loc.DegeneracySet(trans=np.array([[1.0, 0, 0], [0.6, 0.8, 0]])))
    assert f"[{_lib.ERR_BAD_ARGUMENT}]" in str(e.value)


# ---- the scenes of the chain tests -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated(scene, min_category=2):
    """The scene's pair, thresholds from the restatement's first iteration, and the restated constrained chain of ITERS iterations."""
    pair = lref.scan_pair(scene)
    M, Mn, S, Sn, T_true, T_init = pair
    o = orc.OracleIcp(orc.OracleConfig(use_differential=False, max_iters=ITERS), threads=8)
    assert o.init_reference(M, Mn) == orc.OK
    first = dref.constrained_chain(orc, o, M, Mn, S, Sn, T_init, 1, ks=(1.0, 1.0, 1.0))["analyses"][0]
    k1, k2, k3, free = lref.thresholds(scene, first)
    ks = (k1, k2, k3)
    ref = dref.constrained_chain(orc, o, M, Mn, S, Sn, T_init, ITERS, ks=ks, min_category=min_category)
    return pair, ks, free, ref


def new_handle(pair, **cfg):
    g = ICP(IcpConfig(**cfg))
    assert g.init_reference(pair[0], pair[1])
    g.set_reading(pair[2], pair[3])
    return g


# ---- 2. an empty set changes nothing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fixed_empty", "analyse_room"])
def test_an_empty_set_gives_the_bits_of_off(mode):
    pair, ks, free, ref = restated("room")
    assert not free.any() and ref["masks"] == [0] * ITERS
    T_init = pair[5]
    cfg = dict(error_minimizer=COV, **FIXED_CHAIN)
    off, on = new_handle(pair, **cfg), new_handle(pair, **cfg)

    def arm(g):
        if mode == "fixed_empty":
            g.set_degeneracy(loc.DEGENERACY_FIXED, fixed_set=loc.DegeneracySet())
        else:
            g.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks))

    arm(on)
    want = snapshot(off, off.compute(*pair[2:4], T_init))                       # the eager entry
    assert_same_snapshot(want, snapshot(on, on.compute(*pair[2:4], T_init)))
    assert np.array_equal(on.degeneracy_trace(), np.zeros(ITERS, np.int32)) and len(off.degeneracy_trace()) == 0
    on.set_reading(*pair[2:4])
    for round_ in range(3):                                                      # the graph entry: captured, then replayed
        T = on.compute_resident(T_init)
        assert_same_snapshot(want, snapshot(on, T))
        assert np.array_equal(on.degeneracy_trace(), np.zeros(ITERS, np.int32))
    assert on.host_split_ex()["issued"] == "replayed"
    others = [new_handle(pair, **cfg) for _ in range(2)]                         # o3s_icp_compute_batch
    for h in others:
        arm(h)
    poses, codes, _ = compute_batch(others, [T_init, T_init])
    assert codes == [0, 0]
    for h, T in zip(others, poses):
        assert_same_result(want, snapshot(h, T))
        assert np.array_equal(h.degeneracy_trace(), np.zeros(ITERS, np.int32))
    last = on.last_degeneracy_set()
    assert len(last.rot) == 0 and len(last.trans) == 0


# ---- 3. the constrained chain ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,mask", [("corridor", 0b000001), ("tunnel", 0b001001)])
def test_analyse_mode_constrains_the_free_directions(scene, mask):
    pair, ks, free, ref = restated(scene)
    M, Mn, S, Sn, T_true, T_init = pair
    assert len(S) == 3000 and len(M) == 12000
    # the condition, on the restatement alone: every iteration's sums stay 10 % away from each threshold, and it finds the free ones
    for it, res in enumerate(ref["analyses"]):
        margin = dref.threshold_margins(res, ks)
        print(f"{scene} iteration {it}: margin {margin:.3f}  categories {res['category']}  mask {ref['masks'][it]:06b}")
        assert margin >= 0.10, (it, margin)
        assert np.array_equal(lref.free_mask(scene, res["evec"]), free)
    assert ref["masks"] == [mask] * ITERS and int(sum(1 << j for j in range(6) if free[j])) == mask
    g = new_handle(pair, **FIXED_CHAIN)
    g.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks), min_category=2)
    T = g.compute(S, Sn, T_init)
    assert g.stats.iterations == ITERS
    assert np.array_equal(g.degeneracy_trace(), np.full(ITERS, mask, np.int32))
    # the last iteration's set: what o3s_icp_localizability reports afterwards, bit for bit
    after = g.localizability(params_of(ks))
    low = after.category < 2
    assert int(sum(1 << j for j in range(6) if low[j])) == mask
    last = g.last_degeneracy_set()
    assert np.array_equal(last.trans, after.evec[:3][low[:3]]) and np.array_equal(last.rot, after.evec[3:][low[3:]])
    assert same_bits(after, g.localizability(params_of(ks)))
    dt, ang = orc.pose_error(ref["T"], T)
    off = new_handle(pair, **FIXED_CHAIN).compute(S, Sn, T_init)
    print(f"{scene}: device against the restated constrained chain |dt| {np.linalg.norm(dt):.3e} m  angle {ang:.3e} rad;  "
          f"along the axis: truth {T_true[0, 3]:.4f}  start {T_init[0, 3]:.4f}  constrained {T[0, 3]:.4f}  restated {ref['T'][0, 3]:.4f}  off {off[0, 3]:.4f}")
    assert_pose_close(T, ref["T"])
    assert not np.array_equal(T, off)


# ---- 4. determinism -------------------------------------------------------------------------------------------------------------------------
def test_constrained_computes_are_deterministic_and_batches_equal_single_calls():
    pair, ks, free, ref = restated("corridor")
    T_init = pair[5]
    g = new_handle(pair, error_minimizer=COV, **FIXED_CHAIN)
    g.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks))
    want = snapshot(g, g.compute(*pair[2:4], T_init))
    masks = g.degeneracy_trace()
    assert masks.tolist() == ref["masks"]
    assert_same_snapshot(want, snapshot(g, g.compute(*pair[2:4], T_init)))
    g.set_reading(*pair[2:4])
    for round_ in range(3):                                                      # captured, then replayed
        T = g.compute_resident(T_init)
        assert_same_snapshot(want, snapshot(g, T))
        assert np.array_equal(g.degeneracy_trace(), masks)
    assert g.host_split_ex()["issued"] == "replayed"
    singles = []
    for k in range(4):                                                            # four pairs: four starts
        Tk = lref.make_T([0, 0, 0.001 * k], [0.0, 0.004 * k, 0.0]) @ T_init
        h = new_handle(pair, error_minimizer=COV, **FIXED_CHAIN)
        h.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks))
        singles.append((Tk, snapshot(h, h.compute_resident(Tk)), h.degeneracy_trace()))
    batch = [new_handle(pair, error_minimizer=COV, **FIXED_CHAIN) for _ in range(4)]
    for h in batch:
        h.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks))
    poses, codes, _ = compute_batch(batch, [s[0] for s in singles])
    assert codes == [0] * 4
    for h, T, (_, snap, m) in zip(batch, poses, singles):
        assert_same_result(snap, snapshot(h, T))
        assert np.array_equal(h.degeneracy_trace(), m)


# ---- 5. the sharded mode ----------------------------------------------------------------------------------------------------------------------
def test_a_sharded_handle_refuses_the_constrained_compute():
    pair, ks, free, ref = restated("corridor")
    g = new_handle(pair, **FIXED_CHAIN)
    g.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks))
    g.shard_configure(len(pair[2]), 0, 1, lambda *a: None)
    with pytest.raises(ValueError) as e:
        g.compute(*pair[2:4], pair[5])
    assert f"[{_lib.ERR_BAD_CONFIG}]" in str(e.value) and "sharded" in str(e.value)
    with pytest.raises(ValueError) as e:
        g.set_degeneracy(loc.DEGENERACY_ANALYSE, params=loc.LocalizabilityParams())   # unset thresholds, with a handle
    assert f"[{_lib.ERR_BAD_CONFIG}]" in str(e.value)


# ---- 6. the mode is the handle's, and leaves with it ----------------------------------------------------------------------------------------
def test_off_after_analyse_gives_offs_bits_again():
    pair, ks, free, ref = restated("tunnel")
    T_init = pair[5]
    g = new_handle(pair, error_minimizer=COV, **FIXED_CHAIN)
    off = [snapshot(g, g.compute_resident(T_init)) for _ in range(3)]            # eager, captured, replayed
    assert g.host_split_ex()["issued"] == "replayed"
    g.set_degeneracy(loc.DEGENERACY_ANALYSE, params=params_of(ks))
    on = [snapshot(g, g.compute_resident(T_init)) for _ in range(3)]
    assert g.host_split_ex()["issued"] == "replayed" and g.degeneracy_trace().tolist() == ref["masks"]
    g.set_degeneracy(loc.DEGENERACY_OFF)
    back = [snapshot(g, g.compute_resident(T_init)) for _ in range(3)]
    assert g.host_split_ex()["issued"] == "replayed" and len(g.degeneracy_trace()) == 0
    for s in off[1:] + back:
        assert_same_snapshot(off[0], s)
    for s in on[1:]:
        assert_same_snapshot(on[0], s)
    assert not np.array_equal(on[0]["T"], off[0]["T"])
