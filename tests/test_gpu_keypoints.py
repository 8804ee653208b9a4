"""ISS keypoints on host arrays (o3s_iss_keypoints: k_iss_nn_dist, k_iss_scatter, k_iss_nms in csrc/keypoints_dev.h) against
tests/iss_ref.py.  MI355X only.

Contract of every case: the keypoint set equals the reference's exactly — the fragile set of every cloud used here is empty
(tests/test_iss_ref.py asserts it for the two large ones without a GPU; it is asserted again here, for all) —,
|sal_dev - sal_ref| <= B_i = (3 n_i + 64) 2^-52 trace(S_i) for every point (derived in iss_ref.py, not measured), sal_dev == 0
exactly where the reference's is 0, the output is the input restricted to the indices, normals with it, bit for bit, and a second
call gives the same bits."""
import numpy as np
import pytest

import iss_ref as R
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from test_gpu_outlier_removal import _with_cell_cap, cloud, normals_for, same_bits, spacing

pytestmark = pytest.mark.gpu

BLOCK = 256   # kB of csrc/cloud_dev.h
EDGE_SIZES = (1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1)


def check(label, p, rs, rn, gamma, ref=None, min_nb=5):
    """-> (ref, (points, normals, indices, saliency, radii) of the device)"""
    nrm = normals_for(p)
    if ref is None:
        ref = R.iss(p, rs, rn, gamma, gamma, min_nb)
    assert not ref["fragile"].any(), f"the input {label} was chosen badly: fragile points {np.flatnonzero(ref['fragile'])[:10]}"
    out = co.compute_iss_keypoints(p, rs, rn, gamma, gamma, min_nb, normals=nrm)
    op, on, idx, sal, radii = out
    if rs != 0.0 and rn != 0.0:
        assert (radii == np.array([rs, rn])).all()
    err = np.abs(sal - ref["sal"])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(ref["B"] > 0.0, err / ref["B"], 0.0))) if len(p) else 0.0
    print(f"{label} gamma {gamma}: {len(idx)} keypoints (reference {int(ref['flag'].sum())}), worst |sal_dev - sal_ref| / B = {worst:.3g}")
    got = np.zeros(len(p), bool)
    got[idx] = True
    assert (got == ref["flag"]).all(), (label, np.flatnonzero(got != ref["flag"])[:10])
    assert (np.diff(idx) > 0).all()
    zero = ref["sal"] == 0.0
    assert (sal[zero] == 0.0).all() and (sal[~zero] != 0.0).all()
    assert (err <= ref["B"]).all(), (label, np.flatnonzero(err > ref["B"])[:10], worst)
    assert same_bits(op, p[idx]), "kept points: not the input restricted to the indices, in order"
    assert same_bits(on, nrm[idx]), "normals did not follow their points"
    again = co.compute_iss_keypoints(p, rs, rn, gamma, gamma, min_nb, normals=nrm)
    for a, b in zip(out, again):
        assert same_bits(a, b)
    return ref, out


@pytest.mark.parametrize("N", sorted(R.SHEETS))
@pytest.mark.parametrize("gamma", R.GAMMAS)
def test_sheet(N, gamma):
    rs, rn = R.SHEETS[N]
    check(f"sheet({N})", R.sheet(N), rs, rn, gamma, ref=R.sheet_ref(N, gamma))


@pytest.mark.parametrize("N", EDGE_SIZES)
def test_block_and_wave_edges(N):
    s = spacing(N)
    ref, _ = check(f"sheet({N})", cloud(N), 3.0 * s, 2.0 * s, 0.975)
    assert N < 63 or ref["flag"].any()


def _five(ex):
    return np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.25], [ex, 0.0, 0.0]])


def test_strict_radius():
    """dyadic coordinates: the query (point 0) has min_neighbors - 1 points strictly inside the radius 1 and one at d2 == r^2
    exactly — not a neighbour; one ulp further in it is one.  First for the salient count, then for the non-max count."""
    inside = np.nextafter(1.0, 0.0)
    for rs, rn in ((1.0, 1.0), (2.0, 1.0)):
        on_edge, moved = _five(1.0), _five(inside)
        ra, rb = R.iss(on_edge, rs, rn, 0.975, 0.975, 5), R.iss(moved, rs, rn, 0.975, 0.975, 5)
        assert not ra["flag"][0] and rb["flag"][0]   # the construction
        assert (ra["sal"][0] == 0.0) == (rs == 1.0) and rb["sal"][0] > 0.0
        for p, ref in ((on_edge, ra), (moved, rb)):
            _, _, idx, sal, _ = co.compute_iss_keypoints(p, rs, rn, 0.975, 0.975, 5)
            assert (sal[0] == 0.0) == (ref["sal"][0] == 0.0) and abs(sal[0] - ref["sal"][0]) <= ref["B"][0]
            assert (0 in idx) == bool(ref["flag"][0])
            assert ((sal == 0.0) == (ref["sal"] == 0.0)).all()


def test_ties_of_coincident_points():
    p = cloud(2000)
    rs, rn = R.SHEETS[2000]
    keys = np.flatnonzero(R.sheet_ref(2000, 0.975)["flag"])[:25]
    src = np.concatenate([keys, np.arange(300, 325)])
    q = np.concatenate([p, p[src]])
    _, (op, on, idx, sal, _) = check("duplicates", q, rs, rn, 0.975)
    got = np.zeros(len(q), bool)
    got[idx] = True
    dup = np.arange(len(p), len(q))
    assert same_bits(sal[dup], sal[src]) and (got[dup] == got[src]).all()
    assert got[dup].any()   # ties keep both


def test_non_finite_points():
    p = cloud(2000)
    rng = np.random.default_rng(3)
    bad = rng.choice(len(p), 40, replace=False)
    p[bad, rng.integers(0, 3, 40)] = rng.choice([np.nan, np.inf, -np.inf], 40)
    rs, rn = R.SHEETS[2000]
    fin = np.isfinite(p).all(axis=1)
    sub = R.iss(p[fin], rs, rn, 0.975, 0.975, 5)
    ref, (op, on, idx, sal, _) = check("non-finite", p, rs, rn, 0.975)
    assert fin[idx].all() and (sal[~fin] == 0.0).all()
    assert (ref["flag"][fin] == sub["flag"]).all() and same_bits(ref["sal"][fin], sub["sal"])   # the reference on the finite subset, mapped back


def test_spread_and_lowered_cell_cap():
    p = cloud(2000)
    rs, rn = R.SHEETS[2000]
    q = np.concatenate([p, np.array([[2000.0, 0.0, 0.0], [0.0, -2000.0, 5.0], [1500.0, 1500.0, -3.0]])])
    ref, (op, on, idx, sal, _) = check("strays", q, rs, rn, 0.975)
    assert (idx < len(p)).all()
    nrm = normals_for(q)
    (op2, on2, idx2, sal2, _), recs = _with_cell_cap(512, lambda: co.compute_iss_keypoints(q, rs, rn, 0.975, 0.975, 5, normals=nrm))
    assert recs and recs[-1]["cap_steps"] > 0 and np.prod(recs[-1]["dims"]) <= 512, recs
    assert same_bits(idx, idx2) and same_bits(op, op2) and same_bits(on, on2)
    assert (np.abs(sal2 - ref["sal"]) <= ref["B"]).all() and ((sal2 == 0.0) == (ref["sal"] == 0.0)).all()


def test_shuffled_input_order():
    p = cloud(2000)
    rs, rn = R.SHEETS[2000]
    perm = np.random.default_rng(8).permutation(len(p))
    a = co.compute_iss_keypoints(p, rs, rn)[0]
    b = co.compute_iss_keypoints(p[perm], rs, rn)[0]
    assert same_bits(a[np.lexsort(a.T)], b[np.lexsort(b.T)])
    assert (R.sheet_ref(2000, 0.975)["flag"].sum()) == len(a)


@pytest.mark.parametrize("N", (2, 65, 2000))
def test_radii_from_the_resolution(N):
    p = cloud(N)
    res = R.resolution(p)
    op, on, idx, sal, radii = co.compute_iss_keypoints(p, 0.0, 0.0)
    print(f"sheet({N}): resolution {res!r}, radii {radii!r}")
    for got, want in zip(radii, (6.0 * res, 4.0 * res)):
        assert abs(got - want) <= N * R.U * want
    for rs, rn in ((0.0, 0.0), (0.0, 0.7), (0.7, 0.0)):   # one radius 0 replaces both
        assert same_bits(co.compute_iss_keypoints(p, rs, rn)[4], radii)
    ref, out = check(f"sheet({N}) at the returned radii", p, float(radii[0]), float(radii[1]), 0.975)
    assert same_bits(out[2], idx) and same_bits(out[3], sal)


def test_fewer_than_two_finite_points():
    p = np.array([[1.0, 2.0, 3.0], [np.nan, 0.0, 0.0]])
    op, on, idx, sal, radii = co.compute_iss_keypoints(p)
    assert len(idx) == 0 and (sal == 0.0).all() and (radii == 0.0).all()
    op, on, idx, sal, radii = co.compute_iss_keypoints(np.full((3, 3), np.inf), 0.5, 0.5)
    assert len(idx) == 0 and (sal == 0.0).all()
