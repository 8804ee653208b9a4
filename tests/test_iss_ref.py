"""CPU-only checks of tests/iss_ref.py, the numpy restatement of include/keypoints/o3s_keypoints.h: against a brute-force O(N^2)
restatement, on known answers, and — what tests/test_gpu_keypoints.py relies on — that the fragile set of the GPU test's clouds is
empty, so that a change of cloud cannot hide a failure behind exclusions."""
import numpy as np
import pytest

import iss_ref as R


def test_reference_against_brute_force():
    p = R.sheet(300)
    p[17] = np.nan
    p[200, 1] = np.inf
    for rs, rn, g in ((1.6, 1.1, 0.975), (1.1, 1.6, 0.8)):
        ref = R.iss(p, rs, rn, g, g, 5)
        slow = R.iss(p, rs, rn, g, g, 5, use_tree=False)
        sal, flag = R.iss_brute(p, rs, rn, g, g, 5)
        assert not ref["fragile"].any() and ref["flag"].sum() > 0
        for k in ("n", "n_nm", "sal", "flag", "B", "trace"):
            assert (ref[k] == slow[k]).all(), k   # the candidate sets do not show
        assert (ref["flag"] == flag).all()
        assert ((ref["sal"] == 0.0) == (sal == 0.0)).all()
        assert (np.abs(ref["sal"] - sal) <= ref["B"]).all()
        assert ref["sal"][17] == 0.0 and ref["sal"][200] == 0.0 and not ref["flag"][[17, 200]].any()


def test_resolution_against_brute_force():
    p = R.sheet(300)
    p[5] = p[6]   # coincident points: the nearest other point is at 0
    p[9, 2] = np.nan
    a, b = R.resolution(p), R.resolution(p, use_tree=False)
    assert a == b and a > 0.0
    assert R.resolution(p[:1]) == 0.0 and R.resolution(np.full((3, 3), np.nan)) == 0.0
    ref = R.iss(p, 0.0, 1.0)   # one radius 0: both are replaced
    assert (ref["radii"] == np.array([6.0 * a, 4.0 * a])).all()


def _plane(rng, n, origin, u, v, noise):
    a, b = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    w = np.cross(u, v)
    return origin + a[:, None] * u + b[:, None] * v + noise * rng.normal(size=n)[:, None] * w


def test_corner_of_three_planes_is_the_keypoint():
    """one isolated corner of three noisy planes, the radii as large as the faces: only at the corner do the neighbours spread in
    all three directions, so the saliency peaks there, and one non-max radius holds the whole neighbourhood of the peak"""
    rng = np.random.default_rng(5)
    e = np.eye(3)
    o = np.zeros(3)
    p = np.concatenate([_plane(rng, 400, o, e[0], e[1], 0.002), _plane(rng, 400, o, e[1], e[2], 0.002), _plane(rng, 400, o, e[0], e[2], 0.002)])
    rs, rn = 0.5, 0.5
    ref = R.iss(p, rs, rn, 0.975, 0.975, 5)
    best = int(np.argmax(ref["sal"]))
    assert ref["flag"][best]
    assert np.linalg.norm(p[best]) < rn
    near = np.linalg.norm(p, axis=1) < rn
    assert ref["flag"][near].sum() == 1   # the single keypoint within a non-max radius of the corner


def test_plane_alone_has_no_keypoints():
    rng = np.random.default_rng(6)
    p = _plane(rng, 1500, np.zeros(3), np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), 0.002)
    inner = (np.abs(p[:, 0] - 0.5) < 0.3) & (np.abs(p[:, 1] - 0.5) < 0.3)
    ref = R.iss(p, 0.2, 0.15, 0.5, 0.5, 5)
    assert not ref["flag"][inner].any() and (ref["sal"][inner] == 0.0).all()   # l2 / l1 of a disc is near 1


@pytest.mark.parametrize("N", sorted(R.SHEETS))
@pytest.mark.parametrize("gamma", R.GAMMAS)
def test_fragile_set_of_the_gpu_clouds_is_empty(N, gamma):
    ref = R.sheet_ref(N, gamma)
    print(f"sheet({N}) radii {R.SHEETS[N]} gamma {gamma}: {int(ref['flag'].sum())} keypoints, closest ratio margin {ref['margin_ratio']:.3g}, "
          f"closest non-max tie {ref['margin_tie']:.3g} (relative), neighbours {ref['n'].min()} .. {ref['n'].max()}")
    assert not ref["fragile"].any(), np.flatnonzero(ref["fragile"])[:10]
    assert ref["flag"].sum() > 100
    assert ref["margin_ratio"] > 1e-7 and ref["margin_tie"] > 1e-8   # against B of order 1e-13 of the trace
    if N == 20000:
        assert ref["n"].max() > 100   # more than one walk batch per row
