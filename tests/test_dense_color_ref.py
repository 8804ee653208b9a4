"""tests/dense_color_ref.py against answers worked out by hand from the reference's source (croppers.cpp:178-244, helpers.cpp:283-318,
Voxel.cpp:18-114, Voxel.hpp:47-50), and — for everything but colour — bit for bit against the oracle's DenseMap.  CPU only."""
import numpy as np

import dense_color_ref as ref
from oracle import oracle as orc


def test_one_white_point_has_colour_two():
    """Voxel.hpp:50: the colour sum starts at (1, 1, 1); one point of colour (1, 1, 1) -> sum (2, 2, 2) / 1."""
    m = ref.DenseColorMap(0.5)
    m.insert([[0.1, 0.1, 0.1]], None, [[1.0, 1.0, 1.0]])
    p, n, c, k, cnt = m.to_point_cloud()
    assert m.has_colors and n is None and k.tolist() == [[0, 0, 0]] and cnt.tolist() == [1]
    assert c.tolist() == [[2.0, 2.0, 2.0]]
    m.insert([[0.2, 0.1, 0.1]], None, [[0.5, 0.0, 0.25]])            # (1 + 1 + 0.5, 1 + 1 + 0, 1 + 1 + 0.25) / 2
    assert m.to_point_cloud()[2].tolist() == [[1.25, 1.0, 1.125]]


def test_dilution_sticky_flag_and_voxels_that_never_saw_a_colour():
    m = ref.DenseColorMap(1.0)
    m.insert([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5]])                                  # colourless: no flag, nothing to report
    assert not m.has_colors and m.to_point_cloud()[2] is None
    m.insert([[0.25, 0.5, 0.5]], None, [[0.5, 0.25, 0.0]])                        # voxel 0: two points, one colour
    assert m.has_colors
    p, n, c, k, cnt = m.to_point_cloud()
    assert k.tolist() == [[0, 0, 0], [3, 0, 0]] and cnt.tolist() == [2, 1]
    assert c.tolist() == [[1.5 / 2, 1.25 / 2, 1.0 / 2], [1.0, 1.0, 1.0]]          # voxel 3 never saw a colour: (1, 1, 1) / 1
    m.insert([[0.75, 0.5, 0.5], [3.25, 0.5, 0.5]])                                # colourless again: dilutes, flag stays
    p, n, c, k, cnt = m.to_point_cloud()
    assert m.has_colors and cnt.tolist() == [3, 2]
    assert c.tolist() == [[1.5 / 3, 1.25 / 3, 1.0 / 3], [0.5, 0.5, 0.5]]
    # a colour array of another length is no colour at all (Open3D's HasColors: colors_.size() == points_.size())
    m.insert([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5]], None, [[1.0, 1.0, 1.0]])
    assert m.to_point_cloud()[2][0].tolist() == [1.5 / 5, 1.25 / 5, 1.0 / 5]
    # removeKey destroys the voxel: the cell starts from (1, 1, 1) again; clear() keeps the flags
    m.remove_keys([(0, 0, 0)])
    m.insert([[0.5, 0.5, 0.5]], None, [[0.0, 0.0, 0.5]])
    assert m.to_point_cloud()[2][0].tolist() == [1.0, 1.0, 1.5]
    m.clear()
    m.insert([[0.5, 0.5, 0.5]])
    assert m.has_colors and m.to_point_cloud()[2].tolist() == [[1.0, 1.0, 1.0]]


def test_order_of_the_colour_additions():
    """((1 + 1e16) + 1) - 1e16 = 0 in fp64 (1e16 + 1 rounds to 1e16, twice); any other order gives another number."""
    m = ref.DenseColorMap(1.0)
    m.insert([[0.5, 0.5, 0.5]] * 3, None, [[1e16, 0, 0], [1.0, 0, 0], [-1e16, 0, 0]])
    assert m.to_point_cloud()[2][0, 0] == 0.0 / 3
    m = ref.DenseColorMap(1.0)
    m.insert([[0.5, 0.5, 0.5]] * 3, None, [[1e16, 0, 0], [-1e16, 0, 0], [1.0, 0, 0]])
    assert m.to_point_cloud()[2][0, 0] == 1.0 / 3


def test_colour_range_is_inclusive_and_nan_fails():
    up, dn = np.nextafter(1.0, 2.0), np.nextafter(0.0, -1.0)
    col = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 1.0, 0.5], [up, 0.5, 0.5], [0.5, dn, 0.5], [0.5, 0.5, np.nan], [0.5, 0.5, 0.5]])
    pts = np.arange(21.0).reshape(7, 3)
    nrm, cov = pts + 100.0, np.arange(63.0).reshape(7, 9)
    p, n, c, v = ref.color_range_crop(pts, nrm, col, cov)
    keep = [0, 1, 2, 6]
    assert np.array_equal(p, pts[keep]) and np.array_equal(n, nrm[keep]) and np.array_equal(c, col[keep]) and np.array_equal(v, cov[keep])
    p, n, c, v = ref.color_range_crop(pts, None, col, None, rgb_min=[0.5, 0.5, 0.5], rgb_max=[0.5, 0.5, 0.5])
    assert np.array_equal(p, pts[[6]]) and n is None and v is None
    p, n, c, v = ref.color_range_crop(pts, nrm, None, cov, rgb_min=[2, 2, 2])       # no colours: unchanged, whatever the bounds
    assert np.array_equal(p, pts) and n is nrm and c is None and v is cov
    assert ref.color_range_crop(np.zeros((0, 3)), None, np.zeros((0, 3)))[0].shape == (0, 3)


def test_near_identity_pose_doubles_points_and_drops_the_colours():
    pts = np.array([[0.25, 0.5, 0.5], [1.5, 0.5, 0.5]])
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    col = np.array([[0.5, 0.5, 0.5], [0.25, 0.25, 0.25]])
    T = np.eye(4)
    T[0, 3] = 5e-5                                                    # max |T - I| < 1e-4
    assert ref.is_near_identity(T)
    tp, tn, tc = ref.transform_cloud(T, pts, nrm, col)
    assert tp.shape == (4, 3) and tn.shape == (4, 3) and tc.shape == (2, 3)
    assert np.array_equal(tp[:2], pts) and tp[2].tolist() == [0.25 + 5e-5, 0.5, 0.5] and np.array_equal(tn[2:], nrm)
    m = ref.DenseColorMap(1.0)
    assert m.insert_scan(pts, nrm, col, T, [True, True], carve_every=2) is False      # scan 0: 0 % 2 != 1
    assert not m.has_colors and m.has_normals and m.n_scans_inserted == 1
    p, n, c, k, cnt = m.to_point_cloud()
    assert c is None and cnt.tolist() == [2, 2] and n[0].tolist() == [0.0, 0.0, 1.0]
    T[0, 3] = 1e-4                                                    # not below 1e-4: an ordinary pose, colours ride along 1:1
    assert not ref.is_near_identity(T)
    assert m.insert_scan(pts, nrm, col, T, [True, False], carve_every=2) is True      # scan 1: the gate fires
    p, n, c, k, cnt = m.to_point_cloud()
    assert m.has_colors and cnt.tolist() == [3, 2] and c.tolist() == [[1.5 / 3] * 3, [0.5] * 3]
    # a scan rejected entirely by colour inserts nothing and still counts
    assert m.insert_scan(pts, nrm, col + 2.0, T, [True, True], carve_every=2) is False
    assert m.n_scans_inserted == 3 and m.to_point_cloud()[4].tolist() == [3, 2]


def test_everything_but_colour_equals_the_oracle_bit_for_bit():
    rng = np.random.default_rng(11)
    voxel = 0.3
    m, om = ref.DenseColorMap(voxel), orc.DenseMap(voxel)
    T = np.eye(4)
    c, s = np.cos(0.4), np.sin(0.4)
    T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [0.3, -0.2, 0.1]
    for k, pose in enumerate([T, np.eye(4), T]):
        p = rng.uniform(-3.0, 3.0, (4000, 3))
        n = rng.normal(size=(4000, 3))
        col = rng.uniform(-0.1, 1.1, (4000, 3))
        mask = ref.max_radius_mask(p, 2.5)
        assert np.array_equal(mask, orc.crop_mask(orc.make_cropper("MaxRadius", 2.5), p)) and 0 < mask.sum() < 4000
        kp, kn, kc, _ = ref.color_range_crop(p[mask], n[mask], col[mask])
        tp, tn, tc = ref.transform_cloud(pose, kp, kn, kc)
        op, on = orc.transform_cloud(pose, kp, kn)
        assert np.array_equal(tp, op) and np.array_equal(tn, on) and len(tp) == (2 if k == 1 else 1) * len(kp)
        m.insert_scan(p, n if k else None, col, pose, mask)
        om.insert(op, on if k else None)
        P, N, C_, K, cnt = m.to_point_cloud()
        oP, oN, oK, ocnt = om.to_point_cloud()
        assert np.array_equal(K, oK) and np.array_equal(cnt, ocnt) and np.array_equal(P, oP)
        assert (N is None) == (oN is None) and (N is None or np.array_equal(N, oN))
    assert m.has_colors and m.size() == om.size() > 1000
    m.transform(T)
    om.transform(T)
    before = m.to_point_cloud()[2].copy()
    P, N, C_, K, cnt = m.to_point_cloud()
    oP, oN, oK, ocnt = om.to_point_cloud()
    assert np.array_equal(P, oP) and np.array_equal(N, oN) and np.array_equal(K, oK) and np.array_equal(C_, before)
