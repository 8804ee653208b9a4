"""A short randomised GPU-vs-oracle campaign inside the test-suite (the long one is tools/fuzz_parity.py): random pair
sizes, voxel sizes, initial offsets and chain configurations.  Every case must be bit-identical to the oracle in status,
iteration count, per-iteration kept counts and trim limits, or differ from it only by the fp32-ulp drift that a
different fp64 summation order can cause (limits equal to 1e-5 relative); poses within 1e-5 m / 1e-5 rad."""
import numpy as np
import pytest

from oracle import oracle as orc
from open3d_slam_advanced_rss_2024_public_amd import ICP, IcpConfig
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def test_random_configurations_agree_with_the_oracle():
    rng = np.random.default_rng(20240807)
    exact = drift = errors = 0
    for case in range(40):
        N = int(rng.integers(200, 5000))
        M = int(rng.integers(2000, 40000))
        voxel = float(rng.choice([0.05, 0.1, 0.2]))
        sp = syn.make_scan_pair(N, M, voxel, seed=int(rng.integers(0, 10**6)), trans=float(rng.uniform(0, 0.3)), rot_deg=float(rng.uniform(0, 6)))
        kw = dict(max_dist=float(rng.choice([0.1, 0.3, 0.5, 1.0, np.inf])), trim_ratio=float(rng.choice([-1.0, 0.5, 0.9, 1.0])),
                  max_normal_angle=float(rng.choice([-1.0, 0.5, 1.57])), use_differential=bool(rng.integers(0, 2)),
                  max_iters=int(rng.integers(1, 20)), smooth_length=int(rng.integers(0, 5)), counter_first=bool(rng.integers(0, 2)))
        gkw = dict(kw)
        for k in ("trim_ratio", "max_normal_angle"):
            if gkw[k] < 0:
                gkw[k] = None
        gkw.update(grid_cell=float(rng.choice([0.0, 0.0, 0.07, 0.31])), sort_queries=bool(rng.integers(0, 2)), use_graph=bool(rng.integers(0, 2)))
        scan = sp.scan_xyz.copy()
        if rng.random() < 0.15 and np.isfinite(kw["max_dist"]):   # with an unbounded matcher this input makes the run chaotic
            scan[: N // 3] += 50.0
        normals = sp.scan_normals if rng.random() < 0.85 else None
        g = ICP(IcpConfig(**gkw))
        o = orc.OracleIcp(orc.OracleConfig(**kw), threads=8)
        assert g.init_reference(sp.map_xyz, sp.map_normals) and o.init_reference(sp.map_xyz, sp.map_normals) == orc.OK
        eg = None
        try:
            Tg = g.compute(scan, normals, sp.T_init)
        except Exception as e:  # noqa: BLE001
            eg = type(e).__name__
        To, code = o.compute(scan, normals, sp.T_init, raise_on_error=False)
        ctx = (case, N, M, gkw)
        assert (eg is None) == (code == orc.OK), ctx
        if eg is not None:
            errors += 1
            continue
        assert g.stats.iterations == o.stats.iterations, ctx
        n = g.stats.iterations
        assert np.array_equal(g.stats.trace_kept[:n], o.trace_kept[:n]), ctx
        gl, ol = g.stats.trace_limit[:n], o.trace_limit[:n]
        dt, ang = orc.pose_error(To, Tg)
        assert np.linalg.norm(dt) <= 1e-5 and ang <= 1e-5, ctx
        if np.array_equal(gl, ol, equal_nan=True):
            exact += 1
        else:
            fin = np.isfinite(ol)
            assert np.array_equal(np.isfinite(gl), fin) and np.all(np.abs(gl[fin] - ol[fin]) <= 1e-5 * np.abs(ol[fin])), ctx
            drift += 1
        g.close()
    assert exact >= 30 and exact + drift + errors == 40


def test_random_dense_map_histories_agree_with_the_oracle():
    """Random sequences of insert / carve / transform / insertScanDenseMap on the device-resident dense map with random
    voxel sizes, carving radii, ray lengths and clouds (duplicates, points exactly on voxel boundaries, negative
    coordinates, zero-length rays): after every step the voxel keys, counts and fp64 means equal the oracle's."""
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
    from open3d_slam_advanced_rss_2024_public_amd.dense_map import DenseCarvingParamsC, DenseMap

    import os

    rng = np.random.default_rng(int(os.environ.get("O3S_FUZZ_SEED", "99")))   # other seeds: longer campaigns from the shell
    steps = 0
    for case in range(int(os.environ.get("O3S_FUZZ_CASES", "12"))):
        voxel = float(rng.choice([0.05, 0.08, 0.1, 0.25, 0.3]))
        dm, om = DenseMap(voxel), orc.DenseMap(voxel)
        extent = float(rng.uniform(1.0, 6.0))
        scans_inserted = 0
        for step in range(int(rng.integers(3, 8))):
            op = rng.choice(["insert", "insert", "carve", "transform", "scan"])
            n = int(rng.integers(1, 20000))
            p = rng.uniform(-extent, extent, (n, 3))
            if rng.random() < 0.3:   # points exactly on nominal voxel boundaries, and exact duplicates
                p[: n // 2] = np.round(p[: n // 2] / voxel) * voxel
                p[n // 2: n // 2 + n // 8] = p[: n // 8]
            nr = rng.normal(size=(n, 3)) if rng.random() < 0.6 else None
            if op == "insert":
                dm.insert(p, nr)
                om.insert(p, nr)
            elif op == "transform":
                T = syn.make_T(syn.rot_axis_angle(rng.normal(size=3), float(rng.uniform(-1, 1))), rng.uniform(-1, 1, 3))
                dm.transform(T)
                om.transform(T)
            elif op == "carve":
                radius = float(rng.choice([0.5, 1.0, 1.5, 2.0])) * voxel * float(rng.choice([1.0, 0.93]))
                max_len, trunc = float(rng.uniform(0.5, 8.0)), float(rng.choice([0.0, 0.1, 0.3]))
                sensor = rng.uniform(-0.5, 0.5, 3)
                rays = p[: max(1, n // 8)].copy()
                rays[0] = sensor   # a zero-length ray
                cp = DenseCarvingParamsC.make(radius, max_len, trunc)
                assert dm.carve(rays, sensor, cp) == om.carve(rays, sensor, radius, max_len, trunc), (case, step)
            else:   # Submap::insertScanDenseMap with carving every 2nd scan
                radius = 1.0 * voxel
                T = np.eye(4) if rng.random() < 0.3 else syn.make_T(syn.rot_axis_angle([0, 0, 1], float(rng.uniform(-1, 1))), rng.uniform(-1, 1, 3))
                r_crop = float(rng.uniform(0.5, 1.2)) * extent
                cp = DenseCarvingParamsC.make(radius, 4.0, 0.1, 2)
                raw = p[: max(1, n // 4)]
                rawn = None if nr is None else nr[: max(1, n // 4)]
                removed = dm.insertScanDenseMap(raw, T, co.croppingVolumeFactory("MaxRadius", r_crop), raw_normals=rawn, carving=cp)
                keep = orc.crop_mask(orc.make_cropper("MaxRadius", r_crop, centre=(0, 0, 0)), raw)
                if keep.any():
                    tp, tn = orc.transform_cloud(T, raw[keep], None if rawn is None else rawn[keep])
                    om.insert(tp, tn)
                exp = om.carve(raw, T[:3, 3], radius, 4.0, 0.1) if (scans_inserted % 2 == 1 and om.size() > 0) else 0
                assert removed == exp, (case, step)
                scans_inserted += 1
            gp, gn, gk, gc = dm.toPointCloud(with_keys=True)
            op_, on_, ok_, oc_ = om.to_point_cloud()
            assert np.array_equal(gk, ok_) and np.array_equal(gc, oc_) and np.array_equal(gp, op_), (case, step, op)
            assert (gn is None) == (on_ is None) and (gn is None or np.array_equal(gn, on_)), (case, step, op)
            steps += 1
    assert steps >= 40


def test_random_sparse_carve_histories_agree_with_the_oracle():
    """Random sequences of insertScan / carve on the device-resident sparse map with random cropping volumes (bounded, unbounded),
    map voxels, carving voxels of 0.5, 1 and 2.5 map voxels, ray lengths, truncations, min_dot and maps with and without normals;
    scans with exact duplicates, one zero-length ray and half their points snapped to nominal voxel boundaries (with poses that are
    pure translations along the grid, so that they stay there in the map frame).  After every step the whole map equals the
    oracle's bit for bit."""
    import os

    from open3d_slam_advanced_rss_2024_public_amd import Submap
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
    from test_gpu_submap import oracle_insert

    rng = np.random.default_rng(int(os.environ.get("O3S_FUZZ_SEED", "123")))   # other seeds: longer campaigns from the shell
    world = syn.make_world(9000.0, seed=3)
    same = lambda a, b: a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    steps = carves = carves_that_removed = 0
    for case in range(int(os.environ.get("O3S_FUZZ_CASES", "12"))):
        with_normals = bool(rng.random() < 0.6)
        kind = str(rng.choice(["MaxRadius", "Cylinder", "MinMaxRadius", "MinRadius", "Base"], p=[0.4, 0.2, 0.15, 0.15, 0.1]))
        r = float(rng.uniform(6.0, 11.0))
        params = {"MaxRadius": (r,), "Cylinder": (r, float(rng.uniform(-3.0, -0.5)), float(rng.uniform(2.0, 7.0))),
                  "MinMaxRadius": (float(rng.uniform(0.5, 2.0)), r), "MinRadius": (float(rng.uniform(0.5, 3.0)),), "Base": ()}[kind]
        map_voxel = float(rng.choice([0.1, 0.2, 0.35]))
        sm = Submap(map_voxel, co.croppingVolumeFactory("CroppingVolume" if kind == "Base" else kind, *params))
        mp = mn = centre = None
        base = np.array([rng.uniform(-6, 6), rng.uniform(-6, 6), 1.5])
        for step in range(int(rng.integers(3, 8))):
            op = "insert" if mp is None else str(rng.choice(["insert", "carve", "carve"]))
            pos = base + rng.uniform(-1.0, 1.0, 3) * np.array([1.0, 1.0, 0.2])
            if rng.random() < 0.4:       # a pure translation along the map's voxel grid: snapped points stay on voxel boundaries
                T = syn.make_T(None, np.round(pos / map_voxel) * map_voxel)
            else:
                T = syn.make_T(syn.rot_axis_angle(rng.normal(size=3) * np.array([0.1, 0.1, 1.0]), float(rng.uniform(-1, 1))), pos)
            n = int(rng.integers(500, 8000))
            sp, sn = syn.make_scan(world, n, T, radius=9.0, sigma=0.01, seed=int(rng.integers(0, 10**6)))
            sp, sn = sp.astype(np.float64), sn.astype(np.float64)
            sp[: n // 2] = np.round(sp[: n // 2] / map_voxel) * map_voxel
            sp[n // 2: n // 2 + n // 8] = sp[: n // 8]
            sn[n // 2: n // 2 + n // 8] = sn[: n // 8]
            ctx = (case, step, op, kind, params, map_voxel, with_normals)
            if op == "insert":
                assert sm.insertScan(sp, sn if with_normals else None, T)
                mp, mn = oracle_insert(mp, mn, sp, sn if with_normals else None, T, map_voxel, kind, params)
                centre = T[:3, 3].copy()
            else:
                carve_voxel = float(rng.choice([0.5, 1.0, 2.5])) * map_voxel
                max_len, trunc = float(rng.uniform(0.5, 12.0)), float(rng.choice([0.0, 0.1, 0.3, 1.0]))
                min_dot = float(rng.choice([-0.1, 0.0, 0.2, 0.5, 0.9]))
                sp[0] = 0.0              # a return at the sensor origin: a zero-length ray
                scan_map, _ = orc.transform_cloud(T, sp, None)
                subset = orc.crop_mask(orc.make_cropper(kind, *params, centre=centre), mp)
                rm = orc.carve(scan_map, mp, mn, T[:3, 3], carve_voxel, max_len, trunc, min_dot, subset=subset)
                k = sm.carve(sp, T, voxel_size=carve_voxel, max_raytracing_length=max_len, truncation_distance=trunc,
                             min_dot_product_with_normal=min_dot)
                assert k == int(rm.sum()), ctx
                mp, mn = mp[~rm], (None if mn is None else mn[~rm])
                carves += 1
                carves_that_removed += int(k > 0)
            gp, gn = sm.getMapPointCloud()
            assert len(sm) == len(mp) and same(gp, mp), ctx
            assert (gn is None) == (mn is None) and (mn is None or same(gn, mn)), ctx
            steps += 1
    print(f"sparse carve fuzz: {steps} steps, {carves} carves, {carves_that_removed} of them removed points")
    assert steps >= 40
    assert carves and 3 * carves_that_removed >= carves, (carves, carves_that_removed)


def test_random_resident_scan_loops_agree_with_the_oracle():
    """Random histories through the resident side pipelines — pre-process (wide crop, Open3D down-sample, narrow crop), map
    insert (transform, append, re-voxelise inside the map-builder volume) — with random cropping volumes (bounded ones take
    the hinted one-read-back path, unbounded / inverted ones the measuring path), voxel sizes, poses (including an
    almost-identity pose, which doubles the scan as the reference does) and clouds with and without normals.  Merge cloud,
    match cloud and the map after every insert: bit-identical to the oracle's host loops (voxel part in (z, y, x) order)."""
    import os

    from open3d_slam_advanced_rss_2024_public_amd import ProcessedScan, Submap
    from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

    rng = np.random.default_rng(int(os.environ.get("O3S_FUZZ_SEED", "77")))
    world = syn.make_world(9000.0, seed=3)

    def random_cropper(big):
        kind = str(rng.choice(["MaxRadius", "Cylinder", "MinMaxRadius", "MinRadius", "Base"], p=[0.4, 0.25, 0.2, 0.1, 0.05]))
        r = float(rng.uniform(8.0, 14.0) if big else rng.uniform(5.0, 9.0))
        if kind == "MaxRadius":
            return (kind, r)
        if kind == "Cylinder":
            return (kind, r, float(rng.uniform(-3.0, -0.5)), float(rng.uniform(2.0, 7.0)))
        if kind == "MinMaxRadius":
            return (kind, float(rng.uniform(0.5, 2.5)), r)
        if kind == "MinRadius":
            return (kind, float(rng.uniform(0.5, 3.0)))
        return (kind,)

    def gk(c):   # the device mirror names the pass-everything volume after the reference's base class
        return ("CroppingVolume",) + tuple(c[1:]) if c[0] == "Base" else c

    def canonical(p, n, idx, k):
        order = np.lexsort((idx[k:, 0], idx[k:, 1], idx[k:, 2])) + k
        sel = np.concatenate([np.arange(k), order])
        return p[sel], (None if n is None else n[sel])

    for case in range(int(os.environ.get("O3S_FUZZ_CASES", "10"))):
        with_normals = bool(rng.random() < 0.7)
        wide, narrow, builder = random_cropper(True), random_cropper(False), random_cropper(True)
        scan_voxel = float(rng.choice([0.0, 0.08, 0.15, 0.3]))
        map_voxel = float(rng.choice([0.1, 0.2, 0.35]))
        sm = Submap(map_voxel, co.croppingVolumeFactory(*gk(builder)))
        ps = ProcessedScan()
        mp = mn = None
        ctx = (case, wide, narrow, builder, scan_voxel, map_voxel, with_normals)
        for k in range(int(rng.integers(2, 5))):
            pos = np.array([rng.uniform(-8, 8), rng.uniform(-8, 8), 1.5])
            T = syn.make_T(syn.rot_axis_angle([0, 0, 1], float(rng.uniform(-1, 1))), pos) if not (k == 0 and rng.random() < 0.15) else np.eye(4)
            sp, sn = syn.make_scan(world, int(rng.integers(3000, 15000)), T if not np.allclose(T, np.eye(4)) else syn.make_T(None, pos), radius=13.0, sigma=0.01,
                                   seed=int(rng.integers(0, 10**6)))
            sp, sn = sp.astype(np.float64), sn.astype(np.float64)
            if not with_normals:   # the scan side needs normals (estimation has its own tests): keep them there, drop them for the map
                pass
            # ---- pre-process ----
            n_merge, n_match = ps.preprocess(co.croppingVolumeFactory(*gk(wide)), scan_voxel, co.croppingVolumeFactory(*gk(narrow)), sp, sn)
            m = orc.crop_mask(orc.make_cropper(*wide), sp)
            p, nn = sp[m], sn[m]
            if scan_voxel > 0 and len(p):
                p, nn, idx = orc.voxel_downsample_o3d(scan_voxel, p, nn)
                p, nn = canonical(p, nn, idx, 0)
            m2 = orc.crop_mask(orc.make_cropper(*narrow), p) if len(p) else np.zeros(0, bool)
            gp, gn = ps.merge
            assert n_merge == len(p) and np.array_equal(gp, p) and np.array_equal(gn, nn), ctx
            hp, hn = ps.match
            assert n_match == int(m2.sum()) and np.array_equal(hp, p[m2]) and np.array_equal(hn, nn[m2]), ctx
            if n_merge == 0:
                continue
            # ---- insert the merge cloud ----
            if with_normals:
                assert sm.insertProcessed(ps, T)
                ins_p, ins_n = p, nn
            else:
                assert sm.insertScan(p, None, T)
                ins_p, ins_n = p, None
            tp, tn = orc.transform_cloud(T, ins_p, ins_n)
            allp = tp if mp is None else np.concatenate([mp, tp])
            alln = None if ins_n is None else (tn if mn is None else np.concatenate([mn, tn]))
            c = orc.make_cropper(builder[0], *builder[1:], centre=T[:3, 3])
            op, on, oi = orc.voxelize_within_crop(c, map_voxel, allp, alln)
            passthrough = oi[:, 0] == np.iinfo(np.int32).min
            kk = int(passthrough.sum())
            mp, mn = canonical(op, on, oi, kk)
            gp, gn = sm.getMapPointCloud()
            assert len(sm) == len(mp) and np.array_equal(gp, mp), ctx + (k,)
            if with_normals:
                assert np.array_equal(gn, mn), ctx + (k,)


def test_random_registrations_agree_with_the_oracle():
    """tools/fuzz_registration.py, a short campaign: the Open3D-semantics registration (include/o3s_registration.h) against the
    oracle's brute force on random clouds, radii from 2 cm to the whole scene, duplicated target points (ties), sources partly or
    wholly outside the target, 0 - 30 iterations.  The search (counts, fitness; RMSE and information matrix 1e-9) must agree at the
    initial and at the final pose in every case, the whole trajectory wherever the 6 x 6 systems are well-conditioned."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_registration

    out = fuzz_registration.run_cases(int(os.environ.get("O3S_FUZZ_SEED", "11")), int(os.environ.get("O3S_FUZZ_CASES", "30")))
    assert out["disagreements"] == 0, out
    assert out["well_conditioned_cases"] >= 5
