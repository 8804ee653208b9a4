"""FPFH at closure size (csrc/fpfh_dev.h): a 0.4 M-point map at 0.1 m voxelised to 0.25 m — about 145 k sparse points, eleven
times the default sparse cloud — plus a cluster of 2 000 points inside one ball, so that the grid spans many tiles and the
selection has to cut its LDS buffer again and again (a ball with far more candidates than the buffer holds must still be exact).
Stages 1 - 3 of tests/test_gpu_fpfh.py; MI355X only."""
import numpy as np
import pytest

import fpfh_ref as fr
from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co

pytestmark = pytest.mark.gpu

RADIUS, KNN, CLUSTER = 1.25, 100, 2000


def test_closure_size_cloud_with_an_overfull_ball():
    p, n, mp = fr.sparse_cloud(area=9000.0, n_map=400000, voxel=0.25, normal_radius=1.0, normal_knn=20, cluster=CLUSTER)
    assert len(mp) >= 300000 and len(p) > 100000
    r = fr.compute_fpfh(p, n, RADIUS, KNN)
    # the input has what it is there for: balls with 2 000+ candidates (every cluster point sees the whole cluster)
    d = np.linalg.norm(p[-CLUSTER:] - p[-CLUSTER:].mean(axis=0), axis=1)
    assert d.max() < RADIUS / 2 and (r.nn[-CLUSTER:] >= len(p) - CLUSTER).mean() > 0.95
    print(f"points {len(p)}, sensitive {int(r.sensitive.sum())}")
    assert r.sensitive.mean() <= 0.01
    f, spfh, nn = co.computeFPFHFeature(p, n, RADIUS, KNN, want_spfh=True, want_neighbours=True)
    assert np.array_equal(nn, r.nn)                                         # stage 1
    keep = ~r.sensitive
    assert np.array_equal(spfh[keep], r.spfh[keep])                         # stage 2
    assert np.array_equal(f, fr.fpfh_from_spfh(spfh, nn, fr.list_d2(p, nn)))  # stage 3: every point
