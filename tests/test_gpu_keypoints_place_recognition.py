"""Place recognition on ISS keypoints (PlaceRecognitionParameters.feature_keypoints -> SubmapCollection.computeFeatures(keypoints=)
-> Submap.selectKeypoints).  MI355X only; every comparison is bit for bit.

Off (the default) changes nothing: a run whose parameters carry feature_keypoints = None gives the constraints of a run that never
names the parameter.  On, the one-to-many call's intermediate results are those of the per-pair calls on the reduced feature sets
— the property the one-to-many path promises on any feature set.  Whether a closure is still ACCEPTED on keypoints is a property of
the scene and the radii: tools/keypoints_bench.py reports it; it is printed here, not asserted."""
import math

import numpy as np
import pytest

from open3d_slam_advanced_rss_2024_public_amd import cloud_ops as co
from open3d_slam_advanced_rss_2024_public_amd import place_recognition as pr
from open3d_slam_advanced_rss_2024_public_amd import registration as reg
from open3d_slam_advanced_rss_2024_public_amd import synthetic as syn
from open3d_slam_advanced_rss_2024_public_amd.submap_collection import SubmapCollection
from test_gpu_place_recognition import NoScan, disc, rigid, same_ransac, submap_of

pytestmark = pytest.mark.gpu

Q = co.iss_params(0.0, 0.0, 0.975, 0.975, 5)
PRM = reg.RansacParams(seed=3)


def scene():
    """test_gpu_place_recognition's closure scene without feature sets: two candidates (0, 1), two far submaps, the source (4) seeing
    the disc around the third pose from a frame of its own, and the active submap (5)"""
    world = syn.make_world(3000.0, seed=21)
    centres = [syn.loop_pose(world, k)[:3, 3] for k in (0, 20, 40)]
    Ti = np.linalg.inv(rigid(math.radians(10.0), (0.5, -0.3, 0.0)))
    pts = disc(centres[2], 16.0)
    maps = [submap_of(disc(centres[0], 16.0), False), submap_of(disc(centres[1], 16.0), False)]
    maps += [submap_of(disc((0.0, 0.0), 3.0), False) for _ in range(2)]
    maps += [submap_of(np.ascontiguousarray(pts @ Ti[:3, :3].T + Ti[:3, 3]), False), submap_of(disc((0.0, 0.0), 3.0), False)]
    it = iter(maps)
    col = SubmapCollection(20.0, 3, 10 ** 9, 2, 0.1, ("MaxRadius", 1000.0), submap_factory=lambda: next(it), scan_factory=NoScan)
    for _ in range(5):
        col.create(np.zeros(3))
    for i in range(5):
        col.add_edge(i, i + 1)
    col.centers = [centres[0], centres[1], centres[2] + [100.0, 0.0, 0.0], centres[2] + [0.0, 20.5, 0.0], centres[2], centres[2]]
    return col, maps


def params(**kw):
    return pr.PlaceRecognitionParameters(ransac=PRM, overlap_voxel_size=20 * 0.1, registration_type="PointToPointIcp", **kw)


def same_constraints(a, b):
    return len(a) == len(b) and all(x.target_submap_idx == y.target_submap_idx and np.array_equal(x.source_to_target, y.source_to_target)
                                    and np.array_equal(x.information_matrix, y.information_matrix) for x, y in zip(a, b))


def same_candidates(a, b):
    return len(a) == len(b) and all(x.target_submap_idx == y.target_submap_idx and x.rejected == y.rejected and same_ransac(x.ransac, y.ransac)
                                    for x, y in zip(a, b))


def test_off_is_the_run_that_never_names_the_parameter_and_on_equals_the_per_pair_calls():
    col, maps = scene()
    source = maps[4]
    # never named
    sizes = [col.computeFeatures(i) for i in (0, 1, 4)]
    plain = pr.PlaceRecognition(params())
    c_plain = plain.buildLoopClosureConstraints(np.eye(4), col, 4, 5, 42.0)
    # named and off
    off = pr.PlaceRecognition(params(feature_keypoints=None))
    assert [off.computeFeatures(col, i) for i in (0, 1, 4)] == sizes and [maps[i].features_size() for i in (0, 1, 4)] == sizes
    c_off = off.buildLoopClosureConstraints(np.eye(4), col, 4, 5, 42.0)
    assert same_constraints(c_plain, c_off) and same_candidates(plain.last_candidates, off.last_candidates)
    assert [c.target_submap_idx for c in plain.last_candidates] == [0, 1] and len(c_plain) >= 1
    # on: the collection reduces each feature set right behind its computation
    on = pr.PlaceRecognition(params(feature_keypoints=Q))
    kept = [on.computeFeatures(col, i) for i in (0, 1, 4)]
    print(f"sparse points {sizes} -> keypoints {kept}")
    assert [maps[i].features_size() for i in (0, 1, 4)] == kept and all(10 < k < n // 4 for k, n in zip(kept, sizes))
    assert maps[2].features_size() == maps[3].features_size() == maps[5].features_size() == -1
    c_on = on.buildLoopClosureConstraints(np.eye(4), col, 4, 5, 42.0)
    want = []
    for i in (0, 1):
        c = reg.loop_closure_constraint(source, maps[i], PRM, overlap_voxel_size=20 * 0.1, registration_type="PointToPointIcp")
        rejected = c.rejected
        if not (rejected or "").startswith("ransac:") and not pr.is_registration_consistent(c.ransac.transformation):
            rejected = pr.REJECTED_RANSAC_INCONSISTENT
        elif rejected is None and not pr.is_registration_consistent(c.source_to_target):
            rejected = pr.REJECTED_ICP_INCONSISTENT
        want.append((i, rejected, c))
    for (i, rejected, c), g in zip(want, on.last_candidates):
        print(f"candidate {i} on keypoints: {rejected}; ransac inliers {len(c.ransac.correspondence_set)} of {c.ransac.n_correspondences} "
              f"(full set: {plain.last_candidates[i].rejected}, {len(plain.last_candidates[i].ransac.correspondence_set)} of "
              f"{plain.last_candidates[i].ransac.n_correspondences})")
        assert g.target_submap_idx == i and g.rejected == rejected and same_ransac(g.ransac, c.ransac)
        assert same_ransac(g.ransac, source.ransacRegistration(maps[i], PRM))
        if g.refinement is not None:
            assert g.n_overlap == c.n_overlap and np.array_equal(g.refinement.transformation, c.refinement.transformation)
    accepted = [(i, c) for i, rejected, c in want if rejected is None]
    assert [k.target_submap_idx for k in c_on] == [i for i, _ in accepted]
    for k, (i, c) in zip(c_on, accepted):
        assert np.array_equal(k.source_to_target, c.source_to_target) and np.array_equal(k.information_matrix, c.information_matrix)
