"""The two registration health gates in the Python mirror of the drivers (mapper.py: min_refinement_fitness /
ignore_min_refinement_fitness, Mapper.cpp:424-431; submap_collection.py: adjacency_based_revisiting_min_fitness,
SubmapCollection.cpp:392-407) over the scenes of tests/health_scenes.py.  Both gates are off by default: with them off the drivers
take the steps they always took."""
import math

import numpy as np
import pytest

import health_scenes as hs

pytestmark = pytest.mark.gpu


# ---- scan-to-map fitness ------------------------------------------------------------------------------------------------------------
def test_the_scene_does_not_hang_on_rounding():
    sc = hs.fitness_scene()
    print(f"good: max {sc['d_good'].max():.3f} m, junk: min {sc['d_junk'].min():.3f} m from the map; {sc['n_good']} + {sc['n_junk']} points")
    # the share of points within 1 mm of the max_dist radius is zero (by a wide margin: the pose moves by centimetres at most)
    d = np.concatenate([sc["d_good"], sc["d_junk"]])
    assert np.count_nonzero(np.abs(d - hs.MAX_DIST) <= 0.001) == 0
    assert sc["d_good"].max() < 0.4 and sc["d_junk"].min() > 0.6
    # ... and so is the share of coordinates within 1 mm of a voxel face, in the sensor frame (the scan's voxel grid) and, for the
    # sweep that is inserted at a given pose, in the map frame (a translation by a multiple of the voxel, up to an ulp)
    for k, (sp, _) in enumerate(sc["scans"]):
        assert face_share(sp) == 0, k
    assert face_share(sc["scans"][0][0] + sc["poses"][0][:3, 3]) == 0


def face_share(p):
    return np.count_nonzero(hs.face_distance(p) <= 0.001)


def test_gate_on_gives_the_half_matched_scan_up_and_changes_nothing():
    on = hs.fitness_run(False)
    for k, r in enumerate(on):
        print(k, {a: r[a] for a in ("ok", "inserted", "rejected", "n_corr", "n_points", "fitness", "map_size")})
    assert [r["ok"] for r in on] == [1, 1, 0, 1] and [r["rejected"] for r in on] == [0, 0, 1, 0]
    assert [r["threw"] for r in on] == [0, 0, 0, 0]
    assert math.isnan(on[0]["fitness"])                       # the first scan is inserted, not registered
    assert on[1]["fitness"] > 0.99 and on[3]["fitness"] > 0.99
    bad = on[2]
    assert 0.4 < bad["fitness"] < 0.6 and bad["fitness"] < hs.MIN_FITNESS
    assert bad["n_points"] == bad["n_match"] and bad["n_corr"] == round(bad["fitness"] * bad["n_points"])
    # nothing is adopted, pushed or inserted: pose, previous pose, pose buffer, last stamp and map are those after sweep 1
    for a in ("T", "T_prev"):
        assert np.array_equal(bad[a], on[1][a]), a
    assert (bad["n_buffer"], bad["last_stamp"], bad["map_size"], bad["inserted"]) == (on[1]["n_buffer"], on[1]["last_stamp"], on[1]["map_size"], 0)
    # the sweep after it is registered from the pose before it and goes in
    assert on[3]["inserted"] == 1 and on[3]["n_buffer"] == on[1]["n_buffer"] + 1 and on[3]["map_size"] > on[1]["map_size"]


def test_gate_ignored_adopts_the_scan_exactly_as_without_the_feature():
    ignored, default, on = hs.fitness_run(True), hs.fitness_run(None), hs.fitness_run(False)
    assert [r["ok"] for r in ignored] == [1, 1, 1, 1] and [r["inserted"] for r in ignored] == [1, 1, 1, 1]
    for k, (a, b) in enumerate(zip(ignored, default)):        # the constructed parameters ARE "ignore": the same bits
        assert np.array_equal(a["T"], b["T"]) and a["map_size"] == b["map_size"] and a["rejected"] == b["rejected"] == 0, k
        assert math.isnan(a["fitness"]) and a["n_points"] == 0    # nothing is evaluated
    # up to the rejected sweep the gate changes no bit of the trajectory
    for k in (0, 1):
        assert np.array_equal(ignored[k]["T"], on[k]["T"]) and ignored[k]["map_size"] == on[k]["map_size"]
    assert ignored[2]["map_size"] > on[2]["map_size"]


# ---- revisit consistency ------------------------------------------------------------------------------------------------------------
def first(rows, pred):
    return next(k for k, r in enumerate(rows) if pred(r))


def test_a_matching_scan_switches_back_and_a_shifted_one_does_not():
    sc = hs.revisit_scene(False)
    match_on, shift_on = hs.revisit_run(False, True), hs.revisit_run(True, True)
    match_off, shift_off = hs.revisit_run(False, False), hs.revisit_run(True, False)
    for name, rows in (("matching, on", match_on), ("shifted, on", shift_on), ("shifted, off", shift_off)):
        print(name, [(r["active"], r["n_submaps"], round(r["fitness"], 3)) for r in rows])
    R = hs.REVISIT["radius"]
    born = first(match_on, lambda r: r["n_submaps"] == 2)              # submap 1 is created on the way out, in every variant
    assert 5 <= born <= 8
    for rows in (match_on, shift_on, match_off, shift_off):
        assert [(r["active"], r["n_submaps"]) for r in rows[: born + 2]] == [(0, 1)] * born + [(1, 2)] * 2
        assert rows[born]["snapshots"][0] > 0                           # the finished submap has its snapshot (computeFeatures)
    # switch on, matching scan: the collection goes back to submap 0, on the strength of a check it passed
    back = first(match_on, lambda r: r["active"] == 0 and r["n_submaps"] == 2)
    assert back > born + 1 and match_on[back]["switched"] == 1 and match_on[back]["fitness"] > 0.8 > hs.ADJ_MIN_FITNESS
    assert all(math.isnan(r["fitness"]) for r in match_on[:back])       # no check before: the closest submap was the active one
    # switch off: the parent's trajectory of submap ids — the switch happens at the same sweep, asked or not, matching or not
    ids = lambda rows: [(r["active"], r["n_submaps"]) for r in rows]    # noqa: E731
    assert ids(match_off) == ids(shift_off) == ids(match_on)
    assert all(math.isnan(r["fitness"]) for r in match_off + shift_off)
    # switch on, shifted scan: refused where the matching one was accepted, and at every later sweep; a new submap is created only
    # once the sensor is a radius away from the active submap
    assert shift_on[back]["active"] == 1 and shift_on[back]["fitness"] == 0.0
    origin1 = sc["poses"][born][:3, 3]
    away = [float(np.linalg.norm(T[:3, 3] - origin1)) for T in sc["poses"]]
    created = first(shift_on, lambda r: r["n_submaps"] == 3)
    assert created > back and away[created] > R and all(away[k] <= R for k in range(born, created))
    for k in range(back, created):
        assert shift_on[k]["active"] == 1 and shift_on[k]["fitness"] <= hs.ADJ_MIN_FITNESS, k
    assert all(r["active"] != 0 for r in shift_on[born:])
