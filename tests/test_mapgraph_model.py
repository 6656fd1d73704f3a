"""The model of the observation graph (tests/mapgraph_model.py) held to expected values written out by hand, on hand-built maps, so
that the model the device is compared with is not its own judge.  No GPU."""
import pytest

from mapgraph_model import KeyFrame, MapPoint, Refused, SlotGraph
from mapgraph_scenes import CULL_CASES, Scene, random_cull_scene


def _model(scene, max_obs=8):
    return scene.play(SlotGraph(*scene.limits(max_obs)))


@pytest.mark.parametrize("case", CULL_CASES, ids=[c["name"] for c in CULL_CASES])
def test_cull_cases(case):
    g = _model(case["scene"])
    for k, want in case.get("alone", {}).items():      # the keyframe's decision on the untouched graph
        r = g.clone().cull_keyframes([k], [0], case["monocular"])
        assert (r["culled"][0], r["n_mps"][0], r["n_redundant"][0]) == want
    assert g.cull_keyframes(case["local"], case["not_erase"], case["monocular"]) == case["expect"]


def test_case_table_covers_the_issue():
    assert [c["name"] for c in CULL_CASES] == [
        "scale_plus_one_counts", "scale_plus_two_does_not", "finer_scales_count", "two_observers_not_redundant", "nobs_3_does_not_qualify",
        "nobs_4_qualifies", "nobs_4_two_stereo_observations", "far_skipped_in_stereo", "far_counted_monocular", "nine_of_ten_kept",
        "ten_of_eleven_culled", "not_erase", "cascade_a", "cascade_b"]


def test_not_erase_leaves_the_graph_and_still_observes():
    case = [c for c in CULL_CASES if c["name"] == "not_erase"][0]
    g = _model(case["scene"])
    g.cull_keyframes(case["local"], case["not_erase"], True)
    kfs, pts = g.dump()
    assert sorted(kfs) == [0, 2, 3]                                # 1 is gone, 0 stays
    assert kfs[0]["point"] == [0, 1, 2, 3, 4]
    assert pts[0] == dict(n_obs=3, bad=False, obs=[(0, 0), (2, 0), (3, 0)])


def test_cascade_b_graph_after():
    case = [c for c in CULL_CASES if c["name"] == "cascade_b"][0]
    g = _model(case["scene"])
    g.cull_keyframes(case["local"], case["not_erase"], True)
    kfs, pts = g.dump()
    assert pts[20] == dict(n_obs=2, bad=True, obs=[])              # nObs stays what EraseObservation left
    assert kfs[5]["point"] == [-1] and kfs[6]["point"] == [-1]     # the former observers lose their match
    assert kfs[1]["point"][10] == 20                               # a match without an observation is nobody's to clear
    assert pts[0] == dict(n_obs=3, bad=False, obs=[(2, 0), (3, 0), (4, 0)])


def _three(weights):
    s = Scene()
    for k, w in enumerate(weights):
        s.kf(k, 2, stereo=w == 2)
        s.see(0, k, 1)
    return _model(s)


def test_erase_cascade_mono():
    g = _three((1, 1, 1))
    assert g.dump()[1][0]["n_obs"] == 3
    g.erase_observations([0], [0])                                 # 3 -> 2: bad
    kfs, pts = g.dump()
    assert pts[0] == dict(n_obs=2, bad=True, obs=[])
    assert kfs[0]["point"] == [-1, 0]                              # EraseObservation does not touch the eraser's own match
    assert kfs[1]["point"] == [-1, -1] and kfs[2]["point"] == [-1, -1]
    assert [mp.slot for mp in g.went_bad] == [0]


def test_erase_cascade_stereo_weights():
    g = _three((2, 2, 1))
    assert g.dump()[1][0]["n_obs"] == 5
    g.erase_observations([0], [2])                                 # 5 -> 4
    assert g.dump()[1][0] == dict(n_obs=4, bad=False, obs=[(0, 1), (1, 1)])
    g.erase_observations([0], [0])                                 # 4 -> 2: bad
    kfs, pts = g.dump()
    assert pts[0] == dict(n_obs=2, bad=True, obs=[])
    assert kfs[1]["point"] == [-1, -1] and kfs[2]["point"] == [-1, 0] and kfs[0]["point"] == [-1, 0]


def test_erasures_of_one_point_in_a_batch_are_order_free():
    a, b = _three((1, 1, 1, 1, 1)), _three((1, 1, 1, 1, 1))
    a.erase_observations([0, 0], [1, 3])
    b.erase_observations([0, 0], [3, 1])
    assert a.dump() == b.dump()
    assert a.dump()[1][0] == dict(n_obs=3, bad=False, obs=[(0, 1), (2, 1), (4, 1)])


def test_erase_points_and_erase_keyframe():
    g = _three((1, 1, 1, 1))
    g.erase_keyframe(3)                                            # 4 -> 3
    kfs, pts = g.dump()
    assert sorted(kfs) == [0, 1, 2] and pts[0] == dict(n_obs=3, bad=False, obs=[(0, 1), (1, 1), (2, 1)])
    g.erase_points([0])
    kfs, pts = g.dump()
    assert pts[0] == dict(n_obs=3, bad=True, obs=[])               # SetBadFlag leaves nObs
    assert all(kfs[k]["point"] == [-1, -1] for k in (0, 1, 2))


def test_repeated_add_observation():
    g = _three((2, 1, 1))
    g.add_observations([0], [0], [0])                              # src/MapPoint.cc:109: already there
    assert g.dump()[1][0] == dict(n_obs=4, bad=False, obs=[(0, 1), (1, 1), (2, 1)])


def test_match_without_observation_and_observation_without_match():
    s = Scene()
    for k in range(5):
        s.kf(k, 2)
    for k in (1, 2, 3):
        s.see(0, k, 0)
    s.match(0, 0, 0)                                               # keyframe 0 holds point 0, the point does not know
    s.obs(0, 4, 1)                                                 # the point knows keyframe 4, which holds nothing
    g = _model(s)
    assert g.covisibility(0) == {1: 1, 2: 1, 3: 1, 4: 1}
    assert g.covisibility(4) == {}
    assert g.vote([0]) == {1: 1, 2: 1, 3: 1, 4: 1}
    g.erase_keyframe(0)                                            # EraseObservation finds no entry
    assert g.dump()[1][0] == dict(n_obs=4, bad=False, obs=[(1, 0), (2, 0), (3, 0), (4, 1)])
    g.erase_keyframe(4)                                            # no match, so nobody tells the point: the entry outlives the keyframe
    kfs, pts = g.dump()
    assert sorted(kfs) == [1, 2, 3] and pts[0]["obs"] == [(1, 0), (2, 0), (3, 0), (4, 1)] and pts[0]["n_obs"] == 4
    assert g.vote([0]) == {1: 1, 2: 1, 3: 1, 4: 1}


def test_votes_skip_bad_points():
    g = _three((1, 1, 1))
    assert g.vote([0, 0]) == {0: 2, 1: 2, 2: 2}
    assert g.covisibility(1) == {0: 1, 2: 1}
    g.erase_points([0])
    assert g.vote([0]) == {} and g.covisibility(1) == {}


def test_refusals_leave_the_model():
    g = _three((1, 1, 1))
    before = g.dump()
    for call, code in ((lambda: g.set_keyframe(0, [0], [0], [1]), -1), (lambda: g.set_matches(0, [0, 0], [1, 1]), -1),
                       (lambda: g.add_observations([0, 0], [1, 1], [0, 1]), -1), (lambda: g.erase_points([0, 0]), -1),
                       (lambda: g.add_observations([0], [5], [0]), -1), (lambda: g.set_matches(0, [2], [0]), -1)):
        with pytest.raises(Refused) as e:
            call()
        assert e.value.code == code and g.dump() == before


def test_objects_alone():
    # the classes without the slot layer: AddObservation's weights and the idx that a repeated call keeps
    a, b = KeyFrame([0, 0], [1, 0], [1, 1]), KeyFrame([0], [0], [1])
    p = MapPoint()
    p.AddObservation(a, 0); p.AddObservation(b, 0); p.AddObservation(a, 1)
    assert p.nObs == 3 and p.mObservations == {a: 0, b: 0}


def test_random_scenes_are_eventful():
    """the shares that tests/test_mapgraph.py asks of its 200 seeds, on a sample, so that a generator that has gone quiet shows here"""
    culls = bads = 0
    for seed in range(40):
        s, local, ne, mono = random_cull_scene(seed)
        r = _model(s).cull_keyframes(local, ne, mono)
        culls += 1 in r["culled"]
        bads += bool(r["bad_points"])
    assert culls >= 10 and bads >= 4
