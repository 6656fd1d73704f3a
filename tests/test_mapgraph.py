"""The resident observation graph (include/orbx.h: orbx_mapgraph) against the sequential model of tests/mapgraph_model.py: interleaved
edit batches read back whole, every refusal with the graph unchanged behind it, the two votes at every launch form, the hand-built
maps of KeyFrameCulling and 200 seeded random ones with the whole graph compared after the call.  Integer results: everything is equal
or it is wrong.  CPU: the ABI surface."""
import os

import numpy as np
import pytest

from mapgraph_model import Refused, SlotGraph
from mapgraph_scenes import CULL_CASES, Scene, random_cull_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["orbx_mapgraph_create", "orbx_mapgraph_destroy", "orbx_mapgraph_clear", "orbx_mapgraph_set_keyframe", "orbx_mapgraph_set_matches",
               "orbx_mapgraph_add_observations", "orbx_mapgraph_erase_observations", "orbx_mapgraph_erase_points", "orbx_mapgraph_erase_keyframe",
               "orbx_mapgraph_keyframe_observations", "orbx_mapgraph_read_keyframe", "orbx_mapgraph_read_points", "orbx_mapgraph_vote", "orbx_mapgraph_covisibility",
               "orbx_mapgraph_cull_keyframes"]
LDS_KEYFRAMES = 8192    # the vote kernel's histogram lives in LDS up to this many keyframe slots (orbx_mapgraph.hip: MG_LDS_KEYFRAMES)


def test_new_symbols_exported_and_typed(pkg):
    import __graft_entry__ as ge
    ge.build()
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    src = open(os.path.join(ROOT, "orb-slam2_amd", "csrc", "orbx_mapgraph.hip")).read()
    for n in NEW_SYMBOLS:
        assert n + "(" in hdr, n
        assert getattr(L, n).argtypes is not None, n
    assert "orbx_mapgraph.hip" in ge.HIP_SOURCES
    assert "#define MG_LDS_KEYFRAMES %d " % LDS_KEYFRAMES in src
    for m in ("set_keyframe", "set_matches", "add_observations", "erase_observations", "erase_points", "erase_keyframe", "clear", "vote",
              "covisibility", "cull_keyframes", "read_keyframe", "read_points"):
        assert callable(getattr(pkg.MapGraph, m)), m


# ------------------------------------------------------------------------------------------------ helpers

def dump_device(g, max_kf=None):
    kfs = {}
    for k in range(g.max_keyframes if max_kf is None else max_kf):
        r = g.read_keyframe(k)
        if r is not None:
            kfs[k] = dict(point=r["point"].tolist(), octave=r["octave"].tolist(), stereo=[bool(x) for x in r["stereo"]], close=[bool(x) for x in r["close"]])
    return kfs, g.read_points()


def same_graph(g, m, tag=""):
    dk, dp = dump_device(g)
    mk, mp = m.dump()
    assert sorted(dk) == sorted(mk), (tag, "keyframe slots", sorted(dk), sorted(mk))
    for k in mk:
        assert dk[k] == mk[k], (tag, "keyframe", k)
    assert sorted(dp) == sorted(mp), (tag, "point slots", sorted(set(dp) ^ set(mp)))
    for p in mp:
        assert dp[p] == mp[p], (tag, "point", p, dp[p], mp[p])


def both(pkg, g, m, name, *args):
    """one edit on the model and on the device; a refusal must be the same refusal and leave both as they were"""
    try:
        getattr(m, name)(*args)
    except Refused as r:
        with pytest.raises(pkg.OrbxError) as e:
            getattr(g, name)(*args)
        assert e.value.code == r.code, (name, args, str(e.value))
        same_graph(g, m, ("after refusal", name))
        return r.code
    getattr(g, name)(*args)
    return 0


def pair(pkg, limits):
    return pkg.MapGraph(*limits), SlotGraph(*limits)


def same_cull(got, want, tag):
    assert got["culled"].tolist() == list(want["culled"]), (tag, "culled")
    assert got["n_mps"].tolist() == list(want["n_mps"]), (tag, "n_mps")
    assert got["n_redundant"].tolist() == list(want["n_redundant"]), (tag, "n_redundant")
    assert got["bad_points"].tolist() == list(want["bad_points"]), (tag, "bad_points")


def counts_of(d, n):
    c = np.zeros(n, np.int32)
    for k, v in d.items():
        c[k] = v
    return c


def same_votes(g, m, points, tag):
    cnt, nz = g.vote(points)
    want = counts_of(m.vote(points), g.max_keyframes)
    assert np.array_equal(cnt, want), (tag, np.flatnonzero(cnt != want)[:8])
    assert nz.tolist() == np.flatnonzero(want).tolist(), tag


def same_covis(g, m, k, tag):
    cnt, nz = g.covisibility(k)
    want = counts_of(m.covisibility(k), g.max_keyframes)
    assert np.array_equal(cnt, want), (tag, k, np.flatnonzero(cnt != want)[:8])
    assert nz.tolist() == np.flatnonzero(want).tolist(), tag


# ------------------------------------------------------------------------------------------------ edits

@pytest.mark.gpu
def test_random_edit_batches(pkg):
    NK, NF, NP, MO = 6, 40, 60, 4
    g, m = pair(pkg, (NK, NF, NP, MO))
    r = np.random.RandomState(7)

    def new_kf(k):
        stale = [(p, k) for p, mp in m.pt.items() for kf in mp.mObservations if kf.slot == k]   # entries that outlived the slot's last keyframe
        assert g.keyframe_observations(k) == len(stale) == m.keyframe_observations(k)
        if stale:
            assert both(pkg, g, m, "set_keyframe", k, [0], [0], [1]) == -1                      # the slot is not given away under them
            both(pkg, g, m, "erase_observations", [p for p, _ in stale], [k for _, k in stale])
        n = int(r.randint(NF // 2, NF + 1))
        both(pkg, g, m, "set_keyframe", k, r.randint(0, 8, n).tolist(), r.randint(0, 2, n).tolist(), r.randint(0, 2, n).tolist())

    for k in range(NK):
        new_kf(k)
    # rows to capacity, and the overflow refused: alone, and in a batch whose first entries would have fitted
    both(pkg, g, m, "add_observations", [59] * 4, [0, 1, 2, 3], [0, 0, 0, 0])
    assert both(pkg, g, m, "add_observations", [59], [4], [0]) == -2
    assert both(pkg, g, m, "add_observations", [58] * 5 + [57], [0, 1, 2, 3, 4, 0], [1] * 6) == -2
    assert both(pkg, g, m, "add_observations", [59, 57], [3, 0], [5, 1]) == 0      # a keyframe already in the full row: a no-op, not an overflow
    same_graph(g, m, "capacity")
    refused = full = 0
    for step in range(160):
        live = sorted(m.kf)
        known = sorted(m.pt)
        u = r.rand()
        if not live or (u < 0.08 and len(live) < NK):
            new_kf(int(r.choice([k for k in range(NK) if k not in m.kf])))
        elif u < 0.30:
            k = int(r.choice(live))
            idx = r.choice(len(m.kf[k].mvpMapPoints), int(r.randint(1, 9)), replace=False).tolist()
            both(pkg, g, m, "set_matches", k, idx, [int(r.choice(known)) if known and r.rand() < 0.8 else -1 for _ in idx])
        elif u < 0.62:
            n = int(r.randint(1, 9))
            pts = [int(p) for p in r.randint(0, 24 if r.rand() < 0.7 else NP, n)]
            pts = [p for p in pts if p not in m.pt or not m.pt[p].mbBad]           # a bad slot is not used again here (test_slot_reuse)
            ks = [int(r.choice(live)) for _ in pts]
            keep = sorted(set(zip(pts, ks)))
            idx = [int(r.randint(0, len(m.kf[k].mvpMapPoints))) for _, k in keep]
            code = both(pkg, g, m, "add_observations", [p for p, _ in keep], [k for _, k in keep], idx)
            refused += code == -2
            if code == 0 and r.rand() < 0.8:                                       # mostly, the keyframe learns of it too
                for (p, k), i in zip(keep, idx):
                    if m.kf[k].mvpMapPoints[i] is None:
                        both(pkg, g, m, "set_matches", k, [i], [p])
        elif u < 0.80:
            obs = [(p, kf.slot) for p, mp in m.pt.items() for kf in mp.mObservations]
            if obs:
                pick = [obs[j] for j in r.choice(len(obs), min(len(obs), int(r.randint(1, 5))), replace=False)]
                pick.append((int(r.randint(0, NP)), int(r.randint(0, NK))))        # and one that is probably not there
                pick = sorted(set(pick))
                both(pkg, g, m, "erase_observations", [p for p, _ in pick], [k for _, k in pick])
        elif u < 0.88:
            both(pkg, g, m, "erase_points", sorted(set(int(p) for p in r.randint(0, NP, int(r.randint(1, 3))))))
        elif u < 0.94 and len(live) > 2:
            both(pkg, g, m, "erase_keyframe", int(r.choice(live)))
        else:
            same_votes(g, m, r.randint(0, NP, 30).tolist(), step)
            same_covis(g, m, int(r.choice(live)), step)
        full += any(len(mp.mObservations) == MO for mp in m.pt.values())
        same_graph(g, m, step)
    assert full >= 10 and len(m.went_bad) >= 10, (refused, full, len(m.went_bad))   # (the overflow refusals are the ones above; more may come)
    g.clear(); m.clear()
    same_graph(g, m, "clear")
    assert dump_device(g) == ({}, {})


@pytest.mark.gpu
def test_slot_reuse(pkg):
    """an observation on a bad slot starts a new point there; a keyframe slot is used again after erase_keyframe"""
    s = Scene()
    for k in range(3):
        s.kf(k, 2, stereo=True)
        s.see(0, k, 0)
    g, m = pair(pkg, (4, 4, 2, 4))
    s.play(g); s.play(m)
    for name, args in (("erase_points", ([0],)), ("add_observations", ([0, 0], [1, 2], [1, 1])), ("erase_keyframe", (0,)),
                       ("set_keyframe", (0, [1, 2, 3, 4], [0] * 4, [1] * 4)), ("add_observations", ([0], [0], [3]))):
        assert both(pkg, g, m, name, *args) == 0
        same_graph(g, m, name)
    assert g.read_point(0) == dict(n_obs=5, bad=False, obs=[(0, 3), (1, 1), (2, 1)])
    assert g.read_keyframe(0)["octave"].tolist() == [1, 2, 3, 4] and g.read_keyframe(0)["point"].tolist() == [-1] * 4


@pytest.mark.gpu
def test_refusals(pkg):
    with pytest.raises(pkg.OrbxError):
        pkg.MapGraph(0, 4, 4, 4)
    for bad in ((65536, 4, 4, 4), (4, 65536, 4, 4), (4, 4, (1 << 24) + 1, 4), (4, 4, 4, 3), (4, 4, 4, 257), (4, 4, 1 << 24, 256)):   # the last: more than 2^32 - 1 words
        with pytest.raises(pkg.OrbxError) as e:
            pkg.MapGraph(*bad)
        assert e.value.code == -1, bad
    s = Scene()
    for k in range(5):
        s.kf(k, 3)
    for k in range(4):
        s.see(0, k, 0)
    g, m = pair(pkg, (6, 3, 3, 4))
    s.play(g); s.play(m)
    table = [
        ("set_keyframe", (0, [0], [0], [1]), -1),                   # the slot is in use
        ("set_keyframe", (-1, [0], [0], [1]), -1),
        ("set_keyframe", (6, [0], [0], [1]), -2),                   # beyond max_keyframes
        ("set_keyframe", (5, [0] * 4, [0] * 4, [1] * 4), -2),       # beyond max_features
        ("set_keyframe", (5, [32], [0], [1]), -1),                  # an octave that the attribute byte cannot hold
        ("set_matches", (5, [0], [0]), -1),                         # not in use
        ("set_matches", (0, [1, 1], [0, 1]), -1),                   # a feature named twice
        ("set_matches", (0, [3], [0]), -1),
        ("set_matches", (0, [1], [3]), -2),                         # beyond max_points
        ("set_matches", (0, [1], [-2]), -1),
        ("add_observations", ([1, 1], [0, 0], [1, 2]), -1),         # a pair named twice
        ("add_observations", ([1], [5], [0]), -1),
        ("add_observations", ([1], [0], [3]), -1),
        ("add_observations", ([3], [0], [0]), -2),
        ("add_observations", ([-1], [0], [0]), -1),
        ("add_observations", ([1, 0], [0, 4], [1, 1]), -2),         # the second entry overflows point 0's row: the first is taken back
        ("erase_observations", ([0, 0], [1, 1]), -1),
        ("erase_observations", ([3], [0]), -2),
        ("erase_observations", ([0], [6]), -2),
        ("erase_observations", ([0], [-1]), -1),
        ("erase_points", ([0, 0],), -1),
        ("erase_points", ([3],), -2),
        ("erase_points", ([-1],), -1),
        ("erase_keyframe", (5,), -1),
        ("erase_keyframe", (6,), -1),
    ]
    for name, args, code in table:
        assert both(pkg, g, m, name, *args) == code, (name, args)
    for call in (lambda: g.vote([3]), lambda: g.vote([-1]), lambda: g.covisibility(5), lambda: g.cull_keyframes([0, 5], [0, 0], True),
                 lambda: g.cull_keyframes([0, 1, 0], [0, 0, 0], True), lambda: g.cull_keyframes([-1], [0], True)):
        with pytest.raises(pkg.OrbxError) as e:
            call()
        assert e.value.code == -1
        same_graph(g, m, "query refusal")
    # a keyframe without a match is never culled: 0 > 0.9 * 0 fails
    same_cull(g.cull_keyframes([4], [0], True, cap=0), m.cull_keyframes([4], [0], True), "empty keyframe")
    same_graph(g, m, "end")
    # n_local == 0
    r = g.cull_keyframes([], [], True)
    assert len(r["culled"]) == 0 and len(r["bad_points"]) == 0


@pytest.mark.gpu
def test_cull_capacity_reports_the_true_count(pkg):
    case = [c for c in CULL_CASES if c["name"] == "ten_of_eleven_culled"][0]
    lim = case["scene"].limits()
    g, m = pair(pkg, lim)
    case["scene"].play(g); case["scene"].play(m)
    with pytest.raises(pkg.OrbxError) as e:
        g.cull_keyframes(case["local"], case["not_erase"], True, cap=0)
    assert e.value.code == -2 and g.last_n_bad == 1
    m.cull_keyframes(case["local"], case["not_erase"], True)
    same_graph(g, m, "the call has run")


# ------------------------------------------------------------------------------------------------ votes

def _vote_map(pkg, max_kf, slots, max_obs, seed):
    """keyframes in the given slots, 4 features each; 48 points seen by random keyframes; point 0's row full"""
    r = np.random.RandomState(seed)
    g, m = pair(pkg, (max_kf, 4, 64, max_obs))
    for k in slots:
        both(pkg, g, m, "set_keyframe", int(k), [0] * 4, [0] * 4, [1] * 4)
    free = {int(k): [0, 1, 2, 3] for k in slots}
    P, K, I = [], [], []
    for p in range(48):
        want = min(len(slots), max_obs) if p == 0 else int(r.randint(1, min(len(slots), max_obs, 9) + 1))
        open_ = sorted(k for k in free if free[k])
        if not open_:
            continue
        for k in (open_[-want:] if p == 0 else r.choice(open_, min(want, len(open_)), replace=False)):   # point 0: the highest slots
            P.append(p); K.append(int(k)); I.append(free[int(k)].pop())
    both(pkg, g, m, "add_observations", P, K, I)
    for k in sorted(set(K)):
        sel = [j for j in range(len(P)) if K[j] == k]
        both(pkg, g, m, "set_matches", k, [I[j] for j in sel], [P[j] for j in sel])
    both(pkg, g, m, "erase_points", [46, 47])
    return g, m, r


@pytest.mark.gpu
@pytest.mark.parametrize("max_kf,n_kf,max_obs", [(1, 1, 4), (65, 65, 8), (LDS_KEYFRAMES, 300, 256), (LDS_KEYFRAMES + 1, 300, 256)],
                         ids=["1kf", "65kf", "lds_limit", "beyond_lds"])
def test_votes(pkg, max_kf, n_kf, max_obs):
    slots = list(range(n_kf)) if n_kf == max_kf else sorted(set(np.linspace(0, max_kf - 1, n_kf).astype(int).tolist()))
    g, m, r = _vote_map(pkg, max_kf, slots, max_obs, max_kf)
    if max_obs == 256:
        assert len(g.read_point(0)["obs"]) == 256                   # a row at full max_obs
        assert slots[-1] == max_kf - 1 and g.vote([0])[0][max_kf - 1] == 1
    same_votes(g, m, [], "an empty list")
    same_votes(g, m, [46, 47, 46], "bad points only")
    same_votes(g, m, [63], "a slot that never was a point")
    same_votes(g, m, [0], "one point")
    same_votes(g, m, list(range(48)), "every point")
    same_votes(g, m, r.randint(0, 64, 33).tolist(), "33 points")
    same_votes(g, m, r.randint(0, 64, 9001).tolist(), "more points than one pass of the grid takes")
    for k in slots[:3] + slots[-2:]:
        same_covis(g, m, k, "covisibility")


# ------------------------------------------------------------------------------------------------ KeyFrameCulling

@pytest.mark.gpu
@pytest.mark.parametrize("case", CULL_CASES, ids=[c["name"] for c in CULL_CASES])
def test_cull_cases(pkg, case):
    lim = case["scene"].limits()
    for k, want in case.get("alone", {}).items():
        g = case["scene"].play(pkg.MapGraph(*lim))
        r = g.cull_keyframes([k], [0], case["monocular"])
        assert (int(r["culled"][0]), int(r["n_mps"][0]), int(r["n_redundant"][0])) == want
    g, m = pair(pkg, lim)
    case["scene"].play(g); case["scene"].play(m)
    same_graph(g, m, "built")
    same_cull(g.cull_keyframes(case["local"], case["not_erase"], case["monocular"]), case["expect"], case["name"])
    m.cull_keyframes(case["local"], case["not_erase"], case["monocular"])
    same_graph(g, m, "after")


N_SEEDS = 200


@pytest.fixture(scope="module")
def cull_runs():
    """the model's results on the 200 seeded maps, computed once: per seed the scene, the call, the result, the graph after it, a second
    call on that graph, and every keyframe's decision on the untouched graph"""
    runs = []
    for seed in range(N_SEEDS):
        s, local, ne, mono = random_cull_scene(seed)
        m = s.play(SlotGraph(*s.limits()))
        alone = [m.clone().cull_keyframes([k], [n], mono)["culled"][0] for k, n in zip(local, ne)]
        first = m.cull_keyframes(local, ne, mono)
        after = m.clone()
        local2 = [k for k, c in zip(local, first["culled"]) if c != 1][::-1]
        second = m.cull_keyframes(local2, [0] * len(local2), mono)
        runs.append(dict(scene=s, local=local, not_erase=ne, mono=mono, alone=alone, first=first, after=after, local2=local2, second=second, end=m))
    return runs


@pytest.mark.gpu
def test_random_cull_scenes(pkg, cull_runs):
    # on the model alone: the maps are ones on which something happens
    assert sum(1 in r["first"]["culled"] for r in cull_runs) >= N_SEEDS // 4
    assert sum(r["alone"] != r["first"]["culled"] for r in cull_runs) >= N_SEEDS // 10
    assert sum(bool(r["first"]["bad_points"]) for r in cull_runs) >= N_SEEDS // 10
    assert all(len(r["local"]) <= 12 and max(r["scene"].nfeat.values()) <= 64 for r in cull_runs)
    lim = (16, 64, max(r["scene"].limits()[2] for r in cull_runs), 8)
    g = pkg.MapGraph(*lim)
    for seed, r in enumerate(cull_runs):
        g.clear()
        r["scene"].play(g)
        same_cull(g.cull_keyframes(r["local"], r["not_erase"], r["mono"]), r["first"], (seed, "first"))
        same_graph(g, r["after"], (seed, "after the first call"))
        same_cull(g.cull_keyframes(r["local2"], [0] * len(r["local2"]), r["mono"]), r["second"], (seed, "second"))
        same_graph(g, r["end"], (seed, "after the second call"))
