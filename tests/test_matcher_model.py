"""The plain model of the BoW matchers (tests/matcher_model.py) on the crowded scenes (tests/matcher_scene.py), on the CPU:
the oracle equals the model on every scene and ratio, the scenes reach the classes they are there for (floors on the MODEL's class report,
conditions on the inputs alone), every listed defect of a matcher changes a result on at least one scene, and a few nodes small enough to
check by eye have their answers written out."""
import numpy as np
import pytest

import matcher_model as M
import matcher_scene as S

f32 = np.float32
GREEDY = {"kf_f": M.search_by_bow_kf_f, "kf_kf": M.search_by_bow_kf_kf}


greedy_scenes, model_greedy, tri_cases, model_tri = S.greedy_scenes, S.model_greedy, S.tri_cases, S.model_tri


# ------------------------------------------------------------------------------------------ oracle == model

@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("kind", list(GREEDY))
@pytest.mark.parametrize("scene", ["tile", "large", "edges", "passes_rows", "passes_fall", "passes_chunks"])
def test_oracle_equals_model_greedy(oracle, scene, kind, ori):
    a, b, ratios = greedy_scenes()[scene]
    for ratio in ratios:
        exp, en, _ = model_greedy(scene, kind, ratio, ori)
        got, gn = getattr(oracle, "search_by_bow_" + kind)(a, b, ratio, ori)
        assert gn == en == (exp >= 0).sum() and (got == exp).all(), (scene, kind, ratio, ori, np.nonzero(got != exp)[0][:8])
    if scene == "tile":                        # the neighbours of the batched calls
        for nb in S.s_tile()[2][1:]:
            exp, en, _ = GREEDY[kind](a, nb, 0.9, ori)
            got, gn = getattr(oracle, "search_by_bow_" + kind)(a, nb, 0.9, ori)
            assert gn == en and (got == exp).all()


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("only_stereo", [False, True])
@pytest.mark.parametrize("case", ["ab", "ba", "f0", "ab2"])
def test_oracle_equals_model_triangulation(oracle, case, only_stereo, ori):
    a, b, F = tri_cases()[case]
    exp, _ = model_tri(case, ori, only_stereo)
    ex, ey = S.s_tri()["epipole"]
    got = oracle.search_for_triangulation(a, b, F, ex, ey, S.SF, S.SIG2, 0.6, ori, only_stereo)
    assert got.shape == exp.shape and (got == exp).all(), (case, only_stereo, ori)


def test_three_maxima_against_oracle(oracle):
    """ComputeThreeMaxima restated: the oracle's on random counts with ties and on the 0.1f boundary"""
    import ctypes as C
    rng = np.random.Generator(np.random.PCG64(3))
    cases = [rng.integers(0, 4, 30) for _ in range(200)] + [rng.integers(0, 40, 30) for _ in range(200)]
    cases += [np.array([10, 1, 1] + [0] * 27), np.array([11, 1, 1] + [0] * 27), np.array([0] * 30), np.array([5] * 30), np.array([30, 3, 2] + [0] * 27)]
    for cnt in cases:
        cnt = np.ascontiguousarray(cnt, np.int32)
        i = [C.c_int(-1) for _ in range(3)]
        oracle.lib().oracle_three_maxima(cnt.ctypes.data_as(C.c_void_p), 30, *[C.byref(v) for v in i])
        assert tuple(v.value for v in i) == M.compute_three_maxima([[0] * int(c) for c in cnt]), cnt


# ------------------------------------------------------------------------------------------ the floors

@pytest.mark.parametrize("kind", list(GREEDY))
@pytest.mark.parametrize("scene", ["tile", "large"])
def test_floors_greedy(scene, kind):
    c = M.greedy_counts(model_greedy(scene, kind, 0.9, True)[2])
    print(scene, kind, c)
    assert c["steal"] >= 20 and c["rematched"] >= 5 and c["ratio_rej"] >= 20 and c["tie"] >= 10, c
    assert all(c[k] >= 5 for k in M.K_BOW2_CLASSES), c
    a, b, _ = greedy_scenes()[scene]
    rows = model_greedy(scene, kind, 0.9, True)[2]["rows"]
    lost = [r for r in rows.values() if r["k_bow2"] == "small_node" and r["steal"] and r["matched"] < 0]
    assert len(lost) >= 3                     # rows of a 1-to-3-column node that find every column taken
    big = [n for n, (r, cl) in S.node_sizes(a, b).items() if r > 64 or cl > 64]
    if scene == "large":
        assert sum(r["k_bow2"] == "scan" and r["node"] in big for r in rows.values()) >= 20
        assert sum(r["steal"] and r["node"] == 11 for r in rows.values()) >= 5       # the node over 64 on the column side only
    else:
        assert not big
    c75 = M.greedy_counts(model_greedy(scene, kind, 0.75, True)[2])
    assert c75["ratio_rej"] >= 100, c75


@pytest.mark.parametrize("kind", list(GREEDY))
def test_floors_passes(kind):
    """every part of S-passes is crowded: at least 5 steals in each pass, in the node beyond a pass and the node after it, in each chunk"""
    sc = S.s_passes()
    parts = {"rows": [(10, 12), (13, 13)], "fall": [(10, 10), (11, 11)], "chunks": [(10, 265), (266, 309)]}
    for name, (a, b) in sc.items():
        rows = model_greedy("passes_" + name, kind, 0.9, True)[2]["rows"]
        for lo, hi in parts[name]:
            assert sum(r["steal"] and lo <= r["node"] <= hi for r in rows.values()) >= 5, (name, lo, hi)
    sz = S.node_sizes(*sc["rows"])
    assert sum(r for r, _ in sz.values()) > 1024 and len(sz) == 4 and max(r for r, _ in sz.values()) <= 1024
    assert S.node_sizes(*sc["fall"])[10][0] > 1024
    assert len(S.node_sizes(*sc["chunks"])) > 256


def test_floors_triangulation():
    rep = model_tri("ab", True, False)[1]
    c = M.triangulation_counts(rep)
    print(c)
    assert c["within"] / 4 <= c["epipolar"] <= 3 * c["within"] / 4 and c["epipole"] >= 10, c
    assert c["multi"] >= 20 and c["closest_rejected"] >= 5 and c["tie_last"] >= 5 and c["d50"] >= 3, c
    assert M.triangulation_counts(model_tri("ab", True, True)[1])["matches"] >= 20
    assert len(model_tri("f0", True, False)[0]) == 0 and M.triangulation_counts(model_tri("f0", True, False)[1])["within"] == c["within"]
    r, cl = S.node_sizes(S.s_tri()["A"], S.s_tri()["B"])[10]
    assert r >= 70 and cl >= 70 and r * cl > 4096
    assert sum(x["passing"] >= 2 and x["node"] == 10 for x in rep["rows"].values()) >= 10       # the split node decides between columns too


def test_planted_rows_of_s_edges():
    """each planted group does what it was planted for"""
    a, b = S.s_edges()
    E = S.EDGE_ROWS

    def row(kind, ratio, name, i=0):
        return model_greedy("edges", kind, ratio, False)[2]["rows"][E[name][i]]
    for ratio in S.RATIOS:
        assert row("kf_f", ratio, "d50")["matched"] >= 0 and row("kf_f", ratio, "d50")["d50"]       # <= TH_LOW (:242)
        assert row("kf_kf", ratio, "d50")["matched"] < 0                                            # < TH_LOW (:644)
        for kind in GREEDY:
            assert row(kind, ratio, "d49")["matched"] >= 0 and row(kind, ratio, "d49")["d49"]
            assert row(kind, ratio, "d51")["matched"] < 0
    for kind in GREEDY:
        r = row(kind, 0.6, "3_5")
        assert r["ratio_eq"] and r["ratio_rej"] and 3.0 < float(f32(0.6)) * 5.0     # 0.6f * 5.0f rounds to 3.0f; the same product in double is above 3
        assert row(kind, 0.75, "3_5")["matched"] >= 0
        assert row(kind, 0.75, "3_4")["ratio_eq"] and row(kind, 0.75, "3_4")["ratio_rej"]
        assert row(kind, 0.75, "9_12")["ratio_eq"] and row(kind, 0.75, "9_12")["ratio_rej"]
        assert row(kind, 0.9, "3_4")["matched"] >= 0 and row(kind, 0.9, "9_12")["matched"] >= 0
        for name in ("tie_ab", "tie_ba"):
            assert row(kind, 0.9, name)["tie"] and row(kind, 0.9, name)["ratio_rej"]
            r = row(kind, S.TIE_RATIO, name)
            cols = sorted(int(j) for j in np.nonzero(M.POP[a["desc"][E[name][0]] ^ b["desc"]].sum(1) == 7)[0])
            assert len(cols) == 2 and r["matched"] == cols[0]                       # the FIRST of the two (strict <, :229)
        chain = [row(kind, 0.9, "chain", i) for i in range(5)]
        assert [r["steal"] for r in chain] == [False, True, True, True, True] and all(r["matched"] >= 0 for r in chain)
        assert [r["matched"] for r in chain] == sorted(r["matched"] for r in chain) and len({r["matched"] for r in chain}) == 5
    bins = {n: M.rotation_bin(a["angle"][E[n][0]], b["angle"][model_greedy("edges", "kf_f", 0.9, False)[2]["rows"][E[n][0]]["matched"]])
            for n in E if n.startswith("rot")}
    assert bins == {"rot15": 1, "rot45": 2, "rot345": 12, "rot75": 3, "rot354.9": 12, "rot355.1": 12, "rot-0": 0, "rot-360": 0, "rot890": 0}
    rot = f32(a["angle"][E["rot-0"][0]]) - f32(0.0)
    assert rot == 0 and np.signbit(rot)                                             # a difference of exactly -0.0
    # the filter's third maximum is bin 0, and it is the wrapped bin-30 matches that put it there
    out_on = model_greedy("edges", "kf_kf", 0.9, True)[0]
    assert all(out_on[r] >= 0 for n in ("rot890", "rot-0", "rot-360") for r in E[n]) and all(out_on[r] < 0 for r in E["rot15"])


# ------------------------------------------------------------------------------------------ the scenes tell mutants apart

def _greedy_differs(mutant, kinds=("kf_f", "kf_kf"), oris=(False, True)):
    hits = []
    for scene, (a, b, ratios) in greedy_scenes().items():
        if scene.startswith("passes"):
            continue
        for kind in kinds:
            for ratio in ratios:
                for ori in oris:
                    got = GREEDY[kind](a, b, ratio, ori, mutant={mutant})
                    ref = model_greedy(scene, kind, ratio, ori)
                    if got[1] != ref[1] or (got[0] != ref[0]).any():
                        hits.append((scene, kind, ratio, ori))
    return hits


def _tri_differs(mutant, oris=(False, True)):
    hits = []
    ex, ey = S.s_tri()["epipole"]
    for case, (a, b, F) in tri_cases().items():
        for only in (False, True):
            for ori in oris:
                got = M.search_for_triangulation(a, b, F, ex, ey, S.SF, S.SIG2, ori, only, mutant={mutant})[0]
                ref = model_tri(case, ori, only)[0]
                if got.shape != ref.shape or (got != ref).any():
                    hits.append((case, only, ori))
    return hits


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_scenes_tell_mutants_apart(mutant):
    """a matcher with this defect gives another result on at least one scene; where the defect lives in one search or in the rotation bins
    alone, it must show there"""
    if mutant == "kf_f_strict":
        hits = _greedy_differs(mutant, kinds=("kf_f",), oris=(False,))
    elif mutant == "kf_kf_le":
        hits = _greedy_differs(mutant, kinds=("kf_kf",), oris=(False,))
    elif mutant in ("no_claims", "ratio_double", "greedy_last_on_ties"):
        hits = _greedy_differs(mutant, oris=(False,))
        assert {k for _, k, _, _ in hits} == {"kf_f", "kf_kf"}, hits
    elif mutant in ("bin_half_even", "no_bin_wrap"):
        hits = _greedy_differs(mutant, oris=(True,))
        assert {k for _, k, _, _ in hits} == {"kf_f", "kf_kf"}, hits
    else:
        hits = _tri_differs(mutant, oris=(False,))
    print(mutant, hits)
    assert hits, mutant
    if mutant == "no_claims":
        assert {s for s, _, _, _ in hits} == {"tile", "large", "edges"}
    if mutant == "ratio_double":
        assert ("edges", "kf_f", 0.6, False) in hits
    if mutant == "greedy_last_on_ties":
        assert {r for _, _, r, _ in hits} == {S.TIE_RATIO}        # at a ratio <= 1 a tie at the smallest distance fails the ratio test either way


# ------------------------------------------------------------------------------------------ known answers

def _desc(*bits):
    d = np.zeros(256, np.uint8)
    d[list(bits)] = 1
    return np.packbits(d)


def _set(node_lists, desc, flag=None, angle=None, x=None, y=None, octave=None, u_right=None):
    """feature set from {node: [features]} and per-feature lists"""
    n = len(desc)
    ids = sorted(node_lists)
    off = np.cumsum([0] + [len(node_lists[i]) for i in ids]).astype(np.int32)
    z = np.zeros(n, f32)
    return dict(desc=np.stack(desc), node_id=np.array(ids, np.uint32), node_off=off, feat=np.array([j for i in ids for j in node_lists[i]], np.uint32),
                flag=np.array(flag if flag is not None else [1] * n, np.uint8), angle=np.array(angle, f32) if angle is not None else z,
                x=np.array(x, f32) if x is not None else z, y=np.array(y, f32) if y is not None else z,
                octave=np.array(octave, np.int32) if octave is not None else np.zeros(n, np.int32),
                u_right=np.array(u_right, f32) if u_right is not None else z - 1)


def _bits(n, start=0):
    return _desc(*range(start, start + n))


def test_known_answers_greedy(oracle):
    """hand-built nodes; descriptors are given by the bits they set, so a distance is the size of a symmetric difference

    node 1  rows 0, 1 and columns 0, 1, 2.  Row 0 = {} is at 1 / 2 / 40 from the columns, row 1 = {0} at 0 / 3 / 39.  Row 0 takes column 0
            (1 < 0.9 * 2); row 1 would take it too (0 < anything) but finds it taken: 3 < 0.9 * 39 -> column 1.  Without claims both rows
            end on column 0 and the later one wins the slot.
    node 2  row 2 against columns 3, 4 at 50 and 90: matched in (KF,F), not in (KF,KF)
    node 3  row 3 against columns 5, 6 at 3 and 4: 3 < 0.9f * 4 holds, 3 < 0.75f * 4 does not
    node 4  row 4 has no map point: its perfect column 7 stays free;  node 5 is in the first set only, node 6 in the second only
    node 7  (KF,KF) only differs: column 8 at distance 2 has no map point, column 9 at 10 has one -> (KF,F) takes 8, (KF,KF) takes 9"""
    A = _set({1: [0, 1], 2: [2], 3: [3], 4: [4], 5: [5], 7: [6]},
             [_bits(0), _bits(1), _bits(0), _bits(0), _bits(7), _bits(9), _bits(0)], flag=[1, 1, 1, 1, 0, 1, 1])
    B = _set({1: [0, 1, 2], 2: [3, 4], 3: [5, 6], 4: [7], 6: [10], 7: [8, 9]},
             [_bits(1), _bits(2, 1), _bits(40), _bits(50), _bits(90), _bits(3), _bits(4), _bits(7), _bits(2), _bits(10), _bits(9)],
             flag=[1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1])
    want = {("kf_f", 0.9): [0, 1, -1, 2, -1, 3, -1, -1, 6, -1, -1], ("kf_f", 0.75): [0, 1, -1, 2, -1, -1, -1, -1, 6, -1, -1],
            ("kf_kf", 0.9): [0, 1, -1, 5, -1, -1, 9], ("kf_kf", 0.75): [0, 1, -1, -1, -1, -1, 9]}
    for (kind, ratio), exp in want.items():
        got, n, _ = GREEDY[kind](A, B, ratio, False)
        assert got.tolist() == exp and n == sum(v >= 0 for v in exp), (kind, ratio, got.tolist())
        og, on = getattr(oracle, "search_by_bow_" + kind)(A, B, ratio, False)
        assert og.tolist() == exp and on == n
    assert M.search_by_bow_kf_f(A, B, 0.9, False, mutant={"no_claims"})[0].tolist()[:2] == [1, -1]


def test_known_answers_orientation(oracle):
    """12 one-to-one pairs (one node each, identical descriptors).  a2 = 0 throughout; a1 = 10 x 100 (bin 3), 15 (0.5 -> bin 1), 890 (29.67 ->
    bin 30 -> 0): the maxima are bins 3, 0, 1 with 10, 1, 1 matches, and (float)1 < 0.1f * (float)10 is false: everything stays.  With an
    eleventh pair in bin 3 the test reads 1 < 1.1: bins 0 and 1 go."""
    for n3, kept in ((10, 12), (11, 11)):
        n = n3 + 2
        desc = [_bits(3 * i + 1) for i in range(n)]
        A = _set({i + 1: [i] for i in range(n)}, desc, angle=[100.0] * n3 + [15.0, 890.0])
        B = _set({i + 1: [i] for i in range(n)}, desc, angle=[0.0] * n)
        exp = list(range(n)) if kept == n else list(range(n3)) + [-1, -1]
        for kind in GREEDY:
            got, cnt, _ = GREEDY[kind](A, B, 0.9, True)
            assert got.tolist() == exp and cnt == kept, (kind, n3, got.tolist())
            og, on = getattr(oracle, "search_by_bow_" + kind)(A, B, 0.9, True)
            assert og.tolist() == exp and on == kept


def test_known_answers_triangulation(oracle):
    """one node, F12 of a pure x-translation (the epipolar line of (x, y) is the row y: a = 0, b = 1, c = -y, dsqr = (y2 - y1)^2 against
    3.84 * sigma2), octave 0 (sigma2 = 1, radius^2 of the epipole test 100), epipole (100, 100).  Row 0 = {} at (50, 20), monocular:
      column 0 at distance 10, y = 23: 9 >= 3.84 -> rejected by the line           column 1 at 20, y = 21: passes -> best so far
      column 2 at 20, y = 19: passes and dist <= bestDist replaces -> row 0 ends on column 2 (the LAST of the tie)
      column 3 at 30: too far by then                                              column 4 at 5 but it has a map point
    Row 1 = {} at (95, 101), monocular: column 5 at distance 8, (104, 101): 4^2 + 1 < 100 -> too close to the epipole; column 6, the same
    place and distance but stereo: no epipole test, matches.  Row 2 at (50, 60): column 7 at distance exactly 50 on the line -> accepted.
    Row 3 has a map point.  Every row is monocular: bOnlyStereo leaves nothing.  A bestDist that moved before the line test would drop rows 0 and
    2: column 0 (distance 10, off the line) would shut out everything farther."""
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
    A = _set({1: [0, 1, 2, 3]}, [_bits(0)] * 4, flag=[0, 0, 0, 1], x=[50, 95, 50, 50], y=[20, 101, 60, 20], u_right=[-1, -1, -1, -1])
    B = _set({1: list(range(8))}, [_bits(10), _bits(20), _bits(20, 30), _bits(30, 100), _bits(5), _bits(8, 200), _bits(8, 210), _bits(50, 150)],
             flag=[0, 0, 0, 0, 1, 0, 0, 0], x=[50, 50, 50, 50, 50, 104, 104, 50], y=[23, 21, 19, 20, 20, 101, 101, 60],
             u_right=[-1, -1, -1, -1, -1, -1, 7, -1])
    sf = np.ones(8, f32); sg = np.ones(8, f32)
    # row 0 also sees columns 5-7 (distances 8, 8, 50) but they are off its line; row 1 sees columns 0-3 off its line, row 2 likewise
    exp = [[0, 2], [1, 6], [2, 7]]
    got, rep = M.search_for_triangulation(A, B, F, 100.0, 100.0, sf, sg, False, False)
    assert got.tolist() == exp, got.tolist()
    assert rep["rows"][0]["closest_rejected"] and rep["rows"][0]["tie_last"] and rep["rows"][2]["d50"] and rep["rows"][1]["epipole"] == 1
    assert oracle.search_for_triangulation(A, B, F, 100.0, 100.0, sf, sg, 0.6, False, False).tolist() == exp
    assert len(M.search_for_triangulation(A, B, F, 100.0, 100.0, sf, sg, False, True)[0]) == 0
    assert len(oracle.search_for_triangulation(A, B, F, 100.0, 100.0, sf, sg, 0.6, False, True)) == 0
    assert M.search_for_triangulation(A, B, F, 100.0, 100.0, sf, sg, False, False, mutant={"tri_first_on_ties"})[0].tolist()[0] == [0, 1]
    assert M.search_for_triangulation(A, B, F, 100.0, 100.0, sf, sg, False, False, mutant={"tri_bestdist_before_epipolar"})[0].tolist() == [[1, 6]]


def test_db_scene_is_crowded(oracle):
    """the keyframe set of the BowDatabase tests: every (frame, keyframe) pair has steals, and the model equals the oracle on it"""
    frames, kfs = S.s_db(oracle)
    for i, f in enumerate(frames):
        for k, kf in enumerate(kfs):
            exp, n, rep = M.search_by_bow_kf_f(kf, f, 0.9, True)
            c = M.greedy_counts(rep)
            assert c["steal"] >= 5 and c["ratio_rej"] >= 5 and n >= 10, (i, k, c)
            got, gn = oracle.search_by_bow_kf_f(kf, f, 0.9, True)
            assert gn == n and (got == exp).all(), (i, k)
