"""Every device form of the BoW matchers on the crowded scenes of tests/matcher_scene.py, bit-equal to the plain model
(tests/matcher_model.py) AND to the CPU oracle.  On these scenes rows compete for columns, distances tie and sit on TH_LOW, the ratio test
decides and lands on exact float equalities, and k_bow2's rows fall into each of its classes (the floors are asserted on the CPU, in
tests/test_matcher_model.py): a form that skipped claims, compared with the wrong sign, evaluated the ratio in double, broke ties towards
the wrong column or never took its re-walk branch fails here.

Which form ran: the kernels of orbx_bow.hip report it (orbx_debug_bow_last_form); k_match picks its tile or large-node form per node from
the node's size alone (at most 64 x 64 or not), so for it the scenes' node sizes are asserted, together with the fact that no kernel of
orbx_bow.hip was launched in its place.  Every process-wide hook is put back in `finally`."""
import numpy as np
import pytest

import matcher_model as M
import matcher_scene as S

pytestmark = pytest.mark.gpu
KINDS = ("kf_f", "kf_kf")


def _kf(s):
    return dict(s, kind="keyframe")


def _search(m, kind, a, b):
    return m.SearchByBoW(a, b) if kind == "kf_f" else m.SearchByBoW(a, _kf(b))


def _expect(oracle, scene, kind, ratio, ori):
    """the model's answer, checked against the oracle's"""
    a, b, _ = S.greedy_scenes()[scene]
    exp, n, _ = S.model_greedy(scene, kind, ratio, ori)
    og, on = getattr(oracle, "search_by_bow_" + kind)(a, b, ratio, ori)
    assert on == n and (og == exp).all(), ("oracle vs model", scene, kind, ratio, ori)
    return exp, n


def _same(got, exp, tag):
    g, gn = got
    e, en = exp
    assert gn == en and (np.asarray(g) == e).all(), (tag, int(gn), int(en), np.nonzero(np.asarray(g) != e)[0][:8].tolist())


def _tiny():
    d = np.zeros((1, 32), np.uint8)
    return dict(desc=d, node_id=np.array([1], np.uint32), node_off=np.array([0, 1], np.int32), feat=np.zeros(1, np.uint32), flag=np.ones(1, np.uint8),
                angle=np.zeros(1, np.float32))


def _mark_last_form_table(pkg):
    """leaves "table" as the last form bow_launch reports: a later call that fell back to the kernels of orbx_bow.hip on its own (one pair:
    the wave form) would change it"""
    pkg.orbx.debug_set_bow_form("table")
    try:
        got, n = pkg.ORBmatcher(0.9, False).SearchByBoW(_tiny(), _tiny())
    finally:
        pkg.orbx.debug_set_bow_form("auto")
    assert n == 1 and got.tolist() == [0]
    assert pkg.orbx.debug_bow_last_form() == dict(form="table", xcd_grid=False, compact=False)


# ------------------------------------------------------------------------------------------ k_match, per call

@pytest.mark.parametrize("in_memory", [False, True])
@pytest.mark.parametrize("scene", ["tile", "edges", "large"])
def test_percall_forms(pkg, oracle, scene, in_memory):
    """ORBmatcher.SearchByBoW, both kinds, items by value and in memory: S-tile and S-edges run k_match's tile fixpoint in every node,
    S-large its large-node form in the nodes over 64 (one of them over 64 on the column side only) and the tile form in the small ones"""
    a, b, ratios = S.greedy_scenes()[scene]
    big = [n for n, (r, c) in S.node_sizes(a, b).items() if r > 64 or c > 64]
    assert (len(big) == 3 and max(max(v) for v in S.node_sizes(a, b).values()) < 4096) if scene == "large" else not big
    _mark_last_form_table(pkg)
    pkg.orbx.debug_set_match_items(in_memory)
    try:
        for ratio in ratios:
            for ori in (True, False):
                m = pkg.ORBmatcher(ratio, ori)
                for kind in KINDS:
                    _same(_search(m, kind, a, b), _expect(oracle, scene, kind, ratio, ori), (scene, kind, ratio, ori, in_memory))
    finally:
        pkg.orbx.debug_set_match_items(False)
    assert pkg.orbx.debug_bow_last_form() == dict(form="table", xcd_grid=False, compact=False)     # no launch of orbx_bow.hip in between


def test_percall_batches(pkg, oracle):
    """SearchByBoWBatch (every neighbour against one frame) and SearchByBoWKeyFrames (one keyframe against every neighbour) on the three
    unequal neighbours of S-tile"""
    a, _, nbs = S.s_tile()
    assert sorted(len(n["desc"]) for n in nbs) != [len(nbs[0]["desc"])] * 3
    _mark_last_form_table(pkg)
    for ratio, ori in ((0.9, True), (0.75, True), (0.9, False)):
        m = pkg.ORBmatcher(ratio, ori)
        got, n = m.SearchByBoWBatch(nbs, a)
        for i, nb in enumerate(nbs):
            exp = M.search_by_bow_kf_f(nb, a, ratio, ori)[:2]
            _same(oracle.search_by_bow_kf_f(nb, a, ratio, ori), exp, ("oracle", i))
            _same((got[i], n[i]), exp, ("SearchByBoWBatch", i, ratio, ori))
        got, n = m.SearchByBoWKeyFrames(a, nbs)
        for i, nb in enumerate(nbs):
            exp = M.search_by_bow_kf_kf(a, nb, ratio, ori)[:2]
            _same(oracle.search_by_bow_kf_kf(a, nb, ratio, ori), exp, ("oracle", i))
            _same((got[i, :len(a["desc"])], n[i]), exp, ("SearchByBoWKeyFrames", i, ratio, ori))
    assert pkg.orbx.debug_bow_last_form() == dict(form="table", xcd_grid=False, compact=False)


# ------------------------------------------------------------------------------------------ k_bow_wave / k_bow2, forced

@pytest.mark.parametrize("form", ["wave", "table"])
@pytest.mark.parametrize("scene", ["tile", "edges", "large", "passes_rows", "passes_fall", "passes_chunks"])
def test_bow_forms(pkg, oracle, scene, form):
    """node_greedy_wave (k_bow_wave) and k_bow2's three-smallest-keys fixpoint with its re-walk, its `complete` shortcut, several passes
    per chunk, the fall_list path and a second chunk, at every ratio: 0.1 makes best2 = 256 decide (k_bow2 substitutes it by rule)"""
    a, b, ratios = S.greedy_scenes()[scene]
    ratios = tuple(ratios) + tuple(r for r in S.RATIOS + (0.1,) if r not in ratios)
    pkg.orbx.debug_set_bow_form(form)
    try:
        for ratio in ratios:
            for ori in (True, False) if ratio == 0.9 else (True,):
                m = pkg.ORBmatcher(ratio, ori)
                for kind in KINDS:
                    got = _search(m, kind, a, b)
                    assert pkg.orbx.debug_bow_last_form() == dict(form=form, xcd_grid=False, compact=False)
                    _same(got, _expect(oracle, scene, kind, ratio, ori), (scene, form, kind, ratio, ori))
    finally:
        pkg.orbx.debug_set_bow_form("auto")


# ------------------------------------------------------------------------------------------ BowDatabase

class Db:
    """the frames of S-db resident in a BowFrames (FeatureVector by the device vocabulary), the keyframes in a BowDatabase"""

    def __init__(self, pkg, oracle):
        import torch
        self.torch = torch
        raw = S.s_db_raw()
        self.frames, self.kfs = S.s_db(oracle)
        B = len(S.DB_COUNTS)
        kps = np.zeros((B, S.DB_CAP, 7), np.float32)
        kps[:, :, 3] = raw["angle"]
        self.d_kps = torch.from_numpy(kps).cuda(); self.d_desc = torch.from_numpy(raw["desc"]).cuda()
        self.d_n = torch.tensor(S.DB_COUNTS, dtype=torch.int32, device="cuda")
        self.stream = torch.cuda.Stream(); self.st = self.stream.cuda_stream
        self.voc = pkg.ORBVocabulary(4, 2, *raw["voc"])
        self.fr = pkg.BowFrames(B, S.DB_CAP)
        torch.cuda.synchronize()
        self.fr.transform(self.voc, self.d_kps.data_ptr(), self.d_desc.data_ptr(), self.d_n.data_ptr(), B, 1, self.st)
        self.stream.synchronize()
        for i, f in enumerate(self.frames):                       # the device's FeatureVector is the one the model is given
            t = self.fr.read(i, self.st)
            assert (t["fv_node_id"] == f["node_id"]).all() and (t["fv_node_off"] == f["node_off"]).all() and (t["fv_feat"] == f["feat"]).all()
        self.db = pkg.BowDatabase(self.kfs)
        self.expect = {}

    def want(self, oracle, i, k, ratio, ori):
        key = (i, k, ratio, ori)
        if key not in self.expect:
            exp, n, _ = M.search_by_bow_kf_f(self.kfs[k], self.frames[i], ratio, ori)
            og, on = oracle.search_by_bow_kf_f(self.kfs[k], self.frames[i], ratio, ori)
            assert on == n and (og == exp).all()
            self.expect[key] = (exp, n)
        return self.expect[key]


@pytest.fixture(scope="module")
def db(pkg, oracle):
    return Db(pkg, oracle)


@pytest.mark.parametrize("ratio,ori", [(0.9, True), (0.75, True), (0.9, False)])
def test_bow_database(pkg, oracle, db, ratio, ori):
    """BowDatabase.search (host frame), the dense batch search in the wave form and in the table form on the XCD-owned grid (9 keyframes x 2
    frames), the compact lists with a capacity above every count and one below (the model's first entries in slot order), and the
    candidate lists"""
    torch = db.torch
    B, NKF, CAP = len(S.DB_COUNTS), S.DB_NKF, S.DB_CAP
    for i in range(B):
        got, n = db.db.search(db.frames[i], ratio, ori)
        for k in range(NKF):
            _same((got[k], n[k]), db.want(oracle, i, k, ratio, ori), ("BowDatabase.search", i, k))
    for form, xcd in (("wave", False), ("table", True)):
        d_m = torch.full((B, NKF, CAP), -7, dtype=torch.int32, device="cuda"); d_n = torch.full((B, NKF), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        pkg.orbx.debug_set_bow_form(form)
        try:
            db.fr.search(db.db, B, d_m.data_ptr(), d_n.data_ptr(), ratio, ori, db.st)
            db.stream.synchronize()
            assert pkg.orbx.debug_bow_last_form() == dict(form=form, xcd_grid=xcd, compact=False)
        finally:
            pkg.orbx.debug_set_bow_form("auto")
        m = d_m.cpu().numpy(); nm = d_n.cpu().numpy()
        for i in range(B):
            for k in range(NKF):
                _same((m[i, k, :S.DB_COUNTS[i]], nm[i, k]), db.want(oracle, i, k, ratio, ori), ("dense", form, i, k))
                assert (m[i, k, S.DB_COUNTS[i]:] == -7).all()
    counts = [db.want(oracle, i, k, ratio, ori)[1] for i in range(B) for k in range(NKF)]
    small = max(min(counts) // 2, 1)
    assert small < max(counts) and (ratio != 0.9 or small < min(counts))       # the small capacity cuts lists: at 0.9 every one of them
    for cap_pairs in (CAP, small):
        d_p = torch.full((B, NKF, cap_pairs, 2), -7, dtype=torch.int32, device="cuda"); d_n = torch.full((B, NKF), -9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        db.fr.search_compact(db.db, B, d_p.data_ptr(), cap_pairs, d_n.data_ptr(), ratio, ori, db.st)
        db.stream.synchronize()
        assert pkg.orbx.debug_bow_last_form() == dict(form="table", xcd_grid=True, compact=True)
        lst = d_p.cpu().numpy(); nm = d_n.cpu().numpy()
        for i in range(B):
            for k in range(NKF):
                exp, en = db.want(oracle, i, k, ratio, ori)
                slots = np.nonzero(exp >= 0)[0]
                want = np.stack([slots, exp[slots]], 1).astype(np.int32)[:cap_pairs]
                assert nm[i, k] == en and (lst[i, k, :len(want)] == want).all() and (lst[i, k, len(want):] == -7).all(), ("compact", cap_pairs, i, k)
    # the candidate lists: ids are indices; a duplicate, the last keyframe, an id out of range
    stride = 4
    lists = [[8, 0, 8, 3], [5, 99, 1, 0]]
    ncand = [4, 3]
    d_c = torch.tensor(lists, dtype=torch.int32, device="cuda"); d_nc = torch.tensor(ncand, dtype=torch.int32, device="cuda")
    d_m = torch.full((B, stride, CAP), -7, dtype=torch.int32, device="cuda"); d_n = torch.full((B, stride), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    db.fr.search_candidates(db.db, B, d_c.data_ptr(), stride, d_nc.data_ptr(), d_m.data_ptr(), d_n.data_ptr(), ratio, ori, stream=db.st)
    db.stream.synchronize()
    m = d_m.cpu().numpy(); nm = d_n.cpu().numpy()
    for i in range(B):
        for j in range(stride):
            k = lists[i][j]
            if j >= ncand[i] or not 0 <= k < NKF:
                assert nm[i, j] == -1 and (m[i, j] == -7).all(), (i, j)
            else:
                _same((m[i, j, :S.DB_COUNTS[i]], nm[i, j]), db.want(oracle, i, k, ratio, ori), ("candidates", i, j, k))


# ------------------------------------------------------------------------------------------ resident keyframes

def test_resident_keyframes(pkg, oracle):
    """one call each of the resident-keyframe searches: S-tile for the two SearchByBoW, S-tri for the triangulation"""
    a, b, nbs = S.s_tile()
    da, db_ = pkg.DeviceKeyFrame(a), pkg.DeviceKeyFrame(b)
    dn = [pkg.DeviceKeyFrame(n) for n in nbs]
    for ratio, ori in ((0.9, True), (0.75, False)):
        m = pkg.ORBmatcher(ratio, ori)
        _same(m.SearchByBoWResident(da, a["flag"], db_), _expect(oracle, "tile", "kf_f", ratio, ori), ("SearchByBoWResident", ratio, ori))
        got, n = m.SearchByBoWKeyFramesFrameResident(dn, [x["flag"] for x in nbs], a)
        for i, nb in enumerate(nbs):
            exp = M.search_by_bow_kf_f(nb, a, ratio, ori)[:2]
            _same(oracle.search_by_bow_kf_f(nb, a, ratio, ori), exp, ("oracle", i))
            _same((got[i], n[i]), exp, ("SearchByBoWKeyFramesFrameResident", i, ratio, ori))
        got, n = m.SearchByBoWKeyFramesResident(da, a["flag"], dn, [x["flag"] for x in nbs])
        for i, nb in enumerate(nbs):
            exp = M.search_by_bow_kf_kf(a, nb, ratio, ori)[:2]
            _same(oracle.search_by_bow_kf_kf(a, nb, ratio, ori), exp, ("oracle", i))
            _same((got[i], n[i]), exp, ("SearchByBoWKeyFramesResident", i, ratio, ori))


# ------------------------------------------------------------------------------------------ triangulation

def _tri_expect(oracle, case, ori, only_stereo):
    a, b, F = S.tri_cases()[case]
    exp = S.model_tri(case, ori, only_stereo)[0]
    ex, ey = S.s_tri()["epipole"]
    og = oracle.search_for_triangulation(a, b, F, ex, ey, S.SF, S.SIG2, 0.6, ori, only_stereo)
    assert og.shape == exp.shape and (og == exp).all(), ("oracle vs model", case, ori, only_stereo)
    return exp


def _same_pairs(got, exp, tag):
    assert got.shape == exp.shape and (got == exp).all(), (tag, got.shape, exp.shape)


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("only_stereo", [False, True])
def test_triangulation(pkg, oracle, only_stereo, ori):
    """k_match<2> on S-tri: single calls (items by value and in memory), the batch and the resident call over the neighbours (B with F12, B
    with F12 = 0, the smaller B2), and the pair seen the other way round.  Node 10 (80 x 75 features) is split by rows over several items"""
    t = S.s_tri()
    ex, ey = t["epipole"]
    r, c = S.node_sizes(t["A"], t["B"])[10]
    assert r * c > 4096
    m = pkg.ORBmatcher(0.6, ori)
    for in_memory in (False, True):
        pkg.orbx.debug_set_match_items(in_memory)
        try:
            for case in ("ab", "ba", "f0", "ab2"):
                a, b, F = S.tri_cases()[case]
                got = m.SearchForTriangulation(a, b, F, ex, ey, S.SF, S.SIG2, bOnlyStereo=only_stereo)
                _same_pairs(got, _tri_expect(oracle, case, ori, only_stereo), ("single", case, in_memory))
        finally:
            pkg.orbx.debug_set_match_items(False)
    cases = ("ab", "f0", "ab2")
    nbs = [S.tri_cases()[k][1] for k in cases]
    Fs = [S.tri_cases()[k][2] for k in cases]
    eps = [(ex, ey)] * 3
    got = m.SearchForTriangulationBatch(t["A"], nbs, Fs, eps, S.SF, S.SIG2, bOnlyStereo=only_stereo)
    for i, case in enumerate(cases):
        _same_pairs(got[i], _tri_expect(oracle, case, ori, only_stereo), ("batch", case))
    assert len(got[1]) == 0 and (only_stereo or len(got[0]) > 100)
    da = pkg.DeviceKeyFrame(t["A"])
    dn = [pkg.DeviceKeyFrame(n) for n in nbs]
    got = m.SearchForTriangulationResident(da, t["A"]["flag"], dn, [n["flag"] for n in nbs], Fs, eps, S.SF, S.SIG2, bOnlyStereo=only_stereo)
    for i, case in enumerate(cases):
        _same_pairs(got[i], _tri_expect(oracle, case, ori, only_stereo), ("resident", case))
