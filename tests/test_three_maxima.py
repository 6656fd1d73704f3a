"""The rotation filter (ComputeThreeMaxima, reference src/ORBmatcher.cc:1687-1728) at its ties, through every kernel that scans the
histogram serially with three_maxima() (orbx_device.h): k_proj_resolve (SearchByProjection, keyframe form), k_init_resolve
(SearchForInitialization) and histogram_filter (SearchByBoW, wave and table form).  At most 40 one-to-one matches -- every point sits on
its feature and carries its descriptor -- whose angles put chosen counts into the rotation bins; each result equals the CPU oracle's."""
import functools

import numpy as np
import pytest

f32 = np.float32
SF = np.array([f32(1.2) ** i for i in range(8)], f32)
# name -> ((bin, matches in it), ...), matches kept by the filter
CASES = {
    "boundary_kept": (((7, 10), (2, 1), (9, 1)), 12),       # (float)1 < 0.1f * (float)10 is false: 0.1f * 10.0f rounds to 1.0f, the bins stay
    "second_dropped": (((4, 11), (10, 1)), 11),             # 1 < 1.1: the second bin goes, and the third with it
    "four_way_tie": (((11, 5), (3, 5), (8, 5), (5, 5)), 15),  # strict '>': the three LOWEST of four equal bins win, bin 11 goes
    "single_bin": (((6, 3),), 3),
    "no_match": ((), 0),
}


def _bins(a1, a2):
    """the rotation bin as the reference forms it (factor 1 / HISTO_LENGTH, :253-258), in fp32"""
    rot = (a1 - a2).astype(f32)
    rot = np.where(rot < 0, (rot + f32(360)).astype(f32), rot)
    b = np.floor((rot * f32(f32(1) / f32(30))).astype(f32).astype(np.float64) + 0.5).astype(np.int64)
    return np.where(b == 30, 0, b)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """n features on a 60 px lattice with distinct random descriptors; the partner of feature i has its position and descriptor (the
    complement in the case without a match) and an angle that puts the pair into its bin -> (feature side, partner side, bins)"""
    spec, _ = CASES[name]
    rng = np.random.Generator(np.random.PCG64(77))
    want = np.array([b for b, m in spec for _ in range(m)], np.int64)
    n = len(want) if len(want) else 4
    assert n <= 40
    want = rng.permutation(want) if len(want) else np.zeros(n, np.int64)
    x = (50 + 60 * (np.arange(n) % 8)).astype(f32); y = (50 + 60 * (np.arange(n) // 8)).astype(f32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ang_f = rng.uniform(0, 360, n).astype(f32)
    ang_p = ((ang_f + 30 * want + rng.uniform(-8, 8, n)) % 360).astype(f32)
    feat = dict(x=x, y=y, octave=np.zeros(n, np.int32), angle=ang_f, u_right=np.full(n, -1, f32), desc=desc, occupied=np.zeros(n, np.uint8),
                bounds=(0.0, 0.0, 640.0, 480.0))
    part = dict(feat, angle=ang_p, desc=desc if spec else ~desc)
    for a in list(feat.values()) + [ang_p, part["desc"]]:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    bins = _bins(ang_p, ang_f)
    if spec:
        assert (bins == want).all()
        assert sorted(np.bincount(bins, minlength=30)[np.bincount(bins, minlength=30) > 0], reverse=True) == sorted((m for _, m in spec), reverse=True)
    return feat, part, bins


def _kept(name):
    """the pairs the reference's filter keeps, from the bin counts alone"""
    spec, nkeep = CASES[name]
    _, _, bins = _scene(name)
    if not spec:
        return np.zeros(len(bins), bool)
    cnt = np.bincount(bins, minlength=30)
    assert [int(cnt[b]) for b, _ in spec] == [m for _, m in spec]
    top = sorted(range(30), key=lambda b: (-cnt[b], b))[:3]              # strict comparisons: among equals the lowest bin ranks first
    m1 = f32(cnt[top[0]])
    keep = [top[0]] + ([] if f32(cnt[top[1]]) < f32(0.1) * m1 else [top[1]] + ([] if f32(cnt[top[2]]) < f32(0.1) * m1 else [top[2]]))
    keep = [b for b in keep if cnt[b] > 0]
    kept = np.isin(bins, keep)
    assert kept.sum() == nkeep, (name, keep, kept.sum())
    return kept


def _proj_points(part):
    n = len(part["x"])
    return dict(u=part["x"], v=part["y"], aux=np.zeros(n, f32), level=np.zeros(n, np.int32), angle=part["angle"], view_cos=np.ones(n, f32),
                desc=part["desc"], valid=np.ones(n, np.uint8), has_obs=np.ones(n, np.uint8))


def _bow_set(side):
    n = len(side["x"])                                                   # one vocabulary node per feature: the pairs are one-to-one
    return dict(desc=side["desc"], node_id=np.arange(n, dtype=np.uint32), node_off=np.arange(n + 1, dtype=np.int32), feat=np.arange(n, dtype=np.uint32),
                flag=np.ones(n, np.uint8), angle=side["angle"], x=side["x"], y=side["y"], octave=side["octave"], u_right=side["u_right"])


_ORACLE = {}


def _expected(oracle, name):
    """the oracle's three answers, checked against the bin counts; computed once per case"""
    if name not in _ORACLE:
        feat, part, _ = _scene(name)
        kept = _kept(name)
        idx = np.where(kept, np.arange(len(kept)), -1)
        proj = oracle.search_by_projection_keyframe(feat, _proj_points(part), SF, 3.0, 100, True)
        init = oracle.search_for_initialization(part, feat, np.stack([part["x"], part["y"]], 1).astype(f32), 10, 0.9, True)
        bow = oracle.search_by_bow_kf_f(_bow_set(part), _bow_set(feat), 0.75, True)
        for m, nm in (proj, init, bow):
            assert nm == kept.sum() and (m == idx).all(), (name, nm, m)
        _ORACLE[name] = (proj, init, bow)
    return _ORACLE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_bins_and_oracle(oracle, name):
    _expected(oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_rotation_filter_at_ties(pkg, oracle, name):
    proj, init, bow = _expected(oracle, name)                            # the bin counts are checked there, before any GPU call
    feat, part, _ = _scene(name)
    got, n = pkg.ORBmatcher(0.9, True).SearchByProjectionKeyFrame(feat, _proj_points(part), SF, 3.0, 100)           # k_proj_resolve
    assert n == proj[1] and (got == proj[0]).all(), (name, "keyframe", got)
    prev = np.stack([part["x"], part["y"]], 1).astype(f32)
    got, n, _ = pkg.ORBmatcher(0.9, True).SearchForInitialization(part, feat, prev, 10)                             # k_init_resolve
    assert n == init[1] and (got == init[0]).all(), (name, "initialization", got)
    for form in ("wave", "table"):                                                                                  # histogram_filter
        pkg.orbx.debug_set_bow_form(form)
        try:
            got, n = pkg.ORBmatcher(0.75, True).SearchByBoW(_bow_set(part), _bow_set(feat))
            assert pkg.orbx.debug_bow_last_form()["form"] == form
        finally:
            pkg.orbx.debug_set_bow_form("auto")
        assert n == bow[1] and (got == bow[0]).all(), (name, form, got)
