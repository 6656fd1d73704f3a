"""Frame::ComputeStereoMatches (src/Frame.cc:577-751) against the independent numpy model of tests/orb_model.py, bit for bit: the
oracle stage oracle_stereo_match on the CPU, the kernels k_stereo_prep / k_stereo / stereo_cut on the GPU.

Besides two textured pairs, every call here is DIRECTED: caller-supplied keypoints and descriptors over the real pyramids of a
640 x 480 synth.stereo_pair, edited in copies of the extracted arrays so that a value sits exactly on each predicate boundary of
the reference (disparity range, octave +-1, row band ends, Hamming threshold and ties, window limits, zero disparity, the median
cut) and so that more than 2048 left keypoints reach the tail loops of stereo_cut.  A probe is a left keypoint whose descriptor is
replaced by a random one (no other right keypoint comes near it) plus right keypoints made for it, whose descriptors are the
probe's with an exact number of bits flipped.  Each group asserts IN THE MODEL that both sides of its boundary occur at least three
times: a group that cannot reach its edge fails instead of passing empty."""
import numpy as np
import pytest

import orb_model
from orb_model import ACCEPTED, COARSE_FAIL, CUT, NO_CANDIDATE, SHIFT_EDGE, WINDOW_OUT
from tools import synth

W, H, NF = 640, 480, 1000
CFG = (NF, 1.2, 8, 20, 7)
BF, MIN_Z = 386.1448, 386.1448 / 718.856     # Examples/Stereo/KITTI00-02.yaml:8,25
SEED = 104
F32 = np.float32
PATCHES = [(150 + 70 * i, 60 + 75 * i) for i in range(5)]      # centres (column, row) of the zero-disparity patches


def _directed_pair():
    """a pair with disparities 2..12 px (so that uR == uL can still be refined), plus five patches that are identical in both eyes
    at the same place (zero disparity) and left-right symmetric about their centre column"""
    left, right, disp = synth.stereo_pair(SEED, W, H, dmin=2, dmax=12)
    rng = np.random.Generator(np.random.PCG64(SEED + 1))
    left, right = left.copy(), right.copy()
    for c, r in PATCHES:
        half = rng.integers(20, 236, (21, 13)).astype(np.uint8)                    # columns c .. c+12
        patch = np.concatenate([half[:, :0:-1], half], axis=1)                       # columns c-12 .. c+12, mirror image about c
        left[r - 10:r + 11, c - 12:c + 13] = patch
        right[r - 10:r + 11, c - 12:c + 13] = patch
    return left, right, disp


class Base:
    def __init__(self, oracle, left, right, disp):
        self.left, self.right, self.disp = left, right, disp
        self.oL, self.oR = oracle.Oracle(*CFG), oracle.Oracle(*CFG)
        self.kL, self.dL = self.oL.extract(left)
        self.kR, self.dR = self.oR.extract(right)
        self.sf, self.isf = self.oL.scale_factors(), self.oL.inv_scale_factors()
        self.levels_L = [self.oL.level(l) for l in range(CFG[2])]
        self.levels_R = [self.oR.level(l) for l in range(CFG[2])]

    def run(self, oracle, kL, dL, kR, dR, bf=BF, min_z=MIN_Z):
        """one call through the model and through the oracle -> dict"""
        mu, mz, info = orb_model.stereo_model(self.levels_L, self.levels_R, self.sf, self.isf, kL, dL, kR, dR, bf, min_z)
        ou, oz = oracle.stereo_match(self.oL, self.oR, kL, dL, kR, dR, bf, min_z)
        return dict(kL=kL, dL=dL, kR=kR, dR=dR, bf=bf, min_z=min_z, mu=mu, mz=mz, info=info, ou=ou, oz=oz)


class Edit:
    """copies of the extracted arrays and the probes placed in them"""

    def __init__(self, base, seed):
        self.b = base
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.kL, self.dL, self.kR, self.dR = base.kL.copy(), base.dL.copy(), base.kR.copy(), base.dR.copy()
        self.free_r = sorted(self.rng.permutation(len(self.kR))[:400].tolist())      # right keypoints that may be overwritten
        self.used_l = set()
        self.probes = []

    def true_disparity(self, i, margin=3.0):
        """the generator's disparity at left keypoint i, or None where the middle of its SAD window (+-3 of +-5 level rows) straddles two
        disparity bands or it nears a border"""
        k = self.kL[i]; s = float(self.b.sf[k["octave"]])
        lo, hi = int(k["y"] - margin * s - 1), int(k["y"] + margin * s + 1)
        if lo < 0 or hi >= H or self.b.disp[lo] != self.b.disp[hi] or not 100 <= k["x"] <= W - 100:
            return None
        for c, r in PATCHES:
            if abs(k["x"] - c) < 40 + 8 * s and abs(k["y"] - r) < 20 + 8 * s:
                return None
        return int(self.b.disp[int(k["y"])])

    def pick_left(self, n, ok=lambda i, d: True):
        """n unused extracted left keypoints with a well-defined true disparity that satisfy ok(index, disparity)"""
        out = []
        for i in self.rng.permutation(len(self.kL)).tolist():
            if i in self.used_l:
                continue
            d = self.true_disparity(i)
            if d is not None and ok(i, d):
                out.append((i, d)); self.used_l.add(i)
                if len(out) == n:
                    return out
        raise AssertionError(f"only {len(out)} of {n} suitable left keypoints")

    def take_left(self):
        """an unused left slot for a keypoint placed by hand"""
        for i in self.rng.permutation(len(self.kL)).tolist():
            if i not in self.used_l:
                self.used_l.add(i)
                return i

    def unique(self, il):
        self.dL[il] = self.rng.integers(0, 256, 32, dtype=np.uint8)
        return self.dL[il].copy()

    def flipped(self, desc, nbits):
        bits = np.unpackbits(desc)
        bits[self.rng.choice(256, nbits, replace=False)] ^= 1
        return np.packbits(bits)

    def right(self, x, y, octave, desc, slot=None):
        ir = self.free_r.pop(0) if slot is None else slot
        self.kR["x"][ir] = F32(x); self.kR["y"][ir] = F32(y); self.kR["octave"][ir] = octave
        self.dR[ir] = desc
        return ir

    def probe(self, kind, il, ir, **kw):
        self.probes.append(dict(kind=kind, il=il, ir=ir, **kw))

    def arrays(self):
        return self.kL, self.dL, self.kR, self.dR


def _sites(img, rows, x_lo, x_hi, n, sep=14):
    """n columns in [x_lo, x_hi) with the most horizontal structure in the 11-px windows centred on them over `rows`"""
    g = np.abs(np.diff(img[rows].astype(np.int64), axis=1)).sum(axis=0)
    e = np.convolve(g, np.ones(11, np.int64), mode="same")
    order = [int(x) for x in np.argsort(-e, kind="stable") if x_lo <= x < x_hi]
    out = []
    for x in order:
        if all(abs(x - o) >= sep for o in out):
            out.append(x)
            if len(out) == n:
                break
    assert len(out) == n
    return out


# ---------------------------------------------------------------------------------------------------- the directed groups

def group_disparity_range(b):
    """1: uR == minU and uR == maxU are accepted, one fp32 step outside either bound is not (src/Frame.cc:649)"""
    e = Edit(b, 1)
    d_max = int(b.disp.max())
    min_z = 0.5
    bf = (d_max + 1.5) * min_z
    max_d = F32(bf) / F32(min_z)                                     # 1.5 px above the largest true disparity
    for i, d in e.pick_left(12, lambda i, d: d == d_max):
        k = e.kL[i]; u = e.unique(i)
        min_u = F32(k["x"]) - max_d
        inside = len([p for p in e.probes if p["kind"].startswith("minU")]) % 2 == 0
        x = min_u if inside else np.nextafter(min_u, F32(-np.inf), dtype=F32)
        e.probe("minU_in" if inside else "minU_out", i, e.right(x, k["y"], k["octave"], e.flipped(u, 20)), d=d)
    for i, d in e.pick_left(12, lambda i, d: d / float(b.sf[e.kL["octave"][i]]) <= 3.5):
        k = e.kL[i]; u = e.unique(i)
        inside = len([p for p in e.probes if p["kind"].startswith("maxU")]) % 2 == 0
        x = F32(k["x"]) if inside else np.nextafter(F32(k["x"]), F32(np.inf), dtype=F32)
        e.probe("maxU_in" if inside else "maxU_out", i, e.right(x, k["y"], k["octave"], e.flipped(u, 20)), d=d)
    return e, bf, min_z


def group_octave_and_band(b):
    """2: right octave = left +-1 accepted, +-2 rejected (:644), also at left levels 0 and nlevels-1; left row equal to a right
    keypoint's minr / maxr accepted, one row beyond rejected (:599-603); bands clipped at rows 0 and h-1"""
    e = Edit(b, 2)
    top = CFG[2] - 1
    for delta in (-2, -1, 1, 2):
        for i, d in e.pick_left(4, lambda i, d: 2 <= e.kL["octave"][i] <= top - 2):
            k = e.kL[i]; u = e.unique(i)
            e.probe(f"octave{delta:+d}", i, e.right(k["x"] - d, k["y"], k["octave"] + delta, e.flipped(u, 10)), d=d)
    for lvl, deltas in ((0, (1, 2)), (top, (-1, -2))):
        for delta in deltas:
            for i, d in e.pick_left(4, lambda i, d: e.kL["octave"][i] == lvl):
                k = e.kL[i]; u = e.unique(i)
                e.probe(f"octave{delta:+d}", i, e.right(k["x"] - d, k["y"], lvl + delta, e.flipped(u, 10)), d=d, end=lvl)
    for lvl in (0, 1, 3, top - 1, top):                                # the row band of a right keypoint of octave lvl or lvl + 1
        for which in ("minr", "minr_out", "maxr", "maxr_out"):
            for i, d in e.pick_left(2, lambda i, d: e.kL["octave"][i] == lvl and 40 < e.kL["y"][i] < H - 40):
                k = e.kL[i]; u = e.unique(i)
                o_r = min(lvl + (len(e.probes) & 1), top)
                r = F32(2.0) * b.sf[o_r]
                row = int(k["y"])
                if which.startswith("minr"):
                    y = F32(row) + r + F32(0.25)
                    assert int(np.floor(y - r)) == row
                    y = y + F32(1) if which.endswith("out") else y
                else:
                    y = F32(row) - r - F32(0.25)
                    assert int(np.ceil(y + r)) == row
                    y = y - F32(1) if which.endswith("out") else y
                e.probe(which, i, e.right(k["x"] - d, y, o_r, e.flipped(u, 10)), d=d, level=lvl)
    # right keypoints with y < r and y > h-1-r: their bands are clipped at rows 0 and h-1; left keypoints placed by hand in those rows
    for rows, v_l, y_r, kind in ((np.arange(0, 8), 1.0, 0.5, "clip_top"), (np.arange(H - 8, H), H - 2.0, H - 1.25, "clip_bottom")):
        d = int(b.disp[int(v_l)])
        for x in _sites(b.left, rows, 100, W - 100, 4):
            il = e.take_left(); u = e.unique(il)
            e.kL["x"][il] = x; e.kL["y"][il] = v_l; e.kL["octave"][il] = 0
            e.probe(kind, il, e.right(x - d, y_r, 1, e.flipped(u, 10)), d=d)
    return e, BF, MIN_Z


def group_hamming(b):
    """3: best distance 74 goes on to the refinement, 75 does not (:663); of two candidates at the same distance the lower iR wins
    (:654), also when the other one comes first in the memory order of the kernel's row table (sorted by centre row)"""
    e = Edit(b, 3)
    for nbits in (74, 75):
        for i, d in e.pick_left(5):
            k = e.kL[i]; u = e.unique(i)
            e.probe(f"hamming{nbits}", i, e.right(k["x"] - d, k["y"], k["octave"], e.flipped(u, nbits)), d=d)
    for i, d in e.pick_left(6, lambda i, d: e.kL["y"][i] < H - 30):
        k = e.kL[i]; u = e.unique(i); s = float(b.sf[k["octave"]])
        lo, hi = e.free_r.pop(0), e.free_r.pop(0)
        assert lo < hi
        e.right(k["x"] - d, k["y"] + 1.0, k["octave"], e.flipped(u, 30), slot=lo)             # the winner: lower index, later centre row
        e.right(k["x"] - d - 20 * s, k["y"], k["octave"], e.flipped(u, 30), slot=hi)          # the loser would start 20 level px off
        e.probe("tie", i, lo, other=hi, d=d)
    return e, BF, MIN_Z


def group_window_limits(b):
    """4: endu == level width is rejected, width - 1 accepted (:686); a true shift of 5 level px gives bestincR == +-5: rejected (:705)"""
    e = Edit(b, 4)
    d_min = int(b.disp.min())
    rows_of_band = np.nonzero(b.disp == d_min)[0]
    band = rows_of_band[(rows_of_band >= rows_of_band.min() + 12) & (rows_of_band <= rows_of_band.max() - 12)]
    assert d_min <= 5 and len(band) >= 12
    e.d_min = d_min
    for lvl in (0, 1, 2):
        wl = b.levels_R[lvl].shape[1]
        # rows of the band with structure next to the right border of the right eye
        g = np.abs(np.diff(b.right[:, W - 30:].astype(np.int64), axis=1)).sum(axis=1)
        en = np.convolve(g, np.ones(11, np.int64), mode="same")
        ys = [int(y) for y in band[np.argsort(-en[band], kind="stable")]]
        rows = []
        for y in ys:
            if all(abs(y - o) >= 6 for o in rows):
                rows.append(y)
        for y in rows[:4]:
            for target, kind in ((wl - 12, "endu_in"), (wl - 11, "endu_out")):
                x_r = F32(target) * b.sf[lvl]
                assert orb_model._c_round(x_r * b.isf[lvl]) == target
                il = e.take_left(); u = e.unique(il)
                e.kL["x"][il] = x_r + F32(d_min); e.kL["y"][il] = y; e.kL["octave"][il] = lvl
                e.probe(kind, il, e.right(x_r, y, lvl, e.flipped(u, 10)), level=lvl)
    for shift in (-5, -4, 4, 5):
        for i, d in e.pick_left(5, lambda i, d: e.kL["octave"][i] == 0):
            k = e.kL[i]; u = e.unique(i)
            e.probe(f"shift{shift:+d}", i, e.right(k["x"] - d - shift, k["y"], 0, e.flipped(u, 10)), d=d)
    return e, BF, MIN_Z


def group_zero_disparity(b):
    """5: identical, left-right symmetric surroundings at the same place in both eyes, level 0, integer coordinates: delta == 0 and
    disparity == 0, so u_right = float(double(uL) - 0.01) and depth = bf / 0.01f (:725-729)"""
    e = Edit(b, 5)
    for c, r in PATCHES:
        il = e.take_left(); u = e.unique(il)
        e.kL["x"][il] = c; e.kL["y"][il] = r; e.kL["octave"][il] = 0
        e.probe("zero", il, e.right(c, r, 0, e.flipped(u, 5)))
    return e, BF, MIN_Z


GROUPS = dict(range=group_disparity_range, band=group_octave_and_band, hamming=group_hamming, window=group_window_limits,
              zero=group_zero_disparity)


def _many_left(b, n=2600):
    """7: more than 2048 left keypoints (the extracted ones repeated, with their descriptors): the tail loops of stereo_cut"""
    idx = np.arange(n) % len(b.kL)
    return b.kL[idx].copy(), b.dL[idx].copy(), b.kR.copy(), b.dR.copy()


@pytest.fixture(scope="module")
def base(oracle):
    return Base(oracle, *_directed_pair())


def build_calls(base, oracle):
    """every directed call, run once through the model and the oracle"""
    out = {}
    for name, fn in GROUPS.items():
        e, bf, min_z = fn(base)
        out[name] = base.run(oracle, *e.arrays(), bf, min_z)
        out[name]["probes"] = e.probes
        # pair 1 of the batched form: the same keypoints with the descriptors as extracted
        out[name + "/plain"] = base.run(oracle, e.kL, base.dL, e.kR, base.dR, bf, min_z)
    out["many"] = base.run(oracle, *_many_left(base))
    # 6: the median cut on accepted sets chosen from what the unedited call accepts before its cut
    plain = base.run(oracle, base.kL, base.dL, base.kR, base.dR)
    out["plain"] = plain
    st, sad = plain["info"]["stage"], plain["info"]["sad"]
    acc = np.nonzero(((st == ACCEPTED) | (st == CUT)) & (sad > 0))[0]
    acc = acc[np.argsort(sad[acc], kind="stable")]
    a, big = int(acc[0]), int(acc[-1])
    mid = int([i for i in acc if sad[i] > sad[a] and F32(sad[big]) >= F32(1.5) * F32(1.4) * F32(sad[i])][-1])
    assert F32(sad[big]) >= F32(1.5) * F32(1.4) * F32(sad[a])
    out["cut_sads"] = (int(sad[a]), int(sad[mid]), int(sad[big]))
    for name, sel in (("cut1", [mid]), ("cut2", [a, big]), ("cut4", [big, a, big, a]), ("cut5", [big, mid, a, mid, mid]),
                      ("cut6", [mid, big, a, big, mid, a])):
        out[name] = base.run(oracle, base.kL[sel], base.dL[sel], base.kR, base.dR)
    ez, _, _ = group_zero_disparity(base)
    zl = [p["il"] for p in ez.probes]
    out["cut0"] = base.run(oracle, ez.kL[zl], ez.dL[zl], ez.kR, ez.dR)
    # 8: trivial sizes
    one = int(acc[len(acc) // 2])
    r_one = int(plain["info"]["best_r"][one])
    out["nR0"] = base.run(oracle, base.kL[[one]], base.dL[[one]], base.kR[:0], base.dR[:0])
    out["n1"] = base.run(oracle, base.kL[[one]], base.dL[[one]], base.kR[[r_one]], base.dR[[r_one]])
    return out


@pytest.fixture(scope="module")
def calls(base, oracle):
    """shared by the CPU and the GPU tests"""
    return build_calls(base, oracle)


def _same(tag, got_u, got_z, want_u, want_z, what):
    bad = np.nonzero(got_u.view(np.uint32) != want_u.view(np.uint32))[0]
    assert len(bad) == 0, f"{tag}: uRight differs from {what} at {bad[:5].tolist()}: {got_u[bad[:5]]} vs {want_u[bad[:5]]}"
    bad = np.nonzero(got_z.view(np.uint32) != want_z.view(np.uint32))[0]
    assert len(bad) == 0, f"{tag}: depth differs from {what} at {bad[:5].tolist()}: {got_z[bad[:5]]} vs {want_z[bad[:5]]}"
    assert got_u.tobytes() == want_u.tobytes() and got_z.tobytes() == want_z.tobytes()


def _kinds(c):
    """probe kind -> (stages, accepted flags, probes)"""
    out = {}
    for p in c["probes"]:
        out.setdefault(p["kind"], []).append(p)
    return out


def _accepted(c, probes):
    """probes whose coarse stage chose the right keypoint made for them and that are in the final output"""
    return [p for p in probes if c["info"]["best_r"][p["il"]] == p["ir"] and c["info"]["stage"][p["il"]] == ACCEPTED and c["mu"][p["il"]] >= 0]


def _unmatched(c, probes):
    """probes for which the coarse stage found no right keypoint at all"""
    return [p for p in probes if c["info"]["best_r"][p["il"]] == -1 and c["info"]["stage"][p["il"]] == COARSE_FAIL and c["mu"][p["il"]] == -1]


def _stage(c, probes, stage):
    return [p for p in probes if c["info"]["stage"][p["il"]] == stage]


# ---------------------------------------------------------------------------------------------------- CPU: model against oracle

def test_textured_pairs(oracle):
    """the two textured scenes of the existing fixtures: extractor keypoints, nothing edited"""
    for seed in (104, 61):
        b = Base(oracle, *synth.stereo_pair(seed, W, H))
        c = b.run(oracle, b.kL, b.dL, b.kR, b.dR)
        _same(f"seed {seed}", c["ou"], c["oz"], c["mu"], c["mz"], "the model")
        assert (c["mu"] >= 0).sum() > 50 and (c["info"]["stage"] == CUT).sum() >= 1


CALLS = list(GROUPS) + [g + "/plain" for g in GROUPS] + ["many", "plain", "cut1", "cut2", "cut4", "cut5", "cut6", "cut0", "nR0", "n1"]


@pytest.mark.parametrize("name", CALLS)
def test_directed_call_oracle_equals_model(calls, name):
    c = calls[name]
    _same(name, c["ou"], c["oz"], c["mu"], c["mz"], "the model")


def test_every_call_is_compared(calls):
    assert sorted(CALLS + ["cut_sads"]) == sorted(calls)


def test_group1_disparity_range(calls):
    c = calls["range"]; k = _kinds(c)
    n = {kind: len(_accepted(c, k[kind])) for kind in ("minU_in", "maxU_in")}
    n.update({kind: len(_unmatched(c, k[kind])) for kind in ("minU_out", "maxU_out")})
    assert all(v >= 3 for v in n.values()), n
    max_d = F32(c["bf"]) / F32(c["min_z"])
    for p in k["minU_in"]:
        assert c["kR"]["x"][p["ir"]] == F32(c["kL"]["x"][p["il"]]) - max_d
    for p in k["maxU_in"]:
        assert c["kR"]["x"][p["ir"]] == c["kL"]["x"][p["il"]]


def test_group2_octave_and_band(calls):
    c = calls["band"]; k = _kinds(c)
    n = {kind: len(_accepted(c, k[kind])) for kind in ("octave-1", "octave+1", "minr", "maxr", "clip_top", "clip_bottom")}
    n.update({kind: len(_unmatched(c, k[kind])) for kind in ("octave-2", "octave+2", "minr_out", "maxr_out")})
    assert all(v >= 3 for v in n.values()), n
    for end, kind in ((0, "octave+1"), (CFG[2] - 1, "octave-1")):      # the ends of the kernel's per-level reach table
        assert len(_accepted(c, [p for p in k[kind] if p.get("end") == end])) >= 3, (end, kind)
    for lvl in (0, CFG[2] - 1):
        assert len(_accepted(c, [p for p in k["minr"] + k["maxr"] if p["level"] == lvl])) >= 3, lvl


def test_group3_hamming_and_ties(calls):
    c = calls["hamming"]; k = _kinds(c)
    assert len(_accepted(c, k["hamming74"])) >= 3
    rejected = [p for p in _stage(c, k["hamming75"], COARSE_FAIL) if c["info"]["best_dist"][p["il"]] == 75 and c["info"]["best_r"][p["il"]] == p["ir"]]
    assert len(rejected) >= 3
    assert all(c["info"]["best_dist"][p["il"]] == 74 for p in k["hamming74"])
    won = [p for p in _accepted(c, k["tie"]) if p["ir"] < p["other"] and c["kR"]["y"][p["ir"]] > c["kR"]["y"][p["other"]] and
           abs((c["kL"]["x"][p["il"]] - c["mu"][p["il"]]) - p["d"]) < 2.0]       # refined from the winner's column, not from the loser's
    assert len(won) >= 3


def test_group4_window_limits(calls):
    c = calls["window"]; k = _kinds(c)
    n = {kind: len(_accepted(c, k[kind])) for kind in ("endu_in", "shift-4", "shift+4")}
    n["endu_out"] = len(_stage(c, k["endu_out"], WINDOW_OUT))
    for s in (-5, 5):
        n[f"shift{s:+d}"] = len([p for p in _stage(c, k[f"shift{s:+d}"], SHIFT_EDGE) if c["info"]["best_inc"][p["il"]] == s])
    assert all(v >= 3 for v in n.values()), n
    assert all(abs(c["info"]["best_inc"][p["il"]]) == 4 for p in _accepted(c, k["shift-4"] + k["shift+4"]))


def test_group5_zero_disparity(calls):
    c = calls["zero"]
    ok = _accepted(c, c["probes"])
    assert len(ok) >= 3 and c["info"]["median"] > 0
    for p in ok:
        u_l = c["kL"]["x"][p["il"]]
        assert c["info"]["sad"][p["il"]] == 0 and c["info"]["best_inc"][p["il"]] == 0
        assert c["mu"][p["il"]] == F32(np.float64(u_l) - 0.01) and c["mz"][p["il"]] == F32(c["bf"]) / F32(0.01)


def test_group6_median_cut(calls):
    a, mid, big = calls["cut_sads"]
    want = dict(cut1=(1, 0), cut2=(2, 0), cut4=(4, 0), cut5=(4, 1), cut6=(4, 2), cut0=(0, len(PATCHES)))     # (kept, cut)
    for name, (kept, cut) in want.items():
        st = calls[name]["info"]["stage"]
        assert ((st == ACCEPTED).sum(), (st == CUT).sum()) == (kept, cut), (name, st.tolist(), (a, mid, big))
        assert (calls[name]["mu"] >= 0).sum() == kept
    assert calls["cut5"]["info"]["median"] == mid and (calls["cut5"]["info"]["sad"] == mid).sum() == 3     # several SADs equal to the median
    assert calls["cut6"]["info"]["median"] == mid and calls["cut4"]["info"]["median"] == big and calls["cut2"]["info"]["median"] == big
    assert calls["cut0"]["info"]["median"] == 0


def test_group7_many_left_keypoints(calls):
    c = calls["many"]
    st = c["info"]["stage"]
    assert len(st) == 2600 and (st[2048:] == ACCEPTED).sum() >= 1 and (st[2048:] == CUT).sum() >= 1
    assert (c["mu"][2048:] >= 0).sum() >= 1


def test_group8_trivial_sizes(calls):
    assert calls["nR0"]["mu"].tolist() == [-1.0] and calls["nR0"]["info"]["stage"].tolist() == [NO_CANDIDATE]
    assert calls["n1"]["info"]["stage"].tolist() == [ACCEPTED] and calls["n1"]["mu"][0] >= 0


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def hip(pkg, base):
    """both eyes extracted on the device: orbx_stereo_match reads the handles' pyramids"""
    exL = pkg.ORBextractor(*CFG, device=0, max_size=(W, H))
    exR = pkg.ORBextractor(*CFG, device=0, max_size=(W, H))
    kL, dL = exL(base.left); kR, dR = exR(base.right)
    assert kL.tobytes() == base.kL.tobytes() and kR.tobytes() == base.kR.tobytes()
    assert dL.tobytes() == base.dL.tobytes() and dR.tobytes() == base.dR.tobytes()
    return exL, exR


def _hip_call(pkg, exL, exR, tag, c):
    ur, dp = pkg.ComputeStereoMatches(exL, exR, c["kL"], c["dL"], c["kR"], c["dR"], c["bf"], c["min_z"])
    _same(tag, ur, dp, c["mu"], c["mz"], "the model")
    _same(tag, ur, dp, c["ou"], c["oz"], "the oracle")


def _hip_batch(pkg, base, tag, pairs):
    """orbx_stereo_match_batch_device on len(pairs) copies of the image pair, keypoints and descriptors of each pair handed in by the
    caller (ROWTAB_FROM_KEYPOINTS: k_stereo_prep builds the row tables), into poisoned outputs"""
    import torch
    B = len(pairs)
    dev = torch.device("cuda", 0)
    ex = pkg.ORBextractor(*CFG, device=0, max_size=(W, H), max_batch=2 * B)
    host = np.stack([base.left] * B + [base.right] * B)
    imgs = torch.from_numpy(host).to(dev)
    cap_x = ex.max_keypoints(W, H)
    xk = torch.zeros((2 * B, cap_x, 7), dtype=torch.float32, device=dev); xd = torch.zeros((2 * B, cap_x, 32), dtype=torch.uint8, device=dev)
    xn = torch.zeros(2 * B, dtype=torch.int32, device=dev)
    ex.extract_batch_device(imgs.data_ptr(), H * W, W, 2 * B, W, H, xk.data_ptr(), xd.data_ptr(), cap_x, xn.data_ptr(), None)
    ex.sync()
    cap = max(max(len(c["kL"]), len(c["kR"])) for c in pairs)
    hk = np.zeros((2 * B, cap, 28), np.uint8); hd = np.zeros((2 * B, cap, 32), np.uint8); hn = np.zeros(2 * B, np.int32)
    for p, c in enumerate(pairs):
        for slot, k, d in ((p, c["kL"], c["dL"]), (B + p, c["kR"], c["dR"])):
            hk[slot, :len(k)] = np.ascontiguousarray(k).view(np.uint8).reshape(len(k), 28); hd[slot, :len(k)] = d; hn[slot] = len(k)
    dk, dd, dn = torch.from_numpy(hk).to(dev), torch.from_numpy(hd).to(dev), torch.from_numpy(hn).to(dev)
    ur = torch.full((B, cap), 123.0, dtype=torch.float32, device=dev); dp = torch.full((B, cap), 123.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    pkg.orbx.stereo_match_batch_device(ex, 0, ex, B, B, dk.data_ptr(), dd.data_ptr(), dn.data_ptr(), dk[B:].data_ptr(), dd[B:].data_ptr(),
                                       dn[B:].data_ptr(), cap, pairs[0]["bf"], pairs[0]["min_z"], ur.data_ptr(), dp.data_ptr(), None,
                                       row_table=pkg.orbx.ROWTAB_FROM_KEYPOINTS)
    ex.sync()
    ur_h, dp_h = ur.cpu().numpy(), dp.cpu().numpy()
    for p, c in enumerate(pairs):
        n = len(c["kL"])
        _same(f"{tag} pair {p}", ur_h[p, :n], dp_h[p, :n], c["mu"], c["mz"], "the model")
        _same(f"{tag} pair {p}", ur_h[p, :n], dp_h[p, :n], c["ou"], c["oz"], "the oracle")
    return ex.debug_launch_forms()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GROUPS))
def test_hip_directed_groups(pkg, base, calls, hip, name):
    _hip_call(pkg, *hip, name, calls[name])
    if name != "zero":
        assert calls[name]["mu"].tobytes() != calls[name + "/plain"]["mu"].tobytes()      # the two pairs of the batch differ
        _hip_batch(pkg, base, f"batch {name}", [calls[name], calls[name + "/plain"]])


@pytest.mark.gpu
def test_hip_cut_and_trivial_calls(pkg, calls, hip):
    for name in ("plain", "cut1", "cut2", "cut4", "cut5", "cut6", "cut0", "nR0", "n1"):
        _hip_call(pkg, *hip, name, calls[name])


@pytest.mark.gpu
@pytest.mark.parametrize("kpw", ["1", "4"])
def test_hip_many_left_keypoints(pkg, base, calls, monkeypatch, kpw):
    """2600 left keypoints with one keypoint per wave (the cut folded into k_stereo<true>) and with four (k_stereo_cut): the tail
    loops of stereo_cut in both; the variable is read when a handle is created"""
    monkeypatch.setenv("ORBX_STEREO_KPW", kpw)
    exL = pkg.ORBextractor(*CFG, device=0, max_size=(W, H)); exR = pkg.ORBextractor(*CFG, device=0, max_size=(W, H))
    exL(base.left); exR(base.right)
    _hip_call(pkg, exL, exR, f"many kpw={kpw}", calls["many"])
    assert exL.debug_launch_forms()["stereo_kpw"] == int(kpw)
    forms = _hip_batch(pkg, base, f"batch many kpw={kpw}", [calls["many"], calls["many"]])
    assert forms["stereo_kpw"] == int(kpw)
