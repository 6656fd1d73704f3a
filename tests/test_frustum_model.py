"""tests/frustum_model.py, the numpy restatement orbx_mappoints_frustum is compared with on the GPU: hand-computed answers for every
rejection rule, the scale level against the expression of tests/adapter_driver.cc's predict() compiled as the reference compiles it,
and the monotonicity of the level predicate round every threshold -- the property the library's bisection rests on.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import frustum_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
CAM = [500.0, 500.0, 320.0, 240.0, 40.0, 0.0, 0.0, 640.0, 480.0]
POSE = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
LSF = f32(np.log(f32(1.2)))


def _pt(g, limit=0.5, cam=CAM, pose=POSE):
    return fm.frustum_point(np.array(g, f32), np.array(pose, f32), np.array(cam, f32), limit, LSF, 8)


def test_known_answer_in_view():
    # P = (0, 0, 2) seen from the origin along z: u = cx, v = cy, dist = 2, cos = 1, xr = 320 - 40 / 2; ratio = 4 / 2 and
    # log(2) / log(1.2) = 3.80 -> level 4
    assert _pt([0, 0, 2, 1, 0, 0, 1, 4]) == (f32(320), f32(240), f32(300), 4, f32(1))
    # P = (0.4, -0.2, 2): u = 500 * 0.4 / 2 + 320 = 420, v = 500 * -0.2 / 2 + 240 = 190 (float rounding stays within 1e-4)
    u, v, xr, level, vc = _pt([0.4, -0.2, 2, 1, 0, 0, 1, 2.2])
    assert abs(u - 420) < 1e-4 and abs(v - 190) < 1e-4 and abs(xr - (u - 20)) < 1e-4
    d = np.sqrt(0.4 ** 2 + 0.2 ** 2 + 4)
    assert abs(vc - 2 / d) < 1e-6 and level == 1                                  # ratio 1.078: 0 < log ratio / log 1.2 = 0.41 <= 1


@pytest.mark.parametrize("g,why", [
    ([0, 0, -2, 1, 0, 0, -1, 4], "Pc_z < 0"),
    ([0, 0, -1e-30, 1e-31, 0, 0, -1, 1e-29], "Pc_z slightly negative"),
    ([0, 0, 0.0, 0, 0, 0, 1, 4], "Pc_z = +0: u is not finite"),
    ([0, 0, -0.0, 0, 0, 0, 1, 4], "Pc_z = -0: u is not finite"),
    ([2, 0, 2, 1, 0, 0, 1, 4], "u = 820 > mnMaxX"),
    ([-2, 0, 2, 1, 0, 0, 1, 4], "u = -180 < mnMinX"),
    ([0, 2, 2, 1, 0, 0, 1, 4], "v = 740 > mnMaxY"),
    ([0, -2, 2, 1, 0, 0, 1, 4], "v = -260 < mnMinY"),
    ([0, 0, 2, 3, 0, 0, 1, 4], "dist 2 < 0.8 * 3"),
    ([0, 0, 2, 0.1, 0, 0, 1, 1], "dist 2 > 1.2 * 1"),
    ([0, 0, 2, 1, 1, 0, 0, 4], "cos 0 < 0.5"),
    ([0, 0, 2, 1, 0, 0, -1, 4], "cos -1 < 0.5"),
    ([0, 0, 2, 1, float("nan"), 0, 1, 4], "cos is not finite"),
])
def test_known_answer_rejections(g, why):
    assert _pt(g) is None, why


def test_bounds_are_inclusive_and_levels_clamp():
    cam = [512.0, 512.0, 0.0, 0.0, 40.0, 0.0, 0.0, 640.0, 480.0]                # u = 512 * X exactly at Z = 1
    assert _pt([1.25, 0.9375, 1, 0.1, 0, 0, 1, 2], cam=cam)[:2] == (f32(640), f32(480))
    assert _pt([0, 0, 1, 0.1, 0, 0, 1, 1], cam=cam)[:2] == (f32(0), f32(0))
    assert _pt([1.25, 0, 1, 0.1, 0, 0, 1, 2], cam=cam) is not None and _pt([np.nextafter(f32(1.25), f32(2)), 0, 1, 0.1, 0, 0, 1, 2], cam=cam) is None
    assert _pt([0, 0.9375, 1, 0.1, 0, 0, 1, 2], cam=cam) is not None and _pt([0, np.nextafter(f32(0.9375), f32(2)), 1, 0.1, 0, 0, 1, 2], cam=cam) is None
    assert _pt([0, 0, 1, 0.1, 0, 0, 1, 0.9])[3] == 0                            # ceil(log 0.9 / log 1.2) = -0 -> 0
    assert _pt([0, 0, 1, 0.01, 0, 0, 1, 0.84])[3] == 0                          # the lowest ratio the distance rule lets through: still -0
    assert _pt([0, 0, 1, 0.1, 0, 0, 1, 100])[3] == 7                            # ... = 26 -> clamped to nlevels - 1
    assert _pt([0, 0, 2, 2.5, 0, 0, 1, 4]) is not None and _pt([0, 0, np.nextafter(f32(2), f32(0)), 2.5, 0, 0, 1, 4]) is None   # dist == 0.8f * dmin stays


PREAMBLE = """#include <cmath>
#include <cstdio>
#include <vector>
using namespace std;   // as the reference's src/MapPoint.cc: log(float) and ceil(float) are the float overloads
"""
MAIN = """
int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 3;
    float logsf; int nlevels;
    sscanf(argv[3], "%a", &logsf); sscanf(argv[4], "%d", &nlevels);
    float md[2];
    while (fread(md, 4, 2, fi) == 2) { const int l = predict(md[0], md[1], logsf, nlevels); fwrite(&l, 4, 1, fo); }
    fclose(fi); fclose(fo);
    return 0;
}
"""


def test_level_equals_the_adaptor_drivers_predict(tmp_path):
    src = open(os.path.join(ROOT, "tests", "adapter_driver.cc")).read()
    m = re.search(r"static int predict\(float maxd, float dist, float logsf, int nlevels\)\n\{.*?\n\}\n", src, re.S)
    assert m, "tests/adapter_driver.cc no longer has predict()"
    cc, exe = str(tmp_path / "predict.cc"), str(tmp_path / "predict")
    open(cc, "w").write(PREAMBLE + m.group(0) + MAIN)
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", cc, "-o", exe])
    rng = np.random.Generator(np.random.PCG64(5))
    for factor in (1.2, 1.1, 2.0):
        lsf = f32(np.log(f32(factor)))
        thr = fm.level_thresholds(lsf, 8)
        maxd = np.exp(rng.uniform(np.log(0.2), np.log(200.0), 1500)).astype(f32)
        dist = np.exp(rng.uniform(np.log(0.5), np.log(20.0), 1500)).astype(f32)
        edge = np.concatenate([[t, np.nextafter(t, f32(0)), np.nextafter(t, f32(np.inf))] for t in thr]).astype(f32)
        maxd = np.concatenate([maxd, edge]); dist = np.concatenate([dist, np.ones(len(edge), f32)])
        np.stack([maxd, dist], 1).astype(f32).tofile(str(tmp_path / "in.bin"))
        subprocess.check_call([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), float(lsf).hex(), "8"])
        got = np.fromfile(str(tmp_path / "out.bin"), np.int32)
        exp = np.array([fm.level_of(f32(a / b), lsf, 8) for a, b in zip(maxd, dist)], np.int32)
        assert len(got) == len(exp) and (got == exp).all(), (factor, np.nonzero(got != exp)[0][:5])
        assert len(set(exp.tolist())) == 8                                       # every level occurs


@pytest.mark.parametrize("factor", [1.2, 1.1, 2.0])
def test_level_predicate_is_monotone_round_every_threshold(factor):
    lsf = f32(np.log(f32(factor)))
    thr = fm.level_thresholds(lsf, 8)
    assert len(thr) == 7 and (np.diff(thr) > 0).all()
    if factor == 1.2:
        assert [float(t) for t in thr[:3]] == [float(f32(1.0000001)), float(f32(1.2000002)), float(f32(1.4400002))]
    for k, t in enumerate(thr):
        b = fm.bits(t)
        for off in range(1, 4097):                                               # 4096 neighbouring floats on each side
            assert not fm.level_predicate(fm.from_bits(b - off), lsf, k), (factor, k, -off)
            assert fm.level_predicate(fm.from_bits(b + off - 1), lsf, k), (factor, k, off - 1)
        # the level counted from the thresholds is the level computed directly, on both sides of the entry
        for r in (t, np.nextafter(t, f32(0))):
            assert fm.level_of(r, lsf, 8) == int((thr <= r).sum())
