"""orbx_mapgraph_refresh_points against one host core: medians of 200 host-inclusive calls at 2 000 and 8 000 points x ~8 observations (a
local window) for GEOM, DESC and both, and at one whole-map GEOM size of 100 000 points, beside plain C++ loops over std::map on the same
map (tools/refresh_host_loop.cc) -- a lower bound for the reference's cost, not the reference -- and the orbx_mappoints_set re-send that
the call makes unnecessary.
    python tools/bench_refresh.py [--out profiles/r25_refresh.txt] [--reps 200]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NKF, NFEAT, NPT, MAX_OBS = 500, 1000, 100000, 16
SF = np.array([1.2 ** l for l in range(8)], np.float32)


def make_map(seed=5):
    r = np.random.RandomState(seed)
    centre = (r.rand(NKF, 3).astype(np.float32) - np.float32(0.5)) * np.float32(20.0)
    octave = r.randint(0, 8, (NKF, NFEAT)).astype(np.uint8)
    desc = r.randint(0, 256, (NKF, NFEAT, 32)).astype(np.uint8)
    pos = (r.rand(NPT, 3).astype(np.float32) - np.float32(0.5)) * np.float32(20.0) + np.float32(30.0)
    c = r.randint(0, NKF, NPT)
    cnt = r.randint(6, 11, NPT)                      # 8 observers on average, from a window of neighbouring keyframes
    obs = []
    ref = np.zeros(NPT, np.int32)
    for p in range(NPT):
        lo = min(max(c[p] - 8, 0), NKF - 16)
        ks = lo + r.permutation(16)[:cnt[p]]
        ref[p] = ks[0]
        obs.append(np.stack([np.full(cnt[p], p), ks, r.randint(0, NFEAT, cnt[p])], 1))
    return centre, octave, desc, pos, ref, np.concatenate(obs).astype(np.int32)


def median_us(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# Map points refreshed on the device: orbx_mapgraph_refresh_points against one host core (tools/bench_refresh.py, tools/refresh_host_loop.cc)")
    say("# device: " + pkg.orbx.device_identity(0))
    centre, octave, desc, pos, ref, obs = make_map()
    say(f"\n## {NKF} keyframes x {NFEAT} features, {NPT} points, {len(obs)} observations ({len(obs) / NPT:.2f} per point), max_obs {MAX_OBS}; "
        f"medians of {a.reps} host-inclusive calls from Python (ctypes and numpy marshalling inside the clock)")
    g = pkg.MapGraph(NKF, NFEAT, NPT, MAX_OBS)
    zeros = np.zeros(NFEAT, np.uint8)
    for k in range(NKF):
        g.set_keyframe(k, octave[k], zeros, zeros)
    for first in range(0, len(obs), 65536):
        o = obs[first:first + 65536]
        g.add_observations(o[:, 0], o[:, 1], o[:, 2])
    n = NFEAT
    frames = [pkg.DeviceFrame(dict(x=np.full(n, 10, np.float32), y=np.full(n, 10, np.float32), octave=octave[k].astype(np.int32),
                                   angle=np.zeros(n, np.float32), u_right=np.full(n, -1, np.float32), desc=desc[k], bounds=(0.0, 0.0, 640.0, 480.0)))
              for k in range(NKF)]
    kfd = dict(slot=np.arange(NKF, dtype=np.int32), centre=centre, bad=np.zeros(NKF, np.uint8), frame=frames)
    table = pkg.MapPoints(NPT)
    every = np.arange(NPT, dtype=np.int32)
    r0 = g.refresh_points(every, table=table, pos=pos, ref_kf=ref, keyframes=kfd, scale_factors=SF, what=3)
    assert (r0.status == 3).all()
    names = {1: "GEOM", 2: "DESC", 3: "GEOM+DESC"}
    for npts in (2000, 8000, NPT):
        pts = every[:npts]
        for what in (1, 2, 3):
            if npts == NPT and what != 1:
                continue
            out = pkg.RefreshResult(npts)
            us = median_us(lambda: g.refresh_points(pts, table=table, pos=pos[:npts], ref_kf=ref[:npts], keyframes=kfd, scale_factors=SF, what=what,
                                                    out=out), a.reps)
            say(f"orbx_mapgraph_refresh_points {names[what]}, {npts} points, table written in place, all outputs fetched: {us:.1f} us")
        geom, dsc = table.read(pts)
        us = median_us(lambda: (table.set(pts, geom, dsc), table.read(pts[:1])), a.reps)
        say(f"  the re-send the call makes unnecessary: orbx_mappoints_set of {npts} records (geom and desc) until the device has them: {us:.1f} us")
    with tempfile.TemporaryDirectory() as tmp:
        exe, scene = os.path.join(tmp, "refresh_host_loop"), os.path.join(tmp, "scene.bin")
        subprocess.check_call(["g++", "-O2", "-std=c++11", os.path.join(ROOT, "tools", "refresh_host_loop.cc"), "-o", exe])
        with open(scene, "wb") as f:
            np.array([NKF, NFEAT, NPT, len(obs), len(SF)], np.int32).tofile(f)
            for arr in (SF, centre, octave, desc, pos, ref, obs):
                np.ascontiguousarray(arr).tofile(f)
        host_reps = max(a.reps // 10, 5)
        host = subprocess.run([exe, scene, str(host_reps)], capture_output=True, text=True, check=True).stdout
    say(f"the host loops below: medians of {host_reps} runs")
    for ln in host.splitlines():
        if ln.startswith("host "):
            say("  one host core, std::map, a lower bound and not the reference: " + ln)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
