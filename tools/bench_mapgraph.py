"""Resident observation graph (orbx_mapgraph) against one host core: medians of 200 host-inclusive calls of vote, covisibility,
cull_keyframes and a keyframe's edit batches on a map of 500 keyframes x 1000 features and 50 000 points, beside plain C++ loops over
std::map on the same map (tools/mapgraph_host_loop.cc) -- a lower bound for the reference's cost, not the reference.
    python tools/bench_mapgraph.py [--out profiles/r24_mapgraph.txt] [--reps 200]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NKF, NFEAT, NPT = 500, 1000, 50000
CULLED = [100, 250, 400]          # keyframes whose every feature is at the coarsest octave: every observer of their points counts


def make_map(seed=5):
    r = np.random.RandomState(seed)
    octave = r.randint(0, 8, (NKF, NFEAT)).astype(np.int32)
    octave[CULLED] = 7
    used = np.zeros(NKF, np.int64)
    obs = []
    for p in range(NPT):
        c = int(r.randint(0, NKF))
        win = [k for k in range(c - 5, c + 6) if 0 <= k < NKF and used[k] < NFEAT]
        for k in r.choice(win, min(len(win), int(r.randint(4, 7))), replace=False):
            obs.append((p, int(k), int(used[k])))
            used[k] += 1
    return octave, np.array(obs, np.int32)


def median_us(f, reps, after=None):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e6)
        if after:
            after()
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

    say("# Resident observation graph: orbx_mapgraph against one host core (tools/bench_mapgraph.py, tools/mapgraph_host_loop.cc)")
    say("# device: " + pkg.orbx.device_identity(0))
    octave, obs = make_map()
    per_kf = [obs[obs[:, 1] == k] for k in range(NKF)]
    say(f"\n## {NKF} keyframes x {NFEAT} features, {NPT} points, {len(obs)} observations ({len(obs) / NPT:.2f} per point, {len(obs) / NKF:.0f} per keyframe), "
        f"monocular, max_obs 256; medians of {a.reps} host-inclusive calls from Python (ctypes and numpy marshalling inside the clock)")
    g = pkg.MapGraph(NKF, NFEAT, NPT, 256)
    t0 = time.perf_counter()
    zeros, ones = np.zeros(NFEAT, np.uint8), np.ones(NFEAT, np.uint8)
    for k in range(NKF):
        g.set_keyframe(k, octave[k], zeros, ones)
        g.set_matches(k, per_kf[k][:, 2], per_kf[k][:, 0])
    for first in range(0, len(obs), 65536):
        o = obs[first:first + 65536]
        g.add_observations(o[:, 0], o[:, 1], o[:, 2])
    g.vote([])
    say(f"filling the graph ({2 * NKF + (len(obs) + 65535) // 65536} edit calls): {(time.perf_counter() - t0) * 1e3:.1f} ms")

    r = np.random.RandomState(1)
    others = [k for k in range(NKF) if all(abs(k - c) > 12 for c in CULLED)]
    frame = per_kf[300][r.permutation(len(per_kf[300]))[:1000], 0]
    frame = np.concatenate([frame, obs[r.randint(0, len(obs), 1000 - len(frame)), 0]]).astype(np.int32)
    lists = [(0, frame), (1, np.array([300], np.int32)),
             (2, np.array(others[40:60], np.int32)), (2, np.array(others[100:180], np.int32)),
             (2, np.array(CULLED + others[40:57], np.int32)), (2, np.array(CULLED + others[100:177], np.int32)),
             (3, np.array([300], np.int32))]

    dev = []
    cnt, nz = g.vote(frame)
    dev.append(f"orbx_mapgraph_vote, {len(frame)} points: {median_us(lambda: g.vote(frame), a.reps):.1f} us ({len(nz)} keyframes voted for)")
    cnt, nz = g.covisibility(300)
    dev.append(f"orbx_mapgraph_covisibility, keyframe 300 ({len(per_kf[300])} matches): {median_us(lambda: g.covisibility(300), a.reps):.1f} us ({len(nz)} keyframes)")

    def restore():
        for k in CULLED:
            if g.read_keyframe(k) is None:
                g.set_keyframe(k, octave[k], zeros, ones)
                g.set_matches(k, per_kf[k][:, 2], per_kf[k][:, 0])
                g.add_observations(per_kf[k][:, 0], per_kf[k][:, 1], per_kf[k][:, 2])

    for kind, local in lists:
        if kind != 2:
            continue
        ne = np.zeros(len(local), np.uint8)
        res = g.cull_keyframes(local, ne, True)
        restore()
        assert len(res["bad_points"]) == 0
        us = median_us(lambda: g.cull_keyframes(local, ne, True), a.reps, restore)
        dev.append(f"orbx_mapgraph_cull_keyframes, {len(local)} local keyframes, {int((res['culled'] == 1).sum())} culled: {us:.1f} us "
                   f"(nMPs {int(res['n_mps'].mean())} and nRedundant {int(res['n_redundant'].mean())} per keyframe on average)")
    k = 300
    pk = per_kf[k]

    def edits():
        g.set_keyframe(k, octave[k], zeros, ones)
        g.set_matches(k, pk[:, 2], pk[:, 0])
        g.add_observations(pk[:, 0], pk[:, 1], pk[:, 2])

    def edits_applied():
        edits()
        g.vote([])

    g.erase_keyframe(k)
    us = median_us(edits, a.reps, lambda: g.erase_keyframe(k))
    us2 = median_us(edits_applied, a.reps, lambda: g.erase_keyframe(k))
    edits()
    dev.append(f"a keyframe's edit batches (set_keyframe of {NFEAT} features, set_matches and add_observations of {len(pk)}): {us:.1f} us to enqueue, "
               f"{us2:.1f} us until the device has applied them")

    with tempfile.TemporaryDirectory() as tmp:
        words = [NKF, NFEAT, NPT] + (octave | 0x80).reshape(-1).tolist() + [len(obs)] + obs.reshape(-1).tolist() + [len(lists)]
        for kind, lst in lists:
            words += [kind, len(lst)] + lst.tolist()
        np.array(words, np.int32).tofile(os.path.join(tmp, "scene.bin"))
        exe = os.path.join(tmp, "mapgraph_host_loop")
        subprocess.check_call(["g++", "-O2", "-std=c++11", "-Wall", os.path.join(ROOT, "tools", "mapgraph_host_loop.cc"), "-o", exe])
        host = subprocess.run([exe, os.path.join(tmp, "scene.bin"), str(a.reps)], capture_output=True, text=True, check=True).stdout.splitlines()
    for d, h in zip(dev, host):
        say(d)
        say("  one host core, std::map, a lower bound and not the reference: " + h)
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
