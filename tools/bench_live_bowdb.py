"""What the live BowDatabase costs and saves (orbx_bowdb_create_live, k_bowdb_pack), in one process, warmed shapes, the device synchronise
inside the clock.  The set: 500 keyframes at cap = 1000, 32 query frames per batch (BASELINE config 3).
  (a) adding one keyframe: orbx_bowdb_add_from_frames, beside the only route an immutable set has -- orbx_bowdb_create over the 501 host
      feature sets plus orbx_bowdb_destroy;
  (b) new map-point flags for 20 keyframes: orbx_bowdb_set_flags, beside that same rebuild;
  (c) search time on a live set: the candidate search (32 x 16 slots, compact) and the all-keyframes compact search on the live set and on
      an immutable one holding the same keyframes, the two alternated (and, for the candidate search, the immutable set once more with an
      explicit identity id map, which isolates the lookup a live set always makes).  The live set must not be slower than the immutable
      one by more than the immutable one's own spread (max - min over its repeats) in this run: exit status 1 otherwise.
The C entry points are called with prebuilt arguments, so the clock holds the call and nothing of Python's array handling.
Run on the GPU box: python tools/bench_live_bowdb.py [--out FILE] [--nkf 500] [--reps 7]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                     # noqa: E402
import __graft_entry__ as ge           # noqa: E402
from tools import synth                # noqa: E402

CAP, BATCH, NCAND_SLOTS, REFLAG = 1000, 32, 16, 20


def stats(v):
    v = np.asarray(v, np.float64)
    return f"median {np.median(v):9.1f}  min {v.min():9.1f}  max {v.max():9.1f}  (n = {len(v)})"


def a16(v):
    return (int(v) + 15) // 16 * 16


def slot_bytes(cap):
    """bow_slot_layout of orbx_bow.hip restated: the stride of a live slot"""
    p = 64
    while p < cap:
        p *= 2
    o = 16 + a16(32 * cap) + 2 * a16(4 * cap) + a16(4 * (cap + 4)) + a16(4 * p) + a16(cap) + a16(4 * (cap + 4)) + a16(4 * p) + a16(32 * p) + a16(p)
    lines = (o + 255) // 256
    return (lines + (0 if lines & 1 else 1)) * 256


def packed_bytes(n, nnodes, m):
    """feat_bytes of orbx_bow.hip restated, plus the DevFeat record: what one keyframe takes in the immutable set"""
    return 104 + a16(32 * n) + a16(4 * nnodes) + a16(4 * (nnodes + 1)) + a16(4 * m) + a16(n) + a16(4 * n) + a16(32 * m) + a16(m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--nkf", type=int, default=500)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    pkg = ge.build()
    L = pkg.lib()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def check(rc):
        if rc != 0:
            raise SystemExit(f"orbx call failed ({rc}): {L.orbx_last_error().decode(errors='replace')}")

    nkf, reps = a.nkf, max(a.reps, 5)
    say(f"# live BowDatabase: {nkf} keyframes at cap = {CAP}, {BATCH} frames per batch; times in microseconds, host clock around work that ends "
        f"in a stream synchronise; device: {pkg.orbx.device_identity(0)}")
    # ---- the scene: frames of bit-flipped prototype descriptors, keyframes that are shuffled bit-flipped views of them, 0.7-random flags
    rng = np.random.Generator(np.random.PCG64(9101))
    proto = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    par, leaf, nd, w = synth.vocab_tree(9102, 10, 4, stop_frac=0.02, data=proto)
    voc = pkg.ORBVocabulary(10, 4, par, leaf, nd, w)
    fdesc = np.stack([synth.flip_bits(rng, proto[rng.integers(0, len(proto), CAP)], 0.06) for _ in range(BATCH)])
    fang = rng.uniform(0, 360, (BATCH, CAP)).astype(np.float32)
    nall = nkf + 1                                                  # the last one is the keyframe that (a) adds
    kdesc = np.zeros((nall, CAP, 32), np.uint8); kang = np.zeros((nall, CAP), np.float32)
    kcount = rng.integers(CAP - 200, CAP + 1, nall).astype(np.int32)
    for k in range(nall):
        b = int(rng.integers(0, BATCH)); perm = rng.permutation(CAP)[:kcount[k]]
        kdesc[k, :kcount[k]] = synth.flip_bits(rng, fdesc[b], 0.07)[perm]
        kang[k, :kcount[k]] = ((fang[b] + rng.normal(0, 4, CAP)) % 360).astype(np.float32)[perm]
    flags = [(rng.random(kcount[k]) < 0.7).astype(np.uint8) for k in range(nall)]
    flags2 = [(rng.random(kcount[k]) < 0.7).astype(np.uint8) for k in range(REFLAG)]
    stream = torch.cuda.Stream(); st = stream.cuda_stream

    def resident(desc, ang, counts):
        kps = np.zeros((len(counts), CAP, 7), np.float32); kps[:, :, 3] = ang
        t = (torch.from_numpy(kps).cuda(), torch.from_numpy(desc).cuda(), torch.tensor(counts, dtype=torch.int32, device="cuda"))
        fr = pkg.BowFrames(len(counts), CAP)
        torch.cuda.synchronize()
        fr.transform(voc, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(counts), 2, st)
        stream.synchronize()
        return fr, t
    fr, keep_f = resident(fdesc, fang, [CAP] * BATCH)
    kfr, keep_k = resident(kdesc, kang, kcount.tolist())
    hflag = np.ones((nall, CAP), np.uint8)
    for k in range(nall):
        hflag[k, :kcount[k]] = flags[k]
    d_flag = torch.from_numpy(hflag).cuda()
    # the host feature sets of the rebuild route: the FeatureVectors the device computed, downloaded once, outside every clock
    sets = []
    for k in range(nall):
        t = kfr.read(k, st)
        sets.append(pkg.make_featset(dict(desc=kdesc[k, :kcount[k]], node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"],
                                          flag=flags[k], angle=kang[k, :kcount[k]])))
    arr = (pkg.FeatSet * nall)(*[s_[0] for s_ in sets])
    packed = sum(packed_bytes(n, len(s_[1]["node_id"]), len(s_[1]["feat"])) for s_, n in zip(sets, kcount[:nkf])) / nkf
    live = pkg.BowDatabase.live(nkf + 12, CAP, nkf + 12)
    for k in range(nkf):
        live.add_from_frames(k, kfr, k, d_flag[k].data_ptr(), st)
    stream.synchronize()
    frozen = pkg.BowDatabase.__new__(pkg.BowDatabase); frozen._L = L; frozen._h = C.c_void_p(); frozen.nkf = nkf
    check(L.orbx_bowdb_create(0, arr, nkf, C.byref(frozen._h)))

    def clock(fn, n=1):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e6 / n

    c_lines = []
    assert live.size() == nkf and frozen.size() == nkf      # the all-keyframes searches write one row per slot
    # ---- (c) the searches on a live set and on an immutable one, alternated
    cand = torch.from_numpy(rng.integers(0, nkf, (BATCH, NCAND_SLOTS)).astype(np.int32)).cuda()
    ncand = torch.full((BATCH,), NCAND_SLOTS, dtype=torch.int32, device="cuda")
    out = {}
    for name in ("live", "frozen"):
        out[name] = (torch.full((BATCH, NCAND_SLOTS, CAP, 2), -7, dtype=torch.int32, device="cuda"), torch.full((BATCH, NCAND_SLOTS), -9, dtype=torch.int32, device="cuda"),
                     torch.full((BATCH, nkf, CAP, 2), -7, dtype=torch.int32, device="cuda"), torch.full((BATCH, nkf), -9, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    dbs = {"live": live, "frozen": frozen}

    d_map = torch.arange(nkf, dtype=torch.int32, device="cuda")     # the identity join: gives the immutable set the id lookup the live one always makes
    out["frozen+map"] = out["frozen"]; dbs["frozen+map"] = frozen

    def s_cand(name):
        o = out[name]
        kw = dict(kf_of_id=d_map.data_ptr(), n_ids=nkf) if name == "frozen+map" else {}
        fr.search_candidates_compact(dbs[name], BATCH, cand.data_ptr(), NCAND_SLOTS, ncand.data_ptr(), o[0].data_ptr(), CAP, o[1].data_ptr(), 0.75, True, stream=st, **kw)

    def s_all(name):
        o = out[name]
        check(L.orbx_bowdb_search_batch_device_compact(dbs[name]._h, fr._h, BATCH, 0.75, 1, o[2].data_ptr(), CAP, o[3].data_ptr(), st))
    inner = 20
    res = {(k, n): [] for k in ("cand", "all") for n in ("live", "frozen", "frozen+map")}
    for r in range(reps + 1):
        for kind, fn in (("cand", s_cand), ("all", s_all)):
            names = ("live", "frozen") + (("frozen+map",) if kind == "cand" else ())
            for name in (names if r % 2 == 0 else names[::-1]):
                t = clock(lambda: fn(name), inner)
                if r:
                    res[(kind, name)].append(t)
    torch.cuda.synchronize()
    same = all(torch.equal(out["live"][i], out["frozen"][i]) for i in range(4))
    c_lines.append("")
    c_lines.append(f"## (c) searches, live and immutable alternated, each figure the mean of {inner} launches behind one synchronise")
    ok = same
    for kind, title in (("cand", f"orbx_bowdb_search_candidates_device_compact, {BATCH} x {NCAND_SLOTS} slots"), ("all", f"orbx_bowdb_search_batch_device_compact, {nkf} x {BATCH} pairs")):
        lv, fz = np.asarray(res[(kind, "live")]), np.asarray(res[(kind, "frozen")])
        spread = fz.max() - fz.min()
        diff = np.median(lv) - np.median(fz)
        verdict = "within" if diff <= spread else "ABOVE"
        ok = ok and diff <= spread
        c_lines.append(title)
        c_lines.append(f"  live      {stats(lv)}")
        c_lines.append(f"  immutable {stats(fz)}")
        if kind == "cand":
            c_lines.append(f"  immutable, with an explicit identity d_kf_of_id (the lookup alone; not part of the verdict) {stats(res[(kind, 'frozen+map')])}")
        c_lines.append(f"  live - immutable (medians) {diff:+.1f}, the immutable set's own spread (max - min) {spread:.1f}: {verdict}")
    c_lines.append(f"every output of the live set equals the immutable set's: {'yes' if same else 'NO'}")
    # ---- (a) one keyframe more
    def add_one():
        check(L.orbx_bowdb_add_from_frames(live._h, nkf, kfr._h, nkf, d_flag[nkf].data_ptr(), st))

    def rebuild(n):
        h = C.c_void_p()
        check(L.orbx_bowdb_create(0, arr, n, C.byref(h)))
        L.orbx_bowdb_destroy(h)
    t_add, t_rebuild = [], []
    for r in range(reps + 1):
        t = clock(add_one)
        check(L.orbx_bowdb_erase(live._h, nkf, st)); stream.synchronize()
        tb = clock(lambda: rebuild(nkf + 1))
        if r:                                                     # the first round warms both routes
            t_add.append(t); t_rebuild.append(tb)
    say("")
    say(f"## (a) one keyframe more, {nkf} -> {nkf + 1}")
    say(f"orbx_bowdb_add_from_frames + synchronise                 {stats(t_add)}")
    say(f"orbx_bowdb_create over {nkf + 1} host sets + destroy          {stats(t_rebuild)}")
    say(f"ratio of the medians: {np.median(t_rebuild) / np.median(t_add):.0f} x")
    # ---- (b) new flags for 20 keyframes
    ids = np.arange(REFLAG, dtype=np.int32)
    fa = (C.c_void_p * REFLAG)(*[flags[k].ctypes.data for k in range(REFLAG)])
    fb = (C.c_void_p * REFLAG)(*[flags2[k].ctypes.data for k in range(REFLAG)])
    t_flags = []
    for r in range(2 * reps + 2):
        t = clock(lambda: check(L.orbx_bowdb_set_flags(live._h, ids.ctypes.data, REFLAG, fb if r % 2 == 0 else fa, st)))
        if r >= 2:
            t_flags.append(t)
    say("")
    say(f"## (b) new map-point flags for {REFLAG} keyframes (the set ends with the flags it began with)")
    say(f"orbx_bowdb_set_flags, one launch                         {stats(t_flags)}")
    say(f"the rebuild of (a)                                       {stats(t_rebuild)}")
    say(f"ratio of the medians: {np.median(t_rebuild) / np.median(t_flags):.0f} x")
    for ln in c_lines:
        say(ln)
    say("")
    say("## memory")
    say(f"a live slot at cap = {CAP}: {slot_bytes(CAP)} bytes (the master and the searched form, an odd number of 256-byte lines), beside {packed:.0f} bytes "
        f"per keyframe of the immutable set's packed form on this scene")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    L.orbx_bowdb_destroy(frozen._h); frozen._h = None
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
