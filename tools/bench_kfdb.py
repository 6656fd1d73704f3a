"""KeyFrameDatabase measurements -> profiles/r06_kfdb.txt.  Run on the GPU box: python tools/bench_kfdb.py [out] [--trace]
For 500 and 5000 live keyframes of ~1000 words in a vocabulary of 10^6 words, on place scenes (tools/kfdb_scene.py):
  1. per call: host-inclusive latency (Python ctypes caller) of orbx_kfdb_detect_relocalization and orbx_kfdb_detect_loop, p50 / p99;
  2. throughput: orbx_kfdb_detect_relocalization_batch_device at batch 32, queries per second;
  3. baseline: the same queries on one host core through tools/kfdb_baseline.cc (inverted file of std::list, g++ -O3), compiled here.
     Its candidate lists must equal the library's on the whole query sequence before any time is printed.
  4. chain (500 keyframes, 32 frames): images -> orbx_extract_batch_device -> orbx_bow_transform_batch_device -> orbx_kfdb_add_from_frames for the
     keyframes; for the query frames the same front end, then orbx_kfdb_detect_relocalization_batch_device and orbx_kf_search_by_bow_kfs_f on
     the returned candidates only -- beside orbx_bowdb_search_batch_device_compact over all keyframes on the same frames.  The candidate-only
     matches must equal the corresponding rows of the all-keyframes search before a time is printed.  A third route, timed in the same rounds:
     orbx_kfdb_detect_relocalization_batch_device + orbx_bowdb_search_candidates_device_compact on one stream, one synchronise, no download
     inside the clock; its lists must equal the all-keyframes rows too.
--candidates [out] runs leg 4 alone, at 500 and at 5000 keyframes -> profiles/r07_reloc_candidates.txt.
--trace runs a short per-call + batched sequence at 5000 keyframes and nothing else (the rocprofv3 --kernel-trace --stats pass)."""
import os
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
from tools import kfdb_scene  # noqa: E402

NWORDS = 1000000
BATCH = 32


def pct(a, q):
    return float(np.percentile(np.asarray(a) * 1e6, q))


def make(nkf, nq, seed):
    sc = kfdb_scene.Scene(seed, places=nkf // 8, per_place=8, nwords=NWORDS, base=600, keep=0.6, extra=640)
    qs = []
    for i in range(nq):                          # relocalisation and loop queries alternate; a loop query is connected to three keyframes of its place
        p = int(sc.rng.integers(0, nkf // 8))
        qs.append((i % 2, sc.query(p), [p * 8, p * 8 + 1, p * 8 + 2] if i % 2 else [], 0.02 if i % 2 else 0.0))
    return sc, qs


def fill(db, sc):
    for kf in sc.keyframes:
        db.add(kf)
    for i, nb in enumerate(sc.neighbours):
        db.set_covisibility(i, nb)


def run(db, q):
    return db.DetectLoopCandidates(q[1], q[2], q[3]) if q[0] else db.DetectRelocalizationCandidates(q[1])


def baseline(sc, qs, tmp, repeats=3):
    exe = os.path.join(tmp, "kfdb_baseline")
    subprocess.check_call(["g++", "-O3", "-std=c++11", os.path.join(ROOT, "tools", "kfdb_baseline.cc"), "-o", exe])
    scene, out = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "out.bin")
    with open(scene, "wb") as f:
        f.write(struct.pack("<ii", NWORDS, len(sc.keyframes)))
        for (ids, vals), nb in zip(sc.keyframes, sc.neighbours):
            f.write(struct.pack("<i", len(ids))); f.write(ids.astype("<u4").tobytes()); f.write(vals.astype("<f8").tobytes())
            f.write(struct.pack("<i", len(nb))); f.write(np.asarray(nb, "<i4").tobytes())
        f.write(struct.pack("<i", len(qs)))
        for kind, (ids, vals), conn, ms in qs:
            f.write(struct.pack("<ii", kind, len(ids))); f.write(ids.astype("<u4").tobytes()); f.write(vals.astype("<f8").tobytes())
            f.write(struct.pack("<i", len(conn))); f.write(np.asarray(conn, "<i4").tobytes()); f.write(struct.pack("<f", ms))
    subprocess.check_call(["taskset", "-c", "0", exe, scene, out, str(repeats)] if os.path.exists("/usr/bin/taskset") else [exe, scene, out, str(repeats)])
    buf = open(out, "rb").read()
    pos, lists = 0, []
    for _ in qs:
        n = struct.unpack_from("<i", buf, pos)[0]; pos += 4
        lists.append(list(struct.unpack_from(f"<{n}i", buf, pos))); pos += 4 * n
    return lists, np.frombuffer(buf, "<f8", len(qs), pos)


def measure(pkg, nkf, reps, lines, tmp):
    import torch
    sc, qs = make(nkf, 2 * reps, 1000 + nkf)
    db = pkg.KeyFrameDatabase(NWORDS)
    t0 = time.perf_counter(); fill(db, sc); t_fill = time.perf_counter() - t0
    got = [run(db, q) for q in qs]               # the whole sequence once: the lists to verify, and the warm-up
    want, t_base = baseline(sc, qs, tmp)
    if got != want:
        bad = [i for i in range(len(qs)) if got[i] != want[i]]
        raise SystemExit(f"{nkf} keyframes: library and baseline disagree on {len(bad)} of {len(qs)} queries (first: {bad[0]}: {got[bad[0]]} vs {want[bad[0]]})")
    t = [[], []]
    for q in qs:
        a = time.perf_counter(); run(db, q); t[q[0]].append(time.perf_counter() - a)
    words = float(np.mean([len(k[0]) for k in sc.keyframes]))
    lines.append(f"## {nkf} live keyframes, {words:.0f} words each on average, vocabulary of {NWORDS} words ({nkf // 8} places x 8), {reps} calls per query kind")
    lines.append(f"candidate lists of all {len(qs)} queries equal the host baseline's: yes ({sum(len(g) for g in got) / len(got):.2f} candidates per query, "
                 f"{max(len(g) for g in got)} at most, {sum(1 for g in got if not g)} empty)")
    lines.append(f"filling the database (add + set_covisibility per keyframe, host vectors): {t_fill * 1e3:.1f} ms")
    for kind, name in ((0, "orbx_kfdb_detect_relocalization"), (1, "orbx_kfdb_detect_loop")):
        base = t_base[[i for i, q in enumerate(qs) if q[0] == kind]]
        lines.append(f"{name:36s} per call, host-inclusive   p50 {pct(t[kind], 50):8.1f} us   p99 {pct(t[kind], 99):8.1f} us")
        lines.append(f"{'  one host core, inverted file':36s} per query (best of 3 passes)  p50 {pct(base, 50):8.1f} us   p99 {pct(base, 99):8.1f} us")
    # batched, device resident
    fr = pkg.BowFrames(BATCH, 2048)
    rq = [q for q in qs if q[0] == 0][:BATCH]
    for i, q in enumerate(rq):
        fr.set_bow(i, q[1])
    d_cand = torch.zeros((BATCH, 16), dtype=torch.int32, device="cuda"); d_n = torch.zeros(BATCH, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    for _ in range(5):
        db.detect_relocalization_batch_device(fr, BATCH, d_cand.data_ptr(), 16, d_n.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    steps = 50
    a = time.perf_counter()
    for _ in range(steps):
        db.detect_relocalization_batch_device(fr, BATCH, d_cand.data_ptr(), 16, d_n.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    dt = time.perf_counter() - a
    base_reloc = t_base[[i for i, q in enumerate(qs) if q[0] == 0]]
    lines.append(f"orbx_kfdb_detect_relocalization_batch_device, batch {BATCH}, {steps} launches back to back: {dt / steps * 1e6:.1f} us per batch, "
                 f"{dt / steps / BATCH * 1e6:.2f} us per query, {BATCH * steps / dt:.0f} queries/s   (host core: {1e6 / pct(base_reloc, 50):.0f} queries/s at its p50)")
    lines.append("")


def chain(pkg, lines, nkf=500, B=BATCH, places=25, reps=10):
    """leg 4: what searching only the candidates saves.  Keyframes and query frames are views of `places` synthetic images (a small shift and
    noise), extracted and transformed on the device; the keyframe ids orbx_kfdb returns are joined to the resident orbx_kf handles here."""
    import torch
    from tools import synth
    W, H = 640, 480
    rng = np.random.default_rng(9)
    base = [synth.image(700 + p, W, H) for p in range(places)]

    def view(p):
        im = np.roll(base[p], (int(rng.integers(-6, 7)), int(rng.integers(-6, 7))), (0, 1)).astype(np.int16)
        return np.clip(im + rng.integers(-6, 7, im.shape), 0, 255).astype(np.uint8)

    ex = pkg.ORBextractor(1000, 1.2, 8, 20, 7, device=0, max_size=(W, H), max_batch=B)
    cap = ex.max_keypoints(W, H)
    d_kps = torch.zeros((B, cap, 7), device="cuda"); d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream(); st = stream.cuda_stream
    fr = pkg.BowFrames(B, cap)

    def front_end(imgs, voc):
        """extract (+ ComputeBoW when the vocabulary exists) for up to B images, all on `st`; -> host copies for the featsets"""
        d_img = torch.from_numpy(np.stack(imgs)).cuda()
        torch.cuda.synchronize()
        ex.extract_batch_device(d_img.data_ptr(), H * W, W, len(imgs), W, H, d_kps.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
        if voc is not None:
            fr.transform(voc, d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), len(imgs), 4, st)
        stream.synchronize()
        n = d_n.cpu().numpy()
        return n, d_desc.cpu().numpy(), d_kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)

    def featset(i, n, desc, kps, flag):
        t = fr.read(i, st)
        ang = np.frombuffer(kps[i, :n[i]].tobytes(), dtype=pkg.KP_DTYPE)["angle"].copy()
        return dict(desc=desc[i, :n[i]].copy(), node_id=t["fv_node_id"], node_off=t["fv_node_off"], feat=t["fv_feat"], flag=flag(n[i]), angle=ang)

    # vocabulary of ORBvoc's shape (k = 10, L = 6: 10^6 words), its two upper levels seeded from real descriptors (as bench.py's euroc_bow leg)
    n, desc, kps = front_end([base[p] for p in range(min(places, B))], None)
    par, leaf, nd, wt = synth.vocab_tree(709, 10, 6, stop_frac=0.0, data=None)
    d0 = np.concatenate([desc[i, :n[i]] for i in range(min(places, B))])
    nd[:110] = synth.flip_bits(np.random.Generator(np.random.PCG64(710)), d0[rng.integers(0, len(d0), 110)], 0.1)
    voc = pkg.ORBVocabulary(10, 6, par, leaf, nd, wt)
    db = pkg.KeyFrameDatabase(voc.info()["words"])
    kfs, t_add = [], 0.0
    for first in range(0, nkf, B):
        m = min(B, nkf - first)
        n, desc, kps = front_end([view((first + i) % places) for i in range(m)], voc)
        a = time.perf_counter()
        ids = [db.add(fr, i, stream=st) for i in range(m)]               # device to device
        t_add += time.perf_counter() - a
        assert ids == list(range(first, first + m))
        kfs += [featset(i, n, desc, kps, lambda k: (rng.random(k) < 0.6).astype(np.uint8)) for i in range(m)]
    for j in range(nkf):
        mates = sorted((k for k in range(j % places, nkf, places) if k != j), key=lambda k: abs(k - j))
        db.set_covisibility(j, mates[:8])
    resident = [pkg.DeviceKeyFrame(k) for k in kfs]                      # what the candidate ids are joined to
    bowdb = pkg.BowDatabase(kfs)
    qplace = [int(rng.integers(0, places)) for _ in range(B)]
    n, desc, kps = front_end([view(p) for p in qplace], voc)
    frames = [featset(i, n, desc, kps, lambda k: np.zeros(k, np.uint8)) for i in range(B)]
    d_pairs = torch.zeros((B, nkf, cap, 2), dtype=torch.int32, device="cuda"); d_nm = torch.zeros((B, nkf), dtype=torch.int32, device="cuda")
    ccap = 16
    d_cand = torch.zeros((B, ccap), dtype=torch.int32, device="cuda"); d_nc = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_cand3 = torch.zeros((B, ccap), dtype=torch.int32, device="cuda"); d_nc3 = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_pairs3 = torch.full((B, ccap, cap, 2), -7, dtype=torch.int32, device="cuda"); d_nm3 = torch.full((B, ccap), -9, dtype=torch.int32, device="cuda")
    matcher = pkg.ORBmatcher(0.75, True)
    torch.cuda.synchronize()
    t_all, t_det, t_srch, t_dev = [], [], [], []
    for rep in range(reps + 2):                                          # two warm-up rounds, the two forms alternating
        a = time.perf_counter()
        fr.search_compact(bowdb, B, d_pairs.data_ptr(), cap, d_nm.data_ptr(), 0.75, True, st)
        stream.synchronize()
        b = time.perf_counter()
        db.detect_relocalization_batch_device(fr, B, d_cand.data_ptr(), ccap, d_nc.data_ptr(), st)
        stream.synchronize()
        nc = d_nc.cpu().numpy(); cand = d_cand.cpu().numpy()
        c = time.perf_counter()
        found = []
        for i in range(B):
            ids = [int(x) for x in cand[i, :min(nc[i], ccap)]]
            found.append((ids,) + (matcher.SearchByBoWKeyFramesFrameResident([resident[k] for k in ids], [kfs[k]["flag"] for k in ids], frames[i])
                                   if ids else (None, None)))
        d = time.perf_counter()
        db.detect_relocalization_batch_device(fr, B, d_cand3.data_ptr(), ccap, d_nc3.data_ptr(), st)
        fr.search_candidates_compact(bowdb, B, d_cand3.data_ptr(), ccap, d_nc3.data_ptr(), d_pairs3.data_ptr(), cap, d_nm3.data_ptr(), 0.75, True, stream=st)
        stream.synchronize()
        e = time.perf_counter()
        if rep >= 2:
            t_all.append(b - a); t_det.append(c - b); t_srch.append(d - c); t_dev.append(e - d)
    # the candidate-only matches are the rows of the all-keyframes search
    # (only the candidates' lists of the all-keyframes result come to the host: the whole of it is gigabytes at 5000 keyframes)
    nm = d_nm.cpu().numpy()
    sel = [(i, k) for i, (ids, _, _) in enumerate(found) for k in ids]
    si = torch.tensor([p[0] for p in sel], dtype=torch.long, device="cuda"); sk = torch.tensor([p[1] for p in sel], dtype=torch.long, device="cuda")
    pairs = dict(zip(sel, d_pairs[si, sk].cpu().numpy())) if sel else {}
    searched = matched = hit = 0
    for i, (ids, rows, cnt) in enumerate(found):
        hit += any(k % places == qplace[i] for k in ids)
        for j, k in enumerate(ids):
            f = np.nonzero(rows[j] >= 0)[0]
            want = pairs[i, k][:nm[i, k]]
            if cnt[j] != nm[i, k] or len(f) != nm[i, k] or (want[:, 0] != f).any() or (want[:, 1] != rows[j][f]).any():
                raise SystemExit(f"chain: frame {i}, keyframe {k}: the candidate-only search differs from the all-keyframes row ({cnt[j]} vs {nm[i, k]} matches)")
            searched += 1; matched += int(cnt[j])
    # so are the lists of the device route, whose candidates are the downloaded route's
    nc3 = d_nc3.cpu().numpy(); cand3 = d_cand3.cpu().numpy(); nm3 = d_nm3.cpu().numpy(); pairs3 = d_pairs3.cpu().numpy()
    searched3 = 0
    for i, (ids, _, _) in enumerate(found):
        if [int(x) for x in cand3[i, :min(nc3[i], ccap)]] != ids:
            raise SystemExit(f"chain: frame {i}: the two detect calls of a round returned different candidates")
        if (nm3[i, len(ids):] != -1).any():
            raise SystemExit(f"chain: frame {i}: a slot beyond the list is not marked -1")
        for j, k in enumerate(ids):
            if nm3[i, j] != nm[i, k] or (pairs3[i, j, :nm[i, k]] != pairs[i, k][:nm[i, k]]).any():
                raise SystemExit(f"chain: frame {i}, slot {j}, keyframe {k}: the device list differs from the all-keyframes row ({nm3[i, j]} vs {nm[i, k]} matches)")
            searched3 += 1
    # the list launch alone, on the lists of the last round (launch + synchronise), compact and dense
    d_rows3 = torch.zeros((B, ccap, cap), dtype=torch.int32, device="cuda")
    t_list = {"compact": [], "dense": []}
    for rep in range(reps + 2):
        a = time.perf_counter()
        fr.search_candidates_compact(bowdb, B, d_cand3.data_ptr(), ccap, d_nc3.data_ptr(), d_pairs3.data_ptr(), cap, d_nm3.data_ptr(), 0.75, True, stream=st)
        stream.synchronize()
        b = time.perf_counter()
        fr.search_candidates(bowdb, B, d_cand3.data_ptr(), ccap, d_nc3.data_ptr(), d_rows3.data_ptr(), d_nm3.data_ptr(), 0.75, True, stream=st)
        stream.synchronize()
        if rep >= 2:
            t_list["compact"].append(b - a); t_list["dense"].append(time.perf_counter() - b)
    # the two kernel forms at about that many live pairs, by proxy: the all-keyframes entry point on two keyframes x B frames, dense rows (the
    # wave form has no compact output and no list form)
    small = pkg.BowDatabase(kfs[:2])
    d_m2 = torch.zeros((B, 2, cap), dtype=torch.int32, device="cuda"); d_n2 = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    t_form = {"table": [], "wave": []}
    try:
        for rep in range(reps + 2):
            for form in ("table", "wave"):
                pkg.orbx.debug_set_bow_form(form)
                a = time.perf_counter()
                fr.search(small, B, d_m2.data_ptr(), d_n2.data_ptr(), 0.75, True, st)
                stream.synchronize()
                if rep >= 2:
                    t_form[form].append(time.perf_counter() - a)
    finally:
        pkg.orbx.debug_set_bow_form("auto")
    best_all = sum(int(nm[i].max() >= 15) for i in range(B))
    best_cand = sum(int(any(nm[i, k] >= 15 for k in ids)) for i, (ids, _, _) in enumerate(found))
    med = lambda t: float(np.median(t)) * 1e6
    lines.append(f"## chain: {nkf} keyframes ({places} places, views of 640x480 images @ 1000 features), {B} query frames, vocabulary of {voc.info()['words']} words, "
                 f"median of {reps} rounds, host clock around work that ends in a stream synchronise")
    lines.append(f"keyframes: extract_batch_device -> bow_transform_batch_device -> orbx_kfdb_add_from_frames: {t_add / nkf * 1e6:.1f} us per add (the count comes to the host, the vector does not)")
    lines.append(f"all keyframes:   orbx_bowdb_search_batch_device_compact                     {B * nkf:6d} (frame, keyframe) pairs searched   {med(t_all):9.1f} us per batch")
    lines.append(f"candidates only: orbx_kfdb_detect_relocalization_batch_device + download    {med(t_det):9.1f} us per batch")
    lines.append(f"                 orbx_kf_search_by_bow_kfs_f per frame, resident keyframes  {searched:6d} (frame, keyframe) pairs searched   {med(t_srch):9.1f} us per batch")
    lines.append(f"                 together {med(t_det) + med(t_srch):9.1f} us per batch = {med(t_all) / (med(t_det) + med(t_srch)):.2f} x the all-keyframes search"
                 f" ({B * nkf / max(searched, 1):.0f} x fewer pairs)")
    lines.append(f"candidates only, on the device: orbx_kfdb_detect_relocalization_batch_device + orbx_bowdb_search_candidates_device_compact, one stream, "
                 f"one synchronise, nothing downloaded")
    lines.append(f"                 {B} x {ccap} slots launched                                  {searched3:6d} (frame, keyframe) pairs searched   {med(t_dev):9.1f} us per batch"
                 f" = {med(t_all) / med(t_dev):.2f} x the all-keyframes search, {(med(t_det) + med(t_srch)) / med(t_dev):.2f} x the download-and-call route")
    lines.append(f"every device candidate list equals the all-keyframes list: yes ({searched3} lists, the candidates of the downloaded route)")
    lines.append(f"the list launch alone (k_bow2_cand, {B} x {ccap} workgroups of which {searched3} work, launch + synchronise): compact lists "
                 f"{med(t_list['compact']):.1f} us, dense rows {med(t_list['dense']):.1f} us")
    lines.append(f"kernel forms at about that many live pairs, a proxy (orbx_bowdb_search_batch_device on 2 keyframes x {B} frames = {2 * B} workgroups, all live, "
                 f"dense rows, launch + synchronise): table form (k_bow2) {med(t_form['table']):.1f} us, wave form (k_bow_wave) {med(t_form['wave']):.1f} us")
    lines.append(f"every candidate-only match row equals the all-keyframes row: yes ({searched} rows, {matched} matches); a keyframe of the query's own place "
                 f"among the candidates: {hit} of {B} frames; frames with a keyframe of >= 15 matches (Tracking.cc:1675): {best_cand} among the candidates, {best_all} among all")
    lines.append("(the query frame of orbx_kf_search_by_bow_kfs_f is a host feature set -- the Frame of a lost tracker lives on the host --, prepared outside the clock)")
    lines.append("")


def trace(pkg):
    import torch
    sc, qs = make(5000, 40, 77)
    db = pkg.KeyFrameDatabase(NWORDS)
    fill(db, sc)
    for q in qs:
        run(db, q)
    fr = pkg.BowFrames(BATCH, 2048)
    for i in range(BATCH):
        fr.set_bow(i, qs[2 * (i % 20)][1])
    d_cand = torch.zeros((BATCH, 16), dtype=torch.int32, device="cuda"); d_n = torch.zeros(BATCH, dtype=torch.int32, device="cuda")
    for _ in range(5):
        db.detect_relocalization_batch_device(fr, BATCH, d_cand.data_ptr(), 16, d_n.data_ptr(), None)
    torch.cuda.synchronize()
    db.reloc_scores()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    pkg = ge.build()
    if "--trace" in sys.argv:
        trace(pkg)
        return
    if "--candidates" in sys.argv:
        out = args[0] if args else os.path.join(ROOT, "profiles", "r07_reloc_candidates.txt")
        lines = ["# relocalisation search over the candidates only, on the device, beside the all-keyframes search and the download-and-call route "
                 "(tools/bench_kfdb.py --candidates)", f"# device: {pkg.orbx.device_identity(0)}", ""]
        chain(pkg, lines, nkf=500, places=25)
        chain(pkg, lines, nkf=5000, places=250)
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        open(out, "w").write(text)
        print(text)
        return
    out = args[0] if args else os.path.join(ROOT, "profiles", "r06_kfdb.txt")
    lines = ["# KeyFrameDatabase queries: device-resident orbx_kfdb against one host core (tools/bench_kfdb.py)",
             f"# device: {pkg.orbx.device_identity(0)}", ""]
    with tempfile.TemporaryDirectory() as tmp:
        for nkf in (500, 5000):
            measure(pkg, nkf, 200, lines, tmp)
    chain(pkg, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
