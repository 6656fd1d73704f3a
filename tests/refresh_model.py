"""A sequential model of orbx_mapgraph_refresh_points (include/orbx.h): MapPoint::UpdateNormalAndDepth and
MapPoint::ComputeDistinctiveDescriptors on a mapgraph_model.SlotGraph, one point at a time, one numpy scalar operation at a time in the
order the header states -- np.float32 unless a step says np.float64, every operation rounded on its own.  The entries of a row are taken
in ascending keyframe slot.  It knows nothing of waves, ranks or LDS."""
import numpy as np

f32, f64 = np.float32, np.float64
GEOM, DESC = 1, 2


def entries_of(sg, p):
    """the row of point slot p in the order of the contract: [(keyframe slot, feature)] ascending, or None for the early return"""
    mp = sg.pt.get(p)
    if mp is None or mp.mbBad or not mp.mObservations:
        return None
    return sorted((kf.slot, idx) for kf, idx in mp.mObservations.items())


def norm3(d):
    """cv::norm of a 3 x 1 CV_32F: the squares are summed in double"""
    return np.sqrt((f64(d[0]) * f64(d[0]) + f64(d[1]) * f64(d[1])) + f64(d[2]) * f64(d[2]))


def geometry(P, entries, centre, ref, ref_octave, scale_factors):
    """-> [X, Y, Z, mfMinDistance, nx, ny, nz, mfMaxDistance] as float32; centre: {slot: 3 floats}; ref_octave(idx) -> the octave of
    feature idx of the reference keyframe"""
    P = [f32(v) for v in P]
    sf = [f32(v) for v in scale_factors]
    with np.errstate(all="ignore"):
        normal = [f32(0), f32(0), f32(0)]
        for k, _ in entries:                                         # step 1
            d = [P[c] - f32(centre[k][c]) for c in range(3)]
            inv = f64(1.0) / norm3(d)
            normal = [normal[c] + f32(f64(d[c]) * inv) for c in range(3)]
        invn = f64(1.0) / f64(len(entries))                          # step 2
        nv = [f32(f64(normal[c]) * invn) for c in range(3)]
        idx = dict(entries).get(ref, 0)                              # observations[pRefKF] default-inserts 0
        d = [P[c] - f32(centre[ref][c]) for c in range(3)]           # step 3
        dist = f32(norm3(d))
        dmax = dist * sf[ref_octave(idx)]
        dmin = dmax / sf[len(sf) - 1]
    return np.array([P[0], P[1], P[2], dmin, nv[0], nv[1], nv[2], dmax], np.float32)


def hamming_row(D, i):
    """the 256-bit Hamming distances of descriptor i to every descriptor of D [n][32]"""
    return np.unpackbits(np.bitwise_xor(D, D[i]), axis=1).sum(axis=1)


def distinctive(descs):
    """step 4 over the descriptors that take part, in order -> the index of the first row with the smallest median; the k-th smallest
    of a row is found by counting (the smallest v with #(d <= v) > k), not by sorting"""
    D = np.stack([np.asarray(d, np.uint8) for d in descs])
    n = len(D)
    k = int(0.5 * (n - 1))
    best, best_i = None, 0
    for i in range(n):
        at_most = np.cumsum(np.bincount(hamming_row(D, i), minlength=257))
        med = int(np.argmax(at_most > k))
        if best is None or med < best:
            best, best_i = med, i
    return best_i


def refresh(sg, points, what, pos=None, ref_kf=None, centre=None, bad=None, frame_desc=None, scale_factors=None):
    """per listed point: dict(status, geom, best_kf, best_idx, desc) with None for what was not updated.  pos[i] = the position;
    centre / bad: {keyframe slot: ...}; frame_desc: {keyframe slot: descriptors [n][32]}"""
    out = []
    for i, p in enumerate(points):
        r = dict(status=0, geom=None, best_kf=None, best_idx=None, desc=None)
        out.append(r)
        ent = entries_of(sg, p)
        if ent is None:
            continue
        if what & GEOM:
            ref = int(ref_kf[i])
            r["geom"] = geometry(pos[i], ent, centre, ref, lambda idx: sg.kf[ref].octave[idx], scale_factors)
            r["status"] |= GEOM
        if what & DESC:
            part = [(k, idx) for k, idx in ent if not bad[k]]
            if part:
                b = distinctive([np.asarray(frame_desc[k][idx], np.uint8) for k, idx in part])
                r["best_kf"], r["best_idx"] = part[b]
                r["desc"] = np.array(frame_desc[part[b][0]][part[b][1]], np.uint8)
                r["status"] |= DESC
    return out
