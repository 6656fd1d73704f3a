"""Plain numpy models of the per-keypoint stages of the headline path, written from the reference text and independent of
oracle/orb_oracle.c: the intensity-centroid angle (src/ORBextractor.cc:83-111), the steered BRIEF descriptor
(src/ORBextractor.cc:116-157) and Frame::ComputeStereoMatches (src/Frame.cc:577-751).  They pin the oracle stages ic_angle,
orb_descriptor and oracle_stereo_match -- and through them the kernels k_desc and k_stereo / k_stereo_prep / stereo_cut -- bit for bit.
The stages before them (pyramid, per-cell FAST, quadtree, records, blur) are pinned in the same way by tests/front_model.py.

Two helpers are taken from the oracle on purpose, because each has a known-answer test of its own (test_oracle_known_answers.py):
oracle_py.fast_atan2 (the polynomial of cv::fastAtan2) and oracle_py.sincos (the build's deterministic sin / cos).  The models pin
what is done with them: the moment structure, the x0,y0,x1,y1 order of the pattern, the rotation signs, cvRound of the rotated
offsets, t0 < t1, bit k of byte i, and every predicate of the stereo search.

Defined deviations from the reference, the same ones the oracle documents:
  * `mb` (read uninitialised at src/Frame.cc:607) is the explicit min_z argument;
  * rows of a right keypoint's band that lie outside the image are skipped (src/Frame.cc:602-603 indexes vRowIndices out of range),
    and a left keypoint whose row lies outside the image has no candidates;
  * an empty accepted set is not indexed (src/Frame.cc:738 reads vDistIdx[0] of an empty vector).
"""
import os

import numpy as np

from oracle import oracle_py

HALF_PATCH_SIZE = 15          # src/ORBextractor.cc:73
F32 = np.float32

_PATTERN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_bit_pattern_31.npy")


def load_pattern():
    """bit_pattern_31_ (src/ORBextractor.cc:160-418) as 512 points (x, y): the reference reads the int array as Point[512]
    (src/ORBextractor.cc:505-507), so point idx is (flat[2 idx], flat[2 idx + 1])"""
    flat = np.load(_PATTERN_FILE).astype(np.int64).ravel()
    assert flat.shape == (1024,)
    return flat.reshape(512, 2)


def umax_model():
    """src/ORBextractor.cc:510-533: the half-width of each row of the circular patch"""
    umax = np.zeros(HALF_PATCH_SIZE + 1, np.int64)
    vmax = int(np.floor(HALF_PATCH_SIZE * np.sqrt(2.0) / 2 + 1))
    vmin = int(np.ceil(HALF_PATCH_SIZE * np.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        umax[v] = int(np.rint(np.sqrt(float(HALF_PATCH_SIZE * HALF_PATCH_SIZE - v * v))))      # cvRound
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):              # the rest by symmetry of the circle
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax


def ic_moments(level_pixels, x, y, umax):
    """(m_10, m_01) of src/ORBextractor.cc:85-108: sum of u * I and of v * I over the circular patch |u| <= umax[|v|], |v| <= 15"""
    img = np.asarray(level_pixels).astype(np.int64)
    m10 = m01 = 0
    for v in range(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1):
        d = int(umax[abs(v)])
        u = np.arange(-d, d + 1)
        row = img[y + v, x - d:x + d + 1]
        m10 += int((u * row).sum())
        m01 += v * int(row.sum())
    return m10, m01


def ic_angle_model(level_pixels, x, y, umax):
    """IC_Angle, src/ORBextractor.cc:83-111: fastAtan2((float)m_01, (float)m_10), degrees"""
    m10, m01 = ic_moments(level_pixels, x, y, umax)
    return oracle_py.fast_atan2(F32(m01), F32(m10))


def rbrief_pairs(blurred_level, x, y, angle_deg, pattern):
    """the 256 compared pixel pairs (t0, t1) of src/ORBextractor.cc:128-151, in pattern order"""
    factor_pi = F32(np.pi / 180.0)                               # :114, (float)(CV_PI/180.f)
    angle = F32(angle_deg) * factor_pi                           # :121
    b, a = oracle_py.sincos(angle)                               # :123, a = cos, b = sin
    px = pattern[:, 0].astype(F32); py = pattern[:, 1].astype(F32)
    dy = np.rint(px * b + py * a).astype(np.int64)               # :129, cvRound = round half to even; fp32 products and sums
    dx = np.rint(px * a - py * b).astype(np.int64)               # :130
    val = np.asarray(blurred_level)[y + dy, x + dx].astype(np.int64)
    return val[0::2], val[1::2]                                  # GET_VALUE(2 j), GET_VALUE(2 j + 1), pattern += 16 per byte


def rbrief_model(blurred_level, x, y, angle_deg, pattern):
    """computeOrbDescriptor, src/ORBextractor.cc:116-157: 32 bytes, bit k of byte i is t0 < t1 of pair 8 i + k"""
    t0, t1 = rbrief_pairs(blurred_level, x, y, angle_deg, pattern)
    bits = (t0 < t1).astype(np.int64).reshape(32, 8)
    return (bits << np.arange(8)).sum(axis=1).astype(np.uint8)


def extract_tail_model(oracle_handle, kps):
    """angle and descriptor of every keypoint the oracle returned, recomputed from the oracle's own level pixels (orientation,
    src/ORBextractor.cc:538-546) and blurred levels (descriptors, :1302-1325).  Those levels are no longer taken on trust:
    front_model.py restates the pyramid and the blur, tests/test_front_model.py holds the oracle's levels to it pixel for pixel, and
    front_model.extract_model runs ic_angle_model and rbrief_model on the model's own levels, keypoints included.
    -> (angles f32[n], desc u8[n,32], info) with info = level coordinates and the number of compared pairs with equal pixels"""
    pattern = load_pattern()
    umax = umax_model()
    sf = oracle_handle.scale_factors()
    n = len(kps)
    angles = np.zeros(n, F32); desc = np.zeros((n, 32), np.uint8)
    lx = np.zeros(n, np.int64); ly = np.zeros(n, np.int64)
    equal_pairs = 0
    levels = {}
    for i in range(n):
        l = int(kps["octave"][i])
        if l not in levels:
            levels[l] = (oracle_handle.level(l), oracle_handle.level(l, blurred=True))
        pix, blur = levels[l]
        # :1327-1334 scales the level coordinates (integers) by mvScaleFactor[level] in fp32 for level != 0: undo it exactly
        found = False
        for coord, out in ((kps["x"][i], lx), (kps["y"][i], ly)):
            c0 = int(np.rint(float(coord) / float(sf[l])))
            found = False
            for c in (c0, c0 - 1, c0 + 1):
                if (F32(c) * sf[l] if l else F32(c)) == coord:
                    out[i] = c; found = True
                    break
            assert found, f"keypoint {i}: {coord} is no level-{l} integer times the scale factor"
        x, y = int(lx[i]), int(ly[i])
        angles[i] = ic_angle_model(pix, x, y, umax)
        t0, t1 = rbrief_pairs(blur, x, y, angles[i], pattern)
        equal_pairs += int((t0 == t1).sum())
        desc[i] = rbrief_model(blur, x, y, angles[i], pattern)
    return angles, desc, dict(level_x=lx, level_y=ly, equal_pairs=equal_pairs)


# ------------------------------------------------------------------------------------------------ stereo

_POPCNT = np.array([bin(i).count("1") for i in range(256)], np.int64)

# how far a left keypoint got (info["stage"])
NO_CANDIDATE, COARSE_FAIL, WINDOW_OUT, SHIFT_EDGE, DELTA_OUT, DISPARITY_OUT, ACCEPTED, CUT = range(8)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance, src/ORBmatcher.cc:1733-1749: the number of differing bits"""
    return _POPCNT[np.bitwise_xor(a, b)].sum(axis=-1)


def _c_round(v):
    """round() of <cmath>: half away from zero"""
    v = float(v)
    return F32(np.floor(abs(v) + 0.5) * (1.0 if v >= 0 else -1.0))


def _reflect101(i, n):
    """index into a level whose margin is BORDER_REFLECT_101 (src/ORBextractor.cc:1370-1383: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...)"""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _window(level, cx, cy, half_w):
    """rows cy-5..cy+5, columns cx-half_w..cx+half_w of the padded pyramid image (rowRange / colRange of mvImagePyramid)"""
    h, w = level.shape
    ys = _reflect101(np.arange(cy - 5, cy + 6), h)
    xs = _reflect101(np.arange(cx - half_w, cx + half_w + 1), w)
    return level[np.ix_(ys, xs)].astype(np.int64)


def stereo_model(levels_L, levels_R, sf, isf, kL, dL, kR, dR, bf, min_z):
    """Frame::ComputeStereoMatches, src/Frame.cc:577-751 -> (mvuRight f32[nL], mvDepth f32[nL], info).
    levels_*: the unblurred pyramid levels (mvImagePyramid) of both eyes; sf / isf: mvScaleFactors / mvInvScaleFactors;
    kL, kR: keypoint records (x, y, octave); dL, dR: [n,32] descriptors; bf = mbf, min_z = mb.
    info: per left keypoint the stage it reached, the right keypoint of the coarse stage (-1: none), its Hamming distance,
    the best shift and the SAD; and the median of the cut"""
    sf = np.asarray(sf, F32); isf = np.asarray(isf, F32)
    bf = F32(bf); min_z = F32(min_z)
    n_l, n_r = len(kL), len(kR)
    dL = np.asarray(dL, np.uint8).reshape(n_l, 32); dR = np.asarray(dR, np.uint8).reshape(n_r, 32)
    u_right = np.full(n_l, -1.0, F32); depth = np.full(n_l, -1.0, F32)            # :579-580
    stage = np.full(n_l, NO_CANDIDATE, np.int64); best_r = np.full(n_l, -1, np.int64); best_d = np.full(n_l, 100, np.int64)
    best_inc = np.zeros(n_l, np.int64); sad = np.full(n_l, -1, np.int64)
    th_orb_dist = (100 + 50) // 2                                                    # :582, (TH_HIGH + TH_LOW) / 2
    n_rows = levels_L[0].shape[0]                                                    # :584
    rows = [[] for _ in range(n_rows)]                                               # :587
    rx = kR["x"].astype(F32); ry = kR["y"].astype(F32); ro = kR["octave"].astype(np.int64)
    for ir in range(n_r):                                                            # :594-604
        r = F32(2.0) * sf[ro[ir]]
        maxr = int(np.ceil(ry[ir] + r)); minr = int(np.floor(ry[ir] - r))
        for yi in range(max(minr, 0), min(maxr, n_rows - 1) + 1):                    # rows outside the image: skipped (deviation)
            rows[yi].append(ir)
    min_d = F32(0); max_d = bf / min_z                                               # :607-609
    dist_idx = []                                                                    # :612
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for il in range(n_l):                                                        # :615
            level_l = int(kL["octave"][il]); v_l = F32(kL["y"][il]); u_l = F32(kL["x"][il])
            row = int(v_l)                                                           # :622, float -> index truncates
            if row < 0 or row >= n_rows or not rows[row]:                            # :624
                continue
            min_u = u_l - max_d; max_u = u_l - min_d                                 # :627-628
            if max_u < 0:                                                            # :630
                continue
            cand = np.asarray(rows[row], np.int64)                                   # ascending iR: pushed in that order
            ok = (ro[cand] >= level_l - 1) & (ro[cand] <= level_l + 1) & (rx[cand] >= min_u) & (rx[cand] <= max_u)   # :644-649
            cand = cand[ok]
            bd, br = 100, 0                                                          # :633-634, TH_HIGH
            if len(cand):
                dist = descriptor_distance(dL[il][None, :], dR[cand])
                j = int(np.argmin(dist))                                             # :654, strict <: the first minimum
                if dist[j] < bd:
                    bd, br = int(dist[j]), int(cand[j])
                    best_r[il] = br; best_d[il] = bd
            stage[il] = COARSE_FAIL
            if not bd < th_orb_dist:                                                 # :663
                continue
            ur0 = rx[br]                                                             # :666
            scale = isf[level_l]                                                     # :667
            s_ul = _c_round(u_l * scale); s_vl = _c_round(v_l * scale); s_ur0 = _c_round(ur0 * scale)     # :668-670
            w_, L_ = 5, 5
            lev_l, lev_r = levels_L[level_l], levels_R[level_l]
            il_win = _window(lev_l, int(s_ul), int(s_vl), w_)                        # :674-676
            il_win = il_win - il_win[w_, w_]
            iniu = s_ur0 + F32(L_) - F32(w_); endu = s_ur0 + F32(L_) + F32(w_) + F32(1)      # :684-685
            stage[il] = WINDOW_OUT
            if iniu < 0 or endu >= lev_r.shape[1]:                                   # :686
                continue
            strip = _window(lev_r, int(s_ur0), int(s_vl), w_ + L_)                   # the 11 windows of :691 side by side
            best_sad, b_inc = 2 ** 31 - 1, 0                                         # :678-679, INT_MAX
            v_dists = np.zeros(2 * L_ + 1, F32)
            for inc in range(-L_, L_ + 1):                                           # :689
                ir_win = strip[:, L_ + inc:L_ + inc + 2 * w_ + 1]
                ir_win = ir_win - ir_win[w_, w_]                                     # :693
                d = F32(np.abs(il_win - ir_win).sum())                               # :695, L1 norm (exact: integers below 2^24)
                if d < F32(best_sad):                                                # :696, int -> float
                    best_sad = int(d); b_inc = inc                                   # :698, truncates
                v_dists[L_ + inc] = d
            best_inc[il] = b_inc; sad[il] = best_sad
            stage[il] = SHIFT_EDGE
            if b_inc == -L_ or b_inc == L_:                                          # :705
                continue
            d1, d2, d3 = v_dists[L_ + b_inc - 1], v_dists[L_ + b_inc], v_dists[L_ + b_inc + 1]
            delta = (d1 - d3) / (F32(2.0) * (d1 + d3 - F32(2.0) * d2))               # :713
            stage[il] = DELTA_OUT
            if delta < -1 or delta > 1:                                              # :715
                continue
            best_ur = sf[level_l] * (s_ur0 + F32(b_inc) + delta)                     # :719
            disparity = u_l - best_ur                                                # :721
            stage[il] = DISPARITY_OUT
            if disparity >= min_d and disparity < max_d:                             # :723
                if disparity <= 0:                                                   # :725
                    disparity = F32(0.01)                                            # :727
                    best_ur = F32(np.float64(u_l) - 0.01)                            # :728, in double, then stored as float
                depth[il] = bf / disparity                                           # :730
                u_right[il] = best_ur
                dist_idx.append((best_sad, il))                                      # :732
                stage[il] = ACCEPTED
    median = None
    if dist_idx:                                                                     # an empty set is not indexed (deviation)
        dist_idx.sort()                                                              # :737, pairs: by SAD, then by iL
        median = F32(dist_idx[len(dist_idx) // 2][0])                                # :738
        th_dist = F32(1.5) * F32(1.4) * median                                       # :739
        for d, il in reversed(dist_idx):                                             # :741
            if F32(d) < th_dist:
                break
            u_right[il] = -1; depth[il] = -1; stage[il] = CUT
    return u_right, depth, dict(stage=stage, best_r=best_r, best_dist=best_d, best_inc=best_inc, sad=sad, median=median)
