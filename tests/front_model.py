"""Plain numpy models of the front stages of the headline path -- pyramid, per-cell FAST, quadtree cull, record assembly -- and of the
whole extractor, written from the text and independent of oracle/orb_oracle.c (nothing is imported from oracle/ here; only data is
shared with it).  Line references go to the reference's src/ORBextractor.cc, B.x / A.x to the appendices of SURVEY.md.

What kind of pin each stage is:

  * The OpenCV primitives -- cv::resize (B.2), cv::FAST's score and 3x3 suppression (A.3), cv::GaussianBlur (B.3) -- cannot be read:
    OpenCV's source is no part of the reference.  Their models are a SECOND RESTATEMENT of SURVEY B.2, A.3 and B.3, by other means (whole
    arrays of integers instead of loops over pixels; the FAST score by its definition instead of cornerScore's two passes).  They
    guard the arithmetic and the transcription.  They do not guard the memory of OpenCV the survey was written from.
  * The level sizes (:1345-1366), the cell grid (:925-1009), the quadtree (DivideNode :551-609, DistributeOctTree :617-915) and the
    records (:1023-1045, :1327-1334) are read from the reference itself, line by line.
  * Orientation and rBRIEF come from orb_model (pinned in the same way; its two helpers fast_atan2 and sincos are the oracle's, each
    with a known-answer test of its own).

Defined deviations from the reference, the same ones the oracle documents:
  * nodes of equal count are split in creation order, the later one first (:832 sorts pairs of (count, pointer) and so leaves it to
    the addresses the allocator gave);
  * the root index kp.pt.x / hX (:681) is clamped to the last root (the reference would index past vpIniNodes);
  * a level without a cell (nCols or nRows 0: :950-951 divide by zero) is rejected with ValueError.

B.2 writes the resize scale as src / dst; OpenCV computes it as 1. / (dst / src) in double, which is what is done here.
"""
import numpy as np

import orb_model

F32 = np.float32
EDGE_THRESHOLD = 19           # :74
PATCH_SIZE = 31               # :72
CELL_W = 30                   # :929, const float W = 30

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

# cv::FAST TYPE_9_16, A.3: the 16 ring offsets (dx, dy)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))


def _cv_round(v):
    """cvRound: to nearest, halves to even (B.1)"""
    return int(np.rint(v))


# ------------------------------------------------------------------------------------------------ constructor tables, :429-493

def scale_tables(cfg):
    """mvScaleFactor, mvInvScaleFactor (:436-461) and mnFeaturesPerLevel (:468-493) for cfg = (nfeatures, scaleFactor, nlevels, ...)"""
    nfeatures, scale, nlevels = int(cfg[0]), np.float64(F32(cfg[1])), int(cfg[2])       # a float argument stored in a double (:431)
    sf = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        sf[i] = F32(np.float64(sf[i - 1]) * scale)                                       # :450, float * double -> float
    isf = F32(1.0) / sf                                                                  # :459
    factor = F32(np.float64(1.0) / scale)                                                # :468
    n_desired = F32(nfeatures) * (F32(1) - factor) / (F32(1) - F32(np.float64(factor) ** np.float64(nlevels)))      # :472
    quota = np.zeros(nlevels, np.int64)
    for l in range(nlevels - 1):
        quota[l] = _cv_round(n_desired)                                                  # :479
        n_desired = F32(n_desired * factor)                                              # :489
    quota[nlevels - 1] = max(nfeatures - int(quota[:nlevels - 1].sum()), 0)              # :493
    return sf, isf, quota


# ------------------------------------------------------------------------------------------------ pyramid, :1345-1394

def level_dims(w, h, cfg):
    """:1351-1353: Size(cvRound((float)cols * scale), cvRound((float)rows * scale)) with scale = mvInvScaleFactor[level] -> [(w, h)]"""
    isf = scale_tables(cfg)[1]
    return [(_cv_round(F32(w) * s), _cv_round(F32(h) * s)) for s in isf]


def _linear_coeffs(ssize, dsize):
    """B.2, one axis: source offset and the two 11-bit weights of every destination index"""
    scale = 1.0 / (np.float64(dsize) / np.float64(ssize))
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F32)
    lo = s < 0
    s[lo] = 0; f[lo] = 0
    hi = s >= ssize - 1
    s[hi] = ssize - 1; f[hi] = 0
    c0 = np.clip(np.rint((F32(1.0) - f) * F32(2048)), -32768, 32767).astype(np.int64)   # short a0 = sat(cvRound((1.f - fx) * 2048))
    c1 = np.clip(np.rint(f * F32(2048)), -32768, 32767).astype(np.int64)
    return s, c0, c1


def takes_mean_path(sw, sh, dw, dh):
    """B.2, last sentence: INTER_LINEAR becomes INTER_AREA iff BOTH scales are exactly 2"""
    return sw == 2 * dw and sh == 2 * dh


def resize_model(src, dw, dh):
    """cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR) for 8UC1, B.2, in integers"""
    s = np.asarray(src).astype(np.int64)
    sh, sw = s.shape
    if takes_mean_path(sw, sh, dw, dh):                                                  # the rounded mean of each 2 x 2 block
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    return resize_bilinear(src, dw, dh)


def resize_bilinear(src, dw, dh):
    """the bilinear chain of B.2, whatever the sizes"""
    s = np.asarray(src).astype(np.int64)
    sh, sw = s.shape
    sx, a0, a1 = _linear_coeffs(sw, dw)
    sy, b0, b1 = _linear_coeffs(sh, dh)
    sx1 = np.minimum(sx + 1, sw - 1)                                                     # its weight is 0 where sx is the last column
    sy1 = np.minimum(sy + 1, sh - 1)
    t = s[:, sx] * a0 + s[:, sx1] * a1                                                   # horizontal pass, int32 in OpenCV: [sh, dw]
    t0, t1 = t[sy] >> 4, t[sy1] >> 4
    v = (((b0[:, None] * t0) >> 16) + ((b1[:, None] * t1) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def pyramid_model(img, cfg):
    """ComputePyramid, :1345-1394 -> (levels, mean_path): level l is resized from level l - 1 (:1366), its size comes from the size
    of level 0 (:1353).  The 19-px border of :1370 is never read downstream (A.2) and is not built.  mean_path[l]: level l took the
    2 x 2 mean"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    levels, mean_path = [img], [False]
    for lw, lh in level_dims(w, h, cfg)[1:]:
        ph, pw = levels[-1].shape
        mean_path.append(takes_mean_path(pw, ph, lw, lh))
        levels.append(resize_model(levels[-1], lw, lh))
    return levels, mean_path


# ------------------------------------------------------------------------------------------------ blur, :1314

def gaussian_taps(profile=0):
    """B.3: the 7 fixed-point taps of GaussianBlur(Size(7, 7), 2, 2) on 8U.  Profile 0: cvRound(k * 256) of the normalised float
    kernel exp(-x^2 / 8), sum 257, not renormalised; profile 1: the later generation's table, which sums to exactly 256"""
    if profile == 1:
        return np.array([18, 34, 48, 56, 48, 34, 18], np.int64)
    x = np.arange(-3, 4, dtype=np.float64)
    k = np.exp(-x * x / (2.0 * 2.0 * 2.0))
    k = (k / k.sum()).astype(F32)
    return np.rint(k * F32(256)).astype(np.int64)


def blur7_model(img, profile=0):
    """B.3: row pass in int32, column pass (sum + 2^15) >> 16 saturated to uchar, BORDER_REFLECT_101 (numpy's 'reflect')"""
    img = np.asarray(img)
    h, w = img.shape
    taps = gaussian_taps(profile)
    pad = np.pad(img.astype(np.int64), 3, mode="reflect")
    rows = sum(int(taps[k]) * pad[:, k:k + w] for k in range(7))
    full = sum(int(taps[k]) * rows[k:k + h, :] for k in range(7))
    return np.minimum((full + (1 << 15)) >> 16, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ FAST, A.3

def fast_raw_score(level):
    """per pixel the largest threshold at which it is still a FAST-9/16 corner, by definition: a pixel is a corner at t iff 9
    contiguous ring pixels are all darker than v - t or all brighter than v + t, i.e. iff
        max over the 16 arcs of  min over the 9 ring differences of the arc  > t,   differences taken as v - x (dark) or x - v (bright);
    the largest such t is that maximum - 1.  -> int array of the level's shape; -1 where the pixel is a corner at no t >= 0 and on
    the 3-px rim, where the ring leaves the level"""
    lv = np.asarray(level).astype(np.int16)
    h, w = lv.shape
    out = np.full((h, w), -1, np.int16)
    if h < 7 or w < 7:
        return out.astype(np.int64)
    v = lv[3:h - 3, 3:w - 3]
    d = [v - lv[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING]               # v - x_k
    best = None
    for k in range(16):
        arc = [d[(k + j) % 16] for j in range(9)]
        dark = np.minimum.reduce(arc)                                                    # all 9 darker than v - t  iff  min(v - x) > t
        bright = -np.maximum.reduce(arc)                                                 # all 9 brighter than v + t  iff  min(x - v) > t
        m = np.maximum(dark, bright)
        best = m if best is None else np.maximum(best, m)
    out[3:h - 3, 3:w - 3] = np.maximum(best - 1, -1)
    return out.astype(np.int64)


def _suppress(score):
    """cv::FAST with nonmaxSuppression: keep a pixel iff its score is strictly greater than all 8 neighbours'; beyond the buffer: 0.
    -> (kept, tied): tied = corners with no greater neighbour but an equal one"""
    p = np.pad(score, 1)
    h, w = score.shape
    nb = [p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    top = np.maximum.reduce(nb)
    return (score > 0) & (score > top), (score > 0) & (score == top)


def cell_grid(lw, lh):
    """:934-951 for a level of lw x lh pixels -> dict(minBorderX, maxBorderX, minBorderY, maxBorderY, nCols, nRows, wCell, hCell)"""
    min_bx = EDGE_THRESHOLD - 3; min_by = min_bx                                         # :934-935
    max_bx = lw - EDGE_THRESHOLD + 3; max_by = lh - EDGE_THRESHOLD + 3                   # :936-937
    width = F32(max_bx - min_bx); height = F32(max_by - min_by)                          # :944-945
    n_cols = int(width / F32(CELL_W)); n_rows = int(height / F32(CELL_W))                # :947-948, truncation
    if n_cols < 1 or n_rows < 1:
        raise ValueError(f"a {lw} x {lh} level has no cell")                             # deviation: the reference divides by zero
    w_cell = int(np.ceil(width / F32(n_cols))); h_cell = int(np.ceil(height / F32(n_rows)))        # :950-951
    return dict(minBorderX=min_bx, maxBorderX=max_bx, minBorderY=min_by, maxBorderY=max_by, nCols=n_cols, nRows=n_rows, wCell=w_cell, hCell=h_cell)


CELL_SKIPPED_ROW, CELL_SKIPPED_COL, CELL_FIRST_PASS, CELL_SECOND_PASS = range(4)


def cell_candidates_model(level, ini_th, min_th):
    """the cell loop of ComputeKeyPointsOctTree, :929-1009 -> (x, y, response, events).  Candidates come cell-row-major, then row-major
    inside the cell, coordinates relative to (minBorderX, minBorderY) = (16, 16) as at :1002-1003.

    events (for the tests that assert an edge is reached; counted over every pass that ran):
      state[i, j]      CELL_SKIPPED_ROW / CELL_SKIPPED_COL / CELL_FIRST_PASS / CELL_SECOND_PASS (the cell ran FAST at minThFAST)
      roi[i, j]        iniX, maxX, iniY, maxY
      first_corners    [i, j] corners at iniThFAST before suppression;  kept[i, j]: candidates the cell contributed
      emptied          cells whose first pass had corners and kept none
      tie_suppressed   corners with no greater neighbour in the cell's buffer but an equal one
      border_kept      [(x, y, out_x, out_y)]: candidates kept although a neighbour of at least their score, at the pass's threshold,
                       lies in the level -- outside this cell's detectable area, to the side (out_x), above / below (out_y) or both"""
    level = np.asarray(level)
    lh, lw = level.shape
    g = cell_grid(lw, lh)
    raw = fast_raw_score(level)
    n_rows, n_cols, w_cell, h_cell = g["nRows"], g["nCols"], g["wCell"], g["hCell"]
    state = np.zeros((n_rows, n_cols), np.int64); roi = np.zeros((n_rows, n_cols, 4), np.int64)
    first_corners = np.zeros((n_rows, n_cols), np.int64); kept_n = np.zeros((n_rows, n_cols), np.int64)
    ev = dict(grid=g, state=state, roi=roi, first_corners=first_corners, kept=kept_n, emptied=0, tie_suppressed=0, border_kept=[])
    xs, ys, rs = [], [], []
    for i in range(n_rows):                                                              # :953
        ini_y = F32(g["minBorderY"] + i * h_cell)                                        # :957
        max_y = ini_y + F32(h_cell) + F32(6)                                             # :959
        if ini_y >= g["maxBorderY"] - 3:                                                 # :961
            state[i, :] = CELL_SKIPPED_ROW
            continue
        if max_y > g["maxBorderY"]:                                                      # :964
            max_y = F32(g["maxBorderY"])
        for j in range(n_cols):                                                          # :967
            ini_x = F32(g["minBorderX"] + j * w_cell)                                    # :971
            max_x = ini_x + F32(w_cell) + F32(6)                                         # :972
            if ini_x >= g["maxBorderX"] - 6:                                             # :973: 6, not 3
                state[i, j] = CELL_SKIPPED_COL
                continue
            if max_x > g["maxBorderX"]:                                                  # :975
                max_x = F32(g["maxBorderX"])
            x0, x1, y0, y1 = int(ini_x), int(max_x), int(ini_y), int(max_y)              # rowRange(iniY, maxY).colRange(iniX, maxX), :988
            roi[i, j] = (x0, x1, y0, y1)
            cw, ch = x1 - x0, y1 - y0
            buf = np.zeros((ch, cw), np.int64)                                           # cv::FAST's score rows: 0 outside [3, size - 3)
            if ch > 6 and cw > 6:
                buf[3:ch - 3, 3:cw - 3] = raw[y0 + 3:y1 - 3, x0 + 3:x1 - 3]
            # the same pixels seen from the level, one more ring of neighbours: what a suppression over the whole level would compare with
            wide = np.full((ch + 2, cw + 2), -1, np.int64)
            wy0, wy1, wx0, wx1 = max(y0 - 1, 0), min(y1 + 1, lh), max(x0 - 1, 0), min(x1 + 1, lw)
            wide[wy0 - (y0 - 1):wy1 - (y0 - 1), wx0 - (x0 - 1):wx1 - (x0 - 1)] = raw[wy0:wy1, wx0:wx1]
            state[i, j] = CELL_FIRST_PASS
            th = ini_th                                                                  # :988
            score = np.where(buf >= th, buf, 0)                                          # a corner at th keeps its score; anything else is 0
            kept, tied = _suppress(score)
            ev["tie_suppressed"] += int(tied.sum())
            first_corners[i, j] = int((score > 0).sum())
            if not kept.any():                                                           # :991: vKeysCell.empty(), AFTER suppression
                ev["emptied"] += int(first_corners[i, j] > 0)
                state[i, j] = CELL_SECOND_PASS
                th = min_th                                                              # :993
                score = np.where(buf >= th, buf, 0)
                kept, tied = _suppress(score)
                ev["tie_suppressed"] += int(tied.sum())
            cy, cx = np.nonzero(kept)                                                    # row-major
            kept_n[i, j] = len(cx)
            wscore = np.where(wide >= th, wide, 0)
            for x, y in zip(cx.tolist(), cy.tolist()):
                s = score[y, x]
                out_x = out_y = False
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        in_cell = 3 <= x + dx < cw - 3 and 3 <= y + dy < ch - 3
                        if (dx or dy) and not in_cell and wscore[y + dy + 1, x + dx + 1] >= s:
                            out_x |= not 3 <= x + dx < cw - 3
                            out_y |= not 3 <= y + dy < ch - 3
                if out_x or out_y:
                    ev["border_kept"].append((x + j * w_cell, y + i * h_cell, out_x, out_y))
            xs.extend((cx + j * w_cell).tolist())                                        # :1002
            ys.extend((cy + i * h_cell).tolist())                                        # :1003
            rs.extend(score[cy, cx].tolist())
    return np.array(xs, np.int32), np.array(ys, np.int32), np.array(rs, np.int32), ev


# ------------------------------------------------------------------------------------------------ quadtree, :551-915

class _Node:
    """ExtractorNode (include/ORBextractor.h:45-56); keys = indices into the candidate list, in vKeys order"""
    __slots__ = ("UL", "UR", "BL", "BR", "keys", "bNoMore", "seq")

    def __init__(self, seq):
        self.keys = []; self.bNoMore = False; self.seq = seq


def _c_round(v):
    """round() of <cmath>: halves away from zero"""
    return int(np.floor(abs(float(v)) + 0.5)) * (1 if v >= 0 else -1)


def distribute_octtree_model(x, y, resp, minX, maxX, minY, maxY, N, info=None):
    """DistributeOctTree, :617-915, sequentially, a Python list standing for std::list<ExtractorNode> (index 0 = front).
    x, y: candidate coordinates relative to (minX, minY), as vToDistributeKeys holds them; -> indices of the kept candidates, one per
    leaf, in list order.  info (a dict, optional) receives what the tests need to see that an edge is reached: roots (nIni), live_roots,
    sweeps (whole-list sweeps), sorted_passes, breaks [number of nodes of a sorted pass left unsplit when N was reached],
    equal_counts (neighbours of equal count among the nodes a sorted pass did split), leaf_ties (leaves whose best response is shared)"""
    if info is None:
        info = {}
    info.update(roots=0, live_roots=0, sweeps=0, sorted_passes=0, breaks=[], equal_counts=0, leaf_ties=0)
    x = [float(F32(v)) for v in x]; y = [float(F32(v)) for v in y]; resp = [float(F32(v)) for v in resp]      # kp.pt, kp.response: float
    seq = [0]

    def new_node():
        seq[0] += 1
        return _Node(seq[0])

    def divide(nd):                                                                      # DivideNode, :551-609
        half_x = int(np.ceil(F32(nd.UR[0] - nd.UL[0]) / F32(2)))                         # :553
        half_y = int(np.ceil(F32(nd.BR[1] - nd.UL[1]) / F32(2)))                         # :554
        n1, n2, n3, n4 = new_node(), new_node(), new_node(), new_node()
        n1.UL = nd.UL; n1.UR = (nd.UL[0] + half_x, nd.UL[1]); n1.BL = (nd.UL[0], nd.UL[1] + half_y); n1.BR = (nd.UL[0] + half_x, nd.UL[1] + half_y)
        n2.UL = n1.UR; n2.UR = nd.UR; n2.BL = n1.BR; n2.BR = (nd.UR[0], nd.UL[1] + half_y)
        n3.UL = n1.BL; n3.UR = n1.BR; n3.BL = nd.BL; n3.BR = (n1.BR[0], nd.BL[1])
        n4.UL = n3.UR; n4.UR = n2.BR; n4.BL = n3.BR; n4.BR = nd.BR
        for k in nd.keys:                                                                # :583-597
            if x[k] < n1.UR[0]:
                (n1 if y[k] < n1.BR[1] else n3).keys.append(k)
            elif y[k] < n1.BR[1]:
                n2.keys.append(k)
            else:
                n4.keys.append(k)
        for c in (n1, n2, n3, n4):                                                       # :600-607
            if len(c.keys) == 1:
                c.bNoMore = True
        return n1, n2, n3, n4

    n_ini = _c_round(F32(maxX - minX) / F32(maxY - minY))                                # :627
    if n_ini < 1:
        raise ValueError("no root node")                                                 # the reference divides by zero at :629
    hx = F32(maxX - minX) / F32(n_ini)                                                   # :629
    nodes, ini = [], []
    for i in range(n_ini):                                                               # :637-659
        ni = new_node()
        ni.UL = (int(hx * F32(i)), 0); ni.UR = (int(hx * F32(i + 1)), 0)                 # Point2i(float, int) truncates
        ni.BL = (ni.UL[0], maxY - minY); ni.BR = (ni.UR[0], maxY - minY)
        nodes.append(ni); ini.append(ni)
    for k in range(len(x)):                                                              # :665-682
        r = int(F32(x[k]) / hx)
        ini[min(max(r, 0), n_ini - 1)].keys.append(k)                                    # deviation: clamped
    i = 0
    while i < len(nodes):                                                                # :691-705
        if len(nodes[i].keys) == 1:
            nodes[i].bNoMore = True; i += 1
        elif not nodes[i].keys:
            del nodes[i]
        else:
            i += 1
    info["roots"] = n_ini; info["live_roots"] = len(nodes)

    def push_children(children, pos, size_and_node):
        """:752-793 / :840-875: push_front of every child that holds a point -> (new position of the node at pos, nToExpand)"""
        n_exp = 0
        for c in children:
            if c.keys:
                nodes.insert(0, c); pos += 1
                if len(c.keys) > 1:
                    n_exp += 1
                    size_and_node.append((len(c.keys), c))
        return pos, n_exp

    finish = False
    size_and_node = []
    while not finish:                                                                    # :719
        prev_size = len(nodes)
        n_to_expand = 0
        size_and_node = []
        info["sweeps"] += 1
        i = 0
        while i < len(nodes):                                                            # :731-798; children go to the front and are not visited
            if nodes[i].bNoMore:
                i += 1
                continue
            i, e = push_children(divide(nodes[i]), i, size_and_node)
            n_to_expand += e
            del nodes[i]                                                                 # :795, lit = erase(lit)
        if len(nodes) >= N or len(nodes) == prev_size:                                   # :803
            finish = True
        elif len(nodes) + n_to_expand * 3 > N:                                           # :814
            while not finish:                                                            # :817
                prev_size = len(nodes)
                prev = sorted(size_and_node, key=lambda p: (p[0], p[1].seq))             # :832; deviation: creation order for the pointer
                size_and_node = []
                info["sorted_passes"] += 1
                for j in range(len(prev) - 1, -1, -1):                                   # :834
                    nd = prev[j][1]
                    info["equal_counts"] += int(j + 1 < len(prev) and prev[j + 1][0] == prev[j][0])
                    push_children(divide(nd), 0, size_and_node)
                    del nodes[next(p for p, q in enumerate(nodes) if q is nd)]           # :877, erase(node->lit)
                    if len(nodes) >= N:                                                  # :879
                        info["breaks"].append(j)
                        break
                if len(nodes) >= N or len(nodes) == prev_size:                           # :883
                    finish = True
    out = []
    for nd in nodes:                                                                     # :895-912
        best = nd.keys[0]; max_response = resp[best]
        for k in nd.keys[1:]:
            if resp[k] > max_response:                                                   # strict: the first one wins a tie
                best = k; max_response = resp[k]
        info["leaf_ties"] += int(sum(resp[k] == max_response for k in nd.keys) > 1)
        out.append(best)
    return np.array(out, np.int64)


# ------------------------------------------------------------------------------------------------ the whole extractor, :1267-1339

def extract_model(img, cfg, cv_profile=0, front=None):
    """ORBextractor::operator() for cfg = (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) -> (records, descriptors, stages).
    stages: dims, levels, mean_path, candidates [(x, y, response)], events, keep (indices per level), counts, blurred; pass the
    stages of an earlier call as `front` to redo only the blur and the descriptors (another cv_profile)"""
    nfeatures, _, nlevels, ini_th, min_th = cfg
    sf, isf, quota = scale_tables(cfg)
    if front is None:
        levels, mean_path = pyramid_model(img, cfg)                                      # :1276
        st = dict(dims=[lv.shape[::-1] for lv in levels], levels=levels, mean_path=mean_path, candidates=[], events=[], keep=[], level_xy=[])
        umax = orb_model.umax_model()
        per_level = []
        for l in range(nlevels):                                                         # ComputeKeyPointsOctTree, :931
            x, y, r, ev = cell_candidates_model(levels[l], ini_th, min_th)
            g = ev["grid"]
            keep = distribute_octtree_model(x, y, r, g["minBorderX"], g["maxBorderX"], g["minBorderY"], g["maxBorderY"], int(quota[l])) \
                if len(x) else np.zeros(0, np.int64)                                     # :1015
            scaled_patch_size = int(F32(PATCH_SIZE) * sf[l])                             # :1023, float -> int truncates
            k = np.zeros(len(keep), KP_DTYPE)
            k["x"] = (x[keep] + g["minBorderX"]).astype(F32)                             # :1041
            k["y"] = (y[keep] + g["minBorderY"]).astype(F32)                             # :1042
            k["octave"] = l; k["size"] = F32(scaled_patch_size)                          # :1043-1044
            k["response"] = r[keep].astype(F32); k["class_id"] = -1                      # cv::KeyPoint from FAST: response = score, class_id -1
            for i in range(len(k)):                                                      # computeOrientation, :1050-1051
                k["angle"][i] = orb_model.ic_angle_model(levels[l], int(k["x"][i]), int(k["y"][i]), umax)
            st["candidates"].append((x, y, r)); st["events"].append(ev); st["keep"].append(keep)
            st["level_xy"].append((k["x"].astype(np.int64), k["y"].astype(np.int64)))
            per_level.append(k)
        st["counts"] = np.array([len(k) for k in per_level], np.int64)
        st["level_records"] = per_level
    else:
        st = dict(front)
    pattern = orb_model.load_pattern()
    st["blurred"] = []
    recs, descs = [], []
    for l in range(nlevels):                                                             # :1302
        k = st["level_records"][l].copy()
        if len(k) == 0:                                                                  # :1307
            st["blurred"].append(None)
            continue
        blurred = blur7_model(st["levels"][l], cv_profile)                               # :1312-1314
        st["blurred"].append(blurred)
        lx, ly = st["level_xy"][l]
        d = np.zeros((len(k), 32), np.uint8)
        for i in range(len(k)):                                                          # computeDescriptors, :1320
            d[i] = orb_model.rbrief_model(blurred, int(lx[i]), int(ly[i]), k["angle"][i], pattern)
        if l != 0:                                                                       # :1326-1334: pt *= scale, in float
            k["x"] = k["x"] * sf[l]; k["y"] = k["y"] * sf[l]
        recs.append(k); descs.append(d)
    records = np.concatenate(recs) if recs else np.zeros(0, KP_DTYPE)
    desc = np.concatenate(descs) if descs else np.zeros((0, 32), np.uint8)
    return records, desc, st
