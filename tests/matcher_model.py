"""Plain model of the three BoW matchers, written from the reference text alone (reference src/ORBmatcher.cc:147-164 CheckDistEpipolarLine,
:171-303 SearchByBoW(KF,F), :568-702 SearchByBoW(KF,KF), :704-871 SearchForTriangulation, :1687-1728 ComputeThreeMaxima).  Nothing here
touches oracle/: dicts stand in for std::map, lists for std::vector, np.float32 scalars for float.  The functions take the feature-set dicts
the package takes (desc, node_id, node_off, feat, flag, angle[, x, y, octave, u_right]).

flag means what the callers of the package make it mean: in the two SearchByBoW it is "has a good MapPoint" (:204-210, :604-608, :620-626:
a row or column WITHOUT it takes no part); in SearchForTriangulation it is "already has a MapPoint" (:747-751, :770-774: a row or column
WITH it takes no part).

Each function also returns a class report (see _greedy / search_for_triangulation), and takes `mutant`, a set of names from MUTANTS: the
model with one line deliberately wrong, for the test that shows the scenes tell such a defect apart."""
import math

import numpy as np

f32 = np.float32
TH_LOW, HISTO_LENGTH = 50, 30                       # :37-39
POP = np.array([bin(i).count("1") for i in range(256)], np.int64)
MUTANTS = ("no_claims", "kf_f_strict", "kf_kf_le", "ratio_double", "greedy_last_on_ties", "tri_first_on_ties", "tri_claims",
           "tri_bestdist_before_epipolar", "tri_epipole_on_stereo", "bin_half_even", "no_bin_wrap")
K_BOW2_CLASSES = ("two_free", "one_free_d3", "scan", "small_node")


def feature_vector(fs):
    """the FeatureVector as the std::map it is: node id -> list of feature indices, in list order"""
    off = fs["node_off"]
    return {int(i): [int(v) for v in fs["feat"][off[j]:off[j + 1]]] for j, i in enumerate(fs["node_id"])}


def shared_nodes(fv1, fv2):
    """the merge walk with lower_bound (:193-279): the ids both maps hold, ascending"""
    return sorted(set(fv1) & set(fv2))


def distance(a, b):
    """DescriptorDistance (:1733-1752): the Hamming distance of two 256-bit descriptors"""
    return int(POP[np.bitwise_xor(a, b)].sum())


def rotation_bin(a1, a2, mutant=()):
    """:253-258: factor = 1.0f / HISTO_LENGTH; rot = a1 - a2 in float, + 360.0f when negative (-0.0 is not); bin = round(rot * factor),
    half away from zero; bin == HISTO_LENGTH -> 0.  (With this factor a difference of angles in [0, 360) ends in bins 0..12; the wrap
    needs rot >= 885.)"""
    factor = f32(1) / f32(HISTO_LENGTH)
    rot = f32(a1) - f32(a2)
    if rot < 0.0:
        rot = f32(rot + f32(360))
    v = float(f32(rot * factor))
    if "bin_half_even" in mutant:
        b = int(round(v))                                # Python rounds half to even
    else:
        b = int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)
    if b == HISTO_LENGTH and "no_bin_wrap" not in mutant:
        b = 0
    return b


def compute_three_maxima(histo):
    """:1687-1728, on a list of lists: strict '>' (among equal bins the lowest ranks first), 0.1f * (float)max1 in float"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, h in enumerate(histo):
        s = len(h)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def _filter(histo, out, mutant=()):
    """:282-300 / :681-699 / :839-858: every entry of a bin outside the three maxima is cleared; returns how many"""
    ind = compute_three_maxima(histo)
    n = 0
    for i, h in enumerate(histo):
        if i in ind:
            continue
        for j in h:
            out[j] = -1
            n += 1
    return n


def _ratio_ok(b1, b2, ratio, mutant=()):
    """:244 / :647: static_cast<float>(bestDist1) < mfNNratio * static_cast<float>(bestDist2), a float product"""
    if "ratio_double" in mutant:
        return float(b1) < float(f32(ratio)) * float(b2)          # mfNNratio is a float member: the defect is the PRODUCT in double
    return bool(f32(b1) < f32(ratio) * f32(b2))


def _greedy(mode, s1, s2, ratio, check_ori, mutant):
    """the walk the two SearchByBoW share.  mode 0 = (KF,F): result indexed by the frame feature, gate bestDist1 <= TH_LOW (:242), the
    histogram stores the FRAME index (:260); mode 1 = (KF,KF): result indexed by the first keyframe's feature, gate bestDist1 < TH_LOW
    (:644), columns need a good MapPoint too (:620-626), the histogram stores the FIRST-side index (:661).

    Report, per first-side row that takes part (has its flag, in a shared node): dict with
      steal      its best column over all columns of the node that take part was already taken, at a distance <= TH_LOW
      rematched  ... and the row matched another column
      ratio_rej  the gate held, the ratio test rejected
      tie        best1 == best2 at best1 <= TH_LOW;   d50 / d49: best1 == 50 / 49;   ratio_eq: float(best1) == ratio * float(best2) exactly
      matched    the column's feature index or -1 (before the orientation filter)
      k_bow2     the row's class by the rule of k_bow2 (orb-slam2_amd/csrc/orbx_bow.hip, "the throughput form without a distance
                 table"): None when its smallest distance over all columns fails the gate (it leaves at once), "small_node" for a node of
                 at most three columns, "two_free" when two of the three smallest keys (distance, column) are free, "one_free_d3" when one
                 is and the gate fails or best1 < ratio * d3 already holds, else "scan" (the row walks the node again)"""
    fv1, fv2 = feature_vector(s1), feature_vector(s2)
    n_out = len(s2["desc"]) if mode == 0 else len(s1["desc"])
    out = np.full(n_out, -1, np.int32)
    taken = np.zeros(len(s2["desc"]), bool)             # vpMapPointMatches[realIdxF] != NULL (:222) / vbMatched2 (:622)
    histo = [[] for _ in range(HISTO_LENGTH + 1)]       # (one bin more: only the no_bin_wrap mutant reaches it)
    le = (mode == 0) != ("kf_f_strict" in mutant if mode == 0 else "kf_kf_le" in mutant)

    def gate(d):
        return d <= TH_LOW if le else d < TH_LOW
    rows = {}
    nmatches = 0
    for node in shared_nodes(fv1, fv2):
        l1, l2 = fv1[node], fv2[node]
        cols = [j for j in l2 if mode == 0 or s2["flag"][j]]
        D = POP[np.bitwise_xor(s1["desc"][l1][:, None, :], s2["desc"][l2][None, :, :])].sum(-1)
        pos = {j: p for p, j in enumerate(l2)}
        for r, i1 in enumerate(l1):
            if not s1["flag"][i1]:
                continue
            best1, best2, best_idx = 256, 256, -1
            for j in cols:
                if taken[j] and "no_claims" not in mutant:
                    continue
                dist = int(D[r, pos[j]])
                if dist < best1 or ("greedy_last_on_ties" in mutant and dist == best1 and best_idx >= 0):
                    best2, best1, best_idx = best1, dist, j
                elif dist < best2:
                    best2 = dist
            rep = dict(node=node, steal=False, rematched=False, ratio_rej=False, tie=best1 <= TH_LOW and best1 == best2, d50=best1 == 50,
                       d49=best1 == 49, ratio_eq=best1 <= TH_LOW and float(f32(best1)) == float(f32(ratio) * f32(best2)), matched=-1,
                       k_bow2=None)
            keys = sorted((int(D[r, pos[j]]), pos[j], j) for j in cols)
            if keys:
                rep["steal"] = bool(taken[keys[0][2]]) and keys[0][0] <= TH_LOW
                if gate(keys[0][0]):
                    free = [k for k in keys[:3] if not taken[k[2]]]
                    if len(keys) <= 3:
                        rep["k_bow2"] = "small_node"
                    elif len(free) >= 2:
                        rep["k_bow2"] = "two_free"
                    elif len(free) == 1 and (not gate(free[0][0]) or bool(f32(free[0][0]) < f32(ratio) * f32(keys[2][0]))):
                        rep["k_bow2"] = "one_free_d3"
                    else:
                        rep["k_bow2"] = "scan"
            if gate(best1):
                if _ratio_ok(best1, best2, ratio, mutant):
                    if mode == 0:
                        out[best_idx] = i1
                    else:
                        out[i1] = best_idx
                    taken[best_idx] = True
                    rep["matched"] = best_idx
                    rep["rematched"] = rep["steal"]
                    if check_ori:
                        b = rotation_bin(s1["angle"][i1], s2["angle"][best_idx], mutant)
                        histo[b].append(best_idx if mode == 0 else i1)
                    nmatches += 1
                else:
                    rep["ratio_rej"] = True
            rows[i1] = rep
    if check_ori:
        nmatches -= _filter(histo[:HISTO_LENGTH], out, mutant)   # a mutant's bin 30 is outside the histogram the filter scans: it stays
    return out, nmatches, dict(rows=rows)


def search_by_bow_kf_f(kf, f, ratio, check_ori, mutant=()):
    """SearchByBoW(pKF, F) -> (match_f int32[nF]: the keyframe feature per frame feature or -1, nmatches, report)"""
    return _greedy(0, kf, f, ratio, check_ori, mutant)


def search_by_bow_kf_kf(k1, k2, ratio, check_ori, mutant=()):
    """SearchByBoW(pKF1, pKF2) -> (match12 int32[n1]: the second keyframe's feature per first-side feature or -1, nmatches, report)"""
    return _greedy(1, k1, k2, ratio, check_ori, mutant)


def greedy_counts(report):
    """class counts of a greedy report"""
    rows = report["rows"].values()
    c = {k: sum(bool(r[k]) for r in rows) for k in ("steal", "rematched", "ratio_rej", "tie", "d50", "d49", "ratio_eq")}
    c["rows"] = len(report["rows"])
    c["matches"] = sum(r["matched"] >= 0 for r in rows)
    for k in K_BOW2_CLASSES:
        c[k] = sum(r["k_bow2"] == k for r in rows)
    return c


def check_dist_epipolar_line(x1, y1, x2, y2, F12, sigma2, mutant=()):
    """:147-164: a, b, c, num, den, dsqr are floats, every product and sum rounded; den == 0 rejects; the last comparison is in double
    (3.84 is a double constant, mvLevelSigma2 a float)"""
    F = np.asarray(F12, f32).reshape(3, 3)
    x1, y1, x2, y2 = f32(x1), f32(y1), f32(x2), f32(y2)
    a = f32(f32(f32(x1 * F[0, 0]) + f32(y1 * F[1, 0])) + F[2, 0])
    b = f32(f32(f32(x1 * F[0, 1]) + f32(y1 * F[1, 1])) + F[2, 1])
    c = f32(f32(f32(x1 * F[0, 2]) + f32(y1 * F[1, 2])) + F[2, 2])
    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
    den = f32(f32(a * a) + f32(b * b))
    if den == 0:
        return False
    dsqr = f32(f32(num * num) / den)
    return float(dsqr) < 3.84 * float(f32(sigma2))


def search_for_triangulation(k1, k2, F12, ex, ey, scale_factors2, level_sigma2_2, check_ori, only_stereo, mutant=()):
    """SearchForTriangulation -> (pairs int32[npairs, 2] in first-side order (:860-868), report).

    bestDist starts at TH_LOW and a column is skipped when dist > TH_LOW || dist > bestDist (:763, :786): a distance of 50 is accepted and
    an EQUAL distance replaces, so the LAST column wins ties.  This version of the reference never sets vbMatched2 (:806-823 assign
    vMatches12 only): rows are independent.  The epipole test (:791-797) runs only when both keypoints are monocular, in float:
    distex * distex + distey * distey < 100 * mvScaleFactors[octave].  bestDist moves only when CheckDistEpipolarLine holds (:799-803).
    The histogram stores the first-side index (:821).

    Report, per first-side row that takes part: dict(within = columns within TH_LOW among those that take part, epipole = how many of them
    the epipole test rejects, epipolar = how many CheckDistEpipolarLine rejects, passing = the rest, closest_rejected = the column of
    smallest distance was rejected while a worse one won, tie_last = two passing columns tied at the smallest passing distance, d50 = the
    row matched at distance exactly 50, matched)"""
    fv1, fv2 = feature_vector(k1), feature_vector(k2)
    sf2 = np.asarray(scale_factors2, f32)
    sg2 = np.asarray(level_sigma2_2, f32)
    ex, ey = f32(ex), f32(ey)
    n1 = len(k1["desc"])
    matches12 = np.full(n1, -1, np.int32)
    matched2 = np.zeros(len(k2["desc"]), bool)
    histo = [[] for _ in range(HISTO_LENGTH + 1)]
    rows = {}
    for node in shared_nodes(fv1, fv2):
        l1, l2 = fv1[node], fv2[node]
        D = POP[np.bitwise_xor(k1["desc"][l1][:, None, :], k2["desc"][l2][None, :, :])].sum(-1)
        for r, idx1 in enumerate(l1):
            if k1["flag"][idx1]:                                   # already a MapPoint (:747-751)
                continue
            stereo1 = bool(k1["u_right"][idx1] >= 0)
            if only_stereo and not stereo1:
                continue
            best_dist, best_idx2 = TH_LOW, -1
            rep = dict(node=node, within=0, epipole=0, epipolar=0, passing=0, closest_rejected=False, tie_last=False, d50=False, matched=-1)
            seen = []                                              # (dist, passed) of the columns within TH_LOW, all of them judged
            for p, idx2 in enumerate(l2):
                if k2["flag"][idx2] or (matched2[idx2] and "tri_claims" in mutant):
                    continue
                stereo2 = bool(k2["u_right"][idx2] >= 0)
                if only_stereo and not stereo2:
                    continue
                dist = int(D[r, p])
                if dist > TH_LOW:
                    continue
                # the report judges every column within TH_LOW on its own, whatever bestDist is by now
                near = False
                if (not stereo1 and not stereo2) or "tri_epipole_on_stereo" in mutant:
                    distex = f32(ex - f32(k2["x"][idx2]))
                    distey = f32(ey - f32(k2["y"][idx2]))
                    near = bool(f32(f32(distex * distex) + f32(distey * distey)) < f32(f32(100) * sf2[k2["octave"][idx2]]))
                line = (not near) and check_dist_epipolar_line(k1["x"][idx1], k1["y"][idx1], k2["x"][idx2], k2["y"][idx2], F12,
                                                               sg2[k2["octave"][idx2]], mutant)
                rep["within"] += 1
                rep["epipole"] += near
                rep["epipolar"] += (not near) and (not line)
                rep["passing"] += line
                seen.append((dist, bool(line)))
                # the walk itself
                if dist > best_dist or ("tri_first_on_ties" in mutant and dist == best_dist and best_idx2 >= 0):
                    continue
                if near:
                    continue
                if "tri_bestdist_before_epipolar" in mutant:
                    best_dist = dist
                if line:
                    best_idx2, best_dist = idx2, dist
            if best_idx2 >= 0:
                matches12[idx1] = best_idx2
                matched2[best_idx2] = True
                rep["matched"] = best_idx2
                ok = [d for d, passed in seen if passed]
                rep["d50"] = min(ok) == 50
                rep["tie_last"] = ok.count(min(ok)) >= 2
                rep["closest_rejected"] = min(d for d, _ in seen) < min(ok)
                if check_ori:
                    histo[rotation_bin(k1["angle"][idx1], k2["angle"][best_idx2], mutant)].append(idx1)
            rows[idx1] = rep
    if check_ori:
        _filter(histo[:HISTO_LENGTH], matches12, mutant)
    idx = np.nonzero(matches12 >= 0)[0]
    pairs = np.stack([idx, matches12[idx]], axis=1).astype(np.int32).reshape(-1, 2)
    return pairs, dict(rows=rows)


def triangulation_counts(report):
    rows = list(report["rows"].values())
    return dict(rows=len(rows), within=sum(r["within"] for r in rows), epipole=sum(r["epipole"] for r in rows),
                epipolar=sum(r["epipolar"] for r in rows), multi=sum(r["passing"] >= 2 for r in rows),
                closest_rejected=sum(r["closest_rejected"] for r in rows), tie_last=sum(r["tie_last"] for r in rows),
                d50=sum(r["d50"] for r in rows), matches=sum(r["matched"] >= 0 for r in rows))
