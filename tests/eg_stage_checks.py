"""What tests/test_eg_stages.py asks of a stage dump (orbx.eg_stages), as functions of the problem and the dump alone, so that
tests/test_eg_stages_model.py can put the same questions to tests/eg_model.py's stages(): the honest model passes every check, and
every deliberate error of the model fails the check named for it in SEEN_BY.  A check returns the list of what it found wrong.

The equal-bytes checks restate one stage each FROM THE DUMP'S OWN INPUT OF THAT STAGE (the record from the dump's err, the rows from the
dump's rec, the scatter from the dump's Hd / Off / bv, the scale sums from the dump's x and bv), one numpy operation at a time in the order
include/orbx.h states, so nothing but + - x / is between the two sides and no tolerance is needed.  They do not import eg_model.

The comparisons with the model (err, trial) are per row: row_diff() scales a row's largest difference by max(1, |value|), row_bounds() gives
every row 64 x its own spread across the model's nudge settings None, 1, 2 (64: the project's margin, tests/test_lba.py), the spread floored
at the table's median row spread so that a row no seeded nudge happens to move is not held to zero."""
import math

import numpy as np

SCALAR = 1.0 / (2 * 1e-9)
MARGIN = 64
NUDGES = (None, 1, 2)
# mutation -> (the check that sees it, "bytes" | "bound")
SEEN_BY = {
    "g_sign": ("record", "bytes"), "plus_minus_swapped": ("record", "bytes"), "ij_blocks_swapped": ("record", "bytes"),
    "fixed_not_zeroed": ("record", "bytes"), "measurement_inverted": ("setup", "bytes"), "lambda_off_diagonal": ("scatter", "bytes"),
    "y_not_b": ("scatter", "bytes"), "scale_without_lambda": ("update", "bytes"), "b_minus_one": ("err", "bound"), "lu_wrong_row": ("err", "bound"),
    "normal_from_vscw": ("setup", "bytes"), "normalise": ("setup", "bytes"), "x6_not_zeroed": ("update", "bytes"), "bta_untransposed": ("rows", "bytes"),
}


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def where(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return f"shapes {a.shape} {b.shape}"
    bad = np.argwhere(a.view(np.int64) != b.view(np.int64)) if a.dtype == np.float64 and b.dtype == np.float64 else np.argwhere(a != b)
    return f"{len(bad)} entries, first {tuple(bad[0])}: {a[tuple(bad[0])]!r} {b[tuple(bad[0])]!r}" if len(bad) else "equal"


def chi2_rows(e):
    """eg_chi2 of [n][7]"""
    c = e[:, 0] * e[:, 0]
    for m in range(1, 7):
        c = c + e[:, m] * e[:, m]
    return c


def lists(pr):
    """rows, a row's (edge, end) and a pair's (edge, read transposed) in edge order, the pairs sorted by (higher row, lower row)"""
    fixed = np.asarray(pr["fixed"]).reshape(-1) != 0
    row = np.full(len(fixed), -1)
    row[~fixed] = np.arange(len(fixed) - 1)
    ei, ej = np.asarray(pr["edge_i"]).astype(int), np.asarray(pr["edge_j"]).astype(int)
    inc = [[] for _ in range(len(fixed) - 1)]
    pairs = {}
    for e in range(len(ei)):
        ri, rj = row[ei[e]], row[ej[e]]
        if ri >= 0:
            inc[ri].append((e, 0))
        if rj >= 0:
            inc[rj].append((e, 1))
        if ri >= 0 and rj >= 0:
            pairs.setdefault((max(ri, rj), min(ri, rj)), []).append((e, ri < rj))
    return row, ei, ej, inc, sorted(pairs.items())


def up14(r, c):
    return 14 * r - r * (r - 1) // 2 + (c - r)


def up7(r, c):
    return 7 * r - r * (r - 1) // 2 + (c - r)


def record_from_err(pr, err):
    """the 120-double record of every edge from its 29 evaluations [E][29][7]"""
    row, ei, ej, _, _ = lists(pr)
    E = len(ei)
    J = np.zeros((E, 7, 14))
    for c in range(14):
        has = (row[ei] >= 0) if c < 7 else (row[ej] >= 0)
        J[:, :, c] = np.where(has[:, None], SCALAR * (err[:, 1 + 2 * c] - err[:, 2 + 2 * c]), 0.0)
    rec = np.zeros((E, 120))
    for r in range(14):
        for c in range(r, 14):
            v = J[:, 0, r] * J[:, 0, c]
            for m in range(1, 7):
                v = v + J[:, m, r] * J[:, m, c]
            rec[:, up14(r, c)] = v
    for c in range(14):
        v = J[:, 0, c] * -err[:, 0, 0]
        for m in range(1, 7):
            v = v + J[:, m, c] * -err[:, 0, m]
        rec[:, 105 + c] = v
    rec[:, 119] = chi2_rows(err[:, 0])
    return rec


def check_setup(pr, d, model):
    """vS, meas (and xf's exact entries) against the model's: + - x / and sqrt alone"""
    bad = []
    for k in ("vS", "meas"):
        if not same(d[k], model[k]):
            bad.append(f"{k}: {where(d[k], model[k])}")
    return bad


def check_probe(pr, d):
    """the probe's evaluation 0 is the error the linearisation squared"""
    return [] if same(chi2_rows(d["err"][:, 0]), d["echi"]) else [f"eg_chi2(err[:, 0]) != echi: {where(chi2_rows(d['err'][:, 0]), d['echi'])}"]


def check_record(pr, d):
    bad = []
    rec = d["rec"]
    exp = record_from_err(pr, d["err"])
    if not same(rec, exp):
        bad.append(f"rec != the record of the dump's own err: {where(rec, exp)}")
    if not same(rec[:, 119], d["echi"]):
        bad.append("rec[119] != echi")
    row, ei, ej, _, _ = lists(pr)
    for end, idx in ((0, ei), (1, ej)):
        for e in np.nonzero(row[idx] < 0)[0]:
            cols = range(7 * end, 7 * end + 7)
            ent = [rec[e, up14(min(r, c), max(r, c))] for r in range(14) for c in cols] + [rec[e, 105 + c] for c in cols]
            if any(v != 0.0 for v in ent):
                bad.append(f"edge {e}: the blocks of its fixed end {end} are not zeros")
    if pr["fix_scale"]:
        ent = [rec[:, up14(min(r, c), max(r, c))] for r in range(14) for c in (6, 13)] + [rec[:, 105 + 6], rec[:, 105 + 13]]
        if any((v != 0.0).any() for v in ent):
            bad.append("fix_scale: rows and columns 6 and 13 are not zeros")
    return bad


def rows_from_rec(pr, rec):
    """Hd [F][28], bv [F][7], pair [NP][2], Off [NP][49]: the ordered sums of the records in edge order"""
    row, ei, ej, inc, pairs = lists(pr)
    F = len(inc)
    Hd, bv = np.zeros((F, 28)), np.zeros((F, 7))
    for r in range(F):
        for e, w in inc[r]:
            o = 7 * w
            Hd[r] = Hd[r] + np.array([rec[e, up14(o + a, o + c)] for a in range(7) for c in range(a, 7)])
            bv[r] = bv[r] + rec[e, 105 + o:105 + o + 7]
    Off = np.zeros((len(pairs), 49))
    for n, (_, lst) in enumerate(pairs):
        for e, transposed in lst:
            AtB = np.array([[rec[e, up14(r, 7 + s)] for s in range(7)] for r in range(7)])
            Off[n] = Off[n] + (AtB.T if transposed else AtB).reshape(49)
    return Hd, bv, np.array([k for k, _ in pairs], np.int32).reshape(-1, 2), Off


def check_rows(pr, d):
    bad = []
    Hd, bv, pair, Off = rows_from_rec(pr, d["rec"])
    if d["n_pairs"] != len(pair) or not np.array_equal(np.asarray(d["pair"]).reshape(-1, 2), pair):
        bad.append(f"the pair list: {np.asarray(d['pair']).tolist()} for {pair.tolist()}")
        return bad
    for k, exp in (("Hd", Hd), ("bv", bv), ("Off", Off)):
        if not same(d[k], exp):
            bad.append(f"{k} != the ordered sum of the dump's own rec: {where(d[k], exp)}")
    return bad


def check_scatter(pr, d, lam):
    """S's lower triangle = the blocks, lambda on the diagonal and nowhere else, zeros outside the blocks; y == bv"""
    bad = []
    F = len(d["bv"])
    n = 7 * F
    exp = np.zeros((n, n))
    Hd = np.asarray(d["Hd"])
    for r in range(F):
        for a in range(7):
            for c in range(a + 1):
                exp[7 * r + a, 7 * r + c] = Hd[r, up7(c, a)] + lam if a == c else Hd[r, up7(c, a)]
    for (hi, lo), blk in zip(np.asarray(d["pair"]).reshape(-1, 2), np.asarray(d["Off"]).reshape(-1, 7, 7)):
        exp[7 * hi:7 * hi + 7, 7 * lo:7 * lo + 7] = blk
    low = np.tril_indices(n)
    if not same(np.asarray(d["S"])[low], exp[low]):
        got = np.zeros((n, n)); got[low] = np.asarray(d["S"])[low]
        bad.append(f"S's lower triangle != the scatter: {where(got, exp)}")
    if not same(d["y"], np.asarray(d["bv"]).reshape(-1)):
        bad.append("y != bv")
    return bad


def check_update(pr, d, lam):
    """sc = the seven-term sum of the dump's own x and bv; under fix_scale x[6::7] == 0 and the trial's scales are the start's bits"""
    bad = []
    x, b = np.asarray(d["x"]), np.asarray(d["bv"]).reshape(-1)
    per = np.zeros(len(d["bv"]))
    for j in range(7):
        per = per + x[j::7] * (lam * x[j::7] + b[j::7])
    if not same(d["sc"], per):
        bad.append(f"sc != x (lambda x + b): {where(d['sc'], per)}")
    fixed = np.asarray(pr["fixed"]).reshape(-1) != 0
    if not same(np.asarray(d["trial"])[fixed], np.asarray(d["vS"])[fixed]):
        bad.append("the fixed keyframe's trial estimate is not its start")
    if pr["fix_scale"]:
        if (x[6::7] != 0.0).any():
            bad.append("fix_scale: x[6::7] != 0")
        if not same(np.asarray(d["trial"])[:, 7], np.asarray(d["vS"])[:, 7]):
            bad.append("fix_scale: a trial scale is not the start's")
    return bad


def check_status(pr, d, trial=True):
    """status[2] = the largest |diagonal entry| exactly; status[0] and status[1] = the sums of the dump's own echi and sc within 256 eps x
    the sum of the magnitudes (block_sum adds 256 strided partials by a butterfly: every term goes through at most
    ceil(E / 256) + 8 additions)"""
    bad = []
    eps = np.finfo(np.float64).eps
    diag = np.abs(np.asarray(d["Hd"])[:, [up7(k, k) for k in range(7)]])
    if d["status_lin"][2] != diag.max():
        bad.append(f"status[2] {d['status_lin'][2]!r} != the largest |diagonal| {diag.max()!r}")
    sums = [("status_lin[0]", d["status_lin"][0], d["echi"])]
    if trial:
        sums += [("status_trial[0]", d["status_trial"][0], d["echi_trial"]), ("status_trial[1]", d["status_trial"][1], d["sc"])]
    for name, got, terms in sums:
        ref = math.fsum(terms.tolist())
        tol = 256 * eps * math.fsum(np.abs(terms).tolist())
        print(f"{name}: {got!r} fsum {ref!r} difference {abs(got - ref):.3e} bound {tol:.3e}")
        if not abs(got - ref) <= tol:
            bad.append(f"{name} {got!r} != fsum {ref!r} within {tol:.3e}")
    return bad


# ---------------------------------------------------------------- per-row comparison with the model

def row_diff(ref, got):
    """per row (axis 0) the largest |ref - got| / max(1, |ref|)"""
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        q = np.abs(ref - got) / np.maximum(1.0, np.abs(ref))
    q = np.where(np.isnan(q) & (ref.view(np.int64) == got.view(np.int64)), 0.0, q)      # the same inf or NaN on both sides
    q = np.where(np.isnan(q), np.inf, q)
    return q.reshape(len(ref), -1).max(axis=1) if q.size else np.zeros(len(ref))


def row_spread(runs):
    """per row the largest row_diff between any two of the model's runs"""
    s = np.zeros(len(runs[0]))
    for a in range(len(runs)):
        for b in range(a + 1, len(runs)):
            s = np.maximum(s, row_diff(runs[a], runs[b]))
    return s


def row_bounds(runs):
    """-> (bound per row, spread per row, the floor)"""
    s = row_spread(runs)
    floor = float(np.median(s)) if len(s) else 0.0
    return MARGIN * np.maximum(s, floor), s, floor


# ---------------------------------------------------------------- which case of eg_scene.STAGE_CASES shows each mutation

MUTATION_CASES = {
    "g_sign": ("shape-edges-9",), "plus_minus_swapped": ("shape-edges-9",), "ij_blocks_swapped": ("shape-edges-9",),
    "fixed_not_zeroed": ("shape-edges-1", "shape-fixed-is-i"), "measurement_inverted": ("shape-edges-9",), "lambda_off_diagonal": ("shape-edges-9",),
    "y_not_b": ("shape-edges-9",), "scale_without_lambda": ("exp-free",), "b_minus_one": ("log-free", "log-fix"), "lu_wrong_row": ("log-free", "log-fix"),
    "normal_from_vscw": ("shape-edges-9",), "normalise": ("shape-edges-9",), "x6_not_zeroed": ("exp-fix",), "bta_untransposed": ("shape-edges-9",),
}


def run_check(name, pr, d, lam, honest):
    """the named check of a dump -> what it found wrong"""
    if name == "setup":
        return check_setup(pr, d, honest)
    if name in ("scatter", "update"):
        return globals()["check_" + name](pr, d, lam)
    return globals()["check_" + name](pr, d)


def rows_seeing(mutation, honest):
    """the rows of a log table's err that a mutation seen under the bound must move: those whose evaluation 0 takes the path the
    mutation changes -- for "b_minus_one" the branch (rotation < eps, scale >= eps) with a rotation that is not exactly zero (B multiplies
    Omega), for "lu_wrong_row" pivot row 2"""
    if mutation == "b_minus_one":
        return np.nonzero((honest["paths"]["log_rows"][0] == 2) & (np.abs(honest["err"][:, 0, :3]).max(axis=1) > 0.0))[0]
    if mutation == "lu_wrong_row":
        return np.nonzero(honest["paths"]["rows"][0][0] == 2)[0]
    raise KeyError(mutation)


def margin(mutation, runs, mutated):
    """-> (rows, the smallest of change / bound over them, the smallest change, the largest bound) for a mutation seen under the bound"""
    bound, _, _ = row_bounds([r["err"] for r in runs])
    rows = rows_seeing(mutation, runs[0])
    change = row_diff(runs[0]["err"], mutated["err"])[rows]
    with np.errstate(all="ignore"):
        ratio = change / bound[rows]
    return rows, float(ratio.min()) if len(rows) else math.inf, float(change.min()) if len(rows) else math.inf, float(bound[rows].max()) if len(rows) else 0.0
