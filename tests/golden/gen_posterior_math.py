#!/usr/bin/env python3
"""Generate tests/golden/posterior_math.json: the posterior over the support points and the two summaries a fit reports of
a prediction matrix, as exact mathematics (mpmath, 50 digits).  Neither the oracle nor the product is imported.

    q[s][p]     = w[p] exp(ll[s][p] - lpyl[s]) where w[p] > 0, else 0         the posterior of subject s (unnormalised
                                                                              where lpyl is not the mixture's own)
    mean[row]   = sum_p q pred[row][p] / sum_p q   over the columns with q > 0
    median[row] = the smallest pred[row][p], q > 0, with sum_{p': pred[row][p'] <= v} q >= sum_p q / 2   (lower weighted median)
    q = q[s(row)][.] (mode `posterior`) or w (mode `population`)

Inputs are not stored: they come from integer arithmetic that the tests restate (`inputs`, `apply_edits` below,
tests/posterior_cases.py), in float64 operations that every IEEE machine rounds alike.  The file holds seeds, shapes,
edits, truths, bars and a checksum of the inputs.

    r(s, p)   = (s * 2654435761 + p * 40503 + seed) mod 1000003
    ll[s][p]  = -((2.5 scale + 1) + scale * (r / 1000003))
    w[p]      = (((p * 7919 + seed * 31) mod 1009) + 1) / (1009 * P)
    lpyl[s]   = max_p ll[s][p] - ((s * 7 + seed) mod 9) / 4          doubles next to what a mixture would give
    pred[i][p] = -3 + 20 * (((i * 2246822519 + p * 3266489917 + seed * 7) mod 1000033) / 1000033)     both signs occur

Scales 5, 300 and 1e4: at the last two w exp(ll) underflows everywhere.  S = 9: subjects of 7, 1, 2, 40, 1, 2, 7, 1, 2
rows, so that a row that reads its neighbour's posterior is caught (40 rows: more than one chunk of rows); S = 5: 2, 1,
7, 1, 2; S = 1: 2 rows.  P = 4100 comes with one subject of 3 rows.  Every P has an S = 9 case (`edges`, scale 300) and
an S = 5 case (kinds and scales 5 / 1e4 in turn).
Every truth is computed, a sample is stored, to keep the file small: q for the columns `cols` (both ends, five spread
evenly, everything an edit touches) of the subjects `subs` (first, last, two between, everything an edit touches); means
and medians, in both modes, for the rows `kept` (each subject's first and last, rows 15, 16, 17, 31, 32 of a long
subject, everything an edit touches).  null: all.  The tests hold what is not stored to the float64 restatement, which
the stored entries hold to their bars; the median margin below is checked for EVERY row, stored or not.

Edits (applied in order; values are float.hex strings):
    {"ll": [s, p], "value": v}   {"ll_row": s, "value": v}   {"w": p, "value": v}   {"lpyl": s, "value": v}
    {"w_only": [a, b], "values": [va, vb]}      every weight 0 but these
    {"pred": [i, p], "value": v}   {"pred_col": p, "value": v}
    {"pred_round": i}                           row i rounded to integers (numpy.round): some twenty values, many times each
Kinds: `plain`; `edges` (a zero-weight column that holds NaN in ll and in pred; an ll = -inf entry; a NaN prediction under
positive weight in the last row; subject 0 with all entries -inf and lpyl = -inf; a row of duplicates); `heavy` (one
column carries more than half the weight; a row of duplicates; a NaN in ll under positive weight in the last subject - a
failed pair that poisons that subject's rows and nobody else's); `two` (weight on two columns only, 3/8 and 5/8).

Truth rules at the edges, as the C header states them: a column with w == 0 is skipped whatever it holds; ll = -inf
gives q = 0; a NaN q poisons the subject's rows; a NaN prediction under q > 0 gives NaN for that row; no column with
q > 0: NaN.

Bars are derived, not measured; u = 2^-53.
    q      x = ll - lpyl:  bar = 4 u q (|x| + 3) + 2^-1021      (stored: 4 u (|x| + 3), the bar's share of q)
           the difference is rounded (relative error u |x| in the exp), the exp and the product are rounded; a q below
           the normal range may be flushed to zero or carry a denormal's absolute error: two smallest normals of room.
    mean   D = sum q, e_p = |x_p| + 3:
           bar = 4 u (sum q |v| (e_p + P) / D + |mean| (sum q e_p / D + P))
           every q carries its relative error u e_p into numerator and denominator; each product is rounded; P - 1
           additions in ANY order lose at most (P - 1) u of the sum of magnitudes on either side; the division is rounded.
           Population mode: x = 0.
Both hold for every summation order.  The median is an element of the row and is held to equality; every row's median
has the cumulative weights on both sides of the selected element at least 1e-9 of the total away from half the total,
so that no summation order can move it - a case that violates this is generated again under another seed.

The generator checks that a plain sequential float64 implementation stays inside every bar and picks every median, and
that each of six deliberately wrong implementations moves some case by >= 1000 bars, turns a finite truth non-finite or
changes a median: q without the factor w; the row's subject off by one; the median one element too high; the unweighted
median; a zero-weight column not skipped; the unshifted formula w exp(ll) / sum.

Run:  python tests/golden/gen_posterior_math.py     (deterministic; a few minutes)
"""
import base64
import hashlib
import json
import math
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "posterior_math.json")

U = mp.mpf(2) ** -53
TINY = mp.mpf(2) ** -1021
GAP = mp.mpf("1e-9")
PS = [1, 2, 63, 64, 65, 130, 1000, 1024, 1025]
ROWS = {9: [7, 1, 2, 40, 1, 2, 7, 1, 2], 5: [2, 1, 7, 1, 2], 1: [2]}
SECOND = [("plain", 5.0), ("heavy", 1.0e4), ("two", 5.0), ("plain", 1.0e4)]  # the S = 5 case of the i-th P: SECOND[i % 4]
MODES = ("population", "posterior")


# ---- the inputs: restated by the tests ------------------------------------------------------------------------------
def inputs(rows, P, scale, seed):
    S = len(rows)
    s = np.arange(S, dtype=np.int64)[:, None]
    p = np.arange(P, dtype=np.int64)[None, :]
    r = (s * 2654435761 + p * 40503 + seed) % 1000003
    ll = -((2.5 * scale + 1.0) + scale * (r.astype(np.float64) / 1000003.0))
    w = (((p[0] * 7919 + seed * 31) % 1009) + 1).astype(np.float64) / (1009.0 * P)
    lpyl = ll.max(axis=1) - 0.25 * ((s[:, 0] * 7 + seed) % 9).astype(np.float64)
    i = np.arange(int(np.sum(rows)), dtype=np.int64)[:, None]
    r2 = (i * 2246822519 + p * 3266489917 + seed * 7) % 1000033
    pred = -3.0 + 20.0 * (r2.astype(np.float64) / 1000033.0)
    return ll, w, lpyl, pred


def apply_edits(edits, ll, w, lpyl, pred):
    for e in edits:
        if "ll" in e:
            ll[e["ll"][0], e["ll"][1]] = float.fromhex(e["value"])
        elif "ll_row" in e:
            ll[e["ll_row"], :] = float.fromhex(e["value"])
        elif "w" in e:
            w[e["w"]] = float.fromhex(e["value"])
        elif "w_only" in e:
            w[:] = 0.0
            for p, v in zip(e["w_only"], e["values"]):
                w[p] = float.fromhex(v)
        elif "lpyl" in e:
            lpyl[e["lpyl"]] = float.fromhex(e["value"])
        elif "pred" in e:
            pred[e["pred"][0], e["pred"][1]] = float.fromhex(e["value"])
        elif "pred_col" in e:
            pred[:, e["pred_col"]] = float.fromhex(e["value"])
        elif "pred_round" in e:
            pred[e["pred_round"], :] = np.round(pred[e["pred_round"], :])
        else:
            raise KeyError(str(e))


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def all_or(picked, n):
    return None if len(picked) >= n else sorted(picked)


def sample_cols(P, edits):
    """q's stored columns: both ends, five spread evenly, everything an edit touches"""
    return all_or({0, 1, 2, P - 3, P - 2, P - 1} | {(i * (P - 1)) // 6 for i in range(1, 6)} | touched_columns(edits), P) if P > 12 else None


def sample_subs(S, edits):
    """q's stored subjects: first, last, two between, everything an edit touches"""
    touched = {e["ll"][0] for e in edits if "ll" in e} | {e[k] for e in edits for k in ("ll_row", "lpyl") if k in e}
    return all_or({0, S // 3, S // 2, S - 1} | touched, S)


def sample_rows(rows, edits):
    """the rows whose mean and median are stored: each subject's first and last, rows 15, 16, 17, 31, 32 of a subject
    (the ends of its chunks of 16), everything an edit touches"""
    keep = {e["pred"][0] for e in edits if "pred" in e} | {e["pred_round"] for e in edits if "pred_round" in e}
    first = 0
    for n in rows:
        keep |= {first, first + n - 1} | {first + k for k in (15, 16, 17, 31, 32) if k < n}
        first += n
    return all_or(keep, first)


NEG_INF, NAN, ZERO = float("-inf").hex(), float("nan").hex(), (0.0).hex()


def edits_of(kind, S, P, n_rows):
    e = []
    if kind == "edges":
        if P >= 2:
            e += [{"w": P - 1, "value": ZERO}, {"ll": [S // 3, P - 1], "value": NAN}, {"pred_col": P - 1, "value": NAN}]
        e += [{"ll": [S // 2, P // 3], "value": NEG_INF}]
        if P >= 3:
            e += [{"pred": [n_rows - 1, 0], "value": NAN}]
            if n_rows > 1:
                e += [{"pred_round": 1}]
        if S >= 2:
            e += [{"ll_row": 0, "value": NEG_INF}, {"lpyl": 0, "value": NEG_INF}]
    elif kind == "heavy":
        if P >= 2:
            e += [{"w": P // 2, "value": (0.75).hex()}]
        e += [{"pred_round": 0}]
        if S >= 2:
            e += [{"ll": [S - 1, 0], "value": NAN}]
    elif kind == "two" and P >= 2:
        e += [{"w_only": [P // 4, P - 1 - P // 4], "values": [(0.375).hex(), (0.625).hex()]}]
    return e


def touched_columns(edits):
    cols = set()
    for e in edits:
        if "ll" in e:
            cols.add(e["ll"][1])
        elif "w" in e:
            cols.add(e["w"])
        elif "w_only" in e:
            cols |= set(e["w_only"])
        elif "pred_col" in e:
            cols.add(e["pred_col"])
    return cols


# ---- exact mathematics ----------------------------------------------------------------------------------------------
def pack(v, dtype="<f8"):
    return base64.b64encode(np.asarray(v, dtype=dtype).tobytes()).decode()


def pack_bars(bars):
    """float32, rounded towards zero so that no stored bar is wider than the derived one; NaN: the truth is not finite"""
    b = np.array([np.nan if x is None else x for x in bars], dtype=np.float64)
    b32 = b.astype(np.float32)
    b32 = np.where(b32.astype(np.float64) > b, np.nextafter(b32, np.float32(0.0)), b32)
    return pack(b32, "<f4"), [None if np.isnan(x) else float(x) for x in b32]


def exact_q(ll, w, lpyl):
    """per subject: a list of (q, |x|) per column, q an mpf, or None where q is NaN"""
    S, P = ll.shape
    out = []
    for s in range(S):
        row = []
        for p in range(P):
            a, b = float(ll[s, p]), float(lpyl[s])
            if not w[p] > 0.0 or a == -np.inf:
                row.append((mp.mpf(0), mp.mpf(0)))
            elif np.isnan(a) or np.isnan(b) or np.isinf(a) or np.isinf(b):
                row.append((None, None))
            else:
                x = mp.mpf(a) - mp.mpf(b)
                row.append((mp.mpf(float(w[p])) * mp.exp(x), abs(x)))
        out.append(row)
    return out


class Retry(Exception):
    pass


def exact_row(qrow, v, P):
    """(mean, bar, median) of one prediction row v under the weights qrow [(q, |x|)]; non-finite: (nan, None, nan)"""
    nan = float("nan")
    if any(q is None for q, _ in qrow):
        return nan, None, nan
    cols = [p for p in range(P) if qrow[p][0] > 0]
    if not cols or any(np.isnan(v[p]) for p in cols):
        return nan, None, nan
    q = [qrow[p][0] for p in cols]
    e = [qrow[p][1] + 3 for p in cols]
    val = [mp.mpf(float(v[p])) for p in cols]
    D = mp.fsum(q)
    mean = mp.fsum(a * b for a, b in zip(q, val)) / D
    bar = 4 * U * (mp.fsum(a * abs(b) * (c + P) for a, b, c in zip(q, val, e)) / D
                   + abs(mean) * (mp.fsum(a * c for a, c in zip(q, e)) / D + P))
    order = sorted(range(len(cols)), key=lambda k: val[k])
    half, cum, k = D / 2, mp.mpf(0), 0
    while True:  # value by value: duplicates enter together
        below = cum
        v_here = val[order[k]]
        while k < len(order) and val[order[k]] == v_here:
            cum += q[order[k]]
            k += 1
        if cum >= half:
            if (half - below) / D < GAP or (cum - half) / D < GAP:
                raise Retry()
            return float(mean), float(bar), float(v_here)


# ---- a plain sequential float64 implementation, and the wrong ones -----------------------------------------------------
def f64_q(ll, w, lpyl, s, wrong=None):
    P = ll.shape[1]
    q = [0.0] * P
    if wrong == "unshifted":
        t = [w[p] * math.exp(ll[s, p]) if (w[p] > 0.0 and ll[s, p] != -np.inf and not np.isnan(ll[s, p])) else 0.0 for p in range(P)]
        tot = sum(t)
        return [x / tot if tot != 0.0 else float("nan") for x in t]
    for p in range(P):
        if not (w[p] > 0.0 or wrong == "zero_weight_included"):
            continue
        a = ll[s, p]
        if a == -np.inf:
            continue
        x = a - lpyl[s]
        ex = float("nan") if np.isnan(x) else (math.exp(x) if x < 709.0 else float("inf"))
        q[p] = ex if wrong == "no_w" else w[p] * ex
    return q


def f64_rows(mode, ll, w, lpyl, pred, obs_off, wrong=None):
    S, P = ll.shape
    mean, median = [], []
    for s in range(S):
        src = (s + 1) % S if wrong == "neighbour" else s
        if mode == "population":
            q = [float(w[p]) if (w[p] > 0.0 or wrong == "zero_weight_included") else 0.0 for p in range(P)]
        else:
            q = f64_q(ll, w, lpyl, src, wrong)
        for i in range(obs_off[s], obs_off[s + 1]):
            v = pred[i]
            cols = [p for p in range(P) if (q[p] > 0.0 or (wrong == "zero_weight_included" and w[p] == 0.0))]
            if any(np.isnan(q[p]) for p in range(P)) or not cols or any(np.isnan(v[p]) for p in cols):
                mean.append(float("nan"))
                median.append(float("nan"))
                continue
            num = den = 0.0
            for p in cols:
                num += q[p] * v[p]
                den += q[p]
            mean.append(num / den)
            order = sorted(cols, key=lambda p: v[p])
            if wrong == "unweighted":
                median.append(float(v[order[(len(order) - 1) // 2]]))
                continue
            cum, pick = 0.0, None
            for k, p in enumerate(order):
                if wrong == "upper" and cum >= 0.5 * den:
                    pick = p
                    break
                cum += q[p]
                if wrong != "upper" and cum >= 0.5 * den:
                    pick = p
                    break
            median.append(float(v[pick if pick is not None else order[-1]]))
    return np.array(mean), np.array(median)


def shares(got, truths, bars):
    out = []
    for g, t, b in zip(got, truths, bars):
        if b is None:
            out.append(0.0 if ((np.isnan(g) and np.isnan(t)) or g == t) else np.inf)
        else:
            out.append(abs(g - t) / b if np.isfinite(g) else np.inf)
    return out


def same_medians(got, truth):
    return bool(np.all((got == truth) | (np.isnan(got) & np.isnan(truth))))


def build_case(kind, rows, P, scale, seed):
    S, n_rows = len(rows), int(sum(rows))
    ll, w, lpyl, pred = inputs(rows, P, scale, seed)
    edits = edits_of(kind, S, P, n_rows)
    apply_edits(edits, ll, w, lpyl, pred)
    obs_off = [0] + list(np.cumsum(rows))
    q = exact_q(ll, w, lpyl)
    cols, subs, kept = sample_cols(P, edits), sample_subs(S, edits), sample_rows(rows, edits)
    q_at = [(s, p) for s in (subs if subs is not None else range(S)) for p in (cols if cols is not None else range(P))]
    q_truth, q_bars = [], []
    for s, p in q_at:
        v, ax = q[s][p]
        q_truth.append(float("nan") if v is None else float(v))
        q_bars.append(None if v is None else float(4 * U * (ax + 3)))  # as a share of q: q itself may be below float32's range
    q_packed, q_bars = pack_bars(q_bars)
    q_bars = [None if b is None else b * t + float(TINY) for b, t in zip(q_bars, q_truth)]
    case = dict(kind=kind, S=S, P=P, rows=list(rows), scale=scale, seed=seed, edits=edits, checksum=checksum(ll, w, lpyl, pred),
                cols=cols, subs=subs, kept=kept, q=pack(q_truth), q_bar=q_packed)
    wq = [(mp.mpf(float(w[p])) if w[p] > 0.0 else mp.mpf(0), mp.mpf(0)) for p in range(P)]
    keep = list(range(n_rows)) if kept is None else kept
    truths = {}
    for mode in MODES:
        mean, bars, median = [], [], []
        for s in range(S):
            for i in range(obs_off[s], obs_off[s + 1]):  # every row: the median's margin is checked here (Retry)
                m, b, md = exact_row(wq if mode == "population" else q[s], pred[i], P)
                mean.append(m)
                bars.append(b)
                median.append(md)
        packed, _ = pack_bars([bars[i] for i in keep])
        _, bars = pack_bars(bars)
        case[mode] = dict(mean=pack([mean[i] for i in keep]), mean_bar=packed, median=pack([median[i] for i in keep]))
        truths[mode] = (np.array(mean), bars, np.array(median))
    return case, (ll, w, lpyl, pred, obs_off), truths, (q_at, q_truth, q_bars)


def main():
    cases = []
    worst = {"q": 0.0, "mean": 0.0}
    moved = {k: False for k in ("no_w", "neighbour", "upper", "unweighted", "zero_weight_included", "unshifted")}
    seed = 3000
    plan = []
    for i, P in enumerate(PS):
        plan += [("edges", ROWS[9], P, 300.0), (SECOND[i % 4][0], ROWS[5], P, SECOND[i % 4][1])]
    plan += [("plain", ROWS[1], 64, 1.0e4), ("edges", [3], 4100, 300.0)]
    for kind, rows, P, scale in plan:
        while True:
            seed += 1
            try:
                case, (ll, w, lpyl, pred, obs_off), truths, (q_at, q_truth, q_bars) = build_case(kind, rows, P, scale, seed)
                break
            except Retry:
                print(f"  seed {seed}: a median too close to half the weight, generated again", flush=True)
        cases.append(case)
        S = len(rows)
        got_q = [f64_q(ll, w, lpyl, s)[p] for s, p in q_at]
        sh = shares(got_q, q_truth, q_bars)
        assert max(sh) <= 1.0, (kind, S, P, scale, "q", max(sh))
        worst["q"] = max(worst["q"], max(sh))
        for mode in MODES:
            t_mean, bars, t_median = truths[mode]
            mean, median = f64_rows(mode, ll, w, lpyl, pred, obs_off)
            sh = shares(mean, t_mean, bars)
            assert max(sh) <= 1.0, (kind, S, P, scale, mode, max(sh))
            assert same_medians(median, t_median), (kind, S, P, scale, mode)
            worst["mean"] = max(worst["mean"], max(sh))
            for wrong in moved:
                if moved[wrong] or (mode == "population" and wrong in ("no_w", "neighbour", "unshifted")):
                    continue
                mean, median = f64_rows(mode, ll, w, lpyl, pred, obs_off, wrong)
                moved[wrong] = max(shares(mean, t_mean, bars)) >= 1000.0 or not same_medians(median, t_median)
        print(f"{kind} {S} x {P} scale {scale:g} done", flush=True)
    for wrong, did in moved.items():
        assert did, f"the wrong implementation '{wrong}' moves no case by 1000 bars and changes no median"
    print("sequential float64, worst share of a bar: q %.3f, mean %.3f" % (worst["q"], worst["mean"]))
    doc = dict(about="tests/golden/gen_posterior_math.py; q / mean / median: base64 of little-endian float64, q_bar / mean_bar: "
                     "of float32 (NaN: the truth is not finite and is matched in kind and sign)", cases=cases)
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
