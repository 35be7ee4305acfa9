#!/usr/bin/env python3
"""Generate tests/golden/mixture_math.json: the two reductions of a log-likelihood matrix, as exact mathematics (mpmath,
50 digits).  Neither the oracle nor the product is imported.

    lpyl[s] = ln sum_{p: w[p] > 0} w[p] exp(ll[s][p])          the mixture log-likelihood of subject s
    D[p]    = sum_s exp(ll[s][p] - lpyl[s]) - n_subjects       the D-function of candidate p (optimize/parameters.rs:30-52
                                                               returns -D, with p_i / pyl_i in place of the exp)

Inputs are not stored: they come from integer arithmetic that the tests restate (`inputs`, `apply_edits` below), in
float64 operations that every IEEE machine rounds alike.  The file holds seeds, shapes, edits, truths and bars, and a
checksum of the inputs so that a restatement that drifts is seen at once.

    r(s, p)  = (s * 2654435761 + p * 40503 + seed) mod 1000003
    ll[s][p] = -(offset + scale * (r / 1000003)),   offset = 2.5 * scale + 1
    w[p]     = (((p * 7919 + seed * 31) mod 1009) + 1) / (1009 * P)

    lpyl[s]  = max_p ll[s][p] - ((s * 7 + seed) mod 9) / 4       D's input: doubles next to what a mixture would give

Scales 5, 300 and 1e4: at 300 and 1e4 the unshifted formula underflows everywhere.  D's truth is the exact function of
the doubles a kernel is handed.  Shapes with more than 32 rows (lpyl) or columns (D) store the truths of a sample
(`sample`: both ends, 16 spread evenly, everything an edit touches; `rows` / `cols` in the case); the tests hold every
other entry to the float64 restatement, which these same truths hold to its bar.

Edits (a list per case, applied in order; values are float.hex strings, so -inf and nan are spelt out):
    {"ll": [s, p], "value": v}        one entry
    {"row": s, "value": v}            a whole row of ll
    {"w": p, "value": v}              one weight
    {"lpyl": s, "value": v}           one entry of D's lpyl
    {"ll_over": [s, p], "add": a}     ll[s][p] = lpyl[s] + a  (float64), a = 720: exp passes 709.78 and overflows
Four cases per shape and reduction: scales 5 and 1e4 `plain`, scale 300 with the edges edited in, twice.  Truths are
stored as base64 of little-endian float64, bars as float32 rounded towards zero (NaN: the truth is not finite).
Mixture: `skip` (a -inf entry, a zero weight, a NaN under that zero weight: truths finite, the NaN must not be seen;
nothing where P = 1); `poison` (the same, then a NaN under positive weight in the last row: NaN; row 0 all -inf: -inf -
the later edit wins where S = 1).  D: `over` (a
-inf entry: adds 0; one entry pushed past exp's range: that candidate is +inf); `lost` (a subject with lpyl = -inf: +inf for every candidate whose ll there is finite, NaN for the
one whose ll there is -inf too, IEEE's -inf - (-inf)).

Truth rules at the edges, as the C header states them: a column with w == 0 is skipped whatever it holds; ll = -inf
adds 0; all weighted entries -inf: -inf; a NaN under positive weight: NaN.  For D, IEEE decides as in the reference's
p_i / pyl_i: any NaN term: NaN; else any term whose exponent exceeds ln(DBL_MAX) or is +inf: +inf.

Bars are derived, not measured; u = 2^-53.
    lpyl   x_p = ll - max, t_p = w_p e^{x_p}, Sigma = sum t_p (over the weighted, finite entries)
           bar = 4 u (sum t_p (|x_p| + 3) / Sigma + (P - 1) + 2 |ln Sigma| + |truth| + 2)
           a term's exponent is a rounded difference (relative error u |x_p| in the term), its exp and its product with
           w are rounded (2 u), and it may be rescaled when the running maximum moves (the rescalings' exponents add up
           to at most |x_p|: the +3 leaves room); P - 1 additions in ANY order lose at most (P - 1) u of Sigma; ln Sigma
           and the final sum max + ln Sigma are rounded at their own magnitudes.
    D      x_s = ll - lpyl (lpyl the rounded doubles), T = sum_s e^{x_s}
           bar = 4 u (sum_s e^{x_s} (|x_s| + 2) + S T + T + S)
           the rounded difference and the exp per term, S - 1 additions in any order, the subtraction of S.
Both hold for every summation order, so a kernel may tile as it likes.  The generator checks that a plain sequential
float64 implementation stays inside every bar (it prints the worst share) and
that each of five deliberately wrong implementations moves some case by >= 1000 bars (or turns a finite truth
non-finite): no max shift; w read as ln w; zero-weight columns included; the - n_subjects forgotten; lpyl of the
neighbouring subject.

Run:  python tests/golden/gen_mixture_math.py     (deterministic; about a minute)
"""
import base64
import hashlib
import json
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mixture_math.json")

U = mp.mpf(2) ** -53
SHAPES = [(1, 1), (2, 3), (7, 63), (64, 64), (5, 65), (257, 130), (3, 1025), (1031, 7)]
SCALES = [5.0, 300.0, 1.0e4]
LN_DBL_MAX = mp.log(mp.mpf(2) ** 1024 - mp.mpf(2) ** 971)


# ---- the inputs: restated by the tests ------------------------------------------------------------------------------
def inputs(S, P, scale, seed):
    s = np.arange(S, dtype=np.int64)[:, None]
    p = np.arange(P, dtype=np.int64)[None, :]
    r = (s * 2654435761 + p * 40503 + seed) % 1000003
    ll = -((2.5 * scale + 1.0) + scale * (r.astype(np.float64) / 1000003.0))
    w = (((p[0] * 7919 + seed * 31) % 1009) + 1).astype(np.float64) / (1009.0 * P)
    lpyl = ll.max(axis=1) - 0.25 * ((s[:, 0] * 7 + seed) % 9).astype(np.float64)  # D's input: doubles next to the row's top
    return ll, w, lpyl


def sample(n, must=()):
    """which of n rows (lpyl) or columns (D) carry a stored truth: all up to 32; of more, the first and last 8, 16 spread
    evenly, and every one an edit touches.  The tests hold the others to the float64 restatement."""
    if n <= 32:
        return list(range(n))
    return sorted(set(range(8)) | set(range(n - 8, n)) | {(i * (n - 1)) // 17 for i in range(1, 17)} | set(must))


def apply_edits(edits, ll, w, lpyl=None):
    for e in edits:
        if "ll" in e:
            ll[e["ll"][0], e["ll"][1]] = float.fromhex(e["value"])
        elif "row" in e:
            ll[e["row"], :] = float.fromhex(e["value"])
        elif "w" in e:
            w[e["w"]] = float.fromhex(e["value"])
        elif "lpyl" in e:
            lpyl[e["lpyl"]] = float.fromhex(e["value"])
        elif "ll_over" in e:
            ll[e["ll_over"][0], e["ll_over"][1]] = lpyl[e["ll_over"][0]] + float.fromhex(e["add"])
        else:
            raise KeyError(str(e))


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


# ---- exact mathematics ----------------------------------------------------------------------------------------------
def pack(v, dtype="<f8"):
    return base64.b64encode(np.asarray(v, dtype=dtype).tobytes()).decode()


def pack_bars(bars):
    """float32, rounded towards zero so that no stored bar is wider than the derived one; NaN: the truth is not finite"""
    b = np.array([np.nan if x is None else x for x in bars], dtype=np.float64)
    b32 = b.astype(np.float32)
    b32 = np.where(b32.astype(np.float64) > b, np.nextafter(b32, np.float32(0.0)), b32)
    return pack(b32, "<f4"), [None if np.isnan(x) else float(x) for x in b32]


def exact_lpyl(ll, w, rows):
    """(truth as float, bar as float or None) per row of `rows`"""
    S, P = ll.shape
    truths, bars = [], []
    for s in rows:
        cols = [p for p in range(P) if w[p] > 0.0]
        if any(np.isnan(ll[s, p]) for p in cols):
            truths.append(float("nan"))
            bars.append(None)
            continue
        cols = [p for p in cols if ll[s, p] != -np.inf]
        if not cols:
            truths.append(-np.inf)
            bars.append(None)
            continue
        m = max(ll[s, p] for p in cols)
        x = [mp.mpf(float(ll[s, p])) - mp.mpf(float(m)) for p in cols]
        t = [mp.mpf(float(w[p])) * mp.exp(xp) for p, xp in zip(cols, x)]
        sigma = mp.fsum(t)
        truth = mp.mpf(float(m)) + mp.log(sigma)
        bar = 4 * U * (mp.fsum(tp * (abs(xp) + 3) for tp, xp in zip(t, x)) / sigma + (P - 1) + 2 * abs(mp.log(sigma))
                       + abs(truth) + 2)
        truths.append(float(truth))
        bars.append(float(bar))
    return truths, bars


def exact_d(ll, lpyl, cols):
    S, P = ll.shape
    truths, bars = [], []
    for p in cols:
        kind, e, bsum = "finite", [], []
        for s in range(S):
            a, b = float(ll[s, p]), float(lpyl[s])
            if np.isnan(a) or np.isnan(b) or (np.isinf(a) and np.isinf(b) and (a < 0) == (b < 0)):
                kind = "nan"
                break
            if a == -np.inf or b == np.inf:
                continue  # exp(-inf) = 0
            if a == np.inf or b == -np.inf or mp.mpf(a) - mp.mpf(b) > LN_DBL_MAX:
                kind = "inf"
                continue
            x = mp.mpf(a) - mp.mpf(b)
            ex = mp.exp(x)
            e.append(ex)
            bsum.append(ex * (abs(x) + 2))
        if kind != "finite":
            truths.append(float("nan") if kind == "nan" else np.inf)
            bars.append(None)
            continue
        T = mp.fsum(e)
        truths.append(float(T - S))
        bars.append(float(4 * U * (mp.fsum(bsum) + S * T + T + S)))
    return truths, bars


# ---- float64 implementations: the plain one, and the wrong ones -------------------------------------------------------
def f64_lpyl(ll, w, wrong=None):
    S, P = ll.shape
    out = np.empty(S)
    with np.errstate(all="ignore"):
        for s in range(S):
            cols = [p for p in range(P) if (w[p] > 0.0 or wrong == "zero_weight_included")]
            wt = [np.exp(w[p]) if wrong == "w_as_log" else w[p] for p in cols]
            x = [ll[s, p] for p in cols]
            fin = [v for v in x if v != -np.inf and not np.isnan(v)]
            m = 0.0 if (wrong == "no_shift" or not fin) else max(fin)
            acc = 0.0
            for v, ww in zip(x, wt):
                acc += ww * np.exp(v - m)
            out[s] = m + np.log(acc) if fin or np.isnan(acc) else -np.inf
    return out


def f64_d(ll, lpyl, wrong=None):
    S, P = ll.shape
    out = np.empty(P)
    with np.errstate(all="ignore"):
        for p in range(P):
            acc = 0.0
            for s in range(S):
                acc += np.exp(ll[s, p] - lpyl[(s + 1) % S if wrong == "neighbour" else s])
            out[p] = acc - (0.0 if wrong == "no_minus_n" else S)
    return out


def shares(got, truths, bars):
    """|got - truth| / bar per entry; inf where the kind or sign of a non-finite truth is missed"""
    out = []
    for g, t, b in zip(got, truths, bars):
        if b is None:
            same = (np.isnan(g) and np.isnan(t)) or (g == t)
            out.append(0.0 if same else np.inf)
        else:
            out.append(abs(g - t) / b if np.isfinite(g) else np.inf)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------
NEG_INF, NAN, ZERO = float("-inf").hex(), float("nan").hex(), (0.0).hex()


def mixture_edits(kind, S, P):
    if kind == "plain":
        return []
    e = []
    if P >= 2:
        e += [{"ll": [S // 2, P // 3], "value": NEG_INF}, {"w": P - 1, "value": ZERO}, {"ll": [S // 3, P - 1], "value": NAN}]
    if kind == "poison":
        e += [{"ll": [S - 1, 0], "value": NAN}, {"row": 0, "value": NEG_INF}]
    return e


def d_edits(kind, S, P):
    if kind == "plain":
        return []
    if kind == "over":
        e = [{"ll": [S // 2, P // 3], "value": NEG_INF}]
        if P >= 2 or S >= 2:
            e.append({"ll_over": [S - 1, P - 1], "add": (720.0).hex()})
        return e
    return [{"lpyl": S // 2, "value": NEG_INF}, {"ll": [S // 2, P // 2], "value": NEG_INF}]


def main():
    mixture, dfunction = [], []
    worst = {"lpyl": 0.0, "D": 0.0}
    moved = {k: 0.0 for k in ("no_shift", "w_as_log", "zero_weight_included", "no_minus_n", "neighbour")}
    kinds = {"lpyl": set(), "D": set()}  # the non-finite truths that occur
    seed = 1000
    for (S, P) in SHAPES:
        for scale, kind in [(5.0, "plain"), (300.0, "skip"), (1.0e4, "plain"), (300.0, "poison")]:
            seed += 1
            ll, w, _ = inputs(S, P, scale, seed)
            edits = mixture_edits(kind, S, P)
            apply_edits(edits, ll, w)
            rows = sample(S, [e["ll"][0] if "ll" in e else e["row"] for e in edits if "ll" in e or "row" in e])
            truths, bars = exact_lpyl(ll, w, rows)
            packed, bars = pack_bars(bars)
            mixture.append(dict(S=S, P=P, scale=scale, seed=seed, kind=kind, edits=edits, checksum=checksum(ll, w),
                                rows=rows if len(rows) < S else None, lpyl=pack(truths), bar=packed))
            kinds["lpyl"] |= {repr(float(v)) for v in truths if not np.isfinite(v)}
            sh = shares(f64_lpyl(ll, w)[rows], truths, bars)
            assert max(sh) <= 1.0, (S, P, scale, kind, max(sh))
            worst["lpyl"] = max(worst["lpyl"], max(sh))
            for wrong in ("no_shift", "w_as_log", "zero_weight_included"):
                moved[wrong] = max(moved[wrong], max(shares(f64_lpyl(ll, w, wrong)[rows], truths, bars)))
        for scale, kind in [(5.0, "plain"), (300.0, "over"), (1.0e4, "plain"), (300.0, "lost")]:
            seed += 1
            ll, w, lpyl = inputs(S, P, scale, seed)
            edits = d_edits(kind, S, P)
            apply_edits(edits, ll, w, lpyl)
            cols = sample(P, [(e.get("ll") or e["ll_over"])[1] for e in edits if "ll" in e or "ll_over" in e])
            truths, bars = exact_d(ll, lpyl, cols)
            packed, bars = pack_bars(bars)
            dfunction.append(dict(S=S, P=P, scale=scale, seed=seed, kind=kind, edits=edits, checksum=checksum(ll, lpyl),
                                  cols=cols if len(cols) < P else None, D=pack(truths), bar=packed))
            kinds["D"] |= {repr(float(v)) for v in truths if not np.isfinite(v)}
            sh = shares(f64_d(ll, lpyl)[cols], truths, bars)
            assert max(sh) <= 1.0, (S, P, scale, kind, max(sh))
            worst["D"] = max(worst["D"], max(sh))
            for wrong in ("no_minus_n", "neighbour"):
                moved[wrong] = max(moved[wrong], max(shares(f64_d(ll, lpyl, wrong)[cols], truths, bars)))
        print(f"shape {S} x {P} done", flush=True)
    for wrong, by in moved.items():
        assert by >= 1000.0, f"the wrong implementation '{wrong}' moves no case by 1000 bars (at most {by:.3g})"
    assert kinds == {"lpyl": {"nan", "-inf"}, "D": {"nan", "inf"}}, kinds
    print("sequential float64, worst share of a bar: lpyl %.3f, D %.3f" % (worst["lpyl"], worst["D"]))
    doc = dict(about="tests/golden/gen_mixture_math.py; lpyl / D: base64 of little-endian float64, bar: of float32 (NaN: the "
                     "truth is not finite and is matched in kind and sign)", mixture=mixture, dfunction=dfunction)
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
