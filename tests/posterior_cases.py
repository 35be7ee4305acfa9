"""What tests/test_posterior_math.py and tests/test_gpu_posterior.py share: the cases of tests/golden/posterior_math.json
with their inputs restated (the file stores none: tests/golden/gen_posterior_math.py), a float64 numpy restatement of the
posterior and of the two summaries of a prediction matrix, and the comparison against truths and bars.  A plain helper:
no fixture, no plugin."""
import base64
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posterior_math.json")
MODES = ("population", "posterior")
U = 2.0 ** -53
TINY = 2.0 ** -1021  # the absolute part of q's bar: a q below the normal range may be flushed to zero
_doc = None


def _f8(text):
    return np.frombuffer(base64.b64decode(text), dtype="<f8")


def _f4(text):
    return np.frombuffer(base64.b64decode(text), dtype="<f4").astype(np.float64)


def doc():
    """the fixture unpacked: case["q"] [len(subs), len(cols)] and case["q_bar"] (the floor added); case[mode] =
    dict(mean, mean_bar, median), each [len(kept)] (a NaN bar: the truth is not finite and is matched in kind and sign);
    cols / subs / kept as index arrays (stored as null where everything is kept)"""
    global _doc
    if _doc is None:
        with open(GOLDEN) as f:
            _doc = json.load(f)
        for case in _doc["cases"]:
            for key, n in (("cols", case["P"]), ("subs", case["S"]), ("kept", sum(case["rows"]))):
                case[key] = np.arange(n) if case[key] is None else np.asarray(case[key])
            shape = (case["subs"].size, case["cols"].size)
            case["q"] = _f8(case["q"]).reshape(shape)
            case["q_bar"] = _f4(case["q_bar"]).reshape(shape) * np.abs(case["q"]) + TINY  # (stored as a share of q)
            for mode in MODES:
                m = case[mode]
                m["mean"], m["mean_bar"], m["median"] = _f8(m["mean"]), _f4(m["mean_bar"]), _f8(m["median"])
    return _doc


def inputs(rows, P, scale, seed):
    """rows[s]: the observation rows of subject s.  r = (s 2654435761 + p 40503 + seed) mod 1000003;
    ll = -((2.5 scale + 1) + scale r / 1000003); w = (((p 7919 + 31 seed) mod 1009) + 1) / (1009 P);
    lpyl = max_p ll - ((7 s + seed) mod 9) / 4; pred[i][p] = -3 + 20 ((i 2246822519 + p 3266489917 + 7 seed) mod 1000033) / 1000033"""
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


def case_inputs(case):
    """(ll[S, P], w[P], lpyl[S], pred[n_rows, P], obs_off[S + 1]) of a case"""
    ll, w, lpyl, pred = inputs(case["rows"], case["P"], case["scale"], case["seed"])
    apply_edits(case["edits"], ll, w, lpyl, pred)
    return ll, w, lpyl, pred, np.concatenate([[0], np.cumsum(case["rows"])]).astype(np.int64)


def case_id(case):
    return f"{len(case['rows'])}x{case['P']}-{case['scale']:g}-{case['kind']}"


# ---- the float64 restatement -------------------------------------------------------------------------------------------
def np_q(ll, w, lpyl):
    """q[s, p] = w[p] exp(ll[s, p] - lpyl[s]) where w[p] > 0 (0 where ll is -inf), else 0; NaN everywhere for a negative
    or NaN weight"""
    with np.errstate(all="ignore"):
        if not (w >= 0.0).all():
            return np.full(ll.shape, np.nan)
        q = np.where(ll == -np.inf, 0.0, w[None, :] * np.exp(ll - lpyl[:, None]))
        return np.where(w[None, :] > 0.0, q, 0.0)


def row_q(mode, ll, w, lpyl, obs_off):
    """the weights of every prediction row, [n_rows, P]: w itself, or the posterior of the row's subject"""
    n_rows = int(obs_off[-1])
    if mode == "population":
        q = np.where(w > 0.0, w, 0.0) if (w >= 0.0).all() else np.full(w.shape, np.nan)
        return np.broadcast_to(q, (n_rows, w.size))
    return np.repeat(np_q(ll, w, lpyl), np.diff(obs_off), axis=0)


def np_summary(pred, q):
    """(mean, median) per row of pred under the row weights q [n_rows, P]: sum q pred / sum q over the columns with
    q > 0, and the lower weighted median - the smallest value whose cumulative weight reaches half the total"""
    n_rows = pred.shape[0]
    mean, median = np.full(n_rows, np.nan), np.full(n_rows, np.nan)
    with np.errstate(all="ignore"):
        for i in range(n_rows):
            qi = q[i]
            keep = qi > 0.0
            if np.isnan(qi).any() or not keep.any():
                continue
            v, qk = pred[i, keep], qi[keep]
            total = qk.sum()
            mean[i] = (qk * v).sum() / total
            if np.isnan(v).any():
                continue
            order = np.argsort(v, kind="stable")
            cum = np.cumsum(qk[order])
            median[i] = v[order][min(int(np.searchsorted(cum, 0.5 * total, side="left")), v.size - 1)]
    return mean, median


def np_median_gap(pred, q):
    """the smallest distance, as a share of the total weight, between half the total and the cumulative weights on
    either side of a row's median (rows without one do not count): above some 1e-9 no summation order moves a median"""
    gap = np.inf
    with np.errstate(all="ignore"):
        for i in range(pred.shape[0]):
            keep = q[i] > 0.0
            if np.isnan(q[i]).any() or not keep.any() or np.isnan(pred[i, keep]).any():
                continue
            v, qk = pred[i, keep], q[i, keep]
            order = np.argsort(v, kind="stable")
            v, cum = v[order], np.cumsum(qk[order])
            total = cum[-1]
            k = min(int(np.searchsorted(cum, 0.5 * total, side="left")), v.size - 1)
            first, last = int(np.searchsorted(v, v[k], side="left")), int(np.searchsorted(v, v[k], side="right")) - 1
            below = cum[first - 1] if first > 0 else 0.0
            gap = min(gap, (0.5 * total - below) / total, (cum[last] - 0.5 * total) / total)
    return gap


def np_bar_q(ll, w, lpyl):
    """the fixture's bar for q, from float64 values"""
    with np.errstate(all="ignore"):
        x = ll - lpyl[:, None]
        return 4 * U * np_q(ll, w, lpyl) * (np.where(np.isfinite(x), np.abs(x), 0.0) + 3) + TINY


def np_bar_mean(pred, q, x):
    """the fixture's bar for the mean, from float64 values; x [n_rows, P]: the exponents ll - lpyl behind q (0 in
    population mode)"""
    with np.errstate(all="ignore"):
        P = pred.shape[1]
        keep = q > 0.0
        qk = np.where(keep, q, 0.0)
        ax = np.where(keep & np.isfinite(x), np.abs(x), 0.0)
        av = np.where(keep, np.abs(pred), 0.0)
        total = qk.sum(axis=1)
        mean = np.where(keep, q * pred, 0.0).sum(axis=1) / total
        return 4 * U * ((qk * av * (ax + 3 + P)).sum(axis=1) / total + np.abs(mean) * ((qk * (ax + 3)).sum(axis=1) / total + P))


def row_x(mode, ll, lpyl, obs_off):
    n_rows = int(obs_off[-1])
    if mode == "population":
        return np.zeros((n_rows, ll.shape[1]))
    with np.errstate(all="ignore"):
        return np.repeat(ll - lpyl[:, None], np.diff(obs_off), axis=0)


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def assert_within(got, truth, bar, what, bars=1.0):
    """finite truths within `bars` bars, non-finite ones equal in kind and sign; returns the worst share of a bar"""
    got, truth, bar = (np.asarray(a, dtype=np.float64).ravel() for a in (got, truth, bar))
    assert got.shape == truth.shape == bar.shape, (what, got.shape, truth.shape, bar.shape)
    worst = 0.0
    for i, (g, t, b) in enumerate(zip(got, truth, bar)):
        if np.isnan(b) or not np.isfinite(t):
            assert (np.isnan(g) and np.isnan(t)) or g == t, f"{what}[{i}]: got {g}, truth {t}"
        else:
            assert np.isfinite(g) and abs(g - t) <= bars * b, f"{what}[{i}]: got {g!r}, truth {t!r}, off by {abs(g - t) / b:.3g} bars"
            worst = max(worst, abs(g - t) / b)
    return worst


def assert_same_values(got, truth, what):
    """medians: the truth's selected element itself (NaN where the truth is NaN; -0.0 == +0.0)"""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    same = (got == truth) | (np.isnan(got) & np.isnan(truth))
    assert same.all(), f"{what}: rows {np.flatnonzero(~same)[:8].tolist()} got {got[~same][:8]}, truth {truth[~same][:8]}"


def assert_q(got, case, ll, w, lpyl):
    """q [S, P] against a case: the stored entries within their bar, every other entry within 2 float64 bars of the
    restatement (both sides within one bar of the truth; the stored entries hold the restatement to that)"""
    got = np.asarray(got, dtype=np.float64)
    stored = np.zeros(got.shape, dtype=bool)
    stored[np.ix_(case["subs"], case["cols"])] = True
    worst = assert_within(got[stored], case["q"], case["q_bar"], "q")
    if not stored.all():
        want = np_q(ll, w, lpyl)[~stored]
        assert_within(got[~stored], want, np.where(np.isfinite(want), np_bar_q(ll, w, lpyl)[~stored], np.nan), "q (restated)", bars=2.0)
    return worst


def assert_summary(mean, median, case, mode, pred, rq, x):
    """(mean, median) [n_rows] against a case in `mode`: the stored rows within their bar resp. equal; every other row
    within 2 float64 bars of the restatement resp. equal to its median (the generator checked the median's margin for
    every row).  rq, x: row_q and row_x of the case.  Returns the worst share of a stored bar."""
    mean, median = np.asarray(mean, dtype=np.float64), np.asarray(median, dtype=np.float64)
    kept, truth = case["kept"], case[mode]
    worst = assert_within(mean[kept], truth["mean"], truth["mean_bar"], f"{mode} mean")
    assert_same_values(median[kept], truth["median"], f"{mode} median")
    rest = np.setdiff1d(np.arange(mean.size), kept)
    if rest.size:
        want_mean, want_median = np_summary(pred[rest], rq[rest])
        bar = np.where(np.isfinite(want_mean), np_bar_mean(pred[rest], rq[rest], x[rest]), np.nan)
        assert_within(mean[rest], want_mean, bar, f"{mode} mean (restated)", bars=2.0)
        assert_same_values(median[rest], want_median, f"{mode} median (restated)")
    return worst
