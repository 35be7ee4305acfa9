"""What tests/test_mixture_math.py and tests/test_gpu_mixture.py share: the cases of tests/golden/mixture_math.json with
their inputs restated (the file stores none: tests/golden/gen_mixture_math.py), a float64 numpy restatement of the two
reductions, and the comparison against truths and bars.  A plain helper: no fixture, no plugin."""
import base64
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixture_math.json")
_doc = None


def doc():
    """the fixture, truths and bars unpacked: case["lpyl"] / case["D"] float64 arrays, case["bar"] likewise (NaN: the
    truth is not finite)"""
    global _doc
    if _doc is None:
        with open(GOLDEN) as f:
            _doc = json.load(f)
        for case in _doc["mixture"] + _doc["dfunction"]:
            key = "lpyl" if "lpyl" in case else "D"
            case[key] = np.frombuffer(base64.b64decode(case[key]), dtype="<f8")
            case["bar"] = np.frombuffer(base64.b64decode(case["bar"]), dtype="<f4").astype(np.float64)
    return _doc


def inputs(S, P, scale, seed):
    """r = (s 2654435761 + p 40503 + seed) mod 1000003; ll = -((2.5 scale + 1) + scale r / 1000003);
    w = (((p 7919 + 31 seed) mod 1009) + 1) / (1009 P); D's input lpyl = max_p ll - ((7 s + seed) mod 9) / 4"""
    s = np.arange(S, dtype=np.int64)[:, None]
    p = np.arange(P, dtype=np.int64)[None, :]
    r = (s * 2654435761 + p * 40503 + seed) % 1000003
    ll = -((2.5 * scale + 1.0) + scale * (r.astype(np.float64) / 1000003.0))
    w = (((p[0] * 7919 + seed * 31) % 1009) + 1).astype(np.float64) / (1009.0 * P)
    lpyl = ll.max(axis=1) - 0.25 * ((s[:, 0] * 7 + seed) % 9).astype(np.float64)
    return ll, w, lpyl


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


def mixture_inputs(case):
    """(ll[S, P], w[P]) of a mixture case"""
    ll, w, _ = inputs(case["S"], case["P"], case["scale"], case["seed"])
    apply_edits(case["edits"], ll, w)
    return ll, w


def dfunction_inputs(case):
    """(ll[S, P], lpyl[S]) of a D case"""
    ll, w, lpyl = inputs(case["S"], case["P"], case["scale"], case["seed"])
    apply_edits(case["edits"], ll, w, lpyl)
    return ll, lpyl


def np_lpyl(ll, w):
    """ln sum_{p: w > 0} w exp(ll) per row, shifted by the row's largest weighted entry"""
    with np.errstate(all="ignore"):
        x = ll[:, w > 0.0]
        m = np.max(np.where(np.isnan(x), -np.inf, x), axis=1, initial=-np.inf)
        m = np.where(np.isfinite(m), m, 0.0)
        return m + np.log(np.sum(w[w > 0.0] * np.exp(x - m[:, None]), axis=1))


def np_d(ll, lpyl):
    """sum_s exp(ll - lpyl) - S per column"""
    with np.errstate(all="ignore"):
        return np.sum(np.exp(ll - lpyl[:, None]), axis=0) - ll.shape[0]


def assert_within(got, truth, bar, what, bars=1.0):
    """finite truths within `bars` bars, non-finite ones equal in kind and sign; returns the worst share of a bar"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    worst = 0.0
    for i, (g, t, b) in enumerate(zip(got, truth, bar)):
        if np.isnan(b):
            assert (np.isnan(g) and np.isnan(t)) or g == t, f"{what}[{i}]: got {g}, truth {t}"
        else:
            assert np.isfinite(g) and abs(g - t) <= bars * b, f"{what}[{i}]: got {g!r}, truth {t!r}, off by {abs(g - t) / b:.3g} bars"
            worst = max(worst, abs(g - t) / b)
    return worst


def assert_case(got, case, restated, bar64):
    """`got` against a case: the entries whose truth the fixture stores (case["rows"] / case["cols"]; None: all) within
    their bar; every other entry within 2 float64 bars of the restatement (both sides within one bar of the truth; the
    stored entries of the same case hold the restatement to that).  Returns the worst share of a stored bar."""
    key = "lpyl" if "lpyl" in case else "D"
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == restated.shape
    idx = case["rows" if key == "lpyl" else "cols"]
    idx = np.arange(got.size) if idx is None else np.asarray(idx)
    worst = assert_within(got[idx], case[key], case["bar"], key)
    rest = np.setdiff1d(np.arange(got.size), idx)
    assert_within(got[rest], restated[rest], np.where(np.isfinite(restated[rest]), bar64[rest], np.nan), key + " (restated)", bars=2.0)
    return worst


def case_id(case):
    return f"{case['S']}x{case['P']}-{case['scale']:g}-{case['kind']}"


U = 2.0 ** -53


def np_bar_lpyl(ll, w):
    """the fixture's bar for lpyl, from float64 values (rows with a finite result only; elsewhere NaN)"""
    with np.errstate(all="ignore"):
        keep = w > 0.0
        x = ll[:, keep]
        m = np.max(np.where(np.isnan(x), -np.inf, x), axis=1, initial=-np.inf)
        x = x - np.where(np.isfinite(m), m, 0.0)[:, None]
        t = w[keep] * np.exp(x)
        sigma = t.sum(axis=1)
        truth = m + np.log(sigma)
        ax = np.where(np.isfinite(x), np.abs(x), 0.0)
        return 4 * U * ((t * (ax + 3)).sum(axis=1) / sigma + (ll.shape[1] - 1) + 2 * np.abs(np.log(sigma)) + np.abs(truth) + 2)


def np_bar_d(ll, lpyl):
    """the fixture's bar for D, from float64 values"""
    with np.errstate(all="ignore"):
        x = ll - lpyl[:, None]
        e = np.exp(x)
        S, T = ll.shape[0], e.sum(axis=0)
        return 4 * U * ((e * (np.where(np.isfinite(x), np.abs(x), 0.0) + 2)).sum(axis=0) + S * T + T + S)
