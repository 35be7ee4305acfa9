"""What tests/test_exposure_math.py and tests/test_gpu_exposure.py share: the population and the cases of
tests/golden/exposure_math.json with their inputs restated (the file stores none: tests/golden/gen_exposure_math.py), a
float64 numpy restatement of the exposure metrics (include/pmx.h, "What a simulation takes of the matrix") with the
derived bar of every value beside it, the attainment over the support points, and the comparisons.  A plain helper: no
fixture, no plugin."""
import base64
import hashlib
import json
import os

import numpy as np

from tests import posterior_cases as pc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exposure_math.json")
U = 2.0 ** -53
TINY = 2.0 ** -1021
METRICS = ("auc", "aumc", "cmax", "tmax", "cmin", "time_above")  # plane (bit) order
SUMS = ("auc", "aumc", "time_above")
METHODS = ("linear", "lin_up_log_down", "lin_log")  # AUCMethod's order
INF = float("inf")
WINDOWS = {"whole": (-INF, INF), "cuts": (2.25, 10.5), "inside": (12.5, 15.5), "points": (1.0, 8.0), "miss": (100.0, 200.0),
           "one": (24.0, 30.0), "before": (-5.0, -1.0), "late": (4.0, 20.0)}
THRESHOLD = 9.0  # the plateau of the rise-and-fall profile in the columns of scale 1: a threshold equal to a data value
# the rise-and-fall profile: zeros before the dose, a plateau, a ratio on each side of 1e-10 (2e-10: log; 0.5e-10: linear)
SPECIAL_T = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0, 16.0, 24.0)
_C6 = 7.0 / (1.0 + 2e-10)
SPECIAL_C = (0.0, 0.0, 4.0, 9.0, 9.0, 7.0, _C6, _C6 / (1.0 + 0.5e-10), 3.0, 1.5, 0.75, 0.2)
_doc = None


def layout():
    """LAYOUT[subject][occasion] = [(time, outeq), ...] in event order.  Profile lengths 7, 3, 40, 2, 1, 12, 5, 2: subject 0
    has two output equations whose rows interleave, subject 1 two occasions whose clocks restart, subject 2 lacks outeq 1
    and is the rise-and-fall profile, subject 3 has a duplicate time."""
    s0 = [[(0.5, 0), (1.0, 0), (1.0, 1), (2.0, 0), (4.0, 0), (6.0, 1), (8.0, 0), (12.0, 0), (24.0, 0), (24.0, 1)]]
    s1 = [[(0.6 * k, 0) for k in range(40)], [(0.0, 0), (1.5, 1), (3.0, 0)]]
    s2 = [[(t, 0) for t in SPECIAL_T]]
    s3 = [[(1.0, 0), (2.0, 1), (3.0, 0), (3.0, 0), (5.0, 0), (9.0, 0), (10.0, 1)]]
    return [s0, s1, s2, s3]


def profile_table(lay=None):
    """the profiles of a layout, restated: dicts of subject, occasion, outeq, rows (prediction rows, in prediction order)
    and times, ordered by subject, occasion, outeq; only combinations with a row"""
    lay = layout() if lay is None else lay
    out, r = [], 0
    for s, occs in enumerate(lay):
        for o, events in enumerate(occs):
            here = {}
            for t, q in events:
                here.setdefault(q, ([], []))
                here[q][0].append(r)
                here[q][1].append(t)
                r += 1
            for q in sorted(here):
                out.append(dict(subject=s, occasion=o, outeq=q, rows=np.asarray(here[q][0]), times=np.asarray(here[q][1], dtype=np.float64)))
    return out


def n_rows(lay=None):
    return sum(len(ev) for occs in (layout() if lay is None else lay) for ev in occs)


def subject_rows(s, lay=None):
    lay = layout() if lay is None else lay
    first = sum(len(ev) for occs in lay[:s] for ev in occs)
    return np.arange(first, first + sum(len(ev) for ev in lay[s]))


def special_rows():
    return next(p["rows"] for p in profile_table() if p["subject"] == 2)


def inputs(P, seed):
    """pred[i][p] = 0.5 + 20 ((i 2246822519 + p 3266489917 + 7 seed) mod 1000033) / 1000033; the rows of the rise-and-fall
    profile hold SPECIAL_C (1 + (p mod 7) / 8)"""
    i = np.arange(n_rows(), dtype=np.int64)[:, None]
    p = np.arange(P, dtype=np.int64)[None, :]
    r2 = (i * 2246822519 + p * 3266489917 + seed * 7) % 1000033
    pred = 0.5 + 20.0 * (r2.astype(np.float64) / 1000033.0)
    pred[special_rows(), :] = np.asarray(SPECIAL_C)[:, None] * (1.0 + (p % 7).astype(np.float64) / 8.0)
    return pred


def apply_edits(edits, pred):
    for e in edits:
        if "cell" in e:  # a NaN cell
            pred[e["cell"][0], e["cell"][1]] = np.nan
        elif "pair" in e:  # a failed pair: every row of the subject in that column
            pred[subject_rows(e["pair"][0]), e["pair"][1]] = np.nan
        else:
            raise KeyError(str(e))


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:16]


def case_inputs(case):
    pred = inputs(case["P"], case["seed"])
    apply_edits(case["edits"], pred)
    return pred


def case_id(case):
    return f"{case['P']}-{case['method']}-{case['window']}" + ("-edges" if case["edits"] else "")


def _f8(text):
    return np.frombuffer(base64.b64decode(text), dtype="<f8")


def _f4(text):
    return np.frombuffer(base64.b64decode(text), dtype="<f4").astype(np.float64)


def doc():
    """the fixture unpacked: case[metric] = dict(value, bar), each [n_profiles, len(cols)] (a bar of 0: held to equality; a
    NaN value: NaN expected); cols an index array"""
    global _doc
    if _doc is None:
        with open(GOLDEN) as f:
            _doc = json.load(f)
        n = len(profile_table())
        for case in _doc["cases"]:
            case["cols"] = np.asarray(case["cols"])
            for m in METRICS:
                case[m] = dict(value=_f8(case[m]["value"]).reshape(n, -1), bar=_f4(case[m]["bar"]).reshape(n, -1))
    return _doc


# ---- the float64 restatement, columns side by side ----------------------------------------------------------------------
def clip(times, C, a, b):
    """the clipped profile K of times [n], C [n, P]: (Kt [m], Kc [m, P], Kd [m, P]); Kd is the bar of a value - 0 for a data
    point, and for a cut (two roundings in the differences, a product, a quotient, a sum)
    2 u |ce| + 6 u |c - cp|, 0 where c == cp (the product is an exact 0)"""
    Kt, Kc, Kd = [], [], []
    zero = np.zeros(C.shape[1])
    with np.errstate(all="ignore"):
        for i, t in enumerate(times):
            for e in range(3):
                if e < 2:
                    x = (a, b)[e]
                    if not (i > 0 and times[i - 1] < x < t):
                        continue
                    tp, cp, c = times[i - 1], C[i - 1], C[i]
                    if abs(t - tp) < 1e-10:
                        ce, d = cp, zero
                    else:
                        ce = cp + (c - cp) * (x - tp) / (t - tp)
                        d = np.where(c == cp, 0.0, 2 * U * np.abs(ce) + 6 * U * np.abs(c - cp))
                    Kt.append(x), Kc.append(ce), Kd.append(d)
                elif a <= t <= b:
                    Kt.append(t), Kc.append(C[i]), Kd.append(zero)
    P = C.shape[1]
    return np.asarray(Kt, dtype=np.float64), np.asarray(Kc).reshape(len(Kt), P), np.asarray(Kd).reshape(len(Kt), P)


def np_profile(times, C, a, b, method, thr):
    """The six metrics of one profile, every column: dict metric -> (value [P], bar [P]), and "ok" [P]: no comparison the
    arithmetic makes (use_log_linear, the threshold, the extremes) is within bars of a flip.  The bars, u = 2^-53:
      a linear piece (c1 + c2) / 2 dt: (d1 + d2) dt / 2 from the cut values' bars + 4 u of its size in absolute values;
      a log piece (c1 - c2) dt / ln(c1 / c2): relative (d1 + d2) / |c1 - c2| + rho / |ln| + 8 u, rho = d1 / c1 + d2 / c2 + u
        the error of the ratio - the conditioning of the logarithm near ratio 1 - and 4 u of the 8 for a device log that is
        not correctly rounded;
      the AUMC log piece A / k + B / k^2, k = ln / dt: k relative ek = rho / |ln| + 6 u, A = t1 c1 - t2 c2 absolute
        |t1| d1 + |t2| d2 + 3 u (|t1 c1| + |t2 c2|), so dA / k + |A / k| (ek + 2 u) + |B / k^2| ((d1 + d2) / |B| + 2 ek + 4 u)
        + 2 u of the piece;
      a crossing t1 + dt (c1 - thr) / (c1 - c2): the quotient g absolute (d1 + u |c1 - thr|) / |den| + g ((d1 + d2) / |den|
        + 2 u), times dt, + 3 u dt g, + u |t_cross| + u of the piece (the absolute time enters: the conditioning of the
        crossing);
      every running sum: + u |sum| per addition."""
    method = METHODS.index(method) if isinstance(method, str) else method
    times = np.asarray(times, dtype=np.float64)
    P = C.shape[1]
    nan = np.full(P, np.nan)
    Kt, Kc, Kd = clip(times, C, a, b)
    m = len(Kt)
    bad = np.isnan(C).any(axis=0)
    out, ok = {}, np.ones(P, dtype=bool)
    with np.errstate(all="ignore"):
        tmax_all = times[np.argmax(np.where(np.isnan(C), -INF, C), axis=0)]  # first occurrence, the unclipped profile
        auc, aumc, above = np.zeros(P), np.zeros(P), np.zeros(P)
        auc_b, aumc_b, above_b = np.zeros(P), np.zeros(P), np.zeros(P)
        zero_len = False
        for j in range(1, m):
            t1, t2, c1, c2, d1, d2 = Kt[j - 1], Kt[j], Kc[j - 1], Kc[j], Kd[j - 1], Kd[j]
            dt = t2 - t1
            exact = (d1 + d2) == 0.0
            if dt <= 0.0:
                zero_len = True
            else:
                v = (c1 + c2) / 2.0 * dt
                vb = (d1 + d2) * dt / 2 + 4 * U * (np.abs(c1) + np.abs(c2)) / 2 * dt
                w = (t1 * c1 + t2 * c2) / 2.0 * dt
                wb = (abs(t1) * d1 + abs(t2) * d2) * dt / 2 + 5 * U * (np.abs(t1 * c1) + np.abs(t2 * c2)) / 2 * dt
                if method != 0:
                    r = c1 / c2
                    lg = (c2 < c1) & (c1 > 0.0) & (c2 > 0.0) & (np.abs(r - 1.0) >= 1e-10)
                    rho = d1 / np.abs(c1) + d2 / np.abs(c2) + 2 * U
                    # no flip: c2 < c1 decided beyond the bars (or between two data points), the ratio test beyond rho
                    pos = (c1 > 0.0) & (c2 > 0.0)
                    ok &= exact | (np.abs(c1 - c2) > d1 + d2)
                    ok &= ~(pos & (c2 < c1)) | (np.abs(np.abs(r - 1.0) - 1e-10) > 2 * rho * np.abs(r))
                    ok &= (d1 == 0.0) | (np.abs(c1) > d1)
                    ok &= (d2 == 0.0) | (np.abs(c2) > d2)
                    if method == 2:
                        lg = lg & (t2 > tmax_all)
                    L = np.log(np.where(lg, r, 2.0))
                    B = c1 - c2
                    rel = (d1 + d2) / np.abs(B) + rho / np.abs(L) + 8 * U
                    v_log = B * dt / L
                    k = L / dt
                    ek = rho / np.abs(L) + 6 * U
                    A = t1 * c1 - t2 * c2
                    dA = abs(t1) * d1 + abs(t2) * d2 + 3 * U * (np.abs(t1 * c1) + np.abs(t2 * c2))
                    w_log = A / k + B / (k * k)
                    wb_log = dA / np.abs(k) + np.abs(A / k) * (ek + 2 * U) + np.abs(B / (k * k)) * ((d1 + d2) / np.abs(B) + 2 * ek + 4 * U) \
                        + 2 * U * np.abs(w_log)
                    v, vb = np.where(lg, v_log, v), np.where(lg, np.abs(v_log) * rel, vb)
                    w, wb = np.where(lg, w_log, w), np.where(lg, wb_log, wb)
                auc = auc + v
                auc_b = auc_b + vb + U * np.abs(auc)
                aumc = aumc + w
                aumc_b = aumc_b + wb + U * np.abs(aumc)
            # time above: nca/calc.rs:719-737 (a zero-length pair adds 0)
            up1, up2 = c1 >= thr, c2 >= thr
            ok &= ((d1 == 0.0) | (np.abs(c1 - thr) > d1)) & ((d2 == 0.0) | (np.abs(c2 - thr) > d2))
            down, rise = up1 & (c2 < thr), (c1 < thr) & up2
            num = np.where(down, c1 - thr, thr - c1)
            den = np.where(down, c1 - c2, c2 - c1)
            g = num / den
            dn = d1 + U * np.abs(num)
            gb = dn / np.abs(den) + np.abs(g) * ((d1 + d2) / np.abs(den) + 2 * U)
            t_cross = t1 + dt * num / den
            piece = np.where(down, t_cross - t1, t2 - t_cross)
            pb = dt * gb + 3 * U * dt * np.abs(g) + U * np.abs(t_cross) + U * np.abs(piece)
            add = np.where(up1 & up2, dt, np.where(down | rise, piece, 0.0))
            addb = np.where(up1 & up2, U * abs(dt), np.where(down | rise, pb, 0.0))
            above = above + add
            above_b = above_b + addb + U * np.abs(above)
        no_pair = bad | (m < 2)
        out["auc"] = (np.where(no_pair | zero_len, nan, auc), auc_b)
        out["aumc"] = (np.where(no_pair | zero_len, nan, aumc), aumc_b)
        out["time_above"] = (np.where(no_pair, nan, above), above_b)
        if m == 0:
            for name in ("cmax", "tmax", "cmin"):
                out[name] = (nan, np.zeros(P))
            return out, ok | bad
        cols = np.arange(P)
        for name, sign in (("cmax", 1.0), ("cmin", -1.0)):
            sel = np.argmax(sign * Kc, axis=0)  # first occurrence of the extreme, as the `>` / `<` folds find it
            cs, ds = Kc[sel, cols], Kd[sel, cols]
            apart = ((Kd + ds) == 0.0) | (np.abs(Kc - cs) > Kd + ds) | (np.arange(m)[:, None] == sel[None, :])
            ok &= apart.all(axis=0)
            out[name] = (np.where(bad, nan, cs), ds)
            if name == "cmax":
                out["tmax"] = (np.where(bad, nan, Kt[sel]), np.zeros(P))
    return out, ok | bad  # (a NaN anywhere: every metric is NaN, nothing is compared)


def np_exposure(pred, a, b, method, thr, table=None):
    """every profile: dict metric -> (value [n_profiles, P], bar [n_profiles, P]), and ok [n_profiles, P]"""
    table = profile_table() if table is None else table
    res = [np_profile(p["times"], pred[p["rows"]], a, b, method, thr) for p in table]
    out = {m: (np.stack([r[0][m][0] for r in res]), np.stack([r[0][m][1] for r in res])) for m in METRICS}
    return out, np.stack([r[1] for r in res])


def case_exposure(case, pred=None):
    a, b = WINDOWS[case["window"]]
    return np_exposure(case_inputs(case) if pred is None else pred, a, b, case["method"], THRESHOLD)


# ---- attainment -------------------------------------------------------------------------------------------------------
def weights(P):
    return ((np.arange(P) * 7919) % 1009 + 1.0) / (1009.0 * P)


def np_attainment(plane, q, target):
    """(pta, mean) per profile of plane [n, P] under the row weights q [n, P]"""
    n = plane.shape[0]
    pta, mean = np.full(n, np.nan), np.full(n, np.nan)
    with np.errstate(all="ignore"):
        for k in range(n):
            keep = q[k] > 0.0
            if np.isnan(q[k]).any() or not keep.any() or np.isnan(plane[k, keep]).any():
                continue
            v, qk = plane[k, keep], q[k, keep]
            total = qk.sum()
            pta[k] = qk[v >= target[k]].sum() / total
            mean[k] = (qk * v).sum() / total
    return pta, mean


def np_bar_pta(q, x):
    """the bar of a pta: two sums of up to P non-negative terms and a quotient, 2 P u; in posterior mode the weights carry
    the relative error 4 u (|x| + 3) of q (tests/posterior_cases.np_bar_q), twice their weighted mean"""
    with np.errstate(all="ignore"):
        P = q.shape[1]
        keep = q > 0.0
        qk = np.where(keep, q, 0.0)
        ax = np.where(keep & np.isfinite(x), np.abs(x), 0.0)
        eq = np.where(x == 0.0, 0.0, 4 * U * (ax + 3))
        return 2 * U * (P + 2) + 2 * (qk * eq).sum(axis=1) / qk.sum(axis=1)


def profile_q(mode, ll, w, lpyl, table=None):
    """(q, x) [n_profiles, P]: the weights of every profile and the exponents behind them"""
    table = profile_table() if table is None else table
    subj = np.asarray([p["subject"] for p in table])
    if mode == "population":
        q = np.where(w > 0.0, w, 0.0) if (w >= 0.0).all() else np.full(w.shape, np.nan)
        return np.broadcast_to(q, (len(table), w.size)).copy(), np.zeros((len(table), w.size))
    with np.errstate(all="ignore"):
        return pc.np_q(ll, w, lpyl)[subj], (ll - lpyl[:, None])[subj]


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def assert_values(got, want, bar, what, bars=1.0):
    """NaN where NaN is wanted; equal where the bar is 0 (selections; -0.0 == +0.0); else within `bars` bars.  Returns the
    worst share of a bar."""
    got, want, bar = (np.asarray(x, dtype=np.float64) for x in (got, want, bar))
    assert got.shape == want.shape == bar.shape, (what, got.shape, want.shape, bar.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN at {np.argwhere(np.isnan(got) != nan)[:6].tolist()}"
    with np.errstate(all="ignore"):
        off = np.where(nan, 0.0, np.abs(got - want))
        fine = nan | np.where(bar == 0.0, got == want, off <= bars * bar)
        assert fine.all(), (f"{what}: at {np.argwhere(~fine)[:6].tolist()} got {got[~fine][:6]}, want {want[~fine][:6]}, "
                            f"bars {(off[~fine] / bar[~fine])[:6]}")
        share = np.where(nan | (bar == 0.0), 0.0, off / bar)
    return float(share.max()) if share.size else 0.0


def assert_planes(got, case, pred=None):
    """got: dict metric -> [n_profiles, P].  The stored columns within one stored bar (selections equal), every other
    column within two float64 bars of the restatement (both sides within one of the truth; the stored columns hold the
    restatement to that).  Returns the worst share of a stored bar."""
    want, ok = case_exposure(case, pred)
    assert ok.all(), "a comparison within bars of a flip"
    cols = case["cols"]
    rest = np.setdiff1d(np.arange(case["P"]), cols)
    worst = 0.0
    for m in METRICS:
        g = np.asarray(got[m], dtype=np.float64)
        worst = max(worst, assert_values(g[:, cols], case[m]["value"], case[m]["bar"], f"{m}"))
        if rest.size:
            assert_values(g[:, rest], want[m][0][:, rest], want[m][1][:, rest], f"{m} (restated)", bars=2.0)
    return worst
