#!/usr/bin/env python3
"""Generate tests/golden/exposure_math.json: the exposure metrics of predicted concentration profiles - AUC, AUMC, Cmax,
Tmax, Cmin and the time above a threshold, over a window - as exact mathematics (mpmath, 40 digits) of the formulas of
include/pmx.h, evaluated on the float64 inputs.  Neither the oracle nor the product is imported.

A profile's points are (t_i, c_i); the window is [a, b].  The clipped profile K holds the points with a <= t_i <= b, with
(a, lerp(a)) in front when t_{i-1} < a < t_i and (b, lerp(b)) behind when b does likewise; lerp(x) = v1 + (v2 - v1) (x - t1) /
(t2 - t1), v1 where |t2 - t1| < 1e-10.  AUC and AUMC sum the reference's segment formulas over the consecutive pairs of K
(linear: (c1 + c2) / 2 dt and (t1 c1 + t2 c2) / 2 dt; log: (c1 - c2) dt / ln(c1 / c2) and, with k = ln(c1 / c2) / dt,
(t1 c1 - t2 c2) / k + (c1 - c2) / k^2; log where use_log_linear(c1, c2) = c2 < c1, both positive, |c1 / c2 - 1| >= 1e-10 says
so - for lin-log only in pairs that end after tmax, the time of the first-occurrence maximum of the UNCLIPPED profile);
the time above adds dt, or the part of dt on the upper side of the linear crossing, by the `>=` rule; Cmax / Tmax / Cmin
are first-occurrence folds over K.  A NaN anywhere in the profile: everything NaN; a zero-length pair in K: AUC and AUMC
NaN; fewer than two points in K: AUC, AUMC and the time above NaN; none: everything NaN.  The constants 1e-10 are the
float64 numbers the product compares with; every comparison is made exactly, on the float64 inputs.

Inputs are not stored: they come from integer arithmetic that the tests restate (`inputs`, `apply_edits` below,
tests/exposure_cases.py), in float64 operations that every IEEE machine rounds alike.  The file holds seeds, shapes,
the names of method and window, the edits, a checksum of the inputs, and per metric the truths of a few columns - the
first, the middle, the last, column 64 - rounded to float64, each with its bar (float32).

THE BARS ARE DERIVED, not tuned; u = 2^-53.  They are computed in float64 by tests/exposure_cases.np_profile, the same
function the tests hold the unstored columns to, and this generator refuses to write a file in which the float64
restatement misses a truth by more than one bar.
  * A data point is exact.  A cut value ce = cp + (c - cp) (x - tp) / (t - tp) carries d = 2 u |ce| + 6 u |c - cp| (a rounding
    in each difference, the product, the quotient, the sum: five of at most |c - cp| u each and one of |ce| u, each with a
    spare), and d = 0 where c == cp: the product is an exact zero.  This is the conditioning of the lerp quotient.
  * A linear piece: (d1 + d2) dt / 2 from its ends, + 4 u (|c1| + |c2|) / 2 dt for the sum, the halving (exact), dt and the
    product; AUMC alike with |t1| d1 + |t2| d2 and 5 u (one product more).
  * A log piece (c1 - c2) dt / ln(c1 / c2): with rho = d1 / c1 + d2 / c2 + 2 u the relative error of the ratio, the
    logarithm is off by rho absolutely, rho / |ln| relatively - this is the conditioning of the log pieces: about
    u / |ln(c1 / c2)|, 1e-6 at the ratio 1 + 1e-10 where use_log_linear starts to say yes - and by the device's log,
    which is not correctly rounded: 4 u allows it two ulps.  With the numerator's (d1 + d2) / |c1 - c2| + 2 u and the
    quotient's rounding the piece is held to (d1 + d2) / |c1 - c2| + rho / |ln| + 8 u of its size.
  * The AUMC log piece A / k + B / k^2: k = ln / dt relative ek = rho / |ln| + 6 u; A = t1 c1 - t2 c2 absolute dA = |t1| d1 +
    |t2| d2 + 3 u (|t1 c1| + |t2 c2|); so dA / |k| + |A / k| (ek + 2 u) + |B / k^2| ((d1 + d2) / |B| + 2 ek + 4 u) + 2 u of the piece:
    the same conditioning with k k.
  * A crossing t1 + dt (c1 - thr) / (c1 - c2): the quotient g is off by (d1 + u |num|) / |den| + g ((d1 + d2) / |den| + 2 u); the
    piece by dt times that, + 3 u dt g, + u |t_cross| (the sum with t1 rounds at the size of the absolute time: the
    conditioning of the crossing) + u of the piece.  A pair on one side of the threshold adds dt (u dt) or nothing.
  * Every running sum adds u |sum| per addition.
Cmax, Cmin and Tmax are selections and are compared for equality (bar 0); an extreme attained at a window cut is
compared within that cut's d, its time for equality.  MARGINS: the generator refuses a case in which rounding could
change a decision - the selected extreme must be apart from every other point of K by more than the two bars (two data
points compare exactly: ties keep their first occurrence on both sides), and no `>=` test may sit within bars of a flip:
the threshold against every cut value (a data point equal to the threshold compares exactly and is wanted: THRESHOLD is
the plateau of the rise-and-fall profile), c2 < c1 and the positivity of cut values, |c1 / c2 - 1| against 1e-10 by more
than 2 rho.  (A PTA target is compared with a metric plane that is an input of the attainment: exactly.)

Usage: python3 tests/golden/gen_exposure_math.py   (needs mpmath; takes a few seconds)
"""
import base64
import json
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import exposure_cases as ec  # noqa: E402  (the layout, the bars and the margins; the inputs are restated below)

mp.mp.dps = 40
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "exposure_math.json")
E10 = mp.mpf(1e-10)  # the float64 number
PS = (1, 2, 63, 64, 65, 130, 1000)
FULL = [(m, w) for w in ("whole", "cuts") for m in ec.METHODS] + [
    ("lin_up_log_down", "inside"), ("lin_log", "points"), ("linear", "miss"), ("lin_log", "one"), ("lin_up_log_down", "before"),
    ("lin_log", "late")]
FEW = [("linear", "cuts"), ("lin_up_log_down", "whole"), ("lin_log", "cuts"), ("lin_log", "points")]


def inputs(P, seed):
    n = ec.n_rows()
    pred = np.empty((n, P))
    special = {int(r): k for k, r in enumerate(ec.special_rows())}
    for i in range(n):
        for p in range(P):
            if i in special:
                pred[i, p] = ec.SPECIAL_C[special[i]] * (1.0 + float(p % 7) / 8.0)
            else:
                pred[i, p] = 0.5 + 20.0 * (float((i * 2246822519 + p * 3266489917 + seed * 7) % 1000033) / 1000033.0)
    return pred


def edits_of(P, method, window):
    """a NaN cell in the middle column (row 3: subject 0, outeq 0) and a failed pair of subject 1 in the last one"""
    if not ((method == "lin_log" and window == "cuts") or (method == "linear" and window == "whole")):
        return []
    return [{"cell": [3, P // 2]}] + ([{"pair": [1, P - 1]}] if P > 1 else [])


def use_log(c1, c2):
    return c2 < c1 and c1 > 0 and c2 > 0 and abs(c1 / c2 - 1) >= E10


def mp_profile(times, c, a, b, method, thr):
    """one column of one profile in 40 digits: dict metric -> mpf, or None for NaN"""
    names = ec.METRICS
    if any(np.isnan(v) for v in c):
        return dict.fromkeys(names)
    t = [mp.mpf(float(x)) for x in times]
    v = [mp.mpf(float(x)) for x in c]
    K = []
    for i in range(len(t)):
        for x in (a, b):
            if i > 0 and t[i - 1] < x < t[i]:
                x = mp.mpf(x)
                K.append((x, v[i - 1] if abs(t[i] - t[i - 1]) < E10 else v[i - 1] + (v[i] - v[i - 1]) * (x - t[i - 1]) / (t[i] - t[i - 1])))
        if a <= t[i] <= b:
            K.append((t[i], v[i]))
    if not K:
        return dict.fromkeys(names)
    out = {}
    imax = max(range(len(K)), key=lambda j: (K[j][1], -j))
    imin = min(range(len(K)), key=lambda j: (K[j][1], j))
    out["cmax"], out["tmax"], out["cmin"] = K[imax][1], K[imax][0], K[imin][1]
    if len(K) < 2:
        out["auc"] = out["aumc"] = out["time_above"] = None
        return out
    tmax_all = t[max(range(len(v)), key=lambda j: (v[j], -j))]
    auc = aumc = above = mp.mpf(0)
    thr = mp.mpf(thr)
    zero_len = False
    for (t1, c1), (t2, c2) in zip(K[:-1], K[1:]):
        dt = t2 - t1
        if dt <= 0:
            zero_len = True
        else:
            log = method != "linear" and use_log(c1, c2) and (method != "lin_log" or t2 > tmax_all)
            if log:
                k = mp.log(c1 / c2) / dt
                auc += (c1 - c2) / k
                aumc += (t1 * c1 - t2 * c2) / k + (c1 - c2) / (k * k)
            else:
                auc += (c1 + c2) / 2 * dt
                aumc += (t1 * c1 + t2 * c2) / 2 * dt
        if c1 >= thr and c2 >= thr:
            above += dt
        elif c1 >= thr and c2 < thr:
            above += dt * (c1 - thr) / (c1 - c2)
        elif c1 < thr and c2 >= thr:
            above += dt - dt * (thr - c1) / (c2 - c1)
    out["auc"], out["aumc"], out["time_above"] = (None if zero_len else auc), (None if zero_len else aumc), above
    return out


def b64(a, dtype):
    return base64.b64encode(np.ascontiguousarray(a, dtype=dtype).tobytes()).decode()


def main():
    table = ec.profile_table()
    cases, worst = [], 0.0
    for P in PS:
        for k, (method, window) in enumerate(FULL if P in (64, 1000) else FEW):
            seed = 100 * P + k
            edits = edits_of(P, method, window)
            pred = inputs(P, seed)
            assert np.array_equal(pred, ec.inputs(P, seed))
            ec.apply_edits(edits, pred)
            a, b = ec.WINDOWS[window]
            cols = sorted({0, P // 2, P - 1, min(64, P - 1)})
            got, ok = ec.np_exposure(pred, a, b, method, ec.THRESHOLD, table)
            assert ok.all(), (P, method, window, "a decision within bars of a flip", np.argwhere(~ok)[:4])
            case = dict(P=P, seed=seed, method=method, window=window, edits=edits, cols=cols, checksum=ec.checksum(pred))
            truth = {m: np.full((len(table), len(cols)), np.nan) for m in ec.METRICS}
            for ip, prof in enumerate(table):
                for ic, p in enumerate(cols):
                    res = mp_profile(prof["times"], pred[prof["rows"], p], a, b, method, ec.THRESHOLD)
                    for m in ec.METRICS:
                        val, bar = got[m][0][ip, p], got[m][1][ip, p]
                        if res[m] is None:
                            assert np.isnan(val), (P, method, window, ip, p, m, val)
                            continue
                        truth[m][ip, ic] = float(res[m])
                        off = abs(mp.mpf(float(val)) - res[m])
                        if bar == 0.0:
                            assert off == 0, (P, method, window, ip, p, m, val, res[m])
                        else:
                            assert off <= bar, (P, method, window, ip, p, m, val, res[m], float(off / bar))
                            worst = max(worst, float(off / mp.mpf(bar)))
            for m in ec.METRICS:
                bar32 = got[m][1][:, cols].astype(np.float32)
                assert (bar32[got[m][1][:, cols] > 0.0] > 0.0).all()
                case[m] = dict(value=b64(truth[m], "<f8"), bar=b64(bar32, "<f4"))
            cases.append(case)
    doc = dict(about="tests/golden/gen_exposure_math.py", dps=mp.mp.dps, threshold=ec.THRESHOLD, cases=cases)
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"{len(cases)} cases, {os.path.getsize(OUT)} bytes; the float64 restatement's worst share of a bar: {worst:.3f}")


if __name__ == "__main__":
    main()
