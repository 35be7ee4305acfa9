#!/usr/bin/env python3
"""Generate tests/golden/user_closures.json: what the closure walkers (Analytical.user, ODE.user) must return, from an
event march that shares no code with the oracle or the device walkers.

Same method as gen_edge.py / gen_ode_exact.py: mpmath at 40 digits, neither `oracle` nor `pharmsol_amd` imported; the
closures are the Python twins of tests/user_closure_models.py.  The event rules are restated from the reference:

  lag       fn_lag(theta, bolus.time(), cov) at the RECORDED time; `if l != 0.0 { t += l }`; the list is re-sorted only
            when something moved                                                     src/data/structs.rs:611-643
  order     time by total_cmp, then Observation < Bolus < Infusion; the sort is stable, so list order holds among
            equals                                                                   src/data/event.rs:292-304
  fa        fn_fa(theta, bolus.time(), cov) AFTER the shift; multiplies the amount    structs.rs:645-666
  infusions never lagged                                                             structs.rs:622-625
  covariate slope * t + intercept in doubles on [from, to); the first value before the first knot, the last one from
            the last knot on                                                         src/data/covariate.rs:50-65,189-241
  init      at t = 0, occasion index 0 only, every occasion starts from zero        analytical/mod.rs:409-426, ode/mod.rs:536-549
  out       at the observation time                                                 analytical/mod.rs:373-407, ode/mod.rs:692-715
  occasions every occasion rewrites its own list: a bolus lagged past the last event stays in its occasion
                                                                                     equation/mod.rs:247-273
Analytical solve (simulate_event equation/mod.rs:300-358, solve analytical/mod.rs:299-370): the event acts, then
  solve(event.time, next.time): nothing when the two are equal; split at the ends (and starts) of the infusions pushed so
  far that lie strictly inside; times closer than 1e-12 deduplicated; the parameter vector rebuilt from theta per solve
  and kept across its sub-segments; per sub-segment rateiv = sum of amount / duration of the infusions with
  current >= start and next <= end, seq_eq at the absolute end, eq over dt = next - current (a double) with its derive
  at dt (the macro lowering, expand/analytical.rs:254,286) or at the absolute end (`segment_end_abs`).  A NaN landing
  time makes `ts.sort_by(partial_cmp().unwrap())` panic (analytical/mod.rs:326): status PMX_PAIR_BAD_LAG, every row NaN.
  The pm_* wrapper drops state / rateiv slot 0 before the structure and pads 0 back after it (analytical/mod.rs:62-90).
ODE (ode/mod.rs:348, 647-686, 719-739): the solver clock starts at occasion.initial_time(), the earliest RECORDED time
  (structs.rs:782-793); every event of the rewritten list is applied at the clock as it stands and the solver advances
  only `while next_event_time > solver.state().t`, stopping at every infusion start and end on the way; a bolus is the
  jump f(x, t, b, 0) - f(x, t, 0, 0) at its landing time; an infusion contributes amount / duration to rateiv[input] on
  [start, end) (ode/closure.rs:43-60).  The project's stepper (DESIGN.md "ODE step partition"): classic RK4 per piece with
  n = max(1, ceil(dt / h_max)), h = dt / n formed in doubles; covariates are read at every stage time.

Formed in Python doubles, because the reference forms them in doubles and they decide an order or a branch: event
times, t + l, infusion ends, rates amount / duration, the covariate line at a double time, the fa clamp.  Everything that
propagates is mpf.  Condition, asserted for every case: each landing time is exact (the double equals the value in exact
arithmetic), and any two times of a rewritten list (infusion ends included) are bit-equal or at least 1e-6 apart.

Truth: the augmented matrix exponential per sub-segment with that sub-segment's rate constants (built-in structures),
the user's formula in mpf (pmx_eq), exact-arithmetic RK4 steps (ODE; `n_steps` and the kappa of gen_ode_exact.py).
Analytical kappa: gen_edge.py's (largest rate over the smallest node gap, over every parameter set met); 1 for pmx_eq.

A group is one model and one schedule; its cases are theta vectors that give the lanes of one wave different landing
orders (>= 4 distinct orders asserted in the groups marked `reorder`), the first of them an easy one without lag.
Self-checks, asserted: for every rule a group names, the deliberately wrong variant of that rule moves at least one of
its cases by >= 1000 bars; a group marked `scalable` doubles its truth when every dose doubles.

Run:  python tests/golden/gen_user_closures.py     (deterministic; rewrites user_closures.json byte for byte)
"""
import json
import math
import os
import sys

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from gen_edge import kappa_of  # noqa: E402  (condition number of the closed forms)
from gen_independent import rate_matrix  # noqa: E402
from gen_ode_exact import RK4, erk_step  # noqa: E402
from user_closure_models import MODELS  # noqa: E402  (the Python twins; no product import)

mp.mp.dps = 40
mpf = mp.mpf
OUT = os.path.join(HERE, "user_closures.json")
U = 2.0 ** -53
RANK = {"obs": 0, "bolus": 1, "inf": 2}
VARIANTS = ("lag_at_landed", "fa_at_recorded", "bolus_before_obs", "unstable_equal_boluses", "params_not_rebuilt",
            "derive_abs_under_dt", "clock_at_first_rewritten", "bolus_as_add", "init_every_occasion")


class BadLag(Exception):
    pass


# ------------------------------------------------------------------------------------------------------- covariates
def segments(knots):
    """Covariate::build_segments (covariate.rs:189-212), in doubles."""
    kn = sorted((float(t), float(v)) for t, v in knots)
    segs = []
    for i, (t0, v0) in enumerate(kn):
        if i + 1 < len(kn):
            t1, v1 = kn[i + 1]
            slope = (v1 - v0) / (t1 - t0)
            segs.append((t0, t1, slope, v0 - slope * t0))
        else:
            segs.append((t0, None, None, v0))
    return kn, segs


def cov_value(knots, t):
    """Covariate::interpolate at a double time (double arithmetic) or at an mpf stage time (mpf arithmetic on the
    double slope and intercept)."""
    kn, segs = segments(knots)
    for t0, t1, slope, icpt in segs:
        if t0 <= t and (t1 is None or t < t1):
            return icpt if slope is None else slope * t + icpt
    return kn[0][1] if t < kn[0][0] else kn[-1][1]


def cov_exact(knots, t):
    """The interpolant in exact arithmetic (for the exactness condition on landing times)."""
    kn = sorted((float(a), float(b)) for a, b in knots)
    if t < kn[0][0]:
        return mpf(kn[0][1])
    for (t0, v0), (t1, v1) in zip(kn[:-1], kn[1:]):
        if t0 <= t < t1:
            return mpf(v0) + (mpf(v1) - mpf(v0)) * (mpf(t) - mpf(t0)) / (mpf(t1) - mpf(t0))
    return mpf(kn[-1][1])


def covs_at(mdl, occ, t):
    return [cov_value(occ["cov"][n], t) for n in mdl["covariates"]]


# ---------------------------------------------------------------------------------------------------- event rewrite
def total_key(t):
    return (t, math.copysign(1.0, t))  # f64::total_cmp on the values that occur here (no NaN reaches the sort)


def rewrite(mdl, occ, theta, V=()):
    """The occasion's rewritten list [(time, kind, amount (mpf for a bolus), duration, input, id)], `id` = position in
    the recorded list.  Raises BadLag on a NaN landing time."""
    rec = sorted(enumerate(occ["events"]), key=lambda ie: (total_key(float(ie[1][1])), RANK[ie[1][0]]))
    rank = dict(RANK, **({"bolus": 0, "obs": 1} if "bolus_before_obs" in V else {}))
    ev, shifted = [], False
    for i, (_, (kind, t, val, dur, io)) in enumerate(rec):
        t, t_rec = float(t), float(t)
        if kind == "bolus" and "lag" in mdl:
            l = mdl["lag"](t, theta, covs_at(mdl, occ, t))[int(io)]
            if "lag_at_landed" in V and l == l:
                l = mdl["lag"](t + l, theta, covs_at(mdl, occ, t + l))[int(io)]
            if l != 0.0:
                exact = mpf(t) + mdl["lag"](mpf(t), [mpf(v) for v in theta], [cov_exact(occ["cov"][n], t) for n in mdl["covariates"]])[int(io)] \
                    if l == l else None
                t = t + l
                shifted = True
                if t != t:
                    raise BadLag()
                assert "lag_at_landed" in V or mpf(t) == exact, ("landing time not exact", theta, t_rec, t)
        ev.append([t, kind, val, float(dur), int(io), i, t_rec])
    if shifted or V:
        flip = -1 if "unstable_equal_boluses" in V else 1
        ev.sort(key=lambda e: (total_key(e[0]), rank[e[1]], flip * e[5] if e[1] == "bolus" else 0))
    out = []
    for t, kind, val, dur, io, i, t_rec in ev:
        if kind == "bolus":
            val = mpf(float(val))
            if "fa" in mdl:
                tf = t_rec if "fa_at_recorded" in V else t
                val = val * mdl["fa"](tf, theta, covs_at(mdl, occ, tf))[io]
        out.append((t, kind, val, dur, io, i))
    return out


def check_separation(ev):
    ts = sorted({e[0] for e in ev} | {e[0] + e[3] for e in ev if e[1] == "inf"})
    for a, b in zip(ts[:-1], ts[1:]):
        assert b - a >= 1e-6, ("times closer than 1e-6", a, b)


# ------------------------------------------------------------------------------------------------- analytical march
def expm_step(structure, k, x, rate_central, dt):
    A, central = rate_matrix(structure, k)
    n = len(A)
    Mx = mp.matrix(n + 1, n + 1)
    for i in range(n):
        for j in range(n):
            Mx[i, j] = A[i][j]
    Mx[central, n] = rate_central
    xb = mp.expm(Mx * dt) * mp.matrix(list(x) + [1])
    return [xb[i] for i in range(n)]


def march_analytical(mdl, group, theta, V=(), dose=1.0):
    """-> (predictions, kappa, order of every occasion's rewritten list)."""
    structure = (mdl["eq"] or "")[3:] if mdl.get("pm") else mdl["eq"]
    pm = 1 if mdl.get("pm") else 0
    abs_time = (mdl.get("cov_time") == "segment_end_abs") != ("derive_abs_under_dt" in V and mdl.get("cov_time") == "segment_dt")
    p_theta = [mpf(v) for v in theta]
    preds, orders, kap = [], [], mpf(1)
    pw = None
    for o, occ in enumerate(group["occasions"]):
        ev = rewrite(mdl, occ, theta, V)
        if not V:
            check_separation(ev)
        orders.append(tuple(e[5] for e in ev))
        x = [mpf(0)] * mdl["nstates"]
        if "init" in mdl and (o == 0 or "init_every_occasion" in V):
            x = list(mdl["init"](theta, covs_at(mdl, group["occasions"][0], 0.0)))
        infusions = []
        for k, (t, kind, val, dur, io, _) in enumerate(ev):
            if kind == "bolus":
                x[io] = x[io] + val * mpf(dose)
            elif kind == "inf":
                infusions.append((t, t + dur, float(val) * dose / dur, io))
            else:
                cv = covs_at(mdl, occ, t)
                der = mdl["derive"](t, theta, cv) if "derive" in mdl else []
                preds.append(mdl["out"](t, x, theta, cv, der))
            if k + 1 == len(ev):
                break
            ti, tf = t, ev[k + 1][0]
            if ti == tf:
                continue
            ts = [ti, tf]
            for (s, e, _, _) in infusions:
                ts += [b for b in (s, e) if ti < b < tf]
            ts.sort()
            kept = [ts[0]]
            for b in ts[1:]:  # Vec::dedup_by(|a, b| (a - b).abs() < 1e-12): against the last one kept
                if not abs(b - kept[-1]) < 1e-12:
                    kept.append(b)
            if pw is None or "params_not_rebuilt" not in V:
                pw = list(p_theta)
            cur = kept[0]
            for nxt in kept[1:]:
                rate = [mpf(0)] * mdl["ndrugs"]
                for (s, e, r, inp) in infusions:
                    if cur >= s and nxt <= e:
                        rate[inp] += mpf(r)
                if "seq" in mdl:
                    mdl["seq"](nxt, theta, covs_at(mdl, occ, nxt), pw)
                dt = nxt - cur
                t_cov = nxt if abs_time else dt
                cv = covs_at(mdl, occ, t_cov)
                if structure:
                    der = mdl["derive"](t_cov, theta, cv) if "derive" in mdl else []
                    kp = mdl["kernel_params"](pw, der)
                    kap = max(kap, kappa_of(structure, kp))
                    x[pm:] = expm_step(structure, kp, x[pm:pm + len(rate_matrix(structure, [1] * 8)[0])], rate[pm], mpf(dt))
                    if pm:
                        x[0] = mpf(0)
                else:
                    x = mdl["eq_fn"](mpf(dt), x, pw, cv, rate)
                cur = nxt
    return preds, float(kap), orders


# -------------------------------------------------------------------------------------------------------- ODE march
def march_ode(mdl, group, theta, V=(), dose=1.0):
    """-> (predictions, n_steps, kappa, orders)."""
    h_max = mdl["h_max"]
    n_steps, x_max, out_max, hs = 0, mpf(0), mpf(0), set()
    preds, orders = [], []
    cmax = max(abs(v) for occ in group["occasions"] for kn in occ["cov"].values() for _, v in kn)
    for o, occ in enumerate(group["occasions"]):
        ev = rewrite(mdl, occ, theta, V)
        if not V:
            check_separation(ev)
        orders.append(tuple(e[5] for e in ev))
        x = [mpf(0)] * mdl["nstates"]
        if o == 0 or "init_every_occasion" in V:
            x = list(mdl["init"](theta, covs_at(mdl, group["occasions"][0], 0.0)))
        clock = min(float(e[1]) for e in occ["events"])  # Occasion::initial_time(): the list as recorded
        if "clock_at_first_rewritten" in V:
            clock = ev[0][0]
        infs = [(t, t + dur, float(val) * dose / dur, io) for (t, kind, val, dur, io, _) in ev if kind == "inf"]
        bounds = sorted({b for (s, e, _, _) in infs for b in (s, e)})
        x_max = max([x_max] + [abs(v) for v in x])

        def cov_m(t):
            return [mpf(cov_value(occ["cov"][n], t)) if not isinstance(t, mpf) else cov_value(occ["cov"][n], t)
                    for n in mdl["covariates"]]

        for k, (t, kind, val, dur, io, _) in enumerate(ev):
            if kind == "bolus":
                amt = val * mpf(dose)
                if mdl["bolus_arg"] and "bolus_as_add" not in V:
                    zr = [mpf(0)] * mdl["ndrugs"]
                    b = [amt if i == io else mpf(0) for i in range(mdl["ndrugs"])]
                    f1 = mdl["rhs"](mpf(t), x, theta, cov_m(t), zr, b)
                    f0 = mdl["rhs"](mpf(t), x, theta, cov_m(t), zr, [mpf(0)] * mdl["ndrugs"])
                    x = [a + (p1 - p0) for a, p1, p0 in zip(x, f1, f0)]
                else:
                    x = list(x)
                    x[io] = x[io] + amt
                x_max = max([x_max] + [abs(v) for v in x])
            elif kind == "obs":
                preds.append(mdl["out"](t, x, theta, covs_at(mdl, occ, t), []))
                out_max = max(out_max, abs(x[mdl["central"]]))
            if k + 1 == len(ev):
                break
            nxt_t = ev[k + 1][0]
            while nxt_t > clock:
                stops = [b for b in bounds if clock < b <= nxt_t]
                stop = stops[0] if stops else nxt_t
                rate = [mpf(0)] * mdl["ndrugs"]
                for (s, e, r, inp) in infs:
                    if s <= clock and stop <= e:
                        rate[inp] += mpf(r)
                dt = stop - clock
                n = max(1, math.ceil(dt / h_max))
                h = dt / n
                hm, t0m = mpf(h), mpf(clock)

                def f(ts, xs):
                    return mdl["rhs"](ts, xs, theta, cov_m(ts), rate, None)

                for j in range(n):
                    x, _ = erk_step(RK4, f, t0m + j * hm, x, hm)
                    n_steps += 1
                    x_max = max([x_max] + [abs(v) for v in x])
                hs.add(h)
                clock = stop
    lam = mdl["rate_max"](theta, cmax)
    assert lam * max(hs) <= 1.0  # well inside RK4's stability interval: later steps are contractive
    kappa = float(n_steps * mp.exp(mpf(lam) * mpf(max(hs))) * x_max / out_max)
    return preds, n_steps, kappa, orders


# ------------------------------------------------------------------------------------------------------------ groups
def O(t):
    return ["obs", t, 0.0, 0.0, 0]


def B(t, amt, io=0):
    return ["bolus", t, amt, 0.0, io]


def I(t, amt, dur, io=0):
    return ["inf", t, amt, dur, io]


def occ(events, **cov):
    return dict(cov={k: [list(map(float, kv)) for kv in v] for k, v in cov.items()}, events=events)


FALL = [(0.0, 4.0), (16.0, -4.0)]                       # c(t) = 4 - t / 2: positive, then negative
ZIGZAG = [(0.0, 4.0), (8.0, -2.0), (16.0, 4.0), (24.0, -2.0)]
ZIGZAG_ODE = [(0.0, 4.0), (4.0, -2.0), (8.0, 4.0), (12.0, -2.0)]
FLAT2 = [(0.0, 2.0), (16.0, 2.0)]
WT = [(0.0, 64.0), (8.0, 96.0), (16.0, 48.0)]
TWO_RATES = ([0.2, 0.6, 0.3], [0.35, 0.4, 0.25], [0.15, 0.9, 0.5], [0.5, 0.3, 0.2], [0.25, 0.7, 0.35], [0.3, 0.5, 0.4])


def big_schedule(n, step, obs):
    return [occ([B(step * k, 5.0 + (k % 7), 0) for k in range(n)] + [O(t) for t in obs], c=ZIGZAG if step == 0.25 else ZIGZAG_ODE)]


BIG_OBS = (0.5, 2.0, 4.0625, 6.0, 8.0, 10.0, 12.0, 14.0, 16.5, 20.0, 23.0, 30.0)
FA_OCC = [occ([B(1.0, 100.0, 0), B(4.0, 80.0, 0), B(6.0, 50.0, 1), I(9.0, 120.0, 2.0, 0)] +
              [O(t) for t in (0.5, 2.0, 3.0, 5.0, 7.0, 8.0, 10.0, 11.5, 14.0, 18.0)], wt=WT)]
# theta = [ka, ke0, v, lag_scale, f0, x1(0)]
FA_THETAS = [[1.5, 0.2, 10.0, 0.0, 0.8, 0.0], [1.2, 0.25, 12.0, 1.0, 0.8, 15.0], [2.0, 0.15, 8.0, 2.0, 2.0, 0.0],
             [0.9, 0.3, 15.0, 4.0, -1.0, 30.0], [1.7, 0.1, 20.0, 0.5, 1.5, 5.0]]
TWO_OCC = [occ([B(1.0, 100.0, 0), O(2.0), O(4.0), B(5.0, 60.0, 0), O(6.0)], wt=[(0.0, 64.0), (8.0, 96.0)]),
           occ([O(0.5), B(1.0, 70.0, 0), O(2.0), O(3.0), O(6.0)], wt=[(0.0, 80.0), (8.0, 48.0)])]
ODE_EASY = [1.5, 0.2, 10.0, 0.0, 0.0, 8.0, 0.0]  # theta = [ka, ke, v, lag_scale, lag1, f0, x1(0)]; f0 = 8: fa clamps to 1
OVERTAKE_ODE = [occ([B(1.0, 100.0, 0), B(2.0, 80.0, 0), B(3.0, 60.0, 0), B(4.0, 40.0, 0), B(5.0, 20.0, 0), B(1.5, 30.0, 1),
                     I(3.0, 50.0, 2.5, 0)] + [O(t) for t in (0.5, 2.0, 4.5, 6.0, 8.0, 10.0, 12.0)], c=FALL)]
OVERTAKE_ODE_THETAS = [ODE_EASY, [1.1, 0.3, 12.0, 1.0, 0.5, 1.0, 0.0], [2.0, 0.15, 8.0, 2.0, -0.0, 0.8, 0.0],
                       [0.8, 0.25, 15.0, 3.0, 0.25, 2.0, 0.0], [3.0, 0.1, 20.0, -0.5, 1.0, 8.0, 0.0]]

GROUPS = [
    # ---- analytical
    dict(name="an_a_overtake", model="an_two", scalable=True, reorder=True, rules=["lag_at_landed"],
         why="a, d: a covariate-dependent lag; later doses overtake earlier ones and pass observations; lag +0.0 and -0.0",
         occasions=[occ([B(1.0, 100.0, 0), B(3.0, 80.0, 0), B(5.0, 60.0, 0), B(7.0, 40.0, 0), B(9.0, 30.0, 0), B(11.0, 20.0, 0),
                         B(2.0, 50.0, 1), I(3.0, 90.0, 4.0, 0)] + [O(t) for t in (0.5, 2.0, 4.5, 6.0, 8.0, 10.0, 12.0, 16.0, 20.0)],
                        c=FALL)],
         thetas=[r + [s, l1, v] for r, (s, l1, v) in zip(TWO_RATES, [(0.0, 0.0, 10.0), (1.0, 0.5, 12.0), (2.0, -0.0, 8.0),
                                                                    (3.0, 0.25, 15.0), (2.5, 0.0, 20.0), (-0.5, 1.0, 10.0)])]),
    dict(name="an_b_ties", model="an_oral", scalable=True, reorder=False, rules=["bolus_before_obs"],
         why="b: boluses landing exactly on an observation, another bolus, an infusion start, an infusion end, the first event",
         occasions=[occ([O(1.0), B(2.0, 100.0, 0), B(2.5, 40.0, 0), I(4.0, 60.0, 2.0, 0), B(3.0, 30.0, 1), O(3.0), O(4.0), O(5.0),
                         O(6.0), O(8.0), O(12.0)])],
         thetas=[[1.5, 0.2, 10.0, 0.0, 1.0], [1.2, 0.25, 12.0, 1.0, 1.0], [2.0, 0.15, 8.0, 4.0, 0.25], [0.9, 0.3, 15.0, 4.0, 1.0],
                 [1.7, 0.1, 20.0, -1.0, 1.0], [1.4, 0.22, 9.0, 0.5, 1.0], [1.1, 0.18, 11.0, 3.5, 1.0]]),
    dict(name="an_c_negative", model="an_oral", scalable=True, reorder=True, rules=[],
         why="c, j: negative lags put doses before the first event and before time 0; a NaN lag (sqrt of -1) in the last case",
         occasions=[occ([O(1.0), B(1.5, 100.0, 0), B(3.0, 50.0, 0), I(2.0, 40.0, 1.0, 0), O(2.0), O(4.0), O(6.0), O(9.0)])],
         thetas=[[1.5, 0.2, 10.0, 0.0, 1.0], [1.2, 0.25, 12.0, -1.0, 1.0], [2.0, 0.15, 8.0, -2.0, 1.0], [0.9, 0.3, 15.0, -2.5, 0.25],
                 [1.7, 0.1, 20.0, -2.5, 1.0], [1.4, 0.22, 9.0, 1.0, -1.0]]),
    dict(name="an_e_fa_segment_dt", model="an_cov_dt", scalable=False, reorder=False, rules=["fa_at_recorded", "derive_abs_under_dt"],
         why="e, h: fa of time and covariate with both clamps hit; derive on an interpolated covariate at the segment length",
         occasions=FA_OCC, thetas=FA_THETAS),
    dict(name="an_h_segment_end_abs", model="an_cov_abs", scalable=False, reorder=False, rules=["fa_at_recorded"],
         why="h: the same model with derive at the sub-segment's absolute end", occasions=FA_OCC, thetas=FA_THETAS),
    dict(name="an_f_seq_eq", model="an_user_eq", scalable=False, reorder=False, rules=["params_not_rebuilt"],
         why="f: seq_eq accumulates over a solve split at two infusion ends; a lagged bolus cuts it in two in some lanes; "
             "pmx_eq reads two rateiv entries",
         occasions=[occ([O(0.25), B(0.5, 10.0, 0), O(1.0), I(1.0, 8.0, 2.0, 0), I(1.5, 6.0, 1.0, 1), O(4.0), B(4.5, 5.0, 1), O(5.0)])],
         thetas=[[0.5, 0.0, 0.125], [0.4, 1.5, 0.25], [0.7, 2.25, 0.0625], [0.3, 2.0, 0.5], [0.6, 3.0, 0.125]]),
    dict(name="an_g_two_occasions", model="an_cov_dt", scalable=False, reorder=False, rules=["init_every_occasion"],
         why="g: two occasions, a lag in both, init in the first only, a bolus lagged beyond the first occasion's last event",
         occasions=TWO_OCC,
         thetas=[[1.5, 0.2, 10.0, 0.0, 0.8, 20.0], [1.2, 0.25, 12.0, 1.0, 0.8, 20.0], [2.0, 0.15, 8.0, 2.0, 2.0, 10.0],
                 [0.9, 0.3, 15.0, 0.5, 1.0, 40.0]]),
    dict(name="an_pm_wrapper", model="an_pm", scalable=True, reorder=True, rules=["lag_at_landed"],
         why="a on the pm_ wrapper: 1-based inputs, a bolus into the dead slot 0, the pad re-zeroed after every step",
         occasions=[occ([B(1.0, 100.0, 1), B(3.0, 80.0, 1), B(5.0, 60.0, 1), B(2.0, 40.0, 2), B(2.5, 1000.0, 0), I(3.0, 60.0, 2.0, 1)] +
                        [O(t) for t in (0.5, 2.0, 4.0, 4.5, 6.0, 8.0, 10.0, 12.0)], c=FALL)],
         thetas=[[1.5, 0.2, 10.0, 0.0], [1.2, 0.25, 12.0, 1.0], [2.0, 0.15, 8.0, 2.0], [0.9, 0.3, 15.0, 3.0], [1.7, 0.1, 20.0, -0.5]]),
] + [
    dict(name=f"an_i_big_{n}", model="an_two", scalable=True, reorder=True, rules=[],
         why=f"i: {n} boluses in one occasion (64 are kept per lane), a zigzag lag that reorders them",
         occasions=big_schedule(n, 0.25, BIG_OBS),
         thetas=[r + [s, 0.0, 10.0] for r, s in zip(TWO_RATES, (0.0, 2.0, 3.0, 2.5, -1.0))]) for n in (64, 65, 90)
] + [
    # ---- ODE
    dict(name=f"ode_a_overtake_{form}", model=f"ode_{form}", scalable=True, reorder=True, rules=["lag_at_landed"],
         why="a, d: later doses overtake earlier ones; one lane lands a dose before the clock; dynamics on a moving covariate",
         occasions=OVERTAKE_ODE, thetas=OVERTAKE_ODE_THETAS) for form in ("routes", "bolus")
] + [
    dict(name="ode_b_ties", model="ode_bolus", scalable=True, reorder=False, rules=["bolus_before_obs"],
         why="b: a bolus recorded before the first remaining event, an infusion, lands exactly on it (and acts from the clock "
             "on); ties with an observation, with another bolus and an infusion end, with the recorded initial time",
         occasions=[occ([B(0.5, 100.0, 0), I(1.0, 60.0, 2.0, 0), O(2.0), O(3.0), B(3.0, 30.0, 1), O(4.0), O(6.0)], c=FLAT2)],
         thetas=[ODE_EASY, [1.1, 0.3, 12.0, 0.25, 0.0, 8.0, 0.0], [2.0, 0.15, 8.0, 0.75, 0.0, 8.0, 0.0],
                 [0.8, 0.25, 15.0, 1.25, 0.0, 8.0, 0.0], [3.0, 0.1, 20.0, 1.75, 1.0, 8.0, 0.0], [1.3, 0.2, 9.0, -0.25, 0.0, 8.0, 0.0]]),
    dict(name="ode_c_clock", model="ode_routes", scalable=True, reorder=True, rules=["clock_at_first_rewritten"],
         why="c: the first event of the rewritten list is a lagged bolus: it acts from the recorded initial time on",
         occasions=[occ([B(1.0, 100.0, 0), O(2.0), O(3.0), B(2.5, 50.0, 0), O(4.0), O(6.0)], c=FLAT2)],
         thetas=[ODE_EASY, [1.1, 0.3, 12.0, 0.25, 0.0, 8.0, 0.0], [2.0, 0.15, 8.0, -0.25, 0.0, 8.0, 0.0],
                 [0.8, 0.25, 15.0, 0.75, 0.0, 8.0, 0.0], [3.0, 0.1, 20.0, 1.25, 0.0, 8.0, 0.0]]),
    dict(name="ode_e_fa", model="ode_routes", scalable=True, reorder=False, rules=["fa_at_recorded"],
         why="e: fa of the landing time and the covariate there, both clamps hit",
         occasions=[occ([O(0.0), B(0.5, 20.0, 1), B(1.0, 100.0, 0), B(3.0, 80.0, 0)] + [O(t) for t in (2.0, 4.0, 5.0, 6.0, 8.0)], c=FALL)],
         thetas=[[1.5, 0.2, 10.0, 0.0, 0.0, 1.0, 0.0], [1.1, 0.3, 12.0, 1.0, 0.0, 0.8, 0.0], [2.0, 0.15, 8.0, 0.5, 0.0, 4.0, 0.0],
                 [0.8, 0.25, 15.0, 1.0, 0.0, -1.0, 0.0], [3.0, 0.1, 20.0, 2.0, 0.0, 0.5, 0.0]]),
    dict(name="ode_g_two_occasions", model="ode_bolus", scalable=False, reorder=False, rules=["init_every_occasion"],
         why="g: two occasions, a lag in both, init in the first only, a bolus lagged beyond the first occasion's last event",
         occasions=[occ(TWO_OCC[0]["events"], c=[(0.0, 4.0), (8.0, 0.0)]), occ(TWO_OCC[1]["events"], c=[(0.0, 2.0), (8.0, -2.0)])],
         thetas=[[1.5, 0.2, 10.0, 0.0, 0.0, 8.0, 20.0], [1.1, 0.3, 12.0, 0.5, 0.0, 1.0, 20.0], [2.0, 0.15, 8.0, 1.0, 0.0, 0.8, 10.0],
                 [0.8, 0.25, 15.0, -0.125, 0.0, 2.0, 40.0]]),
    dict(name="ode_weighted_bolus", model="ode_weighted", scalable=False, reorder=False, rules=["bolus_as_add", "unstable_equal_boluses"],
         why="a bolus argument entering two states with different weights, one of them state-dependent; two boluses at one time",
         occasions=[occ([O(0.0), B(1.0, 100.0, 0), B(1.0, 60.0, 0), B(1.5, 30.0, 1)] + [O(t) for t in (1.25, 2.5, 3.0, 4.0, 6.0)],
                        c=FLAT2)],
         thetas=[ODE_EASY, [1.1, 0.3, 12.0, 0.25, 0.5, 8.0, 5.0], [2.0, 0.15, 8.0, 0.5, 0.0, 8.0, 0.0], [0.8, 0.25, 15.0, -0.25, 0.25, 2.0, 0.0]]),
    dict(name="ode_i_big_65", model="ode_routes", scalable=True, reorder=True, rules=[],
         why="i: 65 boluses in one occasion, a zigzag lag that reorders them",
         occasions=big_schedule(65, 0.125, (0.5, 1.0, 2.0, 3.0625, 4.0, 6.0, 8.0, 10.0, 12.0)),
         thetas=[ODE_EASY] + [[ka, ke, v, s, 0.0, 8.0, 0.0] for ka, ke, v, s in ((1.1, 0.3, 12.0, 1.0), (2.0, 0.15, 8.0, 2.0),
                                                                                (0.8, 0.25, 15.0, 0.5), (3.0, 0.1, 20.0, -1.0))]),
]


# ------------------------------------------------------------------------------------------------------------- build
def fl(xs):
    return [float(v) for v in xs]


def rel(a, b):
    return float(max(abs(x - y) for x, y in zip(a, b)) / max(abs(v) for v in b))


def run(mdl, group, theta, V=(), dose=1.0):
    """-> dict(pred, kappa, bar, orders[, n_steps]) or None for a NaN lag."""
    try:
        if mdl["backend"] == "ode":
            pred, n_steps, kappa, orders = march_ode(mdl, group, theta, V, dose)
            return dict(pred=pred, kappa=kappa, bar=64 * U * kappa, orders=orders, n_steps=n_steps)
        pred, kappa, orders = march_analytical(mdl, group, theta, V, dose)
        return dict(pred=pred, kappa=kappa, bar=max(1e-10, 64 * U * kappa), orders=orders)
    except BadLag:
        return None


def build(group):
    mdl = MODELS[group["model"]]
    n_dose = sum(1 for o in group["occasions"] for e in o["events"] if e[0] != "obs")
    n_obs = sum(1 for o in group["occasions"] for e in o["events"] if e[0] == "obs")
    assert n_obs <= 12 and (n_dose <= 12 or "_big_" in group["name"]), group["name"]
    runs = [run(mdl, group, th) for th in group["thetas"]]
    r0 = rewrite(mdl, group["occasions"][0], group["thetas"][0])
    assert [e[0] for e in r0] == sorted(float(e[1]) for e in group["occasions"][0]["events"]), "the first case has no lag"
    cases = []
    for th, r in zip(group["thetas"], runs):
        if r is None:
            cases.append(dict(theta=fl(th), status="PMX_PAIR_BAD_LAG", kappa=1.0, expected=None))
            continue
        c = dict(theta=fl(th), status=None, kappa=r["kappa"], expected=fl(r["pred"]))
        if "n_steps" in r:
            c["n_steps"] = r["n_steps"]
            assert r["bar"] <= 1e-10, (group["name"], th, r["kappa"])  # far below what any rule moves a case by
        cases.append(c)
    if group["reorder"]:
        assert len({tuple(r["orders"]) for r in runs if r}) >= 4, (group["name"], "fewer than 4 landing orders")
    for rule in group["rules"]:
        assert rule in VARIANTS
        moved = 0.0
        for th, r in zip(group["thetas"], runs):
            if r is not None:
                w = run(mdl, group, th, (rule,))
                moved = max(moved, rel(w["pred"], r["pred"]) / r["bar"])
        assert moved >= 1000, (group["name"], rule, moved)
        print(f"  {rule}: moves a case by {moved:.3g} bars", flush=True)
    if group["scalable"]:
        th, r = next((th, r) for th, r in reversed(list(zip(group["thetas"], runs))) if r)
        twice = run(mdl, group, th, dose=2.0)
        assert rel(twice["pred"], [2 * v for v in r["pred"]]) <= 1e-30, group["name"]
    return dict(name=group["name"], model=group["model"], why=group["why"], scalable=group["scalable"], rules=group["rules"],
                occasions=group["occasions"], cases=cases)


def main():
    groups = []
    for g in GROUPS:
        print(g["name"], flush=True)
        groups.append(build(g))
    with open(OUT, "w") as f:
        json.dump(dict(generator="tests/golden/gen_user_closures.py", dps=40, groups=groups), f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {OUT}: {len(groups)} groups, {sum(len(g['cases']) for g in groups)} cases, {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(HERE, "edge_math.json"))


if __name__ == "__main__":
    main()
