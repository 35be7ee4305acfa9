#!/usr/bin/env python3
"""Generate tests/golden/ode_exact.json: what the ODE walkers must return, to rounding.

A classic RK4 step (and a Dormand-Prince step that the controller accepts at full length) is a finite sequence of
rational operations, so its result can be evaluated exactly: here stage by stage in mpmath at 40 digits, from textbook
tableaux, the published equations of the bodies and the project's documented step rule - without the oracle and without
the device code.  A fixed-step kernel is then held to rounding (bar = 64 u kappa), not to the 1e-4 that a comparison
with the true solution allows at easy rates.

Partition rule ("ODE step partition"):
  * the events of an occasion are rewritten: a bolus on a lagged input moves to t + lag, its amount is multiplied by fa;
  * integration pieces end at every time of the rewritten list and at every infusion start and end;
  * the RECORDED time of a moved bolus is not a break;
  * at equal times the order is observation, bolus, infusion;
  * every occasion starts from a zero state at its first event; `init` applies to the first occasion only.
Per piece [t0, t1], in Python doubles exactly as written:  dt = t1 - t0,  n = max(1, ceil(dt / h_max)),  h = dt / n;  only
then converted to mpf.  An infusion contributes amount / duration to rateiv[input] on [t, t + duration).

Steppers: one explicit Runge-Kutta routine over a tableau; tableau 1 = classic RK4, tableau 2 = Dormand-Prince 5(4)
with both weight rows.  Forced-step DOPRI5: with loose tolerances and a small h_max every step is min(h_max, left) and
the controller never shortens one while each step's scaled error norm stays <= 0.9^5; asserted <= 0.25 here.

Stored per case: `rk4` (exact-arithmetic RK4 predictions), `exact` (the true solution: augmented matrix exponential for
the linear bodies, Lambert-W closed form for Michaelis-Menten, closed form for the non-autonomous body), `n_steps`, and
kappa = n_steps exp(max|lambda| h) max_k |x_k|_inf / max_obs |x_out|: a first-order bound on accumulated rounding (each
step perturbs by O(u) T4(|hA|) |x|; later steps are contractive, which is asserted).

Self-checks (conditions, asserted): (a) 64 u kappa <= 1e-11 for every case; (b) in every group at least half the cases
have |rk4 - exact| / scale >= 1000 bar; (c) in every lag group, recorded times as extra breaks move at least one case
by >= 100 bar; (d) for the non-autonomous body, stage times frozen at the piece start move every case by >= 1000 bar.

Run:  python tests/golden/gen_ode_exact.py      (deterministic; rewrites ode_exact.json byte for byte)
"""
import json
import math
import os

import mpmath as mp

mp.mp.dps = 40
mpf = mp.mpf
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ode_exact.json")
U = 2.0 ** -53

# ----------------------------------------------------------------------------------------------------------- tableaux
F = mp.mpf
RK4 = dict(c=[F(0), F(1) / 2, F(1) / 2, F(1)],
           a=[[], [F(1) / 2], [F(0), F(1) / 2], [F(0), F(0), F(1)]],
           b=[F(1) / 6, F(1) / 3, F(1) / 3, F(1) / 6], order=4)
DP = dict(c=[F(0), F(1) / 5, F(3) / 10, F(4) / 5, F(8) / 9, F(1), F(1)],
          a=[[],
             [F(1) / 5],
             [F(3) / 40, F(9) / 40],
             [F(44) / 45, F(-56) / 15, F(32) / 9],
             [F(19372) / 6561, F(-25360) / 2187, F(64448) / 6561, F(-212) / 729],
             [F(9017) / 3168, F(-355) / 33, F(46732) / 5247, F(49) / 176, F(-5103) / 18656],
             [F(35) / 384, F(0), F(500) / 1113, F(125) / 192, F(-2187) / 6784, F(11) / 84]],
          b=[F(35) / 384, F(0), F(500) / 1113, F(125) / 192, F(-2187) / 6784, F(11) / 84, F(0)],
          bhat=[F(5179) / 57600, F(0), F(7571) / 16695, F(393) / 640, F(-92097) / 339200, F(187) / 2100, F(1) / 40], order=5)


def erk_step(tab, f, t, x, h, freeze_t=False):
    """One explicit Runge-Kutta step; returns (x_new, x_hat or None)."""
    ks = []
    for i, ci in enumerate(tab["c"]):
        xi = [x[s] + h * sum((tab["a"][i][j] * ks[j][s] for j in range(i)), mpf(0)) for s in range(len(x))]
        ks.append(f(t if freeze_t else t + ci * h, xi))
    new = [x[s] + h * sum((tab["b"][i] * ks[i][s] for i in range(len(ks))), mpf(0)) for s in range(len(x))]
    hat = None
    if "bhat" in tab:
        hat = [x[s] + h * sum((tab["bhat"][i] * ks[i][s] for i in range(len(ks))), mpf(0)) for s in range(len(x))]
    return new, hat


# ------------------------------------------------------------------------------------------------------------- bodies
# name -> (n states, n body parameters, central state).  Equations: include/pmx.h PMX_ODE_* (SURVEY.md section 3 cites
# the reference's test ODEs they restate); rateiv[0] enters the central compartment.
BODIES = {"one_cmt_iv": (1, 1, 0), "one_cmt_oral": (2, 2, 1), "two_cmt_iv": (2, 3, 0), "two_cmt_oral": (3, 4, 1),
          "three_cmt_iv": (3, 5, 0), "three_cmt_oral": (4, 6, 1), "one_cmt_mm": (1, 3, 0),
          "custom_lin2": (2, 3, 0), "custom_nonaut": (1, 3, 0)}


def matrix_of(body, p):
    """A of the linear bodies (dx = A x + B rateiv)."""
    if body == "one_cmt_iv":
        return [[-p[0]]]
    if body == "one_cmt_oral":
        ka, ke = p[:2]
        return [[-ka, 0], [ka, -ke]]
    if body == "two_cmt_iv":
        ke, kcp, kpc = p[:3]
        return [[-(ke + kcp), kpc], [kcp, -kpc]]
    if body == "two_cmt_oral":
        ke, ka, kcp, kpc = p[:4]
        return [[-ka, 0, 0], [ka, -(ke + kcp), kpc], [0, kcp, -kpc]]
    if body == "three_cmt_iv":
        k10, k12, k13, k21, k31 = p[:5]
        return [[-(k10 + k12 + k13), k21, k31], [k12, -k21, 0], [k13, 0, -k31]]
    if body == "three_cmt_oral":
        ka, k10, k12, k13, k21, k31 = p[:6]
        return [[-ka, 0, 0, 0], [ka, -(k10 + k12 + k13), k21, k31], [0, k12, -k21, 0], [0, k13, 0, -k31]]
    if body == "custom_lin2":  # dx0 = -(p0 + p1) x0 + p2 x1 + rateiv0 ; dx1 = p1 x0 - p2 x1 + rateiv1
        return [[-(p[0] + p[1]), p[2]], [p[1], -p[2]]]
    if body == "custom_nonaut":
        return [[-p[0]]]
    return None


def rate_vector(body, r):
    ns, _, central = BODIES[body]
    b = [mpf(0)] * ns
    if body == "custom_lin2":
        return [r[0], r[1]]
    b[central] = r[0]
    return b


def rhs_of(body, p, r):
    """f(t, x) with rateiv = r (mpf per input)."""
    if body == "one_cmt_mm":
        vmax, km, v = p[:3]

        def f(t, x):
            c = x[0] / v
            return [-vmax * c / (km + c) + r[0]]
        return f
    A = matrix_of(body, p)
    b = rate_vector(body, r)
    n = len(A)
    if body == "custom_nonaut":
        def f(t, x):
            return [-p[0] * x[0] + r[0] + p[2] * (t - 3) ** 2]
        return f

    def f(t, x):
        return [sum((A[i][j] * x[j] for j in range(n)), mpf(0)) + b[i] for i in range(n)]
    return f


def lambda_max(body, p):
    if body == "one_cmt_mm":
        return p[0] / (p[2] * p[1])  # |df/dx| is largest at x = 0
    A = matrix_of(body, p)
    ev = mp.eig(mp.matrix(A), left=False, right=False)
    ev = list(ev[0]) if isinstance(ev, tuple) else list(ev)
    assert all(abs(mp.im(e)) < mpf(10) ** -30 and mp.re(e) < 0 for e in ev), (body, ev)
    return max(abs(mp.re(e)) for e in ev)


def stability(order, z):
    """|R(z)| of the s-stage order-p methods used here on the real axis (RK4: Taylor 4; DOPRI5: Taylor 5 + z^6/600)."""
    r = sum((z ** k / mp.factorial(k) for k in range(order + 1)), mpf(0))
    if order == 5:
        r += z ** 6 / 600
    return abs(r)


# ----------------------------------------------------------------------------------------------------------- schedule
RANK = {"obs": 0, "bolus": 1, "inf": 2}


def rewrite(occasion, lag, fa, theta, recorded_breaks=False):
    """The occasion's rewritten event list, time-sorted (stable; observation < bolus < infusion at equal times), as
    (t, kind, value, duration, input) in doubles, and the extra break times (infusion ends; recorded times on demand)."""
    ev, extra = [], []
    for kind, t, val, dur, io in occasion:
        t, val, dur = float(t), float(val), float(dur)
        if kind == "bolus":
            if str(io) in lag:
                if recorded_breaks:
                    extra.append(t)
                t = t + float(theta[lag[str(io)]])
            if str(io) in fa:
                val = val * float(theta[fa[str(io)]])
        if kind == "inf":
            extra.append(t + dur)
        ev.append((t, kind, val, dur, io))
    ev = sorted(ev, key=lambda e: (e[0], RANK[e[1]]))
    return ev, sorted(extra)


class Walk:
    """State, counters and the piece walker shared by every stepper."""

    def __init__(self, group, theta, recorded_breaks=False):
        self.g, self.theta = group, [float(v) for v in theta]
        mdl = group["model"]
        self.body = mdl["body"]
        self.ns, self.nb, self.central = BODIES[self.body]
        self.p = [mpf(v) for v in self.theta]
        self.recorded_breaks = recorded_breaks
        self.v = self.p[mdl["v"]] if mdl["v"] is not None else mpf(1)
        self.n_steps, self.x_max, self.h_all = 0, mpf(0), set()

    def run(self, piece_fn):
        """piece_fn(x, t0, t1, rates, first_obs_row_after) -> x.  Returns predictions (amount / v) per observation."""
        mdl = self.g["model"]
        out = []
        for o, occ in enumerate(self.g["occasions"]):
            ev, extra = rewrite(occ, mdl["lag"], mdl["fa"], self.theta, self.recorded_breaks)
            x = [mpf(0)] * self.ns
            if o == 0:
                for st, par in mdl["init"].items():
                    x[int(st)] = self.p[par]
            t = ev[0][0]
            t_end = ev[-1][0]
            active = []  # (end, rate, input)
            self.x_max = max([self.x_max] + [abs(v) for v in x])
            for (te, kind, val, dur, io) in ev:
                while t < te:
                    nxt = min([te] + [b for b in extra if t < b < te])
                    rates = [mpf(0)] * mdl["ndrugs"]
                    for (end, rate, inp) in active:
                        if end > t:
                            rates[inp] += mpf(rate)
                    x = piece_fn(x, t, nxt, rates, len(out))
                    t = nxt
                if kind == "obs":
                    out.append(x[self.central] / self.v)
                elif kind == "bolus":
                    x = list(x)
                    x[int(io)] += mpf(val)
                    self.x_max = max(self.x_max, abs(x[int(io)]))
                else:
                    active.append((te + dur, val / dur, int(io)))
            assert t == t_end
        return out

    def note(self, x, h):
        self.n_steps += 1
        self.h_all.add(h)
        self.x_max = max([self.x_max] + [abs(v) for v in x])


def step_count(t0, t1, h_max):
    dt = t1 - t0
    n = max(1, math.ceil(dt / h_max))
    return n, dt / n


def walk_rk4(group, theta, recorded_breaks=False, freeze_t=False, probe=None):
    """Exact-arithmetic RK4.  probe = (rtol, atol): also the step-doubling estimate q of every piece's first step;
    returns (pred, walk, [(q, first observation row after the piece)])."""
    w = Walk(group, theta, recorded_breaks)
    h_max = group["h_max"]
    qs = []

    def piece(x, t0, t1, rates, row):
        f = rhs_of(w.body, w.p, rates)
        n, h = step_count(t0, t1, h_max)
        hm, t0m = mpf(h), mpf(t0)
        if probe:
            rtol, atol = mpf(probe[0]), mpf(probe[1])
            xa, _ = erk_step(RK4, f, t0m, x, hm)
            xh, _ = erk_step(RK4, f, t0m, x, hm / 2)
            xb, _ = erk_step(RK4, f, t0m + hm / 2, xh, hm / 2)
            e = [mpf(16) / 15 * (b - a) / (atol + rtol * max(abs(a), abs(b))) for a, b in zip(xa, xb)]
            qs.append((mp.sqrt(sum(v * v for v in e) / len(e)), row))
        for j in range(n):
            tj = t0m if freeze_t else t0m + j * hm
            x, _ = erk_step(RK4, f, tj, x, hm, freeze_t)
            w.note(x, h)
        return x

    return w.run(piece), w, qs


def walk_dopri5(group, theta, h_max, tol):
    """Forced-step DOPRI5: every step min(h_max, left); returns (pred, walk, largest scaled error norm of a step)."""
    w = Walk(group, theta)
    worst = [mpf(0)]
    rtol = atol = mpf(tol)

    def piece(x, t0, t1, rates, row):
        f = rhs_of(w.body, w.p, rates)
        t = t0
        while t < t1:
            left = t1 - t
            h = min(h_max, left)
            new, hat = erk_step(DP, f, mpf(t), x, mpf(h))
            e = [(a - b) / (atol + rtol * max(abs(xo), abs(a))) for a, b, xo in zip(new, hat, x)]
            worst[0] = max(worst[0], mp.sqrt(sum(v * v for v in e) / len(e)))
            x = new
            w.note(x, h)
            t = t1 if h == left else t + h
        return x

    return w.run(piece), w, worst[0]


def walk_exact(group, theta):
    w = Walk(group, theta)
    mp.mp.dps = 60

    def piece(x, t0, t1, rates, row):
        dt = mpf(t1) - mpf(t0)
        if w.body == "one_cmt_mm":
            assert rates[0] == 0
            vmax, km, v = w.p[:3]
            c0 = x[0] / v
            if c0 == 0:
                return x
            c = km * mp.lambertw(c0 / km * mp.exp((c0 - vmax / v * dt) / km))
            return [c * v]
        if w.body == "custom_nonaut":
            k, c2, r = w.p[0], w.p[2], rates[0]
            a2 = c2 / k
            a1 = -2 * a2 / k
            a0 = (r - a1) / k

            def part(t):
                s = mpf(t) - 3
                return a0 + a1 * s + a2 * s * s
            return [part(t1) + (x[0] - part(t0)) * mp.exp(-k * dt)]
        A = matrix_of(w.body, w.p)
        b = rate_vector(w.body, rates)
        n = len(A)
        M = mp.matrix(n + 1, n + 1)
        for i in range(n):
            for j in range(n):
                M[i, j] = A[i][j]
            M[i, n] = b[i]
        E = mp.expm(M * dt)
        xa = mp.matrix([*x, 1])
        xb = E * xa
        return [xb[i] for i in range(n)]

    try:
        return w.run(piece)
    finally:
        mp.mp.dps = 40


# ------------------------------------------------------------------------------------------------------------- groups
def O(t):
    return ["obs", t, 0.0, 0.0, 0]


def B(t, amt, io=0):
    return ["bolus", t, amt, 0.0, io]


def I(t, amt, dur, io=0):
    return ["inf", t, amt, dur, io]


# Every schedule: an observation and a bolus at one time; an infusion ending at 1.8 (or 2.1) strictly inside an
# observation gap; two overlapping infusions; a gap of 3.1 h (62 steps at h_max = 0.05, more than one trip of the PAIR
# state machine); a second occasion.  An observation 0.002 h after the largest bolus into the observed compartment puts
# the largest state among the predictions, whatever the rates, so that kappa stays near the step count.
def plain_schedule(oral=False, first=100.0):
    head = [O(0.0), B(0.0, first, 0)] + ([B(0.0, first, 1)] if oral else []) + [O(0.002)]
    return [head + [O(0.13), O(0.5), I(0.5, 60.0, 1.3, 0), O(1.0), I(1.0, 45.0, 1.45, 0), B(1.0, 30.0, 1 if oral else 0),
                    O(1.5), O(2.0), O(2.6), O(5.7)],
            [O(0.0), B(0.1, 50.0, 0), O(0.35), I(0.35, 20.0, 0.4, 0), O(1.0)]]


# lag groups: an observation opens each occasion; input 0 (the depot) is lagged; recorded times 1.23 (state non-zero, off
# the h_max raster) and landing times off the raster; input 1 (central) lands at `t_central` with an observation just after
def lag_schedule(t_central_recorded, t_central_lands):
    return [[O(0.0), B(0.0, 100.0, 0), O(0.2), O(0.5), B(t_central_recorded, 100.0, 1), O(round(t_central_lands + 0.002, 3)),
             O(0.9), I(1.2, 50.0, 0.9, 0), B(1.23, 40.0, 0), I(1.5, 30.0, 1.0, 0), O(1.5), O(2.0), O(2.5), O(5.6)],
            [O(0.0), B(0.5, 80.0, 0), O(1.0), O(1.6)]]


MM_SCHEDULE = [[O(0.0), B(0.0, 100.0, 0), O(0.13), O(0.5), B(1.0, 40.0, 0), O(1.0), O(1.5), O(2.0), O(2.6), O(5.7)],
               [O(0.0), B(0.1, 50.0, 0), O(0.35), O(1.0)]]


def model(body, nparams, v, ndrugs, init=None, lag=None, fa=None):
    return dict(body=body, nparams=nparams, v=v, ndrugs=ndrugs, init={str(k): i for k, i in (init or {}).items()},
                lag={str(k): i for k, i in (lag or {}).items()}, fa={str(k): i for k, i in (fa or {}).items()})


H = 0.05
CK = dict(rtol=1e-4, atol=1e-4)
# `scalable`: the truth is linear in the doses (linear body, no initial amount, no forcing)
GROUPS = [
    # theta = [ke, v, x0(0)]: init on the first occasion only
    dict(name="one_cmt_iv_init", scalable=False, model=model("one_cmt_iv", 3, 1, 1, init={0: 2}), h_max=H,
         occasions=plain_schedule(first=20.0),
         thetas=[[0.37, 12.0, 100.0], [10.0, 12.0, 100.0], [25.0, 9.0, 100.0], [37.0, 30.0, 100.0]],
         dopri5=dict(h_max=0.1, tol=0.05, thetas=[[0.37, 12.0, 100.0], [3.1, 12.0, 100.0]]), checked=CK,
         adaptive=dict(dopri5=[[0.37, 12.0, 100.0], [3.1, 9.0, 50.0]], ros2=[[0.37, 12.0, 100.0]])),
    # theta = [ka, ke, v, lag0, fa0]; input 1 = a bolus into the central compartment, not lagged
    dict(name="one_cmt_oral_lag_fa", scalable=True, model=model("one_cmt_oral", 5, 2, 2, lag={0: 3}, fa={0: 4}), h_max=H,
         occasions=lag_schedule(1.03, 1.03),
         thetas=[[1.1, 0.3, 20.0, 0.26, 0.8], [12.0, 0.9, 20.0, 0.26, 0.8], [30.0, 2.0, 15.0, 0.26, 0.65], [38.0, 0.4, 15.0, 0.31, 1.0]],
         dopri5=dict(h_max=0.1, tol=0.05, thetas=[[1.1, 0.3, 20.0, 0.26, 0.8], [3.0, 0.9, 20.0, 0.26, 0.8]]), checked=CK,
         adaptive=dict(dopri5=[[1.1, 0.3, 20.0, 0.26, 0.8]],
                       ros2=[[1.1, 0.3, 20.0, 0.26, 0.8], [200.0, 0.3, 20.0, 0.26, 0.8], [5000.0, 0.9, 20.0, 0.26, 0.8]])),
    # theta = [ke, kcp, kpc, v]
    dict(name="two_cmt_iv", scalable=True, model=model("two_cmt_iv", 4, 3, 1), h_max=H, occasions=plain_schedule(),
         thetas=[[0.2, 0.5, 0.3, 25.0], [6.0, 4.0, 1.5, 25.0], [14.0, 12.0, 3.0, 10.0], [20.0, 15.0, 8.0, 10.0]],
         dopri5=dict(h_max=0.15, tol=0.1, thetas=[[0.2, 0.5, 0.3, 25.0], [1.0, 1.5, 0.6, 25.0]]), checked=CK,
         adaptive=dict(dopri5=[[0.2, 0.5, 0.3, 25.0]], ros2=[[0.2, 0.5, 0.3, 25.0]])),
    # theta = [ke, ka, kcp, kpc, v, lag0, lag1, fa0]: two inputs, two lags, one of them negative (1.03 - 0.3 = 0.73)
    dict(name="two_cmt_oral_two_lags", scalable=True, model=model("two_cmt_oral", 8, 4, 2, lag={0: 5, 1: 6}, fa={0: 7}), h_max=H,
         occasions=lag_schedule(1.03, 0.73),
         thetas=[[0.25, 1.3, 0.4, 0.2, 30.0, 0.26, -0.3, 0.9], [1.0, 14.0, 2.0, 1.0, 30.0, 0.26, -0.3, 0.9],
                 [3.0, 28.0, 6.0, 2.5, 12.0, 0.26, -0.3, 0.7], [2.0, 39.0, 1.0, 0.5, 12.0, 0.37, -0.3, 1.0]],
         dopri5=dict(h_max=0.1, tol=0.05, thetas=[[0.25, 1.3, 0.4, 0.2, 30.0, 0.26, -0.3, 0.9], [1.0, 3.0, 1.0, 0.5, 30.0, 0.26, -0.3, 0.9]]),
         checked=CK,
         adaptive=dict(dopri5=[[0.25, 1.3, 0.4, 0.2, 30.0, 0.26, -0.3, 0.9]],
                       ros2=[[0.25, 1.3, 0.4, 0.2, 30.0, 0.26, -0.3, 0.9], [0.25, 1000.0, 0.4, 0.2, 30.0, 0.26, -0.3, 0.9]])),
    # theta = [k10, k12, k13, k21, k31, v]
    dict(name="three_cmt_iv", scalable=True, model=model("three_cmt_iv", 6, 5, 1), h_max=H, occasions=plain_schedule(),
         thetas=[[0.15, 0.4, 0.2, 0.3, 0.1, 40.0], [5.0, 3.0, 2.0, 1.0, 0.5, 40.0], [12.0, 8.0, 6.0, 3.0, 1.0, 15.0],
                 [18.0, 10.0, 7.0, 6.0, 2.0, 15.0]],
         dopri5=dict(h_max=0.1, tol=0.05, thetas=[[0.15, 0.4, 0.2, 0.3, 0.1, 40.0]]), checked=CK,
         adaptive=dict(dopri5=[[0.15, 0.4, 0.2, 0.3, 0.1, 40.0]], ros2=[])),
    # theta = [ka, k10, k12, k13, k21, k31, v]: boluses on both inputs (depot, central)
    dict(name="three_cmt_oral", scalable=True, model=model("three_cmt_oral", 7, 6, 2), h_max=H, occasions=plain_schedule(oral=True),
         thetas=[[0.9, 0.15, 0.4, 0.2, 0.3, 0.1, 40.0], [11.0, 1.0, 1.0, 0.5, 0.6, 0.2, 40.0], [26.0, 2.0, 3.0, 1.0, 1.0, 0.4, 18.0],
                 [38.0, 0.5, 0.8, 0.3, 0.5, 0.2, 18.0]],
         dopri5=dict(h_max=0.1, tol=0.05, thetas=[[0.9, 0.15, 0.4, 0.2, 0.3, 0.1, 40.0]]), checked=CK,
         adaptive=dict(dopri5=[[0.9, 0.15, 0.4, 0.2, 0.3, 0.1, 40.0]], ros2=[[2000.0, 0.15, 0.4, 0.2, 0.3, 0.1, 40.0]])),
    # theta = [vmax, km, v]: nonlinear, bolus only (the closed form needs a zero rate)
    dict(name="one_cmt_mm", scalable=False, model=model("one_cmt_mm", 3, 2, 1), h_max=H, occasions=MM_SCHEDULE,
         thetas=[[8.0, 4.0, 10.0], [30.0, 0.3, 10.0], [45.0, 0.15, 10.0], [70.0, 0.2, 10.0]],
         dopri5=dict(h_max=0.1, tol=0.05, thetas=[[8.0, 4.0, 10.0]]), checked=dict(rtol=1e-7, atol=1e-7),
         adaptive=dict(dopri5=[[8.0, 4.0, 10.0]], ros2=[[8.0, 4.0, 10.0]])),
    # custom bodies (hiprtc); theta = [p0, p1, p2], output x0; rateiv on both states
    dict(name="custom_lin2", scalable=True, model=model("custom_lin2", 3, None, 2), h_max=H,
         occasions=[[O(0.0), B(0.0, 100.0, 0), O(0.002), O(0.13), O(0.5), I(0.5, 60.0, 1.3, 0), O(1.0), I(1.0, 45.0, 1.45, 1),
                     B(1.0, 30.0, 1), O(1.5), O(2.0), O(2.6), O(5.7)], [O(0.0), B(0.1, 50.0, 0), O(0.35), O(1.0)]],
         thetas=[[0.3, 0.5, 0.2], [6.0, 4.0, 1.5], [14.0, 12.0, 3.0], [20.0, 15.0, 8.0]],
         dopri5=dict(h_max=0.1, tol=0.05, thetas=[[0.3, 0.5, 0.2]]), checked=CK, adaptive=dict(dopri5=[], ros2=[])),
    # dx0 = -p0 x0 + rateiv0 + p2 (t - 3)^2, output x0 / p1: the stage times matter
    dict(name="custom_nonaut", scalable=False, model=model("custom_nonaut", 3, 1, 1), h_max=H,
         occasions=[[O(0.0), B(0.0, 100.0, 0), O(0.002), O(0.13), O(0.5), I(0.5, 60.0, 1.3, 0), O(1.0), B(1.0, 30.0, 0), O(1.5),
                     O(2.0), O(2.6), O(5.7)], [O(0.0), B(0.1, 50.0, 0), O(0.35), O(1.0)]],
         thetas=[[0.4, 2.0, 25.0], [10.0, 2.0, 25.0], [24.0, 2.0, 60.0], [36.0, 2.0, 300.0]],
         dopri5=dict(h_max=0.1, tol=0.05, thetas=[[0.4, 2.0, 25.0]]), checked=CK, adaptive=dict(dopri5=[], ros2=[])),
]


def fl(xs):
    return [float(v) for v in xs]


def kappa_of(w, pred_amount, order):
    lam = lambda_max(w.body, w.p)
    h = max(w.h_all)
    for hh in w.h_all:  # contractive: |R(h lambda)| <= 1 for the fastest rate at every step length used
        assert stability(order, -lam * mpf(hh)) <= 1, (w.body, w.theta, hh)
    return float(w.n_steps * mp.exp(lam * mpf(h)) * w.x_max / max(abs(v) for v in pred_amount)), float(lam * mpf(h))


def rel(a, b):
    scale = max(abs(v) for v in b)
    return float(max(abs(x - y) for x, y in zip(a, b)) / scale)


def build(group):
    g = {k: group[k] for k in ("name", "scalable", "model", "h_max", "occasions")}
    lagged = bool(group["model"]["lag"])
    nonaut = group["model"]["body"] == "custom_nonaut"
    cases, sharp, moved = [], 0, 0
    for th in group["thetas"]:
        pred, w, _ = walk_rk4(group, th)
        exact = walk_exact(group, th)
        kap, lam_h = kappa_of(w, [v * w.v for v in pred], 4)
        bar = 64 * U * kap
        assert bar <= 1e-11, (group["name"], th, kap)  # (a)
        sharp += rel(pred, exact) >= 1000 * bar
        if lagged:
            alt, _, _ = walk_rk4(group, th, recorded_breaks=True)
            moved += rel(alt, pred) >= 100 * bar
        if nonaut:
            frozen, _, _ = walk_rk4(group, th, freeze_t=True)
            assert rel(frozen, pred) >= 1000 * bar, (group["name"], th)  # (d)
        cases.append(dict(theta=fl(th), rk4=fl(pred), exact=fl(exact), n_steps=w.n_steps, kappa=kap, lambda_h=lam_h))
    assert 2 * sharp >= len(cases), (group["name"], sharp)  # (b)
    assert not lagged or moved >= 1, group["name"]  # (c)
    assert lam_h <= 2.05 and cases[-1]["lambda_h"] >= 1.7 and any(0.5 <= c["lambda_h"] <= 1.0 for c in cases), group["name"]
    g["cases"] = cases

    d = group["dopri5"]
    dcases = []
    for th in d["thetas"]:
        pred, w, worst = walk_dopri5(group, th, d["h_max"], d["tol"])
        assert worst <= 0.25, (group["name"], th, float(worst))
        kap, _ = kappa_of(w, [v * w.v for v in pred], 5)
        assert 64 * U * kap <= 1e-11
        dcases.append(dict(theta=fl(th), dopri5=fl(pred), n_steps=w.n_steps, kappa=kap, max_step_err=float(worst)))
    g["dopri5"] = dict(h_max=d["h_max"], rtol=d["tol"], atol=d["tol"], cases=dcases)

    ck = group["checked"]
    ccases = []
    for i, th in enumerate(group["thetas"]):
        _, _, qs = walk_rk4(group, th, probe=(ck["rtol"], ck["atol"]))
        q_max = max(q for q, _ in qs)
        fail = next((row for q, row in qs if not q <= 1), None)
        decisive = all(q <= 0.5 for q, _ in qs) or any(q >= 2 for q, _ in qs)
        # the first failing piece must itself be decisive, and no piece before it in the undecided band
        if fail is not None:
            first = next(k for k, (q, _) in enumerate(qs) if not q <= 1)
            decisive = qs[first][0] >= 2 and all(q <= 0.5 for q, _ in qs[:first])
        if decisive:
            ccases.append(dict(case=i, q_max=float(q_max), fail_row=fail))
    assert any(c["fail_row"] is None for c in ccases) and any(c["fail_row"] is not None for c in ccases), group["name"]
    g["checked"] = dict(rtol=ck["rtol"], atol=ck["atol"], cases=ccases)

    ad = {}
    for solver, thetas in group["adaptive"].items():
        ad[solver] = []
        for th in thetas:
            exact = walk_exact(group, th)
            ad[solver].append(dict(theta=fl(th), exact=fl(exact)))
    g["adaptive"] = dict(h_max=4.0, tols=[1e-6, 1e-9], **ad)
    return g


def main():
    doc = dict(generator="tests/golden/gen_ode_exact.py", dps=40, groups=[build(g) for g in GROUPS])
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    n = sum(len(g["cases"]) for g in doc["groups"])
    print(f"wrote {OUT}: {len(doc['groups'])} groups, {n} fixed-step cases, {os.path.getsize(OUT)} bytes")
    for g in doc["groups"]:
        print(g["name"], [(c["n_steps"], round(c["kappa"]), round(c["lambda_h"], 2)) for c in g["cases"]],
              [(c["case"], round(c["q_max"], 3), c["fail_row"]) for c in g["checked"]["cases"]],
              [round(c["max_step_err"], 3) for c in g["dopri5"]["cases"]])


if __name__ == "__main__":
    main()
