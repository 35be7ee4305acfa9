#!/usr/bin/env python3
"""Generate tests/golden/ode_exact_general.json: ROS2 and the auto solver on user bodies OUTSIDE the compartmental class.

The bodies are tests/general_ode_bodies.py's (C text and Python twin side by side): a growing state held stable by feedback
(2 states, and twice inside 8 states) and a predator-prey pair.  For none of them is W = I - gamma h J a column-diagonally-
dominant M-matrix, which every body of gen_ode_exact_stiff.py is.  The exact ROS2 and DOPRI5 steps, the switch walk, the
difference rule and the mutations are gen_ode_exact_stiff.py's, the walk with its partition rule is gen_ode_exact.py's,
imported; 40-digit mpmath; neither the oracle nor the product is imported.  Their `solve` exchanges rows, which in exact
arithmetic changes nothing: the fixture says what the STEP is, not how to eliminate.

Forced steps (`groups`).  One group per body, solver "ros2", tolerances 2.0, h_max 0.05, four cases; every step is
min(h_max, left) and its scaled error is asserted <= 0.25.  No step is near a singular leading minor: the pivots of
natural-order elimination, evaluated exactly, are asserted >= 1/8 in size (`min_pivot`), so these cases pin the METHOD on
such bodies whatever the elimination order - though in two cases of each feedback body a sub-diagonal entry is the larger
one, so an implementation that exchanges rows does so here.  lotka2's expected values include the truncation of the
documented difference quotient (the body is nonlinear), as one_cmt_mm's do.  `dopri5`: the same schedules walked by the
exact DOPRI5 step, with the switch rule's stiffness quotient asserted calm by a margin at every step that has one
(`walk_explicit`): what a lane of the auto solver returns here, with the counts (n_steps, 0, 0, 0).

Pivot ladder (`ladder`).  One group per feedback body; five cases = five rungs.  A bolus of 1024 recorded at t = 0 lands
at theta[lag]; the one observation is at t = 2; h_max = 2.  So the walk is: one step over [0, lag] on the zero state (which
stays zero), then ONE step of h = 2 - lag, formed in doubles as the device forms it (piece end minus landing time,
DESIGN.md "ODE step partition"), from the exact state (1024, 0, ...).  The lag of rung k is chosen so that
W[q][q] = 1 - gamma h a = 2^-k, k = 4, 12, 24, 36, 44, q the first state of the feedback pair (0 | 0 | 6; in
feedback8_tail that pivot is met at elimination stage 6, after six updates that leave it as it is).  a, b, c, kt, kd are
dyadic (1/2, 3, 5, 4, 1/4), so every function value entering that step's Jacobian quotients is exact in float64 and so
are their differences: asserted by evaluating the twin in Python doubles.  Rounding in the quotients therefore costs
nothing on these steps - the rule "an entry whose two function values are equal stays" of gen_ode_exact_stiff.py is
extended to "an entry whose difference is exact in float64 stays" (`difference_quotients` below), and `diff_noise` of
every ladder case is asserted 0.  The device's own float64 chain for the pivot entry - gh = kGamma h, s = -gh / d,
(f1 - f0) s + 1 - is emulated with and without a fused multiply-add; both results are asserted within a factor 2 of the
nominal rung and stored (`pivot`, `pivot_fma`).  W itself stays well conditioned (`cond`: 8 to 26, asserted <= 64).

kappa.  A step is one solve with W and a handful of sums: it perturbs by O(u) (4 + cond_1(W)) |x|, cond_1(W) =
||W||_1 ||W^-1||_1 MEASURED per step from the step's own W (the bound 1 + gamma h ||J||_1 of gen_ode_exact_stiff.py holds
for M-matrices only).  Later steps need not be contractive here, so the amplification is measured as well: `growth` = the
largest ||S_j ... S_k+1||_1 over all runs of consecutive steps, S = the derivative of the step map (a difference quotient
in 40-digit arithmetic).      kappa = n_steps (4 + max cond) growth max_k |x_k|_inf / max_obs |x_out|
A case's bar is max(64 u kappa, diff_noise) here; the tests add 8 err_oracle.

Conditions asserted (what makes the tests able to fail):
  * each wrong method of gen_ode_exact_stiff.py's MUTATIONS that applies moves some case of every group, forced and
    ladder, by >= 100 bar of that case;
  * a float64 restatement of the step (tests/general_ode_bodies.py `ros2_doubles`, no fused multiply-add) with
    natural-order elimination misses the 2^-36 and 2^-44 rungs by >= 100 bar (`natural_err`); the same restatement with
    row exchanges is inside every bar of every rung (`exchanged_err`).

Adaptive (`adaptive`).  lotka2 over two cycles with a bolus into the predator, feedback2 over ten time constants, solvers
"ros2" and "auto", rtol = atol = 1e-6, h_max 4.  `exact`: the 40-digit solution (mpmath.odefun per event-free stretch;
the matrix exponential for the linear body).  Adaptive step sequences depend on rounding, so no bar follows from a step
count: `oracle_err` is the error the CPU oracle achieves on that case and solver (largest error relative to the largest
value - feedback2's solutions swing through zero, where only the absolute part of a step's tolerance acts and a pointwise
relative error says nothing; the oracle has no auto mode and runs DOPRI5 there, which is what a lane that never switches
walks).  These are recorded measurements - ORACLE_ERR below, taken with tests/test_oracle_ode_general_exact.py, which
asserts that today's oracle reproduces each within a factor 2 and stays under 1e-4.  The device is held to 4 oracle_err
(another rounding of the step sequence) and to 1e-4 whatever the oracle does.

Run:  python tests/golden/gen_ode_exact_general.py      (deterministic; rewrites ode_exact_general.json byte for byte)
"""
import json
import os
import sys

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_ode_exact as base  # noqa: E402
import gen_ode_exact_stiff as stiff  # noqa: E402
from gen_ode_exact import B, I, O, U, Walk, fl, model, rel, walk_exact  # noqa: E402
from gen_ode_exact_stiff import DELTA, GAMMA, MUTATIONS, ros_step, scaled_norm, walk_ros2  # noqa: E402
from general_ode_bodies import BODIES as GENERAL, GAMMA_D, SQRT_EPS, ros2_doubles  # noqa: E402  (no product import)

mp.mp.dps = 40
mpf = mp.mpf
OUT = os.path.join(HERE, "ode_exact_general.json")
assert float(GAMMA) == GAMMA_D and float(DELTA) == SQRT_EPS

# ---------------------------------------------------------------------------------------- the bodies join the walkers
for _name, _b in GENERAL.items():
    base.BODIES[_name] = (_b["nstates"], _b["nparams"], _b["central"])
_matrix_of, _rate_vector, _rhs_of = base.matrix_of, base.rate_vector, base.rhs_of


def matrix_of(body, p):
    if body in GENERAL:
        return GENERAL[body]["jac"](None, p) if GENERAL[body]["linear"] else None
    return _matrix_of(body, p)


def rate_vector(body, r):
    if body in GENERAL:  # input i goes to state i
        return [r[i] if i < len(r) else mpf(0) for i in range(GENERAL[body]["nstates"])]
    return _rate_vector(body, r)


def rhs_of(body, p, r):
    """f(t, x) in mpf; `f.doubles(t, x)`: the same text in Python doubles (no fused multiply-add)."""
    if body not in GENERAL:
        return _rhs_of(body, p, r)
    rhs = GENERAL[body]["rhs"]
    pd, rd = [float(v) for v in p], [float(v) for v in r]

    def f(t, x):
        return rhs(t, x, p, r)

    f.doubles = lambda t, x: rhs(t, x, pd, rd)
    return f


# (the imported walkers look the bodies up in their own modules)
base.matrix_of, base.rate_vector, base.rhs_of, stiff.rhs_of = matrix_of, rate_vector, rhs_of, rhs_of


# ------------------------------------------------------------------------------------------------- the difference rule
def is_double(v):
    return mpf(float(v)) == v


def exact_in_float64(f, t, x, j, d, f0, f1):
    """Per component i: is (f1_i - f0_i) of column j what float64 arithmetic gives, bit for bit?  True where both function
    values, evaluated in doubles at arguments that are themselves doubles, equal the exact ones and their difference is a
    double.  j = None: the time quotient."""
    n = len(x)
    fd = getattr(f, "doubles", None)
    if fd is None or not (is_double(t) and all(is_double(v) for v in x) and is_double(d)):
        return [False] * n
    td, xd = float(t), [float(v) for v in x]
    if j is None:
        if mpf(td + float(d)) != t + d:
            return [False] * n
        g0, g1 = fd(td, xd), fd(td + float(d), xd)
    else:
        if mpf(xd[j] + float(d)) != x[j] + d:
            return [False] * n
        xt = list(xd)
        xt[j] = xd[j] + float(d)
        g0, g1 = fd(td, xd), fd(td, xt)
    return [mpf(g0[i]) == f0[i] and mpf(g1[i]) == f1[i] and mpf(g1[i] - g0[i]) == f1[i] - f0[i] for i in range(n)]


EXACT_LOG = []  # one entry per quotient evaluation of a shifted walk: were all its differences exact?


def difference_quotients(f, t, x, shift=0):
    """gen_ode_exact_stiff.py's rule, with its exemption widened: an entry whose difference is exact in float64 is moved
    by no rounding (equal function values are the special case of a zero difference)."""
    n = len(x)
    f0 = f(t, x)
    J = [[mpf(0)] * n for _ in range(n)]
    every = True
    for j in range(n):
        d = DELTA * max(abs(x[j]), 1)
        xt = list(x)
        xt[j] = x[j] + d
        f1 = f(t, xt)
        ex = exact_in_float64(f, t, x, j, d, f0, f1) if shift else [False] * n
        every = every and all(ex)
        for i in range(n):
            J[i][j] = (f1[i] - f0[i]) / d + (0 if ex[i] else stiff.noise(shift, f0[i], f1[i], d))
    dt = DELTA * max(abs(t), 1)
    f1 = f(t + dt, x)
    ex = exact_in_float64(f, t, x, None, dt, f0, f1) if shift else [False] * n
    every = every and all(ex)
    ft = [(f1[i] - f0[i]) / dt + (0 if ex[i] else stiff.noise(shift, f0[i], f1[i], dt)) for i in range(n)]
    if shift:
        EXACT_LOG.append(every)
    return f0, J, ft


stiff.difference_quotients = difference_quotients


# --------------------------------------------------------------------------------------------------------------- kappa
def norm1(A):
    n = len(A)
    return max(sum(abs(A[i][j]) for i in range(n)) for j in range(n))


def natural_pivots(W, exchange=False):
    """The pivots of elimination in the natural order, in exact arithmetic.  exchange: with row exchanges instead (a
    strictly larger entry below the diagonal comes up) -> has any stage exchanged?"""
    n = len(W)
    M = [list(r) for r in W]
    piv, moved = [], False
    for k in range(n):
        if exchange:
            top = max(range(k, n), key=lambda i: (abs(M[i][k]), -i))
            moved = moved or top != k
            M[k], M[top] = M[top], M[k]
        piv.append(M[k][k])
        for i in range(k + 1, n):
            l = M[i][k] / M[k][k]
            for j in range(k, n):
                M[i][j] -= l * M[k][j]
    return moved if exchange else piv


class Track:
    """What a forced walk records for kappa: cond_1(W) and the natural-order pivots per implicit step, the largest
    scaled error, and the largest norm of a product of consecutive step derivatives."""

    def __init__(self, linear):
        self.linear, self.cond, self.min_pivot, self.worst, self.growth = linear, mpf(1), mpf(1), mpf(0), 1.0
        self.exchange = False
        self._w, self._s, self._tails = {}, {}, []

    def implicit(self, J, h):
        key = (h,) if self.linear else None
        if key not in self._w:
            n = len(J)
            W = [[(1 if i == j else 0) - GAMMA * h * J[i][j] for j in range(n)] for i in range(n)]
            Wi = mp.inverse(mp.matrix(W))
            piv = natural_pivots(W)
            exch = natural_pivots(W, exchange=True)
            val = (norm1(W) * norm1([[Wi[i, j] for j in range(n)] for i in range(n)]), min(abs(v) for v in piv), exch)
            if key is None:
                self._note(val)
                return
            self._w[key] = val
        self._note(self._w[key])

    def _note(self, val):
        self.cond, self.min_pivot, self.exchange = max(self.cond, val[0]), min(self.min_pivot, val[1]), self.exchange or val[2]

    def step(self, step_fn, x, new, h, homogeneous=None):
        """step_fn(x) -> the step's result.  S = d new / d x by a difference quotient at 40 digits (exact for the linear
        bodies, whose S depends on h alone); then every product S_j ... S_k+1 that ends at this step, in doubles."""
        n = len(x)
        key = (h,) if self.linear else None
        S = self._s.get(key) if key else None
        if S is None:
            S = [[0.0] * n for _ in range(n)]
            for j in range(n):
                eps = mpf(10) ** -18 * max(abs(x[j]), 1)
                xt = list(x)
                xt[j] = x[j] + eps
                moved = step_fn(xt)
                for i in range(n):
                    S[i][j] = float((moved[i] - new[i]) / eps)
            if key:
                self._s[key] = S
        eye = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
        self._tails = [[[sum(S[i][k] * P[k][j] for k in range(n)) for j in range(n)] for i in range(n)] for P in self._tails + [eye]]
        self.growth = max([self.growth] + [float(norm1(P)) for P in self._tails])


def walk_tracked(group, theta, h_max, tol, shift=0, track=None):
    """gen_ode_exact_stiff.py's forced-step ROS2 walk (every step min(h_max, left), times in doubles), recording for
    `track`.  Returns (predictions, walk, [(t, x, h) of every step])."""
    w = Walk(group, theta)
    rtol = atol = mpf(tol)
    steps = []

    def piece(x, t0, t1, rates, row):
        f = rhs_of(w.body, w.p, rates)
        t = t0
        while t < t1:
            left = t1 - t
            h = min(h_max, left)
            new, e, J = ros_step(f, mpf(t), x, mpf(h), None, shift)
            steps.append((t, x, h, f))
            if track is not None:
                track.implicit(J, mpf(h))
                track.step(lambda xx: ros_step(f, mpf(t), xx, mpf(h))[0], x, new, h)
                track.worst = max(track.worst, scaled_norm(e, x, new, rtol, atol))
            x = new
            w.note(x, h)
            t = t1 if h == left else t + h
        return x

    return w.run(piece), w, steps


def walk_explicit(group, theta, h_max, tol, linear):
    """Forced-step DOPRI5 as a lane of the auto solver walks it, and why that lane stays explicit: per step the stiffness
    quotient h rho of gen_ode_exact_stiff.py's walk_auto.  A step whose denominator is exactly zero (the zero state before
    the first dose lands: f(0) = 0 in any arithmetic) moves no counter; a step with sqrt(den) >= 1e-6 max|x| must be calm
    by a margin, h rho <= 3.23; what is left are slivers at a piece end, where the quotient belongs to rounding: never more
    than two in a row, against the fifteen a switch takes.  Returns (predictions, walk, largest scaled error, growth,
    largest h ||J||_1)."""
    w = Walk(group, theta)
    rtol = atol = mpf(tol)
    tr = Track(linear)
    st = dict(worst=mpf(0), hj=mpf(0), loose=0)

    def piece(x, t0, t1, rates, row):
        f = rhs_of(w.body, w.p, rates)
        t = t0
        while t < t1:
            left = t1 - t
            h = min(h_max, left)
            hm = mpf(h)
            calls = []

            def rec(tt, xx):
                calls.append((xx, f(tt, xx)))
                return calls[-1][1]
            new, hat = base.erk_step(base.DP, rec, mpf(t), x, hm)
            st["worst"] = max(st["worst"], scaled_norm([a - b for a, b in zip(new, hat)], x, new, rtol, atol))
            (g6, k6), (_, k7) = calls[5], calls[6]
            num = sum((a - b) ** 2 for a, b in zip(k7, k6))
            den = sum((a - b) ** 2 for a, b in zip(new, g6))
            if den == 0 and all(v == 0 for v in list(x) + list(new)):
                pass
            elif den > 0 and mp.sqrt(den) >= mpf(10) ** -6 * max(abs(v) for v in list(x) + list(new)):
                assert hm * mp.sqrt(num / den) <= mpf("3.23"), (theta, t, float(hm * mp.sqrt(num / den)))
                st["loose"] = 0
            else:
                st["loose"] += 1
                assert st["loose"] <= 2, (theta, t)
            tr.step(lambda xx: base.erk_step(base.DP, f, mpf(t), xx, hm)[0], x, new, h)
            st["hj"] = max(st["hj"], hm * norm1(GENERAL[w.body]["jac"](x, w.p)))
            x = new
            w.note(x, h)
            t = t1 if h == left else t + h
        return x

    pred = w.run(piece)
    return pred, w, st["worst"], tr.growth, st["hj"]


def kappa_of(w, pred, per_step, growth):
    return float(w.n_steps * per_step * growth * w.x_max / max(abs(v * w.v) for v in pred))


def mutated(g, th, tol, m, pred):
    """How far wrong method m lands from `pred`; 1e300 where it breaks down (a walk that diverges until W is singular
    at 40 digits)."""
    try:
        return min(rel(walk_ros2(g, th, g["h_max"], tol, mutation=m)[0], pred), 1e300)
    except ZeroDivisionError:
        return 1e300


def applicable(body):
    multi = GENERAL[body]["nstates"] > 1
    return [m for m, where in MUTATIONS.items() if where is None or where == body or (where == "multi" and multi)]


def model_of(body):
    b = GENERAL[body]
    return model(body, b["nparams"], b["v"], b["ndrugs"], init=b["init"], lag=b["lag"])


# ------------------------------------------------------------------------------------------------------- forced steps
H = 0.05
TOL = 2.0
FEEDBACK_SCHEDULE = [[O(0.0), B(0.0, 100.0, 0), O(0.3), O(0.5), I(0.5, 60.0, 0.8, 0), O(1.0), B(1.03, 40.0, 0), O(1.5), O(2.0),
                      O(2.6)], [O(0.0), B(0.1, 50.0, 0), O(0.6), O(1.0)]]
LOTKA_SCHEDULE = [[O(0.0), O(0.002), O(0.13), O(0.5), B(0.5, 4.0, 1), O(0.502), O(1.0), I(1.0, 3.0, 0.7, 0), O(1.5), O(2.0),
                   O(2.6)], [O(0.0), B(0.1, 6.0, 1), B(0.1, 10.0, 0), O(0.35), O(1.0)]]
GROUPS = [
    # theta = [a, b, c, v, lag]; W[0][0] = 1 - gamma h a; in the last two a sub-diagonal entry is the larger one
    dict(name="feedback2", scalable=True, occasions=FEEDBACK_SCHEDULE,
         thetas=[[0.5, 2.0, 3.0, 8.0, 0.26], [2.0, 6.0, 5.0, 8.0, 0.26], [4.0, 12.0, 10.0, 8.0, 0.31], [5.0, 10.0, 7.0, 8.0, 0.26]]),
    # theta = [a, b, c, v, lag, kt, kd]
    dict(name="feedback8_head", scalable=True, occasions=FEEDBACK_SCHEDULE,
         thetas=[[0.5, 2.0, 3.0, 8.0, 0.26, 6.0, 0.5], [2.0, 6.0, 5.0, 8.0, 0.26, 8.0, 0.25], [4.0, 12.0, 10.0, 8.0, 0.31, 10.0, 0.5],
                 [5.0, 10.0, 7.0, 8.0, 0.26, 8.0, 1.0]]),
    dict(name="feedback8_tail", scalable=True, occasions=FEEDBACK_SCHEDULE,
         thetas=[[0.5, 2.0, 3.0, 8.0, 0.26, 6.0, 0.5], [2.0, 6.0, 5.0, 8.0, 0.26, 8.0, 0.25], [4.0, 12.0, 10.0, 8.0, 0.31, 10.0, 0.5],
                 [5.0, 10.0, 7.0, 8.0, 0.26, 8.0, 1.0]]),
    # theta = [g, k, e, d, v, x0(0), x1(0)]
    dict(name="lotka2", scalable=False, occasions=LOTKA_SCHEDULE,
         thetas=[[1.0, 0.1, 0.5, 0.8, 2.0, 20.0, 5.0], [4.0, 0.5, 0.25, 3.0, 2.0, 30.0, 6.0], [10.0, 0.8, 0.5, 6.0, 2.0, 12.0, 9.0],
                 [6.0, 1.0, 0.125, 2.0, 2.0, 16.0, 5.0]]),
]


def build(spec):
    body = spec.get("body", spec["name"])
    g = dict(name=spec["name"], scalable=spec["scalable"], model=model_of(body), h_max=spec.get("h_max", H),
             occasions=spec["occasions"])
    g["rtol"] = g["atol"] = tol = TOL
    linear = GENERAL[body]["linear"]
    applies = applicable(body)
    cases, moved = [], {m: [] for m in applies}
    for th in spec["thetas"]:
        tr = Track(linear)
        pred, w, _ = walk_tracked(g, th, g["h_max"], tol, track=tr)
        assert tr.worst <= 0.25, (g["name"], th, float(tr.worst))
        assert tr.min_pivot >= 0.125, (g["name"], th, float(tr.min_pivot))  # no step near a singular leading minor
        assert rel(walk_ros2(g, th, g["h_max"], tol)[0], pred) == 0  # (the imported walk walks the same)
        kappa = kappa_of(w, pred, 4 + tr.cond, tr.growth)
        noise = max(rel(walk_tracked(g, th, g["h_max"], tol, shift=s)[0], pred) for s in (1, -1))
        for m in applies:
            moved[m].append(mutated(g, th, tol, m, pred))
        case = dict(theta=fl(th), ros2=fl(pred), n_steps=w.n_steps, kappa=kappa, cond=float(tr.cond), growth=tr.growth,
                    min_pivot=float(tr.min_pivot), exchange=tr.exchange, max_step_err=float(tr.worst), diff_noise=noise)
        cases.append(case)
    bars = [max(64 * U * c["kappa"], c["diff_noise"]) for c in cases]
    for m in applies:  # at least one case moves by >= 100 x its bar
        assert any(d >= 100 * b for d, b in zip(moved[m], bars)), (g["name"], m, moved[m], bars)
    if body.startswith("feedback"):
        assert [c["exchange"] for c in cases] == [False, False, True, True], g["name"]
    g["cases"], g["mutations"] = cases, moved

    # what a lane of the auto solver that never switches returns: forced DOPRI5, and the rule keeps it explicit
    dcases = []
    for th in spec["thetas"]:
        pred, w, worst, growth, hj = walk_explicit(g, th, g["h_max"], tol, linear)
        assert worst <= 0.25, (g["name"], th, float(worst))
        dcases.append(dict(theta=fl(th), dopri5=fl(pred), n_steps=w.n_steps, kappa=kappa_of(w, pred, mp.exp(hj), growth),
                           max_step_err=float(worst), counts=[w.n_steps, 0, 0, 0]))
        assert 64 * U * dcases[-1]["kappa"] <= 1e-9
    g["dopri5"] = dict(h_max=g["h_max"], rtol=tol, atol=tol, cases=dcases)
    return g


# -------------------------------------------------------------------------------------------------------- pivot ladder
RUNGS = (4, 12, 24, 36, 44)
DOSE = 1024.0
T_OBS = 2.0
LADDER = [dict(name="feedback2_ladder", body="feedback2", q=0, tail=[]),
          dict(name="feedback8_head_ladder", body="feedback8_head", q=0, tail=[4.0, 0.25]),
          dict(name="feedback8_tail_ladder", body="feedback8_tail", q=6, tail=[4.0, 0.25])]
A_, B_, C_, V_ = 0.5, 3.0, 5.0, 8.0


def fma(a, b, c):
    return float(mpf(a) * mpf(b) + mpf(c))


def build_ladder(spec):
    body, q = spec["body"], spec["q"]
    g = dict(name=spec["name"], scalable=False, model=model_of(body), h_max=T_OBS,
             occasions=[[O(0.0), B(0.0, DOSE, 0), O(T_OBS)]])
    g["rtol"] = g["atol"] = tol = TOL
    applies = applicable(body)
    cases, moved = [], {m: [] for m in applies}
    for k in RUNGS:
        h_want = (2.0 - 2.0 ** (1 - k)) / GAMMA_D / (2.0 * A_)  # gamma h a = 1 - 2^-k, in doubles
        th = [A_, B_, C_, V_, T_OBS - h_want] + spec["tail"]
        tr = Track(True)
        pred, w, steps = walk_tracked(g, th, g["h_max"], tol, track=tr)
        assert tr.worst <= 0.25, (g["name"], k, float(tr.worst))
        (t0, x0, h0, _), (t1, x1, h1, f) = steps  # the step over the zero state, then THE step
        assert all(v == 0 for v in x0) and h1 == T_OBS - (0.0 + th[4]) and x1[0] == DOSE and all(v == 0 for v in x1[1:])
        # the differences of that step's quotients are exact in float64, so rounding costs them nothing
        del EXACT_LOG[:]
        noise = max(rel(walk_tracked(g, th, g["h_max"], tol, shift=s)[0], pred) for s in (1, -1))
        assert EXACT_LOG and all(EXACT_LOG) and noise == 0, (g["name"], k, EXACT_LOG, noise)
        # the device's own float64 chain for W[q][q]
        xd = [float(v) for v in x1]
        gh = GAMMA_D * h1
        d = SQRT_EPS * max(abs(xd[q]), 1.0)
        s = -gh / d
        xt = list(xd)
        xt[q] = xd[q] + d
        df = f.doubles(t1, xt)[q] - f.doubles(t1, xd)[q]
        pivot, pivot_fma = df * s + 1.0, fma(df, s, 1.0)
        nominal = 2.0 ** -k
        assert nominal / 2 <= pivot <= nominal * 2 and nominal / 2 <= pivot_fma <= nominal * 2, (g["name"], k, pivot, pivot_fma)
        # ... and natural-order elimination meets it at stage q (exact arithmetic: the six updates before it add nothing)
        J = GENERAL[body]["jac"](None, w.p)
        n = len(J)
        W = [[(1 if i == j else 0) - GAMMA * mpf(h1) * J[i][j] for j in range(n)] for i in range(n)]
        piv = natural_pivots(W)
        assert nominal / 2 <= piv[q] <= nominal * 2 and all(abs(v) >= 0.125 for i, v in enumerate(piv) if i != q and i != q + 1)
        assert tr.cond <= 64, (g["name"], k, float(tr.cond))  # W itself is well conditioned
        kappa = kappa_of(w, pred, 4 + tr.cond, tr.growth)
        bar = 64 * U * kappa
        # float64 restatements of the step: natural order, and with row exchanges
        errs = {}
        for exchange in (False, True):
            xn, err = ros2_doubles(f.doubles, t1, xd, h1, tol, exchange)
            got = xn[GENERAL[body]["central"]] / th[3]
            errs[exchange] = float(abs(mpf(got) - pred[-1]) / max(abs(v) for v in pred))
        assert errs[True] <= bar, (g["name"], k, errs, bar)
        assert k < 36 or errs[False] >= 100 * bar, (g["name"], k, errs, bar)
        for m in applies:
            moved[m].append(mutated(g, th, tol, m, pred))
        cases.append(dict(theta=fl(th), ros2=fl(pred), n_steps=w.n_steps, rung=k, h=h1, pivot=pivot, pivot_fma=pivot_fma,
                          kappa=kappa, cond=float(tr.cond), growth=tr.growth, max_step_err=float(tr.worst), diff_noise=noise,
                          natural_err=errs[False], exchanged_err=errs[True]))
    bars = [64 * U * c["kappa"] for c in cases]
    for m in applies:
        assert any(dv >= 100 * b for dv, b in zip(moved[m], bars)), (g["name"], m, moved[m], bars)
    g["cases"], g["mutations"] = cases, moved
    return g


# ------------------------------------------------------------------------------------------------------------ adaptive
# The error the CPU oracle achieves per (group, solver, case): recorded measurements, see the module's docstring.
ORACLE_ERR = {
    ("lotka2", "ros2"): [4.96e-06, 3.08e-06],
    ("lotka2", "auto"): [7.44e-07, 1.38e-06],
    ("feedback2", "ros2"): [1.66e-06, 2.38e-06],
    ("feedback2", "auto"): [2.21e-07, 7.59e-07],
}
ADAPTIVE = [
    # two cycles (period about 2 pi / sqrt(g d) = 7), a bolus into the predator in between
    dict(name="lotka2", scalable=False,
         occasions=[[O(0.0), O(0.5), O(1.5), O(3.0), O(4.5), O(6.0), B(6.0, 4.0, 1), O(6.5), O(8.0), O(10.0), O(12.0), O(14.0)]],
         thetas=[[1.0, 0.1, 0.5, 0.8, 2.0, 20.0, 5.0], [1.5, 0.25, 0.5, 1.0, 2.0, 10.0, 2.0]]),
    # ten time constants of the slower pair (real part -1.25), then of the faster (-2, oscillating at 9 /h)
    dict(name="feedback2", scalable=True,
         occasions=[[O(0.0), B(0.0, 100.0, 0), O(0.3), O(0.6), O(1.0), O(1.5), O(2.0), O(3.0), B(3.0, 50.0, 0), O(3.5), O(4.0),
                     O(5.0), O(6.5), O(8.0)]],
         thetas=[[0.5, 2.0, 3.0, 8.0, 0.25], [2.0, 10.0, 6.0, 8.0, 0.25]]),
]


def lotka_exact(group, theta):
    """mpmath.odefun (Taylor series at working precision) over every event-free stretch."""
    w = Walk(group, theta)

    def piece(x, t0, t1, rates, row):
        f = rhs_of(w.body, w.p, rates)
        sol = mp.odefun(lambda t, y: f(t, y), mpf(t0), list(x))
        return list(sol(mpf(t1)))

    return w.run(piece)


def build_adaptive(spec):
    body = spec["name"]
    g = dict(name=spec["name"], scalable=spec["scalable"], model=model_of(body), h_max=4.0, occasions=spec["occasions"])
    g["rtol"] = g["atol"] = 1e-6
    cases = []
    for c, th in enumerate(spec["thetas"]):
        exact = walk_exact(g, th) if GENERAL[body]["linear"] else lotka_exact(g, th)
        cases.append(dict(theta=fl(th), exact=fl(exact),
                          oracle_err={s: ORACLE_ERR[(body, s)][c] for s in ("ros2", "auto")}))
    g["cases"] = cases
    return g


def main():
    doc = dict(generator="tests/golden/gen_ode_exact_general.py", dps=40, groups=[build(g) for g in GROUPS],
               ladder=[build_ladder(g) for g in LADDER], adaptive=[build_adaptive(g) for g in ADAPTIVE])
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 256 << 10
    for g in doc["groups"] + doc["ladder"]:
        print(g["name"])
        for c in g["cases"]:
            bar = max(64 * U * c["kappa"], c["diff_noise"])
            extra = (f"  rung 2^-{c['rung']} pivot {c['pivot']:.3e} natural/bar {c['natural_err'] / bar:.3g} exchanged/bar "
                     f"{c['exchanged_err'] / bar:.3g}") if "rung" in c else f"  min pivot {c['min_pivot']:.3f} exchange {c['exchange']}"
            print(f"  steps {c['n_steps']}  err {c['max_step_err']:.3f}  cond {c['cond']:.3g}  growth {c['growth']:.3g}  kappa "
                  f"{c['kappa']:.3g}  diff_noise {c['diff_noise']:.2e}  bar {bar:.2e}{extra}")
        for m, d in g["mutations"].items():
            best = max(dv / max(64 * U * c["kappa"], c["diff_noise"]) for dv, c in zip(d, g["cases"]))
            print(f"  {m:22s} moved / bar, best case {best:.3g}")
        for c in g.get("dopri5", {}).get("cases", []):
            print(f"  dopri5 steps {c['n_steps']}  err {c['max_step_err']:.3f}  kappa {c['kappa']:.3g}")
    for g in doc["adaptive"]:
        for c in g["cases"]:
            print(g["name"], c["theta"], c["oracle_err"])


if __name__ == "__main__":
    main()
