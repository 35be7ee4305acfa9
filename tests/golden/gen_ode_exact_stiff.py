#!/usr/bin/env python3
"""Generate tests/golden/ode_exact_stiff.json: what ROS2 and the auto solver must return, to rounding.

A ROS2 step that the controller accepts at full length is a finite sequence of rational operations (one linear solve
included), so its result can be evaluated exactly: here in mpmath at 40 digits, from the published scheme (Verwer, Spee,
Blom, Hundsdorfer 1999, gamma = 1 + 1/sqrt(2)) and the rule of DESIGN.md's "Stiff option" - without the oracle and without
the device code.  Walk (with the partition rule), the groups' schedules and settings, the bodies, the explicit step and the
true solutions are gen_ode_exact.py's, imported.

    W = I - gamma h J
    W k1 = f(t, y) + gamma h f_t
    W k2 = f(t + h, y + h k1) - gamma h f_t - 2 k1
    y+ = y + 3/2 h k1 + 1/2 h k2,        e = h/2 (k1 + k2),     err = rms(e_i / (atol + rtol max(|y_i|, |y+_i|)))

The documented difference rule is part of the method and is evaluated in exact arithmetic: column j of J is
(f(y + d_j e_j) - f(y)) / d_j with d_j = 2^-26 max(|y_j|, 1); f_t = (f(t + d_t) - f(t)) / d_t, d_t = 2^-26 max(|t|, 1).
Exact for the linear bodies; for Michaelis-Menten and the non-autonomous body the truncation error of the quotient belongs
to the expected value.

Forced steps: with loose tolerances and a small h_max every step is min(h_max, left); ROS2 keeps its proposal while
0.9 err^(-1/2) >= 1 (err <= 0.81), asserted err <= 0.25 here, so rounding cannot change the step sequence.

Stored per case: `ros2`, `exact` (the true solution), `n_steps`, `max_step_err`, `lambda_h`, and
  kappa = n_steps (4 + cond) max_k |x_k|_inf / max_obs |x_out|,   cond = max over steps of 1 + gamma h ||J||_1:
    a first-order bound on accumulated rounding.  A step is one solve with W and a handful of sums; elimination in the
    natural order on a column-diagonally-dominant M-matrix has no growth, so a step perturbs by O(u) cond_1(W) |x| with
    cond_1(W) <= ||W||_1 ||W^-1||_1 <= 1 + gamma h ||J||_1, plus the four sums of the stage formulas; later steps are
    contractive (|R(z)| <= 1 at every eigenvalue and step length, asserted).  The bound is valid for THIS file's bodies:
    each is a compartmental M-matrix, Michaelis-Menten or the one-state non-autonomous body, none with growth.  A body
    with a growing state, feedback or a predator-prey term obeys neither ||W^-1||_1 <= 1 nor the contraction, and the
    natural order is not stable for it: gen_ode_exact_general.py measures cond_1(W) and the amplification per step there.
  diff_noise: what rounding in the difference quotients costs, which no double-precision implementation avoids: two more
    exact walks with every J entry shifted by +/- 4u max(|f0_i|, |f1_i|) / d_j and f_t likewise (an entry whose two
    function values are equal stays: that difference is exact in any arithmetic); the larger deviation.
A case's bar is max(64 u kappa, diff_noise) here (the tests add 8 err_oracle).

Conditions asserted (what makes the test able to fail): for each wrong method of MUTATIONS a second exact walk; at least
one case of every group it applies to moves by >= 100 bar of that case.

Auto section: a deterministic switch walked by the exact DOPRI5 and ROS2 steps under the documented rule (DESIGN.md,
"Auto solver"): h rho > 3.25 fifteen times in a row -> implicit, six calm steps forget the count, six implicit steps in a
row with h ||J||_inf <= 1 -> explicit, a switch zeroes the counters.  One state: rho = |lambda| exactly; h_max lambda =
3.28, inside DOPRI5's stability interval and 1 % over the threshold.  Asserted per accepted step: |h rho - 3.25| >= 0.02,
|h ||J|| - 1| >= 0.2, |xn - g6| >= 1e-6 max|x|, scaled error <= 0.25.

Run:  python tests/golden/gen_ode_exact_stiff.py      (deterministic; rewrites ode_exact_stiff.json byte for byte)
"""
import json
import os
import sys

import mpmath as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_ode_exact as base  # noqa: E402
from gen_ode_exact import (DP, GROUPS as BASE_GROUPS, B, I, O, U, Walk, erk_step, fl, matrix_of as base_matrix_of,  # noqa: E402
                           model, rate_vector as base_rate_vector, rel, rhs_of, stability, walk_exact)

mp.mp.dps = 40
mpf = mp.mpf
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ode_exact_stiff.json")
GAMMA = 1 + 1 / mp.sqrt(2)
DELTA = mpf(2) ** -26

# ------------------------------------------------------------------------------------------------------------- bodies
# custom_chain8: a catenary chain of 8 compartments, theta = [ke, kf, kr, v]; compartment i passes kf (1 + i/4) x_i on
# to i + 1 and gets kr (1 + i/2) x_{i+1} back; elimination ke from the first, which also takes the doses; output
# x_3 / v.  Tridiagonal, column sums (-ke, 0, ..., 0): column-diagonally dominant.
CHAIN = 8
base.BODIES["custom_chain8"] = (CHAIN, 4, 3)


def matrix_of(body, p):
    if body != "custom_chain8":
        return base_matrix_of(body, p)
    A = [[mpf(0)] * CHAIN for _ in range(CHAIN)]
    A[0][0] -= p[0]
    for i in range(CHAIN - 1):
        kf, kr = p[1] * (1 + mpf(i) / 4), p[2] * (1 + mpf(i) / 2)
        A[i][i] -= kf
        A[i + 1][i] += kf
        A[i + 1][i + 1] -= kr
        A[i][i + 1] += kr
    return A


def rate_vector(body, r):
    if body != "custom_chain8":
        return base_rate_vector(body, r)
    return [r[0]] + [mpf(0)] * (CHAIN - 1)


# the imported walkers look the bodies up in their own module
base.matrix_of, base.rate_vector = matrix_of, rate_vector
# (rhs_of and walk_exact read the two hooks above for a linear body; Walk.run applies the partition rule, `rewrite`)


def jacobian_exact(body, p, x):
    """df/dx of the body itself (for kappa and the contraction check only; the method uses the quotient)."""
    if body == "one_cmt_mm":
        vmax, km, v = p[:3]
        return [[-vmax * km / (v * (km + x[0] / v) ** 2)]]
    return matrix_of(body, p)


# ------------------------------------------------------------------------------------------------------------ the step
def solve(W, b):
    """W y = b by elimination with row exchanges (exact arithmetic: the solve is the solve)."""
    n = len(b)
    M = [list(W[i]) + [b[i]] for i in range(n)]
    for k in range(n):
        piv = max(range(k, n), key=lambda i: abs(M[i][k]))
        M[k], M[piv] = M[piv], M[k]
        for i in range(k + 1, n):
            l = M[i][k] / M[k][k]
            if l != 0:
                for j in range(k, n + 1):
                    M[i][j] -= l * M[k][j]
    y = [mpf(0)] * n
    for i in range(n - 1, -1, -1):
        y[i] = (M[i][n] - sum((M[i][j] * y[j] for j in range(i + 1, n)), mpf(0))) / M[i][i]
    return y


# the wrong methods a test must be able to tell from the right one -> the bodies each applies to (None: all)
MUTATIONS = {"gamma_other_root": None, "jacobian_dropped": None, "jacobian_transposed": "multi", "no_minus_2k1": None,
             "weights_swapped": None, "stage2_at_t": "custom_nonaut", "ft_dropped": "custom_nonaut",
             "ft_same_sign": "custom_nonaut", "jacobian_frozen": "one_cmt_mm"}


def noise(shift, f0, f1, d):
    """What rounding can move a quotient by: 4u max(|f0|, |f1|) / d - and nothing where the two values are equal (a
    component that does not depend on the moved argument is evaluated twice to the same bits; their difference is 0)."""
    return shift * 4 * U * max(abs(f0), abs(f1)) / d if shift and f1 != f0 else 0


def difference_quotients(f, t, x, shift=0):
    """(f0, J, f_t) by the documented rule; shift = +1 | -1: every entry moved by `noise`."""
    n = len(x)
    f0 = f(t, x)
    J = [[mpf(0)] * n for _ in range(n)]
    for j in range(n):
        d = DELTA * max(abs(x[j]), 1)
        xt = list(x)
        xt[j] = x[j] + d
        f1 = f(t, xt)
        for i in range(n):
            J[i][j] = (f1[i] - f0[i]) / d + noise(shift, f0[i], f1[i], d)
    dt = DELTA * max(abs(t), 1)
    f1 = f(t + dt, x)
    ft = [(f1[i] - f0[i]) / dt + noise(shift, f0[i], f1[i], dt) for i in range(n)]
    return f0, J, ft


def ros_step(f, t, x, h, mutation=None, shift=0, frozen=None):
    """One ROS2 step; returns (y+, e, J).  `frozen`: a Jacobian to use instead of this step's (mutation only)."""
    n = len(x)
    gamma = 1 - 1 / mp.sqrt(2) if mutation == "gamma_other_root" else GAMMA
    f0, J, ft = difference_quotients(f, t, x, shift)
    if frozen is not None:
        J = frozen
    if mutation == "jacobian_transposed":
        J = [[J[j][i] for j in range(n)] for i in range(n)]
    if mutation == "ft_dropped":
        ft = [mpf(0)] * n
    gh = gamma * h
    W = [[(1 if i == j else 0) - (0 if mutation == "jacobian_dropped" else gh * J[i][j]) for j in range(n)] for i in range(n)]
    k1 = solve(W, [f0[i] + gh * ft[i] for i in range(n)])
    f1 = f(t if mutation == "stage2_at_t" else t + h, [x[i] + h * k1[i] for i in range(n)])
    s2 = 1 if mutation == "ft_same_sign" else -1
    m2 = 0 if mutation == "no_minus_2k1" else 2
    k2 = solve(W, [f1[i] + s2 * gh * ft[i] - m2 * k1[i] for i in range(n)])
    b1, b2 = (mpf(1) / 2, mpf(3) / 2) if mutation == "weights_swapped" else (mpf(3) / 2, mpf(1) / 2)
    new = [x[i] + h * (b1 * k1[i] + b2 * k2[i]) for i in range(n)]
    e = [h / 2 * (k1[i] + k2[i]) for i in range(n)]
    return new, e, J


def scaled_norm(e, x, new, rtol, atol):
    q = [ei / (atol + rtol * max(abs(a), abs(b))) for ei, a, b in zip(e, x, new)]
    return mp.sqrt(sum(v * v for v in q) / len(q))


def ros2_R(z):
    """Stability function of ROS2 (the z^2 coefficient gamma^2 - 2 gamma + 1/2 vanishes at this gamma: L-stable)."""
    return abs((1 + (1 - 2 * GAMMA) * z + (GAMMA * GAMMA - 2 * GAMMA + mpf(1) / 2) * z * z) / (1 - GAMMA * z) ** 2)


def spectrum(A):
    ev = mp.eig(mp.matrix(A), left=False, right=False)
    ev = list(ev[0]) if isinstance(ev, tuple) else list(ev)
    assert all(abs(mp.im(e)) < mpf(10) ** -25 and mp.re(e) <= mpf(10) ** -25 for e in ev), ev
    return [mp.re(e) for e in ev]


def norm1(A):
    return max(sum(abs(A[i][j]) for i in range(len(A))) for j in range(len(A)))


def norm_inf(A):
    return max(sum(abs(v) for v in row) for row in A)


class Track:
    """What a walk records for kappa: the largest cond bound, the largest scaled error, contraction at every step."""

    def __init__(self):
        self.cond, self.worst, self.lam_h = mpf(1), mpf(0), mpf(0)
        self._seen = {}

    def step(self, w, x, h):
        A = jacobian_exact(w.body, w.p, x)
        key = (h, None if w.body != "one_cmt_mm" else x[0])
        if key not in self._seen:
            ev = spectrum(A)
            for lam in ev:  # contractive: |R(h lambda)| <= 1 at every eigenvalue and step length used
                assert ros2_R(mpf(h) * lam) <= 1, (w.body, w.theta, h)
            self._seen[key] = (max(abs(lam) for lam in ev) * mpf(h), 1 + GAMMA * mpf(h) * norm1(A))
        lam_h, cond = self._seen[key]
        self.lam_h, self.cond = max(self.lam_h, lam_h), max(self.cond, cond)


def walk_ros2(group, theta, h_max, tol, mutation=None, shift=0, track=None):
    """Forced-step ROS2: every step min(h_max, left), times in doubles as the controller holds them."""
    w = Walk(group, theta)
    rtol = atol = mpf(tol)

    def piece(x, t0, t1, rates, row):
        f = rhs_of(w.body, w.p, rates)
        t, frozen = t0, None
        while t < t1:
            left = t1 - t
            h = min(h_max, left)
            new, e, J = ros_step(f, mpf(t), x, mpf(h), mutation, shift, frozen)
            if mutation == "jacobian_frozen" and frozen is None:
                frozen = J
            if track is not None:
                track.step(w, x, h)
                track.worst = max(track.worst, scaled_norm(e, x, new, rtol, atol))
            x = new
            w.note(x, h)
            t = t1 if h == left else t + h
        return x

    return w.run(piece), w


# ------------------------------------------------------------------------------------------------------------- groups
def from_base(name):
    return next(g for g in BASE_GROUPS if g["name"] == name)


H = 0.05
CHAIN_SCHEDULE = [[O(0.0), B(0.0, 100.0, 0), O(0.002), O(0.13), O(0.5), I(0.5, 60.0, 1.3, 0), O(1.0), B(1.0, 30.0, 0), O(1.5),
                   O(2.0), O(2.6), O(5.7)], [O(0.0), B(0.1, 50.0, 0), O(0.35), I(0.35, 20.0, 0.4, 0), O(1.0)]]
# thetas: easy (h lambda < 0.1), near 1, and two no explicit method could step through (about 50 and about 1000)
GROUPS = [
    # theta = [ka, ke, v, lag0, fa0]
    dict(base="one_cmt_oral_lag_fa", tol=2.0,
         thetas=[[1.1, 0.3, 20.0, 0.26, 0.8], [20.0, 0.9, 20.0, 0.26, 0.8], [1000.0, 2.0, 15.0, 0.26, 0.65],
                 [20000.0, 0.4, 15.0, 0.31, 1.0]]),
    # theta = [ke, ka, kcp, kpc, v, lag0, lag1, fa0]; the first hard case is fast in the distribution, not the absorption
    dict(base="two_cmt_oral_two_lags", tol=2.0,
         thetas=[[0.25, 1.3, 0.4, 0.2, 30.0, 0.26, -0.3, 0.9], [1.0, 20.0, 2.0, 1.0, 30.0, 0.26, -0.3, 0.9],
                 [3.0, 28.0, 700.0, 250.0, 12.0, 0.26, -0.3, 0.7], [2.0, 20000.0, 1.0, 0.5, 12.0, 0.37, -0.3, 1.0]]),
    # theta = [ka, k10, k12, k13, k21, k31, v]
    dict(base="three_cmt_oral", tol=2.0,
         thetas=[[0.9, 0.15, 0.4, 0.2, 0.3, 0.1, 40.0], [20.0, 1.0, 1.0, 0.5, 0.6, 0.2, 40.0],
                 [26.0, 2.0, 600.0, 1.0, 350.0, 0.4, 18.0], [20000.0, 0.5, 0.8, 0.3, 0.5, 0.2, 18.0]]),
    # theta = [vmax, km, v]: lambda = vmax / (v km) at x = 0; the Jacobian changes every step
    dict(base="one_cmt_mm", tol=2.0,
         thetas=[[8.0, 4.0, 10.0], [30.0, 0.15, 10.0], [50.0, 0.005, 10.0], [40.0, 0.0002, 10.0]]),
    # theta = [k, v, c2]: dx = -k x + rateiv + c2 (t - 3)^2: the f_t term
    dict(base="custom_nonaut", tol=2.0,
         thetas=[[0.4, 2.0, 25.0], [20.0, 2.0, 25.0], [1000.0, 2.0, 3000.0], [20000.0, 2.0, 60000.0]]),
    # theta = [ke, kf, kr, v]
    dict(name="custom_chain8", scalable=True, model=model("custom_chain8", 4, 3, 1), h_max=H, occasions=CHAIN_SCHEDULE, tol=2.0,
         thetas=[[0.2, 0.25, 0.15, 8.0], [1.0, 3.0, 2.0, 8.0], [0.5, 160.0, 90.0, 8.0], [2.0, 3000.0, 1800.0, 8.0]]),
]
LAMBDA_H = [(0.0, 0.1), (0.5, 2.0), (25.0, 100.0), (500.0, 2000.0)]


def build(spec):
    group = dict(from_base(spec["base"])) if "base" in spec else dict(spec)
    g = {k: group[k] for k in ("name", "scalable", "model", "h_max", "occasions")}
    body, multi = g["model"]["body"], base.BODIES[g["model"]["body"]][0] > 1
    g["rtol"] = g["atol"] = tol = spec["tol"]
    h_max = g["h_max"]
    applies = [m for m, where in MUTATIONS.items() if where is None or where == body or (where == "multi" and multi)]
    cases, moved = [], {m: [] for m in applies}
    for th, (lo, hi) in zip(spec["thetas"], LAMBDA_H):
        tr = Track()
        pred, w = walk_ros2(g, th, h_max, tol, track=tr)
        assert tr.worst <= 0.25, (g["name"], th, float(tr.worst))
        assert lo <= tr.lam_h <= hi, (g["name"], th, float(tr.lam_h))
        amount = [v * w.v for v in pred]
        kappa = float(w.n_steps * (4 + tr.cond) * w.x_max / max(abs(v) for v in amount))
        noise = max(rel(walk_ros2(g, th, h_max, tol, shift=s)[0], pred) for s in (1, -1))
        bar = max(64 * U * kappa, noise)
        for m in applies:
            moved[m].append(rel(walk_ros2(g, th, h_max, tol, mutation=m)[0], pred))
        cases.append(dict(theta=fl(th), ros2=fl(pred), exact=fl(walk_exact(g, th)), n_steps=w.n_steps, kappa=kappa,
                          lambda_h=float(tr.lam_h), max_step_err=float(tr.worst), diff_noise=noise, bar=bar))
    for m in applies:  # at least one case moves by >= 100 x its bar
        assert any(d >= 100 * c["bar"] for d, c in zip(moved[m], cases)), (g["name"], m, moved[m], [c["bar"] for c in cases])
    for c in cases:
        del c["bar"]
    g["cases"], g["mutations"] = cases, moved
    return g


# --------------------------------------------------------------------------------------------------------------- auto
STIFF_RHO, STIFF_STEPS, CALM_STEPS, BACK_RHO, BACK_STEPS = mpf("3.25"), 15, 6, mpf(1), 6
AH = 0.0625  # a power of two: the long gaps are whole numbers of steps, no sliver at a piece end


def auto_schedule(events):
    """A long first gap (26 steps), ten observations h_max / 5 apart, a long tail (30.5 steps); `events` ride on the
    raster inside the long gaps."""
    t_a = 26 * AH
    short = [O(round(t_a + k * AH / 5, 6)) for k in range(1, 11)]
    t_b = short[-1][1]
    return [sorted([O(0.0), O(t_a)] + short + [O(t_b + 30.5 * AH)] + events(t_b), key=lambda e: (e[1], base.RANK[e[0]]))]


AUTO_GROUPS = [
    # dx = -k x + rateiv + c2 (t - 3)^2: the forcing keeps the state moving and f_t live after the switch; a bolus every
    # other implicit step keeps f from cancelling to a small remainder of large terms, where the rounding of a difference
    # quotient is no longer bounded by 4u max(|f0|, |f1|) / d and `diff_noise` would understate it
    dict(name="custom_nonaut", scalable=False, model=model("custom_nonaut", 3, 1, 1), h_max=AH, tol=8.0,
         occasions=auto_schedule(lambda tb: [B(0.0, 100.0, 0), I(8 * AH, 60.0, 12 * AH, 0)]
                                 + [B(k * AH, 100.0 - 5 * k, 0) for k in (16, 18, 20, 22, 24)]
                                 + [B(tb + k * AH, 40.0 + 3 * k, 0) for k in (3, 10, 16, 18, 20, 22, 24, 26, 28)]),
         thetas=[[3.28 / AH, 2.0, 300.0], [1.0 / AH, 2.0, 300.0]]),
    # theta = [ke, v, x0(0)]: boluses keep the state off zero
    dict(name="one_cmt_iv_init", scalable=False, model=model("one_cmt_iv", 3, 1, 1, init={0: 2}), h_max=AH, tol=8.0,
         occasions=auto_schedule(lambda tb: [B(0.0, 20.0, 0), B(6 * AH, 50.0, 0), B(14 * AH, 80.0, 0), B(22 * AH, 40.0, 0),
                                             B(tb + 7 * AH, 70.0, 0), B(tb + 16 * AH, 30.0, 0), B(tb + 25 * AH, 60.0, 0)]),
         thetas=[[3.28 / AH, 12.0, 100.0], [1.0 / AH, 12.0, 100.0]]),
]
DP_AMP = sum((mpf("3.28") ** k / mp.factorial(k) for k in range(6)), mpf(0)) + mpf("3.28") ** 6 / 600  # sum |z|^k terms of R


def walk_auto(group, theta, h_max, tol, shift=0, checks=True):
    """The auto solver where nothing is rejected: every step min(h_max, left), the mode by the documented counters.
    Returns (pred, walk, mode string, [explicit, implicit, rejected, switches], worst scaled error)."""
    w = Walk(group, theta)
    rtol = atol = mpf(tol)
    st = dict(implicit=False, stiff=0, calm=0, back=0, n=[0, 0, 0, 0], modes=[], worst=mpf(0))

    def piece(x, t0, t1, rates, row):
        f = rhs_of(w.body, w.p, rates)
        t = t0
        while t < t1:
            left = t1 - t
            h = min(h_max, left)
            hm = mpf(h)
            sw = False
            if st["implicit"]:
                new, e, J = ros_step(f, mpf(t), x, hm, shift=shift)
                err = scaled_norm(e, x, new, rtol, atol)
                hj = hm * norm_inf(J)
                if checks:
                    assert abs(hj - BACK_RHO) >= 0.2, (theta, t, float(hj))
                if hj <= BACK_RHO:
                    st["back"] += 1
                    sw = st["back"] == BACK_STEPS
                else:
                    st["back"] = 0
                st["n"][1] += 1
            else:
                calls = []

                def rec(tt, xx):
                    calls.append((xx, f(tt, xx)))
                    return calls[-1][1]
                new, hat = erk_step(DP, rec, mpf(t), x, hm)
                err = scaled_norm([a - b for a, b in zip(new, hat)], x, new, rtol, atol)
                (g6, k6), (x7, k7) = calls[5], calls[6]  # stages 6 and 7 both sit at t + h; stage 7's argument is y+
                assert all(a == b for a, b in zip(x7, new))
                num = sum((a - b) ** 2 for a, b in zip(k7, k6))
                den = sum((a - b) ** 2 for a, b in zip(new, g6))
                if checks:
                    assert mp.sqrt(den) >= mpf(10) ** -6 * max(abs(v) for v in list(x) + list(new)), (theta, t)
                if den > 0:
                    hr = hm * mp.sqrt(num / den)
                    if checks:
                        assert abs(hr - STIFF_RHO) >= 0.02, (theta, t, float(hr))
                    if hr > STIFF_RHO:
                        st["calm"], st["stiff"] = 0, st["stiff"] + 1
                        sw = st["stiff"] == STIFF_STEPS
                    else:
                        st["calm"] += 1
                        if st["calm"] == CALM_STEPS:
                            st["stiff"] = 0
                st["n"][0] += 1
            st["modes"].append("I" if st["implicit"] else "E")
            st["worst"] = max(st["worst"], err)
            if sw:
                st.update(implicit=not st["implicit"], stiff=0, calm=0, back=0)
                st["n"][3] += 1
            x = new
            w.note(x, h)
            t = t1 if h == left else t + h
        return x

    pred = w.run(piece)
    return pred, w, "".join(st["modes"]), st["n"], st["worst"]


def build_auto(group):
    g = {k: group[k] for k in ("name", "scalable", "model", "h_max", "occasions")}
    g["rtol"] = g["atol"] = tol = group["tol"]
    cases = []
    for th in group["thetas"]:
        pred, w, modes, counts, worst = walk_auto(group, th, group["h_max"], tol)
        assert worst <= 0.25, (g["name"], th, float(worst))
        lam_h = mpf(th[0]) * mpf(group["h_max"])
        assert stability(5, -lam_h) <= 1 and ros2_R(-lam_h) <= 1
        amount = [v * w.v for v in pred]
        amp = max(DP_AMP, 4 + 1 + GAMMA * lam_h)  # per step: the explicit stages' sum |z|^k, or the solve's condition
        kappa = float(w.n_steps * amp * w.x_max / max(abs(v) for v in amount))
        noise = 0.0
        for s in (1, -1):
            alt, _, m2, c2, _ = walk_auto(group, th, group["h_max"], tol, shift=s, checks=False)
            assert m2 == modes and c2 == counts
            noise = max(noise, rel(alt, pred))
        cases.append(dict(theta=fl(th), auto=fl(pred), exact=fl(walk_exact(group, th)), n_steps=w.n_steps, kappa=kappa,
                          lambda_h=float(lam_h), max_step_err=float(worst), diff_noise=noise, counts=counts, modes=modes))
    sw, calm = cases
    assert sw["counts"][2] == 0 and sw["counts"][3] == 3 and sw["modes"].startswith("E" * 15 + "I" * 17 + "E" * 19 + "I"), sw["modes"]
    assert set(sw["modes"][51:]) == {"I"}
    assert calm["counts"] == [calm["n_steps"], 0, 0, 0]
    g["cases"] = cases
    return g


def main():
    doc = dict(generator="tests/golden/gen_ode_exact_stiff.py", dps=40, groups=[build(g) for g in GROUPS],
               auto=[build_auto(g) for g in AUTO_GROUPS])
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(doc['groups'])} groups, {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < 256 << 10
    for g in doc["groups"]:
        print(g["name"])
        for c in g["cases"]:
            bar = max(64 * U * c["kappa"], c["diff_noise"])
            print(f"  h lambda {c['lambda_h']:9.3f}  steps {c['n_steps']}  err {c['max_step_err']:.3f}  kappa {c['kappa']:.3g}"
                  f"  diff_noise {c['diff_noise']:.2e}  bar {bar:.2e}  |ros2 - exact| {rel(c['ros2'], c['exact']):.2e}")
        for m, d in g["mutations"].items():
            best = max(dv / max(64 * U * c["kappa"], c["diff_noise"]) for dv, c in zip(d, g["cases"]))
            print(f"  {m:22s} moved / bar, best case {best:.3g}   {[f'{v:.1e}' for v in d]}")
    for g in doc["auto"]:
        for c in g["cases"]:
            print(g["name"], c["counts"], c["modes"], f"err {c['max_step_err']:.3f} kappa {c['kappa']:.3g} diff_noise {c['diff_noise']:.2e}")


if __name__ == "__main__":
    main()
