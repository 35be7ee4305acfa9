#!/usr/bin/env python3
"""Generate tests/golden/edge_math.json: independent-mathematics fixtures at the edges where closed-form
propagators go wrong (near-coincident nodes, extreme rates and horizons, ladder chains, infusion edges, CL
parametrisations, covariate models, lagged inputs).

Same method as gen_independent.py, and still neither the oracle nor the product is imported: the linear system
dx/dt = A(t) x + b(t) is propagated with the augmented matrix exponential expm([[A, b], [0, 0]] dt) in mpmath at
40 digits, split at every breakpoint, boluses added at their times, y = x[central] / v at the observations
(observation before dose at equal times; infusion rate amount / duration on [t, t + dur), the end time formed in
double precision as the reference forms it).

Covariate models follow the reference's analytical solve (src/simulator/equation/analytical/mod.rs, `solve`):
between two consecutive events the interval is split at the infusion ends strictly inside it, and each
sub-interval [t0, t1] is propagated with the rate constants derived from the covariate at t1 (cov_time
"segment_end_abs") or at t1 - t0 (cov_time "segment_dt": the derive closure receives the step length, the
quirk pinned in tests/test_oracle_known_answers.py).  The covariate is the piecewise-linear interpolant of
its knots, the first value before the first knot and the last one from the last knot on.  Derived constant:
k_elim = k_elim_0 (wt / 70)^0.75.

Lagged inputs: the same schedule with the lagged boluses moved by the lag.

Each case stores kappa = max scale / |node_i - node_j| over the nodes the closed form divides by (eigenvalues
of the disposition part, plus ka), scale = the largest rate constant, over every parameter set the case meets,
and `singular`: the PMX_PAIR_* status the reference's own double-precision formulas imply (0 = none), restated
here from the reference: the two- and three-compartment eigen-solves panic on a negative discriminant (q > 0,
evaluated in the reference's order of operations), and ka equal to an eigenvalue divides 0 by 0.

A group is one model and one dosing schedule with several parameter vectors; `variants` are the same schedule
with every time and duration stretched (same program shape, other step lengths), each with its own truth.

Run:  python tests/golden/gen_edge.py     (deterministic; numpy Generator seed 20261016)
"""
import json
import math
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_independent import rate_matrix  # noqa: E402  (the micro-constant matrices, unchanged)

mp.mp.dps = 40
OUT = os.path.join(HERE, "edge_math.json")

MICRO = {"one_compartment": 1, "one_compartment_with_absorption": 2, "two_compartments": 3,
         "two_compartments_with_absorption": 4, "three_compartments": 5, "three_compartments_with_absorption": 6}
CENTRAL = {"one_compartment": 0, "one_compartment_with_absorption": 1, "two_compartments": 0,
           "two_compartments_with_absorption": 1, "three_compartments": 0, "three_compartments_with_absorption": 1}
# CL kernels -> (micro structure, number of kernel parameters); conversions from {one,two,three}_compartment_cl_models.rs
CL = {"one_compartment_cl": ("one_compartment", 2), "one_compartment_cl_with_absorption": ("one_compartment_with_absorption", 3),
      "two_compartments_cl": ("two_compartments", 4), "two_compartments_cl_with_absorption": ("two_compartments_with_absorption", 5),
      "three_compartments_cl": ("three_compartments", 6),
      "three_compartments_cl_with_absorption": ("three_compartments_with_absorption", 7)}
# the elimination constant a covariate scales, per micro structure
ELIM = {"one_compartment": 0, "one_compartment_with_absorption": 1, "two_compartments": 0,
        "two_compartments_with_absorption": 0, "three_compartments": 0, "three_compartments_with_absorption": 1}


def micro_of(kernel, p):
    """Kernel parameters (mp) -> micro-constants of the micro structure."""
    if kernel in MICRO:
        return list(p)
    if kernel == "one_compartment_cl":
        return [p[0] / p[1]]
    if kernel == "one_compartment_cl_with_absorption":
        return [p[0], p[1] / p[2]]
    if kernel == "two_compartments_cl":
        cl, q, vc, vp = p
        return [cl / vc, q / vc, q / vp]
    if kernel == "two_compartments_cl_with_absorption":
        ka, cl, q, vc, vp = p
        return [cl / vc, ka, q / vc, q / vp]
    if kernel == "three_compartments_cl":
        cl, q2, q3, vc, v2, v3 = p
        return [cl / vc, q2 / vc, q3 / vc, q2 / v2, q3 / v3]
    if kernel == "three_compartments_cl_with_absorption":
        ka, cl, q2, q3, vc, v2, v3 = p
        return [ka, cl / vc, q2 / vc, q3 / vc, q2 / v2, q3 / v3]
    raise KeyError(kernel)


def structure_of(kernel):
    return CL[kernel][0] if kernel in CL else kernel


def n_kernel_params(kernel):
    return CL[kernel][1] if kernel in CL else MICRO[kernel]


def disposition(structure, k):
    """(eigenvalues of the disposition part, ka or None) in mp, from the micro-constants."""
    if structure == "one_compartment":
        return [k[0]], None
    if structure == "one_compartment_with_absorption":
        return [k[1]], k[0]
    if structure in ("two_compartments", "two_compartments_with_absorption"):
        ke, kcp, kpc = (k[0], k[1], k[2]) if structure == "two_compartments" else (k[0], k[2], k[3])
        s = ke + kcp + kpc
        d = mp.sqrt(s * s - 4 * ke * kpc)
        return [(s + d) / 2, (s - d) / 2], (k[1] if structure == "two_compartments_with_absorption" else None)
    ka = None
    if structure == "three_compartments_with_absorption":
        ka, k = k[0], k[1:]
    k10, k12, k13, k21, k31 = k
    A = mp.matrix([[-(k10 + k12 + k13), k21, k31], [k12, -k21, 0], [k13, 0, -k31]])
    ev = mp.eig(A, left=False, right=False)
    return sorted((-mp.re(e) for e in ev), reverse=True), ka


def kappa_of(structure, k):
    lam, ka = disposition(structure, k)
    nodes = lam + ([ka] if ka is not None else [])
    scale = max(abs(x) for x in k)
    kap = mp.mpf(1)
    for i in range(len(nodes)):
        for j in range(i + 1, len(nodes)):
            g = abs(nodes[i] - nodes[j])
            kap = max(kap, scale / g) if g > 0 else mp.inf
    return kap


def reference_singular(structure, k):
    """PMX_PAIR_* status the reference's double-precision formulas imply for micro-constants k (doubles)."""
    k = [float(x) for x in k]
    if structure in ("two_compartments", "two_compartments_with_absorption"):
        ke, kcp, kpc = (k[0], k[1], k[2]) if structure == "two_compartments" else (k[0], k[2], k[3])
        s = ke + kcp + kpc
        sq = s * s - 4.0 * ke * kpc
        if sq < 0.0:
            return 1
        if structure == "two_compartments_with_absorption":
            sq = math.sqrt(sq)
            if k[1] in ((ke + kcp + kpc + sq) / 2.0, (ke + kcp + kpc - sq) / 2.0):
                return 2
        return 0
    if structure == "one_compartment_with_absorption":
        return 2 if k[0] == k[1] else 0
    if structure.startswith("three"):
        k10, k12, k13, k21, k31 = k[-5:]
        a = k10 + k12 + k13 + k21 + k31
        b = k10 * k21 + k13 * k21 + k10 * k31 + k12 * k31 + k21 * k31
        c = k10 * k21 * k31
        m = (3.0 * b - a * a) / 3.0
        n = (2.0 * (a * a * a) - 9.0 * a * b + 27.0 * c) / 27.0
        q = (n * n) / 4.0 + (m * m * m) / 27.0
        return 1 if q > 0.0 else 0
    return 0


def wt_at(knots, t):
    ts, vs = knots
    if t <= ts[0]:
        return mp.mpf(vs[0])
    for i in range(len(ts) - 1):
        if ts[i] <= t < ts[i + 1]:
            t0, t1 = mp.mpf(ts[i]), mp.mpf(ts[i + 1])
            return mp.mpf(vs[i]) + (mp.mpf(vs[i + 1]) - mp.mpf(vs[i])) * (t - t0) / (t1 - t0)
    return mp.mpf(vs[-1])


def params_at(model, theta, t0, t1):
    """Micro-constants (mp) on the sub-interval [t0, t1]."""
    kernel = model["kernel"]
    p = [mp.mpf(x) for x in theta[:n_kernel_params(kernel)]]
    cov = model.get("cov")
    if cov:
        tc = (t1 - t0) if cov["mode"] == "segment_dt" else t1
        p[ELIM[kernel]] *= (wt_at(cov["knots"], tc) / 70) ** mp.mpf("0.75")
    return micro_of(kernel, p)


def simulate(model, theta, events, with_kappa=False):
    """Predictions at the observations (and kappa, singular status over every parameter set met)."""
    kernel = model["kernel"]
    structure = structure_of(kernel)
    central = CENTRAL[structure]
    n = len(rate_matrix(structure, [1.0] * 8)[0])
    v = mp.mpf(theta[n_kernel_params(kernel)])
    lag = model.get("lag")
    ev = []
    for e in events:
        kind, t, val, dur, io = e
        if kind == "bolus" and lag is not None and int(io) == lag["input"]:
            t = t + theta[lag["param"]]  # (double, as the reference rewrites the event time)
        ev.append((kind, t, val, dur, io))
    rank = {"obs": 0, "bolus": 1, "inf": 2}
    ev.sort(key=lambda e: (e[1], rank[e[0]]))
    x = mp.matrix(n, 1)
    t = ev[0][1] if ev else 0.0
    infs = []
    kap, sing = mp.mpf(1), 0

    def segment(x, a, b):
        nonlocal kap, sing
        k = params_at(model, theta, mp.mpf(a), mp.mpf(b))
        if with_kappa:
            kap = max(kap, kappa_of(structure, k))
            sing = sing or reference_singular(structure, k)
        A, _ = rate_matrix(structure, k)
        rate = sum((mp.mpf(val) / mp.mpf(dur) for (s, e, val, dur) in infs if s <= a and b <= e), mp.mpf(0))
        M = mp.matrix(n + 1, n + 1)
        for i in range(n):
            for j in range(n):
                M[i, j] = A[i][j]
        M[central, n] = rate
        E = mp.expm(M * (mp.mpf(b) - mp.mpf(a)))
        xa = mp.matrix(n + 1, 1)
        for i in range(n):
            xa[i] = x[i]
        xa[n] = 1
        xb = E * xa
        return mp.matrix([xb[i] for i in range(n)])

    preds = []
    for e in ev:
        te = e[1]
        if te > t:
            pts = sorted({t, te} | {en for (s, en, _, _) in infs if t < en < te})
            pts = [p for i, p in enumerate(pts) if i == 0 or abs(p - pts[i - 1]) >= 1e-12]  # (the reference's dedup)
            if pts[-1] != te:
                pts[-1] = te
            for a, b in zip(pts[:-1], pts[1:]):
                x = segment(x, a, b)
            t = te
        if e[0] == "bolus":
            x[int(e[4])] += mp.mpf(e[2])
        elif e[0] == "inf":
            infs.append((e[1], e[1] + e[3], e[2], e[3]))  # end time in double
        else:
            preds.append(float(x[central] / v))
    if with_kappa:
        return preds, float(kap), int(sing)
    return preds


# ------------------------------------------------------------------------------------------------ schedules
def obs(*ts):
    return [["obs", float(t), 0.0, 0.0, 0] for t in ts]


def sched_plain(has_gut, horizon=48.0, infusion=True):
    ev = [["bolus", 0.0, 100.0, 0.0, 1 if has_gut else 0]]
    if has_gut:
        ev.append(["bolus", 12.0, 80.0, 0.0, 0])
    if infusion:
        ev.append(["inf", 24.0, 150.0, 2.5, 0])
    h = horizon / 48.0
    ev += obs(*[h * t for t in (0.25, 1.0, 2.0, 4.0, 8.0, 12.0, 20.0, 24.0, 25.0, 26.5, 30.0, 48.0)])
    return ev


def stretched(events, f):
    return [[e[0], e[1] * f, e[2], e[3] * f, e[4]] for e in events]


def easy_theta(kernel, rng):
    """A parameter vector in the well-conditioned region (the lane a bad neighbour could hide behind)."""
    structure = structure_of(kernel)
    if kernel in CL:
        base = {"one_compartment_cl": [1.0, 10.0], "one_compartment_cl_with_absorption": [1.5, 1.0, 10.0],
                "two_compartments_cl": [1.0, 2.0, 10.0, 20.0], "two_compartments_cl_with_absorption": [1.5, 1.0, 2.0, 10.0, 20.0],
                "three_compartments_cl": [1.0, 2.0, 0.5, 10.0, 20.0, 40.0],
                "three_compartments_cl_with_absorption": [1.5, 1.0, 2.0, 0.5, 10.0, 20.0, 40.0]}[kernel]
    else:
        base = {"one_compartment": [0.2], "one_compartment_with_absorption": [1.5, 0.2], "two_compartments": [0.2, 0.6, 0.3],
                "two_compartments_with_absorption": [0.2, 1.5, 0.6, 0.3], "three_compartments": [0.2, 0.6, 0.3, 0.4, 0.05],
                "three_compartments_with_absorption": [1.5, 0.2, 0.6, 0.3, 0.4, 0.05]}[structure]
    return [float(b * rng.uniform(0.8, 1.25)) for b in base] + [float(rng.uniform(5, 50))]


# relative node gaps; 0.0 = exact equality.  (For ka placed on a two- or three-compartment eigenvalue, "exact" is the
# eigenvalue rounded to double: kappa comes out near 1/u and the bar 64 u kappa above 1, so those cases check the
# status and finiteness only.  ka == ke in the one-compartment model is exact: the reference's 0/0, `singular` 2.)
GAPS = [1e-2, 1e-4, 1e-6, 1e-8, 0.0]


def fam_near(rng):
    groups = []
    # three compartments, k21 ~ k31, weak coupling
    th = [easy_theta("three_compartments", rng)]
    for _ in range(2):
        r = float(rng.uniform(0.2, 2.0))
        for d in GAPS:
            c = max(d, 1e-8) * r
            th.append([float(rng.uniform(0.05, 0.5)), c * float(rng.uniform(0.5, 2)), c * float(rng.uniform(0.5, 2)), r,
                       r * (1 + d), float(rng.uniform(5, 50))])
    groups.append(("a_three_k21_k31", {"kernel": "three_compartments"}, sched_plain(False), th, 3))
    # three compartments with absorption, ka near each eigenvalue
    th = [easy_theta("three_compartments_with_absorption", rng)]
    for _ in range(2):
        k = [float(rng.uniform(0.05, 0.5)), float(rng.uniform(0.2, 2)), float(rng.uniform(0.2, 2)), float(rng.uniform(0.2, 2)),
             float(rng.uniform(0.02, 0.2))]
        lam, _ = disposition("three_compartments", [mp.mpf(x) for x in k])
        for li in lam:
            for d in GAPS:
                th.append([float(li * (1 + mp.mpf(d)))] + k + [float(rng.uniform(5, 50))])
    groups.append(("a_three_abs_ka_lambda", {"kernel": "three_compartments_with_absorption"}, sched_plain(True), th, 3))
    # two compartments with absorption, ka near lambda1 or lambda2
    th = [easy_theta("two_compartments_with_absorption", rng)]
    for _ in range(2):
        ke, kcp, kpc = (float(rng.uniform(0.05, 0.5)), float(rng.uniform(0.2, 2)), float(rng.uniform(0.1, 1)))
        lam, _ = disposition("two_compartments", [mp.mpf(ke), mp.mpf(kcp), mp.mpf(kpc)])
        for li in lam:
            for d in GAPS:
                th.append([ke, float(li * (1 + mp.mpf(d))), kcp, kpc, float(rng.uniform(5, 50))])
    groups.append(("a_two_abs_ka_lambda", {"kernel": "two_compartments_with_absorption"}, sched_plain(True), th, 6))
    # one compartment with absorption, ka ~ ke
    th = [easy_theta("one_compartment_with_absorption", rng)]
    for _ in range(3):
        ke = float(rng.uniform(0.05, 2.0))
        for d in GAPS:
            th.append([ke * (1 + d), ke, float(rng.uniform(5, 50))])
    groups.append(("a_one_abs_ka_ke", {"kernel": "one_compartment_with_absorption"}, sched_plain(True), th, 6))
    return groups


def fam_range(rng):
    groups = []
    lo, hi = math.log(1e-4), math.log(5e3)
    long_obs = obs(1e-9, 0.5, 3.0, 24.0, 200.0, 800.0, 2000.0)
    for kernel in ("one_compartment", "two_compartments", "three_compartments", "three_compartments_with_absorption"):
        has_gut = kernel.endswith("absorption")
        ev = [["bolus", 0.0, 100.0, 0.0, 1 if has_gut else 0], ["bolus", 0.0, 50.0, 0.0, 0],
              ["inf", 100.0, 300.0, 50.0, 0]] + long_obs
        ev += obs(1e-10 + 1e-6, 1e-3)
        th = [easy_theta(kernel, rng)]
        for _ in range(8):
            th.append([float(math.exp(rng.uniform(lo, hi))) for _ in range(MICRO[kernel])] + [float(rng.uniform(1, 50))])
        # a fast and a very slow mode side by side; everything slow; everything fast
        nk = MICRO[kernel]
        th.append([5e3] + [1e-4] * (nk - 1) + [10.0])
        th.append([1e-4 * (1 + 0.37 * i) for i in range(nk)] + [10.0])
        th.append([5e3 * (0.5 + 0.1 * i) for i in range(nk)] + [10.0])
        groups.append((f"b_range_{kernel}", {"kernel": kernel}, ev, th, 0))
    # A long infusion towards steady state with a slow terminal phase: the prediction is dominated by the slow mode's
    # c3 / lambda3 term, so a relative error in the smallest eigenvalue shows up undamped in the peak concentration
    # (elsewhere the slow phase only carries the small tail).  Fixed rates (no draws: the other groups stay as they are).
    ev = [["inf", 0.0, 4000.0, 400.0, 0]] + obs(1.0, 10.0, 50.0, 100.0, 200.0, 300.0, 400.0, 450.0, 600.0)
    slow = [[k10, 3.0, 1.0, 2.0, k31, 10.0] for k10 in (0.1, 1.0) for k31 in (0.02, 0.002, 0.0005)]
    groups.append(("b_range_slow_phase_three_compartments", {"kernel": "three_compartments"}, ev,
                   [easy_theta("three_compartments", np.random.default_rng(7))] + slow, 0))
    groups.append(("b_range_slow_phase_three_compartments_with_absorption", {"kernel": "three_compartments_with_absorption"},
                   ev + [["bolus", 0.0, 500.0, 0.0, 0]],
                   [easy_theta("three_compartments_with_absorption", np.random.default_rng(7))] + [[1.5] + s for s in slow], 0))
    return groups


def ladder_times(d, factors, t0=0.0, ulp_at=None):
    ts, t, dt = [t0], t0, d
    for i, f in enumerate(factors):
        t = t + dt
        if ulp_at == i:
            t = float(np.nextafter(t, np.inf))
        ts.append(t)
        dt *= f
    return ts


def fam_ladder(rng):
    groups = []
    d = 1.0 / 64
    doubling = ladder_times(d, [2] * 13)  # rungs 1,2,4,...: the span reaches 1024 and then starts over
    tripling = ladder_times(d / 4, [3] * 8)
    mixed = ladder_times(d, [1, 1, 2, 4, 3, 1, 4, 2, 2, 1, 4, 4])
    for name, ts in (("doubling", doubling), ("tripling", tripling), ("mixed", mixed),
                     ("doubling_ulp", ladder_times(d, [2] * 13, ulp_at=6))):
        for kernel in ("two_compartments", "three_compartments_with_absorption"):
            has_gut = kernel.endswith("absorption")
            ev = [["bolus", 0.0, 100.0, 0.0, 1 if has_gut else 0]] + obs(*ts[1:])
            th = [easy_theta(kernel, rng)]
            for scale in (1.0, 40.0, 400.0):  # ladder chains at large lambda too
                for _ in range(2):
                    t = easy_theta(kernel, rng)
                    th.append([x * scale for x in t[:-1]] + t[-1:])
            groups.append((f"c_ladder_{name}_{kernel}", {"kernel": kernel}, ev, th, 0))
    return groups


def fam_infusion(rng):
    groups = []
    for kernel in ("one_compartment", "two_compartments", "three_compartments", "three_compartments_with_absorption"):
        has_gut = kernel.endswith("absorption")
        ev = [["inf", 0.0, 100.0, 2.0, 0],          # ends exactly on an observation (t = 2)
              ["inf", 2.0, 60.0, 2.0, 0],           # back to back with the first
              ["inf", 3.0, 40.0, 3.0, 0],           # overlaps the second
              ["bolus", 6.0, 30.0, 0.0, 1 if has_gut else 0],  # ends exactly on a dose (3 + 3 = 6)
              ["bolus", 10.0, 50.0, 0.0, 0], ["inf", 10.0, 80.0, 1.5, 0],  # bolus and infusion at the same time
              ["inf", 14.0, 5.0, 1e-6, 0],          # a very short infusion
              ["inf", 20.0, 70.0, 0.5, 0], ["inf", 20.25, 70.0, 0.25, 0]]  # nested, ending together
        ev += obs(0.5, 2.0, 3.0, 4.0, 5.5, 6.0, 10.0, 11.5, 14.0, 14.0000005, 14.5, 20.25, 20.5, 24.0, 36.0)
        th = [easy_theta(kernel, rng) for _ in range(6)]
        groups.append((f"d_infusion_{kernel}", {"kernel": kernel}, ev, th, 0))
    return groups


def fam_cl(rng):
    groups = []
    for kernel in ("one_compartment_cl", "one_compartment_cl_with_absorption", "two_compartments_cl",
                   "two_compartments_cl_with_absorption", "three_compartments_cl", "three_compartments_cl_with_absorption"):
        has_gut = kernel.endswith("absorption")
        th = [easy_theta(kernel, rng) for _ in range(5)]
        np_ = n_kernel_params(kernel)
        for _ in range(3):  # wide ranges
            th.append([float(math.exp(rng.uniform(math.log(0.01), math.log(100.0)))) for _ in range(np_)] + [10.0])
        groups.append((f"e_{kernel}", {"kernel": kernel}, sched_plain(has_gut), th, 0))
    return groups


def cov_subject(has_gut, infusion, constant):
    ev = [["bolus", 0.0, 200.0, 0.0, 1 if has_gut else 0]]
    if has_gut:
        ev.append(["bolus", 24.0, 150.0, 0.0, 0])
    if infusion:
        ev.append(["inf", 12.0, 100.0, 3.0, 0])
    ev += obs(0.5, 1.0, 2.0, 4.0, 6.0, 8.0, 12.0, 14.0, 16.0, 24.0, 26.0, 30.0, 36.0, 48.0)
    knots = [[0.0], [82.0]] if constant else [[0.0, 6.0, 20.0, 40.0], [60.0, 75.0, 90.0, 70.0]]
    return ev, knots


def fam_cov(rng):
    groups = []
    for kernel, infusion, variants in (("three_compartments_with_absorption", False, 3),  # the C5 shape: matrix-free walker
                                       ("three_compartments", True, 3),  # an infusion: the generic covariate walker
                                       ("one_compartment_with_absorption", False, 6), ("two_compartments", True, 6)):
        has_gut = kernel.endswith("absorption")
        for mode in ("segment_dt", "segment_end_abs"):
            for constant in (False, True):
                ev, knots = cov_subject(has_gut, infusion, constant)
                th = [easy_theta(kernel, rng) for _ in range(3)]
                if kernel.startswith("three"):  # near-coincident nodes under a covariate too
                    for d in (1e-4, 1e-6):
                        r = float(rng.uniform(0.2, 2.0))
                        t = [float(rng.uniform(0.05, 0.5)), d * r, d * r * 1.3, r, r * (1 + d)]
                        th.append(([1.5] if has_gut else []) + t + [20.0])
                model = {"kernel": kernel, "cov": {"mode": mode, "knots": knots}}
                name = f"f_cov_{kernel}_{mode}_{'const' if constant else 'interp'}"
                groups.append((name, model, ev, th, variants if not constant and mode == "segment_dt" else 0))
    return groups


def fam_lag(rng):
    groups = []
    for kernel in ("one_compartment_with_absorption", "two_compartments_with_absorption", "three_compartments_with_absorption"):
        ev = sched_plain(True)
        th = [easy_theta(kernel, rng) + [0.37], easy_theta(kernel, rng) + [1.9]]
        if kernel == "one_compartment_with_absorption":
            th += [[0.3 * (1 + d), 0.3, 12.0, 0.61] for d in (1e-4, 1e-8)]
        groups.append((f"g_lag_{kernel}", {"kernel": kernel, "lag": {"input": 0, "param": MICRO[kernel] + 1}}, ev, th, 0))
    return groups


def main():
    rng = np.random.default_rng(20261016)
    out = []
    for fam in (fam_near, fam_range, fam_ladder, fam_infusion, fam_cl, fam_cov, fam_lag):
        for name, model, ev, thetas, n_var in fam(rng):
            cases = []
            for th in thetas:
                pred, kap, sing = simulate(model, th, ev, with_kappa=True)
                cases.append({"theta": th, "kappa": kap, "singular": sing, "expected": pred})
            variants = []
            for j in range(1, n_var):
                evj = stretched(ev, 1.0 + 0.125 * j)
                variants.append({"events": evj, "expected": [simulate(model, th, evj) for th in thetas]})
            out.append({"name": name, "model": model, "events": ev, "cases": cases, "variants": variants})
            print(f"{name}: {len(cases)} cases, {len(variants)} variants", flush=True)
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/gen_edge.py", "mp_dps": 40, "groups": out}, f, indent=None,
                  separators=(",", ":"))
        f.write("\n")
    print(f"wrote {sum(len(g['cases']) for g in out)} cases in {len(out)} groups to {OUT}")


if __name__ == "__main__":
    main()
