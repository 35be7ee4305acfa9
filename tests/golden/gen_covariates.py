#!/usr/bin/env python3
"""Generate tests/golden/covariate_math.json: covariate models beyond one linear weight, against 40-digit truth.

Same method as gen_edge.py / gen_ode_exact.py / gen_user_closures.py: mpmath at 40 digits, neither `oracle` nor
`pharmsol_amd` imported.  The rules are restated from the reference:

  covariate  knots sorted by time; segment i covers [t_i, t_{i+1}), the last one is open-ended; a segment carries its
             value forward when the covariate is fixed or when it is the last one, otherwise it is the line
             slope * t + intercept with slope = (v_{i+1} - v_i) / (t_{i+1} - t_i) and intercept = v_i - slope t_i formed in
             doubles and evaluated in doubles (only then converted to mpf); before the first knot the first value
                                                                          src/data/covariate.rs:60-65,189-241
  analytical one solve per pair of events, split at the infusion ends strictly inside; per sub-interval [t0, t1] the
             derive closure sees t1 - t0 (cov_time "segment_dt", the macro lowering expand/analytical.rs:254,286) or
             t1 ("segment_end_abs")                                      src/simulator/equation/analytical/mod.rs:299-370
  derived    derived[d] = (theta[src] * f0) * f1, Pow = (cov / ref)^coef, Lin = 1 + coef (cov - ref); a `bind` gives
             every kernel parameter its theta or derived value              bindings.rs:98-117
  volume     out = x[central] / v at the observation's absolute time in both modes    analytical/mod.rs:373-407
  occasions  every occasion starts from a zero state and reads its own knots (cell = occasion * n_cov + covariate)
                                                                          analytical/mod.rs:409-426
  lag        a bolus on the lagged input moves to t + lag (a double)     src/data/structs.rs:611-643
  ODE        the partition rule and the exact-arithmetic RK4 step of gen_ode_exact.py; the rate constants are rebuilt
             from the covariates at every stage's absolute time            expand/ode.rs:150
             the clock starts at the earliest recorded time and the first rewritten event acts at it  ode/mod.rs:348,639-721
             With carry-forward covariates only, the true solution is a chain of augmented matrix exponentials between
             the jumps (`exact`); `rk4` is the exact-arithmetic walk, kappa as gen_ode_exact.py defines it.

Every analytical group carries NINE subjects (a whole chunk of 8 and a partial one) on one event schedule, each with
its own knot values (own knot times where the group says so), its own dose scale and its own truth, so a kernel that
read another member's factor row cannot pass.  Per case: kappa (gen_edge.py's, the largest over every parameter set
the nine subjects meet) and `singular`.  Per group: the times every PROP / OBS of the march reads the covariates at
(`march`, indices into `seen` = [occasion, time]) and the double-precision covariate values there (`cov_seen`, per
subject), for the bit-equality check of the host compiler.  A subject's knots are stored per occasion as
{name: [[times], [values]]}; the carry-forward covariates are named in the model's `fixed`.  To keep the file small the
analytical truth is rounded to 13 significant digits (5e-14 relative, 1 / 2000 of the tightest analytical bar); the ODE
values, whose bars are near 1e-12, are full doubles.

Self-checks, asserted: 64 u kappa <= 1e-10 (analytical) / <= 1e-11 (ODE); any two subjects of an analytical group
differ by >= 1000 bars on some case; every deliberately wrong rule in WRONG moves a case of a group named for it by
>= 1000 bars (printed); every ODE time is dyadic, so every stage time is exact in double however it is summed.

Run:  python tests/golden/gen_covariates.py     (deterministic; rewrites covariate_math.json byte for byte)
"""
import json
import math
import os
import sys

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_edge import CENTRAL, kappa_of, micro_of, n_kernel_params, reference_singular, structure_of  # noqa: E402
from gen_independent import rate_matrix  # noqa: E402
from gen_ode_exact import BODIES, RK4, erk_step, lambda_max, matrix_of, rate_vector, rewrite, stability, step_count  # noqa: E402

mp.mp.dps = 40
mpf = mp.mpf
OUT = os.path.join(HERE, "covariate_math.json")
U = 2.0 ** -53
RANK = {"obs": 0, "bolus": 1, "inf": 2}
SCALES = (1.0, 2.0, 0.5, 3.0, 0.25, 1.5, 4.0, 0.75, 5.0)
# wrong rule -> the groups named for it (prefix match)
WRONG = {"fixed_as_linear": ("a_",), "le_at_knot": ("d_",), "extrapolate_before_first": ("d_",),
         "extrapolate_past_last": ("d_",), "occasion_two_reads_one": ("e_",), "volume_at_derive_time": ("c_three",),
         "second_factor_dropped": ("c_",), "factors_swapped": ("c_three",), "modes_exchanged": ("a_", "c_three"),
         "first_propagator_of_a_length_reused": ("a_dyn3_step_segment_end_abs",),
         "previous_step_constants": ("a_dyn3_step_segment_end_abs",), "covariates_frozen_at_step_start": ("g_",)}


# ------------------------------------------------------------------------------------------------------- covariates
def cov_value(knots, fixed, t, V=()):
    """Covariate::interpolate at a double time (double arithmetic) or at an mpf stage time (mpf arithmetic on the double
    slope and intercept)."""
    kn = sorted((float(a), float(b)) for a, b in knots)
    n = len(kn)
    lin = not fixed or "fixed_as_linear" in V

    def line(i):
        (t0, v0), (t1, v1) = kn[i], kn[i + 1]
        slope = (v1 - v0) / (t1 - t0)
        return slope * t + (v0 - slope * t0)

    for i, (t0, v0) in enumerate(kn):
        last = i + 1 == n
        inside = t0 <= t and (last or (t <= kn[i + 1][0] if "le_at_knot" in V else t < kn[i + 1][0]))
        if inside:
            if last:
                return line(i - 1) if ("extrapolate_past_last" in V and lin and n > 1) else v0
            return line(i) if lin else v0
    if "extrapolate_before_first" in V and lin and n > 1:
        return line(0)
    return kn[0][1]


def covs_at(mdl, sub, occ, t, V=()):
    cell = sub["cov"][0 if "occasion_two_reads_one" in V else occ]
    return [cov_value(zip(*cell[n]), n in mdl["fixed"], t, V) for n in mdl["covariates"]]


def factor(f, cv):
    op, _, ref, coef = f
    cv = mpf(cv)
    return (cv / mpf(ref)) ** mpf(coef) if op == "pow" else 1 + mpf(coef) * (cv - mpf(ref))


def values_at(mdl, theta, covs, V=()):
    """name -> value (mpf) of every primary and derived parameter at the covariate row `covs`."""
    val = {n: mpf(theta[i]) for i, n in enumerate(mdl["params"])}
    derived = dict(mdl["derived"])
    if "factors_swapped" in V:
        a, b = list(derived)[:2]
        derived[a], derived[b] = [derived[a][0], derived[b][1]], [derived[b][0], derived[a][1]]
    for name, (src, facs) in derived.items():
        x = mpf(theta[mdl["params"].index(src)])
        for k, f in enumerate(facs):
            if k == 1 and "second_factor_dropped" in V:
                break
            x = x * factor(f, covs[mdl["covariates"].index(f[1])])
        val[name] = x
    return val


# ------------------------------------------------------------------------------------------------- analytical march
def simulate(group, sub, theta, V=(), stats=None):
    """Predictions of one subject (mpf).  stats: dict collecting kappa / singular / the march."""
    mdl = group["model"]
    kernel = mdl["kernel"]
    structure = structure_of(kernel)
    central = CENTRAL[structure]
    names = mdl["kernel_params"]
    n = len(rate_matrix(structure, [1.0] * 8)[0])
    mode = mdl["mode"]
    if "modes_exchanged" in V:
        mode = "segment_dt" if mode == "segment_end_abs" else "segment_end_abs"
    lag = mdl.get("lag")
    preds = []
    for o, events in enumerate(group["occasions"]):
        ev = []
        for kind, t, val, dur, io in events:
            t = float(t)
            if kind == "bolus":
                val = val * sub["scale"]
                if lag is not None and int(io) == lag["input"]:
                    t = t + float(theta[mdl["params"].index(lag["param"])])
            elif kind == "inf":
                val = val * sub["scale"]
            ev.append((kind, t, val, dur, io))
        ev.sort(key=lambda e: (e[1], RANK[e[0]]))
        x = mp.matrix(n, 1)
        t = ev[0][1]
        infs = []
        built = {}  # wrong rules: step length -> constants; the previous step's constants
        prev = [None]

        def segment(x, a, b):
            tc = (b - a) if mode == "segment_dt" else b
            covs = covs_at(mdl, sub, o, tc, V)
            if stats is not None:
                stats["march"].append(("P", o, tc, covs))
            val = values_at(mdl, theta, covs, V)
            k = micro_of(kernel, [val[p] for p in names])
            if "first_propagator_of_a_length_reused" in V:
                k = built.setdefault((b - a, any(s <= a and b <= e for (s, e, _, _) in infs)), k)
            if "previous_step_constants" in V:
                k, prev[0] = (prev[0] or k), k
            if stats is not None:
                key = tuple(str(v) for v in k)
                if key not in stats["seen_k"]:
                    stats["seen_k"][key] = (kappa_of(structure, k), reference_singular(structure, k))
                kap, sing = stats["seen_k"][key]
                stats["kappa"] = max(stats["kappa"], kap)
                stats["singular"] = stats["singular"] or sing
            A, _ = rate_matrix(structure, k)
            rate = sum((mpf(v) / mpf(d) for (s, e, v, d) in infs if s <= a and b <= e), mpf(0))
            M = mp.matrix(n + 1, n + 1)
            for i in range(n):
                for j in range(n):
                    M[i, j] = A[i][j]
            M[central, n] = rate
            xb = mp.expm(M * (mpf(b) - mpf(a))) * mp.matrix([*x, 1])
            return mp.matrix([xb[i] for i in range(n)])

        for e in ev:
            te = e[1]
            if te > t:
                pts = sorted({t, te} | {en for (s, en, _, _) in infs if t < en < te})
                pts = [p for i, p in enumerate(pts) if i == 0 or abs(p - pts[i - 1]) >= 1e-12]
                if pts[-1] != te:
                    pts[-1] = te
                for a, b in zip(pts[:-1], pts[1:]):
                    x = segment(x, a, b)
                t = te
            if e[0] == "bolus":
                x[int(e[4])] += mpf(e[2])
            elif e[0] == "inf":
                infs.append((e[1], e[1] + e[3], e[2], e[3]))  # end time in double
            else:
                tv = (t - prev_t(ev, e)) if "volume_at_derive_time" in V and mode == "segment_dt" else te
                covs = covs_at(mdl, sub, o, tv, V)
                if stats is not None:
                    stats["march"].append(("O", o, te, covs))
                preds.append(x[central] / values_at(mdl, theta, covs, V)[mdl["vol"]])
    return preds


def prev_t(ev, e):
    """The time of the event before observation e (wrong rule: the volume read where the last derive was)."""
    i = ev.index(e)
    return ev[i - 1][1] if i else e[1]


def rel(a, b):
    scale = max(abs(v) for v in b)
    return float(max(abs(x - y) for x, y in zip(a, b)) / scale)


# --------------------------------------------------------------------------------------------------------- groups
def obs(*ts):
    return [["obs", float(t), 0.0, 0.0, 0] for t in ts]


def B(t, amt, io=0):
    return ["bolus", float(t), float(amt), 0.0, io]


def I(t, amt, dur, io=0):
    return ["inf", float(t), float(amt), float(dur), io]


def POW(cov, ref=70.0, coef=0.75):
    return ["pow", cov, ref, coef]


def LIN(cov, ref=90.0, coef=0.004):
    return ["lin", cov, ref, coef]


def spread(base, s, step, k0=2):
    """Subject s's knot values: the base values moved by small dyadic amounts, different for every subject and knot."""
    return [b + step * (((s + 1) * (k + k0)) % 7 - 3) + step * 0.5 * s for k, b in enumerate(base)]


def subjects(cells):
    """cells(s) -> per-occasion {name: (times, values)} for subject s; stored as {name: [[times], [values]]}."""
    out = []
    for s in range(9):
        cov = [{n: [[float(a) for a in ts], [float(b) for b in vs]] for n, (ts, vs) in occ.items()} for occ in cells(s)]
        out.append({"scale": SCALES[s], "cov": cov})
    return out


WT_T, WT_V = [0.0, 6.0, 20.0, 40.0], [60.0, 75.0, 90.0, 70.0]
THREE_ABS = ["ka", "k10", "k12", "k13", "k21", "k31"]
EASY = {"three_compartments_with_absorption": [1.5, 0.2, 0.6, 0.3, 0.4, 0.05], "three_compartments": [0.2, 0.6, 0.3, 0.4, 0.05],
        "two_compartments": [0.2, 0.6, 0.3], "two_compartments_with_absorption": [0.2, 1.5, 0.6, 0.3],
        "one_compartment": [0.2], "one_compartment_with_absorption": [1.5, 0.2], "two_compartments_cl": [1.0, 2.0, 10.0, 20.0]}


def thetas(kernel, extra=()):
    """Three parameter vectors: the easy one and two others in the well-conditioned region, + the volume (+ extra)."""
    base = EASY[kernel]
    out = []
    for j, (f, v) in enumerate(((1.0, 20.0), (1.3, 8.0), (0.7, 35.0))):
        th = [b * f * (1.0 + 0.11 * ((i * (j + 1)) % 3) * (j > 0)) for i, b in enumerate(base)]
        out.append(th + ([] if kernel == "two_compartments_cl" else [v]) + [e[j] for e in extra])
    return out


def model(kernel, mode, params, derived, covariates, vol="v", kernel_params=None, lag=None, fixed=()):
    m = dict(kernel=kernel, mode=mode, params=params, derived=derived, covariates=covariates, fixed=list(fixed), vol=vol,
             kernel_params=kernel_params or KERNEL_PARAMS[kernel])
    if lag:
        m["lag"] = lag
    return m


KERNEL_PARAMS = {"one_compartment": ["ke"], "one_compartment_with_absorption": ["ka", "ke"], "two_compartments": ["ke", "kcp", "kpc"],
                 "two_compartments_with_absorption": ["ke", "ka", "kcp", "kpc"], "three_compartments": ["k10", "k12", "k13", "k21", "k31"],
                 "three_compartments_with_absorption": THREE_ABS, "two_compartments_cl": ["cl", "q", "vc", "vp"]}


def analytical_groups():
    groups = []
    step_wt = lambda s: [{"wt": (WT_T, spread(WT_V, s, 2.5))}]  # noqa: E731
    # a: a carry-forward covariate through dyn3; equal step lengths on both sides of the jumps at 6 and 20
    for mode in ("segment_dt", "segment_end_abs"):
        groups.append(dict(
            name=f"a_dyn3_step_{mode}",
            model=model("three_compartments_with_absorption", mode, ["ka", "k10_0", "k12", "k13", "k21", "k31", "v"],
                        {"k10": ["k10_0", [POW("wt")]]}, ["wt"], fixed=["wt"]),
            occasions=[[B(0, 200, 0), B(24, 150, 1)] + obs(2, 4, 8, 10, 12, 16, 22, 24, 48)],
            subjects=subjects(step_wt), thetas=thetas("three_compartments_with_absorption")))
    # b: a carry-forward covariate with an infusion whose end (8) lies between the jump at 6 and the next event (10)
    for kernel, mode, elim in (("three_compartments", "segment_end_abs", "k10"), ("two_compartments", "segment_dt", "ke")):
        names = [p + "_0" if p == elim else p for p in KERNEL_PARAMS[kernel]]
        groups.append(dict(
            name=f"b_step_infusion_{kernel}", model=model(kernel, mode, names + ["v"], {elim: [elim + "_0", [POW("wt")]]}, ["wt"],
                                                              fixed=["wt"]),
            occasions=[[B(0, 100, 0), I(5, 120, 3, 0)] + obs(1, 4, 10, 12, 18, 30)],
            subjects=subjects(step_wt), thetas=thetas(kernel)))
    # c: two or three covariates, up to four derived values, a derived volume
    three = lambda s: [{"wt": ([0.0, 8.0, 24.0], spread([60.0, 76.0, 68.0], s, 1.0)),  # noqa: E731
                        "crcl": ([0.0, 16.0, 48.0], spread([80.0, 110.0, 60.0], s, 2.0, 3)),
                        "age": ([0.0, 12.0], spread([40.0, 55.0], s, 0.5, 4))}]
    for mode in ("segment_dt", "segment_end_abs"):
        groups.append(dict(
            name=f"c_three_abs_four_derived_{mode}",
            model=model("three_compartments_with_absorption", mode, ["ka_0", "k10_0", "k12_0", "k13", "k21", "k31", "v_0"],
                        {"k10": ["k10_0", [POW("wt"), LIN("crcl")]], "k12": ["k12_0", [LIN("wt", 70.0, 0.01)]],
                         "ka": ["ka_0", [POW("age", 40.0, -0.3)]], "v": ["v_0", [POW("wt", 70.0, 1.0)]]}, ["wt", "crcl", "age"], fixed=["age"]),
            occasions=[[B(0, 200, 0), B(12, 150, 1)] + obs(1, 4, 8, 12, 20, 36)],
            subjects=subjects(three), thetas=thetas("three_compartments_with_absorption")))
    groups.append(dict(
        name="c_one_abs_three_derived",
        model=model("one_compartment_with_absorption", "segment_dt", ["ka_0", "ke_0", "v_0"],
                    {"ke": ["ke_0", [POW("wt"), LIN("crcl")]], "ka": ["ka_0", [POW("age", 40.0, -0.3)]],
                     "v": ["v_0", [POW("wt", 70.0, 1.0)]]}, ["wt", "crcl", "age"], fixed=["age"]),
        occasions=[[B(0, 200, 0), B(12, 150, 1)] + obs(1, 2, 4, 12, 36)],
        subjects=subjects(three), thetas=thetas("one_compartment_with_absorption")))
    two = lambda s: [{k: v for k, v in three(s)[0].items() if k != "age"}]  # noqa: E731
    groups.append(dict(
        name="c_two_cl_three_derived",
        model=model("two_compartments_cl", "segment_end_abs", ["cl_0", "q_0", "vc_0", "vp"],
                    {"cl": ["cl_0", [POW("wt"), LIN("crcl")]], "q": ["q_0", [LIN("wt", 70.0, 0.01)]],
                     "vc": ["vc_0", [POW("wt", 70.0, 1.0)]]}, ["wt", "crcl"], vol="vc"),
        occasions=[[B(0, 100, 0), I(5, 120, 3, 0)] + obs(1, 4, 10, 12, 36)],
        subjects=subjects(two), thetas=thetas("two_compartments_cl")))
    # d: knot edges.  First knot (2) after the first dose and two observations; an observation on the linear knot at 4,
    # an observation and a dose on the fixed knot at 8; last knots (12, 8) well before the last observation; step
    # lengths 0.5, 1 (below the first knot), 2, 4, 8 (on a knot), 22 (past the last)
    edge = lambda s: [{"wt": ([2.0, 4.0, 12.0], spread([60.0, 76.0, 68.0], s, 1.0)),  # noqa: E731
                       "crcl": ([2.0, 8.0], spread([80.0, 110.0], s, 2.0, 3))}]
    for kernel, mode in (("one_compartment", "segment_dt"), ("two_compartments_with_absorption", "segment_end_abs")):
        names = [p + "_0" if p == "ke" else p for p in KERNEL_PARAMS[kernel]]
        gut = kernel.endswith("absorption")
        groups.append(dict(
            name=f"d_knot_edges_{kernel}",
            model=model(kernel, mode, names + ["v_0"], {"ke": ["ke_0", [POW("wt"), LIN("crcl")]], "v": ["v_0", [POW("wt", 70.0, 1.0)]]},
                        ["wt", "crcl"], fixed=["crcl"]),
            occasions=[[B(0, 200, 0), B(8, 150, 1 if gut else 0)] + obs(0.5, 1, 3, 4, 8, 10, 18, 40)],
            subjects=subjects(edge), thetas=thetas(kernel)))

    # e: two occasions; the second has other knots, its first knot after its first event; subject 4's holds single knots;
    # odd subjects have their own knot times in it
    def occasions_two(s):
        second = {"wt": ([1.0, 5.0 + 4.0 * (s % 2)], spread([90.0, 64.0], s, 1.0)), "crcl": ([2.0, 6.0], spread([60.0, 100.0], s, 2.0, 3))}
        if s == 4:
            second = {"wt": ([3.0], [83.0]), "crcl": ([2.0], [71.0])}
        return [{"wt": ([0.0, 8.0, 16.0], spread([60.0, 76.0, 68.0], s, 1.0)), "crcl": ([0.0, 4.0], spread([80.0, 110.0], s, 2.0, 3))},
                second]
    groups.append(dict(
        name="e_two_occasions",
        model=model("one_compartment_with_absorption", "segment_end_abs", ["ka", "ke_0", "v_0"],
                    {"ke": ["ke_0", [POW("wt"), LIN("crcl")]], "v": ["v_0", [POW("wt", 70.0, 1.0)]]}, ["wt", "crcl"], fixed=["crcl"]),
        occasions=[[B(0, 200, 0)] + obs(1, 4, 8, 12), [B(0, 150, 0)] + obs(0.5, 2, 6, 10)],
        subjects=subjects(occasions_two), thetas=thetas("one_compartment_with_absorption")))
    # f: a lagged input together with covariate-derived constants (runs on the generated source)
    groups.append(dict(
        name="f_lag_with_derived",
        model=model("one_compartment_with_absorption", "segment_dt", ["ka", "ke_0", "v_0", "tlag"],
                    {"ke": ["ke_0", [POW("wt")]], "v": ["v_0", [POW("wt", 70.0, 1.0)]]}, ["wt"], lag={"input": 0, "param": "tlag"}),
        occasions=[[B(0, 200, 0), B(12, 150, 1), B(24, 100, 0)] + obs(0.25, 2, 6, 13, 25, 36)],
        subjects=subjects(lambda s: [{"wt": ([0.0, 8.0, 24.0], spread([60.0, 76.0, 68.0], s, 1.0))}]),
        thetas=thetas("one_compartment_with_absorption", extra=[(0.0, 0.37, 1.25)])))
    return groups


def build_analytical(group):
    mdl = group["model"]
    n_cases = len(group["thetas"])
    kappa, sing = [mpf(1)] * n_cases, [0] * n_cases
    seen_k = {}
    truth = []  # [subject][case] -> mpf list
    march0 = None
    for s, sub in enumerate(group["subjects"]):
        rows, cov_rows = [], None
        for c, th in enumerate(group["thetas"]):
            st = dict(kappa=mpf(1), singular=0, march=[], seen_k=seen_k)
            rows.append(simulate(group, sub, th, stats=st))
            kappa[c], sing[c] = max(kappa[c], st["kappa"]), sing[c] or st["singular"]
            if c == 0:
                cov_rows = st["march"]
        truth.append(rows)
        sub["expected"] = [[float(mp.nstr(v, 13)) for v in r] for r in rows]
        if "lag" not in mdl:  # (the march of a lagged model depends on theta; its model reads the knots on the device)
            key = [(k, o, t) for k, o, t, _ in cov_rows]
            march0 = march0 or key
            assert key == march0
            seen = sorted({(o, t) for _, o, t in key})
            group["seen"] = [[o, t] for o, t in seen]
            group["march"] = [[k, seen.index((o, t))] for k, o, t in key]
            at = {(o, t): cv for _, o, t, cv in cov_rows}
            sub["cov_seen"] = [[float(v) for v in at[ot]] for ot in seen]
    cases = []
    for c, th in enumerate(group["thetas"]):
        assert 64 * U * kappa[c] <= 1e-10 and sing[c] == 0, (group["name"], c, float(kappa[c]))
        cases.append(dict(theta=[float(v) for v in th], kappa=float(kappa[c]), singular=sing[c]))
    bars = [max(1e-10, 64 * U * float(k)) for k in kappa]
    # any two subjects >= 1000 bars apart on some case (per unit dose)
    for i in range(9):
        for j in range(i + 1, 9):
            far = max(rel([v / group["subjects"][i]["scale"] for v in truth[i][c]], [v / group["subjects"][j]["scale"] for v in truth[j][c]]) / bars[c]
                      for c in range(n_cases))
            assert far >= 1000, (group["name"], i, j, far)
    # deliberately wrong rules
    for rule, prefixes in WRONG.items():
        if not group["name"].startswith(prefixes):
            continue
        moved = max(rel(simulate(group, sub, th, V=(rule,)), truth[s][c]) / bars[c]
                    for s, sub in list(enumerate(group["subjects"]))[:3] for c, th in enumerate(group["thetas"]))
        print(f"  wrong rule {rule:40s} moves {group['name']} by {moved:.3g} bars", flush=True)
        group.setdefault("moved", {})[rule] = moved
    out = {k: group[k] for k in ("name", "model", "occasions", "subjects") if k in group}
    out.update(kind="analytical", cases=cases, **({k: group[k] for k in ("seen", "march")} if "seen" in group else {}))
    return out, group.get("moved", {})


# -------------------------------------------------------------------------------------------------------------- ODE
H_MAX = 0.0625


def dyadic(t):
    return float(t) * 64.0 == math.floor(float(t) * 64.0) and abs(float(t)) < 2.0 ** 20


def ode_params(mdl, theta, sub, t, V=()):
    """The body's parameter vector at time t (mpf): derived entries rebuilt from the covariates at t."""
    val = values_at(mdl, theta, covs_at(mdl, sub, 0, t, V), V)
    return [val[p] for p in mdl["body_params"]], val[mdl["vol"]]


def knot_times(sub):
    return sorted({t for cell in sub["cov"] for c in cell.values() for t in c[0]})


def ode_walk(group, theta, kind, V=()):
    """kind 'rk4': exact-arithmetic RK4 steps (-> predictions, n_steps, kappa); 'exact': matrix exponentials between the
    jumps of carry-forward covariates."""
    mdl, sub = group["model"], group["subject"]
    body = mdl["body"]
    ns, _, central = BODIES[body]
    th = [float(v) for v in theta]
    lag = {k: mdl["params"].index(p) for k, p in mdl["lag"].items()}
    ev, extra = rewrite(group["occasions"][0], lag, {}, th)
    x = [mpf(0)] * ns
    # The solver clock starts at the earliest RECORDED time and the first event of the rewritten list acts at the clock as
    # it stands (ode/mod.rs:348, 639-721: the event acts, then the solver advances to the NEXT event): a lagged bolus that
    # is still the first event acts at the initial time.  Case g_one_cmt_oral_fixed_lag[1] pins it (lag 1/8, first
    # observation at 1/4): an earlier version of this march started at the landing time and the oracle, which follows
    # the reference, disagreed by 15 %.
    t = min(float(e[1]) for e in group["occasions"][0])
    active, out = [], []
    n_steps, x_max, lam = 0, mpf(0), mpf(0)
    frozen = "covariates_frozen_at_step_start" in V
    for i, (te, kind_e, val, dur, io) in enumerate(ev):
        while i and t < te:
            nxt = min([te] + [b for b in extra if t < b < te])
            rates = [mpf(0)] * mdl["ndrugs"]
            for (end, rate, inp) in active:
                if end > t:
                    rates[inp] += mpf(rate)
            b = rate_vector(body, rates)
            if kind == "rk4":
                n, h = step_count(t, nxt, group["h_max"])
                assert dyadic(t) and dyadic(nxt) and dyadic(h / 2) and h == group["h_max"], (t, nxt, h)
                for j in range(n):
                    tj = mpf(t) + j * mpf(h)

                    def f(ts, xs, tj=tj):
                        p, _ = ode_params(mdl, th, sub, tj if frozen else ts, V)
                        A = matrix_of(body, p)
                        return [sum((A[i][k] * xs[k] for k in range(ns)), mpf(0)) + b[i] for i in range(ns)]
                    p0, _ = ode_params(mdl, th, sub, tj)
                    lam = max(lam, lambda_max(body, p0))
                    x, _ = erk_step(RK4, f, tj, x, mpf(h))
                    n_steps += 1
                    x_max = max([x_max] + [abs(v) for v in x])
            else:
                cuts = [t] + [k for k in knot_times(sub) if t < k < nxt] + [nxt]
                for a, c in zip(cuts[:-1], cuts[1:]):
                    p, _ = ode_params(mdl, th, sub, a)
                    A = matrix_of(body, p)
                    M = mp.matrix(ns + 1, ns + 1)
                    for i in range(ns):
                        for k in range(ns):
                            M[i, k] = A[i][k]
                        M[i, ns] = b[i]
                    xb = mp.expm(M * (mpf(c) - mpf(a))) * mp.matrix([*x, 1])
                    x = [xb[i] for i in range(ns)]
            t = nxt
        if kind_e == "obs":
            out.append((x[central], ode_params(mdl, th, sub, te)[1]))
        elif kind_e == "bolus":
            x = list(x)
            x[int(io)] += mpf(val)
            x_max = max(x_max, abs(x[int(io)]))
        else:
            active.append((te + dur, val / dur, int(io)))
    pred = [a / v for a, v in out]
    if kind != "rk4":
        return pred
    assert stability(4, -lam * mpf(group["h_max"])) <= 1
    kappa = float(n_steps * mp.exp(lam * mpf(group["h_max"])) * x_max / max(abs(a) for a, _ in out))
    return pred, n_steps, kappa


def ode_groups():
    # knots: 17/32 = a stage time t + h/2 (t = 1/2, h = 1/16); 1 + 3/64 strictly inside a step, on no stage time; 2 = a piece
    # boundary (an observation)
    groups = []
    for body, names, sched, ths, lag in (
            ("one_cmt_oral", ["ka", "ke_0", "v_0", "tlag"],
             [B(0, 100, 0), I(1.0, 40, 0.5, 0)] + obs(0.25, 0.5, 1, 1.25, 2, 2.5, 3),
             [[1.1, 0.3, 20.0, 0.25], [14.0, 2.0, 15.0, 0.125], [3.0, 5.0, 30.0, 0.375]], {"0": "tlag"}),
            ("two_cmt_iv", ["ke_0", "kcp", "kpc", "v_0"],
             [B(0, 100, 0), I(1.0, 40, 0.5, 0)] + obs(0.25, 0.5, 1, 1.25, 2, 2.5, 3),
             [[0.2, 0.5, 0.3, 25.0], [7.0, 6.0, 3.0, 10.0], [10.0, 3.0, 8.0, 10.0]], {})):
        for fixed in (False, True):
            body_params = ["ke" if p == "ke_0" else p for p in names if p not in ("v_0", "tlag")]
            mdl = dict(body=body, params=names, body_params=body_params, vol="v", covariates=["wt", "crcl"], fixed=["wt", "crcl"] if fixed else [], ndrugs=1,
                       lag=lag if fixed else {},
                       derived={"ke": ["ke_0", [POW("wt"), LIN("crcl")]], "v": ["v_0", [POW("wt", 70.0, 1.0)]]})
            sub = {"cov": [{"wt": [[0.0, 0.53125, 2.0], [60.0, 82.0, 71.0]], "crcl": [[0.0, 1.046875], [80.0, 115.0]]}]}
            name = f"g_{body}_{'fixed' if fixed else 'linear'}" + ("_lag" if fixed and lag else "")
            groups.append(dict(name=name, kind="ode", scalable=True, model=mdl, h_max=H_MAX, occasions=[sched], subject=sub, thetas=ths))
    return groups


def build_ode(group):
    fixed = bool(group["model"]["fixed"])
    for e in group["occasions"][0]:
        assert dyadic(e[1]) and dyadic(e[3])
    assert all(dyadic(t) for t in knot_times(group["subject"])) and dyadic(group["h_max"])
    cases, moved = [], 0.0
    for th in group["thetas"]:
        assert all(dyadic(th[group["model"]["params"].index(p)]) for p in group["model"]["lag"].values())
        pred, n_steps, kappa = ode_walk(group, th, "rk4")
        assert 64 * U * kappa <= 1e-11, (group["name"], th, kappa)
        case = dict(theta=[float(v) for v in th], rk4=[float(v) for v in pred], n_steps=n_steps, kappa=kappa)
        if fixed:
            case["exact"] = [float(v) for v in ode_walk(group, th, "exact")]
        else:
            wrong, _, _ = ode_walk(group, th, "rk4", V=("covariates_frozen_at_step_start",))
            moved = max(moved, rel(wrong, pred) / (64 * U * kappa))
        cases.append(case)
    out = {k: group[k] for k in ("name", "kind", "scalable", "model", "h_max", "occasions", "subject")}
    out["cases"] = cases
    if fixed:
        # (h) the adaptive solvers against the true solution at the tolerances of ode_exact.json.  A step that ends on a
        # jump reads the value after it in its last stages (c = 1), and a step across a jump is judged by an estimate that
        # does not see it.  Measured on the oracle's DOPRI5, which does not end steps at knots: the fixed-step subject's
        # jumps cost 20 to 150 tol inside a piece; on piece boundaries jumps of 26 %, 7 %, 3 % and 1 % at two or three knots
        # all cost 5 to 35 tol on the faster cases (the cost does not go with the size of the jump: the controller shrinks
        # the step until the estimate passes).  The cap on the inputs of an adaptive check is 10 tol, so "dopri5" runs on
        # the easy case with one knot on a piece boundary (the observation at 2) and a jump of 1 % (measured 1.4 to 4.8 tol).
        # "ros2" and "auto" (which ends its steps at knots) also run on the fixed-step subject's knots (`interior`, the
        # cases listed, truth = their `exact`).
        sub = {"cov": [{"wt": [[0.0, 2.0], [60.0, 60.75]], "crcl": [[0.0], [80.0]]}]}
        ad = dict(group, subject=sub)
        out["adaptive"] = dict(h_max=4.0, tols=[1e-6, 1e-9], subject=sub, interior=[0],
                               cases=[dict(theta=[float(v) for v in th], exact=[float(v) for v in ode_walk(ad, th, "exact")])
                                      for th in group["thetas"][:1]])
    else:
        print(f"  wrong rule {'covariates_frozen_at_step_start':40s} moves {group['name']} by {moved:.3g} bars", flush=True)
    return out, ({} if fixed else {"covariates_frozen_at_step_start": moved})


def main():
    out, moved = [], {}
    for group in analytical_groups():
        print(group["name"], flush=True)
        g, mv = build_analytical(group)
        out.append(g)
        for k, v in mv.items():
            moved[k] = max(moved.get(k, 0.0), v)
    for group in ode_groups():
        print(group["name"], flush=True)
        g, mv = build_ode(group)
        out.append(g)
        for k, v in mv.items():
            moved[k] = max(moved.get(k, 0.0), v)
    for rule in WRONG:
        assert moved.get(rule, 0.0) >= 1000, (rule, moved.get(rule))
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/gen_covariates.py", "mp_dps": 40, "groups": out}, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {len(out)} groups to {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) <= os.path.getsize(os.path.join(HERE, "loglik_terms.json"))  # (the largest fixture so far)


if __name__ == "__main__":
    main()
