#!/usr/bin/env python3
"""Generate tests/golden/loglik_terms.json: every kind of log-likelihood term at its edges, as exact mathematics
(mpmath, 40 digits).  Neither the oracle nor the product is imported; the rules are the reference's, restated:

  lognormpdf / lognormcdf / lognormccdf     likelihood/distributions.rs:31-103
      pdf  = -ln(2 pi)/2 - ln sigma - (obs - f)^2 / (2 sigma^2)
      BLOQ = ln cdf, cdf = erfc((f - obs) / (sigma sqrt 2)) / 2; where cdf <= 0: pdf - ln|z| if z < -37, else Err
      ALOQ = ln(1 - cdf);                                 where 1 - cdf <= 0: pdf - ln z   if z >  37, else Err
      (Normal::new rejects sigma <= 0: Err)
  AssayErrorModel::sigma                     error_model.rs:1045-1080
      alpha = c0 + c1 y + c2 y^2 + c3 y^3 with the OBSERVATION y and the observation's own polynomial if it has one;
      additive: sqrt(alpha^2 + lambda^2), proportional: gamma alpha; negative or non-finite sigma: Err
  ResidualErrorModel::sigma, log_likelihood   residual_error.rs:178-191, 265-271
      sigma from the PREDICTION f: a | b |f| | sqrt(a^2 + b^2 f^2) | sigma_exp, floored at sqrt(f64::EPSILON);
      term = -(ln(2 pi) + 2 ln sigma + ((obs - f) / sigma)^2) / 2
  Prediction::log_likelihood                 prediction.rs:105-125
      a missing observation contributes 0 whatever f is; a non-finite term is an Err.

Every term sits on a prediction that is exact by construction: f = 0 (an observation before the first dose) or
f = 12.5 (an observation at the instant of a bolus of 100 into a central compartment of volume 8).  To put z where it
is wanted the row carries its own polynomial (sigma, 0, 0, 0) under an additive model with lambda = 0 and
obs = f + z sigma rounded to double; sigma, z, the term and its slope are then computed from the doubles stored.

Per term:  `bar`, the absolute error every double-precision implementation of the rules is held to on this term, and
`cond` = bar / 4, the error one rounding in what the term is computed from can cause (a term with cond > 1e-6 is
ill-conditioned; a subject holds at most one).  With u = 2^-53:
  plain      4 u (ln(2 pi)/2 + |ln sigma| + z^2 / 2): the parts of the term by magnitude, not |const| of their sum
             const = -ln(2 pi)/2 - ln sigma, which cancels to nothing near sigma = 0.399 while its rounding does not
  missing    0
  BLOQ       4 (ulp(cdf) / cdf + u |z dterm/dz| + u |term|): the rounding of cdf itself (ulp = the spacing of doubles at
             cdf, denormals included), the roundings on the way to erfc's argument (the subtraction, 1/(sigma sqrt 2),
             the product: each moves z by u relatively), and the rounding of the logarithm.  The first part alone is
             below the spacing of doubles at the term from |z| = 2 on (ln cdf = -700 at z = -37.4 has spacing 1e-13),
             so it cannot be the whole bar.
  ALOQ       4 (2^-53 / sf + u |z dterm/dz| + u |term|): 1 - cdf is formed from a cdf next to 1, spacing 2^-53
  asymptote  4 u |term|
  residual   4 u (ln(2 pi)/2 + |ln sigma| + z^2)
  failing    status only
`dterm_df` = |d term / d f| and `slope`, the same with its sign.
The factor 4: the reference's erfc (statrs, not vendored) is only known to be good to ~1e-15.

`expect`: "ok" (finite, within the bar), "err" (the pair is flagged, its sum NaN) or "either".  The bands rest on the
exact cdf and sf, not on an implementation:
  BLOQ  ok: cdf is a normal double (>= 2^-1022).  either: cdf is denormal (an erfc that flushes it to 0 takes the
        asymptote, `alt`; one that keeps it takes ln cdf).  asymptote (ok): cdf < 2^-1075 rounds to 0 for everybody.
  ALOQ  ok: sf >= 2^-51, four spacings of the doubles below 1: a cdf one spacing off still leaves 1 - cdf >= 3 spacings,
        and the bar stays below 1.  err: sf <= 2^-55.9 and z <= 37: cdf rounds to 1 unless erfc is more than a third
        of a spacing off.  either: between.  z > 37: the asymptote (ok).
        (The ladder's rungs at z = 8.0, sf = 2^-50.51, and z = 8.45, sf = 2^-55.93, fix these two thresholds.)

`later`: the rows behind the two exact ones, after real propagation: one-compartment IV, f = 12.5 exp(-ke (t - 1)) for
the lanes' ke, plain rows (or residual ones) with |z| <= 2 under each model, in `variants` of the schedule (same
program, other step lengths).  `populations`: which terms each subject's two exact rows carry.

Run:  python tests/golden/gen_loglik_terms.py     (deterministic)
"""
import json
import math
import os

import mpmath as mp

mp.mp.dps = 40
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "loglik_terms.json")

U = mp.mpf(2) ** -53
LN2PI = mp.log(2 * mp.pi)
SQRT_EPS = mp.sqrt(mp.mpf(2) ** -52)
F0, F1 = 0.0, 12.5
DOSE, VOL = 100.0, 8.0
T_PRE, T_DOSE, T_AT = 0.0, 1.0, 1.0 + 2.0 ** -41  # (closer than the solve's 1e-12 dedup: no propagation in between)
# (six: with at most three subjects each no exact class reaches the planner's minimum, the population is one loose class)
VARIANTS = [[2.0, 3.5, 6.0], [2.5, 4.25, 7.0], [3.0, 5.0, 8.5], [2.25, 3.75, 6.5], [2.75, 4.5, 7.5], [2.125, 4.0, 6.25]]
KE = [0.1, 0.105, 0.115, 0.125]
LATER_SCALE = [1.02, 0.9, 0.88]  # later observation r = f(ke[0], variant 0, r) times this, rounded to 6 decimals

CUBIC = [0.3, 0.08, 0.004, 0.0002]  # positive for y >= 0, negative at y = -8
MODELS = {
    "add0": {"kind": "additive", "c": CUBIC, "scalar": 0.0},
    "addl": {"kind": "additive", "c": CUBIC, "scalar": 0.1},
    "prop": {"kind": "proportional", "c": CUBIC, "scalar": 1.3},
    "res_const": {"kind": "res_constant", "a": 0.7, "b": 0.0},
    "res_prop": {"kind": "res_proportional", "a": 0.2, "b": 0.0},
    "res_comb": {"kind": "res_combined", "a": 0.5, "b": 0.15},
    "res_comb0": {"kind": "res_combined", "a": 0.0, "b": 0.15},
    "res_exp": {"kind": "res_exponential", "a": 0.35, "b": 0.0},
}
ASSAY = ("add0", "addl", "prop")
RESIDUAL = ("res_const", "res_prop", "res_comb", "res_comb0", "res_exp")


def D(x):
    return mp.mpf(float(x))


def fl(x):
    return float(x)


def ulp(p):
    """Spacing of the doubles at p > 0 (denormals included)."""
    if p < mp.mpf(2) ** -1022:
        return mp.mpf(2) ** -1074
    return mp.mpf(2) ** (int(mp.floor(mp.log(p, 2))) - 52)


def assay_sigma(model, poly, y):
    """(sigma, failure or None) for an observed value y (a double)."""
    c = poly if poly is not None else model["c"]
    if any(not math.isfinite(v) for v in c):
        return None, "NonFiniteSigma"
    c0, c1, c2, c3 = (D(v) for v in c)
    y = D(y)
    alpha = c0 + c1 * y + c2 * y ** 2 + c3 * y ** 3
    s = mp.sqrt(alpha ** 2 + D(model["scalar"]) ** 2) if model["kind"] == "additive" else D(model["scalar"]) * alpha
    if s < 0:
        return None, "NegativeSigma"
    return s, None


def residual_sigma(model, f):
    """(sigma, d sigma / d f) from the prediction."""
    a, b, f = D(model["a"]), D(model["b"]), D(f)
    kind = model["kind"]
    if kind == "res_proportional":
        raw, slope = a * abs(f), a * mp.sign(f)
    elif kind == "res_combined":
        raw = mp.sqrt(a ** 2 + b ** 2 * f ** 2)
        slope = b ** 2 * f / raw if raw > 0 else mp.mpf(0)
    else:
        raw, slope = a, mp.mpf(0)
    return (raw, slope) if raw >= SQRT_EPS else (SQRT_EPS, mp.mpf(0))


def norm_tail(z):
    """P(X <= z) for the standard normal, exact at any z."""
    return mp.erfc(-z / mp.sqrt(2)) / 2


def phi(z):
    return mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)


def plain_parts(obs, f, s):
    z = (D(obs) - D(f)) / s
    const = -LN2PI / 2 - mp.log(s)
    return z, const, const - z * z / 2


def term_record(name, model_name, kind, f, obs, poly=None, censor=0, expect=None):
    """One term on an exact prediction f; `expect` given = the ladder's own label, checked against the bands."""
    model = MODELS[model_name]
    rec = {"name": name, "model": model_name, "kind": kind, "f": f, "obs": obs, "poly": poly, "censor": censor,
           "sigma": None, "z": None, "term": None, "alt": None, "dterm_df": 0.0, "slope": 0.0, "cond": 0.0, "bar": 0.0, "expect": "ok"}
    if kind == "missing":
        rec["term"] = 0.0
        return rec
    if kind == "residual":
        s, ds = residual_sigma(model, f)
        r = D(obs) - D(f)
        z = r / s
        term = -(LN2PI + 2 * mp.log(s) + z * z) / 2
        slope = -ds / s + r / s ** 2 + r * r * ds / s ** 3
        bar = 4 * U * (LN2PI / 2 + abs(mp.log(s)) + z * z)
        rec.update(sigma=fl(s), z=fl(z), term=fl(term), dterm_df=fl(abs(slope)), slope=fl(slope), bar=fl(bar), cond=fl(bar / 4))
        return rec
    s, failure = assay_sigma(model, poly, obs)
    if failure or (censor != 0 and s == 0):
        rec.update(kind="failing", expect="err", sigma=None if failure else 0.0)
        return rec
    z, const, pdf = plain_parts(obs, f, s)
    rec.update(sigma=fl(s), z=fl(z))
    if censor == 0:
        bar = 4 * U * (LN2PI / 2 + abs(mp.log(s)) + z * z / 2)
        rec.update(term=fl(pdf), dterm_df=fl(abs(z) / s), slope=fl(z / s), bar=fl(bar), cond=fl(bar / 4))
        return rec
    asym_rec = None
    if abs(z) > 37:  # the reference's asymptote, evaluated exactly (it carries lognormpdf's -ln sigma)
        asym = pdf - mp.log(abs(z))
        asym_rec = dict(term=fl(asym), dterm_df=fl(abs(z + 1 / z) / s), slope=fl((z + 1 / z) / s), bar=fl(4 * U * abs(asym)), cond=fl(U * abs(asym)))
    if censor > 0:  # BLOQ
        p = norm_tail(z)
        band = "ok" if p >= mp.mpf(2) ** -1022 else ("either" if p >= mp.mpf(2) ** -1075 else "asym")
        spacing = ulp(p) / p
    else:  # ALOQ
        p = norm_tail(-z)
        band = ("asym" if z > 37 else "ok" if p >= mp.mpf(2) ** -51 else "err" if p <= mp.mpf(2) ** mp.mpf("-55.9") else "either")
        spacing = U / p
    if band == "asym":
        assert (z < -37) if censor > 0 else (z > 37)
        rec.update(asym_rec, kind=kind + "_asymptote")
        band = "ok"
    else:
        term = mp.log(p)
        dz = phi(z) / p  # |d term / d z|
        bar = 4 * (spacing + U * abs(z) * dz + U * abs(term))
        rec.update(term=fl(term), dterm_df=fl(dz / s), slope=fl((-dz if censor > 0 else dz) / s), bar=fl(bar), cond=fl(bar / 4))
        if band == "either" and censor > 0:
            rec["alt"] = asym_rec["term"]
        if band == "err":
            rec.update(term=None, dterm_df=0.0, slope=0.0, bar=0.0, cond=0.0)
    rec["expect"] = band
    assert expect is None or expect == band, (name, expect, band, mp.nstr(mp.log(p, 2), 8))
    return rec


TERMS = {}


def add(rec):
    key = f"{rec['name']}@{rec['model']}"
    assert key not in TERMS, key
    TERMS[key] = rec
    return rec["name"]


def rung(name, kind, f, z, sigma, censor=0, expect=None, model="add0"):
    """A term at a wanted z: its own polynomial (sigma, 0, 0, 0) under additive, lambda = 0."""
    obs = fl(D(f) + D(z) * D(sigma))
    return add(term_record(name, model, kind, f, obs, [sigma, 0.0, 0.0, 0.0], censor, expect))


def tag(z):
    return ("m" if z < 0 else "p") + f"{abs(z):g}".replace(".", "_")


def build_terms():
    pick = {}  # rung name -> f, chosen by the populations below
    sig_cycle = [0.5, 2.0, 0.8, 1.25]
    n = [0]

    def sig():
        n[0] += 1
        return sig_cycle[n[0] % 4]

    def ladder(prefix, kind, censor, zs, expect, f_of, sigma=None):
        for z in zs:
            nm = f"{prefix}_{tag(z)}"
            rung(nm, kind, f_of[nm], z, sigma if sigma is not None else sig(), censor, expect)

    f_of = {
        # BLOQ ok
        "bloq_p6": F1, "bloq_p0": F1, "bloq_m1": F0, "bloq_m5": F0, "bloq_m20": F1, "bloq_m36_9": F0, "bloq_m37_1": F1,
        "bloq_m37_4": F0,
        # BLOQ either / asymptote
        "bloq_m37_6": F0, "bloq_m38": F1, "bloq_m38_3": F0, "bloq_m38_45": F1,
        "bloq_m38_6": F1, "bloq_m40": F0, "bloq_m400": F1,
        # ALOQ
        "aloq_m6": F1, "aloq_p0": F0, "aloq_p1": F0, "aloq_p3": F1, "aloq_p5": F0, "aloq_p6": F1, "aloq_p7": F1,
        "aloq_p7_5": F1, "aloq_p8": F0,
        "aloq_p8_15": F0, "aloq_p8_22": F1, "aloq_p8_29": F0,
        "aloq_p8_45": F1, "aloq_p9": F0, "aloq_p13": F1, "aloq_p36_9": F0,
        "aloq_p37_1": F0, "aloq_p40": F1, "aloq_p400": F0,
        # plain
        "plain_p0": F0, "plain_p1": F0, "plain_m1": F1, "plain_p30": F0, "plain_m30": F1, "plain_p400": F0,
    }
    ladder("bloq", "bloq", 1, [6, 0, -1, -5, -20, -36.9, -37.1, -37.4], "ok", f_of)
    ladder("bloq", "bloq", 1, [-37.6, -38.0, -38.3, -38.45], "either", f_of)
    ladder("bloq", "bloq", 1, [-38.6, -40, -400], "ok", f_of, sigma=0.25)  # sigma != 1: the carried -ln sigma shows
    ladder("aloq", "aloq", -1, [-6, 0, 1, 3, 5, 6, 7, 7.5, 8.0], "ok", f_of)
    ladder("aloq", "aloq", -1, [8.15, 8.22, 8.29], "either", f_of)
    ladder("aloq", "aloq", -1, [8.45, 9, 13, 36.9], "err", f_of)
    ladder("aloq", "aloq", -1, [37.1, 40, 400], "ok", f_of, sigma=0.25)
    ladder("plain", "plain", 0, [0, 1, -1, 30, -30, 400], "ok", f_of)
    rung("plain_sigma_1em8", "plain", F1, 1.0, 1e-8)
    rung("plain_sigma_1e8", "plain", F0, 1.0, 1e8)
    # sigma from a full cubic polynomial of the observation's own, y in {0.05, 3, 40}
    own = [0.2, 0.05, 0.003, 0.0001]
    add(term_record("plain_cubic_y0_05", "add0", "plain", F0, 0.05, own))
    add(term_record("plain_cubic_y3", "add0", "plain", F1, 3.0, own))
    add(term_record("plain_cubic_y40", "add0", "plain", F1, 40.0, own))
    add(term_record("missing_f0", "add0", "missing", F0, None))
    add(term_record("missing_f1", "add0", "missing", F1, None))
    # mild company for the hard rows of the failing population, and the plain rows of the 66-observation design
    rung("mild_f0", "plain", F0, 0.5, 0.6)
    rung("mild_f1", "plain", F1, -0.75, 1.5)
    add(term_record("long_f0", "add0", "plain", F0, 0.2))   # sigma from the model's cubic
    add(term_record("long_f1", "add0", "plain", F1, 12.0))
    # failing rows
    add(term_record("fail_nonfinite_coefficient", "add0", "plain", F0, 0.5, [0.5, math.inf, 0.0, 0.0]))
    add(term_record("fail_censored_sigma_zero", "add0", "bloq", F1, 12.0, [0.0, 0.0, 0.0, 0.0], 1))
    # sigma from the model, not the row: additive with lambda != 0, proportional with gamma != 1
    for mdl in ("addl", "prop"):
        for nm, kind, f, y, cz in [
                ("model_plain_y0_3", "plain", F0, 0.3, 0), ("model_plain_y11", "plain", F1, 11.0, 0),
                ("model_plain_y0_05", "plain", F0, 0.05, 0), ("model_plain_y40", "plain", F1, 40.0, 0),
                ("model_plain_y3", "plain", F1, 3.0, 0), ("model_plain_y12", "plain", F1, 12.0, 0),
                ("model_plain_y13", "plain", F1, 13.0, 0),
                ("model_bloq_ym0_4", "bloq", F0, -0.4, 1), ("model_bloq_y12_5", "bloq", F1, 12.5, 1),
                ("model_bloq_y0_5", "bloq", F0, 0.5, 1), ("model_bloq_y14", "bloq", F1, 14.0, 1),
                ("model_bloq_y0_1", "bloq", F0, 0.1, 1),
                ("model_aloq_y13", "aloq", F1, 13.0, -1), ("model_aloq_y0_2", "aloq", F0, 0.2, -1),
                ("model_aloq_y10_5", "aloq", F1, 10.5, -1), ("model_aloq_ym0_3", "aloq", F0, -0.3, -1),
                ("model_cubic_negative_ym8", "plain", F0, -8.0, 0),  # NegativeSigma under proportional only
                ("model_missing", "missing", F0, None, 0)]:
            rec = term_record(nm, mdl, kind, f, y, None, cz)
            assert rec["expect"] == ("err" if (mdl == "prop" and nm.endswith("ym8")) else "ok"), (nm, mdl, rec)
            assert kind not in ("bloq", "aloq") or abs(rec["z"]) < 4, (nm, mdl, rec["z"])
            add(rec)
    # residual models: sigma from the prediction; f = 0 engages the floor for proportional (and combined with a = 0)
    for mdl in RESIDUAL:
        for f, ftag in ((F0, "f0"), (F1, "f1")):
            s, _ = residual_sigma(MODELS[mdl], f)
            for z in (0, 2, 30):
                obs = fl(D(f) + z * s)
                add(term_record(f"res_{ftag}_z{z}", mdl, "residual", f, obs))
            # ... and a row with a polynomial of its own, which a residual model never reads
            add(term_record(f"res_{ftag}_poly", mdl, "residual", f, fl(D(f) + 2 * s), [0.7, 0.1, 0.0, 0.0]))
        add(term_record("res_missing", mdl, "missing", F0, None))
    assert fl(residual_sigma(MODELS["res_prop"], F0)[0]) == 1.4901161193847656e-08
    assert fl(residual_sigma(MODELS["res_comb0"], F0)[0]) == 1.4901161193847656e-08


def later_rows():
    """Rows after real propagation, per model / schedule variant / lane: exact f and the exact mild term."""
    f = [[[fl(D(F1) * mp.exp(-D(ke) * (D(t) - D(T_DOSE)))) for t in times] for ke in KE] for times in VARIANTS]
    fx = [[[D(F1) * mp.exp(-D(ke) * (D(t) - D(T_DOSE))) for t in times] for ke in KE] for times in VARIANTS]
    obs = [round(f[0][0][r] * LATER_SCALE[r], 6) for r in range(3)]
    out = {"f": f, "obs": obs, "models": {}}
    for mdl in MODELS:
        model = MODELS[mdl]
        terms, slopes, bars = [], [], []
        for v in range(len(VARIANTS)):
            tv, sv, bv = [], [], []
            for lane in range(len(KE)):
                tl, sl, bl = [], [], []
                for r in range(3):
                    pred = fx[v][lane][r]
                    if mdl in ASSAY:
                        s, failure = assay_sigma(model, None, obs[r])
                        assert failure is None
                        z = (D(obs[r]) - pred) / s
                        const = -LN2PI / 2 - mp.log(s)
                        term, slope, bar = const - z * z / 2, abs(z) / s, 4 * U * (LN2PI / 2 + abs(mp.log(s)) + z * z / 2)
                    else:
                        a, b = D(model["a"]), D(model["b"])
                        kind = model["kind"]
                        if kind == "res_proportional":
                            s, ds = a * pred, a
                        elif kind == "res_combined":
                            s = mp.sqrt(a * a + b * b * pred * pred)
                            ds = b * b * pred / s
                        else:
                            s, ds = a, mp.mpf(0)
                        assert s > SQRT_EPS
                        rr = D(obs[r]) - pred
                        z = rr / s
                        term = -(LN2PI + 2 * mp.log(s) + z * z) / 2
                        slope = abs(-ds / s + rr / s ** 2 + rr * rr * ds / s ** 3)
                        bar = 4 * U * (LN2PI / 2 + abs(mp.log(s)) + z * z)
                    assert mdl not in ASSAY or abs(z) <= 2, (mdl, v, lane, r, fl(z))
                    tl.append(fl(term))
                    sl.append(fl(slope))
                    bl.append(fl(bar))
                tv.append(tl)
                sv.append(sl)
                bv.append(bl)
            terms.append(tv)
            slopes.append(sv)
            bars.append(bv)
        out["models"][mdl] = {"term": terms, "dterm_df": slopes, "bar": bars}
    return out


# subject -> the terms of its two exact rows [row at f = 0, row at f = 12.5]
POPULATIONS = {
    # every ok and asymptote rung, at most one ill-conditioned term per subject.  Chunk 0, row 0 is the mixed slot: plain,
    # BLOQ, missing, ALOQ, plain with a cubic of its own in members 0..4; subject 16 is alone in the last chunk, censored.
    "ok": {"models": ["add0"], "subjects": [
        ["plain_p1", "bloq_p6"], ["bloq_m5", "plain_m1"], ["missing_f0", "aloq_p7"], ["aloq_p5", "bloq_p0"],
        ["plain_cubic_y0_05", "plain_cubic_y3"], ["bloq_m1", "aloq_p7_5"], ["aloq_p8", "bloq_m20"],
        ["bloq_m36_9", "aloq_m6"], ["aloq_p0", "bloq_m37_1"], ["plain_sigma_1e8", "plain_cubic_y40"],
        ["aloq_p1", "bloq_m38_6"], ["bloq_m40", "aloq_p6"], ["aloq_p37_1", "bloq_m400"], ["plain_p30", "aloq_p40"],
        ["aloq_p400", "plain_m30"], ["plain_p400", "plain_sigma_1em8"], ["bloq_m37_4", "aloq_p3"]]},
    # err and either rungs and the failing rows, each alone in its subject beside a mild plain row; four good subjects
    "bad": {"models": ["add0"], "subjects": [
        ["mild_f0", "aloq_p8_45"], ["aloq_p9", "mild_f1"], ["plain_p0", "mild_f1"], ["mild_f0", "aloq_p13"],
        ["aloq_p36_9", "mild_f1"], ["aloq_p8_15", "mild_f1"], ["mild_f0", "aloq_p8_22"], ["mild_f0", "missing_f1"],
        ["aloq_p8_29", "mild_f1"], ["bloq_m37_6", "mild_f1"], ["mild_f0", "bloq_m38"], ["bloq_m38_3", "mild_f1"],
        ["mild_f0", "bloq_m38_45"], ["mild_f0", "mild_f1"], ["fail_nonfinite_coefficient", "mild_f1"],
        ["mild_f0", "fail_censored_sigma_zero"], ["plain_p1", "plain_m1"]]},
    # sigma from the model; the cubic is negative at y = -8 (NegativeSigma under proportional, a plain row under additive)
    "model": {"models": ["addl", "prop"], "subjects": [
        ["model_plain_y0_3", "model_plain_y11"], ["model_bloq_ym0_4", "model_aloq_y13"],
        ["model_aloq_y0_2", "model_bloq_y12_5"], ["model_bloq_y0_5", "model_aloq_y10_5"],
        ["model_aloq_ym0_3", "model_bloq_y14"], ["model_plain_y0_05", "model_plain_y40"],
        ["model_cubic_negative_ym8", "model_plain_y3"], ["model_missing", "model_plain_y12"],
        ["model_bloq_y0_1", "model_plain_y13"]]},
    # residual models: every z at both predictions, a missing row, rows with a polynomial of their own
    "res": {"models": list(RESIDUAL), "subjects": [
        ["res_f0_z0", "res_f1_z0"], ["res_f0_z2", "res_f1_z2"], ["res_missing", "res_f1_z30"], ["res_f0_z30", "res_f1_z0"],
        ["res_f0_poly", "res_f1_poly"], ["res_f0_z0", "res_f1_z30"], ["res_f0_z2", "res_f1_z0"], ["res_f0_z30", "res_f1_z2"],
        ["res_f0_z0", "res_f1_z2"]]},
}
# The 66-observation design: 64 observations before the dose (f = 0), one at its instant, one later row.  Every row is
# `long_f0` / `long_f1` except the mixed slot, repeated at observations 62, 63 (f = 0) and 64 (f = 12.5).
LONG = {"models": ["add0"], "n_pre": 64, "default": ["long_f0", "long_f1"], "slots": [62, 63, 64],
        "mixed_f0": ["plain_p1", "bloq_m5", "missing_f0", "aloq_p5", "plain_cubic_y0_05", None, None, None, "bloq_m1"],
        "mixed_f1": ["plain_m1", "bloq_p0", "missing_f1", "aloq_p3", "plain_cubic_y3", None, None, None, "bloq_m20"]}


def main():
    build_terms()
    for name, pop in POPULATIONS.items():
        for mdl in pop["models"]:
            for a, b in pop["subjects"]:
                ta, tb = TERMS[f"{a}@{mdl}"], TERMS[f"{b}@{mdl}"]
                assert ta["kind"] == "missing" or ta["f"] == F0, a
                assert tb["kind"] == "missing" or tb["f"] == F1, b
                assert sum(t["cond"] > 1e-6 for t in (ta, tb)) <= 1, (a, b)
    used = {n for pop in POPULATIONS.values() for s in pop["subjects"] for n in s}
    used |= {n for k in ("default", "mixed_f0", "mixed_f1") for n in LONG[k] if n}
    assert used == {t["name"] for t in TERMS.values()}, sorted({t["name"] for t in TERMS.values()} ^ used)
    doc = {"generator": "tests/golden/gen_loglik_terms.py", "dps": mp.mp.dps,
           "design": {"dose": DOSE, "v": VOL, "t_pre": T_PRE, "t_dose": T_DOSE, "t_at": T_AT, "variants": VARIANTS, "ke": KE},
           "models": MODELS, "terms": list(TERMS.values()), "later": later_rows(), "populations": POPULATIONS, "long": LONG}
    with open(OUT, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{OUT}: {len(TERMS)} terms, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
