"""The closure models of tests/golden/user_closures.json: every closure as C text (what hiprtc and g++ compile) and, side
by side, as a Python twin (what tests/golden/gen_user_closures.py evaluates in mpmath).  Importing this module needs
neither the product nor the oracle: `build(name)` imports pharmsol_amd only when it is called.

Twin conventions.  `p` is the parameter vector as Python doubles, `cov` the covariates at the closure's time.
  lag(t, p, cov)            -> [double per input]   plain double arithmetic; every value here is exact in double (dyadic
                                                    constants, dyadic schedules), so that a fused multiply-add on the device
                                                    cannot move a landing time
  fa(t, p, cov)             -> [mpf per input]      the clamp decided in doubles, as the C text decides it
  init(p, cov)              -> [mpf per state]
  out(t, x, p, cov, der)    -> mpf
  derive(t, p, cov)         -> [mpf]
  kernel_params(pw, der)    -> the built-in structure's rate constants, in its own order (the model's `bind`)
  seq(t, p, cov, pw)        mutates pw
  eq(dt, x, pw, cov, rate)  -> [mpf per state]      the user's own propagator
  rhs(t, x, p, cov, rate, bolus) -> [mpf per state] the dynamics; `bolus` is None for the route form (pmx_dynamics)
"""
import math

import mpmath as mp

mpf = mp.mpf

SIG = ("double t, const double* x, const double* p, const double* cov, const double* rateiv, "
       "const double* derived, double* ")
SIGB = ("double t, const double* x, const double* p, const double* cov, const double* rateiv, const double* bolus, "
        "const double* derived, double* ")


def M(v):
    return [mpf(a) for a in v]


def clamp01(raw_double, value):
    """fmin(fmax(v, 0), 1): the branch taken on the double the C text forms, the value in mpf."""
    if raw_double >= 1.0:
        return mpf(1)
    if raw_double <= 0.0:
        return mpf(0)
    return value


# ------------------------------------------------------------------------------------------------------ analytical
# theta = [ke, kcp, kpc, lag_scale, lag1, v]; two inputs (central, peripheral); lag of input 0 follows the covariate
TWO_SRC = f"""
PMX_DEVICE void pmx_route_lag({SIG}lag) {{ lag[0] = p[3] * cov[0]; lag[1] = p[4]; }}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[0] / p[5]; }}
"""
TWO = dict(backend="analytical", eq="two_compartments", nstates=2, nparams=6, ndrugs=2, covariates=["c"], src=TWO_SRC,
           linear=True, central=0,
           lag=lambda t, p, cov: [p[3] * cov[0], p[4]],
           kernel_params=lambda pw, der: pw[:3],
           out=lambda t, x, p, cov, der: x[0] / mpf(p[5]))

# theta = [ka, ke, v, lag0, s]: lag = lag0 * sqrt(s) (s = 1: lag0; s = 0.25: half of it; s = -1: NaN)
ORAL_SRC = f"""
PMX_DEVICE void pmx_route_lag({SIG}lag) {{ lag[0] = p[3] * sqrt(p[4]); }}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[1] / p[2]; }}
"""


def _oral_lag(t, p, cov):
    return [p[3] * mp.sqrt(p[4]) if isinstance(p[4], mpf) else (p[3] * math.sqrt(p[4]) if p[4] >= 0.0 else float("nan")), 0.0]


ORAL = dict(backend="analytical", eq="one_compartment_with_absorption", nstates=2, nparams=5, ndrugs=2, covariates=[],
            src=ORAL_SRC, linear=True, central=1, lag=_oral_lag, kernel_params=lambda pw, der: pw[:2],
            out=lambda t, x, p, cov, der: x[1] / mpf(p[2]))

# theta = [ka, ke0, v, lag_scale, f0, x1(0)]; ke = ke0 wt / 64 (derive), lag and fa follow wt, fa also the time
COV_SRC = f"""
PMX_DEVICE void pmx_derive({SIG}d) {{ d[0] = p[1] * (cov[0] / 64.0); }}
PMX_DEVICE void pmx_route_lag({SIG}lag) {{ lag[0] = p[3] * (cov[0] / 64.0); }}
PMX_DEVICE void pmx_route_bioavailability({SIG}fa) {{ fa[0] = fmin(fmax(p[4] * (0.25 + 0.125 * t) * (cov[0] / 64.0), 0.0), 1.0); }}
PMX_DEVICE void pmx_init({SIG}xi) {{ xi[1] = p[5]; }}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[1] / (p[2] * (cov[0] / 64.0)); }}
"""


def _cov_fa(t, p, cov):
    raw = p[4] * (0.25 + 0.125 * t) * (cov[0] / 64.0)
    return [clamp01(raw, mpf(p[4]) * (mpf("0.25") + mpf("0.125") * mpf(t)) * (mpf(cov[0]) / 64)), mpf(1)]


def _cov(cov_time):
    return dict(backend="analytical", eq="one_compartment_with_absorption", nstates=2, nparams=6, ndrugs=2, covariates=["wt"],
                n_derived=1, bind=[("p", 0), ("d", 0)], cov_time=cov_time, src=COV_SRC, linear=False, central=1,
                derive=lambda t, p, cov: [mpf(p[1]) * (mpf(cov[0]) / 64)],
                lag=lambda t, p, cov: [p[3] * (cov[0] / 64.0), 0.0], fa=_cov_fa,
                init=lambda p, cov: [mpf(0), mpf(p[5])],
                kernel_params=lambda pw, der: [pw[0], der[0]],
                out=lambda t, x, p, cov, der: x[1] / (mpf(p[2]) * (mpf(cov[0]) / 64)))


# the user's own propagator over two inputs, with seq_eq; theta = [k, lag0, step]; affine in the state
EQ_SRC = f"""
PMX_DEVICE void pmx_eq({SIG}xn) {{
  const double e = exp(-p[0] * t);
  xn[0] = x[0] * e + rateiv[0] * t;
  xn[1] = x[1] + p[0] * t + 0.5 * rateiv[1] * t;
}}
PMX_DEVICE void pmx_seq_eq({SIG}pw) {{ pw[0] += p[2] * (1.0 + 0.0625 * t); }}
PMX_DEVICE void pmx_route_lag({SIG}lag) {{ lag[0] = p[1]; }}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[0] + x[1]; }}
"""


def _eq_seq(t, p, cov, pw):
    pw[0] = pw[0] + mpf(p[2]) * (1 + mpf("0.0625") * mpf(t))


def _eq_eq(dt, x, pw, cov, rate):
    e = mp.exp(-pw[0] * dt)
    return [x[0] * e + rate[0] * dt, x[1] + pw[0] * dt + rate[1] * dt / 2]


USER_EQ = dict(backend="analytical", eq=None, nstates=2, nparams=3, ndrugs=2, covariates=[], src=EQ_SRC, linear=False, central=None,
               lag=lambda t, p, cov: [p[1], 0.0], seq=_eq_seq, eq_fn=_eq_eq,
               out=lambda t, x, p, cov, der: x[0] + x[1])

# the Pmetrics wrapper: state / input 0 is the dead pad slot; theta = [ka, ke, v, lag_scale]
PM_SRC = f"""
PMX_DEVICE void pmx_route_lag({SIG}lag) {{ lag[1] = p[3] * cov[0]; }}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[2] / p[2]; }}
"""
PM = dict(backend="analytical", eq="pm_one_compartment_with_absorption", nstates=3, nparams=4, ndrugs=3, covariates=["c"],
          src=PM_SRC, linear=True, central=2, pm=True,
          lag=lambda t, p, cov: [0.0, p[3] * cov[0], 0.0], kernel_params=lambda pw, der: pw[:2],
          out=lambda t, x, p, cov, der: x[2] / mpf(p[2]))

# ------------------------------------------------------------------------------------------------------------- ODE
# two-state oral body; theta = [ka, ke, v, lag_scale, lag1, f0, x1(0)]; elimination follows the covariate at every stage
_LAGFA = f"""
PMX_DEVICE void pmx_route_lag({SIG}lag) {{ lag[0] = p[3] * cov[0]; lag[1] = p[4]; }}
PMX_DEVICE void pmx_route_bioavailability({SIG}fa) {{ fa[0] = fmin(fmax(p[5] * (0.25 + 0.125 * t) * (1.0 + 0.0625 * cov[0]), 0.0), 1.0); }}
PMX_DEVICE void pmx_init({SIG}xi) {{ xi[1] = p[6]; }}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[1] / p[2]; }}
"""
ODE_ROUTES_SRC = f"""
PMX_DEVICE void pmx_dynamics({SIG}dx) {{
  dx[0] = -p[0] * x[0];
  dx[1] = p[0] * x[0] - p[1] * (1.0 + 0.0625 * cov[0]) * x[1] + rateiv[0];
}}
""" + _LAGFA
ODE_BOLUS_SRC = f"""
PMX_DEVICE void pmx_dynamics_bolus({SIGB}dx) {{
  dx[0] = bolus[0] - p[0] * x[0];
  dx[1] = bolus[1] + p[0] * x[0] - p[1] * (1.0 + 0.0625 * cov[0]) * x[1] + rateiv[0];
}}
""" + _LAGFA
# the bolus argument enters two states with different weights, and state 0 through a saturating term: the jump depends
# on the state it meets, so the order of two boluses at one time matters
ODE_WEIGHTED_SRC = f"""
PMX_DEVICE void pmx_dynamics_bolus({SIGB}dx) {{
  dx[0] = 0.75 * bolus[0] / (1.0 + 0.015625 * x[0]) - p[0] * x[0];
  dx[1] = 0.25 * bolus[0] + bolus[1] + p[0] * x[0] - p[1] * (1.0 + 0.0625 * cov[0]) * x[1] + rateiv[0];
}}
""" + _LAGFA


def _ode_fa(t, p, cov):
    raw = p[5] * (0.25 + 0.125 * t) * (1.0 + 0.0625 * cov[0])
    return [clamp01(raw, mpf(p[5]) * (mpf("0.25") + mpf("0.125") * mpf(t)) * (1 + mpf("0.0625") * mpf(cov[0]))), mpf(1)]


def _ode_rhs(weighted):
    def rhs(t, x, p, cov, rate, bolus):
        ka, ke = mpf(p[0]), mpf(p[1])
        k = ke * (1 + mpf("0.0625") * cov[0])
        b = bolus if bolus is not None else [mpf(0), mpf(0)]
        if weighted:
            return [mpf("0.75") * b[0] / (1 + mpf("0.015625") * x[0]) - ka * x[0],
                    mpf("0.25") * b[0] + b[1] + ka * x[0] - k * x[1] + rate[0]]
        return [b[0] - ka * x[0], b[1] + ka * x[0] - k * x[1] + rate[0]]
    return rhs


def _ode(src, bolus_arg, weighted=False):
    return dict(backend="ode", nstates=2, nparams=7, ndrugs=2, covariates=["c"], src=src, h_max=0.05, bolus_arg=bolus_arg,
                linear=False, central=1, lag=lambda t, p, cov: [p[3] * cov[0], p[4]], fa=_ode_fa,
                init=lambda p, cov: [mpf(0), mpf(p[6])], rhs=_ode_rhs(weighted),
                rate_max=lambda p, cmax: max(p[0], p[1] * (1.0 + 0.0625 * cmax)),
                out=lambda t, x, p, cov, der: x[1] / mpf(p[2]))


MODELS = {"an_two": TWO, "an_oral": ORAL, "an_cov_dt": _cov("segment_dt"), "an_cov_abs": _cov("segment_end_abs"),
          "an_user_eq": USER_EQ, "an_pm": PM, "ode_routes": _ode(ODE_ROUTES_SRC, False), "ode_bolus": _ode(ODE_BOLUS_SRC, True),
          "ode_weighted": _ode(ODE_WEIGHTED_SRC, True, weighted=True)}


def build(name):
    """The product's model object of MODELS[name]."""
    from pharmsol_amd import ODE, Analytical

    m = MODELS[name]
    if m["backend"] == "ode":
        return ODE.user(m["src"], nstates=m["nstates"], nparams=m["nparams"], ndrugs=m["ndrugs"], nout=1,
                        covariates=m["covariates"], h_max=m["h_max"])
    return Analytical.user(m["src"], eq=m["eq"], nstates=m["nstates"], nparams=m["nparams"], ndrugs=m["ndrugs"], nout=1,
                           covariates=m["covariates"], n_derived=m.get("n_derived", 0), bind=m.get("bind"),
                           cov_time=m.get("cov_time", "segment_dt"))
