#!/usr/bin/env python3
"""Generate tests/golden/model_refusals.json: what the model-creation calls of include/pmx.h answer, recorded from a build
of the library BEFORE model creation was gathered into csrc/pmx_model.cpp (commit d184749), so that the refactored code is
held to the old answers and not to its own.

Five creation paths - built-in analytical structure, built-in diffeq body, custom diffeq body (state-machine kernels), user
analytical, user ODE (general walker) - each with one valid base descriptor.  A case applies field edits to its base
(usually one fault), calls one of pmx_model_create / _create_custom / _create_user / pmx_debug_jit_source / _source_user
and records the return code and the first line of pmx_last_error() (a compile failure's further lines are the compiler's).
Accepted cases are recorded as code 0; a debug call that returns text records its SHA-256 (`sha256`), which pins the
translation unit handed to hiprtc.  Cases that compile are kept few: accepted forms go through the debug calls, which run
the same checks, wherever the path has one.

MESSAGES lists every refusal text of the recorded library's validators.  The generator asserts that each is reached by a
case or named in UNREACHABLE together with the earlier check that shadows it.

Run (needs no GPU; hiprtc compiles for gfx950 without one):
    PMX_LIB=<libpmx_hip.so of the commit to record> python tests/golden/gen_model_refusals.py
Deterministic; rewrites model_refusals.json byte for byte.
"""
import ctypes as C
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
try:
    from pharmsol_amd import _abi, _ffi
except ImportError:  # run as a script from anywhere: the package is two levels up
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from pharmsol_amd import _abi, _ffi

OUT = os.path.join(HERE, "model_refusals.json")
RECORDED_AT = "d184749"

SIG = "double t, const double* x, const double* p, const double* cov, const double* rateiv, const double* derived, double* "
SIGB = ("double t, const double* x, const double* p, const double* cov, const double* rateiv, const double* bolus, "
        "const double* derived, double* ")
_DYN = f"PMX_DEVICE void pmx_dynamics({SIG}dx) {{ dx[0] = -p[0] * x[0]; dx[1] = p[0] * x[0] - p[1] * x[1] + rateiv[0]; }}\n"
_DYNB = (f"PMX_DEVICE void pmx_dynamics_bolus({SIGB}dx) {{ dx[0] = bolus[0] - p[0] * x[0]; "
         f"dx[1] = p[0] * x[0] - p[1] * x[1] + rateiv[0]; }}\n")
_OUT = f"PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[1] / p[2]; }}\n"
_INIT = f"PMX_DEVICE void pmx_init({SIG}xi) {{ xi[1] = p[2]; }}\n"
_LAG = f"PMX_DEVICE void pmx_route_lag({SIG}lag) {{ lag[0] = p[3]; }}\n"
_FA = f"PMX_DEVICE void pmx_route_bioavailability({SIG}fa) {{ fa[0] = p[3]; }}\n"
_DERIVE = f"PMX_DEVICE void pmx_derive({SIG}d) {{ d[0] = p[1] * pow(cov[0] / 70.0, 0.75); }}\n"
SOURCES = {
    "body": _DYN + _OUT,
    "body_init": _DYN + _OUT + _INIT,
    "ode_lag": _DYN + _OUT + _LAG,
    "ode_fa": _DYN + _OUT + _FA,
    "ode_derive": (f"PMX_DEVICE void pmx_dynamics({SIG}dx) {{ dx[0] = -p[0] * x[0]; dx[1] = p[0] * x[0] - derived[0] * x[1]; }}\n"
                   + _OUT + _DERIVE),
    "ode_bolus": _DYNB + _OUT,
    "an_lag": _LAG,
    "an_eq": f"PMX_DEVICE void pmx_eq({SIG}xn) {{ xn[0] = x[0] + p[0] * t; }}\n" + f"PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[0]; }}\n",
    "an_closures": _LAG + f"PMX_DEVICE void pmx_route_bioavailability({SIG}fa) {{ fa[0] = p[2]; }}\n" + _DERIVE,
    "broken": "this is not C++\n",
}

FN = {k[len("PMX_FN_"):]: getattr(_abi, k) for k in dir(_abi) if k.startswith("PMX_FN_")}
ODE, AN = _abi.PMX_EQ_ODE, _abi.PMX_EQ_ANALYTICAL
PRIMARY, DERIVED = _abi.PMX_SRC_PRIMARY, _abi.PMX_SRC_DERIVED
_NUM = {"rk4_h_max": 0.05, "ode_solver": _abi.PMX_SOLVER_RK4, "ode_rtol": 1e-6, "ode_atol": 1e-6}
# one valid descriptor per path: field path -> value, on a zeroed pmx_model_desc whose *_param / *_dest arrays hold -1
BASES = {
    # one compartment with absorption (ka, ke; 2 states), ke bound to a covariate-derived value: the DYN kernels, no compile
    "analytical": {"eq_kind": AN, "kernel": 3, "nstates": 2, "ndrugs": 1, "nout": 1, "nparams": 4, "n_covariates": 1,
                   "n_derived": 1, "derived[0].src_param": 1, "derived[0].n_factors": 1, "derived[0].f[0].op": _abi.PMX_F_POW,
                   "derived[0].f[0].cov": 0, "derived[0].f[0].ref": 70.0, "derived[0].f[0].coef": 0.75,
                   "n_bind": 2, "bind[0].src": PRIMARY, "bind[0].index": 0, "bind[1].src": DERIVED, "bind[1].index": 0,
                   "out[0].state": 1, "out[0].vol_src": PRIMARY, "out[0].vol_index": 2, "bolus_dest[0]": 0, **_NUM},
    # one_cmt_oral (2 states, 2 parameters): the built-in ODE kernels, no compile
    "ode_body": {"eq_kind": ODE, "kernel": 1, "nstates": 2, "ndrugs": 1, "nout": 1, "nparams": 3, "out[0].state": 1,
                 "out[0].vol_src": PRIMARY, "out[0].vol_index": 2, "bolus_dest[0]": 0, "infusion_dest[0]": 1, **_NUM},
    "custom": {"eq_kind": ODE, "kernel": _abi.PMX_ODE_CUSTOM, "nstates": 2, "ndrugs": 1, "nout": 1, "nparams": 3,
               "bolus_dest[0]": 0, **_NUM},
    "user_analytical": {"eq_kind": AN, "kernel": 3, "nstates": 2, "ndrugs": 1, "nout": 1, "nparams": 4, "n_covariates": 1,
                        "out[0].state": 1, "out[0].vol_src": PRIMARY, "out[0].vol_index": 2, "bolus_dest[0]": 0, **_NUM},
    "user_ode": {"eq_kind": ODE, "kernel": _abi.PMX_ODE_CUSTOM, "nstates": 2, "ndrugs": 1, "nout": 1, "nparams": 4,
                 "n_covariates": 1, "bolus_dest[0]": 0, **_NUM},
}
# how each base is called when a case says nothing else
DEFAULTS = {
    "analytical": {"call": "create"},
    "ode_body": {"call": "create"},
    "custom": {"call": "debug_jit_source", "source": "body", "has_init": 0},
    "user_analytical": {"call": "debug_jit_source_user", "source": "an_lag", "fns": ["ROUTE_LAG"]},
    "user_ode": {"call": "debug_jit_source_user", "source": "ode_lag", "fns": ["DYNAMICS", "OUTPUTS", "ROUTE_LAG"]},
}


def set_field(d, path, value):
    *head, last = re.findall(r"[A-Za-z_]\w*|\[\d+\]", path)
    for tok in head:
        d = d[int(tok[1:-1])] if tok[0] == "[" else getattr(d, tok)
    if last[0] == "[":
        d[int(last[1:-1])] = value
    else:
        setattr(d, last, value)


def make_desc(base, edits):
    d = _abi.pmx_model_desc()
    for arr in ("init_param", "lag_param", "fa_param", "bolus_dest", "infusion_dest"):
        for i in range(len(getattr(d, arr))):
            getattr(d, arr)[i] = -1
    for path, value in list(base.items()) + [tuple(e) for e in edits]:
        set_field(d, path, value)
    return d


def run_case(L, fixture, case):
    """(code, first line of the error text, handle-or-text is null, sha256 of a returned text or None)"""
    d = make_desc(fixture["bases"][case["base"]], case["edits"])
    dp = None if case.get("null_desc") else C.byref(d)
    src = None if case.get("source") is None else fixture["sources"][case["source"]].encode()
    fns = 0
    for name in case.get("fns", []):
        fns |= FN[name]
    h = C.c_void_p()
    call = case["call"]
    if call == "create":
        rc = L.pmx_model_create(dp, C.byref(h))
    elif call == "create_custom":
        rc = L.pmx_model_create_custom(dp, src, case.get("has_init", 0), C.byref(h))
    elif call == "create_user":
        rc = L.pmx_model_create_user(dp, src, fns, C.byref(h))
    elif call == "debug_jit_source":
        rc = L.pmx_debug_jit_source(dp, src, case.get("has_init", 0), C.byref(h))
    elif call == "debug_jit_source_user":
        rc = L.pmx_debug_jit_source_user(dp, src, fns, C.byref(h))
    else:
        raise ValueError(call)
    text = L.pmx_last_error().decode().split("\n")[0]
    sha = None
    if h.value:
        if call.startswith("debug"):
            sha = hashlib.sha256(C.string_at(h.value)).hexdigest()
            L.pmx_free_text(h)
        else:
            L.pmx_model_destroy(h)
    return rc, text, not h.value, sha


def _cases():
    out = []

    def case(name, base, edits=(), **how):
        c = {"name": name, "base": base, "edits": [list(e) for e in edits]}
        c.update(DEFAULTS[base])
        c.update(how)
        out.append(c)

    def sizes(base, **how):  # the bounds every path checks the same way
        for f, v in (("nstates", 0), ("nstates", 9), ("ndrugs", -1), ("ndrugs", 9), ("nout", 0), ("nout", 5), ("nparams", -1),
                     ("nparams", 17), ("n_covariates", -1), ("n_covariates", 9)):
            case(f"{base}/{f}={v}", base, [(f, v)], **how)

    def numerics(base, **how):
        case(f"{base}/rk4_h_max=0", base, [("rk4_h_max", 0.0)], **how)
        case(f"{base}/ode_solver=4", base, [("ode_solver", 4)], **how)
        case(f"{base}/dopri5_rtol=0", base, [("ode_solver", _abi.PMX_SOLVER_DOPRI5), ("ode_rtol", 0.0)], **how)

    def routes(base, **how):
        case(f"{base}/lag_param=nparams", base, [("lag_param[0]", BASES[base]["nparams"])], **how)
        case(f"{base}/fa_param=nparams", base, [("fa_param[7]", BASES[base]["nparams"])], **how)
        case(f"{base}/bolus_dest=nstates", base, [("bolus_dest[0]", 2)], **how)
        case(f"{base}/infusion_dest=nstates", base, [("infusion_dest[0]", 2)], **how)

    def out_init(base, **how):
        case(f"{base}/out.state=nstates", base, [("out[0].state", 2)], **how)
        case(f"{base}/out.state=-1", base, [("out[0].state", -1)], **how)
        case(f"{base}/out.vol_index=nparams", base, [("out[0].vol_src", PRIMARY), ("out[0].vol_index", BASES[base]["nparams"])], **how)
        case(f"{base}/out.vol_index_derived", base, [("out[0].vol_src", DERIVED), ("out[0].vol_index", 1)], **how)
        case(f"{base}/init_param=nparams", base, [("init_param[0]", BASES[base]["nparams"])], **how)

    def derived_desc(base, pre=()):
        pre = list(pre)
        case(f"{base}/derived.src_param", base, pre + [("derived[0].src_param", BASES[base]["nparams"])])
        case(f"{base}/derived.n_factors", base, pre + [("derived[0].n_factors", 3)])
        case(f"{base}/derived.factor_cov", base, pre + [("derived[0].n_factors", 1), ("derived[0].f[0].op", _abi.PMX_F_POW), ("derived[0].f[0].cov", 1)])

    def binds(base, pre=(), **how):  # `pre` makes bind[0] PRIMARY 0 and bind[1] a valid entry
        pre = list(pre)
        case(f"{base}/n_bind=3", base, pre + [("n_bind", 3)], **how)
        case(f"{base}/bind_index", base, pre + [("bind[0].index", BASES[base]["nparams"])], **how)
        case(f"{base}/bind_index_negative", base, pre + [("bind[0].index", -1)], **how)
        case(f"{base}/bind_derived_index", base, pre + [("bind[1].src", DERIVED), ("bind[1].index", 1)], **how)
        case(f"{base}/bind_src", base, pre + [("bind[0].src", 0)], **how)

    # ---- null pointers, wrong entry point, unknown eq_kind
    case("analytical/valid", "analytical")
    case("create/null_desc", "analytical", null_desc=True)
    case("create/ode_custom_kernel", "ode_body", [("kernel", _abi.PMX_ODE_CUSTOM)])
    case("create/k_custom_kernel", "analytical", [("kernel", _abi.PMX_K_CUSTOM)])
    case("create/eq_kind=7", "analytical", [("eq_kind", 7)])
    case("create_user/eq_kind=7", "user_analytical", [("eq_kind", 7)], call="create_user")
    case("create_user/null_desc", "user_analytical", null_desc=True, call="create_user")
    for base in ("custom", "user_analytical", "user_ode"):
        for call in {"custom": ("create_custom", "debug_jit_source"), }.get(base, ("create_user", "debug_jit_source_user")):
            case(f"{base}/{call}/null_source", base, call=call, source=None)
    case("custom/create_custom/null_desc", "custom", call="create_custom", null_desc=True)
    case("custom/debug_jit_source/null_desc", "custom", null_desc=True)
    case("user/debug_jit_source_user/null_desc", "user_ode", null_desc=True)

    # ---- built-in analytical
    sizes("analytical")
    case("analytical/ndrugs=0", "analytical", [("ndrugs", 0)])
    case("analytical/nparams=0", "analytical", [("nparams", 0)])
    case("analytical/n_derived=-1", "analytical", [("n_derived", -1)])
    case("analytical/n_derived=5", "analytical", [("n_derived", 5)])
    derived_desc("analytical")
    case("analytical/kernel=12", "analytical", [("kernel", 12)])
    case("analytical/kernel=-1", "analytical", [("kernel", -1)])
    case("analytical/nstates=1", "analytical", [("nstates", 1), ("out[0].state", 0)])
    case("analytical/pm_needs_a_state", "analytical", [("pmetrics_indexing", 1)])
    case("analytical/pm", "analytical", [("pmetrics_indexing", 1), ("nstates", 3)])
    case("analytical/too_few_params", "analytical", [("n_bind", 0), ("n_derived", 0), ("nparams", 1), ("out[0].vol_src", 0)])
    binds("analytical")
    routes("analytical")
    out_init("analytical")

    # ---- built-in diffeq body
    case("ode_body/valid", "ode_body")
    sizes("ode_body")
    case("ode_body/ndrugs=0", "ode_body", [("ndrugs", 0)])
    case("ode_body/nparams=0", "ode_body", [("nparams", 0)])
    case("ode_body/n_derived=5", "ode_body", [("n_derived", 5)])
    derived_desc("ode_body", [("n_derived", 1), ("n_covariates", 1)])
    case("ode_body/kernel=7", "ode_body", [("kernel", 7)])
    case("ode_body/nstates=1", "ode_body", [("nstates", 1), ("out[0].state", 0), ("infusion_dest[0]", 0)])
    case("ode_body/nparams=1", "ode_body", [("nparams", 1), ("out[0].vol_src", 0)])
    numerics("ode_body")
    case("ode_body/pm", "ode_body", [("pmetrics_indexing", 1), ("nstates", 3)])
    case("ode_body/n_bind=1", "ode_body", [("n_bind", 1), ("bind[0].src", PRIMARY)])
    binds("ode_body", [("n_bind", 2), ("bind[0].src", PRIMARY), ("bind[0].index", 0), ("bind[1].src", PRIMARY), ("bind[1].index", 1)])
    routes("ode_body")
    out_init("ode_body")

    # ---- custom diffeq body: refusals through the creating call, accepted forms and the rest through the debug view
    case("custom/valid", "custom", call="create_custom")
    case("custom/valid_init", "custom", call="create_custom", source="body_init", has_init=1)
    case("custom/broken_source", "custom", call="create_custom", source="broken")
    case("custom/kernel=1", "custom", [("kernel", 1)], call="create_custom")
    case("custom/eq_kind=analytical", "custom", [("eq_kind", AN)])
    sizes("custom", call="create_custom")
    case("custom/ndrugs=0", "custom", [("ndrugs", 0)])
    case("custom/nparams=0", "custom", [("nparams", 0)], call="create_custom")
    numerics("custom", call="create_custom")
    for f in ("n_derived", "n_bind", "pmetrics_indexing"):
        case(f"custom/{f}=1", "custom", [(f, 1)], call="create_custom")
    case("custom/n_derived=-1", "custom", [("n_derived", -1)])
    routes("custom")
    out_init("custom")
    case("custom/debug/valid", "custom")
    case("custom/debug/valid_init", "custom", source="body_init", has_init=1)
    case("custom/via_create_user", "custom", call="debug_jit_source_user", fns=["DYNAMICS", "OUTPUTS"])
    case("custom/via_create_user_init", "custom", call="debug_jit_source_user", source="body_init", fns=["DYNAMICS", "OUTPUTS", "INIT"])
    case("custom/via_create_user/kernel=1", "custom", [("kernel", 1)], call="create_user", fns=["DYNAMICS", "OUTPUTS"])

    # ---- user analytical
    ua = "user_analytical"
    case("user_analytical/valid", ua, call="create_user")
    case("user_analytical/broken_source", ua, call="create_user", source="broken", fns=["ROUTE_LAG"])
    sizes(ua)
    case("user_analytical/ndrugs=0", ua, [("ndrugs", 0)], call="create_user")
    case("user_analytical/nparams=0", ua, [("nparams", 0)], call="create_user")
    case("user_analytical/n_derived=16", ua, [("n_derived", 16)], source="an_closures", fns=["ROUTE_LAG", "ROUTE_BIOAVAILABILITY", "DERIVE"])
    case("user_analytical/n_derived=17", ua, [("n_derived", 17)], source="an_closures", fns=["ROUTE_LAG", "ROUTE_BIOAVAILABILITY", "DERIVE"])
    case("user_analytical/n_derived=-1", ua, [("n_derived", -1)])
    case("user_analytical/n_derived_without_derive", ua, [("n_derived", 1)], call="create_user")
    case("user_analytical/dynamics", ua, fns=["ROUTE_LAG", "DYNAMICS"])
    case("user_analytical/eq_with_structure", ua, fns=["ROUTE_LAG", "EQ"])
    case("user_analytical/k_custom_without_eq", ua, [("kernel", _abi.PMX_K_CUSTOM)])
    case("user_analytical/k_custom_pm", ua, [("kernel", _abi.PMX_K_CUSTOM), ("pmetrics_indexing", 1)], source="an_eq", fns=["EQ", "OUTPUTS"])
    case("user_analytical/k_custom", ua, [("kernel", _abi.PMX_K_CUSTOM), ("nstates", 1), ("nparams", 1), ("n_covariates", 0)], source="an_eq", fns=["EQ", "OUTPUTS"])
    case("user_analytical/k_custom_ignores_bind", ua, [("kernel", _abi.PMX_K_CUSTOM), ("n_bind", 3), ("bind[0].src", 7)], source="an_eq", fns=["EQ", "OUTPUTS"])
    case("user_analytical/closures", ua, [("n_derived", 1)], source="an_closures", fns=["ROUTE_LAG", "ROUTE_BIOAVAILABILITY", "DERIVE"])
    case("user_analytical/kernel=12", ua, [("kernel", 12)])
    case("user_analytical/nstates=1", ua, [("nstates", 1), ("out[0].state", 0)])
    case("user_analytical/pm_needs_a_state", ua, [("pmetrics_indexing", 1)])
    case("user_analytical/pm", ua, [("pmetrics_indexing", 1), ("nstates", 3)])
    case("user_analytical/too_few_params", ua, [("nparams", 1), ("out[0].vol_src", 0)], fns=[], source="body")
    binds(ua, [("n_bind", 2), ("bind[0].src", PRIMARY), ("bind[0].index", 0), ("bind[1].src", PRIMARY), ("bind[1].index", 1)])
    routes(ua)
    out_init(ua)
    case("user_analytical/out.state_with_outputs_closure", ua, [("out[0].state", 2)], fns=["ROUTE_LAG", "OUTPUTS"])

    # ---- user ODE on the general walker
    uo = "user_ode"
    case("user_ode/valid", uo, call="create_user")
    case("user_ode/broken_source", uo, call="create_user", source="broken")
    case("user_ode/fa", uo, source="ode_fa", fns=["DYNAMICS", "OUTPUTS", "ROUTE_BIOAVAILABILITY"])
    case("user_ode/derive", uo, [("n_derived", 1)], source="ode_derive", fns=["DYNAMICS", "OUTPUTS", "DERIVE"])
    case("user_ode/dynamics_bolus", uo, source="ode_bolus", fns=["DYNAMICS_BOLUS", "OUTPUTS"])
    case("user_ode/kernel=1", uo, [("kernel", 1)], call="create_user")
    case("user_ode/dynamics_and_dynamics_bolus", uo, fns=["DYNAMICS", "DYNAMICS_BOLUS", "OUTPUTS", "ROUTE_LAG"])
    case("user_ode/no_dynamics", uo, fns=["OUTPUTS", "ROUTE_LAG"])
    case("user_ode/no_outputs", uo, fns=["DYNAMICS", "ROUTE_LAG"])
    case("user_ode/eq", uo, fns=["DYNAMICS", "OUTPUTS", "ROUTE_LAG", "EQ"])
    case("user_ode/seq_eq", uo, fns=["DYNAMICS", "OUTPUTS", "ROUTE_LAG", "SEQ_EQ"])
    sizes(uo)
    case("user_ode/ndrugs=0", uo, [("ndrugs", 0)], call="create_user")
    case("user_ode/nparams=0", uo, [("nparams", 0)], call="create_user")
    case("user_ode/n_derived=16", uo, [("n_derived", 16)], source="ode_derive", fns=["DYNAMICS", "OUTPUTS", "DERIVE"])
    case("user_ode/n_derived=17", uo, [("n_derived", 17)], source="ode_derive", fns=["DYNAMICS", "OUTPUTS", "DERIVE"])
    case("user_ode/n_derived_without_derive", uo, [("n_derived", 1)])
    case("user_ode/n_bind=1", uo, [("n_bind", 1)], call="create_user")
    case("user_ode/pm", uo, [("pmetrics_indexing", 1)])
    numerics(uo, call="create_user")
    routes(uo)
    out_init(uo)
    return out


# every refusal text of the four validators and the entry points of the recorded library
MESSAGES = [
    "null argument", "out is null", "out_text is null",
    "PMX_ODE_CUSTOM models are created with pmx_model_create_custom", "PMX_K_CUSTOM models are created with pmx_model_create_user",
    "unknown eq_kind", "nstates out of range", "ndrugs out of range", "ndrugs out of range (1..8 for a model with user closures)",
    "nout out of range", "nparams out of range", "n_covariates out of range", "n_derived out of range",
    "derived.src_param out of range", "derived.n_factors out of range", "derived factor covariate out of range",
    "unknown analytical kernel", "model has fewer states than its structure", "too few parameters for the structure",
    "n_bind must equal the structure's parameter count", "bind index out of range", "bind derived index out of range",
    "bind.src must be PRIMARY or DERIVED", "bind entry out of range", "lag_param / fa_param out of range",
    "unknown ODE model", "model has fewer states than its diffeq", "too few parameters for the diffeq",
    "rk4_h_max must be > 0", "unknown ode_solver", "the adaptive solvers and checked RK4 need ode_rtol > 0 and ode_atol > 0",
    "pm_* indexing is a wrapper of the analytical structures (analytical/mod.rs:62-90): it does not apply to ODE models",
    "n_bind must equal the diffeq's parameter count", "route destination out of range", "out.state out of range",
    "out.vol_index out of range", "out.vol_index (derived) out of range", "init_param out of range",
    "custom models need eq_kind = PMX_EQ_ODE and kernel = PMX_ODE_CUSTOM",
    "derived-parameter descriptors / pm indexing do not apply to custom ODE bodies (compute them in the body)",
    "n_derived > 0 needs PMX_FN_DERIVE (desc.derived[] is not read for user models)",
    "pm_* indexing wraps a built-in structure: it does not apply to a user propagator (pmx_eq)",
    "PMX_FN_DYNAMICS belongs to ODE models", "kernel = PMX_K_CUSTOM needs PMX_FN_EQ", "PMX_FN_EQ needs kernel = PMX_K_CUSTOM",
    "ODE models with user closures need kernel = PMX_ODE_CUSTOM",
    "ODE models define pmx_dynamics OR pmx_dynamics_bolus (PMX_FN_DYNAMICS | PMX_FN_DYNAMICS_BOLUS)",
    "ODE models define pmx_outputs (PMX_FN_OUTPUTS)", "PMX_FN_SEQ_EQ / PMX_FN_EQ belong to analytical models",
    "bind[] / pm indexing do not apply to ODE models with user closures",
    "hiprtc could not compile the model source:", "hiprtc could not compile the generated closures:",
    "hiprtc could not compile the generated diffeq body:", "malloc",
]
UNREACHABLE = {
    "out is null": "the binding always passes an out pointer; the check precedes every descriptor check and reads no descriptor field",
    "out_text is null": "as 'out is null', for the two debug calls",
    "hiprtc could not compile the generated closures:": "the text is generated from a descriptor that passed every check (derived[] "
        "ranges, bind[]); no descriptor fault survives those checks to reach the compiler",
    "hiprtc could not compile the generated diffeq body:": "as the generated closures: shadowed by the derived[] / bind[] / structure checks",
    "malloc": "an allocation failure of the returned text, not a property of the arguments",
}


def main():
    L = _ffi.lib()
    fixture = {"recorded_at": RECORDED_AT, "sources": SOURCES, "bases": BASES, "cases": _cases(), "unreachable": UNREACHABLE}
    names = [c["name"] for c in fixture["cases"]]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    seen = set()
    for c in fixture["cases"]:
        rc, text, null, sha = run_case(L, fixture, c)
        assert null == (rc != 0), c
        c["code"], c["text"] = rc, text
        if sha:
            c["sha256"] = sha
        seen.add(text)
    missing = [m for m in MESSAGES if m not in seen and m not in UNREACHABLE]
    stray = sorted(t for t in seen if t and t not in MESSAGES)
    assert not missing and not stray, (missing, stray)
    with open(OUT, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    n_ok = sum(c["code"] == 0 for c in fixture["cases"])
    print(f"{len(names)} cases ({n_ok} accepted, {sum('sha256' in c for c in fixture['cases'])} translation units), "
          f"{len(seen) - 1} distinct refusals -> {OUT}")


if __name__ == "__main__":
    main()
