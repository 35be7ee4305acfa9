"""Which code objects model creation compiles: every JIT branch of pmx_model_create, pmx_model_create_custom and
pmx_model_create_user once, with the disk level of the code-object cache in an empty directory.  The cache names one file
per content key (translation unit + options), so two builds of the library compile the same code exactly when the listings
are equal on one machine:
    PMX_LIB=<a>.so python tools/experiments/model_creation_keys.py > a.txt;  PMX_LIB=<b>.so python ... > b.txt;  diff a.txt b.txt
Descriptors and sources: tests/golden/model_refusals.json (bases, sources) through tests/golden/gen_model_refusals.py."""
import importlib.util, json, os, sys, tempfile
sys.path.insert(0, ".")
cache = tempfile.mkdtemp(prefix="pmx_keys_")
os.environ["PMX_JIT_CACHE_DIR"] = cache
from pharmsol_amd import _abi, _ffi

spec = importlib.util.spec_from_file_location("gen", "tests/golden/gen_model_refusals.py")
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)
fx = json.load(open("tests/golden/model_refusals.json"))
L = _ffi.lib()
P, D = _abi.PMX_SRC_PRIMARY, _abi.PMX_SRC_DERIVED
plain = [["n_bind", 0], ["n_derived", 0], ["n_covariates", 0]]


def lags(n, p):
    return [["ndrugs", max(n, 1)]] + [[f"lag_param[{i}]", p] for i in range(n)] + [[f"bolus_dest[{i}]", 0] for i in range(n)]


ode_derived = [["n_covariates", 1], ["n_derived", 1], ["derived[0].src_param", 1], ["derived[0].n_factors", 1],
               ["derived[0].f[0].op", _abi.PMX_F_POW], ["derived[0].f[0].cov", 0], ["derived[0].f[0].ref", 70.0],
               ["derived[0].f[0].coef", 0.75], ["n_bind", 2], ["bind[0].src", P], ["bind[0].index", 0], ["bind[1].src", D], ["bind[1].index", 0]]
body, user_ode = ["DYNAMICS", "OUTPUTS"], dict(call="create_user")
CORPUS = [
    ("create: analytical, lag + covariate-derived rate constant", "analytical", lags(1, 3), dict(call="create")),
    ("create: analytical, lag + pm indexing", "analytical", plain + lags(1, 3) + [["pmetrics_indexing", 1], ["nstates", 3]], dict(call="create")),
    ("create: analytical, five lagged inputs", "analytical", plain + lags(5, 3), dict(call="create")),
    ("create: diffeq body with a derived parameter", "ode_body", ode_derived, dict(call="create")),
    ("create: diffeq body, derived parameter + init_param", "ode_body", ode_derived + [["init_param[1]", 2]], dict(call="create")),
    ("create: diffeq body, five lagged inputs", "ode_body", lags(5, 2), dict(call="create")),
    ("create_custom: body", "custom", [], dict(call="create_custom", source="body", has_init=0)),
    ("create_custom: body + init", "custom", [], dict(call="create_custom", source="body_init", has_init=1)),
    ("create_custom: five lagged inputs", "custom", lags(5, 2), dict(call="create_custom", source="body", has_init=0)),
    ("create_custom: five lagged inputs + init", "custom", lags(5, 2), dict(call="create_custom", source="body_init", has_init=1)),
    ("create_user: ODE body only (the custom path)", "custom", [], dict(call="create_user", source="body_init", fns=body + ["INIT"])),
    ("create_user: ODE body only, five lagged inputs", "custom", lags(5, 2), dict(call="create_user", source="body", fns=body)),
    ("create_user: ODE + lag closure", "user_ode", [], dict(user_ode, source="ode_lag", fns=body + ["ROUTE_LAG"])),
    ("create_user: ODE + fa closure", "user_ode", [], dict(user_ode, source="ode_fa", fns=body + ["ROUTE_BIOAVAILABILITY"])),
    ("create_user: ODE + derive", "user_ode", [["n_derived", 1]], dict(user_ode, source="ode_derive", fns=body + ["DERIVE"])),
    ("create_user: ODE, pmx_dynamics_bolus", "user_ode", [], dict(user_ode, source="ode_bolus", fns=["DYNAMICS_BOLUS", "OUTPUTS"])),
    ("create_user: analytical structure + lag closure", "user_analytical", [], dict(call="create_user", source="an_lag", fns=["ROUTE_LAG"])),
    ("create_user: analytical structure + lag, fa, derive", "user_analytical", [["n_derived", 1]],
     dict(call="create_user", source="an_closures", fns=["ROUTE_LAG", "ROUTE_BIOAVAILABILITY", "DERIVE"])),
    ("create_user: PMX_K_CUSTOM", "user_analytical", [["kernel", _abi.PMX_K_CUSTOM], ["nstates", 1], ["nparams", 1], ["n_covariates", 0]],
     dict(call="create_user", source="an_eq", fns=["EQ", "OUTPUTS"])),
]
for label, base, edits, how in CORPUS:
    before = set(os.listdir(cache))
    rc, text, _, _ = gen.run_case(L, fx, dict(base=base, edits=edits, **how))
    new = sorted(set(os.listdir(cache)) - before)
    print(f"{label:58s} rc={rc} {text}  ->  {', '.join(new) if new else '(already cached)'}")
print("\n".join(sorted(os.listdir(cache))))
