"""Every covariate path on the device against 40-digit truth: tests/golden/covariate_math.json (tests/golden/gen_covariates.py)
through each walker that can serve a group - carry-forward covariates, per-member factor rows, several covariates,
factors and derived values, knot edges, two occasions, a lag with derived constants (generated source), and the built-in
ODE bodies with descriptor-derived parameters (generated source, fixed-step and adaptive).

Bars, per case: analytical max(1e-10, 64 u kappa, 8 err_oracle) relative to the largest prediction; fixed-step ODE
max(64 u kappa, 8 err_oracle); adaptive max(8 err_oracle, 64 u kappa) against the true solution with a floor at 1e-3 of
the largest value; statuses equal the fixture's (0 everywhere).  err_oracle is the oracle's own error on the case
(tests/test_oracle_covariate_math.py; for "auto", which the oracle does not have, its DOPRI5 with an observation on every
knot).  An analytical launch carries the group's nine subjects - one whole chunk of 8 and a partial one, each with its
own knots, dose scale and truth - and mixes the group's cases over the support points, so neither a member reading
another member's factor row nor a bad lane behind a good one can pass.  Every launch asserts the kernel that served it."""
import math
import time

import numpy as np
import pytest

from pharmsol_amd import Data, _abi, _ffi, runtime
from tests.test_gpu_edge_accuracy import EM, cycle, expected_loglik, pair_chunks
from tests.test_oracle_covariate_math import (ANALYTICAL, GROUPS, NAMES, ODE, U, adaptive_cases, bar, build_model, build_population,
                                              oracle_errors, rel_err_floor)

pytestmark = pytest.mark.gpu

SWITCHES = ("PMX_DISABLE_CLASSING", "PMX_DISABLE_DYN3", "PMX_TUNE_PROP_SLOTS", "PMX_TUNE_STEPS_PER_TRIP")
GRID_P = (63, 64, 257)  # a partial wave, a whole one, a second tile with one live lane
ODE_GRID_P = (33, 257)
ODE_PAIR_P = (7, 31)
WORST = {}  # walker -> (err / bar, where)
TIMES = {}
_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    for w, (r, where) in sorted(WORST.items()):
        print(f"COV-WORST {w:44s} err/bar {r:.3e}  {where}")
    slow = max(TIMES, key=TIMES.get) if TIMES else "-"
    print(f"COV-TIME module {time.time() - t0:.1f} s, slowest {slow} {TIMES.get(slow, 0.0):.1f} s")


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    TIMES[request.node.name] = time.time() - t0


@pytest.fixture
def env(monkeypatch):
    """Set developer switches for one test and re-read them; restored (and re-read) afterwards."""

    def set_(**kw):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            monkeypatch.setenv(k, v)
        _ffi.lib().pmx_debug_reload_env()

    yield set_
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    _ffi.lib().pmx_debug_reload_env()


def note(walker, ratio, where):
    if not np.isfinite(ratio):
        ratio = math.inf
    if ratio > WORST.get(walker, (-1.0,))[0]:
        WORST[walker] = (ratio, where)


def model_of(g, **kw):
    """One model per (group, solver settings) and module: the run-time compile is the slow part."""
    key = (g, tuple(sorted(kw.items())))
    if key not in _MODELS:
        _MODELS[key] = build_model(GROUPS[g], **kw)
    return _MODELS[key]


def launch(m, flat, theta, expect, batch=False):
    import torch

    pop = runtime.DevicePopulation(flat, 0)
    pred, status = runtime.predict(m, pop, np.ascontiguousarray(theta), batch=batch)
    torch.cuda.synchronize()
    name = runtime.last_kernel_name()
    assert name == expect, f"routed to {name}, expected {expect}"
    return pred.cpu().numpy().reshape(flat.n_observations, -1), status.cpu().numpy().reshape(flat.n_subjects, -1)


def check(g, m, flat, truth, idx, expect, bars, thetas, batch=False, walker=None, err_fn=None):
    """One launch; idx[k] = the case of support point k (of subject k in a batch).  Returns the raw predictions."""
    group = GROUPS[g]
    S, P = len(truth), len(idx)
    assert not batch or P == S
    pred, status = launch(m, flat, np.array([thetas[i] for i in idx]), expect, batch)
    n_obs = truth[0].shape[0]
    walker = walker or expect
    for s in range(S):
        rows = pred[s * n_obs:(s + 1) * n_obs]
        for k in ([s] if batch else range(P)):
            c, col = idx[k], 0 if batch else k
            where = f"{group['name']}[{c}] subject {s} P={P}"
            assert status[s, col] == 0, f"{walker}: {where}: status {status[s, col]}"
            got, want = rows[:, col], truth[s][:, c]
            assert np.isfinite(got).all(), f"{walker}: {where}: {got}"
            err = err_fn(got, want) if err_fn else float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
            note(walker, err / bars[c], f"{group['name']}[{c}]")
            assert err <= bars[c], f"{walker}: {where}: err {err:.3e} > bar {bars[c]:.3e}"
    return pred


# ------------------------------------------------------------------------------------------------------ analytical
def grid_route(group):
    """The GRID walker of a group, from the launch path's rules (pmx_launch.cpp key_for / plan_routes)."""
    mdl = group["model"]
    if mdl.get("lag"):  # lag with covariate-derived constants: the closure walker on generated source
        return "pmx_jit_analytical_grid"
    infusion = any(e[0] == "inf" for occ in group["occasions"] for e in occ)
    if mdl["kernel"].startswith("three"):  # the matrix-free walker takes populations without infusions
        return "pmx_analytical_grid<dyn>" if infusion else "pmx_analytical_dyn3"
    if mdl["kernel"] == "two_compartments_with_absorption":  # classes of covariate models: one and two states only
        return "pmx_analytical_grid<dyn>"
    return "pmx_analytical_classed<dyn>"


def pair_route(group):
    return "pmx_jit_analytical_pair" if group["model"].get("lag") else "pmx_analytical_pair<dyn>"


def analytical(g, n=None):
    """(model, flat population of the nine subjects, truth per subject, bars per case, thetas)."""
    group = GROUPS[g]
    errs, status = oracle_errors(g)
    assert (status == 0).all()
    for c, case in enumerate(group["cases"]):  # a wrong oracle must not widen the device's bar
        assert errs[c] <= bar(group, case), f"{group['name']}[{c}]: the oracle itself misses the fixture"
    m = model_of(g)
    subs, truth = build_population(group, n)
    return (m, m.flatten(Data(subs)), truth, [bar(group, c, e) for c, e in zip(group["cases"], errs)],
            [c["theta"] for c in group["cases"]])


def keeps_eigenvalues(m, flat, env, slots):
    """Which dyn3 instantiation the host chooses, read from the op stream it compiles: <eigr> when some PROP repeats the
    rate constants of the one built before it (SameFac, bit 27)."""
    env(**({} if slots is None else {"PMX_TUNE_PROP_SLOTS": slots}))
    ops = runtime.compile_ops(m, flat)
    return bool(np.any((ops["kind"] == _abi.PMX_OP_PROP) & ((ops["flags"] & 8) != 0)))


def every_analytical_mapping(g, env, slots=None):
    group = GROUPS[g]
    m, flat, truth, bars, thetas = analytical(g)
    route = walker = grid_route(group)
    sw = {} if slots is None else {"PMX_TUNE_PROP_SLOTS": slots}
    tag = "" if slots is None else f" slots={slots}"
    if route == "pmx_analytical_dyn3":
        eigr = keeps_eigenvalues(m, flat, env, slots)
        if group["name"].startswith("a_"):  # a carry-forward covariate repeats rate constants between its jumps
            assert eigr == (slots != "0"), "the step covariate must reach dyn3<eigr> (and plain dyn3 without slots)"
        walker = route + ("<eigr>" if eigr else "")
    env(**sw)
    for P in GRID_P:
        check(g, m, flat, truth, cycle(group, P), route, bars, thetas, walker=walker + tag)
    for idx in pair_chunks(group):
        check(g, m, flat, truth, idx, pair_route(group), bars, thetas, walker=pair_route(group) + tag)
    check(g, m, flat, truth, cycle(group, len(truth)), pair_route(group), bars, thetas, batch=True,
          walker=pair_route(group) + "(batch)" + tag)
    if route == "pmx_analytical_dyn3":
        env(PMX_DISABLE_DYN3="1", **sw)
        check(g, m, flat, truth, cycle(group, 64), "pmx_analytical_grid<dyn>", bars, thetas, walker="pmx_analytical_grid<dyn>" + tag)
    elif route == "pmx_analytical_classed<dyn>":
        env(PMX_DISABLE_CLASSING="1", **sw)
        check(g, m, flat, truth, cycle(group, 64), "pmx_analytical_grid<dyn>", bars, thetas, walker="pmx_analytical_grid<dyn>" + tag)
    elif route == "pmx_analytical_grid<dyn>":  # (already the generic walker: the switches change nothing)
        env(PMX_DISABLE_CLASSING="1", PMX_DISABLE_DYN3="1", **sw)
        check(g, m, flat, truth, cycle(group, 64), "pmx_analytical_grid<dyn>", bars, thetas)


@pytest.mark.parametrize("g", ANALYTICAL, ids=[NAMES[g] for g in ANALYTICAL])
def test_analytical_walkers(g, env):
    every_analytical_mapping(g, env)


STEP = [g for g in ANALYTICAL if NAMES[g].startswith("a_")]


@pytest.mark.parametrize("slots", ["0", "1", "2"])
@pytest.mark.parametrize("g", STEP, ids=[NAMES[g] for g in STEP])
def test_step_covariate_under_every_slot_count(g, slots, env):
    """0, 1 and 2 kept-segment slots: the slot count and the evictions differ (tests/test_oracle_covariate_math.py
    asserts the situations each stream contains); without slots the plain dyn3 instantiation runs."""
    every_analytical_mapping(g, env, slots)


def test_both_dyn3_instantiations_are_reached(env):
    """<eigr> by the step covariate; plain dyn3 by covariates interpolated at the segment's absolute end."""
    reached = set()
    for g in ANALYTICAL:
        if grid_route(GROUPS[g]) == "pmx_analytical_dyn3":
            m, flat, _, _, _ = analytical(g)
            reached.add(keeps_eigenvalues(m, flat, env, None))
    assert reached == {True, False}


# ------------------------------------------------------------------------------------------------------------- ODE
def ode_kernel(group, solver, pair):
    lag = "<lag>" if group["model"]["lag"] else ""
    return f"pmx_jit_ode_{solver.replace('-', '_')}_{'pair' if pair else 'grid'}{lag}"


def every_ode_mapping(g, m, solver, truth_of, bars, thetas, env, tripped=(None,), err_fn=None):
    """GRID at both sizes, PAIR at both sizes and the batch form; under every steps-per-trip setting in `tripped` the PAIR
    outputs are bit-identical."""
    group = GROUPS[g]
    out = {}
    subs, truth = truth_of(None)
    flat = m.flatten(Data(subs))
    n_cases = len(thetas)
    idx_of = lambda n: np.arange(n) % n_cases  # noqa: E731
    env()
    for P in ODE_GRID_P:
        check(g, m, flat, truth, idx_of(P), ode_kernel(group, solver, False), bars, thetas, err_fn=err_fn)
    for t in tripped:
        env(**({} if t is None else {"PMX_TUNE_STEPS_PER_TRIP": t}))
        tag = "" if t is None else f" steps/trip={t}"
        name = ode_kernel(group, solver, True)
        for P in ODE_PAIR_P:
            got = check(g, m, flat, truth, idx_of(P), name, bars, thetas, walker=name + tag, err_fn=err_fn)
            np.testing.assert_array_equal(got, out.setdefault(P, got), err_msg=f"{name}{tag}: P={P} differs from the default trip")
        got = check(g, m, flat, truth, idx_of(len(truth)), name, bars, thetas, batch=True, walker=name + "(batch)" + tag, err_fn=err_fn)
        np.testing.assert_array_equal(got, out.setdefault("batch", got), err_msg=f"{name}{tag}: batch differs from the default trip")


def fixed_step(g):
    group = GROUPS[g]
    errs, status = oracle_errors(g)
    assert (status == 0).all()
    for c, case in enumerate(group["cases"]):
        assert errs[c] <= bar(group, case), f"{group['name']}[{c}]: the oracle itself misses the fixture"
    return [bar(group, c, e) for c, e in zip(group["cases"], errs)], [c["theta"] for c in group["cases"]]


@pytest.mark.parametrize("g", ODE, ids=[NAMES[g] for g in ODE])
def test_ode_rk4_every_mapping(g, env):
    group = GROUPS[g]
    bars, thetas = fixed_step(g)
    tripped = (None, "1", "5") if group["model"]["lag"] else (None,)  # (one group: a trip boundary is bookkeeping only)
    every_ode_mapping(g, model_of(g), "rk4", lambda n: build_population(group, n), bars, thetas, env, tripped)


ADAPTIVE = [(g, s, k) for g in ODE if "adaptive" in GROUPS[g]
            for s, k in (("dopri5", "boundary"), ("ros2", "boundary"), ("ros2", "interior"), ("auto", "boundary"), ("auto", "interior"))]


@pytest.mark.parametrize("g,solver,knots", ADAPTIVE, ids=[f"{NAMES[g]}-{s}-{k}" for g, s, k in ADAPTIVE])
def test_ode_adaptive_against_the_true_solution(g, solver, knots, env):
    """"dopri5" on knots that are piece boundaries; "ros2" and "auto" also on knots strictly inside a piece and on a
    stage time (tests/golden/gen_covariates.py says why)."""
    group = GROUPS[g]
    ad = group["adaptive"]
    _, cases = adaptive_cases(group, knots)
    kappa = group["cases"][0]["kappa"]  # (the fixed-step walk's; far below 8 err_oracle)
    for tol in ad["tols"]:
        errs, status = oracle_errors(g, solver, tol, knots)
        assert (status == 0).all()
        if solver != "auto":
            assert (errs <= 10.0 * tol).all()  # (the cap tests/test_oracle_covariate_math.py sets)
        bars = [max(8.0 * e, 64.0 * U * kappa) for e in errs]
        m = model_of(g, solver=solver, h_max=ad["h_max"], rtol=tol, atol=tol)
        every_ode_mapping(g, m, solver, lambda n: build_population(group, n, adaptive=knots), bars, [c["theta"] for c in cases], env,
                          err_fn=rel_err_floor)


# ------------------------------------------------------------------------------------------------ fused log-likelihood
def check_ll(g, m, flat, truth, idx, expect, bars, thetas):
    import torch

    group = GROUPS[g]
    n_obs = truth[0].shape[0]
    rng = np.random.default_rng(5)
    y = [np.abs(truth[s][:, 0]) * np.exp(rng.normal(0, 0.2, n_obs)) + 0.05 for s in range(len(truth))]
    flat.ev_value = flat.ev_value.copy()
    flat.ev_value[flat.ev_kind == _abi.PMX_EV_OBSERVATION] = np.concatenate(y)
    pop = runtime.DevicePopulation(flat, 0)
    ll, st = runtime.loglik(m, pop, EM, np.array([thetas[i] for i in idx]))
    torch.cuda.synchronize()
    assert runtime.last_kernel_name() == expect, runtime.last_kernel_name()
    ll, st = ll.cpu().numpy(), st.cpu().numpy()
    for s in range(len(truth)):
        for k, c in enumerate(idx):
            assert st[s, k] == 0
            want, slope = expected_loglik(y[s], truth[s][:, c])
            tol = slope * bars[c] * float(np.max(np.abs(truth[s][:, c]))) + 1e-13 * (abs(want) + n_obs)
            note(expect + " (loglik)", abs(ll[s, k] - want) / tol, f"{group['name']}[{c}]")
            assert abs(ll[s, k] - want) <= tol, f"{expect}: {group['name']}[{c}] subject {s}: {ll[s, k]!r} vs {want!r}"


LL_ANALYTICAL = [g for g in ANALYTICAL if NAMES[g].startswith(("a_", "c_"))]


def ll_grid_route(group):
    route = grid_route(group)
    return "pmx_analytical_classed<ll,dyn>" if route == "pmx_analytical_classed<dyn>" else route


@pytest.mark.parametrize("g", LL_ANALYTICAL, ids=[NAMES[g] for g in LL_ANALYTICAL])
def test_loglik_analytical(g, env):
    group = GROUPS[g]
    m, flat, truth, bars, thetas = analytical(g)
    env()
    check_ll(g, m, flat, truth, cycle(group, 64), ll_grid_route(group), bars, thetas)
    for idx in pair_chunks(group):
        check_ll(g, m, flat, truth, idx, pair_route(group), bars, thetas)


def test_loglik_ode(env):
    g = NAMES.index("g_one_cmt_oral_fixed_lag")
    group = GROUPS[g]
    bars, thetas = fixed_step(g)
    m = model_of(g)
    subs, truth = build_population(group)
    flat = m.flatten(Data(subs))
    env()
    check_ll(g, m, flat, truth, np.arange(ODE_GRID_P[0]) % len(thetas), ode_kernel(group, "rk4", False), bars, thetas)
    check_ll(g, m, flat, truth, np.arange(ODE_PAIR_P[0]) % len(thetas), ode_kernel(group, "rk4", True), bars, thetas)
