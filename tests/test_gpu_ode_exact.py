"""Every ODE walker against exact-arithmetic RK4 / DOPRI5 steps: tests/golden/ode_exact.json (mpmath, 40 digits;
tests/golden/gen_ode_exact.py) through the GRID, PAIR and batched PAIR mappings of the built-in bodies, the `<lag>`
instantiations, the hiprtc-compiled custom bodies, the checked solver and the fused log-likelihood.

Bar for every prediction of a fixed-step case:  |gpu - fixture| / max|fixture| <= max(64 u kappa, 8 err_oracle), per
case (no floor: kappa is about n_steps, the bar about 1e-12, while RK4's own distance to the true solution on the hard
cases is 1e-6 .. 1e-2).  The factor 8 over the oracle's own error on the same case allows for another contraction and
summation order on the device.  Adaptive launches are held to max(8 err_oracle, 64 u kappa) against the true solution,
measured with a floor at 1e-3 of the largest value.  The status of every (subject, support point) equals the fixture's.

A launch mixes the group's cases (the easy one first) over the support points and 9 copies of the case's subject - with
every dose scaled where the truth is linear in the doses - so a bad lane cannot hide behind a good one.  Every launch
asserts the kernel that served it.  The PAIR launches run under the default number of steps per trip and under 1 and 5:
the three outputs must be bit-identical (a trip boundary is bookkeeping, not arithmetic), which covers the custom
bodies' stage-time bookkeeping and the checked solver's probe trigger across trips."""
import math

import numpy as np
import pytest

from pharmsol_amd import Data, _abi, _ffi, runtime
from tests.test_gpu_edge_accuracy import EM, expected_loglik
from tests.test_oracle_ode_exact import (GROUPS, NAMES, U, bar, build_model, build_subject, checked_cases, fixed_cases,
                                         is_custom, oracle_adaptive, oracle_fixed, rel_err_floor)

pytestmark = pytest.mark.gpu

SCALES = (1.0, 2.0, 0.5, 3.0, 0.25, 1.5, 4.0, 0.75, 5.0)
SWITCHES = ("PMX_TUNE_STEPS_PER_TRIP", "PMX_TUNE_GRID_MIN_P")
GRID_P = (33, 257)  # a partial wave; a second tile with one live lane
PAIR_P = (7, 31)    # 63 pairs: a partial wave; 279 pairs: a partial second block
TRIPS = (None, "1", "5")
WORST = {}  # walker -> (err / bar, err / u, where)

BUILTIN = [g for g in range(len(GROUPS)) if not is_custom(GROUPS[g])]
CUSTOM = [g for g in range(len(GROUPS)) if is_custom(GROUPS[g])]
ADAPTIVE = [(g, s) for g in range(len(GROUPS)) for s in ("dopri5", "ros2") if GROUPS[g]["adaptive"][s]]
LL_GROUPS = [NAMES.index("two_cmt_iv"), NAMES.index("one_cmt_oral_lag_fa")]


def gid(gs):
    return [NAMES[g] for g in gs]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for w, (r, eu, where) in sorted(WORST.items()):
        print(f"ODE-EXACT-WORST {w:44s} err/bar {r:.3e}  err/u {eu:.1f}  {where}")


def note(walker, err, b, where):
    r = err / b if np.isfinite(err) else math.inf
    if r > WORST.get(walker, (-1.0,))[0]:
        WORST[walker] = (r, err / U, where)


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


def trips(env, t):
    env(**({} if t is None else {"PMX_TUNE_STEPS_PER_TRIP": t}))


def kernel_name(group, solver, pair):
    lag = "<lag>" if group["model"]["lag"] else ""
    return f"pmx_{'jit_' if is_custom(group) else ''}ode_{solver.replace('-', '_')}_{'pair' if pair else 'grid'}{lag}"


def population(group, model, n_copies=len(SCALES)):
    """(flat population, dose scale per subject): `n_copies` copies of the group's subject, dose-scaled where that
    scales the truth."""
    scales = [SCALES[i % len(SCALES)] if group["scalable"] else 1.0 for i in range(n_copies)]
    subs = [build_subject(group, s, name=f"c{i}") for i, s in enumerate(scales)]
    return model.flatten(Data(subs)), scales


def launch(model, flat, theta, expect, batch=False, stats=False):
    """-> (predictions, status); stats (auto solver): also the four step counts per pair, [n_subjects, n, 4]."""
    import torch

    pop = runtime.DevicePopulation(flat, 0)
    out = runtime.predict(model, pop, np.ascontiguousarray(theta), batch=batch, solver_stats=stats)
    torch.cuda.synchronize()
    name = runtime.last_kernel_name()
    assert name == expect, f"routed to {name}, expected {expect}"
    res = (out[0].cpu().numpy().reshape(flat.n_observations, -1), out[1].cpu().numpy().reshape(flat.n_subjects, -1))
    return res + ((out[2].cpu().numpy().reshape(flat.n_subjects, -1, 4),) if stats else ())


def check(group, model, cases, want, wstatus, bars, idx, expect, batch=False, walker=None, err_fn=None, wstats=None):
    """One launch; idx[k] = the case of support point k (of subject k in a batch).  want [n_obs, n_cases] may hold NaN
    (rows a checked lane refuses).  wstats (auto solver): the four step counts of every case, which every pair's
    statistics record must equal.  Returns the raw predictions."""
    n = len(idx)
    flat, scales = population(group, model, n if batch else len(SCALES))
    theta = np.array([cases[i]["theta"] for i in idx])
    pred, status, *stats = launch(model, flat, theta, expect, batch, stats=wstats is not None)
    n_obs = want.shape[0]
    walker = walker or expect
    for s, scale in enumerate(scales):
        rows = pred[s * n_obs:(s + 1) * n_obs]
        for k in ([s] if batch else range(n)):
            c = idx[k]
            col = 0 if batch else k
            where = f"{group['name']}[{c}] subject {s} P={n}"
            assert status[s, col] == wstatus[c], f"{walker}: {where}: status {status[s, col]}, fixture {wstatus[c]}"
            if wstats is not None:
                assert list(stats[0][s, col]) == list(wstats[c]), f"{walker}: {where}: steps {stats[0][s, col]}, fixture {wstats[c]}"
            got, w = rows[:, col], want[:, c] * scale
            bad = np.isnan(w)
            assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all(), f"{walker}: {where}: {got}"
            if err_fn:
                err = err_fn(got, w)
            else:  # relative to the case's largest prediction (of the unrefused walk)
                err = float(np.max(np.abs(got[~bad] - w[~bad]))) / (float(np.max(np.abs(cases[c]["scale_of"]))) * scale)
            note(walker, err, bars[c], where)
            assert err <= bars[c], f"{walker}: {where}: err {err:.3e} > bar {bars[c]:.3e} (err/u {err / U:.1f})"
    return pred


def fixed(group_index, kind):
    """(cases, model arguments, expected [n_obs, n_cases], status, bars) of a group's fixed-step cases."""
    group = GROUPS[group_index]
    cases, args, key = fixed_cases(group, kind)
    _, status_o, errs_o = oracle_fixed(group_index, kind)
    assert (status_o == 0).all()
    for c, e in zip(cases, errs_o):  # a wrong oracle must not widen the device's bar
        assert e <= bar(c), f"{group['name']}: the oracle itself misses the fixture ({e:.3e} > {bar(c):.3e})"
        c["scale_of"] = c[key]
    want = np.array([c[key] for c in cases]).T
    return cases, args, want, np.zeros(len(cases), dtype=np.uint8), [bar(c, e) for c, e in zip(cases, errs_o)]


def cycle(cases, n):
    return np.arange(n) % len(cases)


def every_mapping(group, model, solver, cases, want, wstatus, bars, env, tripped, **kw):
    """GRID at both sizes, PAIR at both sizes and the batch form; the PAIR launches under every steps-per-trip setting
    in `tripped`, bit-identical to one another.  Returns {shape: predictions} of the default setting."""
    out = {}
    trips(env, None)
    for P in GRID_P:
        out[P] = check(group, model, cases, want, wstatus, bars, cycle(cases, P), kernel_name(group, solver, False), **kw)
    n_batch = max(len(SCALES), len(cases))
    for t in tripped:
        trips(env, t)
        tag = "" if t is None else f" steps/trip={t}"
        for P in PAIR_P:
            name = kernel_name(group, solver, True)
            got = check(group, model, cases, want, wstatus, bars, cycle(cases, P), name, walker=name + tag, **kw)
            np.testing.assert_array_equal(got, out.setdefault(P, got), err_msg=f"{name}{tag}: P={P} differs from the default trip")
        name = kernel_name(group, solver, True)
        got = check(group, model, cases, want, wstatus, bars, cycle(cases, n_batch), name, batch=True,
                    walker=name + "(batch)" + tag, **kw)
        np.testing.assert_array_equal(got, out.setdefault("batch", got), err_msg=f"{name}{tag}: batch differs from the default trip")
    return out


# ------------------------------------------------------------------------------------------------- plain fixed-step RK4
@pytest.mark.parametrize("g", BUILTIN + CUSTOM, ids=gid(BUILTIN + CUSTOM))
def test_rk4_every_mapping(g, env):
    group = GROUPS[g]
    cases, args, want, wst, bars = fixed(g, "rk4")
    every_mapping(group, build_model(group, **args), "rk4", cases, want, wst, bars, env, TRIPS)


# --------------------------------------------------------------------------------------------------------- checked RK4
@pytest.mark.parametrize("g", BUILTIN + CUSTOM, ids=gid(BUILTIN + CUSTOM))
def test_checked_rk4_every_mapping(g, env):
    """The verdicts and the refused rows of the fixture; lanes that pass are bit-identical to plain RK4's in the launch
    of the same shape.  steps per trip = 1: the probe consumes a whole trip."""
    group = GROUPS[g]
    ck = group["checked"]
    all_cases, _, _, _, all_bars = fixed(g, "rk4")
    cases, want, wst = checked_cases(group)
    bars = [all_bars[c["case"]] for c in ck["cases"]]
    for c in cases:
        c["scale_of"] = c["rk4"]
    checked = every_mapping(group, build_model(group, solver="rk4-checked", rtol=ck["rtol"], atol=ck["atol"]), "rk4-checked",
                            cases, want, wst, bars, env, TRIPS)
    full = np.array([c["rk4"] for c in cases]).T
    plain = every_mapping(group, build_model(group, solver="rk4"), "rk4", cases, full, np.zeros(len(cases), dtype=np.uint8),
                          bars, env, (None,))
    for shape, got in checked.items():
        ok = ~np.isnan(got)
        assert ok.any() and (~ok).any()  # both kinds of lane in every launch
        np.testing.assert_array_equal(got[ok], plain[shape][ok], err_msg=f"{group['name']} {shape}: passing lanes differ from plain RK4")


# --------------------------------------------------------------------------------------------------- forced-step DOPRI5
@pytest.mark.parametrize("g", BUILTIN + CUSTOM, ids=gid(BUILTIN + CUSTOM))
def test_dopri5_forced_steps_every_mapping(g, env):
    group = GROUPS[g]
    cases, args, want, wst, bars = fixed(g, "dopri5")
    tripped = TRIPS if group["model"]["body"] == "custom_nonaut" else (None,)
    every_mapping(group, build_model(group, **args), "dopri5", cases, want, wst, bars, env, tripped)


# ------------------------------------------------------------------------------------------------------------ adaptive
@pytest.mark.parametrize("g,solver", ADAPTIVE, ids=[f"{NAMES[g]}-{s}" for g, s in ADAPTIVE])
def test_adaptive_solvers_against_the_true_solution(g, solver, env):
    group = GROUPS[g]
    ad = group["adaptive"]
    cases = ad[solver]
    want = np.array([c["exact"] for c in cases]).T
    kappa = group["cases"][0]["kappa"]  # (the fixed-step walk's; the floor is far below 8 err_oracle)
    for tol in ad["tols"]:
        status_o, errs_o = oracle_adaptive(g, solver, tol)
        assert (status_o == 0).all() and (errs_o <= 10.0 * tol).all()  # (the cap tests/test_oracle_ode_exact.py sets)
        bars = [max(8.0 * e, 64.0 * U * kappa) for e in errs_o]
        model = build_model(group, solver=solver, h_max=ad["h_max"], rtol=tol, atol=tol)
        every_mapping(group, model, solver, cases, want, np.zeros(len(cases), dtype=np.uint8), bars, env, (None,),
                      err_fn=rel_err_floor)


# ------------------------------------------------------------------------------------------------ fused log-likelihood
def check_ll(group, model, cases, want, wstatus, bars, idx, expect, key="rk4"):
    import torch

    flat, scales = population(group, model)
    n_obs = want.shape[0]
    full = np.array([c[key] for c in cases]).T
    rng = np.random.default_rng(5)
    y = [np.abs(full[:, 0] * s) * np.exp(rng.normal(0, 0.2, n_obs)) + 0.05 for s in scales]
    flat.ev_value = flat.ev_value.copy()
    flat.ev_value[flat.ev_kind == _abi.PMX_EV_OBSERVATION] = np.concatenate(y)
    theta = np.array([cases[i]["theta"] for i in idx])
    pop = runtime.DevicePopulation(flat, 0)
    ll, st = runtime.loglik(model, pop, EM, theta)
    torch.cuda.synchronize()
    assert runtime.last_kernel_name() == expect, runtime.last_kernel_name()
    ll, st = ll.cpu().numpy(), st.cpu().numpy()
    for s, scale in enumerate(scales):
        for k, c in enumerate(idx):
            assert st[s, k] == wstatus[c]
            if wstatus[c]:
                assert np.isnan(ll[s, k])
                continue
            truth = full[:, c] * scale
            w, slope = expected_loglik(y[s], truth)
            tol = slope * bars[c] * float(np.max(np.abs(truth))) + 1e-13 * (abs(w) + n_obs)
            note(expect + " (loglik)", abs(ll[s, k] - w), tol, f"{group['name']}[{c}]")
            assert abs(ll[s, k] - w) <= tol, f"{expect}: {group['name']}[{c}] subject {s}: {ll[s, k]!r} vs {w!r}"
    return flat, y


@pytest.mark.parametrize("solver", ["rk4", "rk4-checked"])
@pytest.mark.parametrize("g", LL_GROUPS, ids=gid(LL_GROUPS))
def test_fused_loglik(g, solver, env):
    group = GROUPS[g]
    ck = group["checked"]
    _, _, _, _, all_bars = fixed(g, "rk4")
    if solver == "rk4":
        cases, args, want, wst, bars = fixed(g, "rk4")
    else:
        cases, want, wst = checked_cases(group)
        bars = [all_bars[c["case"]] for c in ck["cases"]]
        args = dict(solver=solver, rtol=ck["rtol"], atol=ck["atol"])
    model = build_model(group, **args)
    env()
    check_ll(group, model, cases, want, wst, bars, cycle(cases, GRID_P[0]), kernel_name(group, solver, False))
    for t in TRIPS:
        trips(env, t)
        flat, y = check_ll(group, model, cases, want, wst, bars, cycle(cases, PAIR_P[0]), kernel_name(group, solver, True))
    # the batch host form: subject s with case s; a refused subject is -inf
    trips(env, None)
    idx = cycle(cases, len(SCALES))
    ll, st = runtime.loglik_batch_host(model, flat, EM, np.array([cases[i]["theta"] for i in idx]))
    np.testing.assert_array_equal(st, wst[idx])
    full = np.array([c["rk4"] for c in cases]).T
    _, scales = population(group, model)
    for s, c in enumerate(idx):
        if wst[c]:
            assert ll[s] == -np.inf
            continue
        truth = full[:, c] * scales[s]
        w, slope = expected_loglik(y[s], truth)
        assert abs(ll[s] - w) <= slope * bars[c] * float(np.max(np.abs(truth))) + 1e-13 * (abs(w) + len(truth))
