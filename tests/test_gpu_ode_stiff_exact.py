"""The ROS2 and auto walkers against exact-arithmetic steps: tests/golden/ode_exact_stiff.json (mpmath, 40 digits;
tests/golden/gen_ode_exact_stiff.py) through the GRID, PAIR and batched PAIR mappings of the built-in bodies, the `<lag>`
instantiations, the hiprtc-compiled bodies (8 states among them) and the fused log-likelihood.

Forced-step ROS2, every prediction:  |gpu - fixture| / max|fixture| <= max(64 u kappa, 8 err_oracle, diff_noise) per case,
status 0 (tests/test_oracle_ode_stiff_exact.py derives the terms and asserts that the oracle cannot widen the bar and that
each wrong stage, root, sign or Jacobian of the fixture's list moves some case by 100 bars or more).  Launches are those
of tests/test_gpu_ode_exact.py: the group's four cases (h lambda 0.05 .. 1000, the easy one in lane 0) cycled over the
support points, 9 dose-scaled copies of the subject where the truth is linear, the serving kernel asserted, PAIR under the
default steps per trip and under 1 and 5 with bit-identical results.

Auto: the fixture's deterministic switch (E x 15, I x 17, E x 19, I to the end) beside a lane that never switches, in
neighbouring lanes.  Predictions to max(64 u kappa, 8 err_ref, diff_noise), err_ref = the error of the numpy restatement
of the rule; the statistics record of every pair equals the fixture's four counts.  Lanes that never switch are also held
to the forced-step DOPRI5 values of ode_exact.json at that fixture's bar, with (n_steps, 0, 0, 0)."""
import numpy as np
import pytest

from pharmsol_amd import runtime
from tests import test_gpu_ode_exact as base
from tests.test_gpu_edge_accuracy import EM, expected_loglik
from tests.test_gpu_ode_exact import (GRID_P, PAIR_P, SCALES, TRIPS, check_ll, cycle, env, every_mapping,  # noqa: F401
                                      kernel_name, note, population, trips)
from tests.test_oracle_ode_exact import U, build_model
from tests.test_oracle_ode_stiff_exact import AUTO, AUTO_NAMES, GROUPS, NAMES, bar, model_of, oracle_ros2, restated_auto

pytestmark = pytest.mark.gpu

LL_ROS2 = ["one_cmt_oral_lag_fa", "custom_chain8"]


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The module's worst err / bar per walker (the shared table is set aside for the module and merged back)."""
    before = dict(base.WORST)
    base.WORST.clear()
    yield
    for w, (r, eu, where) in sorted(base.WORST.items()):
        print(f"ODE-STIFF-EXACT-WORST {w:44s} err/bar {r:.3e}  err/u {eu:.3g}  {where}")
    for w, v in before.items():
        if v[0] > base.WORST.get(w, (-1.0,))[0]:
            base.WORST[w] = v


def ros2_cases(g):
    """(cases, expected [n_obs, n_cases], status, bars) of a group's forced-step ROS2 cases."""
    group = GROUPS[g]
    cases = group["cases"]
    _, status_o, errs_o = oracle_ros2(g)
    assert (status_o == 0).all()
    for c, e in zip(cases, errs_o):  # a wrong oracle must not widen the device's bar
        cap = 8.0 * c["diff_noise"] + 64.0 * U * c["kappa"]
        assert e <= cap, f"{group['name']}: the oracle itself misses the fixture ({e:.3e} > {cap:.3e})"
        c["scale_of"] = c["ros2"]
    want = np.array([c["ros2"] for c in cases]).T
    return cases, want, np.zeros(len(cases), dtype=np.uint8), [bar(c, e) for c, e in zip(cases, errs_o)]


def auto_cases(g):
    """(cases, expected, status, bars, the four counts per case) of an auto group: the switching lane, the calm one."""
    group = AUTO[g]
    cases = group["cases"]
    bars = []
    for c, (_, counts, modes, err) in zip(cases, restated_auto(g)):
        assert counts == c["counts"] and modes == c["modes"]
        c["scale_of"] = c["auto"]
        bars.append(bar(c, err))
    want = np.array([c["auto"] for c in cases]).T
    return cases, want, np.zeros(len(cases), dtype=np.uint8), bars, [c["counts"] for c in cases]


# ---------------------------------------------------------------------------------------------------- forced-step ROS2
@pytest.mark.parametrize("g", range(len(GROUPS)), ids=NAMES)
def test_ros2_forced_steps_every_mapping(g, env):
    group = GROUPS[g]
    cases, want, wst, bars = ros2_cases(g)
    every_mapping(group, model_of(group, "ros2"), "ros2", cases, want, wst, bars, env, TRIPS)


# ---------------------------------------------------------------------------------------------------------------- auto
@pytest.mark.parametrize("g", range(len(AUTO)), ids=AUTO_NAMES)
def test_auto_switch_counts_and_values_every_mapping(g, env):
    group = AUTO[g]
    cases, want, wst, bars, counts = auto_cases(g)
    assert counts[0][3] == 3 and counts[1][1:] == [0, 0, 0]  # neighbouring lanes: one switches three times, one never
    every_mapping(group, model_of(group, "auto"), "auto", cases, want, wst, bars, env, TRIPS, wstats=counts)


@pytest.mark.parametrize("name", AUTO_NAMES)
def test_auto_lanes_that_never_switch_take_the_exact_dopri5_steps(name, env):
    g = base.NAMES.index(name)
    group = base.GROUPS[g]
    cases, args, want, wst, bars = base.fixed(g, "dopri5")
    model = build_model(group, **dict(args, solver="auto"))
    counts = [[c["n_steps"], 0, 0, 0] for c in cases]
    every_mapping(group, model, "auto", cases, want, wst, bars, env, (None,), wstats=counts)


# ------------------------------------------------------------------------------------------------ fused log-likelihood
def loglik_every_mapping(group, model, solver, cases, want, wst, bars, key, env):
    env()
    check_ll(group, model, cases, want, wst, bars, cycle(cases, GRID_P[0]), kernel_name(group, solver, False), key=key)
    for t in TRIPS:
        trips(env, t)
        flat, y = check_ll(group, model, cases, want, wst, bars, cycle(cases, PAIR_P[0]), kernel_name(group, solver, True), key=key)
    trips(env, None)  # the batch host form: subject s with case s
    idx = cycle(cases, len(SCALES))
    ll, st = runtime.loglik_batch_host(model, flat, EM, np.array([cases[i]["theta"] for i in idx]))
    np.testing.assert_array_equal(st, wst[idx])
    _, scales = population(group, model)
    for s, c in enumerate(idx):
        truth = want[:, c] * scales[s]
        w, slope = expected_loglik(y[s], truth)
        tol = slope * bars[c] * float(np.max(np.abs(truth))) + 1e-13 * (abs(w) + len(truth))
        note(kernel_name(group, solver, True) + " (loglik, batch host)", abs(ll[s] - w), tol, f"{group['name']}[{c}]")
        assert abs(ll[s] - w) <= tol, f"{group['name']}[{c}] subject {s}: {ll[s]!r} vs {w!r}"


@pytest.mark.parametrize("name", LL_ROS2)
def test_fused_loglik_ros2(name, env):
    g = NAMES.index(name)
    cases, want, wst, bars = ros2_cases(g)
    loglik_every_mapping(GROUPS[g], model_of(GROUPS[g], "ros2"), "ros2", cases, want, wst, bars, "ros2", env)


def test_fused_loglik_auto(env):
    g = AUTO_NAMES.index("custom_nonaut")
    cases, want, wst, bars, _ = auto_cases(g)
    loglik_every_mapping(AUTO[g], model_of(AUTO[g], "auto"), "auto", cases, want, wst, bars, "auto", env)
