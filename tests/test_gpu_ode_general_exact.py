"""The ROS2 and auto walkers on user bodies outside the compartmental class: tests/golden/ode_exact_general.json (mpmath,
40 digits; tests/golden/gen_ode_exact_general.py) through the GRID, PAIR and batched PAIR mappings of the hiprtc-compiled
bodies of tests/general_ode_bodies.py - a growing state held stable by feedback (2 states, and at either end of 8) and a
predator-prey pair - and through the fused log-likelihood.  tests/test_oracle_ode_general_exact.py derives the bars.

Forced-step ROS2 and the pivot ladder, every prediction:  |gpu - fixture| / max|fixture| <= max(64 u kappa, 8 err_oracle,
diff_noise) per case, status 0.  The ladder's five rungs - one step each from (1024, 0, ...) with a pivot of 2^-4 .. 2^-44
in a well-conditioned W, diff_noise 0 - are five support points of one subject, so they sit in neighbouring lanes of one
wave in every launch; elimination in the natural order misses the two lowest by 1e4 .. 1e8 bars.  Launches are those of
tests/test_gpu_ode_exact.py: the cases cycled over the support points (GRID 33 and 257, PAIR 7 and 31, batch), nine copies
of the subject, dose-scaled where the truth is linear, the serving kernel asserted, PAIR under the default steps per trip
and under 1 and 5 with bit-identical results.

Auto on the forced-step schedules: no lane switches (the generator asserts the stiffness quotient calm at every step), so
every lane must return the forced DOPRI5 values at 64 u kappa (+ 8 err_oracle) with the statistics (n_steps, 0, 0, 0).

Adaptive ROS2 and auto at rtol = atol = 1e-6 against the 40-digit solution (largest error relative to the largest
value): within 4 x the error the CPU oracle achieves on the case (`oracle_err` of the fixture, which the oracle
module holds today's oracle to) and within 1e-4 whatever the oracle does."""
import numpy as np
import pytest

from tests import test_gpu_ode_exact as base
from tests.test_gpu_ode_exact import TRIPS, env, every_mapping  # noqa: F401
from tests.test_gpu_ode_stiff_exact import loglik_every_mapping
from tests.test_oracle_ode_exact import U
from tests.test_oracle_ode_general_exact import (ADAPTIVE, ADAPTIVE_NAMES, CAP, GROUPS, LADDER, LADDER_NAMES, NAMES, bar,
                                                 model_of, oracle_run)

pytestmark = pytest.mark.gpu

LL_ROS2 = ["feedback2", "feedback8_tail"]
OK = np.zeros(8, dtype=np.uint8)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """The module's worst err / bar per walker (the shared table is set aside for the module and merged back)."""
    before = dict(base.WORST)
    base.WORST.clear()
    yield
    for w, (r, eu, where) in sorted(base.WORST.items()):
        print(f"ODE-GENERAL-EXACT-WORST {w:44s} err/bar {r:.3e}  err/u {eu:.3g}  {where}")
    for w, v in before.items():
        if v[0] > base.WORST.get(w, (-1.0,))[0]:
            base.WORST[w] = v


def ros2_cases(group):
    """(cases, expected [n_obs, n_cases], status, bars) of a group's forced-step or ladder cases."""
    cases = group["cases"]
    _, status_o, errs_o = oracle_run(group, "ros2", "ros2")
    assert (status_o == 0).all()
    for c, e in zip(cases, errs_o):  # a wrong oracle must not widen the device's bar
        cap = 8.0 * c["diff_noise"] + 64.0 * U * c["kappa"]
        assert e <= cap, f"{group['name']}: the oracle itself misses the fixture ({e:.3e} > {cap:.3e})"
        c["scale_of"] = c["ros2"]
    want = np.array([c["ros2"] for c in cases]).T
    return cases, want, OK[:len(cases)], [bar(c, e) for c, e in zip(cases, errs_o)]


# ---------------------------------------------------------------------------------------------------- forced-step ROS2
@pytest.mark.parametrize("g", range(len(GROUPS)), ids=NAMES)
def test_ros2_forced_steps_every_mapping(g, env):
    group = GROUPS[g]
    cases, want, wst, bars = ros2_cases(group)
    every_mapping(group, model_of(group, "ros2"), "ros2", cases, want, wst, bars, env, TRIPS)


# -------------------------------------------------------------------------------------------------------- pivot ladder
@pytest.mark.parametrize("g", range(len(LADDER)), ids=LADDER_NAMES)
def test_ros2_pivot_ladder_every_mapping(g, env):
    group = LADDER[g]
    cases, want, wst, bars = ros2_cases(group)
    assert [c["rung"] for c in cases] == [4, 12, 24, 36, 44]  # five neighbouring lanes in every launch
    every_mapping(group, model_of(group, "ros2"), "ros2", cases, want, wst, bars, env, TRIPS)


# ---------------------------------------------------------------------------------------------------------------- auto
@pytest.mark.parametrize("g", range(len(GROUPS)), ids=NAMES)
def test_auto_lanes_that_never_switch_take_the_exact_dopri5_steps(g, env):
    group = GROUPS[g]
    d = group["dopri5"]
    cases = d["cases"]
    args = dict(h_max=d["h_max"], rtol=d["rtol"], atol=d["atol"])
    _, status_o, errs_o = oracle_run(group, "dopri5", "dopri5", cases=cases, **args)
    assert (status_o == 0).all()
    for c, e in zip(cases, errs_o):
        assert e <= 64.0 * U * c["kappa"], f"{group['name']}: the oracle itself misses the fixture ({e:.3e})"
        c["scale_of"] = c["dopri5"]
    want = np.array([c["dopri5"] for c in cases]).T
    bars = [max(64.0 * U * c["kappa"], 8.0 * e) for c, e in zip(cases, errs_o)]
    every_mapping(group, model_of(group, "auto", **args), "auto", cases, want, OK[:len(cases)], bars, env, (None,),
                  wstats=[c["counts"] for c in cases])


# ------------------------------------------------------------------------------------------------------------ adaptive
@pytest.mark.parametrize("solver", ["ros2", "auto"])
@pytest.mark.parametrize("g", range(len(ADAPTIVE)), ids=ADAPTIVE_NAMES)
def test_adaptive_solvers_against_the_true_solution(g, solver, env):
    group = ADAPTIVE[g]
    cases = group["cases"]
    for c in cases:
        c["scale_of"] = c["exact"]
    want = np.array([c["exact"] for c in cases]).T
    bars = [min(4.0 * c["oracle_err"][solver], CAP) for c in cases]
    every_mapping(group, model_of(group, solver), solver, cases, want, OK[:len(cases)], bars, env, (None,))


# ------------------------------------------------------------------------------------------------ fused log-likelihood
@pytest.mark.parametrize("name", LL_ROS2)
def test_fused_loglik_ros2(name, env):
    group = GROUPS[NAMES.index(name)]
    cases, want, wst, bars = ros2_cases(group)
    loglik_every_mapping(group, model_of(group, "ros2"), "ros2", cases, want, wst, bars, "ros2", env)
