"""What a FAILED pair's log-likelihood slot and status byte hold, on every per-lane walker (include/pmx.h, pair status).

The finish rule every walker shares: a pair whose status is neither PMX_PAIR_OK nor PMX_PAIR_NONFINITE stores NaN in its
log-likelihood slot; an OK or NONFINITE pair stores its sum (a NONFINITE pair's sum is the non-finite number itself,
never a NaN put in its place); the status byte of a failure that does not depend on the output mode (complex
eigenvalues, a NaN lag time, a solver failure, a step too coarse) is the same in predict and in log-likelihood mode.

One tiny population per walker: 3 subjects with 3 / 4 + 2 / 4 valued observations, the second subject over two
occasions; 8 and 9 support points (8: the status array is cleared eight bytes at a time and only failures are stored, on
the walkers that know that protocol; 9: every byte is stored), of which column FAIL alone fails.  Every launch asserts
the kernel that served it.  The expectation for the columns that do not fail is the CPU oracle on those columns alone at
the suite's bar for a log-likelihood (TOL_LL, tests/test_gpu_likelihood.py); the failing column's expectation is the
rule above.  The zero-volume cases observe only after a dose, so every prediction is +inf, every term -inf and the sum
-inf exactly.  Every case runs with a status array whose every byte is 0xFF before the launch (a walker that neither
clears nor stores a byte leaves it standing) and with a NULL one."""
import numpy as np
import pytest

import oracle
from pharmsol_amd import ODE, Data, Subject, _abi, runtime, synth
from tests.test_custom_models import SIG
from tests.test_gpu_likelihood import EM_ADD, TOL_LL
from tests.test_gpu_output_contract import (BOTH, COMPLEX2, COMPLEX3_ORAL, GRID, PAIR, WALKER, cov2_model, env,  # noqa: F401
                                            lag_model, m2, ode_lag, ode_rk4)
from tests.test_rk4_checked import KE, _builtin, _user_lag

pytestmark = pytest.mark.gpu

FAIL = 5  # the failing column, for 8 and for 9 support points
SIZES = (8, 9)
KEEPS_ITS_SUM = (_abi.PMX_PAIR_OK, _abi.PMX_PAIR_NONFINITE)
STATE = {"hip_error": None}
CACHE = {}


@pytest.fixture(autouse=True)
def _stop_after_a_hip_error():
    """A HIP error ends the module: nothing more is launched on a device that has faulted."""
    if STATE["hip_error"]:
        pytest.fail(f"not run: an earlier launch of this module ended in a HIP error ({STATE['hip_error']})")
    yield


def subjects(route=0, out=0, scale=1.0, covariates=()):
    """Doses first, every observation valued and after a dose; subject 1 has a second occasion."""
    subs = []
    for i, amount in enumerate((100.0, 60.0, 30.0)):
        def cov(b):
            for k, (name, v) in enumerate(covariates):
                b = b.covariate(name, 0.0, v + 4.0 * i).covariate(name, 6.0, v - 3.0 * i + k)
            return b

        b = cov(Subject.builder(f"f{i}").bolus(0.0, amount * scale, route))
        for k, t in enumerate((0.1, 0.5, 1.0, 4.0)[(1 if i == 0 else 0):]):
            b = b.observation(t, 0.4 + 0.3 * k + 0.2 * i, out)
        if i == 1:
            b = cov(b.reset().bolus(0.0, 50.0 * scale, route)).observation(0.5, 0.7, out).observation(1.0, 0.5, out)
        subs.append(b.build())
    return subs


def cached(key, make):
    if key not in CACHE:
        CACHE[key] = make()
    return CACHE[key]


def column(theta_of, **cols):
    """theta(P) with the given values in row FAIL."""

    def theta(P):
        th = np.ascontiguousarray(theta_of(P), dtype=np.float64).copy()
        for c, v in cols.items():
            th[FAIL, int(c[1:])] = v
        return th

    return theta


def theta_ka(ncol):
    def theta(P):  # rates the step-doubling probe passes with q <= 0.1 (tests/test_rk4_checked.py), 150 /h refused at q >= 10
        th = np.stack([np.array([0.5, 1.0, 2.0, 5.0])[np.arange(P) % 4], np.full(P, KE), np.full(P, 0.25)], axis=1)[:, :ncol].copy()
        th[FAIL, 0] = 150.0
        return th

    return theta


BOOM = f"""
PMX_DEVICE void pmx_dynamics({SIG}dx) {{ dx[0] = p[0] * x[0] * x[0]; }}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[0]; }}
"""


def boom_model():
    """x' = p x^2 (tests/test_custom_models.py): singular at t = 1 / (p x(0)); the controller runs out of step size."""
    oracle.compile_custom(BOOM)
    return ODE.custom(BOOM, nstates=1, nparams=1, h_max=1.0).with_solver("dopri5").with_tolerances(1e-6, 1e-6)


def theta_boom(P):  # doses 1 / 0.6 / 0.3 (0.5 in the second occasion): p = 8 is singular before every subject's second observation
    th = np.linspace(0.01, 0.1, P).reshape(P, 1).copy()
    th[FAIL, 0] = 8.0
    return th


def theta_oral_lag(ncol):
    def theta(P):  # ka, ke, v, lag(, fa): lags that land before, between and after the observations
        rng = np.random.default_rng(7)
        return np.stack([rng.uniform(1.0, 3.0, P), rng.uniform(0.05, 0.4, P), rng.uniform(10, 60, P),
                         rng.choice([0.0, 0.25, 0.75, 1.5, 3.0], size=P), rng.uniform(0.4, 1.0, P)], axis=1)[:, :ncol].copy()

    return theta


COMPLEX = {f"c{k}": v for k, v in COMPLEX2.items()}
COMPLEX_ORAL = {f"c{k}": v for k, v in COMPLEX3_ORAL.items()}
ROOTS, NONFINITE, BAD_LAG = _abi.PMX_PAIR_COMPLEX_ROOTS, _abi.PMX_PAIR_NONFINITE, _abi.PMX_PAIR_BAD_LAG
SOLVER_FAIL, TOO_COARSE = _abi.PMX_PAIR_SOLVER_FAIL, _abi.PMX_PAIR_STEP_TOO_COARSE
WT = (("wt", 70.0),)
WT_RENAL = (("wt", 70.0), ("renal", 90.0))

# name: (model, subjects, theta(P), switches, kernel, the failing column's status in predict mode)
CASES = {
    "grid:complex": (m2, subjects, column(synth.theta_c3, **COMPLEX), BOTH, "pmx_analytical_grid", ROOTS),
    "grid:zero-volume": (m2, subjects, column(synth.theta_c3, c3=0.0), BOTH, "pmx_analytical_grid", NONFINITE),
    "grid-lag:nan-lag": (lag_model, subjects, column(theta_oral_lag(5), c3=np.nan), WALKER, "pmx_analytical_grid<lag>", BAD_LAG),
    "grid-dyn:complex": (cov2_model, lambda: subjects("dose", "cp", covariates=WT), column(synth.theta_c3, **COMPLEX), WALKER,
                         "pmx_analytical_grid<dyn>", ROOTS),
    "pair:complex": (m2, subjects, column(synth.theta_c3, **COMPLEX), PAIR, "pmx_analytical_pair", ROOTS),
    "pair:zero-volume": (m2, subjects, column(synth.theta_c3, c3=0.0), PAIR, "pmx_analytical_pair", NONFINITE),
    "pair-lag:nan-lag": (lag_model, subjects, column(theta_oral_lag(5), c3=np.nan), PAIR, "pmx_analytical_pair<lag>", BAD_LAG),
    "pair-dyn:complex": (cov2_model, lambda: subjects("dose", "cp", covariates=WT), column(synth.theta_c3, **COMPLEX), PAIR,
                         "pmx_analytical_pair<dyn>", ROOTS),
    "steps:complex": (m2, subjects, column(synth.theta_c3, **COMPLEX), WALKER, "pmx_analytical_steps", ROOTS),
    "steps:zero-volume": (m2, subjects, column(synth.theta_c3, c3=0.0), WALKER, "pmx_analytical_steps", NONFINITE),
    "dyn3:complex": (synth.model_three_cpt_abs_wt, lambda: subjects("oral", "cp", covariates=WT),
                     column(synth.theta_c5, **COMPLEX_ORAL), GRID, "pmx_analytical_dyn3", ROOTS),
    "ode-grid:rk4": (ode_rk4, subjects, column(synth.theta_c3, c3=0.0), GRID, "pmx_ode_rk4_grid", NONFINITE),
    "ode-pair:rk4": (ode_rk4, subjects, column(synth.theta_c3, c3=0.0), PAIR, "pmx_ode_rk4_pair", NONFINITE),
    "ode-grid:rk4-lag": (ode_lag, subjects, column(theta_oral_lag(4), c3=np.nan), GRID, "pmx_ode_rk4_grid<lag>", BAD_LAG),
    "ode-pair:rk4-lag": (ode_lag, subjects, column(theta_oral_lag(4), c3=np.nan), PAIR, "pmx_ode_rk4_pair<lag>", BAD_LAG),
    "ode-grid:rk4-checked": (_builtin, subjects, theta_ka(2), GRID, "pmx_ode_rk4_checked_grid", TOO_COARSE),
    "ode-pair:rk4-checked": (_builtin, subjects, theta_ka(2), PAIR, "pmx_ode_rk4_checked_pair", TOO_COARSE),
    "ode-grid:dopri5": (boom_model, lambda: subjects(scale=0.01), theta_boom, GRID, "pmx_jit_ode_dopri5_grid", SOLVER_FAIL),
    "ode-pair:dopri5": (boom_model, lambda: subjects(scale=0.01), theta_boom, PAIR, "pmx_jit_ode_dopri5_pair", SOLVER_FAIL),
    "user-analytical-grid:nan-lag": (synth.model_user_covariates, lambda: subjects("oral", "cp", covariates=WT_RENAL),
                                     column(synth.theta_user, c3=np.nan), GRID, "pmx_jit_analytical_grid", BAD_LAG),
    "user-analytical-pair:nan-lag": (synth.model_user_covariates, lambda: subjects("oral", "cp", covariates=WT_RENAL),
                                     column(synth.theta_user, c3=np.nan), PAIR, "pmx_jit_analytical_pair", BAD_LAG),
    "user-ode-grid:rk4-checked": (_user_lag, subjects, theta_ka(3), GRID, "pmx_jit_ode_user_rk4_checked_grid", TOO_COARSE),
    "user-ode-pair:rk4-checked": (_user_lag, subjects, theta_ka(3), PAIR, "pmx_jit_ode_user_rk4_checked_pair", TOO_COARSE),
}


def prepared(name):
    """(model, flat, device population), one per (model, subjects) among the cases; the reference of the good columns."""
    model_of, subjects_of, theta_of, _, _, _ = CASES[name]
    model = cached(("model", model_of), model_of)
    flat = cached(("flat", model_of, subjects_of), lambda: model.flatten(Data(subjects_of())))
    return model, flat, theta_of


def reference(name, P):
    model, flat, theta_of = prepared(name)
    good = np.delete(theta_of(P), FAIL, axis=0)

    def compute():
        want, wst = oracle.loglik(model, flat, EM_ADD, good)
        assert (wst == _abi.PMX_PAIR_OK).all() and np.isfinite(want).all()
        want.setflags(write=False)
        return want

    return cached(("ll", CASES[name][0], CASES[name][1], good.tobytes()), compute)


def run(call, kernel, where):
    import torch

    try:
        out = call()
        torch.cuda.synchronize()
    except (_abi.PmxError, RuntimeError) as e:
        STATE["hip_error"] = str(e).splitlines()[0]
        raise
    assert runtime.last_kernel_name() == kernel, f"{where}: routed to {runtime.last_kernel_name()}, expected {kernel}"
    return [None if t is None else t.cpu().numpy() for t in out]


def poisoned_status(P):
    import torch

    return torch.full((3, P), 0xFF, dtype=torch.uint8, device="cuda")


def check_values(ll, fails, sum_kept, want, where):
    """`fails`: per subject, whether the pair of column FAIL stores NaN; `sum_kept`: its sum is the -inf of a zero volume."""
    print(f"{where}: column {FAIL} = {ll[:, FAIL].tolist()}")
    np.testing.assert_array_equal(np.isnan(ll[:, FAIL]), fails, err_msg=f"{where}: NaN exactly where the pair failed")
    if sum_kept:
        assert (ll[:, FAIL] == -np.inf).all(), f"{where}: a NONFINITE pair keeps its sum: {ll[:, FAIL]}"
    got = np.delete(ll, FAIL, axis=1)
    err = (np.abs(got - want) / np.maximum(np.abs(want), 1.0)).max()
    print(f"{where}: good columns off by {err:.3e}")
    assert np.isfinite(got).all() and err <= TOL_LL, f"{where}: log-likelihood off by {err:.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_failed_pair_in_loglik_mode(name, env):  # noqa: F811
    _, _, _, switches, kernel, fail_status = CASES[name]
    model, flat, theta_of = prepared(name)
    pop = cached(("pop", CASES[name][0], CASES[name][1]), lambda: runtime.DevicePopulation(flat, 0))
    assert flat.n_subjects == 3 and flat.n_observations == 13
    env(**switches)
    for P in SIZES:
        where = f"{name} P={P}"
        theta = theta_of(P)
        want = reference(name, P)
        _, pst = run(lambda: runtime.predict(model, pop, theta, status=poisoned_status(P)), kernel, where + " predict")
        assert (pst[:, FAIL] == fail_status).all() and (np.delete(pst, FAIL, axis=1) == _abi.PMX_PAIR_OK).all(), f"{where}: {pst}"
        ll, lst = run(lambda: runtime.loglik(model, pop, EM_ADD, theta, status=poisoned_status(P)), kernel, where + " loglik")
        mode_free = ~np.isin(pst, KEEPS_ITS_SUM)
        np.testing.assert_array_equal(lst[mode_free], pst[mode_free], err_msg=f"{where}: status byte, loglik against predict")
        np.testing.assert_array_equal(np.isnan(ll), ~np.isin(lst, KEEPS_ITS_SUM), err_msg=f"{where}: NaN exactly off OK / NONFINITE")
        assert (np.delete(lst, FAIL, axis=1) == _abi.PMX_PAIR_OK).all(), f"{where}: {lst}"
        sum_kept = fail_status == NONFINITE
        if sum_kept:
            assert (lst[:, FAIL] == NONFINITE).all(), f"{where}: {lst[:, FAIL]}"
        fails = ~np.isin(lst[:, FAIL], KEEPS_ITS_SUM)
        assert fails.all() != sum_kept
        check_values(ll, fails, sum_kept, want, where)
        ll0, none = run(lambda: runtime.loglik(model, pop, EM_ADD, theta, want_status=False), kernel, where + " loglik, NULL status")
        assert none is None
        check_values(ll0, fails, sum_kept, want, where + " NULL status")
