"""Every kind of log-likelihood term through every device fold site, against exact mathematics at its edges:
tests/golden/loglik_terms.json (mpmath, 40 digits; tests/golden/gen_loglik_terms.py).

Two rows of every subject sit on predictions that are exact by construction (f = 0 before the first dose, f = 12.5 at
the instant of a bolus of 100 into a volume of 8) and carry the hard terms: every rung of the BLOQ and ALOQ ladders, the
asymptotes, plain rows at |z| up to 400 and sigma from 1e-8 to 1e8, cubic error polynomials, missing rows, the four
residual models at f = 0 (where their floor engages) and f = 12.5, and the failing rows.  The rows behind them, after real
propagation, carry mild plain terms whose exact predictions are in the fixture as well.  One fixture serves every walker:
each route's model has the same central amount 100 exp(-ke (t - 1)) (tests/test_oracle_loglik_terms.py, KITS, where the
oracle is held to the same bars).

Bar on a subject's sum:  sum over rows (own bar + dterm_df delta_f) + n u sum |term|;  delta_f = 0 on the exact rows and
1e-10 max|f| on the others, never taken from the device.  `err` rungs and failing rows: the pair is PMX_PAIR_NONFINITE
with a NaN sum and every other subject of the launch is untouched.  `either` rungs: the pair is in the legal set, and the
side taken is printed (LLTERM-SIDE route rung side): a recorded difference between two erfc implementations.

The classed routes also run the 66-observation design (the mixed slot - plain, BLOQ, missing, ALOQ, plain with a cubic
of its own in members 0..4 - at observations 62, 63 and 64, across the end of the 63-bit plain masks).  The last chunk
of the `ok`, `model` and `long` populations is a partial one whose only live member holds censored rows (of `bad`:
plain rows, of `res`: residual rows).

Each launch asserts the kernel that served it.  LLTERM-WORST route err/bar rung is printed when the module ends."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from pharmsol_amd import _ffi, runtime
from tests.test_oracle_loglik_terms import DOC, KE, Population, print_sides, theta

pytestmark = pytest.mark.gpu

SWITCHES = ("PMX_DISABLE_LADDER", "PMX_DISABLE_CLASSING", "PMX_DISABLE_STEPS", "PMX_DISABLE_DYN3", "PMX_TUNE_LOOSE",
            "PMX_TUNE_LL_OLD")
WORST = {}    # route -> (err / bar, where)
SUMS = {}     # route -> {(population, model): (ll [S, lanes], status)} of the first len(KE) support points
RESIDUAL = tuple(DOC["populations"]["res"]["models"])
ASSAY_RUNS = (("ok", "add0"), ("bad", "add0"), ("model", "addl"), ("model", "prop"))
ALL_RUNS = ASSAY_RUNS + tuple(("res", m) for m in RESIDUAL)
CLASSED_RUNS = ALL_RUNS + (("long", "add0"),)

# route -> (model kit, developer switches, support points per launch, kernel, what runs)
ROUTES = {
    "classed_ll": ("one_cmt", {}, (64, 65), "pmx_analytical_classed_ll", CLASSED_RUNS),
    "classed<ll>": ("one_cmt", {"PMX_TUNE_LL_OLD": "1"}, (64, 65), "pmx_analytical_classed<ll>", CLASSED_RUNS),
    "classed<ll,loose>": ("one_cmt", {}, (64, 65), "pmx_analytical_classed<ll,loose>", ALL_RUNS),
    "classed<ll,lag>": ("lag", {}, (64, 65), "pmx_analytical_classed<ll,lag>", CLASSED_RUNS),
    "steps": ("one_cmt", {"PMX_DISABLE_CLASSING": "1"}, (64, 65), "pmx_analytical_steps", ALL_RUNS),
    "grid": ("one_cmt", {"PMX_DISABLE_CLASSING": "1", "PMX_DISABLE_STEPS": "1"}, (64, 65), "pmx_analytical_grid", ALL_RUNS),
    "pair": ("one_cmt", {}, (5,), "pmx_analytical_pair", ALL_RUNS),
    "pair(batch)": ("one_cmt", {}, ("batch",), "pmx_analytical_pair", ALL_RUNS),
    "dyn3": ("dyn3", {}, (64, 65), "pmx_analytical_dyn3", ALL_RUNS),
    "grid<dyn>": ("dyn3", {"PMX_DISABLE_DYN3": "1"}, (64, 65), "pmx_analytical_grid<dyn>", ALL_RUNS),
    "ode_rk4_grid": ("ode", {}, (64, 65), "pmx_ode_rk4_grid", ALL_RUNS),
    "ode_rk4_pair": ("ode", {}, (5,), "pmx_ode_rk4_pair", ALL_RUNS),
    "jit_analytical_grid": ("user_analytical", {}, (64, 65), "pmx_jit_analytical_grid", ALL_RUNS),
    "jit_ode_rk4_grid": ("user_ode", {}, (64, 65), "pmx_jit_ode_rk4_grid", ALL_RUNS),
}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for route, (r, where) in sorted(WORST.items()):
        print(f"LLTERM-WORST {route:22s} err/bar {r:.3e}  {where}")
    print_sides()


@contextlib.contextmanager
def switches(**kw):
    """Developer switches for one route, re-read by the library; restored (and re-read) afterwards."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(kw)
    _ffi.lib().pmx_debug_reload_env()
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
        _ffi.lib().pmx_debug_reload_env()


def launch(pop, kit, P, expect):
    """-> (ll [S, n], status [S, n], lane of column k of subject s).  P = "batch": subject s under theta row s."""
    import torch

    dpop = runtime.DevicePopulation(pop.flat, 0)
    S = len(pop.rows)
    if P == "batch":
        dm, dev = runtime._as_model(pop.model), torch.device("cuda", 0)
        th = torch.as_tensor(theta(S, kit), device=dev)
        ll = torch.empty((S,), dtype=torch.float64, device=dev)
        st = torch.zeros((S,), dtype=torch.uint8, device=dev)
        em = pop.em.to_c(pop.model)
        _ffi.check(_ffi.lib().pmx_loglik_batch_device(dm.handle, dpop.handle, C.cast(em, C.c_void_p), th.data_ptr(), ll.data_ptr(),
                                                      st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
        ll, st = ll.cpu().numpy().reshape(S, 1), st.cpu().numpy().reshape(S, 1)
        ll = np.where((st != 0) & np.isneginf(ll), np.nan, ll)  # the batch form scores a failed subject -inf
        lane = lambda s, k: s % len(KE)  # noqa: E731
    else:
        ll, st = runtime.loglik(pop.model, dpop, pop.em, theta(P, kit))
        torch.cuda.synchronize()
        ll, st = ll.cpu().numpy(), st.cpu().numpy()
        lane = lambda s, k: k % len(KE)  # noqa: E731
    name = runtime.last_kernel_name()
    assert name == expect, f"routed to {name}, expected {expect}"
    return ll, st, lane


_POPS = {}


def population(name, mdl, kit, loose):
    key = (name, mdl, kit, loose)
    if key not in _POPS:
        _POPS[key] = Population(name, mdl, loose=loose, kit=kit)
    return _POPS[key]


def run_route(route):
    """Every launch of one route, judged; the sums of the first len(KE) support points are kept for the comparison
    across routes.  Runs once per module, also where it fails: a route that went red is recorded as None and not
    launched a second time."""
    if route in SUMS:
        return SUMS[route]
    SUMS[route] = None
    kit, env, Ps, expect, runs = ROUTES[route]
    out = {}
    with switches(**env):
        for name, mdl in runs:
            pop = population(name, mdl, kit, loose="loose" in route)
            for P in Ps:
                ll, st, lane = launch(pop, kit, P, expect)
                for s in range(ll.shape[0]):
                    for k in range(ll.shape[1]):
                        pop.judge(s, lane(s, k), float(ll[s, k]), int(st[s, k]), route, WORST)
                if P != "batch":
                    out[(name, mdl)] = (ll[:, :len(KE)].copy(), st[:, :len(KE)].copy())
    SUMS[route] = out
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_route(route):
    run_route(route)


def test_routes_agree_on_ok_rows():
    """The sums of two routes over the same subjects agree within the sum of their bars (nothing tighter: the fold order
    differs).  Routes whose walker integrates across the gap at the bolus see another prediction there: they are
    compared among themselves.  A route that failed its own test is left out: it is not launched again."""
    groups = (("classed_ll", "classed<ll>", "steps", "grid", "pair", "dyn3", "grid<dyn>", "jit_analytical_grid",
               "classed<ll,lag>"), ("ode_rk4_grid", "ode_rk4_pair", "jit_ode_rk4_grid"))
    for group in groups:
        sums = {r: run_route(r) for r in group}
        group = [r for r in group if sums[r] is not None]  # (a route that went red in its own test is not compared)
        if len(group) < 2:
            continue
        first = group[0]
        for name, mdl in ALL_RUNS:
            pop = population(name, mdl, ROUTES[first][0], False)
            a_ll, a_st = sums[first][(name, mdl)]
            for other in group[1:]:
                b_ll, b_st = sums[other][(name, mdl)]
                for s in range(a_ll.shape[0]):
                    if pop.special(s):
                        continue
                    for k in range(len(KE)):
                        _, bar = pop.expected(s, k)
                        assert abs(a_ll[s, k] - b_ll[s, k]) <= 2 * bar, (first, other, name, mdl, s, k, a_ll[s, k], b_ll[s, k])
