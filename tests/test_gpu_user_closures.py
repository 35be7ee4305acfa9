"""The closure walkers (pmx_analytical.hpp, pmx_ode_user.hpp, pmx_userlag.hpp) against an independent 40-digit event
march: tests/golden/user_closures.json (tests/golden/gen_user_closures.py) through the GRID, PAIR and batched PAIR
mappings of the hiprtc-compiled models, and through the fused log-likelihood.

Bar for every prediction:  |gpu - fixture| / max|fixture| <= max(bar(case), 8 err_oracle), per case, bar = the analytical
fixtures' max(1e-10, 64 u kappa) or the ODE fixtures' 64 u kappa (tests/test_oracle_user_closures.bar) - measured
against the fixture, never against the oracle's output; the oracle's own error only enters through the factor 8, and only
after the oracle itself has met the bar.  The status of every (subject, support point) equals the fixture's; the rows of
a pair with a non-zero status must all be NaN and are exempt from accuracy.

A launch mixes the group's cases over the support points - the easy one first, so that lanes of one wave see different
landing orders - and 9 copies of the group's subject, with every dose scaled where the truth is linear in the doses
(`scalable`; groups with an initial amount, an affine propagator or a non-linear bolus term get plain copies).  GRID at
P = 65 and 257, PAIR in chunks of at most 7 support points each led by the easy case, batched PAIR with a subject per
case; every launch asserts the kernel that served it.  The groups with more than 64 boluses in an occasion also assert
that the model's big-lists build exists after the launch without a further request to the compiler; the 64-bolus
subject, launched alone on a model of its own, must leave that build unmade.

PMX_TUNE_STEPS_PER_TRIP: the closure walker of the ODE back-end does not read it (its PAIR mapping walks a piece in one
go, pmx_ode_user.hpp uode_pair_body; the trip state machine is pmx_ode.hpp's), so there are no per-trip launches here."""
import math

import numpy as np
import pytest

from pharmsol_amd import Data, _abi, _ffi, runtime
from tests import user_closure_models
from tests.test_gpu_edge_accuracy import EM, expected_loglik
from tests.test_oracle_user_closures import GROUPS, NAMES, bar, build_model, build_subject, is_ode, oracle_errors, status_of

pytestmark = pytest.mark.gpu

SCALES = (1.0, 2.0, 0.5, 3.0, 0.25, 1.5, 4.0, 0.75, 5.0)  # 9 copies: one whole chunk of 8 and a partial one
GRID_P = (65, 257)  # a partial second wave; a second tile with one live lane
PAIR_CHUNK = 7      # support points per PAIR launch: below every GRID crossover
WORST = {}          # walker -> (err / bar, err, where)
LL_GROUPS = [NAMES.index("an_a_overtake"), NAMES.index("ode_a_overtake_routes")]
BIG = [g for g in range(len(GROUPS)) if max(sum(e[0] == "bolus" for e in o["events"]) for o in GROUPS[g]["occasions"]) > 64]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for w, (r, err, where) in sorted(WORST.items()):
        print(f"USER-CLOSURE-WORST {w:44s} err/bar {r:.3e}  err {err:.3e}  {where}")


def note(walker, err, b, where):
    r = err / b if np.isfinite(err) else math.inf
    if r > WORST.get(walker, (-1.0,))[0]:
        WORST[walker] = (r, err, where)


def kernel_name(group, pair):
    stem = "pmx_jit_ode_user_rk4_" if is_ode(group) else "pmx_jit_analytical_"
    return stem + ("pair" if pair else "grid")


def cycle(group, n):
    """Support point k -> case k mod n_cases (n >= n_cases reaches every case)."""
    return np.arange(n) % len(group["cases"])


def pair_chunks(group):
    """Every case in PAIR launches of at most PAIR_CHUNK support points, each launch led by the easy case 0."""
    hard = list(range(1, len(group["cases"])))
    step = PAIR_CHUNK - 1
    return [np.array([0] + hard[i:i + step]) for i in range(0, max(len(hard), 1), step)]


def bars_of(g):
    """(bar per case, status per case): the oracle must itself meet the fixture before its error may widen a bar."""
    group = GROUPS[g]
    errs_o, status_o, _ = oracle_errors(g)
    out = []
    for c, case in enumerate(group["cases"]):
        assert status_o[c] == status_of(case)
        assert errs_o[c] <= bar(case), f"{group['name']}[{c}]: the oracle itself misses the fixture ({errs_o[c]:.3e} > {bar(case):.3e})"
        out.append(bar(case, errs_o[c]))
    return out, [status_of(c) for c in group["cases"]]


_POP = {}


def population(g, n_copies=len(SCALES)):
    """(model, flat population, dose scale per subject, truth [n_obs, n_cases]) - built once per (group, size)."""
    if (g, n_copies) not in _POP:
        group = GROUPS[g]
        m = build_model(group)
        scales = [SCALES[i % len(SCALES)] if group["scalable"] else 1.0 for i in range(n_copies)]
        flat = m.flatten(Data([build_subject(group, s, name=f"c{i}") for i, s in enumerate(scales)]))
        n_obs = sum(e[0] == "obs" for o in group["occasions"] for e in o["events"])
        truth = np.array([c["expected"] if c["expected"] is not None else [np.nan] * n_obs for c in group["cases"]]).T
        _POP[(g, n_copies)] = (m, flat, scales, truth)
    return _POP[(g, n_copies)]


def check(g, idx, expect, batch=False, walker=None):
    """One launch; idx[k] = the case of support point k (of subject k in a batch)."""
    import torch

    group = GROUPS[g]
    cases = group["cases"]
    bars, wstatus = bars_of(g)
    m, flat, scales, truth = population(g, len(idx) if batch else len(SCALES))
    theta = np.array([cases[i]["theta"] for i in idx])
    pop = runtime.DevicePopulation(flat, 0)
    pred, status = runtime.predict(m, pop, np.ascontiguousarray(theta), batch=batch)
    torch.cuda.synchronize()
    name = runtime.last_kernel_name()
    assert name == expect, f"routed to {name}, expected {expect}"
    pred = pred.cpu().numpy().reshape(flat.n_observations, -1)
    status = status.cpu().numpy().reshape(flat.n_subjects, -1)
    n_obs = truth.shape[0]
    walker = walker or expect
    for s, scale in enumerate(scales):
        rows = pred[s * n_obs:(s + 1) * n_obs]
        for k in ([s] if batch else range(len(idx))):
            c, col = idx[k], (0 if batch else k)
            where = f"{group['name']}[{c}] subject {s} P={len(idx)}"
            assert status[s, col] == wstatus[c], f"{walker}: {where}: status {status[s, col]}, fixture {wstatus[c]}"
            got = rows[:, col]
            if wstatus[c]:
                assert np.isnan(got).all(), f"{walker}: {where}: {got}"
                continue
            want = truth[:, c] * scale
            err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
            note(walker, err, bars[c], where)
            assert err <= bars[c], (f"{walker}: {where}: err {err:.3e} > bar {bars[c]:.3e} (kappa {cases[c]['kappa']:.3g}); "
                                    f"gpu {got} fixture {want}")


def jit_requests():
    s = runtime.jit_cache_stats()
    return s["compiles"] + s["mem_hits"] + s["disk_hits"]


def big_build_requests(model):
    """How many requests to the compiler (served or cached) asking for the model's big-lists build costs now: 0 when the
    model already keeps that build."""
    before = jit_requests()
    _ffi.check(_ffi.lib().pmx_debug_jit_compile_big_lists(runtime._as_model(model).handle))
    return jit_requests() - before


@pytest.mark.parametrize("g", range(len(GROUPS)), ids=NAMES)
def test_every_mapping(g):
    group = GROUPS[g]
    for P in GRID_P:
        check(g, cycle(group, P), kernel_name(group, False))
    if g in BIG:  # the launch above was served by the build with the scan path in: the model keeps it
        assert big_build_requests(build_model(group)) == 0
    for idx in pair_chunks(group):
        check(g, idx, kernel_name(group, True))
    n = max(len(SCALES), len(group["cases"]))  # a subject for every case
    check(g, cycle(group, n), kernel_name(group, True), batch=True, walker=kernel_name(group, True) + "(batch)")


def test_64_boluses_are_served_by_the_ordinary_build():
    """kUserLagKept = 64 boluses of one occasion fit a lane's sorted list: a model that has only ever met the 64-bolus
    subject has not made its big-lists build."""
    import torch

    g = NAMES.index("an_i_big_64")
    group = GROUPS[g]
    bars, _ = bars_of(g)
    m = user_closure_models.build(group["model"])  # a model of its own: the module's shared one meets 65 and 90 too
    flat = m.flatten(build_subject(group))
    theta = np.array([c["theta"] for c in group["cases"]])
    for th, expect in ((np.tile(theta, (13, 1)), kernel_name(group, False)), (theta, kernel_name(group, True))):
        pred, status = runtime.predict(m, runtime.DevicePopulation(flat, 0), np.ascontiguousarray(th))
        torch.cuda.synchronize()
        assert runtime.last_kernel_name() == expect
        pred = pred.cpu().numpy().reshape(flat.n_observations, -1)
        assert (status.cpu().numpy() == 0).all()
        for k in range(len(th)):
            c = k % len(theta)
            want = np.array(group["cases"][c]["expected"])
            err = float(np.max(np.abs(pred[:, k] - want))) / float(np.max(np.abs(want)))
            note(expect + " (64 alone)", err, bars[c], f"{group['name']}[{c}]")
            assert err <= bars[c], f"{group['name']}[{c}]: err {err:.3e} > bar {bars[c]:.3e}"
    assert big_build_requests(m) == 1


@pytest.mark.parametrize("g", LL_GROUPS, ids=[NAMES[g] for g in LL_GROUPS])
def test_fused_loglik(g):
    """The same walkers with the log-likelihood fused in: expected value and tolerance as in
    tests/test_gpu_edge_accuracy.check_ll (the prediction bar carried through the slope of the likelihood)."""
    import torch

    group = GROUPS[g]
    cases = group["cases"]
    bars, wstatus = bars_of(g)
    m, _, scales, truth = population(g)
    n_obs = truth.shape[0]
    rng = np.random.default_rng(5)
    y = [np.abs(truth[:, 0] * s) * np.exp(rng.normal(0, 0.2, n_obs)) + 0.05 for s in scales]
    flat = m.flatten(Data([build_subject(group, s, name=f"c{i}") for i, s in enumerate(scales)]))
    flat.ev_value = flat.ev_value.copy()
    flat.ev_value[flat.ev_kind == _abi.PMX_EV_OBSERVATION] = np.concatenate(y)
    launches = [(cycle(group, GRID_P[0]), kernel_name(group, False))] + [(idx, kernel_name(group, True)) for idx in pair_chunks(group)]
    for idx, expect in launches:
        theta = np.array([cases[i]["theta"] for i in idx])
        ll, st = runtime.loglik(m, runtime.DevicePopulation(flat, 0), EM, np.ascontiguousarray(theta))
        torch.cuda.synchronize()
        assert runtime.last_kernel_name() == expect, runtime.last_kernel_name()
        ll, st = ll.cpu().numpy(), st.cpu().numpy()
        for s, scale in enumerate(scales):
            for k, c in enumerate(idx):
                assert st[s, k] == wstatus[c] == 0
                want, slope = expected_loglik(y[s], truth[:, c] * scale)
                tol = slope * bars[c] * float(np.max(np.abs(truth[:, c] * scale))) + 1e-13 * (abs(want) + n_obs)
                note(expect + " (loglik)", abs(ll[s, k] - want), tol, f"{group['name']}[{c}]")
                assert abs(ll[s, k] - want) <= tol, f"{expect}: {group['name']}[{c}] subject {s}: {ll[s, k]!r} vs {want!r}"
