"""Every analytical walker against exact propagation at hard rates: tests/golden/edge_math.json (mpmath, 40 digits;
tests/golden/gen_edge.py) through each device walker that can serve the case, with the ladder on and off.

Bar for every prediction:  |gpu - truth| / max|truth| <= max(1e-10, 64 u kappa, 8 err_oracle), per case, the same for
every walker; the status of every (subject, support point) equals the oracle's.  A launch mixes several support points
(the group's cases, the first of them an easy one) and several subjects (copies of the case's subject with every dose
scaled: the truth scales with it), so a bad lane cannot hide behind a good one.  Every case of a group reaches every
walker that serves the group: the GRID launches cycle through the cases (P >= the number of cases), the PAIR launches
take them in chunks of at most 7 support points (below the GRID crossover) that each carry the easy case too, and the
batched PAIR launch gives every case a subject of its own.  Each launch asserts the kernel that served it, so a
routing change cannot turn a check into a no-op.

Cases whose kappa is near 1/u (ka set to an eigenvalue rounded to double, in the two- and three-compartment oral
models) have a bar above 1: for them the check is the status and the finiteness, not the accuracy."""
import math

import numpy as np
import pytest

from pharmsol_amd import AssayErrorModel, AssayErrorModels, Data, ErrorPoly, _abi, _ffi, runtime
from tests.test_oracle_edge_math import GROUPS, bar, build_model, build_subject, oracle_errors

pytestmark = pytest.mark.gpu

SCALES = (1.0, 2.0, 0.5, 3.0, 0.25, 1.5, 4.0, 0.75, 5.0)  # 9 copies: one whole chunk of 8 and a partial one
SWITCHES = ("PMX_DISABLE_LADDER", "PMX_DISABLE_CLASSING", "PMX_DISABLE_STEPS", "PMX_DISABLE_DYN3", "PMX_TUNE_LOOSE",
            "PMX_TUNE_PROP_SLOTS")
WORST = {}  # walker -> (err / bar, kappa, case): printed when the module ends (pytest -s)
PAIR_CHUNK = 7  # support points per PAIR launch: below the GRID crossover (8 when classes serve most subjects)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for w, (r, kap, where) in sorted(WORST.items()):
        print(f"EDGE-WORST {w:44s} err/bar {r:.3e}  kappa {kap:.3g}  {where}")


def note(walker, ratio, case, where):
    if ratio > WORST.get(walker, (-1.0,))[0]:
        WORST[walker] = (ratio, case["kappa"], where)


def cycle(group, P):
    """Support point k -> case k mod n (a GRID launch: P >= n reaches every case)."""
    return np.arange(P) % len(group["cases"])


def pair_chunks(group):
    """Every case in PAIR launches of at most PAIR_CHUNK support points, each launch led by the easy case 0."""
    hard = list(range(1, len(group["cases"])))
    step = PAIR_CHUNK - 1
    return [np.array([0] + hard[i:i + step]) for i in range(0, max(len(hard), 1), step)]


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


def group_population(group, variants=False, n_copies=len(SCALES)):
    """(model, flat population, truth [n_obs, n_cases] per subject): `n_copies` dose-scaled copies of the case subject,
    or one subject per stretched variant (same program shape, other step lengths: loose classes)."""
    m = build_model(group)
    base = np.array([c["expected"] for c in group["cases"]]).T
    subs, truth = [], []
    if variants:
        schedules = [(group["events"], base)] + [(v["events"], np.array(v["expected"]).T) for v in group["variants"]]
        for i, (ev, want) in enumerate(schedules):
            s = SCALES[i % len(SCALES)]
            subs.append(build_subject(group, ev, s, name=f"v{i}"))
            truth.append(want * s)
    else:
        for i in range(n_copies):
            s = SCALES[i % len(SCALES)]
            subs.append(build_subject(group, None, s, name=f"c{i}"))
            truth.append(base * s)
    return m, m.flatten(Data(subs)), truth


def check(group, m, flat, truth, idx, expect, batch=False, walker=None):
    """One launch; idx[k] = the case of support point k (of subject k in a batch)."""
    import torch

    g = GROUPS.index(group)
    cases = group["cases"]
    errs_o, status_o = oracle_errors(g)
    S = len(truth)
    P = len(idx)
    if batch:
        assert P == S
    theta = np.array([cases[i]["theta"] for i in idx])
    pop = runtime.DevicePopulation(flat, 0)
    pred, status = runtime.predict(m, pop, theta, batch=batch)
    torch.cuda.synchronize()
    name = runtime.last_kernel_name()
    assert name == expect, f"routed to {name}, expected {expect}"
    pred, status = pred.cpu().numpy().reshape(flat.n_observations, -1), status.cpu().numpy()
    n_obs = truth[0].shape[0]
    walker = walker or expect
    for s in range(S):
        rows = pred[s * n_obs:(s + 1) * n_obs]
        cols = [s] if batch else range(P)
        for k in cols:
            c = idx[k]
            st = status.reshape(S, -1)[s, 0] if batch else status[s, k]
            assert st == status_o[c], f"{group['name']}[{c}] subject {s}: status {st}, oracle {status_o[c]}"
            if status_o[c]:
                continue
            got = rows[:, 0] if batch else rows[:, k]
            want = truth[s][:, c]
            err = float(np.max(np.abs(got - want))) / max(float(np.max(np.abs(want))), 1e-300)
            b = bar(cases[c], errs_o[c])
            note(walker, err / b if np.isfinite(err) else math.inf, cases[c], f"{group['name']}[{c}]")
            assert err <= b, (f"{walker}: {group['name']}[{c}] subject {s} P={P}: err {err:.3e} > bar {b:.3e} "
                              f"(kappa {cases[c]['kappa']:.3g}, oracle {errs_o[c]:.3e})")


def kind(group):
    mdl = group["model"]
    if mdl.get("cov"):
        return "cov"
    if mdl.get("lag"):
        return "lag"
    return "plain"


def ids(groups):
    return [g["name"] for g in groups]


PLAIN = [g for g in GROUPS if kind(g) == "plain"]
LAG = [g for g in GROUPS if kind(g) == "lag"]
COV = [g for g in GROUPS if kind(g) == "cov"]
LOOSE = [g for g in PLAIN if len(g["variants"]) >= 2]


@pytest.mark.parametrize("ladder", ["on", "off"])
@pytest.mark.parametrize("group", PLAIN, ids=ids(PLAIN))
def test_plain_walkers(group, ladder, env):
    lad = {} if ladder == "on" else {"PMX_DISABLE_LADDER": "1"}
    m, flat, truth = group_population(group)
    env(**lad)
    for P in (8, 65):
        check(group, m, flat, truth, cycle(group, P), "pmx_analytical_classed")
    for idx in pair_chunks(group):
        check(group, m, flat, truth, idx, "pmx_analytical_pair")
    n = max(len(SCALES), len(group["cases"]))  # a subject for every case
    mb, flatb, truthb = group_population(group, n_copies=n)
    check(group, mb, flatb, truthb, cycle(group, n), "pmx_analytical_pair", batch=True, walker="pmx_analytical_pair(batch)")
    env(PMX_DISABLE_CLASSING="1", **lad)
    for P in (63, 64, 257):
        check(group, m, flat, truth, cycle(group, P), "pmx_analytical_steps")
    env(PMX_DISABLE_CLASSING="1", PMX_DISABLE_STEPS="1", **lad)
    check(group, m, flat, truth, cycle(group, 64), "pmx_analytical_grid")


@pytest.mark.parametrize("group", LOOSE, ids=ids(LOOSE))
def test_loose_classes(group, env):
    m, flat, truth = group_population(group, variants=True)
    env()
    for P in (64, 65):
        check(group, m, flat, truth, cycle(group, P), "pmx_analytical_classed<loose>")


@pytest.mark.parametrize("group", LAG, ids=ids(LAG))
def test_lag_walkers(group, env):
    # (no ladder run: the host never builds the exponential ladder for a model with a lagged input, pmx_launch.cpp key_for)
    m, flat, truth = group_population(group)
    env()
    check(group, m, flat, truth, cycle(group, 64), "pmx_analytical_classed<lag>")
    for idx in pair_chunks(group):
        check(group, m, flat, truth, idx, "pmx_analytical_pair<lag>")
    env(PMX_DISABLE_CLASSING="1")
    check(group, m, flat, truth, cycle(group, 65), "pmx_analytical_grid<lag>")


def cov_routes(group):
    kernel = group["model"]["kernel"]
    infusion = any(e[0] == "inf" for e in group["events"])
    if kernel.startswith("three"):
        return "pmx_analytical_grid<dyn>" if infusion else "pmx_analytical_dyn3"
    return "pmx_analytical_classed<dyn>"


def keeps_eigenvalues(m, flat, env):
    """The host's choice between the two dyn3 instantiations, read from the op stream it compiles: the walker keeps the
    eigenvalues across segments (EIGR) when some segment repeats the rate constants of the one built before it (bit 27
    of a PROP, pmx_compile.cpp), with the two kept-segment slots a population without infusions gets."""
    env(PMX_TUNE_PROP_SLOTS="2")
    ops = runtime.compile_ops(m, flat)
    env()
    return bool(np.any((ops["kind"] == _abi.PMX_OP_PROP) & ((ops["flags"] & 8) != 0)))


@pytest.mark.parametrize("group", COV, ids=ids(COV))
def test_covariate_walkers(group, env):
    m, flat, truth = group_population(group)
    route = walker = cov_routes(group)
    if route == "pmx_analytical_dyn3":
        # a subject-constant covariate repeats the rate constants in every segment; a covariate read at the segment's
        # end (interpolated) never repeats them here: both instantiations run
        cov = group["model"]["cov"]
        eigr = keeps_eigenvalues(m, flat, env)
        if len(cov["knots"][0]) == 1:
            assert eigr
        if cov["mode"] == "segment_end_abs" and len(cov["knots"][0]) > 1:
            assert not eigr
        walker = route + ("<eigr>" if eigr else "")
    env()
    for P in (63, 64, 257):
        check(group, m, flat, truth, cycle(group, P), route, walker=walker)
    for idx in pair_chunks(group):
        check(group, m, flat, truth, idx, "pmx_analytical_pair<dyn>")
    if route == "pmx_analytical_dyn3":
        env(PMX_DISABLE_DYN3="1")
        check(group, m, flat, truth, cycle(group, 64), "pmx_analytical_grid<dyn>")
    if route == "pmx_analytical_classed<dyn>":
        env(PMX_DISABLE_CLASSING="1")
        check(group, m, flat, truth, cycle(group, 64), "pmx_analytical_grid<dyn>")
    if group["variants"]:
        m, flat, truth = group_population(group, variants=True)
        env()
        check(group, m, flat, truth, cycle(group, 64), route, walker=walker)


# ------------------------------------------------------------------------------------------- fused log-likelihood
EM = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.05, 0.1, 0.0, 0.0), 0.1))


def expected_loglik(y, f):
    """Gaussian log-likelihood of observations y under predictions f, sigma from the observation (additive assay model:
    sigma = sqrt((c0 + c1 y)^2 + lambda^2)); returns (ll, d ll / d f summed in absolute value)."""
    sig = np.sqrt((0.05 + 0.1 * y) ** 2 + 0.1 ** 2)
    r = (y - f) / sig
    return float(np.sum(-0.5 * math.log(2 * math.pi) - np.log(sig) - 0.5 * r * r)), float(np.sum(np.abs(r / sig)))


def check_ll(group, m, flat, truth, idx, expect):
    import torch

    g = GROUPS.index(group)
    cases = group["cases"]
    errs_o, status_o = oracle_errors(g)
    n_obs = truth[0].shape[0]
    rng = np.random.default_rng(5)
    y = []
    for s in range(len(truth)):
        y.append(np.abs(truth[s][:, 0]) * np.exp(rng.normal(0, 0.2, n_obs)) + 0.05)
    flat.ev_value = flat.ev_value.copy()
    flat.ev_value[flat.ev_kind == _abi.PMX_EV_OBSERVATION] = np.concatenate(y)
    P = len(idx)
    theta = np.array([cases[i]["theta"] for i in idx])
    pop = runtime.DevicePopulation(flat, 0)
    ll, st = runtime.loglik(m, pop, EM, theta)
    torch.cuda.synchronize()
    assert runtime.last_kernel_name() == expect, runtime.last_kernel_name()
    ll, st = ll.cpu().numpy(), st.cpu().numpy()
    for s in range(len(truth)):
        for k in range(P):
            c = idx[k]
            assert st[s, k] == status_o[c]
            if status_o[c]:
                continue
            want, slope = expected_loglik(y[s], truth[s][:, c])
            tol = slope * bar(cases[c], errs_o[c]) * float(np.max(np.abs(truth[s][:, c]))) + 1e-13 * (abs(want) + n_obs)
            note(expect + " (loglik)", abs(ll[s, k] - want) / tol, cases[c], f"{group['name']}[{c}]")
            assert abs(ll[s, k] - want) <= tol, f"{expect}: {group['name']}[{c}] subject {s}: {ll[s, k]!r} vs {want!r}"


LL_PLAIN = [g for g in PLAIN if g["name"].startswith(("a_", "c_ladder_doubling", "e_three"))]
LL_DYN3 = [g for g in COV if cov_routes(g) == "pmx_analytical_dyn3"]


@pytest.mark.parametrize("group", LL_PLAIN, ids=ids(LL_PLAIN))
def test_loglik_plain(group, env):
    m, flat, truth = group_population(group)
    env()
    check_ll(group, m, flat, truth, cycle(group, 64), "pmx_analytical_classed_ll")
    for idx in pair_chunks(group):
        check_ll(group, m, flat, truth, idx, "pmx_analytical_pair")
    env(PMX_DISABLE_CLASSING="1")
    check_ll(group, m, flat, truth, cycle(group, 65), "pmx_analytical_steps")


@pytest.mark.parametrize("group", LL_DYN3, ids=ids(LL_DYN3))
def test_loglik_dyn3(group, env):
    m, flat, truth = group_population(group)
    env()
    check_ll(group, m, flat, truth, cycle(group, 64), "pmx_analytical_dyn3")
