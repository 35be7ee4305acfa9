"""PMX_SOLVER_RK4_CHECKED (``ODE.with_solver("rk4-checked")``): fixed-step RK4 that refuses to lie.  At the first step of
every integration piece the step is also taken as two half steps; Richardson's estimate of its local error, in the
adaptive solvers' scaled norm, must be <= 1 or the pair ends as PMX_PAIR_STEP_TOO_COARSE with NaN rows from that piece on.

The expectation is a plain numpy restatement of the probe and of the RK4 march (independent of the oracle's twin of the
rule, which tests/test_oracle_ode_exact.py holds to exact arithmetic).  Only cases whose numpy q is <= 0.1 or >= 10 on every deciding piece are used, so an FMA
contraction on the device cannot flip a verdict; the band 15 <= ka <= 25, where q crosses 1, is left out.

Tolerances: a lane whose probes pass keeps the full step, i.e. it walks what plain RK4 walks - 1e-12 relative between the
two device instantiations (not bitwise: they may contract FMAs differently); against the numpy march 1e-10 (a few hundred
steps, each a handful of roundings of 1.1e-16); against the closed form the 1e-4 the probe's tolerances promise."""
import ctypes as C
import math

import numpy as np
import pytest

from pharmsol_amd import ODE, AssayErrorModel, AssayErrorModels, Data, ErrorPoly, Ratio, Subject, _abi, _ffi, runtime

KE, H_MAX, RTOL, ATOL = 0.1, 0.02, 1e-4, 1e-4
KA_PASS = [0.5, 1.0, 2.0, 5.0, 10.0]
KA_FAIL = [30.0, 40.0, 60.0, 100.0, 130.0, 150.0, 300.0]
OBS_T = [0.1, 0.5, 1.0, 4.0]
AMOUNTS = [100.0, 60.0, 30.0]  # three subjects: the fixture's timeline at three doses (atol makes q depend on the dose: above 100, ka = 10 leaves q <= 0.1)


# ------------------------------------------------------------------------------------- the rule, restated in numpy
def _rhs(ka, ke, x):
    return np.array([-ka * x[0], ka * x[0] - ke * x[1]])


def _rk4(ka, ke, x, h):
    k1 = _rhs(ka, ke, x)
    k2 = _rhs(ka, ke, x + 0.5 * h * k1)
    k3 = _rhs(ka, ke, x + 0.5 * h * k2)
    k4 = _rhs(ka, ke, x + h * k3)
    return x + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def _probe(ka, ke, x, h):
    """(xa, q) of the first step of a piece."""
    xa = _rk4(ka, ke, x, h)
    xb = _rk4(ka, ke, _rk4(ka, ke, x, 0.5 * h), 0.5 * h)
    e = (16.0 / 15.0) * (xb - xa)
    with np.errstate(all="ignore"):
        q = math.sqrt(np.mean((e / (ATOL + RTOL * np.maximum(np.abs(xa), np.abs(xb)))) ** 2))
    return xa, q


def march(ka, ke, events, checked=True):
    """events: time-sorted (t, "obs" | "bolus", amount), lag already applied.  Returns (rows, status, [q of every piece
    up to and including the first failing one]).  The walk starts at the first event's time."""
    x = np.zeros(2)
    t = events[0][0]
    rows, qs, coarse = [], [], False
    for (te, kind, amt) in events:
        dt = te - t
        if dt > 0.0:
            n = max(1, math.ceil(dt / H_MAX))
            h = dt / n
            xa, q = _probe(ka, ke, x, h)
            if checked and not coarse:
                qs.append(q)
                coarse = not (q <= 1.0)
            x = xa
            with np.errstate(all="ignore"):
                for _ in range(1, n):
                    x = _rk4(ka, ke, x, h)
            t = te
        if kind == "bolus":
            x = x + np.array([amt, 0.0])
        else:
            rows.append(float("nan") if (checked and coarse) else x[1])
    return np.array(rows), (_abi.PMX_PAIR_STEP_TOO_COARSE if (checked and coarse) else 0), qs


def closed_form(ka, ke, amount, t):
    return amount * ka / (ka - ke) * (math.exp(-ke * t) - math.exp(-ka * t))


def _events(amount, t_bolus=0.0, obs=OBS_T):
    ev = [(t_bolus, "bolus", amount)] + [(t, "obs", 0.0) for t in obs]
    return sorted(ev, key=lambda e: (e[0], 0 if e[1] == "obs" else 1))  # Observation < Bolus at equal times


def _decisive(qs):
    return all(q <= 0.1 or q >= 10.0 for q in qs)


def test_numpy_rule_reproduces_the_recorded_probe_values():
    """h_max = 0.02, rtol = atol = 1e-4, ke = 0.1, bolus of 100, observations at 0.1 / 0.5 / 1 / 4 h."""
    ev = _events(100.0)
    for ka in KA_PASS:
        rows, st, qs = march(ka, KE, ev)
        assert st == 0 and len(qs) == 4 and max(qs) <= 0.0996, (ka, qs)
        want = np.array([closed_form(ka, KE, 100.0, t) for t in OBS_T])
        assert (np.abs(rows - want) / want).max() <= 9.4e-6
    assert abs(max(march(15.0, KE, ev)[2]) - 0.546) < 1e-3
    assert abs(march(20.0, KE, ev)[2][0] - 1.89) < 1e-2
    for ka in KA_FAIL:
        rows, st, qs = march(ka, KE, ev)
        assert st == 5 and len(qs) == 1 and qs[0] >= 11.89 and np.isnan(rows).all(), (ka, qs)
    # what the probe protects from: plain RK4 at ka = 150 is finite nonsense
    plain, st, _ = march(150.0, KE, ev, checked=False)
    assert st == 0 and np.isfinite(plain).all() and np.abs(plain).max() > 1e20


# ------------------------------------------------------------------------------------- host path (no GPU)
def _builtin(solver="rk4-checked", lag=None, nparams=2):
    return (ODE.new("one_cmt_oral", {0: Ratio(1)}, nparams=nparams, lag=lag, h_max=H_MAX).with_nstates(2).with_ndrugs(1)
            .with_nout(1).with_solver(solver))


def test_enum_values_and_descriptor():
    assert _abi.PMX_PAIR_STEP_TOO_COARSE == 5 and _abi.PMX_SOLVER_RK4_CHECKED == 3
    d = _builtin().desc()
    assert d.ode_solver == 3 and d.ode_rtol == 1e-4 and d.ode_atol == 1e-4  # the tolerances keep their defaults
    assert _builtin().with_tolerances(1e-6, 1e-8).desc().ode_atol == 1e-8
    assert _builtin("rk4").desc().ode_solver == 0


def test_model_create_accepts_the_solver_and_wants_tolerances():
    L = _ffi.lib()
    d = _builtin().desc()
    h = C.c_void_p()
    assert L.pmx_model_create(C.byref(d), C.byref(h)) == _abi.PMX_OK
    L.pmx_model_destroy(h)
    for field in ("ode_rtol", "ode_atol"):
        bad = _builtin().desc()
        setattr(bad, field, 0.0)
        assert L.pmx_model_create(C.byref(bad), C.byref(h)) == _abi.PMX_ERR_INVALID_ARGUMENT
    bad = _builtin().desc()
    bad.ode_solver = 4
    assert L.pmx_model_create(C.byref(bad), C.byref(h)) == _abi.PMX_ERR_INVALID_ARGUMENT


SIG = ("double t, const double* x, const double* p, const double* cov, const double* rateiv, "
       "const double* derived, double* ")
ORAL_SRC = f"""
PMX_DEVICE void pmx_dynamics({SIG}dx) {{
  dx[0] = -p[0] * x[0];
  dx[1] = p[0] * x[0] - p[1] * x[1] + rateiv[0];
}}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[1]; }}
"""
ORAL_LAG_SRC = ORAL_SRC + f"PMX_DEVICE void pmx_route_lag({SIG}lag) {{ lag[0] = p[2]; }}\n"


def _custom(solver="rk4-checked"):
    return ODE.custom(ORAL_SRC, nstates=2, nparams=2, h_max=H_MAX).with_solver(solver)


def _user_lag(solver="rk4-checked"):
    return ODE.user(ORAL_LAG_SRC, nstates=2, nparams=3, ndrugs=1, nout=1, h_max=H_MAX).with_solver(solver)


def test_hiprtc_models_compile_the_checked_entry_points_only_when_asked():
    """A model's solver is fixed at creation: a checked model's translation unit holds the checked walkers INSTEAD of
    the fixed-step and adaptive ones, every other model's is what it always was (no compile time added)."""
    tu = runtime.jit_translation_unit(_custom())
    assert tu.count('extern "C" __global__') == 8 and tu.count("pmx::SOLV_CHECKED>") == 8  # grid/pair x lag x loglik
    plain = runtime.jit_translation_unit(_custom("rk4"))
    assert plain.count('extern "C" __global__') == 16 and "SOLV_CHECKED" not in plain
    runtime.DeviceModel(_custom())  # hiprtc compiles for gfx950 without a device
    runtime.DeviceModel(_user_lag())
    bad = _custom().with_tolerances(0.0, 1e-4)
    with pytest.raises(_abi.PmxError) as e:
        runtime.DeviceModel(bad)
    assert e.value.status == _abi.PMX_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------- device
def _subjects(values=False):
    subs = []
    for i, amt in enumerate(AMOUNTS):
        b = Subject.builder(f"s{i}").bolus(0.0, amt, 0)
        for t in OBS_T:
            b = b.observation(t, 1.0 + 0.5 * i, 0) if values else b.missing_observation(t, 0)
        subs.append(b.build())
    return subs


def _ka_column(n, fail=KA_FAIL):
    """Passing and failing rates interleaved, so that one wave holds both."""
    mix = [v for pair in zip(KA_PASS + KA_PASS, fail) for v in pair] + KA_PASS  # every passing and failing value is in it
    return np.array([mix[i % len(mix)] for i in range(n)])


def _expected(thetas, per_subject_events, batch):
    """(rows [n_obs(, P)], status [S(, P)], plain-RK4 status-0 mask) from the numpy march; asserts every case decisive."""
    S = len(per_subject_events)
    cols = [None] if batch else range(len(thetas))
    rows, stat = [], []
    for s in range(S):
        r_s, st_s = [], []
        for p in cols:
            th = thetas[s] if batch else thetas[p]
            r, st, qs = march(th[0], th[1], per_subject_events[s])
            assert _decisive(qs), (s, th, qs)
            r_s.append(r)
            st_s.append(st)
        rows.append(np.stack(r_s, axis=1))
        stat.append(st_s)
    rows, stat = np.concatenate(rows, axis=0), np.array(stat, dtype=np.uint8)
    return (rows[:, 0], stat[:, 0]) if batch else (rows, stat)


def _gpu(model, flat, theta, batch=False):
    import torch

    pop = runtime.DevicePopulation(flat, 0)
    pred, st = runtime.predict(model, pop, np.ascontiguousarray(theta), batch=batch)
    torch.cuda.synchronize()
    return pred.cpu().numpy(), st.cpu().numpy(), runtime.last_kernel_name()


def _rows_of(st_pairs, flat_rows_per_subject):
    """status per pair -> the same flag per prediction row"""
    return np.repeat(st_pairs, flat_rows_per_subject, axis=0)


def _check(got, st, want, wst, plain, n_obs_per_subject):
    np.testing.assert_array_equal(st, wst)
    bad = _rows_of(wst != 0, n_obs_per_subject)
    assert np.isnan(got[bad]).all()
    assert bad.any() and (~bad).any()  # both kinds of lane in the launch
    ok = ~bad
    assert (np.abs(got[ok] - plain[ok]) <= 1e-12 * np.abs(plain[ok])).all()
    assert (np.abs(got[ok] - want[ok]) <= 1e-10 * np.abs(want[ok])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_support,batch", [(40, False), (4, False), (0, True)])
def test_gpu_builtin_body_every_lane_mapping(n_support, batch):
    subs = _subjects()
    m, plain_m = _builtin(), _builtin("rk4")
    flat = m.flatten(Data(subs))
    if batch:
        theta = np.array([[2.0, KE], [150.0, KE], [5.0, KE]])
    elif n_support == 4:
        theta = np.array([[1.0, KE], [150.0, KE], [10.0, KE], [40.0, KE]])
    else:
        theta = np.stack([_ka_column(n_support), np.full(n_support, KE)], axis=1)
    want, wst = _expected(theta, [_events(a) for a in AMOUNTS], batch)
    got, st, name = _gpu(m, flat, theta, batch)
    assert name == ("pmx_ode_rk4_checked_grid" if n_support >= 32 else "pmx_ode_rk4_checked_pair")
    plain, pst, pname = _gpu(plain_m, flat, theta, batch)
    assert pname == ("pmx_ode_rk4_grid" if n_support >= 32 else "pmx_ode_rk4_pair")
    _check(got, st, want, wst, plain, len(OBS_T))
    # passing pairs: the closed form, at the tolerance the probe was given
    ok = ~_rows_of(wst != 0, len(OBS_T))
    exact = np.empty_like(want)
    for s, amt in enumerate(AMOUNTS):
        for k, t in enumerate(OBS_T):
            if batch:
                exact[s * 4 + k] = closed_form(theta[s, 0], KE, amt, t)
            else:
                exact[s * 4 + k, :] = [closed_form(ka, KE, amt, t) for ka in theta[:, 0]]
    assert (np.abs(got[ok] - exact[ok]) <= 1e-4 * np.abs(exact[ok])).all()
    # the unchecked solver is unchanged: status 0 and a finite (wrong) prediction at ka = 150
    col = (theta[:, 0] == 150.0)
    assert col.any()
    if batch:
        assert (pst[col] == 0).all() and np.isfinite(plain[np.repeat(col, 4)]).all()
    else:
        assert (pst[:, col] == 0).all() and np.isfinite(plain[:, col]).all() and np.abs(plain[:, col]).max() > 1e20
    # host-pointer form: PMX_ERR_PAIR_FAILED, and the message says what to do about it
    h_pred, h_st = runtime.predict_host(m, flat, theta, batch=batch)
    np.testing.assert_array_equal(h_st, wst)
    np.testing.assert_array_equal(np.isnan(h_pred), np.isnan(got))
    with pytest.raises(_abi.PmxError) as e:
        runtime.predict_host(m, flat, theta, batch=batch, raise_on_pair_failure=True)
    assert e.value.status == _abi.PMX_ERR_PAIR_FAILED
    for word in ("h_max", "with_step", "dopri5", "ros2"):
        assert word in str(e.value)


def _late_bolus_subjects():
    """an observation at 0.5 h BEFORE the bolus at 1.0 h"""
    subs = []
    for i, amt in enumerate(AMOUNTS):
        b = Subject.builder(f"late{i}").missing_observation(0.5, 0).bolus(1.0, amt, 0)
        for t in (1.5, 2.0, 5.0):
            b = b.missing_observation(t, 0)
        subs.append(b.build())
    return subs


@pytest.mark.gpu
@pytest.mark.parametrize("n_support", [40, 4])
def test_gpu_rows_before_the_failing_piece_keep_their_values(n_support):
    m, plain_m = _builtin(), _builtin("rk4")
    flat = m.flatten(Data(_late_bolus_subjects()))
    ka = _ka_column(n_support) if n_support > 4 else np.array([150.0, 2.0, 150.0, 10.0])
    theta = np.stack([ka, np.full(n_support, KE)], axis=1)
    ev = [_events(a, t_bolus=1.0, obs=[0.5, 1.5, 2.0, 5.0]) for a in AMOUNTS]
    want, wst = _expected(theta, ev, False)
    got, st, name = _gpu(m, flat, theta)
    assert name == ("pmx_ode_rk4_checked_grid" if n_support >= 32 else "pmx_ode_rk4_checked_pair")
    np.testing.assert_array_equal(st, wst)
    col = theta[:, 0] == 150.0
    assert (st[:, col] == 5).all()
    g = got.reshape(len(AMOUNTS), 4, n_support)
    assert (g[:, 0, :] == 0.0).all()  # before the dose: written, finite, zero - for every lane
    assert np.isnan(g[:, 1:, :][:, :, col]).all()
    plain, _, _ = _gpu(plain_m, flat, theta)
    ok = ~np.isnan(want)
    assert np.isfinite(got[ok]).all() and (np.abs(got[ok] - plain[ok]) <= 1e-12 * np.abs(plain[ok])).all()
    assert (np.abs(got[ok] - want[ok]) <= 1e-10 * np.abs(want[ok])).all()


LAG = 0.25


def _lag_events(amount):
    """bolus recorded at 0, landing at LAG: the observation at 0.1 h comes first (state still zero)"""
    return _events(amount, t_bolus=LAG)


def _lag_case(model_of, n_support, kernel_prefix):
    m, plain_m = model_of("rk4-checked"), model_of("rk4")
    flat = m.flatten(Data(_subjects()))
    # (ka = 30 is left out here: the sub-piece [0.25, 0.5] has h = 0.25 / 13 < 0.02, which moves its q to 9.8, inside the
    # band an FMA contraction could decide)
    ka = _ka_column(n_support, KA_FAIL[1:]) if n_support > 4 else np.array([5.0, 150.0, 1.0, 150.0])
    theta = np.stack([ka, np.full(n_support, KE), np.full(n_support, LAG)], axis=1)
    want, wst = _expected(theta, [_lag_events(a) for a in AMOUNTS], False)
    got, st, name = _gpu(m, flat, theta)
    assert name.startswith(kernel_prefix + ("_grid" if n_support >= 32 else "_pair")), name
    plain, _, _ = _gpu(plain_m, flat, theta)
    np.testing.assert_array_equal(st, wst)
    col = theta[:, 0] == 150.0
    assert (st[:, col] == 5).all()
    g = got.reshape(len(AMOUNTS), 4, n_support)
    assert (wst == wst[0]).all()  # the verdict does not depend on the dose here
    assert (g[:, 0, :] == 0.0).all() and np.isnan(g[:, 1:, :][:, :, wst[0] != 0]).all()
    ok = ~np.isnan(want)
    assert np.isfinite(got[ok]).all() and (np.abs(got[ok] - plain[ok]) <= 1e-12 * np.abs(plain[ok])).all()
    assert (np.abs(got[ok] - want[ok]) <= 1e-10 * np.abs(want[ok])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n_support", [40, 4])
def test_gpu_lag_variant_probes_the_sub_pieces(n_support):
    _lag_case(lambda s: _builtin(s, lag={0: 2}, nparams=3), n_support, "pmx_ode_rk4_checked")


@pytest.mark.gpu
@pytest.mark.parametrize("n_support", [40, 4])
def test_gpu_user_model_with_a_lag_closure_takes_the_general_walker(n_support):
    _lag_case(_user_lag, n_support, "pmx_jit_ode_user_rk4_checked")


@pytest.mark.gpu
@pytest.mark.parametrize("n_support", [40, 4])
def test_gpu_custom_body(n_support):
    m, plain_m = _custom(), _custom("rk4")
    flat = m.flatten(Data(_subjects()))
    ka = _ka_column(n_support) if n_support > 4 else np.array([1.0, 150.0, 10.0, 40.0])
    theta = np.stack([ka, np.full(n_support, KE)], axis=1)
    want, wst = _expected(theta, [_events(a) for a in AMOUNTS], False)
    got, st, name = _gpu(m, flat, theta)
    assert name == ("pmx_jit_ode_rk4_checked_grid" if n_support >= 32 else "pmx_jit_ode_rk4_checked_pair")
    plain, _, _ = _gpu(plain_m, flat, theta)
    _check(got, st, want, wst, plain, len(OBS_T))


@pytest.mark.gpu
@pytest.mark.parametrize("n_support", [40, 4])
def test_gpu_fused_loglik(n_support):
    import torch

    m, plain_m = _builtin(), _builtin("rk4")
    flat = m.flatten(Data(_subjects(values=True)))
    ka = _ka_column(n_support) if n_support > 4 else np.array([1.0, 150.0, 10.0, 40.0])
    theta = np.stack([ka, np.full(n_support, KE)], axis=1)
    _, wst = _expected(theta, [_events(a) for a in AMOUNTS], False)
    em = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.1, 0.1, 0.0, 0.0), 0.0))
    pop = runtime.DevicePopulation(flat, 0)
    ll, st = runtime.loglik(m, pop, em, theta)
    assert runtime.last_kernel_name() == ("pmx_ode_rk4_checked_grid" if n_support >= 32 else "pmx_ode_rk4_checked_pair")
    pll, _ = runtime.loglik(plain_m, pop, em, theta)
    torch.cuda.synchronize()
    ll, st, pll = ll.cpu().numpy(), st.cpu().numpy(), pll.cpu().numpy()
    np.testing.assert_array_equal(st, wst)
    bad = wst != 0
    assert bad.any() and np.isnan(ll[bad]).all() and np.isfinite(ll[~bad]).all()
    assert (np.abs(ll[~bad] - pll[~bad]) <= 1e-12 * np.abs(pll[~bad])).all()
    hll, hst = runtime.loglik_host(m, flat, em, theta)
    np.testing.assert_array_equal(hst, wst)
    assert np.isnan(hll[bad]).all()
    with pytest.raises(_abi.PmxError) as e:
        runtime.loglik_host(m, flat, em, theta, raise_on_pair_failure=True)
    assert e.value.status == _abi.PMX_ERR_PAIR_FAILED and "with_step" in str(e.value)


@pytest.mark.gpu
def test_gpu_fused_loglik_batch_maps_a_coarse_subject_to_minus_infinity():
    m, plain_m = _builtin(), _builtin("rk4")
    flat = m.flatten(Data(_subjects(values=True)))
    theta = np.array([[2.0, KE], [150.0, KE], [5.0, KE]])
    _, wst = _expected(theta, [_events(a) for a in AMOUNTS], True)
    em = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.1, 0.1, 0.0, 0.0), 0.0))
    ll, st = runtime.loglik_batch_host(m, flat, em, theta)
    np.testing.assert_array_equal(st, wst)
    assert list(wst) == [0, 5, 0] and ll[1] == -np.inf and np.isfinite(ll[[0, 2]]).all()
    pll, pst = runtime.loglik_batch_host(plain_m, flat, em, theta)
    assert (np.abs(ll[[0, 2]] - pll[[0, 2]]) <= 1e-12 * np.abs(pll[[0, 2]])).all()
