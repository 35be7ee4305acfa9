"""API items around the hot path that a pharmsol caller uses to drive it:
``ParameterOrder`` (parameter_order.rs:12-116, parameters.rs:104-165), ``Prediction`` fields / ``PopulationPredictions``
(prediction.rs:18-27, subject.rs:140-165), per-subject ``estimate_log_likelihood`` / ``simulate_subject``
(equation/mod.rs:468-477,569-576), ``log_likelihood_batch`` with prediction-based ``ResidualErrorModels`` and its
failure -> -inf rule (likelihood/mod.rs:119-177, residual_error.rs:178-271), the host-pointer entry points' persistent
workspace (pinned or pageable outputs); what every model-creation path refuses of an ODE descriptor's solver fields."""
import ctypes as C
import importlib.util
import json
import math
import os

import numpy as np
import pytest

import oracle
from pharmsol_amd import (ODE, Analytical, AssayErrorModel, AssayErrorModels, Censor, Data, ErrorPoly, ParameterError,
                          ParameterOrder, Parameters, Ratio, ResidualErrorModel, ResidualErrorModels, Subject, _abi, _ffi,
                          runtime, synth)
from tests import models


# --------------------------------------------------------------------------- ParameterOrder (no GPU)
def test_parameter_order_permutes_values_and_matrices_into_model_order():
    m = models.readme_analytical()  # params ka, ke0, v
    order = ParameterOrder.with_model(m, ["v", "ka", "ke0"])
    assert order.permutation() == [1, 2, 0] and order.width() == 3 and not order.is_identity()
    np.testing.assert_array_equal(order.values([50.0, 1.0, 0.2]), [1.0, 0.2, 50.0])
    mat = order.matrix(np.array([[50.0, 1.0, 0.2], [60.0, 1.5, 0.3]]))
    np.testing.assert_array_equal(mat, [[1.0, 0.2, 50.0], [1.5, 0.3, 60.0]])
    assert mat.flags["C_CONTIGUOUS"]  # the row-major theta the library takes (matrix.rs:62-65)
    assert ParameterOrder.with_model(m, ["ka", "ke0", "v"]).is_identity()
    np.testing.assert_array_equal(order.parameters([50.0, 1.0, 0.2]).as_slice(),
                                  Parameters.with_model(m, [("ka", 1.0), ("ke0", 0.2), ("v", 50.0)]).as_slice())


def test_parameter_order_errors():
    m = models.readme_analytical()
    with pytest.raises(ParameterError, match="UnknownParameter"):
        ParameterOrder.with_model(m, ["ka", "ke0", "volume"])
    with pytest.raises(ParameterError, match="DuplicateParameter"):
        ParameterOrder.with_model(m, ["ka", "ka", "v"])
    with pytest.raises(ParameterError, match="MissingParameters"):
        ParameterOrder.with_model(m, ["ka", "v"])
    with pytest.raises(ParameterError, match="WidthMismatch"):
        ParameterOrder.with_model(m, ["v", "ka", "ke0"]).matrix(np.zeros((2, 4)))


def test_residual_error_model_sigma_rules():
    # residual_error.rs:178-191 (the doc examples :57-66) and the floor at sqrt(f64::EPSILON)
    assert ResidualErrorModel.constant(0.5).sigma(100.0) == 0.5
    assert abs(ResidualErrorModel.proportional(0.1).sigma(-100.0) - 10.0) < 1e-12
    assert abs(ResidualErrorModel.combined(0.5, 0.1).sigma(100.0) - math.sqrt(100.25)) < 1e-12
    assert ResidualErrorModel.proportional(0.1).sigma(0.0) == math.sqrt(2.220446049250313e-16)


def _batch_case(n=37, seed=3):
    rng = np.random.default_rng(seed)
    m = models.handwritten_analytical("two_compartments", 0, 4).with_nout(2)
    m.out = {0: Ratio(0, 3), 1: Ratio(1, None)}
    subs = []
    for i in range(n):
        b = Subject.builder(f"b{i}").infusion(0.0, 300.0 + i, 0, 0.5).bolus(6.0, 50.0, 0)
        for k, t in enumerate(np.sort(rng.uniform(0.6, 24.0, 6))):
            b = b.observation(float(t), float(rng.uniform(0.5, 6.0)), k % 2) if k != 2 else b.missing_observation(float(t), 0)
        subs.append(b.build())
    theta = synth.theta_c3(n, synth.SplitMix64(seed))
    rem = (ResidualErrorModels.new().add(0, ResidualErrorModel.combined(0.3, 0.1)).add(1, ResidualErrorModel.proportional(0.2)))
    return m, subs, theta, rem


def test_oracle_residual_log_likelihood_matches_the_reference_formula():
    m, subs, theta, rem = _batch_case(5)
    flat = m.flatten(Data(subs))
    ll, _ = oracle.loglik(m, flat, rem, theta[:1])
    pred, _ = oracle.predict(m, flat, theta[:1])
    row = 0
    for s, sub in enumerate(subs):
        want = 0.0
        for ev in sub.occasions[0].events:
            if hasattr(ev, "outeq"):
                if ev.value is not None:
                    em = rem._m[int(ev.outeq)]
                    sg = em.sigma(pred[row, 0])
                    want += -0.5 * (math.log(2 * math.pi) + 2 * math.log(sg) + ((ev.value - pred[row, 0]) / sg) ** 2)
                row += 1
        assert abs(ll[s, 0] - want) < 1e-10 * max(1.0, abs(want))


# --------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_log_likelihood_batch_and_the_failure_to_minus_infinity_rule():
    m, subs, theta, rem = _batch_case()
    theta[5, 1], theta[5, 0], theta[5, 2] = -3.0, 1.0, 1.0  # complex eigenvalues for subject 5 (the reference panics; Err -> -inf)
    got = m.log_likelihood_batch(Data(subs), theta, rem)
    assert runtime.last_kernel_name().startswith("pmx_analytical_pair")
    assert got.shape == (len(subs),) and got[5] == -np.inf
    flat = m.flatten(Data(subs))
    for i in (0, 1, 7, 20, 36):
        want, _ = oracle.loglik(m, flat.subject_slice(i, i + 1), rem, theta[i:i + 1])
        assert abs(got[i] - want[0, 0]) <= 1e-9 * max(1.0, abs(want[0, 0]))
    with pytest.raises(ValueError):
        m.log_likelihood_batch(Data(subs), theta[:-1], rem)


@pytest.mark.gpu
@pytest.mark.parametrize("n_support,shared", [(70, True), (70, False), (5, False)])
def test_residual_error_models_through_the_matrix_entry(n_support, shared):
    """Prediction-based sigma inside the fused kernels: classed (exact / loose chunks fold from the full records),
    generic GRID and PAIR, against the oracle."""
    import torch

    m, subs, theta, rem = _batch_case(43, seed=4)
    if shared:  # a shared design: exact classes
        proto = subs[0]
        subs = []
        for i in range(43):
            b = Subject.builder(f"s{i}").infusion(0.0, 300.0 + i, 0, 0.5).bolus(6.0, 50.0, 0)
            for ev in proto.occasions[0].events:
                if hasattr(ev, "outeq"):
                    b = b.observation(ev.time, ev.value * (1 + 0.01 * i), ev.outeq) if ev.value is not None else b.missing_observation(ev.time, ev.outeq)
            subs.append(b.build())
    flat = m.flatten(Data(subs))
    th = synth.theta_c3(n_support)
    ll, st = runtime.loglik(m, runtime.DevicePopulation(flat, 0), rem, th)
    torch.cuda.synchronize()
    want, wst = oracle.loglik(m, flat, rem, th)
    np.testing.assert_array_equal(st.cpu().numpy(), wst)
    assert (np.abs(ll.cpu().numpy() - want) / np.maximum(np.abs(want), 1.0)).max() < 1e-9


@pytest.mark.gpu
def test_per_subject_entry_points_and_result_containers():
    m = models.readme_analytical()
    subj = (Subject.builder("one").bolus(0.0, 500.0, "oral").observation(0.5, 1.2, "cp")
            .censored_observation(1.0, 0.3, "cp", Censor.BLOQ).missing_observation(2.0, "cp").covariate("wt", 0.0, 75.0).build())
    p = Parameters.with_model(m, [("ka", 1.0), ("ke0", 0.08), ("v", 150.0)])
    em = AssayErrorModels.empty().add("cp", AssayErrorModel.additive(ErrorPoly(0.1, 0.1, 0.0, 0.0), 0.0))
    preds = m.estimate_predictions(subj, p, with_state=True)
    flat = m.flatten(subj)
    want, _ = oracle.predict(m, flat, p.as_slice())
    np.testing.assert_allclose(preds.flat_predictions(), want[:, 0], rtol=1e-9)
    # Prediction.state = the amounts at the observation: central / v is the prediction
    for pr in preds.predictions():
        assert len(pr.state) == 2 and abs(pr.state[1] / 150.0 - pr.prediction) < 1e-9 * max(1.0, pr.prediction)
    assert preds.predictions()[0].censoring == Censor.NONE and preds.predictions()[1].censoring == Censor.BLOQ
    assert preds.predictions()[2].observation is None
    assert abs(preds.squared_error() - sum((o - q) ** 2 for o, q in zip(preds.flat_observations(), preds.flat_predictions()) if o is not None)) < 1e-12
    ll = m.estimate_log_likelihood(subj, p, em)
    wll, _ = oracle.loglik(m, flat, em, p.as_slice())
    assert abs(ll - wll[0, 0]) < 1e-9 * max(1.0, abs(ll))
    preds2, lik = m.simulate_subject(subj, p, em)
    assert abs(lik - math.exp(ll)) < 1e-12 * max(1.0, lik) and preds2.flat_predictions() == preds.flat_predictions()
    assert m.simulate_subject(subj, p)[1] is None
    # PopulationPredictions: subjects x support points from one device pass
    th = np.stack([p.as_slice(), p.as_slice() * 1.1])
    pp = m.population_predictions(Data([subj, subj]), th)
    assert pp.shape == (2, 2)
    np.testing.assert_allclose(pp[1, 0].flat_predictions(), preds.flat_predictions(), rtol=1e-12)
    w2, _ = oracle.predict(m, flat, th)
    np.testing.assert_allclose(pp[0, 1].flat_predictions(), w2[:, 1], rtol=1e-9)


@pytest.mark.gpu
def test_host_pointer_entry_points_reuse_their_workspace_and_take_pinned_or_pageable_outputs():
    """pmx_predict / pmx_loglik keep device buffers, streams and pinned staging on the population handle: growing and
    shrinking calls, pageable and page-locked outputs, padded leading dimensions - the same numbers every time."""
    import ctypes as C

    from pharmsol_amd import _ffi

    L = _ffi.lib()
    m, flat, theta = synth.config_c3(3000, 96)
    dm, pop = runtime._as_model(m), runtime.DevicePopulation(flat, 0)
    want, _ = oracle.predict(m, flat, theta)
    NO, P = pop.n_observations, 96
    for trial, (npts, ld, pinned) in enumerate([(96, 96, False), (17, 17, True), (96, 100, False), (96, 128, True), (96, 96, True)]):
        out = (runtime.host_empty((NO, ld)) if pinned else np.empty((NO, ld)))
        out[:] = -7.0
        st = np.zeros((pop.n_subjects, npts), dtype=np.uint8)
        th = np.ascontiguousarray(theta[:npts])
        _ffi.check(L.pmx_predict(dm.handle, pop.handle, th.ctypes.data, npts, out.ctypes.data, ld, st.ctypes.data))
        err = np.abs(out[:, :npts] - want[:, :npts]) / np.maximum(np.abs(want[:, :npts]), 1e-12)
        assert err.max() < 1e-9 and not st.any(), trial
        assert (out[:, npts:] == -7.0).all()  # the caller's padding columns are left alone
    # a matrix larger than the 32 MB bounce buffers through the pageable path (several pieces, split at row ends)
    m2, flat2, theta2 = synth.config_c3(9000, 128)
    pop2 = runtime.DevicePopulation(flat2, 0)
    out = np.empty((pop2.n_observations, 130))
    _ffi.check(L.pmx_predict(runtime._as_model(m2).handle, pop2.handle, theta2.ctypes.data, 128, out.ctypes.data, 130, None))
    w2, _ = oracle.predict(m2, flat2.subject_slice(8990, 9000), theta2)
    np.testing.assert_allclose(out[-w2.shape[0]:, :128], w2, rtol=1e-9)
    # failures: the flag comes from a device-side reduction, the status array is optional
    bad = theta.copy()
    bad[3, 1] = -1.5
    bad[3, 0], bad[3, 2] = 1.0, 1.0  # (ke + kcp + kpc)^2 < 4 ke kpc: complex eigenvalues
    sink = np.empty((NO, 96))
    rc = L.pmx_predict(dm.handle, pop.handle, bad.ctypes.data, 96, sink.ctypes.data, 96, None)
    assert rc == _abi.PMX_ERR_PAIR_FAILED and np.isnan(sink[:, 3]).all() and np.isfinite(np.delete(sink, 3, axis=1)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("want_status", [False, True])
def test_host_pointer_forms_return_what_their_device_twins_return(want_status):
    """pmx_predict, pmx_predict_batch, pmx_loglik and pmx_loglik_batch upload theta, run the kernels of their *_device
    twins and copy out: the same bits, in a padded matrix (ld 8 for 5 support points, the padding left alone), with and
    without a status array.  One pair with complex eigenvalues: PMX_ERR_PAIR_FAILED from the matrix forms and from
    pmx_predict_batch, -inf in that row and PMX_OK from pmx_loglik_batch.  A negative-sigma error model is refused with
    PMX_ERR_ERROR_MODEL, and the next call on the same population succeeds."""
    import torch

    L = _ffi.lib()
    m, subs, thb, rem = _batch_case(43)
    flat = m.flatten(Data(subs))
    dm, pop = runtime._as_model(m), runtime.DevicePopulation(flat, 0)
    S, NO, P, LD = pop.n_subjects, pop.n_observations, 5, 8
    assert S == 43
    th = synth.theta_c3(P)
    th[3, 1], th[3, 0], th[3, 2] = -3.0, 1.0, 1.0    # support point 3: complex eigenvalues
    thb[5, 1], thb[5, 0], thb[5, 2] = -3.0, 1.0, 1.0  # batch forms: subject 5
    em = rem.to_c(m)
    emp = C.cast(em, C.c_void_p)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def same_bits(a, b):
        return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()

    def status_arg(shape):
        st = np.full(shape, 9, dtype=np.uint8) if want_status else None
        return st, (st.ctypes.data if want_status else None)

    # ---- the device twins
    d_pred = torch.full((NO, LD), -7.0, dtype=torch.float64, device=dev)
    _, d_st = runtime.predict(m, pop, th, pred=d_pred[:, :P])
    d_predb, d_stb = runtime.predict(m, pop, thb, batch=True)
    d_ll = torch.full((S, LD), -7.0, dtype=torch.float64, device=dev)
    _, d_llst = runtime.loglik(m, pop, rem, th, ll=d_ll[:, :P])
    d_llb = torch.empty((S,), dtype=torch.float64, device=dev)
    d_llbst = torch.zeros((S,), dtype=torch.uint8, device=dev)
    t_thb = torch.as_tensor(thb, device=dev)
    _ffi.check(L.pmx_loglik_batch_device(dm.handle, pop.handle, emp, t_thb.data_ptr(), d_llb.data_ptr(), d_llbst.data_ptr(), stream))
    torch.cuda.synchronize()
    d_pred, d_st, d_predb, d_stb = d_pred.cpu().numpy(), d_st.cpu().numpy(), d_predb.cpu().numpy(), d_stb.cpu().numpy()
    d_ll, d_llst, d_llb, d_llbst = d_ll.cpu().numpy(), d_llst.cpu().numpy(), d_llb.cpu().numpy(), d_llbst.cpu().numpy()
    assert d_st[:, 3].all() and not np.delete(d_st, 3, axis=1).any() and d_stb[5] and d_llbst[5] and d_llbst.sum() == d_llbst[5]
    assert (d_pred[:, P:] == -7.0).all() and (d_ll[:, P:] == -7.0).all()

    # ---- pmx_predict
    out = np.full((NO, LD), -7.0)
    st, stp = status_arg((S, P))
    rc = L.pmx_predict(dm.handle, pop.handle, th.ctypes.data, P, out.ctypes.data, LD, stp)
    assert rc == _abi.PMX_ERR_PAIR_FAILED and same_bits(out, d_pred)
    assert st is None or np.array_equal(st, d_st)
    # ---- pmx_predict_batch
    outb = np.full((NO,), -7.0)
    st, stp = status_arg((S,))
    rc = L.pmx_predict_batch(dm.handle, pop.handle, thb.ctypes.data, outb.ctypes.data, stp)
    assert rc == _abi.PMX_ERR_PAIR_FAILED and same_bits(outb, d_predb)
    assert st is None or np.array_equal(st, d_stb)
    # ---- pmx_loglik
    ll = np.full((S, LD), -7.0)
    st, stp = status_arg((S, P))
    rc = L.pmx_loglik(dm.handle, pop.handle, emp, th.ctypes.data, P, ll.ctypes.data, LD, stp)
    assert rc == _abi.PMX_ERR_PAIR_FAILED and same_bits(ll, d_ll)
    assert st is None or np.array_equal(st, d_llst)
    # ---- pmx_loglik_batch: the failed subject becomes -inf, the call succeeds
    llb = np.full((S,), -7.0)
    st, stp = status_arg((S,))
    rc = L.pmx_loglik_batch(dm.handle, pop.handle, emp, thb.ctypes.data, llb.ctypes.data, stp)
    assert rc == _abi.PMX_OK and llb[5] == -np.inf and same_bits(np.delete(llb, 5), np.delete(d_llb, 5))
    assert st is None or np.array_equal(st, d_llbst)
    # ---- an error return leaves the workspace usable
    bad = (AssayErrorModels.empty().add(0, AssayErrorModel.proportional(ErrorPoly(0.02, 0.15, 0.0, 0.0), -1.0))
           .add(1, AssayErrorModel.additive(ErrorPoly(0.1, 0.1, 0.0, 0.0), 0.0))).to_c(m)
    ll2 = np.full((S, LD), -7.0)
    st, stp = status_arg((S, P))
    rc = L.pmx_loglik(dm.handle, pop.handle, C.cast(bad, C.c_void_p), th.ctypes.data, P, ll2.ctypes.data, LD, stp)
    assert rc == _abi.PMX_ERR_ERROR_MODEL and "NegativeSigma" in L.pmx_last_error().decode()
    ll2[:] = -7.0
    rc = L.pmx_loglik(dm.handle, pop.handle, emp, th.ctypes.data, P, ll2.ctypes.data, LD, stp)
    assert rc == _abi.PMX_ERR_PAIR_FAILED and same_bits(ll2, d_ll)
    assert st is None or np.array_equal(st, d_llst)


# --------------------------------------------------------------------------- ODE solver fields (no GPU, no compiler)
_SIG = "double t, const double* x, const double* p, const double* cov, const double* rateiv, const double* derived, double* "
_ORAL_SRC = (f"PMX_DEVICE void pmx_dynamics({_SIG}dx) {{ dx[0] = -p[0] * x[0]; dx[1] = p[0] * x[0] - p[1] * x[1] + rateiv[0]; }}\n"
             f"PMX_DEVICE void pmx_outputs({_SIG}y) {{ y[0] = x[1]; }}\n")
_ORAL_LAG_SRC = _ORAL_SRC + f"PMX_DEVICE void pmx_route_lag({_SIG}lag) {{ lag[0] = p[2]; }}\n"


def test_every_creation_path_refuses_unknown_solvers_and_missing_tolerances():
    """pmx_model_create (built-in diffeq body), pmx_model_create_custom and pmx_model_create_user (ODE descriptor with a
    lag closure: the general walker's path) check the same three numbers the same way: ode_solver -1, 4 and 6 are no
    solvers; every solver but plain RK4 needs ode_rtol > 0 and ode_atol > 0.  Each call is refused by the descriptor
    check, before the source text is looked at."""
    L = _ffi.lib()
    builtin = ODE.new("one_cmt_oral", {0: Ratio(1)}, nparams=2, h_max=0.02).with_nstates(2).with_ndrugs(1).with_nout(1)
    custom = ODE.custom(_ORAL_SRC, nstates=2, nparams=2, h_max=0.02)
    user = ODE.user(_ORAL_LAG_SRC, nstates=2, nparams=3, ndrugs=1, nout=1, h_max=0.02)
    assert user.user_fns & _abi.PMX_FN_ROUTE_LAG  # (without a closure beyond the dynamics the call is create_custom's)
    paths = {
        "create": lambda d, h: L.pmx_model_create(C.byref(d), C.byref(h)),
        "create_custom": lambda d, h: L.pmx_model_create_custom(C.byref(d), _ORAL_SRC.encode(), 0, C.byref(h)),
        "create_user": lambda d, h: L.pmx_model_create_user(C.byref(d), _ORAL_LAG_SRC.encode(), int(user.user_fns), C.byref(h)),
    }
    models_ = {"create": builtin, "create_custom": custom, "create_user": user}
    need_tol = (_abi.PMX_SOLVER_DOPRI5, _abi.PMX_SOLVER_ROS2, _abi.PMX_SOLVER_RK4_CHECKED, _abi.PMX_SOLVER_AUTO)

    def refused(path, **fields):
        d = models_[path].desc()
        d.ode_rtol = d.ode_atol = 1e-6
        for k, v in fields.items():
            setattr(d, k, v)
        h = C.c_void_p()
        rc = paths[path](d, h)
        assert rc == _abi.PMX_ERR_INVALID_ARGUMENT and not h.value, (path, fields, rc)

    for path in paths:
        for solver in (-1, 4, 6):
            refused(path, ode_solver=solver)
        for solver in need_tol:
            refused(path, ode_solver=solver, ode_rtol=0.0)
            refused(path, ode_solver=solver, ode_atol=0.0)


# --------------------------------------------------------------------------- model creation (no GPU; hiprtc needs none)
_HERE = os.path.dirname(os.path.abspath(__file__))


def _load_refusals():
    spec = importlib.util.spec_from_file_location("gen_model_refusals", os.path.join(_HERE, "golden", "gen_model_refusals.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(_HERE, "golden", "model_refusals.json")) as f:
        return gen, json.load(f)


# One check that carried two wordings keeps the more specific one on every path: recorded text -> {fault: text now}
_REWORDED = {
    "bind entry out of range": {"bind_index": "bind index out of range", "bind_index_negative": "bind index out of range",
                                "bind_derived_index": "bind derived index out of range",
                                "bind_src": "bind.src must be PRIMARY or DERIVED"},
}


def test_every_creation_path_answers_as_recorded_before_the_path_table():
    """tests/golden/model_refusals.json holds what the five creation paths answered - return code, error text, and the
    SHA-256 of every translation unit the debug calls returned - before the four validators became one path table
    (tests/golden/gen_model_refusals.py; one fault per case, both sides of every bound the paths differ in).  Every case
    is replayed: same code, same text but for the rewordings of _REWORDED, a handle or text exactly when the code is 0,
    the same translation unit."""
    gen, fx = _load_refusals()
    L = _ffi.lib()
    assert len(fx["cases"]) > 200 and sum("sha256" in c for c in fx["cases"]) >= 20
    for c in fx["cases"]:
        rc, text, null, sha = gen.run_case(L, fx, c)
        want = _REWORDED.get(c["text"], {}).get(c["name"].split("/")[-1], c["text"])
        assert (rc, text) == (c["code"], want), c["name"]
        assert null == (rc != _abi.PMX_OK), c["name"]
        assert sha == c.get("sha256"), c["name"]
    reworded = [c["name"] for c in fx["cases"] if c["text"] in _REWORDED]
    assert len(reworded) == 8  # four faults of bind[] on the two paths that said "bind entry out of range"


def test_the_debug_calls_show_what_creation_compiles():
    """A custom diffeq body with five lagged inputs is created on the general ODE walker (the state-machine kernels keep
    four lag cursors): pmx_debug_jit_source shows that translation unit - pmx_ode_user.hpp - and the same text as
    pmx_debug_jit_source_user for the closure set creation passes on.  What creation refuses, the debug calls refuse:
    the general walker's row (init_param here) and an unknown eq_kind."""
    gen, fx = _load_refusals()
    L = _ffi.lib()
    five = [[f"lag_param[{i}]", 2] for i in range(5)] + [["ndrugs", 5]]

    def text_of(call, edits, **how):
        case = dict(base="custom", edits=edits, call=call, source="body_init", **how)
        d = gen.make_desc(fx["bases"]["custom"], edits)
        h = C.c_void_p()
        if call == "debug_jit_source":
            rc = L.pmx_debug_jit_source(C.byref(d), fx["sources"][case["source"]].encode(), how["has_init"], C.byref(h))
        else:
            rc = L.pmx_debug_jit_source_user(C.byref(d), fx["sources"][case["source"]].encode(), how["fns"], C.byref(h))
        if rc != _abi.PMX_OK:
            assert not h.value
            return rc, L.pmx_last_error().decode()
        try:
            return rc, C.string_at(h.value).decode()
        finally:
            L.pmx_free_text(h)

    body = _abi.PMX_FN_DYNAMICS | _abi.PMX_FN_OUTPUTS
    for has_init in (0, 1):
        rc, tu = text_of("debug_jit_source", five, has_init=has_init)
        assert rc == _abi.PMX_OK and '#include "pmx_ode_user.hpp"' in tu and '#include "pmx_ode.hpp"' not in tu
        assert (rc, tu) == text_of("debug_jit_source_user", five, fns=body | (_abi.PMX_FN_INIT if has_init else 0))
        rc4, tu4 = text_of("debug_jit_source", five[1:], has_init=has_init)  # four lagged inputs: the state-machine kernels
        assert rc4 == _abi.PMX_OK and '#include "pmx_ode.hpp"' in tu4
    for call, how in (("debug_jit_source", dict(has_init=0)), ("debug_jit_source_user", dict(fns=body))):
        assert text_of(call, five + [["init_param[0]", 3]], **how) == (_abi.PMX_ERR_INVALID_ARGUMENT, "init_param out of range")
        assert text_of(call, five[1:] + [["init_param[0]", 3]], **how)[0] == _abi.PMX_OK  # (the custom path does not read init_param)
    assert text_of("debug_jit_source_user", [["eq_kind", 7]], fns=_abi.PMX_FN_ROUTE_LAG) == (_abi.PMX_ERR_INVALID_ARGUMENT, "unknown eq_kind")
