"""The mixture log-likelihood and D-function kernels (pmx_mixture.hip) on the device: every case of
tests/golden/mixture_math.json within its bar, bit-identical from run to run and for any alignment and pitch, writing
only what the caller owns; the host forms end to end on the classed, generic and pair kernels; shards that add."""
import ctypes as C

import numpy as np
import pytest

import oracle
from pharmsol_amd import AssayErrorModel, AssayErrorModels, Data, ErrorPoly, Subject, _abi, _ffi, runtime, synth
from tests import mixture_cases as mc
from tests import models
from tests.arena import Arena

pytestmark = pytest.mark.gpu

EM_ADD = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.05, 0.1, 0.0, 0.0), 0.1))
EM_PROP = AssayErrorModels.empty().add(0, AssayErrorModel.proportional(ErrorPoly(0.02, 0.15, 0.001, 0.0), 1.3))
STATE = {}


def two_cpt():
    return models.handwritten_analytical("two_compartments", 0, 4).with_ndrugs(1)


def pop_of(S):
    """a device population of S subjects: the reductions take nothing from it but its subject count and its device"""
    if S not in STATE:
        subs = [Subject.builder(str(i)).infusion(0.0, 300.0, 0, 0.5).observation(1.0, 5.0, 0).build() for i in range(S)]
        STATE[S] = runtime.DevicePopulation(two_cpt().flatten(Data(subs)), 0)
    return STATE[S]


def bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("case", mc.doc()["mixture"], ids=mc.case_id)
def test_mixture_rows_within_the_bar_and_bit_identical(case):
    import torch

    ll, w = mc.mixture_inputs(case)
    pop = pop_of(case["S"])
    d_ll, d_w = torch.as_tensor(ll, device="cuda"), torch.as_tensor(w, device="cuda")
    a = runtime.mixture_loglik(pop, d_ll, d_w)
    b = runtime.mixture_loglik(pop, d_ll, d_w)
    torch.cuda.synchronize()
    worst = mc.assert_case(a.cpu().numpy(), case, mc.np_lpyl(ll, w), mc.np_bar_lpyl(ll, w))
    print(f"{mc.case_id(case)}: worst share of a bar {worst:.3f}")
    assert bits(a) == bits(b)


@pytest.mark.parametrize("case", mc.doc()["dfunction"], ids=mc.case_id)
def test_dfunction_within_the_bar_and_bit_identical(case):
    import torch

    ll, lpyl = mc.dfunction_inputs(case)
    pop = pop_of(case["S"])
    d_ll, d_lpyl = torch.as_tensor(ll, device="cuda"), torch.as_tensor(lpyl, device="cuda")
    a = runtime.d_function(pop, d_ll, d_lpyl)
    b = runtime.d_function(pop, d_ll, d_lpyl)
    torch.cuda.synchronize()
    worst = mc.assert_case(a.cpu().numpy(), case, mc.np_d(ll, lpyl), mc.np_bar_d(ll, lpyl))
    print(f"{mc.case_id(case)}: worst share of a bar {worst:.3f}")
    assert bits(a) == bits(b)


def test_negative_or_nan_weight_gives_nan_on_the_device():
    import torch

    case = next(c for c in mc.doc()["mixture"] if (c["S"], c["P"], c["kind"]) == (7, 63, "plain"))
    ll, w = mc.mixture_inputs(case)
    for bad in (-0.25, float("nan")):
        w2 = w.copy()
        w2[17] = bad
        got = runtime.mixture_loglik(pop_of(7), torch.as_tensor(ll, device="cuda"), w2).cpu().numpy()
        assert np.isnan(got).all()


@pytest.mark.parametrize("S,P", [(6, 700), (5, 1024), (5, 1025)])
def test_row_mappings_on_both_sides_of_their_threshold(S, P):
    """A wave owns a row up to 1024 columns and walks it in trips of 4 x 64, a block beyond: several trips of the wave
    mapping (the fixture's widest wave-owned row has 130 columns) and the two widths at the switch, against the float64
    restatement - both sides sit within one bar of the truth."""
    import torch

    ll, w, _ = mc.inputs(S, P, 300.0, 4242 + P)
    ll[1, 5], w[P - 2], ll[2, P - 2] = -np.inf, 0.0, np.nan
    got = runtime.mixture_loglik(pop_of(S), torch.as_tensor(ll, device="cuda"), w).cpu().numpy()
    want = mc.np_lpyl(ll, w)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert np.max(np.abs(got - want) / mc.np_bar_lpyl(ll, w)) <= 2.0


ONE_PER_SHAPE = [c for c in mc.doc()["mixture"] if c["kind"] == "plain" and c["scale"] == 5.0]


@pytest.mark.parametrize("pitch", ["P+1", "recommended"])
@pytest.mark.parametrize("case", ONE_PER_SHAPE, ids=mc.case_id)
def test_any_alignment_and_pitch_same_bits_and_nothing_else_written(case, pitch):
    """Every buffer carved from a dirty arena, 8 but not 16 bytes aligned, rows P + 1 resp. pmx_recommended_ld(P) doubles
    apart: the bits of the dense aligned run, not a byte outside what the caller owns (the scratch slab has exactly
    pmx_dfunction_scratch_doubles), the inputs untouched."""
    import torch

    L = _ffi.lib()
    S, P = case["S"], case["P"]
    ll, w = mc.mixture_inputs(case)
    pop = pop_of(S)
    d_ll, d_w = torch.as_tensor(ll, device="cuda"), torch.as_tensor(w, device="cuda")
    dense_lpyl = runtime.mixture_loglik(pop, d_ll, d_w)
    dense_d = runtime.d_function(pop, d_ll, dense_lpyl)
    if "arena" not in STATE:
        STATE["arena"] = Arena("cuda", 4 << 20)
    arena = STATE["arena"]
    arena.reset()
    ld = P + 1 if pitch == "P+1" else runtime.recommended_ld(P)
    n_scratch = int(L.pmx_dfunction_scratch_doubles(S, P))
    v_ll = arena.carve(S, P, ld, torch.float64, 8, name="ll")
    v_w = arena.carve(1, P, P, torch.float64, 8, name="w")
    v_lpyl = arena.carve(1, S, S, torch.float64, 8, name="lpyl")
    v_scratch = arena.carve(1, n_scratch, n_scratch, torch.float64, 8, name="scratch")
    v_d = arena.carve(1, P, P, torch.float64, 8, name="D")
    for v in (v_ll, v_w, v_lpyl, v_scratch, v_d):
        assert v.data_ptr() % 16 == 8
    v_ll.copy_(d_ll)
    v_w.copy_(d_w.reshape(1, P))
    stream = torch.cuda.current_stream().cuda_stream
    _ffi.check(L.pmx_mixture_loglik_device(pop.handle, v_ll.data_ptr(), P, ld, v_w.data_ptr(), v_lpyl.data_ptr(), stream))
    got_lpyl = v_lpyl.clone()
    _ffi.check(L.pmx_dfunction_device(pop.handle, v_ll.data_ptr(), P, ld, v_lpyl.data_ptr(), v_scratch.data_ptr(),
                                      v_d.data_ptr(), stream))
    torch.cuda.synchronize()
    assert bits(got_lpyl) == bits(dense_lpyl) and bits(v_d) == bits(dense_d)
    arena.assert_clean()
    assert bits(v_ll) == bits(d_ll) and bits(v_w) == bits(d_w) and bits(v_lpyl) == bits(got_lpyl)


# ---- host forms, end to end ------------------------------------------------------------------------------------------
def with_observed_values(model, flat, theta_true, rng, missing_frac=0.15):
    """'measured' values = the oracle's prediction at theta_true x lognormal noise; a fraction stays missing"""
    pred, _ = oracle.predict(model, flat, theta_true)
    pred = pred.reshape(flat.n_observations, -1)[:, 0]
    vals = np.abs(pred) * np.exp(rng.normal(0, 0.2, pred.shape)) + 0.05
    vals[rng.random(pred.shape) < missing_frac] = np.nan
    flat.ev_value = flat.ev_value.copy()
    flat.ev_value[flat.ev_kind == _abi.PMX_EV_OBSERVATION] = vals
    return flat


def c3_population():
    if "c3" not in STATE:
        m, flat, theta = synth.config_c3(61, 130)
        STATE["c3"] = (m, with_observed_values(m, flat, theta[:1], np.random.default_rng(1)), theta)
    return STATE["c3"]


def ragged_population():
    """the 150 ragged subjects (and an empty one) of tests/test_gpu_likelihood.py"""
    if "ragged" not in STATE:
        rng = np.random.default_rng(2)
        subs = [models.random_subject(rng, multi_occasion=True) for _ in range(150)]
        subs.insert(9, Subject.builder("empty").build())
        m = two_cpt()
        flat = m.flatten(Data(subs))
        theta = synth.theta_c3(70)
        STATE["ragged"] = (m, with_observed_values(m, flat, theta[:1], rng), theta)
    return STATE["ragged"]


def weights(P):
    return ((np.arange(P) * 7919) % 1009 + 1.0) / (1009.0 * P)


def host_form(name, m, flat, em, theta, vec, n_out, want_status=True):
    """pmx_mixture_loglik (vec = w) or pmx_dfunction (vec = lpyl) through the C ABI: (rc, out, status)"""
    pop = runtime.DevicePopulation(flat, 0)
    theta, vec = np.ascontiguousarray(theta, dtype=np.float64), np.ascontiguousarray(vec, dtype=np.float64)
    out = np.full(n_out, -7.0)
    status = np.full((pop.n_subjects, theta.shape[0]), 9, dtype=np.uint8)
    rc = getattr(_ffi.lib(), name)(runtime._as_model(m).handle, pop.handle, C.cast(em.to_c(m), C.c_void_p), theta.ctypes.data,
                                   theta.shape[0], vec.ctypes.data, out.ctypes.data, status.ctypes.data if want_status else None)
    return rc, out, status


@pytest.mark.parametrize("which,em,P,kernel", [("c3", EM_PROP, 130, "pmx_analytical_classed_ll"),
                                               ("ragged", EM_ADD, 70, "pmx_analytical_steps"),
                                               ("ragged", EM_PROP, 3, "pmx_analytical_pair")])
def test_host_forms_match_the_restatement_on_the_device_matrix(which, em, P, kernel):
    import torch

    m, flat, theta = c3_population() if which == "c3" else ragged_population()
    theta = np.ascontiguousarray(theta[:P])
    w = weights(P)
    ll, st = runtime.loglik(m, runtime.DevicePopulation(flat, 0), em, theta)
    torch.cuda.synchronize()
    assert runtime.last_kernel_name().startswith(kernel), runtime.last_kernel_name()
    ll = ll.cpu().numpy()
    S = ll.shape[0]
    assert (st.cpu().numpy() == 0).all() and np.isfinite(ll).all()
    rc, lpyl, status = host_form("pmx_mixture_loglik", m, flat, em, theta, w, S)
    assert rc == _abi.PMX_OK and (status == 0).all()
    worst = np.max(np.abs(lpyl - mc.np_lpyl(ll, w)) / mc.np_bar_lpyl(ll, w))
    print(f"lpyl: worst {worst:.3f} bars")
    assert worst <= 2.0  # both sides sit within one bar of the truth
    rc, D, status = host_form("pmx_dfunction", m, flat, em, theta, lpyl, P)
    assert rc == _abi.PMX_OK and (status == 0).all()
    worst = np.max(np.abs(D - mc.np_d(ll, lpyl)) / mc.np_bar_d(ll, lpyl))
    print(f"D: worst {worst:.3f} bars")
    assert worst <= 2.0


def test_host_forms_failed_pair_under_zero_weight_and_refused_weights():
    m, flat, theta = c3_population()
    P, S = 12, 61
    th = np.ascontiguousarray(theta[:P]).copy()
    th[3, 1], th[3, 0], th[3, 2] = -3.0, 1.0, 1.0  # support point 3: complex eigenvalues
    w = weights(P)
    w[3] = 0.0
    rc, lpyl, status = host_form("pmx_mixture_loglik", m, flat, EM_ADD, th, w, S)
    assert rc == _abi.PMX_ERR_PAIR_FAILED
    assert (status[:, 3] == _abi.PMX_PAIR_COMPLEX_ROOTS).all() and (np.delete(status, 3, axis=1) == 0).all()
    assert np.isfinite(lpyl).all()  # the failed support point carries no weight: it poisons nobody
    rc2, lpyl2, _ = host_form("pmx_mixture_loglik", m, flat, EM_ADD, th, w, S, want_status=False)  # the same without a status array
    assert rc2 == rc and lpyl2.tobytes() == lpyl.tobytes()
    # the D-function of the same candidates: the failed one is NaN, the others finite; the outputs are still copied out
    rc, D, status = host_form("pmx_dfunction", m, flat, EM_ADD, th, lpyl, P)
    assert rc == _abi.PMX_ERR_PAIR_FAILED and (status[:, 3] == _abi.PMX_PAIR_COMPLEX_ROOTS).all()
    assert np.isnan(D[3]) and np.isfinite(np.delete(D, 3)).all()
    for bad in (-0.5, float("nan"), None):  # a negative weight, a NaN weight, no positive weight at all
        w2 = weights(P) if bad is not None else np.zeros(P)
        w2[5] = 0.0 if bad is None else bad
        rc, out, _ = host_form("pmx_mixture_loglik", m, flat, EM_ADD, th, w2, S)
        assert rc == _abi.PMX_ERR_INVALID_ARGUMENT and (out == -7.0).all()


def test_d_of_two_shards_adds_up():
    """each shard's D subtracts its own subject count, so the shards' vectors simply add"""
    import torch

    m, flat, theta = ragged_population()
    w = weights(70)
    whole = runtime.DevicePopulation(flat, 0)
    ll, _ = runtime.loglik(m, whole, EM_ADD, theta)
    lpyl = runtime.mixture_loglik(whole, ll, w)
    D = runtime.d_function(whole, ll, lpyl)
    S, cut = whole.n_subjects, 64
    parts = []
    for s0, s1 in ((0, cut), (cut, S)):
        shard = runtime.DevicePopulation(flat, 0, subjects=(s0, s1))
        assert shard.n_subjects == s1 - s0
        ll_r, _ = runtime.loglik(m, shard, EM_ADD, theta)
        parts.append(runtime.d_function(shard, ll_r, lpyl[s0:s1].contiguous()))
    torch.cuda.synchronize()
    got = (parts[0] + parts[1]).cpu().numpy()
    bar = mc.np_bar_d(ll.cpu().numpy(), lpyl.cpu().numpy())
    worst = np.max(np.abs(got - D.cpu().numpy()) / bar)
    print(f"shards: worst {worst:.3f} bars")
    assert worst <= 1.0
