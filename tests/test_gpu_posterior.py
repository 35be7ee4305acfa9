"""The posterior and the prediction summaries (pmx_posterior.hip) on the device: every case of
tests/golden/posterior_math.json within its bar with medians equal, bit-identical from run to run and for any alignment
and pitch, writing only what the caller owns; both sides of every mapping threshold; end to end on a real population
through the device sequence and through the host form; shards whose rows concatenate."""
import ctypes as C

import numpy as np
import pytest

from pharmsol_amd import AssayErrorModel, AssayErrorModels, Data, ErrorPoly, Subject, _abi, _ffi, runtime, synth
from tests import models
from tests import posterior_cases as pc
from tests.arena import Arena

pytestmark = pytest.mark.gpu

EM_ADD = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.05, 0.1, 0.0, 0.0), 0.1))
STATE = {}
CASES = pc.doc()["cases"]
COMBOS = [(True, True), (True, False), (False, True)]


def two_cpt():
    return models.handwritten_analytical("two_compartments", 0, 4).with_ndrugs(1)


def pop_of(rows):
    """a device population whose subject s owns rows[s] observation rows: the kernels take nothing else from it"""
    key = tuple(rows)
    if key not in STATE:
        subs = []
        for i, n in enumerate(rows):
            b = Subject.builder(str(i)).infusion(0.0, 300.0, 0, 0.5)
            for k in range(n):
                b = b.observation(1.0 + k, 5.0, 0)
            subs.append(b.build())
        STATE[key] = runtime.DevicePopulation(two_cpt().flatten(Data(subs)), 0)
        assert STATE[key].n_observations == sum(rows) and STATE[key].n_subjects == len(rows)
    return STATE[key]


def bits(t):
    return None if t is None else t.cpu().numpy().tobytes()


def dev(x):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def summarize(pop, mode, d_pred, d_w, d_ll, d_lpyl, mean=True, median=True):
    if mode == "population":
        return runtime.summarize_predictions(pop, d_pred, d_w, mean=mean, median=median)
    return runtime.summarize_predictions(pop, d_pred, d_w, d_ll, d_lpyl, mean=mean, median=median)


@pytest.mark.parametrize("case", CASES, ids=pc.case_id)
def test_posterior_within_the_bar_and_bit_identical(case):
    import torch

    ll, w, lpyl, _, _ = pc.case_inputs(case)
    pop = pop_of(case["rows"])
    d_ll, d_w, d_lpyl = dev(ll), dev(w), dev(lpyl)
    a = runtime.posterior(pop, d_ll, d_w, d_lpyl)
    b = runtime.posterior(pop, d_ll, d_w, d_lpyl)
    torch.cuda.synchronize()
    worst = pc.assert_q(a.cpu().numpy(), case, ll, w, lpyl)
    print(f"{pc.case_id(case)}: q worst share of a bar {worst:.3f}")
    assert bits(a) == bits(b)


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("case", CASES, ids=pc.case_id)
def test_summaries_within_the_bar_medians_equal_and_bit_identical(case, mode):
    import torch

    ll, w, lpyl, pred, obs_off = pc.case_inputs(case)
    pop = pop_of(case["rows"])
    d_ll, d_w, d_lpyl, d_pred = dev(ll), dev(w), dev(lpyl), dev(pred)
    got = {}
    for combo in COMBOS:
        got[combo] = summarize(pop, mode, d_pred, d_w, d_ll, d_lpyl, *combo)
    again = summarize(pop, mode, d_pred, d_w, d_ll, d_lpyl)
    torch.cuda.synchronize()
    mean, median = got[(True, True)]
    worst = pc.assert_summary(mean.cpu().numpy(), median.cpu().numpy(), case, mode, pred,
                              pc.row_q(mode, ll, w, lpyl, obs_off), pc.row_x(mode, ll, lpyl, obs_off))
    print(f"{pc.case_id(case)} {mode}: mean worst share of a bar {worst:.3f}")
    assert got[(True, False)][1] is None and got[(False, True)][0] is None
    assert bits(got[(True, False)][0]) == bits(mean) and bits(got[(False, True)][1]) == bits(median)
    assert bits(again[0]) == bits(mean) and bits(again[1]) == bits(median)


@pytest.mark.parametrize("P", [64, 65, 256, 257, 1024, 1025, 4096, 4097])
def test_mappings_on_both_sides_of_their_thresholds(P):
    """A lane keeps 1, 4 or 16 columns of a wave-owned item (up to 64, 256, 1024 columns), 16 of a block-owned one (up to
    4096); wider rows are re-read in every round.  Both widths at every switch, against the float64 restatement - both
    sides sit within one bar of the truth; the medians' margins are checked first, so that no summation order moves one."""
    import torch

    rows = [7, 1, 2, 40, 7] if P <= 1025 else [3, 1, 2]
    ll, w, lpyl, pred = pc.inputs(rows, P, 5.0, 7000 + P)
    ll[1, 5], w[P - 2], ll[2, P - 2], pred[:, P - 2] = -np.inf, 0.0, np.nan, np.nan
    obs_off = np.concatenate([[0], np.cumsum(rows)])
    pop = pop_of(rows)
    d_ll, d_w, d_lpyl, d_pred = dev(ll), dev(w), dev(lpyl), dev(pred)
    q = runtime.posterior(pop, d_ll, d_w, d_lpyl).cpu().numpy()
    want_q = pc.np_q(ll, w, lpyl)
    assert np.isfinite(q).all() and np.max(np.abs(q - want_q) / pc.np_bar_q(ll, w, lpyl)) <= 2.0
    for mode in pc.MODES:
        rq = pc.row_q(mode, ll, w, lpyl, obs_off)
        assert pc.np_median_gap(pred, rq) >= 1e-9
        want_mean, want_median = pc.np_summary(pred, rq)
        mean, median = summarize(pop, mode, d_pred, d_w, d_ll, d_lpyl)
        torch.cuda.synchronize()
        bar = pc.np_bar_mean(pred, rq, pc.row_x(mode, ll, lpyl, obs_off))
        assert np.isfinite(want_mean).all()
        pc.assert_within(mean.cpu().numpy(), want_mean, bar, f"{mode} mean", bars=2.0)
        pc.assert_same_values(median.cpu().numpy(), want_median, f"{mode} median")


def test_negative_or_nan_weight_gives_nan_on_the_device():
    import torch

    case = next(c for c in CASES if (c["P"], c["S"]) == (63, 5))
    ll, w, lpyl, pred, _ = pc.case_inputs(case)
    pop = pop_of(case["rows"])
    for bad in (-0.25, float("nan")):
        w2 = w.copy()
        w2[17] = bad
        assert np.isnan(runtime.posterior(pop, dev(ll), w2, lpyl).cpu().numpy()).all()
        for mode in pc.MODES:
            mean, median = summarize(pop, mode, dev(pred), dev(w2), dev(ll), dev(lpyl))
            torch.cuda.synchronize()
            assert np.isnan(mean.cpu().numpy()).all() and np.isnan(median.cpu().numpy()).all()


ONE_PER_CLASS = [next(c for c in CASES if c["P"] == P and c["kind"] == kind)
                 for P, kind in ((64, "edges"), (130, "edges"), (1000, "edges"), (1025, "edges"), (4100, "edges"))]


@pytest.mark.parametrize("pitch", ["P+1", "recommended"])
@pytest.mark.parametrize("case", ONE_PER_CLASS, ids=pc.case_id)
def test_any_alignment_and_pitch_same_bits_and_nothing_else_written(case, pitch):
    """Every buffer carved from a dirty arena, 8 but not 16 bytes aligned, rows P + 1 resp. pmx_recommended_ld(P) doubles
    apart: the bits of the dense aligned run, not a byte outside what the caller owns - the padding columns of the
    posterior included -, the inputs untouched."""
    import torch

    L = _ffi.lib()
    S, P, n = case["S"], case["P"], sum(case["rows"])
    ll, w, lpyl, pred, _ = pc.case_inputs(case)
    pop = pop_of(case["rows"])
    d_ll, d_w, d_lpyl, d_pred = dev(ll), dev(w), dev(lpyl), dev(pred)
    dense_q = runtime.posterior(pop, d_ll, d_w, d_lpyl)
    dense = {mode: summarize(pop, mode, d_pred, d_w, d_ll, d_lpyl) for mode in pc.MODES}
    if "arena" not in STATE:
        STATE["arena"] = Arena("cuda", 16 << 20)
    arena = STATE["arena"]
    arena.reset()
    ld = P + 1 if pitch == "P+1" else runtime.recommended_ld(P)
    v_ll = arena.carve(S, P, ld, torch.float64, 8, name="ll")
    v_pred = arena.carve(n, P, ld, torch.float64, 8, name="pred")
    v_w = arena.carve(1, P, P, torch.float64, 8, name="w")
    v_lpyl = arena.carve(1, S, S, torch.float64, 8, name="lpyl")
    v_q = arena.carve(S, P, ld, torch.float64, 8, name="q")
    outs = {(mode, what): arena.carve(1, n, n, torch.float64, 8, name=f"{mode} {what}") for mode in pc.MODES
            for what in ("mean", "median")}
    for v in (v_ll, v_pred, v_w, v_lpyl, v_q, *outs.values()):
        assert v.data_ptr() % 16 == 8
    v_ll.copy_(d_ll)
    v_pred.copy_(d_pred)
    v_w.copy_(d_w.reshape(1, P))
    v_lpyl.copy_(d_lpyl.reshape(1, S))
    stream = torch.cuda.current_stream().cuda_stream
    _ffi.check(L.pmx_posterior_device(pop.handle, v_ll.data_ptr(), P, ld, v_w.data_ptr(), v_lpyl.data_ptr(), v_q.data_ptr(), ld, stream))
    for mode in pc.MODES:
        post = mode == "posterior"
        _ffi.check(L.pmx_summarize_predictions_device(
            pop.handle, v_pred.data_ptr(), P, ld, v_w.data_ptr(), v_ll.data_ptr() if post else None, ld if post else 0,
            v_lpyl.data_ptr() if post else None, outs[(mode, "mean")].data_ptr(), outs[(mode, "median")].data_ptr(), stream))
    torch.cuda.synchronize()
    assert bits(v_q.contiguous()) == bits(dense_q)
    for mode in pc.MODES:
        assert bits(outs[(mode, "mean")]) == bits(dense[mode][0]) and bits(outs[(mode, "median")]) == bits(dense[mode][1])
    arena.assert_clean()
    assert bits(v_ll.contiguous()) == bits(d_ll) and bits(v_pred.contiguous()) == bits(d_pred)
    assert bits(v_w) == bits(d_w) and bits(v_lpyl) == bits(d_lpyl)


# ---- end to end on a real population -----------------------------------------------------------------------------------
def weights(P):
    return ((np.arange(P) * 7919) % 1009 + 1.0) / (1009.0 * P)


def real_population(ragged):
    """9 subjects of the C3 schedule (protocol times: exact classes; `ragged`: jittered times, no two designs alike), with
    'measured' values: the device's own prediction at the first support point under a fixed multiplicative wobble"""
    key = ("real", ragged)
    if key not in STATE:
        import torch

        m, flat, theta = synth.model_two_cpt_iv(), synth.population_c23(9, ragged=ragged), synth.theta_c3(64)
        pred, _ = runtime.predict(m, runtime.DevicePopulation(flat, 0), theta[:1])
        torch.cuda.synchronize()
        p0 = pred.cpu().numpy()[:, 0]
        flat.ev_value = flat.ev_value.copy()
        flat.ev_value[flat.ev_kind == _abi.PMX_EV_OBSERVATION] = np.abs(p0) * np.exp(0.2 * np.sin(np.arange(p0.size))) + 0.05
        STATE[key] = (m, flat, theta)
    return STATE[key]


def device_sequence(m, flat, theta, w, subjects=None):
    """predict -> loglik -> mixture_loglik -> summarize_predictions, all on the device; everything as numpy"""
    import torch

    pop = runtime.DevicePopulation(flat, 0) if subjects is None else runtime.DevicePopulation(flat, 0, subjects=subjects)
    pred, st = runtime.predict(m, pop, theta)
    name = runtime.last_kernel_name()
    ll, _ = runtime.loglik(m, pop, EM_ADD, theta)
    lpyl = runtime.mixture_loglik(pop, ll, w)
    out = {"population": runtime.summarize_predictions(pop, pred, w), "posterior": runtime.summarize_predictions(pop, pred, w, ll, lpyl)}
    torch.cuda.synchronize()
    return pop, name, pred.cpu().numpy(), ll.cpu().numpy(), lpyl.cpu().numpy(), st.cpu().numpy(), \
        {k: (a.cpu().numpy(), b.cpu().numpy()) for k, (a, b) in out.items()}


def offsets_of(pop):
    off = np.zeros(pop.n_subjects + 1, dtype=np.int64)
    _ffi.check(_ffi.lib().pmx_population_observation_offsets(pop.handle, off.ctypes.data))
    return off


def host_form(m, flat, em, theta, w, want=(True, True), want_status=True):
    """pmx_summarize_predictions through the C ABI: (rc, mean, median, status)"""
    pop = runtime.DevicePopulation(flat, 0)
    theta, w = np.ascontiguousarray(theta, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    mean, median = np.full(pop.n_observations, -7.0), np.full(pop.n_observations, -7.0)
    status = np.full((pop.n_subjects, theta.shape[0]), 9, dtype=np.uint8)
    rc = _ffi.lib().pmx_summarize_predictions(
        runtime._as_model(m).handle, pop.handle, C.cast(em.to_c(m), C.c_void_p) if em is not None else None, theta.ctypes.data,
        theta.shape[0], w.ctypes.data, mean.ctypes.data if want[0] else None, median.ctypes.data if want[1] else None,
        status.ctypes.data if want_status else None)
    return rc, mean, median, status


@pytest.mark.parametrize("ragged,P,kernel", [(False, 64, "pmx_analytical_classed"), (True, 64, "pmx_analytical_steps"),
                                             (False, 4, "pmx_analytical_pair")], ids=["classes", "jittered", "pair"])
def test_end_to_end_device_sequence_and_host_form(ragged, P, kernel):
    m, flat, theta = real_population(ragged)
    theta, w = np.ascontiguousarray(theta[:P]), weights(P)
    pop, name, pred, ll, lpyl, st, out = device_sequence(m, flat, theta, w)
    assert name.startswith(kernel), name
    assert (st == 0).all() and np.isfinite(pred).all() and np.isfinite(ll).all()
    obs_off = offsets_of(pop)
    assert pop.n_subjects == 9 and pred.shape == (63, P)
    for mode in pc.MODES:
        rq = pc.row_q(mode, ll, w, lpyl, obs_off)
        want_mean, want_median = pc.np_summary(pred, rq)
        bar = pc.np_bar_mean(pred, rq, pc.row_x(mode, ll, lpyl, obs_off))
        worst = pc.assert_within(out[mode][0], want_mean, bar, f"{mode} mean", bars=2.0)
        print(f"{mode}: mean worst {worst:.3f} bars, median margin {pc.np_median_gap(pred, rq):.3g}")
        assert pc.np_median_gap(pred, rq) >= 1e-9  # (the inputs are fixed: no summation order moves these medians)
        pc.assert_same_values(out[mode][1], want_median, f"{mode} median")
        assert all((pred[i] == out[mode][1][i]).any() for i in range(pred.shape[0]))  # an element of its own row
        # the host form runs the same kernels on the same values: the same bits
        rc, mean, median, status = host_form(m, flat, EM_ADD if mode == "posterior" else None, theta, w)
        assert rc == _abi.PMX_OK and (status == 0).all()
        assert mean.tobytes() == out[mode][0].tobytes() and median.tobytes() == out[mode][1].tobytes()
    rc, mean, median, _ = host_form(m, flat, EM_ADD, theta, w, want=(False, True), want_status=False)
    assert rc == _abi.PMX_OK and (mean == -7.0).all() and median.tobytes() == out["posterior"][1].tobytes()


def test_host_form_failed_pair_poisons_only_where_it_has_weight():
    m, flat, theta = real_population(False)
    P, n = 12, 63
    th = np.ascontiguousarray(theta[:P]).copy()
    th[3, 1], th[3, 0], th[3, 2] = -3.0, 1.0, 1.0  # support point 3: complex eigenvalues
    w = weights(P)
    for em in (None, EM_ADD):
        rc, mean, median, status = host_form(m, flat, em, th, w)
        assert rc == _abi.PMX_ERR_PAIR_FAILED
        assert (status[:, 3] == _abi.PMX_PAIR_COMPLEX_ROOTS).all() and (np.delete(status, 3, axis=1) == 0).all()
        assert np.isnan(mean).all() and np.isnan(median).all()  # the point fails for every subject, and it has weight
        w0 = w.copy()
        w0[3] = 0.0
        rc, mean, median, status = host_form(m, flat, em, th, w0)
        assert rc == _abi.PMX_ERR_PAIR_FAILED and (status[:, 3] == _abi.PMX_PAIR_COMPLEX_ROOTS).all()
        assert np.isfinite(mean).all() and np.isfinite(median).all() and mean.shape == (n,)  # no weight: it poisons nobody
        rc2, mean2, median2, _ = host_form(m, flat, em, th, w0, want_status=False)
        assert rc2 == rc and mean2.tobytes() == mean.tobytes() and median2.tobytes() == median.tobytes()
    for bad in (-0.5, float("nan"), None):  # a negative weight, a NaN weight, no positive weight at all
        w2 = weights(P) if bad is not None else np.zeros(P)
        w2[5] = 0.0 if bad is None else bad
        rc, mean, median, _ = host_form(m, flat, EM_ADD, th, w2)
        assert rc == _abi.PMX_ERR_INVALID_ARGUMENT and (mean == -7.0).all() and (median == -7.0).all()


def test_rows_of_two_subject_shards_concatenate_bit_for_bit():
    m, flat, theta = real_population(True)
    w = weights(64)
    _, _, _, _, lpyl, _, whole = device_sequence(m, flat, theta, w)
    parts = [device_sequence(m, flat, theta, w, subjects=(s0, s1)) for s0, s1 in ((0, 4), (4, 9))]
    assert [p[0].n_subjects for p in parts] == [4, 5]
    assert np.concatenate([p[4] for p in parts]).tobytes() == lpyl.tobytes()
    for mode in pc.MODES:
        for k in (0, 1):
            assert np.concatenate([p[6][mode][k] for p in parts]).tobytes() == whole[mode][k].tobytes()
