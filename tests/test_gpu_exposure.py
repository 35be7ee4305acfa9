"""The exposure metrics and the target attainment (pmx_exposure.hip) on the device: the profile table; every case of
tests/golden/exposure_math.json within its bar with the selections equal, bit-identical from run to run, for any subset of
metrics and for any alignment and pitch, writing only what the caller owns; the row counts around the load pipeline's
depth and both sides of the attainment's wave / block switch; the attainment's weight edges; end to end on a real
population through the device sequence and through the host form; shards whose profiles concatenate."""
import ctypes as C

import numpy as np
import pytest

from pharmsol_amd import AssayErrorModel, AssayErrorModels, Data, ErrorPoly, Subject, _abi, _ffi, runtime, synth
from tests import exposure_cases as ec
from tests import models
from tests import posterior_cases as pc
from tests.arena import Arena

pytestmark = pytest.mark.gpu

EM_ADD = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.05, 0.1, 0.0, 0.0), 0.1))
STATE = {}
CASES = ec.doc()["cases"]
BITS = dict(zip(ec.METRICS, (1, 2, 4, 8, 16, 32)))
INF = float("inf")


def pop_of(lay_key="fixture", lay=None):
    """a device population with the observation times and output equations of a layout: the kernels take nothing else"""
    if lay_key not in STATE:
        lay = ec.layout() if lay is None else lay
        subs = []
        for i, occs in enumerate(lay):
            b = Subject.builder(str(i))
            for o, events in enumerate(occs):
                if o > 0:
                    b = b.reset()
                b = b.infusion(0.0, 300.0, 0, 0.25)
                for t, q in events:
                    b = b.observation(t, 5.0, q)
            subs.append(b.build())
        m = models.handwritten_analytical("two_compartments", 0, 4).with_ndrugs(1)
        STATE[lay_key] = runtime.DevicePopulation(m.flatten(Data(subs)), 0)
        assert STATE[lay_key].n_observations == ec.n_rows(lay)
    return STATE[lay_key]


def bits(t):
    return None if t is None else t.cpu().numpy().tobytes()


def dev(x):
    import torch

    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def run_case(pop, case, d_pred, metrics=ec.METRICS):
    return runtime.exposure(pop, d_pred, metrics=metrics, method=case["method"], window=ec.WINDOWS[case["window"]],
                            threshold=ec.THRESHOLD)


def test_profile_table_orders_subject_occasion_outeq():
    pop, table = pop_of(), ec.profile_table()
    assert pop.n_profiles == len(table) == 8
    s, o, q, n = pop.profiles()
    assert s.tolist() == [p["subject"] for p in table] and o.tolist() == [p["occasion"] for p in table]
    assert q.tolist() == [p["outeq"] for p in table] and n.tolist() == [len(p["rows"]) for p in table]
    # the rows and times behind it: what the population says of every prediction row
    t, oq, subj = pop.observation_info()
    for p in table:
        assert (t[p["rows"]] == p["times"]).all() and (oq[p["rows"]] == p["outeq"]).all() and (subj[p["rows"]] == p["subject"]).all()
    assert _ffi.lib().pmx_population_profile_info(pop.handle, None, None, None, None) == _abi.PMX_OK


@pytest.mark.parametrize("case", CASES, ids=ec.case_id)
def test_every_case_within_the_bar_selections_equal_and_bit_identical(case):
    import torch

    pred = ec.case_inputs(case)
    pop, d_pred = pop_of(), dev(pred)
    a = run_case(pop, case, d_pred)
    b = run_case(pop, case, d_pred)
    torch.cuda.synchronize()
    worst = ec.assert_planes({m: a[m].cpu().numpy() for m in ec.METRICS}, case, pred)
    print(f"{ec.case_id(case)}: worst share of a bar {worst:.3f}")
    assert all(bits(a[m]) == bits(b[m]) for m in ec.METRICS)
    assert a["auc"].data_ptr() + a["auc"].numel() * 8 == a["aumc"].data_ptr()  # views of one planes buffer


SUBSETS = [("auc",), ("cmax",), ("time_above",), ("auc", "cmax"), ("aumc", "tmax", "cmin"), ("tmax", "time_above"),
           ("auc", "aumc", "cmin", "time_above")]


@pytest.mark.parametrize("case", [c for c in CASES if c["P"] == 130], ids=ec.case_id)
def test_any_subset_of_metrics_gives_the_bits_of_the_full_set(case):
    import torch

    pop, d_pred = pop_of(), dev(ec.case_inputs(case))
    full = run_case(pop, case, d_pred)
    for subset in SUBSETS:
        got = run_case(pop, case, d_pred, metrics=subset)
        torch.cuda.synchronize()
        assert list(got) == list(subset)
        for m in subset:
            assert bits(got[m]) == bits(full[m]), (subset, m)
    # the raw call takes the bits in any combination: the planes come in bit order
    n, P = pop.n_profiles, case["P"]
    out = torch.full((2, n, P), -7.0, dtype=torch.float64, device="cuda")
    win = (C.c_double * 3)(*ec.WINDOWS[case["window"]], ec.THRESHOLD)
    _ffi.check(_ffi.lib().pmx_exposure_device(pop.handle, d_pred.data_ptr(), P, P, ec.METHODS.index(case["method"]), C.addressof(win),
                                              BITS["cmin"] | BITS["aumc"], out.data_ptr(), P, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bits(out[0]) == bits(full["aumc"]) and bits(out[1]) == bits(full["cmin"])


@pytest.mark.parametrize("P", [3, 64, 70, 257])
def test_row_counts_around_the_pipeline_depth_and_column_tiles(P):
    """The loads run four rows ahead: profiles of 1 to 9 rows sit on both sides of every fill state of that pipeline (the
    prologue's three conditional loads, the loop's first refill).  A wave owns 64 columns and a block four waves: 3, 64,
    70 and 257 columns are one partial tile, one full tile, two tiles and five (a block and a wave of the next).  There is
    no other switch: lin-log needs no second pass and keeps no rows (pmx_exposure.hip), so it has no register cut-off;
    the 32-bit quotient of the item index holds up to 2^32 work items and is not reached by a test.  Against the float64
    restatement: both sides sit within one bar of the truth."""
    import torch

    lay = [[[(float(k), 0) for k in range(n)]] for n in range(1, 10)]
    pop, table = pop_of("rows-1-9", lay), ec.profile_table(lay)
    assert pop.profiles()[3].tolist() == list(range(1, 10))
    i = np.arange(ec.n_rows(lay), dtype=np.int64)[:, None]
    p = np.arange(P, dtype=np.int64)[None, :]
    pred = 0.25 + 12.0 * (((i * 2654435761 + p * 40503 + P) % 1000003).astype(np.float64) / 1000003.0)
    d_pred = dev(pred)
    for method in ec.METHODS:
        for a, b in ((-INF, INF), (1.25, 6.5)):
            want, ok = ec.np_exposure(pred, a, b, method, 6.0, table)
            assert ok.all()
            got = runtime.exposure(pop, d_pred, metrics=ec.METRICS, method=method, window=(a, b), threshold=6.0)
            torch.cuda.synchronize()
            for m in ec.METRICS:
                ec.assert_values(got[m].cpu().numpy(), want[m][0], want[m][1], f"{method} [{a}, {b}] {m}", bars=2.0)


ARENA_CASES = [next(c for c in CASES if c["P"] == P and c["method"] == "lin_log" and c["window"] == "cuts") for P in (63, 64, 130, 1000)]


@pytest.mark.parametrize("pitch", ["P+1", "recommended"])
@pytest.mark.parametrize("case", ARENA_CASES, ids=ec.case_id)
def test_any_alignment_and_pitch_same_bits_and_nothing_else_written(case, pitch):
    """Every buffer carved from a dirty arena, 8 but not 16 bytes aligned, rows P + 1 resp. pmx_recommended_ld(P) doubles
    apart: the bits of the dense aligned run, not a byte outside what the caller owns - the padding columns of the planes
    included -, the inputs untouched."""
    import torch

    L = _ffi.lib()
    pop = pop_of()
    n, P, n_obs = pop.n_profiles, case["P"], pop.n_observations
    pred = ec.case_inputs(case)
    w = ec.weights(P)
    ll, _, lpyl, _ = pc.inputs([1] * pop.n_subjects, P, 5.0, 4000 + P)
    d_pred, d_w, d_ll, d_lpyl = dev(pred), dev(w), dev(ll), dev(lpyl)
    dense = run_case(pop, case, d_pred)
    target = dev(np.nanmedian(np.where(np.isnan(dense["auc"].cpu().numpy()), 1.0, dense["auc"].cpu().numpy()), axis=1))
    dense_att = {mode: runtime.target_attainment(pop, dense["auc"], d_w, target, *((d_ll, d_lpyl) if mode == "posterior" else ()), mean=True)
                 for mode in pc.MODES}
    if "arena" not in STATE:
        STATE["arena"] = Arena("cuda", 16 << 20)
    arena = STATE["arena"]
    arena.reset()
    ld = P + 1 if pitch == "P+1" else runtime.recommended_ld(P)
    v_pred = arena.carve(n_obs, P, ld, torch.float64, 8, name="pred")
    v_out = arena.carve(6 * n, P, ld, torch.float64, 8, name="planes")
    v_w = arena.carve(1, P, P, torch.float64, 8, name="w")
    v_ll = arena.carve(pop.n_subjects, P, ld, torch.float64, 8, name="ll")
    v_lpyl = arena.carve(1, pop.n_subjects, pop.n_subjects, torch.float64, 8, name="lpyl")
    v_target = arena.carve(1, n, n, torch.float64, 8, name="target")
    outs = {(mode, what): arena.carve(1, n, n, torch.float64, 8, name=f"{mode} {what}") for mode in pc.MODES for what in ("pta", "mean")}
    for v in (v_pred, v_out, v_w, v_ll, v_lpyl, v_target, *outs.values()):
        assert v.data_ptr() % 16 == 8
    v_pred.copy_(d_pred)
    v_w.copy_(d_w.reshape(1, P))
    v_ll.copy_(d_ll)
    v_lpyl.copy_(d_lpyl.reshape(1, -1))
    v_target.copy_(target.reshape(1, n))
    stream = torch.cuda.current_stream().cuda_stream
    win = (C.c_double * 3)(*ec.WINDOWS[case["window"]], ec.THRESHOLD)
    _ffi.check(L.pmx_exposure_device(pop.handle, v_pred.data_ptr(), P, ld, ec.METHODS.index(case["method"]), C.addressof(win), 63,
                                     v_out.data_ptr(), ld, stream))
    for mode in pc.MODES:
        post = mode == "posterior"
        _ffi.check(L.pmx_attainment_device(pop.handle, v_out.data_ptr(), P, ld, v_target.data_ptr(), v_w.data_ptr(),
                                           v_ll.data_ptr() if post else None, ld if post else 0, v_lpyl.data_ptr() if post else None,
                                           outs[(mode, "pta")].data_ptr(), outs[(mode, "mean")].data_ptr(), stream))
    torch.cuda.synchronize()
    for k, m in enumerate(ec.METRICS):
        assert bits(v_out[k * n:(k + 1) * n].contiguous()) == bits(dense[m]), m
    for mode in pc.MODES:
        assert bits(outs[(mode, "pta")]) == bits(dense_att[mode][0]) and bits(outs[(mode, "mean")]) == bits(dense_att[mode][1])
    arena.assert_clean()
    assert bits(v_pred.contiguous()) == bits(d_pred) and bits(v_w) == bits(d_w) and bits(v_ll.contiguous()) == bits(d_ll)
    assert bits(v_lpyl) == bits(d_lpyl) and bits(v_target) == bits(target)


# ---- attainment ----------------------------------------------------------------------------------------------------------
def attain(pop, mode, d_plane, d_w, d_target, d_ll, d_lpyl, mean=True):
    if mode == "population":
        return runtime.target_attainment(pop, d_plane, d_w, d_target, mean=mean)
    return runtime.target_attainment(pop, d_plane, d_w, d_target, d_ll, d_lpyl, mean=mean)


def check_attainment(pop, plane, w, ll, lpyl, target, table=None):
    """both modes against the restatement within two bars, twice with the same bits; returns the outputs"""
    import torch

    d_plane, d_w, d_ll, d_lpyl, d_target = dev(plane), dev(w), dev(ll), dev(lpyl), dev(target)
    out = {}
    for mode in pc.MODES:
        q, x = ec.profile_q(mode, ll, w, lpyl, table)
        want_pta, want_mean = ec.np_attainment(plane, q, target)
        pta, mean = attain(pop, mode, d_plane, d_w, d_target, d_ll, d_lpyl)
        pta2, mean2 = attain(pop, mode, d_plane, d_w, d_target, d_ll, d_lpyl)
        only_pta, none = attain(pop, mode, d_plane, d_w, d_target, d_ll, d_lpyl, mean=False)
        torch.cuda.synchronize()
        assert none is None and bits(only_pta) == bits(pta) and bits(pta2) == bits(pta) and bits(mean2) == bits(mean)
        fin = np.isfinite(want_pta)
        with np.errstate(all="ignore"):
            bar_pta = np.where(fin, ec.np_bar_pta(q, x), 1.0)
            bar_mean = np.where(fin, pc.np_bar_mean(np.where(np.isnan(plane), 0.0, plane), q, x), 1.0)
        ec.assert_values(pta.cpu().numpy(), want_pta, bar_pta, f"{mode} pta", bars=2.0)
        ec.assert_values(mean.cpu().numpy(), want_mean, bar_mean, f"{mode} mean", bars=2.0)
        out[mode] = (pta.cpu().numpy(), mean.cpu().numpy(), want_pta)
    return out


@pytest.mark.parametrize("case", [c for c in CASES if c["window"] == "whole" and c["method"] == "linear"], ids=ec.case_id)
def test_attainment_on_the_fixture_s_planes_and_its_weight_edges(case):
    """The planes of a case with a NaN cell and a failed pair, as inputs.  A column of weight 0 is skipped whatever it
    holds; a NaN metric under weight poisons its profile only; a failed pair under weight - a NaN q - every profile of
    its subject and no other subject's; a negative or NaN weight everything; a profile whose q are all 0 gives NaN."""
    import torch

    P, pop, table = case["P"], pop_of(), ec.profile_table()
    pred = ec.case_inputs(case)
    planes, _ = ec.case_exposure(case, pred)
    plane = planes["cmax"][0]  # (finite wherever the profile is: the NaN cell and the failed pair are its only NaNs)
    w = ec.weights(P)
    ll, _, lpyl, _ = pc.inputs([1] * pop.n_subjects, P, 5.0, 4100 + P)
    target = np.asarray([np.median(r[~np.isnan(r)]) if (~np.isnan(r)).any() else 1.0 for r in plane])
    nan_profiles = np.isnan(plane).any(axis=1)
    out = check_attainment(pop, plane, w, ll, lpyl, target)
    for mode in pc.MODES:
        assert (np.isnan(out[mode][0]) == nan_profiles).all() and (np.isnan(out[mode][1]) == nan_profiles).all()
        fin = out[mode][0][~nan_profiles]
        assert ((fin >= 0.0) & (fin <= 1.0)).all()
    if P > 1:
        assert nan_profiles.tolist() == [True, False, True, True, True, False, False, False]
    # weight 0 on the NaN columns: nothing is poisoned
    w0 = w.copy()
    w0[np.isnan(plane).any(axis=0)] = 0.0
    if (w0 > 0.0).any():
        out = check_attainment(pop, plane, w0, ll, lpyl, target)
        assert all(np.isfinite(out[mode][k]).all() for mode in pc.MODES for k in (0, 1))
    # a failed pair of subject 1 in the log-likelihood (NaN q): its profiles, in posterior mode, and no other subject's
    if P > 2:
        ll2 = ll.copy()
        ll2[1, 0] = np.nan
        out = check_attainment(pop, np.where(np.isnan(plane), 2.0, plane), w, ll2, lpyl, target)
        s1 = np.asarray([p["subject"] == 1 for p in table])
        assert (np.isnan(out["posterior"][0]) == s1).all() and np.isfinite(out["population"][0]).all()
        # -inf everywhere but one column for subject 3: q is 0 there; everywhere: a profile whose q are all 0
        ll3 = ll.copy()
        ll3[3, :] = -np.inf
        out = check_attainment(pop, np.where(np.isnan(plane), 2.0, plane), w, ll3, lpyl, target)
        s3 = np.asarray([p["subject"] == 3 for p in table])
        assert (np.isnan(out["posterior"][0]) == s3).all()
    # a negative or NaN weight: NaN everywhere
    for bad in (-0.25, float("nan")):
        w2 = w.copy()
        w2[P // 3] = bad
        for mode in pc.MODES:
            pta, mean = attain(pop, mode, dev(plane), dev(w2), dev(target), dev(ll), dev(lpyl))
            torch.cuda.synchronize()
            assert np.isnan(pta.cpu().numpy()).all() and np.isnan(mean.cpu().numpy()).all()


@pytest.mark.parametrize("P", [1024, 1025])
def test_attainment_on_both_sides_of_the_wave_block_switch(P):
    """a wave owns a profile's row up to 1024 columns (kAttainWaveMax), a block of four beyond"""
    pop, n = pop_of(), pop_of().n_profiles
    k = np.arange(n, dtype=np.int64)[:, None]
    p = np.arange(P, dtype=np.int64)[None, :]
    plane = -3.0 + 20.0 * (((k * 2246822519 + p * 3266489917 + P) % 1000033).astype(np.float64) / 1000033.0)
    plane[2, P - 1] = np.nan
    w = ec.weights(P)
    w[5] = 0.0
    ll, _, lpyl, _ = pc.inputs([1] * pop.n_subjects, P, 5.0, 4200 + P)
    ll[0, 7] = -np.inf
    out = check_attainment(pop, plane, w, ll, lpyl, np.full(n, 7.0))
    assert np.isnan(out["population"][0]).tolist() == [False, False, True] + [False] * (n - 3)


# ---- end to end on a real population -----------------------------------------------------------------------------------
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


def table_of(pop):
    """the profile table of a population with one output equation and one occasion per subject, from what it reports"""
    s, o, q, n = pop.profiles()
    assert (q == 0).all() and (o == 0).all() and s.tolist() == list(range(pop.n_subjects))
    t, _, _ = pop.observation_info()
    off = np.concatenate([[0], np.cumsum(n)])
    return [dict(subject=int(s[k]), occasion=0, outeq=0, rows=np.arange(off[k], off[k + 1]), times=t[off[k]:off[k + 1]]) for k in range(len(s))]


E2E = dict(method="lin_up_log_down", window=(0.75, 20.0), threshold=2.0, metric="auc")


def device_sequence(m, flat, theta, w, target, subjects=None):
    """predict -> loglik -> mixture_loglik -> exposure -> target_attainment, all on the device; everything as numpy"""
    import torch

    pop = runtime.DevicePopulation(flat, 0) if subjects is None else runtime.DevicePopulation(flat, 0, subjects=subjects)
    pred, st = runtime.predict(m, pop, theta)
    ll, _ = runtime.loglik(m, pop, EM_ADD, theta)
    lpyl = runtime.mixture_loglik(pop, ll, w)
    planes = runtime.exposure(pop, pred, metrics=ec.METRICS, method=E2E["method"], window=E2E["window"], threshold=E2E["threshold"])
    tg = dev(target if subjects is None else target[subjects[0]:subjects[1]])
    out = {"population": runtime.target_attainment(pop, planes[E2E["metric"]], w, tg, mean=True),
           "posterior": runtime.target_attainment(pop, planes[E2E["metric"]], w, tg, ll, lpyl, mean=True)}
    torch.cuda.synchronize()
    return pop, pred.cpu().numpy(), ll.cpu().numpy(), lpyl.cpu().numpy(), st.cpu().numpy(), \
        {k: v.cpu().numpy() for k, v in planes.items()}, {k: (a.cpu().numpy(), b.cpu().numpy()) for k, (a, b) in out.items()}


def host_form(m, flat, em, theta, w, target, want=(True, True), want_status=True, metric=1):
    """pmx_exposure_attainment through the C ABI: (rc, pta, mean, status)"""
    pop = runtime.DevicePopulation(flat, 0)
    theta, w = np.ascontiguousarray(theta, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    n = pop.n_profiles
    pta, mean = np.full(n, -7.0), np.full(n, -7.0)
    target = np.ascontiguousarray(target, dtype=np.float64)
    status = np.full((pop.n_subjects, theta.shape[0]), 9, dtype=np.uint8)
    win = (C.c_double * 3)(E2E["window"][0], E2E["window"][1], E2E["threshold"])
    rc = _ffi.lib().pmx_exposure_attainment(
        runtime._as_model(m).handle, pop.handle, C.cast(em.to_c(m), C.c_void_p) if em is not None else None, theta.ctypes.data,
        theta.shape[0], w.ctypes.data, ec.METHODS.index(E2E["method"]), C.addressof(win), metric,
        target.ctypes.data if want[0] else None, pta.ctypes.data if want[0] else None, mean.ctypes.data if want[1] else None,
        status.ctypes.data if want_status else None)
    return rc, pta, mean, status


@pytest.mark.parametrize("ragged", [False, True], ids=["classes", "jittered"])
def test_end_to_end_device_sequence_and_host_form(ragged):
    m, flat, theta = real_population(ragged)
    P = 64
    theta, w = np.ascontiguousarray(theta[:P]), ec.weights(P)
    target = 40.0 + 5.0 * np.arange(9)
    pop, pred, ll, lpyl, st, planes, out = device_sequence(m, flat, theta, w, target)
    assert (st == 0).all() and np.isfinite(pred).all() and np.isfinite(ll).all() and pop.n_profiles == 9
    table = table_of(pop)
    # the restatement applied to the device's own pred
    want, ok = ec.np_exposure(pred, *E2E["window"], E2E["method"], E2E["threshold"], table)
    assert ok.all()
    for name in ec.METRICS:
        assert np.isfinite(planes[name]).all()
        ec.assert_values(planes[name], want[name][0], want[name][1], name, bars=2.0)
    plane = planes[E2E["metric"]]
    target = np.median(plane, axis=1)  # (a target in the middle of every profile's own values)
    pop, pred, ll, lpyl, st, planes, out = device_sequence(m, flat, theta, w, target)
    for mode in pc.MODES:
        q, x = ec.profile_q(mode, ll, w, lpyl, table)
        want_pta, want_mean = ec.np_attainment(plane, q, target)
        assert (out[mode][0] >= 0.0).all() and (out[mode][0] <= 1.0).all()  # (the device's two sums share their order)
        if mode == "population":  # (the posterior may sit on one side of the target altogether)
            assert ((want_pta > 0.0) & (want_pta < 1.0)).all()
        ec.assert_values(out[mode][0], want_pta, ec.np_bar_pta(q, x), f"{mode} pta", bars=2.0)
        ec.assert_values(out[mode][1], want_mean, pc.np_bar_mean(plane, q, x), f"{mode} mean", bars=2.0)
        # the host form runs the same kernels on the same values: the same bits
        rc, pta, mean, status = host_form(m, flat, EM_ADD if mode == "posterior" else None, theta, w, target)
        assert rc == _abi.PMX_OK and (status == 0).all()
        assert pta.tobytes() == out[mode][0].tobytes() and mean.tobytes() == out[mode][1].tobytes()
    rc, pta, mean, _ = host_form(m, flat, EM_ADD, theta, w, target, want=(False, True), want_status=False)
    assert rc == _abi.PMX_OK and (pta == -7.0).all() and mean.tobytes() == out["posterior"][1].tobytes()


def test_host_form_failed_pair_poisons_only_where_it_has_weight():
    m, flat, theta = real_population(False)
    P, n = 12, 9
    th = np.ascontiguousarray(theta[:P]).copy()
    th[3, 1], th[3, 0], th[3, 2] = -3.0, 1.0, 1.0  # support point 3: complex eigenvalues
    w = ec.weights(P)
    target = np.full(n, 50.0)
    for em in (None, EM_ADD):
        rc, pta, mean, status = host_form(m, flat, em, th, w, target)
        assert rc == _abi.PMX_ERR_PAIR_FAILED
        assert (status[:, 3] == _abi.PMX_PAIR_COMPLEX_ROOTS).all() and (np.delete(status, 3, axis=1) == 0).all()
        assert np.isnan(pta).all() and np.isnan(mean).all()  # the point fails for every subject, and it has weight
        w0 = w.copy()
        w0[3] = 0.0
        rc, pta, mean, status = host_form(m, flat, em, th, w0, target)
        assert rc == _abi.PMX_ERR_PAIR_FAILED and (status[:, 3] == _abi.PMX_PAIR_COMPLEX_ROOTS).all()
        assert np.isfinite(pta).all() and np.isfinite(mean).all() and pta.shape == (n,)  # no weight: it poisons nobody
        rc2, pta2, mean2, _ = host_form(m, flat, em, th, w0, target, want_status=False)
        assert rc2 == rc and pta2.tobytes() == pta.tobytes() and mean2.tobytes() == mean.tobytes()
    for bad in (-0.5, float("nan"), None):  # a negative weight, a NaN weight, no positive weight at all
        w2 = ec.weights(P) if bad is not None else np.zeros(P)
        w2[5] = 0.0 if bad is None else bad
        rc, pta, mean, _ = host_form(m, flat, EM_ADD, th, w2, target)
        assert rc == _abi.PMX_ERR_INVALID_ARGUMENT and (pta == -7.0).all() and (mean == -7.0).all()


def test_profiles_of_two_subject_shards_concatenate_bit_for_bit():
    m, flat, theta = real_population(True)
    w = ec.weights(64)
    target = 40.0 + 5.0 * np.arange(9)
    whole = device_sequence(m, flat, theta, w, target)
    parts = [device_sequence(m, flat, theta, w, target, subjects=(s0, s1)) for s0, s1 in ((0, 4), (4, 9))]
    assert [p[0].n_profiles for p in parts] == [4, 5]
    for name in ec.METRICS:
        assert np.concatenate([p[5][name] for p in parts]).tobytes() == whole[5][name].tobytes()
    for mode in pc.MODES:
        for k in (0, 1):
            assert np.concatenate([p[6][mode][k] for p in parts]).tobytes() == whole[6][mode][k].tobytes()
