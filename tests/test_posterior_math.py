"""The posterior and the prediction summaries, as far as they go without a GPU: the fixture
tests/golden/posterior_math.json (50-digit truths with derived bars, tests/golden/gen_posterior_math.py) against the
inputs and the float64 restatement the GPU tests use - the check that the bars are attainable - and the argument checks
of the three new entry points, which are decided before a device is touched."""
import ctypes as C

import numpy as np
import pytest

from pharmsol_amd import _abi, _ffi
from tests import posterior_cases as pc

NEW_SYMBOLS = ["pmx_posterior_device", "pmx_summarize_predictions_device", "pmx_summarize_predictions"]
PS = {1, 2, 63, 64, 65, 130, 1000, 1024, 1025, 4100}


def test_fixture_covers_the_shapes_scales_and_edges():
    cases = pc.doc()["cases"]
    assert {c["P"] for c in cases} == PS
    assert {c["scale"] for c in cases} == {5.0, 300.0, 1.0e4} and {c["S"] for c in cases} == {1, 5, 9}
    assert {c["kind"] for c in cases} == {"plain", "edges", "heavy", "two"}
    for P in PS - {4100}:
        mine = [c for c in cases if c["P"] == P]
        assert {9, 5} <= {c["S"] for c in mine} and any(c["kind"] == "edges" and c["scale"] == 300.0 for c in mine)
    wide = [c for c in cases if c["P"] == 4100]
    assert len(wide) == 1 and wide[0]["rows"] == [3]
    nine = next(c for c in cases if c["S"] == 9)
    assert {1, 2, 7, 40} <= set(nine["rows"])  # every row count in one population
    q = np.concatenate([c["q"].ravel() for c in cases])
    assert np.isnan(q).any() and (q == 0.0).any()
    for mode in pc.MODES:
        mean = np.concatenate([c[mode]["mean"] for c in cases])
        median = np.concatenate([c[mode]["median"] for c in cases])
        assert np.isnan(mean).any() and np.isfinite(mean).any() and (median < 0.0).any() and (median > 0.0).any()


@pytest.mark.parametrize("case", pc.doc()["cases"], ids=pc.case_id)
def test_inputs_and_float64_restatement(case):
    ll, w, lpyl, pred, obs_off = pc.case_inputs(case)
    assert pc.checksum(ll, w, lpyl, pred) == case["checksum"]
    assert pred.shape == (sum(case["rows"]), case["P"])
    pc.assert_q(pc.np_q(ll, w, lpyl), case, ll, w, lpyl)
    for mode in pc.MODES:
        rq, x = pc.row_q(mode, ll, w, lpyl, obs_off), pc.row_x(mode, ll, lpyl, obs_off)
        mean, median = pc.np_summary(pred, rq)
        pc.assert_summary(mean, median, case, mode, pred, rq, x)
        assert pc.np_median_gap(pred, rq) >= 0.99e-9  # every row, stored or not (1e-9 in 50 digits; float64 here)
        # the bar the GPU tests derive from float64 values is the stored one (the stored one is rounded to float32)
        bar64, fin = pc.np_bar_mean(pred, rq, x)[case["kept"]], np.isfinite(case[mode]["mean"])
        np.testing.assert_allclose(bar64[fin], case[mode]["mean_bar"][fin], rtol=1e-6)
    if case["scale"] >= 300.0:  # the unshifted formula underflows everywhere: 0 / 0
        with np.errstate(all="ignore"):
            t = w * np.exp(np.where(np.isnan(ll), -np.inf, ll))
            assert (t.sum(axis=1) == 0.0).all()


def test_the_three_symbols_are_exported_and_bound():
    L = C.CDLL(_ffi.LIB_PATH)
    bound = {n for n, _, _ in _ffi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in bound, name
    assert _ffi.lib().pmx_abi_version() == 3  # additive: the version stays


def test_argument_faults_are_refused_without_a_device():
    """Argument checks come before anything touches a device, so they are the same on a machine without one.  The
    handles are never dereferenced on these paths: any non-null address stands in for them."""
    L = _ffi.lib()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    INV = _abi.PMX_ERR_INVALID_ARGUMENT
    post = L.pmx_posterior_device            # pop, d_ll, n, ld_ll, d_w, d_lpyl, d_post, ld_post, stream
    summ = L.pmx_summarize_predictions_device  # pop, d_pred, n, ld_pred, d_w, d_ll, ld_ll, d_lpyl, d_mean, d_median, stream
    host = L.pmx_summarize_predictions       # model, pop, em, theta, n, w, mean, median, status
    wbuf = (C.c_double * 2)(0.25, 0.75)
    wa = C.addressof(wbuf)
    good_post = [a, a, 2, 2, a, a, a, 2, None]
    good_summ = [a, a, 2, 2, a, a, 2, a, a, a, None]
    good_host = [a, a, a, a, 2, wa, a, a, None]
    for fn, good, pointers, n_at in ((post, good_post, (0, 1, 4, 5, 6), 2), (summ, good_summ, (0, 1, 4), 2),
                                     (host, good_host, (0, 1, 3, 5), 4)):
        for i in pointers:
            args = list(good)
            args[i] = None
            assert fn(*args) == INV and L.pmx_last_error() == b"null argument"
        for n in (0, -3):
            args = list(good)
            args[n_at] = n
            assert fn(*args) == INV and b"n_support" in L.pmx_last_error()
        args = list(good)
        args[0], args[n_at] = None, 0
        assert fn(*args) == INV and L.pmx_last_error() == b"null argument"  # nulls are looked at first
    # pitches below n_support
    for fn, good, at, word in ((post, good_post, 3, b"ld_ll"), (post, good_post, 7, b"ld_post"), (summ, good_summ, 3, b"ld_pred"),
                               (summ, good_summ, 6, b"ld_ll")):
        args = list(good)
        args[at] = 1
        assert fn(*args) == INV and word in L.pmx_last_error()
    # both outputs null
    args = list(good_summ)
    args[8] = args[9] = None
    assert summ(*args) == INV and b"both null" in L.pmx_last_error()
    args = list(good_host)
    args[6] = args[7] = None
    assert host(*args) == INV and b"both null" in L.pmx_last_error()
    # d_ll without d_lpyl, and the reverse
    for gone in (5, 7):
        args = list(good_summ)
        args[gone] = None
        assert summ(*args) == INV and b"go together" in L.pmx_last_error()
    # the host form's weights are on the host: checked before any work
    for w in ([0.5, -0.5], [0.5, float("nan")], [0.0, 0.0]):
        bad = (C.c_double * 2)(*w)
        assert host(a, a, a, a, 2, C.addressof(bad), a, a, None) == INV
        assert b"w" in L.pmx_last_error()
    assert host(a, a, None, a, 2, C.addressof((C.c_double * 2)(0.5, -0.5)), a, a, None) == INV  # population mode too
