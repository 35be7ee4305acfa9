"""The exposure metrics and the target attainment, as far as they go without a GPU: the fixture
tests/golden/exposure_math.json (40-digit truths with derived bars, tests/golden/gen_exposure_math.py) against the inputs
and the float64 restatement the GPU tests use - the check that the bars are attainable -, the reference's own known
answers through that restatement, and the argument checks of the three new entry points, which are decided before a
device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

from pharmsol_amd import _abi, _ffi
from tests import exposure_cases as ec

NEW_SYMBOLS = ["pmx_population_n_profiles", "pmx_population_profile_info", "pmx_exposure_device", "pmx_attainment_device",
               "pmx_exposure_attainment"]
PS = {1, 2, 63, 64, 65, 130, 1000}
INF, NAN = float("inf"), float("nan")


def one(times, concs, a=-INF, b=INF, method="linear", thr=1.0):
    out, ok = ec.np_profile(times, np.asarray(concs, dtype=np.float64)[:, None], a, b, method, thr)
    assert ok.all()
    return {m: float(v[0][0]) for m, v in out.items()}


def test_fixture_covers_the_shapes_windows_and_edges():
    cases = ec.doc()["cases"]
    assert {c["P"] for c in cases} == PS
    table = ec.profile_table()
    assert {1, 2, 3, 7, 40} <= {len(p["rows"]) for p in table}  # every profile length in one population
    s0 = [p for p in table if p["subject"] == 0]
    assert [p["outeq"] for p in s0] == [0, 1] and s0[1]["rows"].min() < s0[0]["rows"].max()  # two outputs, interleaved
    s1 = [p for p in table if p["subject"] == 1]
    assert {p["occasion"] for p in s1} == {0, 1} and s1[1]["times"][0] < s1[0]["times"][-1]  # the second occasion's clock restarts
    assert {p["outeq"] for p in table if p["subject"] == 2} == {0}  # a subject that lacks an output equation
    assert any((np.diff(p["times"]) == 0.0).any() for p in table)  # a duplicate time
    for P in PS:
        mine = [c for c in cases if c["P"] == P]
        assert {c["method"] for c in mine} == set(ec.METHODS) and any(c["edits"] for c in mine)
        assert {"whole", "cuts", "points"} <= {c["window"] for c in mine}
    for P in (64, 1000):
        assert {c["window"] for c in cases if c["P"] == P} == set(ec.WINDOWS)
        assert {(c["method"], c["window"]) for c in cases if c["P"] == P} >= {(m, w) for m in ec.METHODS for w in ("whole", "cuts")}
    # the rise-and-fall profile: zeros before the dose, a plateau, a ratio on each side of 1e-10
    c = np.asarray(ec.SPECIAL_C)
    assert c[0] == c[1] == 0.0 and (c[1:-1] == c[2:]).sum() == 1 and c.argmax() == 3 and (np.diff(c[4:]) < 0).all()
    ratios = c[5:7] / c[6:8] - 1.0
    assert 1e-10 < ratios[0] < 3e-10 and 0.0 < ratios[1] < 1e-10
    assert ec.THRESHOLD in c  # a threshold equal to a data value
    auc = np.concatenate([k["auc"]["value"].ravel() for k in cases])
    assert np.isnan(auc).any() and np.isfinite(auc).any()
    one_point = next(k for k in cases if k["window"] == "one" and k["P"] == 64)
    assert np.isnan(one_point["auc"]["value"]).all() and np.isfinite(one_point["cmax"]["value"]).any()
    assert all(np.isnan(k[m]["value"]).all() for k in cases if k["window"] in ("miss", "before") for m in ec.METRICS)


@pytest.mark.parametrize("case", ec.doc()["cases"], ids=ec.case_id)
def test_inputs_and_float64_restatement(case):
    pred = ec.case_inputs(case)
    assert ec.checksum(pred) == case["checksum"] and pred.shape == (ec.n_rows(), case["P"])
    got, ok = ec.case_exposure(case, pred)
    assert ok.all()
    worst = ec.assert_planes({m: got[m][0] for m in ec.METRICS}, case, pred)
    assert worst <= 1.0
    # the bar the GPU tests derive from float64 values is the stored one (the stored one is rounded to float32)
    for m in ec.METRICS:
        np.testing.assert_allclose(got[m][1][:, case["cols"]], case[m]["bar"], rtol=1e-6, atol=0.0)
    # a NaN poisons its own (profile, column) only: the failed pair every profile of its subject, no other subject's
    for e in case["edits"]:
        col = e["cell"][1] if "cell" in e else e["pair"][1]
        hit = {0} if "cell" in e else {p for p, prof in enumerate(ec.profile_table()) if prof["subject"] == e["pair"][0]}
        for p in range(len(ec.profile_table())):
            if p in hit:
                assert all(np.isnan(got[m][0][p, col]) for m in ec.METRICS)
            elif case["window"] == "whole" and len(ec.profile_table()[p]["rows"]) > 0:
                assert np.isfinite(got["cmax"][0][p, col])


def test_the_reference_s_own_known_answers():
    """data/auc.rs (its doc tests and unit tests) and nca/calc.rs:843-880, through the restatement"""
    assert one([0, 1, 2, 4], [0, 10, 8, 4])["auc"] == 26.0
    long_t, long_c = [0, 1, 2, 4, 8, 12], [0, 10, 8, 4, 2, 1]
    assert one(long_t, long_c)["auc"] == 44.0
    assert 0.0 < one(long_t, long_c, method="lin_up_log_down")["auc"] < 44.0
    assert one([0, 1, 2, 4, 8], [0, 10, 8, 4, 2], 1.0, 4.0)["auc"] == 21.0
    assert one([0, 2, 4], [0, 10, 6], 1.0, 3.0)["auc"] == 16.5
    assert one([0, 1, 2], [0, 10, 8])["aumc"] == 18.0
    assert abs(one([0, 1], [10, 5], method="lin_up_log_down")["auc"] - 5.0 / math.log(2.0)) < 1e-14
    assert one([0, 1], [5, 10], method="lin_up_log_down")["auc"] == 7.5  # ascending: linear
    assert one([0, 1, 2, 4], [0, 10, 8, 4])["tmax"] == 1.0  # first occurrence
    assert one([0, 1, 2, 4], [0, 10, 10, 4])["tmax"] == 1.0
    # lin-log: linear up to tmax, log after it
    lin_log = one([0, 1, 2], [0, 10, 8], method="lin_log")["auc"]
    assert abs(lin_log - (5.0 + 2.0 / math.log(10.0 / 8.0))) < 1e-14
    # nca/calc.rs:843-880
    assert one([0, 1, 2, 4], [10, 8, 6, 5], thr=1.0)["time_above"] == 4.0
    assert one([0, 1, 2], [0.5, 0.3, 0.1], thr=1.0)["time_above"] == 0.0
    assert abs(one([0, 1, 2], [10, 5, 0], thr=4.0)["time_above"] - 1.2) < 1e-14
    assert one([0, 1, 2], [0, 10, 10], thr=5.0)["time_above"] == 1.5
    assert math.isnan(one([1.0], [5.0], thr=1.0)["time_above"])
    # a zero-length pair: InvalidTimeSequence
    assert math.isnan(one([1, 1], [10, 8])["auc"]) and one([1, 1], [10, 8])["cmax"] == 10.0
    # a profile of zeros has AUC 0: nothing is truncated
    assert one([0, 1, 2], [0, 0, 0])["auc"] == 0.0


def test_windows_outside_the_data():
    """auc_interval answers 0.0 for a window that misses the data (auc.rs:486-501).  Here such a window leaves no point
    in the clipped profile, and the rule for that is NaN for every metric (include/pmx.h): a caller can tell an exposure
    of zero from a profile the window does not reach.  The fixture holds the same (windows "miss" and "before")."""
    for a, b in ((0.0, 0.5), (5.0, 10.0)):
        got = one([1, 2, 4], [10, 8, 4], a, b)
        assert all(math.isnan(v) for v in got.values())
    # one end in, a window that holds one point: the extremes exist, the integrals do not
    got = one([1, 2, 4], [10, 8, 4], 4.0, 10.0)
    assert got["cmax"] == got["cmin"] == 4.0 and got["tmax"] == 4.0 and math.isnan(got["auc"]) and math.isnan(got["time_above"])


def test_attainment_restated():
    plane = np.array([[1.0, 2.0, 3.0, 4.0], [1.0, NAN, 3.0, 4.0], [5.0, 5.0, 5.0, 5.0]])
    w = np.array([0.1, 0.0, 0.3, 0.6])
    q, _ = ec.profile_q("population", None, w, None, table=[dict(subject=0)] * 3)
    pta, mean = ec.np_attainment(plane, q, np.array([3.0, 3.5, 6.0]))
    np.testing.assert_allclose(pta, [0.9, 0.6, 0.0], rtol=1e-15)  # `at least`; the NaN sits under weight 0
    np.testing.assert_allclose(mean, [3.4, 3.4, 5.0], rtol=1e-15)
    q[1, 1] = 0.2
    assert np.isnan(ec.np_attainment(plane, q, np.zeros(3))[0]).tolist() == [False, True, False]


def test_the_new_symbols_are_exported_and_bound():
    L = C.CDLL(_ffi.LIB_PATH)
    bound = {n for n, _, _ in _ffi.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in bound, name
    assert _ffi.lib().pmx_abi_version() == 3  # additive: the version stays
    assert (_abi.PMX_AUC_LINEAR, _abi.PMX_AUC_LIN_UP_LOG_DOWN, _abi.PMX_AUC_LIN_LOG) == (0, 1, 2)
    assert [_abi.PMX_EXPO_AUC, _abi.PMX_EXPO_AUMC, _abi.PMX_EXPO_CMAX, _abi.PMX_EXPO_TMAX, _abi.PMX_EXPO_CMIN,
            _abi.PMX_EXPO_TIME_ABOVE, _abi.PMX_EXPO_ALL] == [1, 2, 4, 8, 16, 32, 63]
    assert _ffi.lib().pmx_population_n_profiles(None) == -1
    assert _ffi.lib().pmx_population_profile_info(None, None, None, None, None) == _abi.PMX_ERR_INVALID_ARGUMENT


def test_argument_faults_are_refused_without_a_device():
    """Argument checks come before anything touches a device, so they are the same on a machine without one.  The
    handles are never dereferenced on these paths: any non-null address stands in for them."""
    L = _ffi.lib()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    INV = _abi.PMX_ERR_INVALID_ARGUMENT
    expo = L.pmx_exposure_device      # pop, d_pred, n, ld_pred, method, window, metrics, d_out, ld_out, stream
    att = L.pmx_attainment_device     # pop, d_metric, n, ld_metric, d_target, d_w, d_ll, ld_ll, d_lpyl, d_pta, d_mean, stream
    host = L.pmx_exposure_attainment  # model, pop, em, theta, n, w, method, window, metric, target, pta, mean, status
    wbuf = (C.c_double * 2)(0.25, 0.75)
    wa = C.addressof(wbuf)
    keep = []

    def window(t0, t1, thr):  # three doubles on the host
        keep.append((C.c_double * 3)(t0, t1, thr))
        return C.addressof(keep[-1])

    good_expo = [a, a, 2, 2, 0, window(0.0, 1.0, 1.0), 63, a, 2, None]
    good_att = [a, a, 2, 2, a, a, a, 2, a, a, a, None]
    good_host = [a, a, a, a, 2, wa, 0, window(0.0, 1.0, 1.0), 1, a, a, a, None]

    def refused(fn, good, word=None, **changes):
        args = list(good)
        for at, v in changes.items():
            args[int(at[1:])] = v
        assert fn(*args) == INV, (fn.__name__, changes)
        if word is not None:
            assert word in L.pmx_last_error(), (fn.__name__, changes, L.pmx_last_error())

    for fn, good, pointers, n_at in ((expo, good_expo, (0, 1, 7), 2), (att, good_att, (0, 1, 5), 2), (host, good_host, (0, 1, 3, 5), 4)):
        for i in pointers:
            refused(fn, good, b"null argument", **{f"_{i}": None})
            refused(fn, good, b"null argument", **{f"_{i}": None, f"_{n_at}": 0})  # nulls are looked at first
        for n in (0, -3):
            refused(fn, good, b"n_support", **{f"_{n_at}": n})
    # pitches below n_support
    refused(expo, good_expo, b"ld_pred", _3=1)
    refused(expo, good_expo, b"ld_out", _8=1)
    refused(att, good_att, b"ld_metric", _3=1)
    refused(att, good_att, b"ld_ll", _7=1)
    # metrics: none, a bit above 63; the host form: anything but one bit
    for bits in (0, 64, 63 + 64, 1 << 31):
        refused(expo, good_expo, b"metrics", _6=bits)
        refused(host, good_host, b"metric", _8=bits)
    for bits in (3, 63, 36):
        refused(host, good_host, b"exactly one", _8=bits)
    # method outside 0..2; a >= b; NaN bounds; a NaN threshold, or none, where it is read
    for fn, good, m_at in ((expo, good_expo, 4), (host, good_host, 6)):
        for method in (-1, 3):
            refused(fn, good, b"method", **{f"_{m_at}": method})
        for t0, t1 in ((1.0, 1.0), (2.0, 1.0), (NAN, 1.0), (0.0, NAN), (INF, INF), (-INF, -INF)):
            refused(fn, good, b"window", **{f"_{m_at + 1}": window(t0, t1, 1.0)})
        refused(fn, good, b"threshold", **{f"_{m_at + 1}": window(0.0, 1.0, NAN), f"_{m_at + 2}": 32})
        refused(fn, good, b"threshold", **{f"_{m_at + 1}": None, f"_{m_at + 2}": 32})
    refused(expo, good_expo, b"threshold", _5=window(-INF, INF, NAN), _6=63)
    # both outputs null; d_ll without d_lpyl and the reverse; pta without target (and, host form, the reverse)
    refused(att, good_att, b"both null", _9=None, _10=None)
    refused(host, good_host, b"both null", _10=None, _11=None)
    for gone in (6, 8):
        refused(att, good_att, b"go together", **{f"_{gone}": None})
    refused(att, good_att, b"d_target", _4=None)
    refused(host, good_host, b"go together", _9=None)
    refused(host, good_host, b"go together", _10=None)
    # the host form's weights are on the host: checked before any work
    for w in ([0.5, -0.5], [0.5, NAN], [0.0, 0.0]):
        bad = (C.c_double * 2)(*w)
        refused(host, good_host, b"w", _5=C.addressof(bad))
        refused(host, good_host, b"w", _5=C.addressof(bad), _2=None)  # population mode too
