"""Every kernel entry writes only the rows and bytes the caller owns (include/pmx.h, above pmx_predict): pred / ll /
status / theta need only their natural alignment, the last row needs n_support elements and not ld, nothing outside
[row * ld, row * ld + n_support) is written, a NULL status is never dereferenced.

Each entry runs at several support-grid sizes under five layouts of one sentinel arena (tests/arena.py: every byte
dirty, guard zones around every buffer):

        pred / ll offset, pitch            status offset    theta offset
    A   0,  ld = P   (the reference)       0                0
    B   8,  ld = P                         1                8
    C   0,  ld = P + 1                     4                0
    D   8,  ld = P + 3                     NULL             8        (launched twice into the same arena)
    E   0,  ld = recommended_ld(P + 1)     0                0

  1. layout A equals the CPU oracle at the suite's bars (TOL_ANALYTICAL 1e-6, TOL_ODE 1e-4, TOL_LL 1e-9 on
     max(|want|, 1)), status and finiteness equal;
  2. every other layout's owned bytes equal layout A's bit for bit (a lane's arithmetic depends on its support-point
     index, never on an address), which also proves every owned element was written: the arena's fill would differ;
  3. the arena is clean after every launch.

The support grid holds rows with complex eigenvalues and rows with a zero volume where the model has them and P >= 3,
so the NaN rows and failure bytes are stored under every layout too.  Every launch asserts the kernel that served it.
A lane with complex eigenvalues fails a subject at its first propagation and serves it like any other lane up to an
occasion's first propagation: the mixed population holds an empty subject, a subject with doses only, a subject
observed before its first dose and one observed at the first instant of its second occasion; a shared design with both
kinds of early observation runs through the classed, steps, grid and pair routes.  The host asserts that the oracle has
finite rows (and, in the mixed population, an OK pair) in a column with complex eigenvalues.
Not tested: pitches at or beyond 2^28 doubles (the `ll_ld < 2^28` branch of plan_routes) need multi-gigabyte buffers."""
import ctypes as C

import numpy as np
import pytest

import oracle
from pharmsol_amd import (ODE, Analytical, Data, Pow, Ratio, Scaled, Subject, _abi, _ffi, analytical, bolus, infusion,
                          runtime, synth)
from tests import models
from tests.arena import Arena
from tests.test_gpu_fuzz import kernel_theta
from tests.test_gpu_likelihood import EM_ADD, TOL_LL, _censor_some
from tests.test_gpu_loose_classes import shaped_subject, with_observed_values
from tests.test_gpu_parity import TOL_ANALYTICAL, TOL_ODE, rel_err

pytestmark = pytest.mark.gpu

SWITCHES = ("PMX_DISABLE_LADDER", "PMX_DISABLE_CLASSING", "PMX_DISABLE_STEPS", "PMX_DISABLE_DYN3", "PMX_TUNE_LOOSE",
            "PMX_TUNE_PROP_SLOTS", "PMX_TUNE_GRID_MIN_P", "PMX_TUNE_LL_OLD", "PMX_TUNE_MIN_CLASS")
GRID_P = (1, 8, 9, 64, 65, 129, 136, 257)  # 8 / 64 / 136: 8-byte status clears; 1 / 9 / 65 / 129 / 257: a row ends on a half pair
PAIR_P = (1, 7, 65)                        # 65 with the crossover raised: several 256-lane blocks and a tail
GRID, NO_CLASSES, PAIR = {"PMX_TUNE_GRID_MIN_P": "1"}, {"PMX_DISABLE_CLASSING": "1"}, {"PMX_TUNE_GRID_MIN_P": "1000"}
ARENA_BYTES = 4 << 20
STATE = {"arena": None, "hip_error": None}


def layouts(P):
    """name -> (output offset in bytes, output pitch, status offset or None, theta offset)."""
    return {"A": (0, P, 0, 0), "B": (8, P, 1, 8), "C": (0, P + 1, 4, 0), "D": (8, P + 3, None, 8),
            "E": (0, runtime.recommended_ld(P + 1), 0, 0)}


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


@pytest.fixture(autouse=True)
def _stop_after_a_hip_error():
    """A HIP error ends the module: nothing more is launched on a device that has faulted."""
    if STATE["hip_error"]:
        pytest.fail(f"not run: an earlier launch of this module ended in a HIP error ({STATE['hip_error']})")
    yield


def gpu_arena():
    if STATE["arena"] is None:
        STATE["arena"] = Arena("cuda", ARENA_BYTES)
    return STATE["arena"]


# ----------------------------------------------------------------------------------------------------- populations
def m2():
    return models.handwritten_analytical("two_compartments", 0, 4).with_ndrugs(1)  # theta = ke, kcp, kpc, v


def m3():
    return Analytical.new("three_compartments", {0: Ratio(0, 5)}, nparams=6).with_nstates(3).with_ndrugs(1).with_nout(1)


def shared_subjects(rng, n=11):
    """n copies of one design with scaled doses: exact classes only (two-state models: a chunk of 8 and one of 3)."""
    proto = shaped_subject(rng, 0, 0)
    subs = []
    for i in range(n):
        b = Subject.builder(f"e{i}")
        for ev in proto.occasions[0].events:
            b = b.infusion(ev.time, ev.amount + 9.0 * i, 0, ev.duration) if hasattr(ev, "duration") else b.missing_observation(ev.time, 0)
        subs.append(b.build())
    return subs


def loose_subjects(rng, n=7):
    """One program shape, every subject's own times (min_loose is 6 for G = 8)."""
    return [shaped_subject(rng, 0, 100 + i) for i in range(n)]


def early_observations(name, amount, second_occasion=True):
    """Observed before the first dose (same instant) and, second_occasion, at the first instant of a second occasion."""
    b = Subject.builder(name).missing_observation(0.0, 0).infusion(0.0, amount, 0, 0.5)
    for t in (1.0, 2.0, 6.0):
        b = b.missing_observation(t, 0)
    if second_occasion:
        b = b.reset().missing_observation(0.0, 0).bolus(0.0, amount / 2, 0).missing_observation(3.0, 0)
    return b.build()


def early_shared():
    """A shared design with those early observations: one class of 11."""
    return [early_observations(f"p{i}", 100.0 + 7.0 * i) for i in range(11)]


def mixed_subjects(seed=21):
    """Exact classes, loose classes and subjects no class takes in one population, shuffled: 11 on a shared design,
    7 of one shape with their own times, 3 of shapes nobody shares (one with two occasions), an empty subject and one
    with doses and no observation, and the two subjects of early_observations."""
    rng = np.random.default_rng(seed)
    subs = shared_subjects(rng) + loose_subjects(rng)
    subs += [shaped_subject(rng, 1, 200), shaped_subject(rng, 2, 201), models.random_subject(rng)]
    subs.append(Subject.builder("empty").build())
    subs.append(Subject.builder("doses_only").bolus(0.0, 100.0, 0).infusion(2.0, 50.0, 0, 1.0).build())
    subs += [early_observations("predose", 120.0, second_occasion=False), early_observations("second_occasion", 90.0)]
    return [subs[k] for k in rng.permutation(len(subs))]


def special_rows(theta, complex_row=None, vol_col=None):
    """Rows 1 and 9: complex eigenvalues, rows 2 and 12: a zero volume (where the grid has that many rows)."""
    theta = np.ascontiguousarray(theta, dtype=np.float64).copy()
    for bad, zero in ((1, 2), (9, 12)):
        if theta.shape[0] > zero:
            if complex_row is not None:
                for col, val in complex_row.items():
                    theta[bad, col] = val
            if vol_col is not None:
                theta[zero, vol_col] = 0.0
    return theta


COMPLEX2 = {0: 1.0, 1: -3.0, 2: 1.0}  # (ke + kcp + kpc)^2 < 4 ke kpc
COMPLEX3 = {0: 1.0, 1: -3.0, 2: 0.1, 3: 1.0, 4: 0.5}  # three_compartments k10, k12, k13, k21, k31: a complex pair


def theta_m2(P):
    return special_rows(synth.theta_c3(P), COMPLEX2, 3)


def theta_m3(P):
    rng = np.random.default_rng(5)
    return special_rows(np.concatenate([kernel_theta("three_compartments", P, rng), rng.uniform(10, 80, (P, 1))], axis=1), COMPLEX3, 5)


def lag_model():
    m = Analytical.new("one_compartment_with_absorption", {0: Ratio(1, 2)}, nparams=5, lag={0: 3}, fa={0: 4})
    return m.with_nstates(2).with_ndrugs(1).with_nout(1)  # theta = ka, ke, v, lag, fa


def oral_subjects(n=11, label=0, out=0):
    subs = []
    for i in range(n):
        b = Subject.builder(f"o{i}").bolus(0.0, 100.0 + i, label).bolus(12.0, 40.0 + i, label)
        for t in (0.5, 1.0, 2.0, 4.0, 12.0, 12.5, 20.0):
            b = b.missing_observation(t, out)
        subs.append(b.build())
    return subs


def theta_lag(P):
    rng = np.random.default_rng(7)
    lag = rng.choice([0.0, 0.25, 0.75, 1.5, 3.0, 13.0, 40.0], size=P)
    th = np.stack([rng.uniform(1.0, 3.0, P), rng.uniform(0.05, 0.4, P), rng.uniform(10, 60, P), lag, rng.uniform(0.4, 1.0, P)], axis=1)
    return special_rows(th, None, 2)


def cov2_model():
    return analytical(name="wt_two_compartments", params=["ke0", "kcp", "kpc", "v0"],
                      derived={"ke": Scaled("ke0", (Pow("wt", 70.0, 0.75),)), "v": Scaled("v0", (Pow("wt", 70.0, 1.0),))},
                      covariates=["wt"], structure="two_compartments", states=["central", "periph"], outputs=["cp"],
                      routes=[bolus("dose", "central")], out={"cp": Ratio("central", "v")})


def cov2_subjects(n=12):
    rng = np.random.default_rng(9)
    subs = []
    for i in range(n):
        b = Subject.builder(f"c{i}").bolus(0.0, 100.0 + i, "dose").covariate("wt", 0.0, 55.0 + 3 * i)
        if i % 2:
            b = b.covariate("wt", 10.0, 90.0 - 2 * i)
        for t in np.sort(rng.uniform(0.2, 30.0, 6)):
            b = b.missing_observation(float(t), "cp")
        subs.append(b.build())
    return subs


def cov3_infusion_model():
    return analytical(name="three_cmt_oral_wt_iv", params=["ka", "k10_0", "k12", "k13", "k21", "k31", "v"],
                      derived={"k10": Scaled("k10_0", (Pow("wt", 70.0, 0.75),))}, covariates=["wt"],
                      structure="three_compartments_with_absorption", states=["gut", "central", "periph1", "periph2"],
                      outputs=["cp"], routes=[bolus("oral", "gut"), infusion("iv", "central")], out={"cp": Ratio("central", "v")})


def cov3_infusion_subjects(n=11):
    subs = []
    for i in range(n):
        b = (Subject.builder(f"i{i}").bolus(0.0, 100.0 + 5 * i, "oral").infusion(6.0, 60.0 + i, "iv", 2.0)
             .covariate("wt", 0.0, 60.0 + 2 * i).covariate("wt", 30.0, 85.0 - i))
        for t in (1.0, 2.0, 4.0, 6.5, 8.0, 12.0, 23.5, 36.0):
            b = b.missing_observation(t, "cp")
        subs.append(b.build())
    return subs


COMPLEX3_ORAL = {1: 1.0, 2: -3.0, 4: 1.0}  # three_compartments_with_absorption k10_0, k12, k21: complex for every wt here


def theta_cov3(P):
    return special_rows(synth.theta_c5(P), COMPLEX3_ORAL, 6)


def ode_rk4():
    return models.handwritten_ode("two_cmt_iv", 0, 4, h_max=0.1).with_ndrugs(1)


def ode_lag():
    return (ODE.new("one_cmt_oral", {0: Ratio(1, 2)}, nparams=4, lag={0: 3}, h_max=0.1).with_nstates(2).with_ndrugs(1)
            .with_nout(1))  # theta = ka, ke, v, lag


def theta_ode_lag(P):
    return np.ascontiguousarray(theta_lag(P)[:, :4])


def ode_auto():
    return (ODE.new("two_cmt_oral", {0: Ratio(1, 4)}, nparams=5, h_max=0.1).with_nstates(3).with_ndrugs(1).with_nout(1)
            .with_solver("auto").with_tolerances(1e-8, 1e-8))  # theta = ke, ka, kcp, kpc, v


def theta_auto(P):
    rng = np.random.default_rng(13)
    th = np.stack([rng.uniform(0.05, 0.3, P), rng.uniform(0.5, 3.0, P), rng.uniform(0.2, 0.6, P), rng.uniform(0.1, 0.4, P),
                   rng.uniform(10, 50, P)], axis=1)
    return special_rows(th, None, 4)


def theta_oral(P, ncol):
    rng = np.random.default_rng(17)
    return np.stack([rng.uniform(1.0, 3.0, P), rng.uniform(0.05, 0.4, P), rng.choice([0.0, 0.25, 1.5, 13.0], size=P)], axis=1)[:, :ncol].copy()


JIT = {}


def jit_model(kind):
    """One compile per run-time-compiled model (sources: the suite's own fixtures)."""
    if kind not in JIT:
        from tests.test_api_surface import _ORAL_LAG_SRC, _ORAL_SRC

        if kind == "analytical_user":
            JIT[kind] = synth.model_user_covariates()
        elif kind == "ode_user":
            JIT[kind] = ODE.user(_ORAL_LAG_SRC, nstates=2, nparams=3, ndrugs=1, nout=1, h_max=0.1)
        else:
            JIT[kind] = ODE.custom(_ORAL_SRC, nstates=2, nparams=2, h_max=0.1)
            oracle.compile_custom(_ORAL_SRC)  # the CPU oracle runs the same body
    return JIT[kind]


# --------------------------------------------------------------------------------------------------------- entries
class Entry:
    """One kernel entry: model, population, what is called and what must have served it."""

    def __init__(self, name, build, kernel, sizes, env=None, what="predict", batch=False, tol=TOL_ANALYTICAL, stats=False,
                 state=None, plan=None, censor=False, host=False, only=None, pins=()):
        self.name, self.build, self.kernel, self.sizes, self.env = name, build, kernel, sizes, dict(env or {})
        self.what, self.batch, self.tol, self.stats, self.state, self.plan = what, batch, tol, stats, state, plan
        self.censor, self.host, self.only, self.pins = censor, host, only, pins
        self.em = EM_ADD

    def prepare(self):
        """(model, flat, theta(P)) with, for the log-likelihood, measured values (a fifth missing) in the population."""
        model, flat, theta = self.build()
        if self.what == "loglik":
            flat = with_observed_values(flat, model, theta(8), 3)
            if self.censor:
                flat = _censor_some(flat, np.random.default_rng(12))
        return model, flat, theta

    def expected(self, model, flat, theta):
        """The oracle's (output, status) in the shape of the call's buffers."""
        if self.what == "loglik":
            want, st = oracle.loglik(model, flat, self.em, theta)
            if self.batch:  # subject s under its own row
                want, st = np.diagonal(want).copy(), np.diagonal(st).copy()
        elif self.batch:
            want, st = oracle.predict_batch(model, flat, theta)
        else:
            ref = model
            if self.state is not None:  # Prediction::state: the raw amount of one state
                ref = models.handwritten_analytical("two_compartments", 0, 4).with_ndrugs(1)
                ref.out = {0: Ratio(self.state, None)}
            want, st = oracle.predict(ref, flat, theta)
        return np.asarray(want, dtype=np.float64).reshape(self.out_shape(flat, theta)), np.asarray(st, dtype=np.uint8).reshape(self.status_shape(flat, theta))

    def out_shape(self, flat, theta):
        rows = flat.n_subjects if self.what == "loglik" else flat.n_observations
        return (1, rows) if self.batch else (rows, theta.shape[0])

    def status_shape(self, flat, theta):
        return (1, flat.n_subjects) if self.batch else (flat.n_subjects, theta.shape[0])


def launch(entry, model, pop, v):
    """One call of the C ABI into the carved views `v` (device-pointer forms on a device arena, host-pointer forms on
    a CPU arena); returns the return code of a host-pointer form."""
    L = _ffi.lib()
    dm = runtime._as_model(model)
    th, out, st = v["theta"].data_ptr(), v["out"].data_ptr(), (v["status"].data_ptr() if v["status"] is not None else None)
    P, ld = int(v["theta"].shape[0]), int(v["out"].stride(0))
    tail = ()
    sfx = ""
    if not entry.host:
        import torch

        tail = (torch.cuda.current_stream().cuda_stream,)
        sfx = "_device"
    if entry.what == "loglik":
        em = entry.em.to_c(model)
        emp = C.cast(em, C.c_void_p)
        if entry.batch:
            rc = getattr(L, "pmx_loglik_batch" + sfx)(dm.handle, pop.handle, emp, th, out, st, *tail)
        else:
            rc = getattr(L, "pmx_loglik" + sfx)(dm.handle, pop.handle, emp, th, P, out, ld, st, *tail)
    elif entry.stats:
        rc = L.pmx_predict_stats_device(dm.handle, pop.handle, th, P, out, ld, st, *tail, v["stats"].data_ptr())
    elif entry.state is not None:
        rc = L.pmx_predict_state_device(dm.handle, pop.handle, th, P, entry.state, out, ld, st, *tail)
    elif entry.batch:
        rc = getattr(L, "pmx_predict_batch" + sfx)(dm.handle, pop.handle, th, out, st, *tail)
    else:
        rc = getattr(L, "pmx_predict" + sfx)(dm.handle, pop.handle, th, P, out, ld, st, *tail)
    if rc == _abi.PMX_ERR_HIP:
        STATE["hip_error"] = L.pmx_last_error().decode()
    _ffi.check(rc, allow_pair_failures=entry.host)
    return rc


def synchronize(entry):
    if entry.host:
        return
    import torch

    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a fault inside the kernel: nothing more runs in this module
        STATE["hip_error"] = str(e).splitlines()[0]
        raise


def bits(t):
    """The bytes of a strided view as an integer tensor of its own shape (float64 -> int64; NaN payloads and signed zeros count)."""
    import torch

    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous()


def assert_matches_oracle(entry, got, st, want, wst, where):
    np.testing.assert_array_equal(st, wst, err_msg=f"{where}: status")
    ok = np.isfinite(want)
    if entry.host and entry.what == "loglik" and entry.batch:
        assert (got[~ok] == -np.inf).all(), f"{where}: a failed subject is -inf"  # (pmx_loglik_batch, likelihood/mod.rs:137-140)
    np.testing.assert_array_equal(np.isfinite(got), ok, err_msg=f"{where}: finiteness")
    if not ok.any():
        return
    if entry.what == "loglik":
        err = (np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)).max()
        assert err <= TOL_LL, f"{where}: log-likelihood off by {err:.3e}"
    else:
        err = rel_err(got[ok], want[ok]).max()  # (the suite's metric, tests/test_gpu_parity.py)
        assert err <= entry.tol, f"{where}: max rel err {err:.3e} > {entry.tol:g}"


def run_entry(entry, arena, make_population, kernel_name=runtime.last_kernel_name):
    """Every size of the entry under every layout: oracle for A, A's bits for the others, a clean arena after each launch."""
    import torch

    model, flat, theta_of = entry.prepare()
    pop = make_population(flat)
    S = flat.n_subjects
    if entry.plan is not None:  # the routing this entry is about, decided on the host
        entry.plan(runtime.class_plan(model, flat))
    for P in entry.sizes:
        theta = theta_of(S if entry.batch else P)
        want, wst = entry.expected(model, flat, theta)
        (rows, cols), (srows, scols) = entry.out_shape(flat, theta), entry.status_shape(flat, theta)
        if entry.pins and P >= 3:  # column 1 has complex eigenvalues: the oracle serves the rows in front of a PROP
            assert (wst[:, 1] == _abi.PMX_PAIR_COMPLEX_ROOTS).any() and np.isfinite(want[:, 1]).sum() >= (3 if "shared" in entry.pins else 2)
            assert "ok" not in entry.pins or (wst[:, 1] == _abi.PMX_PAIR_OK).any()
        ref = None
        for name in entry.only or "ABCDE":
            off, ld, st_off, th_off = layouts(cols)[name]
            where = f"{entry.name} P={P} layout {name}"
            arena.reset()
            v = {"theta": arena.carve(theta.shape[0], theta.shape[1], theta.shape[1], torch.float64, th_off, name="theta")}
            v["theta"].copy_(torch.from_numpy(theta))
            v["out"] = arena.carve(rows, cols, ld, torch.float64, off, name="ll" if entry.what == "loglik" else "pred")
            v["status"] = None if st_off is None else arena.carve(srows, scols, scols, torch.uint8, st_off, name="status")
            if entry.stats:
                v["stats"] = arena.carve(S * P, 4, 4, torch.int32, 4 if name in "BCD" else 0, name="stats")
            for rep in range(2 if name == "D" else 1):  # D again: a status store through a stale pointer would land in the arena
                launch(entry, model, pop, v)
                synchronize(entry)
                assert kernel_name() == entry.kernel, f"{where}: routed to {kernel_name()}, expected {entry.kernel}"
                arena.assert_clean()
                assert torch.equal(bits(v["theta"]), bits(torch.from_numpy(theta).to(v["theta"].device))), f"{where}: theta was written"
            got = {k: bits(t).clone() for k, t in v.items() if t is not None and k != "theta"}
            if ref is None:
                assert name == "A"
                assert_matches_oracle(entry, v["out"].cpu().numpy(), v["status"].cpu().numpy(), want, wst, where)
                ref = got
                if entry.stats:  # nothing else vouches for these: every record was written
                    assert not (ref["stats"] == -0x5A5A5A5B).any(), f"{where}: a statistics element still holds the arena's fill"
            else:
                for k, t in got.items():
                    diff = (t != ref[k]).nonzero()
                    assert diff.numel() == 0, (f"{where}: {k} differs from layout A in {diff.shape[0]} element(s), first at "
                                               f"{diff[0].tolist()}: {t[tuple(diff[0])].item():#x} vs {ref[k][tuple(diff[0])].item():#x}")


def device_population(flat):
    return runtime.DevicePopulation(flat, 0)


def has_all_three(plan):
    assert plan["chunks_exact"] > 0 and plan["chunks_loose"] > 0 and plan["generic_subjects"] > 0, plan


def exact_only(plan):
    assert plan["chunks_exact"] > 0 and plan["chunks_loose"] == 0 and plan["generic_subjects"] == 0, plan


def loose_first(plan):
    assert plan["chunks_exact"] == 0 and plan["chunks_loose"] > 0, plan


def pop_of(model_fn, subjects_fn, theta_fn):
    def build():
        m = model_fn()
        return m, m.flatten(Data(subjects_fn())), theta_fn

    return build


def shared11():
    return shared_subjects(np.random.default_rng(21))


def loose7():
    return loose_subjects(np.random.default_rng(21))


def c5_population():
    m = synth.model_three_cpt_abs_wt()
    return m, synth.population_c5(11), theta_cov3


def user_population():
    return jit_model("analytical_user"), synth.population_user(12), lambda P: special_rows(synth.theta_user(P), None, 2)


M2_MIXED = pop_of(m2, mixed_subjects, theta_m2)
M2_SHARED = pop_of(m2, shared11, theta_m2)
M2_EARLY = pop_of(m2, early_shared, theta_m2)
M3_EARLY = pop_of(m3, early_shared, theta_m3)
M2_LOOSE = pop_of(m2, loose7, theta_m2)
M3_MIXED = pop_of(m3, mixed_subjects, theta_m3)
LAG_SHARED = pop_of(lag_model, oral_subjects, theta_lag)
COV2 = pop_of(cov2_model, cov2_subjects, lambda P: special_rows(synth.theta_c3(P), COMPLEX2, 3))
COV3_IV = pop_of(cov3_infusion_model, cov3_infusion_subjects, theta_cov3)
ODE_MIXED = pop_of(ode_rk4, mixed_subjects, lambda P: special_rows(synth.theta_c3(P), None, 3))
ODE_LAG = pop_of(ode_lag, oral_subjects, theta_ode_lag)
ODE_AUTO = pop_of(ode_auto, oral_subjects, theta_auto)
ODE_USER = pop_of(lambda: jit_model("ode_user"), oral_subjects, lambda P: theta_oral(P, 3))
ODE_CUSTOM = pop_of(lambda: jit_model("ode_custom"), oral_subjects, lambda P: theta_oral(P, 2))
BOTH = dict(NO_CLASSES, PMX_DISABLE_STEPS="1", **GRID)
WALKER = dict(NO_CLASSES, **GRID)
LL = dict(what="loglik")

ENTRIES = [
    # two-compartment IV, plain model
    Entry("mixed:classed+loose+steps", M2_MIXED, "pmx_analytical_classed", GRID_P, GRID, plan=has_all_three, pins=("finite", "ok")),
    Entry("classed", M2_SHARED, "pmx_analytical_classed", GRID_P, GRID, plan=exact_only),
    Entry("steps", M2_MIXED, "pmx_analytical_steps", GRID_P, WALKER, pins=("finite", "ok")),
    Entry("grid", M2_MIXED, "pmx_analytical_grid", GRID_P, BOTH, pins=("finite", "ok")),
    Entry("pair", M2_MIXED, "pmx_analytical_pair", PAIR_P, PAIR, pins=("finite", "ok")),
    # observations before the first dose and at a second occasion's first instant, on a shared design, by every route
    Entry("early:classed", M2_EARLY, "pmx_analytical_classed", (9, 65), GRID, plan=exact_only, pins=("finite", "shared")),
    Entry("early:steps", M2_EARLY, "pmx_analytical_steps", (9, 65), WALKER, pins=("finite", "shared")),
    Entry("early:grid", M2_EARLY, "pmx_analytical_grid", (9, 65), BOTH, pins=("finite", "shared")),
    Entry("early:pair", M2_EARLY, "pmx_analytical_pair", (7, 65), PAIR, pins=("finite", "shared")),
    Entry("early:three-state-classed", M3_EARLY, "pmx_analytical_classed", (9, 65), GRID, plan=exact_only, pins=("finite", "shared")),
    Entry("early:three-state-steps", M3_EARLY, "pmx_analytical_steps", (9, 65), WALKER, pins=("finite", "shared")),
    Entry("pair-batch", M2_MIXED, "pmx_analytical_pair", (0,), batch=True),
    Entry("three-state:classed", M3_MIXED, "pmx_analytical_classed", GRID_P, GRID, plan=has_all_three),  # G = 4
    Entry("three-state:steps", M3_MIXED, "pmx_analytical_steps", GRID_P, WALKER),
    # lagged oral model
    Entry("lag:classed", LAG_SHARED, "pmx_analytical_classed<lag>", GRID_P, GRID, plan=exact_only),
    Entry("lag:grid", LAG_SHARED, "pmx_analytical_grid<lag>", GRID_P, WALKER),
    Entry("lag:pair", LAG_SHARED, "pmx_analytical_pair<lag>", PAIR_P, PAIR),
    # covariate models
    Entry("dyn:classed", COV2, "pmx_analytical_classed<dyn>", GRID_P, GRID, plan=loose_first),
    Entry("dyn:grid", COV2, "pmx_analytical_grid<dyn>", GRID_P, WALKER),
    Entry("dyn:pair", COV2, "pmx_analytical_pair<dyn>", PAIR_P, PAIR),
    Entry("dyn3", c5_population, "pmx_analytical_dyn3", GRID_P, GRID),
    Entry("dyn3:infusion-grid", COV3_IV, "pmx_analytical_grid<dyn>", GRID_P, GRID),
    # fused log-likelihood
    Entry("ll:classed_ll", M2_MIXED, "pmx_analytical_classed_ll", GRID_P, GRID, plan=has_all_three, **LL),
    Entry("ll:classed_ll-censored", M2_SHARED, "pmx_analytical_classed_ll", GRID_P, GRID, censor=True, **LL),
    Entry("ll:classed-old", M2_SHARED, "pmx_analytical_classed<ll>", GRID_P, dict(GRID, PMX_TUNE_LL_OLD="1"), **LL),
    Entry("ll:classed-loose", M2_LOOSE, "pmx_analytical_classed<ll,loose>", GRID_P, GRID, plan=loose_first, **LL),
    Entry("ll:steps", M2_MIXED, "pmx_analytical_steps", GRID_P, WALKER, **LL),
    Entry("ll:grid", M2_MIXED, "pmx_analytical_grid", GRID_P, BOTH, **LL),
    Entry("ll:dyn3", c5_population, "pmx_analytical_dyn3", GRID_P, GRID, **LL),
    Entry("ll:pair", M2_MIXED, "pmx_analytical_pair", PAIR_P, PAIR, **LL),
    Entry("ll:pair-batch", M2_MIXED, "pmx_analytical_pair", (0,), batch=True, **LL),
    # built-in ODE, h_max = 0.1
    Entry("ode:rk4-grid", ODE_MIXED, "pmx_ode_rk4_grid", GRID_P, GRID, tol=TOL_ODE),
    Entry("ode:rk4-pair", ODE_MIXED, "pmx_ode_rk4_pair", PAIR_P, PAIR, tol=TOL_ODE),
    Entry("ode:rk4-batch", ODE_MIXED, "pmx_ode_rk4_pair", (0,), batch=True, tol=TOL_ODE),
    Entry("ode:rk4-grid-lag", ODE_LAG, "pmx_ode_rk4_grid<lag>", GRID_P, GRID, tol=TOL_ODE),
    Entry("ode:auto-grid-stats", ODE_AUTO, "pmx_ode_auto_grid", GRID_P, GRID, tol=TOL_ODE, stats=True),
    Entry("ode:auto-pair-stats", ODE_AUTO, "pmx_ode_auto_pair", PAIR_P, PAIR, tol=TOL_ODE, stats=True),
    Entry("ode:ll-grid", ODE_MIXED, "pmx_ode_rk4_grid", GRID_P, GRID, tol=TOL_ODE, **LL),
    Entry("ode:ll-pair", ODE_MIXED, "pmx_ode_rk4_pair", PAIR_P, PAIR, tol=TOL_ODE, **LL),
    # run-time-compiled models
    Entry("jit:analytical-grid", user_population, "pmx_jit_analytical_grid", GRID_P, GRID),
    Entry("jit:analytical-pair", user_population, "pmx_jit_analytical_pair", PAIR_P, PAIR),
    Entry("jit:analytical-ll", user_population, "pmx_jit_analytical_grid", GRID_P, GRID, **LL),
    Entry("jit:ode-user-grid", ODE_USER, "pmx_jit_ode_user_rk4_grid", GRID_P, GRID, tol=TOL_ODE),
    Entry("jit:ode-user-pair", ODE_USER, "pmx_jit_ode_user_rk4_pair", PAIR_P, PAIR, tol=TOL_ODE),
    Entry("jit:ode-custom-grid", ODE_CUSTOM, "pmx_jit_ode_rk4_grid", GRID_P, GRID, tol=TOL_ODE),
    Entry("jit:ode-custom-pair", ODE_CUSTOM, "pmx_jit_ode_rk4_pair", PAIR_P, PAIR, tol=TOL_ODE),
    # Prediction::state with a pitched ld_out, with (A, B, C, E) and without (D) a status array
    Entry("state", M2_MIXED, "pmx_analytical_classed", (9, 65), GRID, state=1, plan=has_all_three),
]
HOST_ENTRIES = [
    # host-pointer forms into a CPU arena: the matrix forms with layout D, then C; the batch forms with layout B
    Entry("host:predict", M2_MIXED, "pmx_analytical_classed", (9, 65), GRID, host=True, only="ADC"),
    Entry("host:loglik", M2_MIXED, "pmx_analytical_classed_ll", (9, 65), GRID, host=True, only="ADC", **LL),
    Entry("host:predict-batch", M2_MIXED, "pmx_analytical_pair", (0,), batch=True, host=True, only="AB"),
    Entry("host:loglik-batch", M2_MIXED, "pmx_analytical_pair", (0,), batch=True, host=True, only="AB", **LL),
]


@pytest.mark.parametrize("entry", ENTRIES, ids=[e.name for e in ENTRIES])
def test_device_entry_writes_only_what_the_caller_owns(entry, env):
    env(**entry.env)
    run_entry(entry, gpu_arena(), device_population)


@pytest.mark.parametrize("entry", HOST_ENTRIES, ids=[e.name for e in HOST_ENTRIES])
def test_host_pointer_entry_writes_only_what_the_caller_owns(entry, env):
    env(**entry.env)
    run_entry(entry, Arena("cpu", ARENA_BYTES), device_population)


# kernel-order parameters with a complex pair of eigenvalues, for every structure that can have one (micro-constants
# ke = 1, kcp = -3, kpc = 1 / k10 = 1, k12 = -3, k13 = 0.1, k21 = 1, k31 = 0.5; the CL forms with vc = 1)
COMPLEX_BY_STRUCTURE = {
    "two_compartments": [1.0, -3.0, 1.0], "two_compartments_cl": [1.0, -3.0, 1.0, -3.0],
    "two_compartments_with_absorption": [1.0, 2.0, -3.0, 1.0], "two_compartments_cl_with_absorption": [2.0, 1.0, -3.0, 1.0, -3.0],
    "three_compartments": [1.0, -3.0, 0.1, 1.0, 0.5], "three_compartments_cl": [1.0, -3.0, 0.1, 1.0, -3.0, 0.2],
    "three_compartments_with_absorption": [2.0, 1.0, -3.0, 0.1, 1.0, 0.5],
    "three_compartments_cl_with_absorption": [2.0, 1.0, -3.0, 0.1, 1.0, -3.0, 0.2],
}


def complex_lane_case(structure):
    from tests.test_gpu_fuzz import STRUCTS

    ns, nk, central = STRUCTS[structure]
    model = Analytical.new(structure, {0: Ratio(central, nk)}, nparams=nk + 1).with_nstates(ns).with_ndrugs(1).with_nout(1)
    subs = [early_observations(f"q{i}", 100.0 + i) for i in range(3)] + [Subject.builder("empty").build()]
    rng = np.random.default_rng(3)
    theta = np.concatenate([kernel_theta(structure, 9, rng), rng.uniform(10, 80, (9, 1))], axis=1)
    theta[1, :nk] = theta[5, :nk] = COMPLEX_BY_STRUCTURE[structure]
    return model, model.flatten(Data(subs)), theta


@pytest.mark.parametrize("structure", sorted(COMPLEX_BY_STRUCTURE))
def test_steps_walker_reads_a_failed_lane_off_its_exponentials(structure, env):
    """The steps walker keeps no flag for "this subject propagated on a lane with complex eigenvalues": it reads the lane's
    exponentials afterwards.  That needs every structure's exponentials to turn NaN from NaN coefficients - held here, per
    structure, against the oracle: COMPLEX_ROOTS where the subject propagated, OK for the empty one, finite early rows."""
    import torch

    model, flat, theta = complex_lane_case(structure)
    want, wst = oracle.predict(model, flat, theta)
    assert (wst[:3, [1, 5]] == _abi.PMX_PAIR_COMPLEX_ROOTS).all() and (wst[3] == 0).all() and np.isfinite(want[:, 1]).sum() == 6
    env(**WALKER)
    pred, st = runtime.predict(model, runtime.DevicePopulation(flat, 0), theta)
    torch.cuda.synchronize()
    assert runtime.last_kernel_name() == "pmx_analytical_steps"
    np.testing.assert_array_equal(st.cpu().numpy(), wst)
    got = pred.cpu().numpy()
    ok = np.isfinite(want)
    np.testing.assert_array_equal(np.isfinite(got), ok)
    assert rel_err(got[ok], want[ok]).max() <= TOL_ANALYTICAL


@pytest.mark.parametrize("n_doubles", [2, 3, 8193, 1 << 16 | 1])
def test_write_ceiling_zeroes_every_double_and_nothing_else(n_doubles):
    """pmx_measure_write_ceiling: "the buffer's contents are overwritten with zeros" - all n_doubles of them, the last
    one of an odd count too, at a 16-byte and at an 8-byte aligned base."""
    import torch

    arena = gpu_arena()
    for off in (0, 8):
        arena.reset()
        buf = arena.carve(1, n_doubles, n_doubles, torch.float64, off, name="fill")
        rate = C.c_double(-1.0)
        rc = _ffi.lib().pmx_measure_write_ceiling(buf.data_ptr(), n_doubles, 2, torch.cuda.current_stream().cuda_stream, C.byref(rate))
        if rc == _abi.PMX_ERR_HIP:
            STATE["hip_error"] = _ffi.lib().pmx_last_error().decode()
        _ffi.check(rc)
        torch.cuda.synchronize()
        arena.assert_clean()
        dirty = (bits(buf) != 0).nonzero()
        assert dirty.numel() == 0, (f"n_doubles={n_doubles} offset {off}: {dirty.shape[0]} double(s) not zeroed, first at index "
                                    f"{int(dirty[0][1])}: {bits(buf)[0, int(dirty[0][1])].item():#x}")
        assert rate.value > 0.0
