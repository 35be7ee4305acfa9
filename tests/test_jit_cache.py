"""The content-addressed cache of hiprtc code objects (csrc/pmx_jit_cache.cpp; include/pmx.h "code-object cache").

Counters are the assertions (`runtime.jit_cache_stats()`), never wall-clock time.  Every test starts from
`jit_cache_clear()`; tests that need a cold process start a fresh child (tests/jit_cache_child.py).  The CPU half needs no
device: hiprtc compiles for gfx950 without one."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import threading

import numpy as np
import pytest

import oracle
from pharmsol_amd import Analytical, _abi, _ffi, runtime
from tests import jit_cache_child as child
from tests import test_user_analytical as tua

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE_VARS = ("PMX_JIT_CACHE", "PMX_JIT_CACHE_DIR", "PMX_JIT_CACHE_ENTRIES", "PMX_DEBUG_JIT_OPTS", "PMX_DEBUG_JIT_DUMP")


def _create(model):
    """A fresh pmx_model every time (runtime._as_model would keep the first handle on the model object)."""
    return runtime.DeviceModel(model)


def _stats():
    return runtime.jit_cache_stats()


def _base(src=tua.SEQ_SRC, **kw):
    args = dict(eq=None, nstates=1, nparams=1, ndrugs=1, nout=1)
    args.update(kw)
    return Analytical.user(src, **args)


@pytest.fixture(autouse=True)
def _clean_cache(monkeypatch):
    """Every test: no cache variable inherited, switches re-read, memory level and counters empty - and the same on
    the way out, so that the order of tests (and of other modules) does not matter."""
    for v in CACHE_VARS:
        monkeypatch.delenv(v, raising=False)
    L = _ffi.lib()
    L.pmx_debug_reload_env()
    runtime.jit_cache_clear()
    yield
    for v in CACHE_VARS:
        monkeypatch.delenv(v, raising=False)
    L.pmx_debug_reload_env()
    runtime.jit_cache_clear()


def _setenv(monkeypatch, **kw):
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    _ffi.lib().pmx_debug_reload_env()


def _child_env(cache_dir=None, **extra):
    env = {k: v for k, v in os.environ.items() if k not in CACHE_VARS}
    if cache_dir is not None:
        env["PMX_JIT_CACHE_DIR"] = str(cache_dir)
    env.update({k: str(v) for k, v in extra.items()})
    return env


def _child_cmd(mode, *args):
    return [sys.executable, "-m", "tests.jit_cache_child", mode, *map(str, args)]


def _run_child(mode, *args, cache_dir=None, timeout=None, **extra):
    """A cold process; returns its counters.  A non-zero exit fails the test at once."""
    cmd = _child_cmd(mode, *args)
    if timeout is not None:  # (a limit of the child's own: it is ended, the test does not wait on it)
        cmd = ["timeout", "-k", "10", str(timeout)] + cmd
    r = subprocess.run(cmd, cwd=ROOT, env=_child_env(cache_dir, **extra), capture_output=True, text=True)
    assert r.returncode == 0, f"child {mode} exited {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1])


def _cache_files(d):
    return sorted(os.listdir(d))


# --------------------------------------------------------------------------------------------- CPU: memory level
def test_memory_hit_returns_the_same_code_object(tmp_path, monkeypatch):
    dumps = [tmp_path / "first.co", tmp_path / "second.co"]
    _setenv(monkeypatch, PMX_DEBUG_JIT_DUMP=dumps[0])
    _create(tua.covariate_model())
    s1 = _stats()
    assert (s1["compiles"], s1["mem_hits"], s1["entries"]) == (1, 0, 1) and s1["bytes"] == dumps[0].stat().st_size > 0
    _setenv(monkeypatch, PMX_DEBUG_JIT_DUMP=dumps[1])
    _create(tua.covariate_model())
    s2 = _stats()
    assert s2["compiles"] == s1["compiles"] and s2["mem_hits"] == s1["mem_hits"] + 1
    assert dumps[0].read_bytes() == dumps[1].read_bytes()  # the dump is written on a hit too, from what was handed back
    assert (s2["disk_hits"], s2["disk_writes"], s2["disk_rejects"]) == (0, 0, 0)  # no PMX_JIT_CACHE_DIR: no disk level


def test_key_covers_source_sizes_function_mask_options_and_big_lists(monkeypatch):
    L = _ffi.lib()
    warm = _create(_base())
    assert _stats()["compiles"] == 1

    def expect_miss(what, make):
        before = _stats()
        keep = make()
        after = _stats()
        assert after["compiles"] == before["compiles"] + 1 and after["mem_hits"] == before["mem_hits"], what
        return keep

    expect_miss("one character of the source", lambda: _create(_base(tua.SEQ_SRC.replace("pw[0] += 1.0", "pw[0] += 2.0"))))
    expect_miss("nstates", lambda: _create(_base(nstates=2)))

    def other_mask():  # the same text, pmx_seq_eq not declared: the generated policy leaves it out
        m = _base()
        m.user_fns &= ~_abi.PMX_FN_SEQ_EQ
        return _create(m)

    expect_miss("functions mask", other_mask)
    _setenv(monkeypatch, PMX_DEBUG_JIT_OPTS="-DPMX_TEST_JIT_CACHE_KEY=1")
    expect_miss("PMX_DEBUG_JIT_OPTS", lambda: _create(_base()))
    _setenv(monkeypatch, PMX_DEBUG_JIT_OPTS=None)
    expect_miss("big-lists build", lambda: _ffi.check(L.pmx_debug_jit_compile_big_lists(warm.handle)))
    before = _stats()
    _ffi.check(L.pmx_debug_jit_compile_big_lists(warm.handle))  # (the model keeps its big-lists build: no second request)
    assert _stats() == before
    _create(_base())  # the unchanged model is still a hit
    after = _stats()
    assert after["compiles"] == before["compiles"] == 6 and after["mem_hits"] == before["mem_hits"] + 1


def test_failed_compile_is_not_cached_and_reports_its_log_every_time():
    _create(_base())
    entries = _stats()["entries"]
    bad = _base(tua.SEQ_SRC.replace("pw[0] += 1.0;", "pw[0] += 1.0 this is not C;"))
    for attempt in range(2):
        with pytest.raises(_abi.PmxError) as e:
            _create(bad)
        assert e.value.status == _abi.PMX_ERR_INVALID_ARGUMENT
        log = str(e.value).split("hiprtc could not compile the model source:\n", 1)[1]
        assert log.strip() and "error" in log, attempt
        assert _stats()["entries"] == entries
    assert _stats()["compiles"] == 3  # both attempts reached the compiler


def test_off_switch_compiles_every_time(monkeypatch):
    _setenv(monkeypatch, PMX_JIT_CACHE=0)
    _create(_base())
    _create(_base())
    s = _stats()
    assert s["compiles"] == 2 and (s["mem_hits"], s["disk_hits"], s["entries"], s["bytes"]) == (0, 0, 0, 0)


def test_least_recently_used_entry_is_evicted(monkeypatch):
    _setenv(monkeypatch, PMX_JIT_CACHE_ENTRIES=2)
    variants = [tua.SEQ_SRC, tua.SEQ_SRC.replace("pw[0] += 1.0", "pw[0] += 2.0"), tua.SEQ_SRC.replace("pw[0] += 1.0", "pw[0] += 3.0")]
    for src in variants:
        _create(_base(src))
        assert _stats()["entries"] <= 2
    assert _stats()["compiles"] == 3
    _create(_base(variants[2]))  # the newest is still there ...
    assert (_stats()["compiles"], _stats()["mem_hits"]) == (3, 1)
    _create(_base(variants[0]))  # ... the first one went out
    s = _stats()
    assert (s["compiles"], s["mem_hits"]) == (4, 1) and s["entries"] <= 2


def test_two_threads_asking_for_the_same_cold_model_compile_once():
    errors = []
    gate = threading.Barrier(2)

    def work():
        try:
            gate.wait()
            _create(_base())
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work) for _ in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    s = _stats()
    assert s["compiles"] == 1 and s["mem_hits"] == 1 and s["entries"] == 1


def test_counters_struct_is_answered_by_sizeof_struct_and_clear_zeroes_them():
    L = _ffi.lib()
    assert L.pmx_sizeof_struct(b"pmx_jit_cache_counters") == C.sizeof(_abi.pmx_jit_cache_counters) == 56
    assert L.pmx_jit_cache_stats(None) == _abi.PMX_ERR_INVALID_ARGUMENT
    _create(_base())
    assert _stats()["entries"] == 1
    runtime.jit_cache_clear()
    assert set(_stats().values()) == {0}


# --------------------------------------------------------------------------------------------- CPU: disk level
@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    """A cache directory written by one cold process, and that process's counters.  Tests work on copies."""
    d = tmp_path_factory.mktemp("jit_cache_seed") / "nested" / "cache"  # (created if missing, parents included)
    stats = _run_child("cpu", cache_dir=d)
    return d, stats


def _copy_of(seeded, tmp_path):
    d = tmp_path / "cache"
    shutil.copytree(seeded[0], d)
    return d


def test_disk_round_trip_between_processes(seeded, tmp_path):
    _, a = seeded
    assert (a["compiles"], a["disk_writes"], a["disk_hits"], a["disk_rejects"]) == (1, 1, 0, 0)
    d = _copy_of(seeded, tmp_path)
    b = _run_child("cpu", cache_dir=d)
    assert (b["compiles"], b["disk_hits"], b["disk_writes"], b["disk_rejects"]) == (0, 1, 0, 0)
    files = _cache_files(d)
    assert len(files) == 1 and files[0] == files[0].lower() and len(files[0].split(".")[0]) == 32
    int(files[0].split(".")[0], 16)  # named by the key in hex
    # the same process, second creation: memory answers before the disk is looked at
    c = _run_child("cpu2", cache_dir=d)
    assert (c["compiles"], c["disk_hits"], c["mem_hits"]) == (0, 1, 1)


@pytest.mark.parametrize("damage", ["truncated", "flipped_code_byte", "flipped_header_byte"])
def test_damaged_cache_file_is_rejected_and_rewritten(seeded, tmp_path, damage):
    d = _copy_of(seeded, tmp_path)
    (name,) = _cache_files(d)
    good = (d / name).read_bytes()
    if damage == "truncated":
        bad = good[: len(good) // 2]
    else:
        at = len(good) - len(good) // 3 if damage == "flipped_code_byte" else 36  # 36: inside the key-material length
        bad = good[:at] + bytes([good[at] ^ 0x40]) + good[at + 1:]
    (d / name).write_bytes(bad)
    s = _run_child("cpu", cache_dir=d)
    assert (s["disk_rejects"], s["compiles"], s["disk_writes"], s["disk_hits"]) == (1, 1, 1, 0)
    assert _cache_files(d) == [name]  # rewritten in place, no temporary left
    again = _run_child("cpu", cache_dir=d)
    assert (again["compiles"], again["disk_hits"], again["disk_rejects"]) == (0, 1, 0)


def test_cache_directory_that_is_a_regular_file_never_fails_a_model(tmp_path, monkeypatch):
    target = tmp_path / "cache"
    target.write_text("not a directory")
    _setenv(monkeypatch, PMX_JIT_CACHE_DIR=target)
    _create(_base())
    _create(_base())
    s = _stats()
    assert (s["compiles"], s["mem_hits"], s["disk_writes"], s["disk_hits"]) == (1, 1, 0, 0)
    runtime.jit_cache_clear(disk=True)  # nothing to remove, nothing to fail
    assert target.read_text() == "not a directory"


def test_cache_directory_without_write_permission_never_fails_a_model():
    """A 0555 directory.  The creation runs in a child that cannot write there whoever runs the suite: a uid-0 process
    ignores the mode bits, so the child gives its privileges up first (jit_cache_child.py cpu_readonly) - and checks
    itself, before it creates the model, that it cannot create a file in the directory."""
    target = tempfile.mkdtemp(prefix="pmx_jit_cache_ro_")  # (not under tmp_path: pytest's base directory is closed to other users)
    try:
        os.chmod(target, 0o555)
        s = _run_child("cpu_readonly", target, timeout=120)
        assert (s["compiles"], s["mem_hits"], s["disk_writes"], s["disk_hits"], s["disk_rejects"]) == (1, 1, 0, 0, 0)
        assert _cache_files(target) == []  # no file, no temporary
    finally:
        os.chmod(target, 0o755)
        shutil.rmtree(target)


def test_concurrent_cold_start_leaves_one_file_and_no_temporaries(tmp_path):
    d = tmp_path / "cache"
    procs = [subprocess.Popen(["timeout", "-k", "10", "120"] + _child_cmd("cpu"), cwd=ROOT, env=_child_env(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for _ in range(4)]
    outs = [p.communicate() for p in procs]
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, err[-4000:]
    stats = [json.loads(out.strip().splitlines()[-1]) for out, _ in outs]
    assert all(s["compiles"] + s["disk_hits"] == 1 and s["disk_rejects"] == 0 for s in stats)  # compiled it, or found it whole
    files = _cache_files(d)
    assert len(files) == 1 and files[0].endswith(".pmxjit")
    fifth = _run_child("cpu", cache_dir=d)
    assert (fifth["compiles"], fifth["disk_hits"]) == (0, 1)


def test_clear_with_disk_removes_only_the_caches_own_files(seeded, tmp_path, monkeypatch):
    d = _copy_of(seeded, tmp_path)
    (d / "README.txt").write_text("someone else's file")
    _setenv(monkeypatch, PMX_JIT_CACHE_DIR=d)
    _create(_base())
    assert _stats()["disk_hits"] == 1
    runtime.jit_cache_clear()  # memory only
    assert len(_cache_files(d)) == 2
    runtime.jit_cache_clear(disk=True)
    assert _cache_files(d) == ["README.txt"]
    _create(_base())
    s = _stats()
    assert (s["compiles"], s["disk_writes"]) == (1, 1) and len(_cache_files(d)) == 2


# --------------------------------------------------------------------------------------------- GPU
def _oracle_outputs(name):
    model, subs, th = child.gpu_cases()[name]
    flat = child.flat_with_observations(model, subs)
    pred, pst = oracle.predict(model, flat, th)
    batch, bst = oracle.predict_batch(model, flat, th[:child.N_SUBJECTS])
    ll, lst = oracle.loglik(model, flat, child.ERROR_MODELS, th)
    return {"pred": pred, "pred_status": pst, "batch": batch, "batch_status": bst, "ll": ll, "ll_status": lst}


# (prediction tolerance, log-likelihood tolerance) against the oracle: those of the existing closure tests for these
# models - test_user_analytical.py (1e-6, 1e-6), test_full_feature_parity.py RK4 (1e-9, 1e-8) and dopri5 at
# rtol = atol = 1e-8 (1e-6; that file has no dopri5 log-likelihood: _dopri5_ll_bound below).
TOLERANCES = {"analytical": (1e-6, 1e-6), "ode_rk4": (1e-9, 1e-8), "ode_dopri5": (1e-6, None)}


def _dopri5_ll_bound(want, e=1e-6):
    """What the prediction tolerance e allows the adaptive solver's log-likelihood to differ by, per (subject, support
    point), from the oracle's own numbers: sigma depends on the observation alone (additive assay model,
    sigma^2 = (c0 + c1 y)^2 + lambda^2), so a prediction f moved by at most e |f| moves its term (y - f)^2 / (2 sigma^2)
    by at most (|y - f| e |f| + (e f)^2 / 2) / sigma^2; summed over the subject's valued observations, plus 1e-9 of the
    sum for its rounding."""
    model, subs, _ = child.gpu_cases()["ode_dopri5"]
    flat = child.flat_with_observations(model, subs)
    y = flat.ev_value[flat.ev_kind == _abi.PMX_EV_OBSERVATION]
    off = flat.observation_offsets()
    sigma2 = (0.05 + 0.1 * y) ** 2 + 0.1 ** 2  # child.ERROR_MODELS
    f = want["pred"]
    term = np.where(np.isfinite(y)[:, None], (np.abs(y[:, None] - f) * e * np.abs(f) + 0.5 * (e * f) ** 2) / sigma2[:, None], 0.0)
    per_subject = np.stack([term[off[s]:off[s + 1]].sum(axis=0) for s in range(len(off) - 1)])
    return per_subject + 1e-9 * np.maximum(np.abs(want["ll"]), 1.0)


@pytest.mark.gpu
def test_code_loaded_from_disk_computes_the_same_numbers(tmp_path):
    cache, out_a, out_b = tmp_path / "cache", tmp_path / "a", tmp_path / "b"
    out_a.mkdir()
    out_b.mkdir()
    grid = {"PMX_TUNE_GRID_MIN_P": 1}  # 5 support points on the GRID kernels (the batch form is PAIR): both lane mappings
    a = _run_child("gpu", out_a, cache_dir=cache, timeout=240, **grid)
    assert (a["compiles"], a["disk_writes"], a["disk_hits"]) == (2, 2, 0)  # RK4 and dopri5 share one translation unit
    b = _run_child("gpu", out_b, cache_dir=cache, timeout=120, **grid)
    assert (b["compiles"], b["disk_hits"], b["disk_rejects"]) == (0, 2, 0)
    assert len(_cache_files(cache)) == 2
    for name, (tol_pred, tol_ll) in TOLERANCES.items():
        kernels = json.loads((out_b / f"{name}_kernels.json").read_text())
        assert kernels == json.loads((out_a / f"{name}_kernels.json").read_text())
        assert kernels[0].startswith("pmx_jit_") and kernels[0].endswith("_grid") and kernels[1].endswith("_pair"), kernels
        # the log-likelihood entry points carry their family's name: 5 support points with PMX_TUNE_GRID_MIN_P=1 = the GRID one
        assert kernels[2] == kernels[0], kernels
        assert all(("dopri5" in k) == (name == "ode_dopri5") for k in kernels), kernels
        family = {"analytical": "pmx_jit_analytical", "ode_rk4": "pmx_jit_ode_user_rk4", "ode_dopri5": "pmx_jit_ode_user_dopri5"}[name]
        assert kernels == [family + "_grid", family + "_pair", family + "_grid"], kernels
        want = _oracle_outputs(name)
        for key in ("pred", "pred_status", "batch", "batch_status", "ll", "ll_status"):
            got_a, got_b = np.load(out_a / f"{name}_{key}.npy"), np.load(out_b / f"{name}_{key}.npy")
            assert got_a.tobytes() == got_b.tobytes(), (name, key)  # bit for bit
            w = want[key]
            assert got_b.shape == w.shape, (name, key)
            if key.endswith("status"):
                np.testing.assert_array_equal(got_b, w)
            elif key == "ll":
                if tol_ll is None:
                    err, bound = np.abs(got_b - w), _dopri5_ll_bound(want)
                    print(f"{name} ll: max abs err {err.max():.3e} (smallest bound {bound.min():.1e})")
                    assert (err <= bound).all(), (name, err.max())
                else:
                    err = (np.abs(got_b - w) / np.maximum(np.abs(w), 1.0)).max()
                    print(f"{name} ll: max err {err:.3e} (bound {tol_ll:.1e})")
                    assert err < tol_ll, (name, err)
            else:
                assert np.isfinite(w).all() and np.isfinite(got_b).all()
                err = (np.abs(got_b - w) / np.maximum(np.abs(w), 1e-12 * np.abs(w).max() + 1e-300)).max()
                print(f"{name} {key}: max rel err {err:.3e} (bound {tol_pred:.1e})")
                assert err <= tol_pred, (name, key, err)


@pytest.mark.gpu
def test_memory_hit_across_models_predicts_the_same_bits():
    import torch

    model, subs, th = child.gpu_cases()["analytical"]
    flat = child.flat_with_observations(model, subs)
    pop = runtime.DevicePopulation(flat, 0)
    outs = []
    for k in range(2):
        before = _stats()
        dm = _create(model)
        after = _stats()
        assert (after["compiles"] - before["compiles"], after["mem_hits"] - before["mem_hits"]) == ((1, 0) if k == 0 else (0, 1))
        pred, st = runtime.predict(dm, pop, np.ascontiguousarray(th))
        torch.cuda.synchronize()
        outs.append((pred.cpu().numpy(), st.cpu().numpy()))
        del dm  # pmx_model_destroy: its module is unloaded, the cache keeps the code object
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and np.isfinite(outs[0][0]).all()
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    want, _ = oracle.predict(model, flat, th)
    assert (np.abs(outs[1][0] - want) / np.abs(want)).max() <= 1e-6
