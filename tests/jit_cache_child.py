"""A cold process for tests/test_jit_cache.py: `python -m tests.jit_cache_child <mode> [outdir]`.

  cpu   create the small closure model once (hiprtc needs no device; no GPU is opened)
  cpu2  create it twice
  cpu_readonly DIR
        create it twice with DIR (mode 0555) as the cache directory, as a user who cannot write there: a process
        running as uid 0 writes anywhere, so it first becomes an unprivileged user (the library and every module are
        loaded before that, the checkout need not be readable afterwards)
  gpu   create the covariate closure model and the full-feature ODE model (RK4 and dopri5), run every cached entry
        point on 3 subjects x 5 support points and write the outputs as .npy files into outdir

The last line printed is the cache's counters as JSON."""
import json
import os
import sys

import numpy as np

from pharmsol_amd import AssayErrorModel, AssayErrorModels, Data, ErrorPoly, _abi, _ffi, runtime
from tests import test_full_feature_parity as ffp
from tests import test_user_analytical as tua

N_SUBJECTS, N_SUPPORT = 3, 5
# the error model of the existing closure log-likelihood tests (test_user_analytical.py, test_full_feature_parity.py)
ERROR_MODELS = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.05, 0.1, 0.0, 0.0), 0.1))


def gpu_cases():
    """name -> (model, subjects, support points): at most 6 events per subject."""

    def trimmed(subject, keep_obs):  # the fixtures' subjects with their first observations only
        occ = subject.occasions[0]
        seen, events = 0, []
        for ev in occ.events:
            if hasattr(ev, "outeq"):
                seen += 1
                if seen > keep_obs:
                    continue
            events.append(ev)
        occ.events = events
        return subject

    rng = np.random.default_rng(41)
    an = tua.covariate_model()
    an_subs = [trimmed(tua.covariate_subject(i, 1.0 + 0.05 * i), 4) for i in range(N_SUBJECTS)]  # bolus + infusion + 4 obs
    an_th = tua._theta_around(tua.COVARIATE_THETA, N_SUPPORT, rng)
    ode_subs = [trimmed(ffp.ode_subject(i, 1.0 + 0.05 * i), 3) for i in range(N_SUBJECTS)]  # 2 boluses + infusion + 3 obs
    ode_th = ffp._theta_around(ffp.ODE_THETA, N_SUPPORT, rng)
    return {
        "analytical": (an, an_subs, an_th),
        "ode_rk4": (ffp.ode_macro_model(), ode_subs, ode_th),
        "ode_dopri5": (ffp.ode_macro_model().with_solver("dopri5").with_tolerances(1e-8, 1e-8), ode_subs, ode_th),
    }


def observed_values(n_obs):
    """Observation values for the log-likelihood (fixed, positive, one missing)."""
    vals = 0.5 + 0.25 * np.arange(n_obs, dtype=np.float64)
    vals[1] = np.nan
    return vals


def flat_with_observations(model, subs):
    flat = model.flatten(Data(subs))
    obs = flat.ev_kind == _abi.PMX_EV_OBSERVATION
    flat.ev_value = flat.ev_value.copy()
    flat.ev_value[obs] = observed_values(int(obs.sum()))
    return flat


def run_gpu(outdir):
    import torch

    for name, (model, subs, th) in gpu_cases().items():
        flat = flat_with_observations(model, subs)
        pop = runtime.DevicePopulation(flat, 0)
        th = np.ascontiguousarray(th)
        kernels = []
        pred, st = runtime.predict(model, pop, th)
        kernels.append(runtime.last_kernel_name())
        batch, bst = runtime.predict(model, pop, np.ascontiguousarray(th[:N_SUBJECTS]), batch=True)
        kernels.append(runtime.last_kernel_name())
        ll, lst = runtime.loglik(model, pop, ERROR_MODELS, th)
        kernels.append(runtime.last_kernel_name())
        torch.cuda.synchronize()
        for key, t in (("pred", pred), ("pred_status", st), ("batch", batch), ("batch_status", bst), ("ll", ll), ("ll_status", lst)):
            np.save(os.path.join(outdir, f"{name}_{key}.npy"), t.cpu().numpy())
        with open(os.path.join(outdir, f"{name}_kernels.json"), "w") as f:
            json.dump(kernels, f)


def small_model():
    return tua.seq_model()


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode in ("cpu", "cpu2"):
        for _ in range(2 if mode == "cpu2" else 1):
            runtime.DeviceModel(small_model())
    elif mode == "cpu_readonly":
        target = sys.argv[2]
        runtime.jit_cache_stats()  # (loads the library)
        model = small_model()
        if os.geteuid() == 0:
            os.setgroups([])
            os.setgid(65534)
            os.setuid(65534)
        # the premise, checked and not assumed: the directory can be entered and read, nothing can be created in it
        assert os.access(target, os.R_OK | os.X_OK) and not os.access(target, os.W_OK), "the directory is writable"
        try:
            os.close(os.open(os.path.join(target, "probe"), os.O_WRONLY | os.O_CREAT | os.O_EXCL, 0o600))
            raise SystemExit("a file could be created in the read-only directory")
        except PermissionError:
            pass
        os.environ["PMX_JIT_CACHE_DIR"] = target
        _ffi.lib().pmx_debug_reload_env()
        for _ in range(2):
            runtime.DeviceModel(model)
    elif mode == "gpu":
        run_gpu(sys.argv[2])
    else:
        raise SystemExit(f"unknown mode {mode}")
    print(json.dumps(runtime.jit_cache_stats()))
