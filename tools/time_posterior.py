#!/usr/bin/env python3
"""Time the posterior and the prediction summaries at C3 size and write profiles/posterior_summaries.txt.

One process, one device: 100 000 subjects x 7 observations = 700 000 prediction rows x 1000 support points (5.6 GB).
After warm-up every variant is timed with device events, the two sides of a comparison alternating inside the process,
`--reps` repetitions each (default 20); the file gives median, fastest, slowest and the spread of each.

  kernels     pmx_summarize_predictions_device, population mode, mean only     vs  pred @ w / w.sum()
              ... posterior mode, mean only                                     vs  (q[subject_of_row] * pred).sum(1) / q.sum(1)[subject_of_row]
              ... both modes, mean + median                                     beside pmx_predict_device on the same matrix
              pmx_posterior_device
  host form   pmx_summarize_predictions, both modes, mean + median (host clock, calls end synchronised)

Beside each mean-only kernel the file states bytes read / time, and beside that the read rate pmx_dfunction_device
reaches in profiles/mixture_reductions.txt (4423 GB/s): mean-only is a pure read stream like it.

usage: tools/time_posterior.py [--subjects N] [--support P] [--reps R] [--host-reps H] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DFUNCTION_READ_GBS = 4423.0  # profiles/mixture_reductions.txt


def summary(ms):
    return (f"median {statistics.median(ms):8.3f} ms   fastest {min(ms):8.3f}   slowest {max(ms):8.3f}   "
            f"spread {max(ms) - min(ms):7.3f}   n={len(ms)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=100_000)
    ap.add_argument("--support", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_summaries.txt"))
    args = ap.parse_args()

    import torch

    from pharmsol_amd import AssayErrorModel, AssayErrorModels, ErrorPoly, _abi, _ffi, runtime, synth

    assert torch.cuda.is_available(), "tools/time_posterior.py measures on a GPU; there is no fallback"
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    S, P = args.subjects, args.support
    lines = [f"tools/time_posterior.py --subjects {S} --support {P} --reps {args.reps} --host-reps {args.host_reps}",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # the population, with 'measured' values as tools/time_mixture.py makes them
    model, flat, theta = synth.config_c3(S, P)
    pop0 = runtime.DevicePopulation(flat, 0)
    p0, _ = runtime.predict(model, pop0, theta[:1])
    torch.cuda.synchronize()
    rng = synth.SplitMix64(synth.SEED ^ 0x11)
    vals = np.abs(p0.cpu().numpy()[:, 0]) * np.exp(0.2 * (rng.uniform(pop0.n_observations) - 0.5)) + 0.05
    flat.ev_value = flat.ev_value.copy()
    flat.ev_value[flat.ev_kind == _abi.PMX_EV_OBSERVATION] = vals
    del pop0, p0
    em = AssayErrorModels.empty().add(0, AssayErrorModel.additive(ErrorPoly(0.05, 0.1, 0.0, 0.0), 0.1))
    pop = runtime.DevicePopulation(flat, 0)
    n = pop.n_observations
    w = torch.full((P,), 1.0 / P, dtype=torch.float64, device=dev)
    d_theta = torch.as_tensor(theta, device=dev)
    pred, _ = runtime.predict(model, pop, d_theta, want_status=False)
    ll, _ = runtime.loglik(model, pop, em, d_theta, want_status=False)
    lpyl = runtime.mixture_loglik(pop, ll, w)
    off = np.zeros(S + 1, dtype=np.int64)
    _ffi.check(L.pmx_population_observation_offsets(pop.handle, off.ctypes.data))
    subject_of_row = torch.as_tensor(np.repeat(np.arange(S), np.diff(off)), device=dev)
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def alternate(variants, reps):
        for fn in variants.values():  # warm-up: code objects, torch's allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                ms[k].append(timed(fn))
        return ms

    def rate(n_bytes, ms):
        return (f"{n_bytes / 1e9:.2f} GB read / median = {n_bytes / 1e6 / statistics.median(ms):.0f} GB/s "
                f"(pmx_dfunction_device, profiles/mixture_reductions.txt: {DFUNCTION_READ_GBS:.0f} GB/s)")

    say(f"pred [{n} x {P}], ll [{S} x {P}] on the device; every kernel call includes the torch.empty of its outputs")
    say()
    # ---- population mode
    ms = alternate({"kernel": lambda: runtime.summarize_predictions(pop, pred, w, median=False),
                    "torch": lambda: pred @ w / w.sum(),
                    "both": lambda: runtime.summarize_predictions(pop, pred, w),
                    "predict": lambda: runtime.predict(model, pop, d_theta, pred=pred, want_status=False)}, args.reps)
    say("population mode")
    say(f"  pmx_summarize_predictions_device, mean only       {summary(ms['kernel'])}")
    say(f"  pred @ w / w.sum()                                {summary(ms['torch'])}")
    say(f"  mean only: {rate(n * P * 8, ms['kernel'])}")
    say(f"  torch / kernel (medians): {statistics.median(ms['torch']) / statistics.median(ms['kernel']):.2f}")
    say(f"  pmx_summarize_predictions_device, mean + median   {summary(ms['both'])}")
    say(f"  pmx_predict_device, the same matrix               {summary(ms['predict'])}")
    got = runtime.summarize_predictions(pop, pred, w, median=False)[0]
    want = pred @ w / w.sum()
    say(f"  largest relative difference kernel / torch mean: {float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()):.3e}")
    say()
    # ---- posterior mode
    q = runtime.posterior(pop, ll, w, lpyl)

    def torch_posterior_mean():
        return (q[subject_of_row] * pred).sum(1) / q.sum(1)[subject_of_row]

    ms = alternate({"kernel": lambda: runtime.summarize_predictions(pop, pred, w, ll, lpyl, median=False),
                    "torch": torch_posterior_mean,
                    "both": lambda: runtime.summarize_predictions(pop, pred, w, ll, lpyl),
                    "posterior": lambda: runtime.posterior(pop, ll, w, lpyl, out=q)}, args.reps)
    say("posterior mode")
    say(f"  pmx_summarize_predictions_device, mean only       {summary(ms['kernel'])}")
    say(f"  (q[subject_of_row] * pred).sum(1) / q.sum(1)[..]  {summary(ms['torch'])}   (q given)")
    say(f"  mean only: {rate((n + S) * P * 8, ms['kernel'])}")
    say(f"  torch / kernel (medians): {statistics.median(ms['torch']) / statistics.median(ms['kernel']):.2f}")
    say(f"  pmx_summarize_predictions_device, mean + median   {summary(ms['both'])}")
    say(f"  pmx_posterior_device                              {summary(ms['posterior'])}")
    got = runtime.summarize_predictions(pop, pred, w, ll, lpyl, median=False)[0]
    want = torch_posterior_mean()
    say(f"  largest relative difference kernel / torch mean: {float(((got - want).abs() / want.abs().clamp_min(1e-300)).max()):.3e}")
    say()
    del q, want, got

    # ---- host form (host clock around calls that end synchronised)
    dm = runtime._as_model(model)
    emp = C.cast(em.to_c(model), C.c_void_p)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    w_h = np.full(P, 1.0 / P)
    mean_h, median_h = runtime.host_empty((n,)), runtime.host_empty((n,))

    def host(e, med):
        _ffi.check(L.pmx_summarize_predictions(dm.handle, pop.handle, e, th.ctypes.data, P, w_h.ctypes.data, mean_h.ctypes.data,
                                               median_h.ctypes.data if med else None, None))

    t_host = {}
    for key, e, med in (("population, mean", None, False), ("population, mean + median", None, True),
                        ("posterior, mean", emp, False), ("posterior, mean + median", emp, True)):
        for _ in range(2):
            host(e, med)
        t_host[key] = []
        for _ in range(args.host_reps):
            t = time.perf_counter()
            host(e, med)
            t_host[key].append((time.perf_counter() - t) * 1e3)
    say(f"host form pmx_summarize_predictions, theta [{P} x 4] in, {n} doubles out per output (host clock; predict, and in")
    say("posterior mode loglik and the mixture rows, included)")
    for key, ms_h in t_host.items():
        say(f"  {key:<28} {summary(ms_h)}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
