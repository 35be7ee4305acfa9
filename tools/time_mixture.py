#!/usr/bin/env python3
"""Time the mixture log-likelihood and D-function reductions at C3 size and write profiles/mixture_reductions.txt.

One process, one device: 100 000 subjects x 1000 support points for the mixture, x 3000 candidates for the D-function
(NPOD's 1000 simplices of three vertices).  After warm-up every variant is timed with device events, the variants of a
comparison alternating inside the process, `--reps` repetitions each (default 20); the file gives median, fastest,
slowest and the spread (slowest - fastest) of each.

  kernels     pmx_mixture_loglik_device   vs  torch.logsumexp(ll + w.log(), 1)           on the same device tensor
              pmx_dfunction_device        vs  (ll - lpyl[:, None]).exp().sum(0) - S      (what a caller of the parent
                                                                                          commit can do)
  host forms  pmx_mixture_loglik          vs  pmx_loglik into page-locked memory + the numpy reduction
              pmx_dfunction               vs  the same                                    (1000 candidates; host clock)

"done" for a kernel: no slower than its torch baseline beyond the baseline's own run-to-run spread.  Beside each kernel
the file states bytes read / time and, as context only, the flat-fill rate of pmx_measure_write_ceiling: no read
ceiling has been measured in this project, so no share of a peak is quoted.

usage: tools/time_mixture.py [--subjects N] [--support P] [--cand C] [--reps R] [--host-reps H] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return (f"median {statistics.median(ms):8.3f} ms   fastest {min(ms):8.3f}   slowest {max(ms):8.3f}   "
            f"spread {max(ms) - min(ms):7.3f}   n={len(ms)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subjects", type=int, default=100_000)
    ap.add_argument("--support", type=int, default=1000)
    ap.add_argument("--cand", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture_reductions.txt"))
    args = ap.parse_args()

    import torch

    from pharmsol_amd import AssayErrorModel, AssayErrorModels, ErrorPoly, _abi, _ffi, runtime, synth

    assert torch.cuda.is_available(), "tools/time_mixture.py measures on a GPU; there is no fallback"
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    S, P, NC = args.subjects, args.support, args.cand
    lines = [f"tools/time_mixture.py --subjects {S} --support {P} --cand {NC} --reps {args.reps} --host-reps {args.host_reps}",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # the population, with 'measured' values as bench.py --loglik makes them
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
    theta_c = synth.theta_c3(NC)
    w = torch.full((P,), 1.0 / P, dtype=torch.float64, device=dev)
    ll, _ = runtime.loglik(model, pop, em, theta, want_status=False)
    ll_c, _ = runtime.loglik(model, pop, em, theta_c, want_status=False)
    lpyl = runtime.mixture_loglik(pop, ll, w)
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

    # ---- kernels
    gbs = C.c_double()
    fill = torch.empty((S * P,), dtype=torch.float64, device=dev)
    _ffi.check(L.pmx_measure_write_ceiling(fill.data_ptr(), fill.numel(), 10, torch.cuda.current_stream(dev).cuda_stream,
                                           C.byref(gbs)))
    del fill
    say(f"flat-fill rate (pmx_measure_write_ceiling, {S * P * 8 / 1e6:.0f} MB): {gbs.value:.0f} GB/s - context only; a read "
        "ceiling: not measured")
    say()
    out_l = torch.empty((S,), dtype=torch.float64, device=dev)
    ms = alternate({"kernel": lambda: runtime.mixture_loglik(pop, ll, w, out=out_l),
                    "torch": lambda: torch.logsumexp(ll + w.log(), 1)}, args.reps)
    say(f"mixture log-likelihood, ll [{S} x {P}] on the device")
    say(f"  pmx_mixture_loglik_device          {summary(ms['kernel'])}")
    say(f"  torch.logsumexp(ll + w.log(), 1)   {summary(ms['torch'])}")
    say(f"  kernel: {S * P * 8 / 1e9:.2f} GB read / median = {S * P * 8 / 1e6 / statistics.median(ms['kernel']):.0f} GB/s")
    want = torch.logsumexp(ll + w.log(), 1)
    say(f"  largest difference between the two: {float((out_l - want).abs().max()):.3e}")
    say()
    out_d = torch.empty((NC,), dtype=torch.float64, device=dev)
    ms = alternate({"kernel": lambda: runtime.d_function(pop, ll_c, lpyl, out=out_d),
                    "torch": lambda: (ll_c - lpyl[:, None]).exp().sum(0) - S}, args.reps)
    say(f"D-function, ll [{S} x {NC}] on the device (two launches and the slab allocation included)")
    say(f"  pmx_dfunction_device                        {summary(ms['kernel'])}")
    say(f"  (ll - lpyl[:, None]).exp().sum(0) - S       {summary(ms['torch'])}")
    say(f"  kernel: {S * NC * 8 / 1e9:.2f} GB read / median = {S * NC * 8 / 1e6 / statistics.median(ms['kernel']):.0f} GB/s")
    want = (ll_c - lpyl[:, None]).exp().sum(0) - S
    say(f"  largest relative difference between the two: {float(((out_d - want).abs() / want.abs().clamp_min(1.0)).max()):.3e}")
    say()
    del ll_c, want

    # ---- host forms (host clock around calls that end synchronised), P columns both times
    dm = runtime._as_model(model)
    emp = C.cast(em.to_c(model), C.c_void_p)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    w_h = np.full(P, 1.0 / P)
    ll_h = runtime.host_empty((S, P))
    lpyl_h, d_h = np.empty(S), np.empty(P)

    def parent_mixture():
        _ffi.check(L.pmx_loglik(dm.handle, pop.handle, emp, th.ctypes.data, P, ll_h.ctypes.data, P, None))
        t = time.perf_counter()
        m = ll_h.max(axis=1)
        r = m + np.log(np.exp(ll_h - m[:, None]) @ w_h)
        return r, time.perf_counter() - t

    def parent_d(lp):
        _ffi.check(L.pmx_loglik(dm.handle, pop.handle, emp, th.ctypes.data, P, ll_h.ctypes.data, P, None))
        t = time.perf_counter()
        r = np.exp(ll_h - lp[:, None]).sum(axis=0) - S
        return r, time.perf_counter() - t

    def new_mixture():
        _ffi.check(L.pmx_mixture_loglik(dm.handle, pop.handle, emp, th.ctypes.data, P, w_h.ctypes.data, lpyl_h.ctypes.data, None))

    def new_d():
        _ffi.check(L.pmx_dfunction(dm.handle, pop.handle, emp, th.ctypes.data, P, lpyl_h.ctypes.data, d_h.ctypes.data, None))

    for _ in range(2):
        parent_mixture(), new_mixture(), parent_d(lpyl_h), new_d()
    t_parent, t_numpy, t_new = {"mix": [], "d": []}, {"mix": [], "d": []}, {"mix": [], "d": []}
    for _ in range(args.host_reps):
        for key, parent, new in (("mix", parent_mixture, new_mixture), ("d", lambda: parent_d(lpyl_h), new_d)):
            t = time.perf_counter()
            _, t_np = parent()
            t_parent[key].append((time.perf_counter() - t) * 1e3)
            t_numpy[key].append(t_np * 1e3)
            t = time.perf_counter()
            new()
            t_new[key].append((time.perf_counter() - t) * 1e3)
    say(f"host forms, theta [{P} x 4] in, {S} resp. {P} doubles out (host clock, calls end synchronised)")
    say(f"  pmx_mixture_loglik                                  {summary(t_new['mix'])}")
    say(f"  pmx_loglik into page-locked memory + numpy          {summary(t_parent['mix'])}")
    say(f"      of which the numpy reduction                    {summary(t_numpy['mix'])}")
    say(f"  pmx_dfunction                                       {summary(t_new['d'])}")
    say(f"  pmx_loglik into page-locked memory + numpy          {summary(t_parent['d'])}")
    say(f"      of which the numpy reduction                    {summary(t_numpy['d'])}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
