#!/usr/bin/env python3
"""Time the exposure metrics and the target attainment at C3 size and write profiles/exposure.txt.

One process, one device: 100 000 subjects x 7 observations = 100 000 profiles of 7 rows x 1000 support points, the
prediction matrix (5.6 GB) at the pitch pmx_recommended_ld gives.  After warm-up every variant is timed with device
events, the variants alternating inside the process, `--reps` repetitions each (default 20); the file gives median,
fastest, slowest and the spread of each.

  (a) pmx_exposure_device, linear, AUC + Cmax
  (b) pmx_exposure_device, lin-up/log-down, all six metrics
  (c) pmx_exposure_device, lin-log, AUC + Cmax
  (d) pmx_summarize_predictions_device, population mode, mean only: it reads the same matrix once and is the yardstick
      for a one-pass read
  (e) torch on the same tensors: AUC (linear) + Cmax of every profile
  (f) the host form pmx_exposure_attainment per call (host clock, calls end synchronised), population and posterior mode
and pmx_attainment_device on one plane.  Bytes over time for (a) to (d), and the ratios a / d and b / d.

usage: tools/time_exposure.py [--subjects N] [--support P] [--reps R] [--host-reps H] [--out FILE]"""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure.txt"))
    args = ap.parse_args()

    import torch

    from pharmsol_amd import AssayErrorModel, AssayErrorModels, ErrorPoly, _abi, _ffi, runtime, synth

    assert torch.cuda.is_available(), "tools/time_exposure.py measures on a GPU; there is no fallback"
    L = _ffi.lib()
    dev = torch.device("cuda", 0)
    S, P = args.subjects, args.support
    lines = [f"tools/time_exposure.py --subjects {S} --support {P} --reps {args.reps} --host-reps {args.host_reps}",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    # the population, with 'measured' values as tools/time_posterior.py makes them
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
    n, n_prof = pop.n_observations, pop.n_profiles
    rows = pop.profiles()[3]
    assert n_prof == S and (rows == rows[0]).all()
    R = int(rows[0])
    ld = runtime.recommended_ld(P)
    w = torch.full((P,), 1.0 / P, dtype=torch.float64, device=dev)
    d_theta = torch.as_tensor(theta, device=dev)
    pred_full = torch.empty((n, ld), dtype=torch.float64, device=dev)
    pred = pred_full[:, :P]
    runtime.predict(model, pop, d_theta, pred=pred, want_status=False)
    planes = torch.empty((6, n_prof, P), dtype=torch.float64, device=dev)
    t_obs = pop.observation_info()[0][:R]
    half_dt = torch.as_tensor(0.5 * np.diff(t_obs), device=dev)[None, :, None]
    thr = float(pred[: 7 * 1000].median())
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

    def torch_auc_cmax():
        v = pred_full.view(S, R, ld)[:, :, :P]
        return ((v[:, 1:] + v[:, :-1]) * half_dt).sum(1), v.amax(1)

    all_six = runtime.EXPOSURE_METRICS.keys()
    variants = {
        "a": lambda: runtime.exposure(pop, pred, metrics=("auc", "cmax"), method="linear", out=planes[:2]),
        "b": lambda: runtime.exposure(pop, pred, metrics=all_six, method="lin_up_log_down", threshold=thr, out=planes),
        "c": lambda: runtime.exposure(pop, pred, metrics=("auc", "cmax"), method="lin_log", out=planes[:2]),
        "d": lambda: runtime.summarize_predictions(pop, pred, w, median=False),
        "e": torch_auc_cmax,
    }
    ms = alternate(variants, args.reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    read, plane_bytes = n * P * 8, n_prof * P * 8

    def rate(k, written):
        return f"{(read + written) / 1e9:.2f} GB moved ({read / 1e9:.2f} read) / median = {(read + written) / 1e6 / med[k]:.0f} GB/s"

    say(f"pred [{n} x {P}], rows {ld} doubles apart; {n_prof} profiles of {R} rows; planes [{n_prof} x {P}] dense; threshold {thr:.4g}")
    say()
    say(f"(a) pmx_exposure_device, linear, AUC + Cmax             {summary(ms['a'])}")
    say(f"    {rate('a', 2 * plane_bytes)}")
    say(f"(b) pmx_exposure_device, lin-up/log-down, six metrics   {summary(ms['b'])}")
    say(f"    {rate('b', 6 * plane_bytes)}")
    say(f"(c) pmx_exposure_device, lin-log, AUC + Cmax            {summary(ms['c'])}")
    say(f"    {rate('c', 2 * plane_bytes)}")
    say(f"(d) pmx_summarize_predictions_device, population, mean  {summary(ms['d'])}")
    say(f"    {rate('d', n * 8)}")
    say(f"(e) torch: trapezoid sum + amax over the profile rows   {summary(ms['e'])}")
    say(f"ratios of medians: a / d {med['a'] / med['d']:.2f}   b / d {med['b'] / med['d']:.2f}   c / d {med['c'] / med['d']:.2f}   "
        f"e / a {med['e'] / med['a']:.2f}")
    got = runtime.exposure(pop, pred, metrics=("auc", "cmax"), method="linear", out=planes[:2])
    want_auc, want_cmax = torch_auc_cmax()
    say(f"largest relative difference kernel / torch AUC: {float(((got['auc'] - want_auc).abs() / want_auc.abs().clamp_min(1e-300)).max()):.3e}; "
        f"Cmax equal: {bool((got['cmax'] == want_cmax).all())}")
    del want_auc, want_cmax
    say()

    # ---- attainment of one plane
    ll, _ = runtime.loglik(model, pop, em, d_theta, want_status=False)
    lpyl = runtime.mixture_loglik(pop, ll, w)
    auc = planes[0]
    target = auc.median(dim=1).values.contiguous()
    ms = alternate({"population": lambda: runtime.target_attainment(pop, auc, w, target, mean=True),
                    "posterior": lambda: runtime.target_attainment(pop, auc, w, target, ll, lpyl, mean=True)}, args.reps)
    say(f"pmx_attainment_device, pta + mean, population mode      {summary(ms['population'])}")
    say(f"pmx_attainment_device, pta + mean, posterior mode       {summary(ms['posterior'])}")
    say()

    # ---- host form (host clock around calls that end synchronised)
    dm = runtime._as_model(model)
    emp = C.cast(em.to_c(model), C.c_void_p)
    th = np.ascontiguousarray(theta, dtype=np.float64)
    w_h = np.full(P, 1.0 / P)
    tg_h = np.ascontiguousarray(target.cpu().numpy())
    pta_h, mean_h = runtime.host_empty((n_prof,)), runtime.host_empty((n_prof,))

    def host(e):
        _ffi.check(L.pmx_exposure_attainment(dm.handle, pop.handle, e, th.ctypes.data, P, w_h.ctypes.data, _abi.PMX_AUC_LINEAR,
                                             None, _abi.PMX_EXPO_AUC, tg_h.ctypes.data, pta_h.ctypes.data, mean_h.ctypes.data, None))

    say(f"(f) host form pmx_exposure_attainment, theta [{P} x 4] in, {n_prof} doubles out per output (host clock; predict, the")
    say("    exposure plane, and in posterior mode loglik and the mixture rows, included)")
    for key, e in (("population", None), ("posterior", emp)):
        for _ in range(2):
            host(e)
        ms_h = []
        for _ in range(args.host_reps):
            t = time.perf_counter()
            host(e)
            ms_h.append((time.perf_counter() - t) * 1e3)
        say(f"    {key:<12} {summary(ms_h)}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
