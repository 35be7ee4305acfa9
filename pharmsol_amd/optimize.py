"""``ParameterOptimizer`` (optimize/parameters.rs): the D-function of candidate support points as a cost, and the short
Nelder-Mead refinement NPOD runs on every support point - here on many points at once.

The reference evaluates ``cost`` one point at a time: one ``log_likelihood_matrix`` of one column, ``exp``, a division
by ``pyl`` per subject.  Here ``costs`` takes any number of points: one ``loglik`` launch writes their columns and one
``d_function`` reduces them on the device, in the log domain (``exp(ll - ln pyl)``: the same quantity, finite where
``exp(ll)`` and ``pyl`` both underflow).  ``optimize_points`` advances the simplices of all its points in lock-step, so
that an iteration costs at most three such launches however many points there are.

Deviations from the reference, both deliberate:
  * a NaN cost (a failed pair, e.g. a complex-root vertex) counts as ``+inf``, so that a simplex moves away from it; the
    reference's ``?`` would abort the whole run;
  * the Nelder-Mead steps are the standard ones (Lagarias et al. 1998) with the reference's settings; ``argmin``, whose
    step order the reference inherits, is not vendored with it, so step-for-step parity is not pinned.
"""
from __future__ import annotations

import numpy as np

from . import runtime

ALPHA, GAMMA, RHO, SIGMA = 1.0, 2.0, 0.5, 0.5  # reflection, expansion, contraction, shrink
MAX_ITERS = 5        # Executor::configure(|state| state.max_iters(5)), parameters.rs:82
SD_TOLERANCE = 1e-2  # NelderMead::with_sd_tolerance(1e-2), parameters.rs:80


def create_initial_simplex(point) -> np.ndarray:
    """``create_initial_simplex`` (parameters.rs:89-109): ``[k + 1, k]``, the point itself, then one vertex per
    coordinate moved by 0.8 % of its value (by 0.00025 where the coordinate is zero)."""
    point = np.asarray(point, dtype=np.float64).reshape(-1)
    vertices = np.tile(point, (point.size + 1, 1))
    for i in range(point.size):
        perturbation = 0.00025 if point[i] == 0.0 else 0.008 * point[i]
        vertices[i + 1, i] += perturbation
    return vertices


def _sample_sd(f: np.ndarray) -> np.ndarray:
    """Sample standard deviation of each row; not finite where a cost is infinite (such a simplex is never converged)."""
    with np.errstate(invalid="ignore"):
        return np.std(f, axis=1, ddof=1)


class ParameterOptimizer:
    def __init__(self, model, pop, error_models, pyl=None, *, log_pyl=None):
        """``pop``: a ``runtime.DevicePopulation``.  Exactly one of ``pyl`` - the mixture likelihood per subject as the
        reference passes it, its logarithm taken once here - and ``log_pyl`` (``runtime.mixture_loglik``'s output, a torch
        CUDA tensor or an array)."""
        import torch

        if (pyl is None) == (log_pyl is None):
            raise ValueError("pass exactly one of pyl and log_pyl")
        if pyl is not None:
            with np.errstate(divide="ignore", invalid="ignore"):
                log_pyl = np.log(np.asarray(pyl, dtype=np.float64))
        self.model, self.pop, self.error_models = model, pop, error_models
        self.log_pyl = runtime._device_vector(log_pyl, pop.n_subjects, torch.device("cuda", pop.device))
        self.n_cost_calls = 0  # launches of `costs` so far

    def costs(self, thetas):
        """``-D`` of every row of ``thetas [n, k]``: a torch CUDA tensor ``[n]``, not synchronised.  One ``loglik`` launch
        and one ``d_function``; a row with a failed pair costs NaN."""
        import torch

        thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        assert thetas.ndim == 2
        ll, status = runtime.loglik(self.model, self.pop, self.error_models, thetas)
        d = runtime.d_function(self.pop, ll, self.log_pyl)
        self.n_cost_calls += 1
        return torch.where((status != 0).any(dim=0), torch.full_like(d, float("nan")), -d)

    def cost(self, parameters) -> float:
        """``CostFunction::cost`` (parameters.rs:30-52) of one point."""
        return float(self.costs(np.asarray(parameters, dtype=np.float64).reshape(1, -1))[0])

    def _f(self, x: np.ndarray) -> np.ndarray:
        f = self.costs(x.reshape(-1, x.shape[-1])).cpu().numpy().reshape(x.shape[:-1])
        return np.where(np.isnan(f), np.inf, f)

    def optimize_points(self, points) -> np.ndarray:
        """``optimize_point`` (parameters.rs:78-86) of every row of ``points [n, k]``: ``[n, k]``, the best vertex of each
        simplex after at most 5 iterations, or fewer where the sample standard deviation of its costs falls below 1e-2."""
        points = np.ascontiguousarray(points, dtype=np.float64)
        assert points.ndim == 2
        n, k = points.shape
        x = np.stack([create_initial_simplex(p) for p in points])  # [n, k + 1, k]
        f = self._f(x)                                             # [n, k + 1]
        rows = np.arange(n)
        for _ in range(MAX_ITERS):
            order = np.argsort(f, axis=1, kind="stable")
            f = np.take_along_axis(f, order, axis=1)
            x = np.take_along_axis(x, order[:, :, None], axis=1)
            live = rows[~(_sample_sd(f) < SD_TOLERANCE)]
            if live.size == 0:
                break
            xl, fl = x[live], f[live]
            f1, fn, fw = fl[:, 0], fl[:, -2], fl[:, -1]
            xo = xl[:, :-1].mean(axis=1)
            xw = xl[:, -1]
            xr = xo + ALPHA * (xo - xw)
            fr = self._f(xr)
            expand = fr < f1
            outside = ~expand & (fr >= fn) & (fr < fw)
            inside = fr >= fw
            # the second point of every simplex that needs one: expansion, or a contraction on either side
            second = expand | outside | inside
            x2 = np.where(expand[:, None], xo + GAMMA * (xr - xo),
                          np.where(outside[:, None], xo + RHO * (xr - xo), xo + RHO * (xw - xo)))
            f2 = np.full(live.size, np.inf)
            if second.any():
                f2[second] = self._f(x2[second])
            take2 = (expand & (f2 < fr)) | (outside & (f2 <= fr)) | (inside & (f2 < fw))
            shrink = (outside | inside) & ~take2
            new_x = np.where(take2[:, None], x2, xr)
            new_f = np.where(take2, f2, fr)
            keep = ~shrink
            xl[keep, -1], fl[keep, -1] = new_x[keep], new_f[keep]
            if shrink.any():
                xs = xl[shrink]
                xs[:, 1:] = xs[:, :1] + SIGMA * (xs[:, 1:] - xs[:, :1])
                fs = fl[shrink]
                fs[:, 1:] = self._f(xs[:, 1:])
                xl[shrink], fl[shrink] = xs, fs
            x[live], f[live] = xl, fl
        best = np.argmin(f, axis=1)
        return x[rows, best]

    def optimize_point(self, parameters) -> np.ndarray:
        return self.optimize_points(np.asarray(parameters, dtype=np.float64).reshape(1, -1))[0]
