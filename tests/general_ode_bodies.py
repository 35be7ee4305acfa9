"""User ODE bodies outside the compartmental class, for tests/golden/ode_exact_general.json: every body as the C text the
library compiles (hiprtc for the device, the host compiler for the oracle) and, side by side, as a Python twin that
tests/golden/gen_ode_exact_general.py evaluates in mpmath.  Importing this module needs neither the product nor the oracle.

What sets these bodies apart from every other ODE body of the suite: I - gamma h J is NOT a column-diagonally-dominant
M-matrix.  A state that grows (a positive diagonal entry of J), positive feedback and a predator-prey term give W a
diagonal entry that shrinks, vanishes or changes sign as h grows, while W itself stays well conditioned - elimination in
the natural order then loses digits that elimination with row exchanges keeps.

Twin conventions.  `rhs(t, x, p, rate)` and `jac(x, p)` use only + - * on what they are given, so the same text
evaluates in mpf (the generator's exact walk) and in Python doubles (the generator's check that a difference quotient is
exact in float64, and the float64 restatements of the step).  The order of operations is the C text's.

  feedback2        theta = [a, b, c, v, lag]            x0' = a x0 - b x1 + rateiv0,  x1' = b x0 - c x1;  output x1 / v
                   growth a > 0 in state 0, held stable by the feedback through state 1 (trace a - c < 0, det b^2 - a c > 0)
  feedback8_head   theta = [a, b, c, v, lag, kt, kd]    the pair at states 0-1 feeds a chain of six (transit kt, loss kd);
                   output x7 / v: the shrinking pivot is the FIRST of the 8 x 8 elimination
  feedback8_tail   theta = [a, b, c, v, lag, kt, kd]    the chain (states 0-5, dosed at 0) feeds the pair at states 6-7;
                   output x7 / v: the shrinking pivot is the SEVENTH, after six updates of the trailing block
  lotka2           theta = [g, k, e, d, v, x0(0), x1(0)]  x0' = g x0 - k x0 x1 + rateiv0,  x1' = e k x0 x1 - d x1 + rateiv1;
                   output x1 / v; J = [[g - k x1, -k x0], [e k x1, e k x0 - d]]: a positive diagonal entry, off-diagonal
                   entries of both signs, and it changes every step
Doses: input i goes to state i (the library's rule for an index-based user body); the lag of input 0 is theta[4] in the
feedback bodies."""
SIG = ("double t, const double* x, const double* p, const double* cov, const double* rateiv, "
       "const double* derived, double* ")

FEEDBACK2_SRC = f"""
PMX_DEVICE void pmx_dynamics({SIG}dx) {{
  dx[0] = p[0] * x[0] - p[1] * x[1] + rateiv[0];
  dx[1] = p[1] * x[0] - p[2] * x[1];
}}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[1] / p[3]; }}
"""

FEEDBACK8_HEAD_SRC = f"""
PMX_DEVICE void pmx_dynamics({SIG}dx) {{
  dx[0] = p[0] * x[0] - p[1] * x[1] + rateiv[0];
  dx[1] = p[1] * x[0] - p[2] * x[1];
  for (int i = 2; i < 8; ++i) dx[i] = p[5] * x[i - 1] - (p[5] + p[6]) * x[i];
}}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[7] / p[3]; }}
"""

FEEDBACK8_TAIL_SRC = f"""
PMX_DEVICE void pmx_dynamics({SIG}dx) {{
  dx[0] = rateiv[0] - (p[5] + p[6]) * x[0];
  for (int i = 1; i < 6; ++i) dx[i] = p[5] * x[i - 1] - (p[5] + p[6]) * x[i];
  dx[6] = p[0] * x[6] - p[1] * x[7] + p[5] * x[5];
  dx[7] = p[1] * x[6] - p[2] * x[7];
}}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[7] / p[3]; }}
"""

LOTKA2_SRC = f"""
PMX_DEVICE void pmx_dynamics({SIG}dx) {{
  dx[0] = p[0] * x[0] - p[1] * x[0] * x[1] + rateiv[0];
  dx[1] = p[2] * p[1] * x[0] * x[1] - p[3] * x[1] + rateiv[1];
}}
PMX_DEVICE void pmx_outputs({SIG}y) {{ y[0] = x[1] / p[4]; }}
PMX_DEVICE void pmx_init({SIG}xi) {{ xi[0] = p[5]; xi[1] = p[6]; }}
"""


def _feedback2_rhs(t, x, p, rate):
    return [p[0] * x[0] - p[1] * x[1] + rate[0], p[1] * x[0] - p[2] * x[1]]


def _feedback2_jac(x, p):
    return [[p[0], -p[1]], [p[1], -p[2]]]


def _head_rhs(t, x, p, rate):
    return ([p[0] * x[0] - p[1] * x[1] + rate[0], p[1] * x[0] - p[2] * x[1]]
            + [p[5] * x[i - 1] - (p[5] + p[6]) * x[i] for i in range(2, 8)])


def _head_jac(x, p):
    J = [[0 * p[0]] * 8 for _ in range(8)]
    J[0][0], J[0][1], J[1][0], J[1][1] = p[0], -p[1], p[1], -p[2]
    for i in range(2, 8):
        J[i][i - 1], J[i][i] = p[5], -(p[5] + p[6])
    return J


def _tail_rhs(t, x, p, rate):
    return ([rate[0] - (p[5] + p[6]) * x[0]] + [p[5] * x[i - 1] - (p[5] + p[6]) * x[i] for i in range(1, 6)]
            + [p[0] * x[6] - p[1] * x[7] + p[5] * x[5], p[1] * x[6] - p[2] * x[7]])


def _tail_jac(x, p):
    J = [[0 * p[0]] * 8 for _ in range(8)]
    J[0][0] = -(p[5] + p[6])
    for i in range(1, 6):
        J[i][i - 1], J[i][i] = p[5], -(p[5] + p[6])
    J[6][5], J[6][6], J[6][7], J[7][6], J[7][7] = p[5], p[0], -p[1], p[1], -p[2]
    return J


def _lotka2_rhs(t, x, p, rate):
    return [p[0] * x[0] - p[1] * x[0] * x[1] + rate[0], p[2] * p[1] * x[0] * x[1] - p[3] * x[1] + rate[1]]


def _lotka2_jac(x, p):
    return [[p[0] - p[1] * x[1], -p[1] * x[0]], [p[2] * p[1] * x[1], p[2] * p[1] * x[0] - p[3]]]


# `central`: the state whose amount / theta[v] is the output; `init`: state -> theta index (first occasion only)
BODIES = {
    "feedback2": dict(src=FEEDBACK2_SRC, nstates=2, nparams=5, ndrugs=1, central=1, v=3, lag={0: 4}, init={}, linear=True,
                      rhs=_feedback2_rhs, jac=_feedback2_jac, marker="p[1] * x[0] - p[2] * x[1]"),
    "feedback8_head": dict(src=FEEDBACK8_HEAD_SRC, nstates=8, nparams=7, ndrugs=1, central=7, v=3, lag={0: 4}, init={},
                           linear=True, rhs=_head_rhs, jac=_head_jac, marker="i = 2; i < 8"),
    "feedback8_tail": dict(src=FEEDBACK8_TAIL_SRC, nstates=8, nparams=7, ndrugs=1, central=7, v=3, lag={0: 4}, init={},
                           linear=True, rhs=_tail_rhs, jac=_tail_jac, marker="p[5] * x[5]"),
    "lotka2": dict(src=LOTKA2_SRC, nstates=2, nparams=7, ndrugs=2, central=1, v=4, lag={}, init={0: 5, 1: 6}, linear=False,
                   rhs=_lotka2_rhs, jac=_lotka2_jac, marker="p[2] * p[1] * x[0] * x[1]"),
}


GAMMA_D = 1.7071067811865475  # the library's kGamma and kSqrtEps
SQRT_EPS = 1.4901161193847656e-08


def ros2_doubles(f, t, x, h, tol, exchange):
    """One ROS2 try restated in Python doubles, operation by operation as DESIGN.md's "Stiff option" describes it (no
    fused multiply-add): f(t, x) -> list.  exchange = False: elimination in the natural order; True: with row exchanges
    (stage k brings the largest of column k's remaining entries up, by pairwise exchanges of the rows' remaining parts;
    the right-hand sides replay the exchanges stage by stage).  -> (new state, scaled error)."""
    n = len(x)
    gh = GAMMA_D * h
    f0 = f(t, x)
    W = [[0.0] * n for _ in range(n)]
    for j in range(n):
        xt = list(x)
        d = SQRT_EPS * max(abs(x[j]), 1.0)
        xt[j] = x[j] + d
        f1 = f(t, xt)
        s = -gh / d
        for i in range(n):
            W[i][j] = (f1[i] - f0[i]) * s + (1.0 if i == j else 0.0)
    dt = SQRT_EPS * max(abs(t), 1.0)
    f1 = f(t + dt, x)
    ft = [(f1[i] - f0[i]) * (gh / dt) for i in range(n)]
    swaps = []
    for k in range(n):
        for i in range(k + 1, n):
            swaps.append(exchange and abs(W[i][k]) > abs(W[k][k]))
            if swaps[-1]:
                for j in range(k, n):
                    W[k][j], W[i][j] = W[i][j], W[k][j]
        inv = 1.0 / W[k][k]
        for i in range(k + 1, n):
            l = W[i][k] * inv
            W[i][k] = l
            for j in range(k + 1, n):
                W[i][j] -= l * W[k][j]
        W[k][k] = inv

    def solve(b):
        it = iter(swaps)
        for k in range(n):
            for i in range(k + 1, n):
                if next(it):
                    b[k], b[i] = b[i], b[k]
            for i in range(k + 1, n):
                b[i] -= W[i][k] * b[k]
        for i in reversed(range(n)):
            for j in range(i + 1, n):
                b[i] -= W[i][j] * b[j]
            b[i] *= W[i][i]
        return b

    k1 = solve([f0[i] + ft[i] for i in range(n)])
    f1 = f(t + h, [x[i] + h * k1[i] for i in range(n)])
    k2 = solve([f1[i] - ft[i] - 2.0 * k1[i] for i in range(n)])
    xn = [x[i] + h * (1.5 * k1[i] + 0.5 * k2[i]) for i in range(n)]
    q = [(0.5 * h) * (k1[i] + k2[i]) / (tol + tol * max(abs(x[i]), abs(xn[i]))) for i in range(n)]
    return xn, (sum(v * v for v in q) / n) ** 0.5


def build(name, solver, h_max, rtol=None, atol=None):
    """The body as a library model (imports pharmsol_amd only here)."""
    from pharmsol_amd import ODE

    b = BODIES[name]
    m = ODE.custom(b["src"], nstates=b["nstates"], nparams=b["nparams"], ndrugs=b["ndrugs"], nout=1, has_init=bool(b["init"]),
                   lag=b["lag"] or None, h_max=h_max).with_solver(solver)
    return m if rtol is None else m.with_tolerances(rtol, atol)
