"""numpy statement of the zero-order term and the theta step (mgx_set_reaction, mgx_theta_steps; csrc/mgx_theta.hpp) on
top of tests/galerkin_ref.py: the shift c = c0 + d, the right-hand-side pass operation by operation, and the step loop
around any solver.  numpy rounds every elementwise operation on its own, which is what the kernels do, so the shift
and the pass are meant bit for bit in the operator's dtype.

An operator is a list of nine interior n x n arrays in the storage order c, n, s, w, e, nw, ne, sw, se (a five-point
one: gr.nine(st5))."""
import numpy as np

import galerkin_ref as gr


def shift(st9, d):
    """S = A0 + diag(d): slot 0 is c0 + d, one rounding in the operator's dtype; every other slot is A0's"""
    dt = st9[0].dtype
    return [st9[0] + np.asarray(d, dtype=dt)] + [np.array(a, copy=True) for a in st9[1:]]


def apply(st9, u):
    """(S u) in the kernels' order: CSR order, centre included, ring-pointing coefficients times the zero ring"""
    return gr._apply9(st9, st9[0], u)


def coefficients(theta, dtype):
    """(c1, c0) = (1 / theta, (1 - theta) / theta), formed in double and rounded to the working type once"""
    dt = np.dtype(dtype).type
    return dt(1.0 / float(theta)), dt((1.0 - float(theta)) / float(theta))


def rhs_pass(Su, u, d, g, theta):
    """the pass: m = d u;  theta = 1: b = m;  theta < 1: b = c1 m - c0 (S u);  then + g when g is given.  Su is (S u) in
    u's dtype (apply(), or minus the device's residual of u against a zero right-hand side); not read for theta = 1"""
    dt = u.dtype
    m = np.asarray(d, dtype=dt) * u
    if float(theta) == 1.0:
        b = m
    else:
        c1, c0 = coefficients(theta, dt)
        b = c1 * m - c0 * np.asarray(Su, dtype=dt)
    if g is not None:
        b = b + np.asarray(g, dtype=dt)
    return b


def steps(S9, d, u0, g, theta, nsteps, solve):
    """nsteps theta steps from u0 on S9 = shift(A0, d): u <- solve(rhs_pass(S u, u, d, g, theta), u), the solver
    warm-started with the previous time level; returns the list of the iterates after every step"""
    u = np.array(u0, copy=True)
    out = []
    for _ in range(nsteps):
        b = rhs_pass(None if float(theta) == 1.0 else apply(S9, u), u, d, g, theta)
        u = solve(b, u)
        out.append(u)
    return out


def dense_solver(S9):
    """solve(b, u) by a dense float64 factorisation of S (the guess is not used)"""
    M = gr.dense(S9)
    n = S9[0].shape[0]
    return lambda b, u: np.linalg.solve(M, np.asarray(b, dtype=np.float64).ravel()).reshape(n, n)


def poisson9(L, dtype=np.float64):
    """the nine arrays of the five-point Poisson stencil (a = 1 in mgx_set_coefficient) on level L"""
    n = (1 << L) - 1
    full = lambda v: np.full((n, n), v, dtype=dtype)
    return gr.nine([full(4.0), full(-1.0), full(-1.0), full(-1.0), full(-1.0)])


def sine_mode(L, k, l):
    """sin(k pi x) sin(l pi y) on the interior nodes of level L (x along a row), and its eigenvalue
    4 - 2 cos(k pi / N) - 2 cos(l pi / N) of the Poisson stencil"""
    N = 1 << L
    x = np.arange(1, N) / N
    lam = 4.0 - 2.0 * np.cos(k * np.pi / N) - 2.0 * np.cos(l * np.pi / N)
    return np.sin(l * np.pi * x)[:, None] * np.sin(k * np.pi * x)[None, :], lam
