"""CPU checks of tests/newton_ref.py - the numpy statement tests/test_gpu_newton.py holds the device to - against the
formula per point and against mathematics (one step for a linear problem, quadratic convergence, the line search on an
input whose full step overshoots), and of the new entry points' argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import galerkin_ref as gr
import newton_ref as nf
import theta_ref as tr

INVALID = 1                                # MGX_ERR_INVALID


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_pass_operation_by_operation(dtype):
    """newton_pass against the formula written out per point in scalars of the working type (every product and sum
    rounded on its own), on a random nine-point operator, for the first evaluation and for a trial with lam = 1/4"""
    L = 4
    n = (1 << L) - 1
    rng = np.random.default_rng(5)
    rand = lambda lo, hi: rng.uniform(lo, hi, (n, n)).astype(dtype)
    A0 = [rand(3.0, 5.0)] + [rand(-1.0, -0.2) for _ in range(8)]
    kap, f, u, de = rand(0.1, 2.0), rand(-1.0, 1.0), rand(-1.0, 1.0), rand(-1.0, 1.0)
    p = (-0.7, 0.3, 1.1)
    T = np.dtype(dtype).type
    p1, p2, p3, q2, q3 = T(p[0]), T(p[1]), T(p[2]), T(2.0 * p[1]), T(3.0 * p[2])
    for lam in (None, 0.25):
        v, b, d = nf.newton_pass(A0, kap, f, p, u, None if lam is None else de, lam)
        vv = u if lam is None else np.array([[u[i, j] + T(lam) * de[i, j] for j in range(n)] for i in range(n)], dtype=dtype)
        assert np.array_equal(v, vv) and v.dtype == b.dtype == d.dtype == np.dtype(dtype)
        P = np.pad(vv, 1)
        for i, j in ((0, 0), (3, 7), (n - 1, n - 1)):
            q = None
            for dy, dx in gr.ROW_MAJOR:                        # NW, N, NE, W, C, E, SW, S, SE
                term = A0[gr.SLOT[dy, dx]][i, j] * P[1 + i + dy, 1 + j + dx]
                q = term if q is None else q + term
            x = vv[i, j]
            ph = ((p3 * x + p2) * x + p1) * x
            dp = (q3 * x + q2) * x + p1
            assert type(q) is T and type(ph) is T and type(dp) is T
            assert b[i, j] == f[i, j] - (q + kap[i, j] * ph), (lam, i, j)
            assert d[i, j] == kap[i, j] * dp, (lam, i, j)


def test_a_linear_problem_takes_one_full_step():
    """p = (0, 0, 0): F(u) = A0 u - f, d = 0, the Jacobian is A0 and one full step solves the problem: the residual of a
    direct solve is rounding, far below 1e-10 of the initial one"""
    L = 4
    n = (1 << L) - 1
    rng = np.random.default_rng(6)
    A0 = tr.poisson9(L)
    kap, f, u0 = rng.uniform(0.5, 2.0, (n, n)), rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    seen = []

    def solve(S9, b, d, k):
        seen.append((S9, b, d))
        return nf.direct_solve(S9, b)

    o = nf.newton(A0, kap, f, (0.0, 0.0, 0.0), u0, solve, 1e-10, 5, 4)
    assert len(seen) == 1 and not seen[0][2].any() and np.array_equal(seen[0][0][0], A0[0])
    assert np.array_equal(seen[0][1], f - tr.apply(A0, u0))
    assert o["converged"] and len(o["hist"]) == 2 and o["backtracks"] == 0 and list(o["lam"]) == [1.0]
    assert np.array_equal(o["u"], u0 + nf.direct_solve(A0, f - tr.apply(A0, u0))[0])


def test_convergence_is_quadratic():
    """L = 4, A0 = Poisson, kap = 1, phi = u^3, f manufactured from sin(pi x) sin(pi y), direct solves, a random guess of
    amplitude 10 (seed 0), tol = 1e-12: ten full steps, the last three with r_{k+1} / r_k^2 = 0.0590, 0.0773, 0.0804 (the
    residuals 7.8e-1, 3.6e-2, 1.0e-4, 8.0e-10; rounding of F is about 1e-14).  Quadratic convergence: the constant stays
    within a factor 2 of its previous value over the last two steps"""
    L = 4
    N = 1 << L
    n = N - 1
    x = np.arange(1, N) / N
    us = np.sin(np.pi * x)[:, None] * np.sin(np.pi * x)[None, :]
    A0, kap = tr.poisson9(L), np.ones((n, n))
    f = tr.apply(A0, us) + kap * us ** 3
    u0 = np.random.default_rng(0).uniform(-10.0, 10.0, (n, n))
    o = nf.newton(A0, kap, f, (0.0, 0.0, 1.0), u0, nf.direct_solve, 1e-12, 30, 10)
    h = o["hist"]
    assert o["converged"] and len(h) >= 5
    c = h[1:] / h[:-1] ** 2
    print("r_{k+1} / r_k^2:", c[-3:], "residuals:", h[-4:])
    for k in (-1, -2):
        assert 0.5 <= c[k] / c[k - 1] <= 2.0, (k, c)
    assert np.max(np.abs(o["u"] - us)) <= 1e-9             # (the discrete problem was manufactured: its solution is us)


@pytest.mark.parametrize("dtype, tol", [(np.float64, 1e-10), (np.float32, 1e-5)])
@pytest.mark.parametrize("L", [4, 5, 6])
def test_the_backtracking_input_backtracks_in_its_first_step_only(L, dtype, tol):
    """the input of the GPU line-search cases, on the reference alone with direct solves: the first step rejects at least
    one trial, no later step does, the run converges, and the Jacobian of every linear solve is positive definite - so the
    device cases cannot pass vacuously.  With max_backtracks = 2 the same input is the line-search failure"""
    A0, kap, f, p, u0 = nf.backtracking_input(L, dtype)
    o = nf.newton(A0, kap, f, p, u0, nf.direct_solve, tol, 20, 8)
    assert o["converged"] and not o["failed"]
    assert o["lam"][0] < 1.0 and (o["lam"][1:] == 1.0).all(), o["lam"]
    assert o["backtracks"] == round(-np.log2(o["lam"][0])) >= 1
    assert 4 <= len(o["lam"]) <= 6
    lmin = nf.poisson_lambda_min(L)
    eigs = [nf.smallest_eigenvalue(tr.shift(A0, d)) for d in o["ds"]]
    assert all(e > 0.0 for e in eigs), eigs
    assert abs(eigs[0] - 0.1 * lmin) <= 1e-3 * lmin, (eigs[0], lmin)       # (u0 is constant: the shift is exact but for rounding in the working type)
    short = nf.newton(A0, kap, f, p, u0, nf.direct_solve, tol, 20, 2)
    assert short["failed"] and not short["converged"] and short["backtracks"] == 3 and len(short["hist"]) == 1
    assert np.array_equal(short["u"], u0)


def test_null_handles_are_refused_without_a_device(pkg):
    """NULL handle (with and without opt) from both entry points: MGX_ERR_INVALID, every output left alone"""
    lib = pkg.lib()
    B = pkg.binding
    opt = B.NewtonOpts(0.0, 0.0, 1.0, pkg.STEP_SOLVE, 1e-8, 10, 4, 1e-10, 5, 4)
    kap = np.ones(9)
    ns = B.NewtonStats(iterations=-7, converged=-7, history_len=-7)
    st = (B.Stats * 5)()
    for s in st:
        s.cycles = -7
    lam, hist = np.full(5, -1.0), np.full(6, -1.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for o in (C.byref(opt), None):
        assert lib.mgx_newton(None, o, kap.ctypes.data, kap.size, C.byref(ns), st, dp(lam), dp(hist), 6) == INVALID
    assert (ns.iterations, ns.converged, ns.history_len) == (-7, -7, -7)
    assert all(s.cycles == -7 for s in st) and (lam == -1.0).all() and (hist == -1.0).all()
    ms = C.c_double(-1.0)
    for step in (0, 1):
        assert lib.mgx_time_newton_pass(None, step, 1, C.byref(ms)) == INVALID and ms.value == -1.0
