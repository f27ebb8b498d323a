"""CPU checks of tests/theta_ref.py - the numpy statement tests/test_gpu_theta.py holds the device to - against
mathematics, and of the new entry points' argument checks that need no device.

The 15 x 15 Poisson operator (a = 1) has the eigenvectors sin(k pi x) sin(l pi y) with lambda = 4 - 2 cos(k pi / N) -
2 cos(l pi / N), so one theta step of M u_t + A0 u = 0 with d = M / (theta dt) multiplies such a mode by
(d - kappa lambda) / (d + lambda), kappa = (1 - theta) / theta, and the exact solution by exp(-lambda dt / M)."""
import ctypes as C

import numpy as np
import pytest

import theta_ref as tr

L = 4
INVALID = 1                                # MGX_ERR_INVALID


@pytest.mark.parametrize("theta", [1.0, 0.5, 0.75])
def test_a_sine_mode_decays_by_the_amplification_factor(theta):
    """d = 1, five steps, dense float64 solves: cond(S) <= (1 + 8) / 1 = 9 and rounding is about 1e-14 per step, so 1e-10
    relative is an ample margin"""
    k, l = 2, 3
    u0, lam = tr.sine_mode(L, k, l)
    n = u0.shape[0]
    d = np.ones((n, n))
    S = tr.shift(tr.poisson9(L), d)
    kappa = (1.0 - theta) / theta
    us = tr.steps(S, d, u0, None, theta, 5, tr.dense_solver(S))
    for j, u in enumerate(us, start=1):
        want = ((1.0 - kappa * lam) / (1.0 + lam)) ** j
        amp = np.vdot(u, u0) / np.vdot(u0, u0)
        assert abs(amp - want) <= 1e-10 * abs(want), (theta, j, amp, want)
        assert np.max(np.abs(u - amp * u0)) <= 1e-10 * abs(want), (theta, j)     # still the one mode


def end_error(theta, dt, t_end):
    """|amplitude after t_end / dt theta steps - exp(-lambda t_end)| of the mode (1, 1), M = 1"""
    u0, lam = tr.sine_mode(L, 1, 1)
    n = u0.shape[0]
    d = np.full((n, n), 1.0 / (theta * dt))
    S = tr.shift(tr.poisson9(L), d)
    u = tr.steps(S, d, u0, None, theta, int(round(t_end / dt)), tr.dense_solver(S))[-1]
    return abs(np.vdot(u, u0) / np.vdot(u0, u0) - np.exp(-lam * t_end))


@pytest.mark.parametrize("theta, lo, hi", [(0.5, 3.5, 4.5), (1.0, 1.8, 2.2)])
def test_halving_the_step_reduces_the_error_by_the_order_of_the_scheme(theta, lo, hi):
    """lambda(1, 1) = 4 - 4 cos(pi / 16) = 0.0769; t_end = 4, dt = 0.5 and 0.25 (lambda dt = 0.038 and 0.019): the error
    constants' next terms are O(lambda dt) of the leading one, well inside the brackets, and the errors (1e-3 .. 1e-5)
    are far above the rounding of 16 dense solves"""
    ratio = end_error(theta, 0.5, 4.0) / end_error(theta, 0.25, 4.0)
    assert lo <= ratio <= hi, (theta, ratio)


def test_the_pass_operation_by_operation():
    """rhs_pass against the formula written out per point in Python floats (float64 arithmetic), with and without g"""
    rng = np.random.default_rng(3)
    n = (1 << L) - 1
    u, d, g = rng.uniform(-1, 1, (n, n)), rng.uniform(0.5, 2, (n, n)), rng.uniform(-1, 1, (n, n))
    S = tr.shift(tr.poisson9(L), d)
    Su = tr.apply(S, u)
    assert np.array_equal(S[0], 4.0 + d) and all(np.array_equal(S[q], tr.poisson9(L)[q]) for q in range(1, 9))
    for theta in (1.0, 0.5, 0.75):
        c1, c0 = 1.0 / theta, (1.0 - theta) / theta
        for gg in (None, g):
            b = tr.rhs_pass(Su, u, d, gg, theta)
            for i, j in ((0, 0), (3, 7), (n - 1, n - 1)):
                m = float(d[i, j]) * float(u[i, j])
                want = m if theta == 1.0 else c1 * m - c0 * float(Su[i, j])
                if gg is not None:
                    want = want + float(g[i, j])
                assert b[i, j] == want, (theta, i, j)


def test_null_handles_are_refused_without_a_device(pkg):
    lib = pkg.lib()
    assert lib.mgx_set_reaction(None, None, 0) == INVALID
    assert lib.mgx_get_reaction(None, None, 0) == INVALID
    done = C.c_int(7)
    assert lib.mgx_theta_steps(None, 1.0, 1, None, pkg.STEP_SOLVE, 1e-8, 5, 4, C.byref(done), None, None, 0) == INVALID
    assert done.value == 7
    ms = C.c_double(-1.0)
    assert lib.mgx_time_theta_rhs(None, 1.0, 1, C.byref(ms)) == INVALID and ms.value == -1.0
