"""CPU checks of the numpy statement of mgx_solve_gcr (tests/gcr_ref.py) - no device - and of the header, the library's
exports and the binding.  The cycles are those of tests/line_ref.py (GALERKIN, bilinear transfers, LINE_ALT V(1,1),
coarsest level 3) with lr.NumpyOps; b = default_rng(3).uniform(-1, 1), tol 1e-8, at most 60 iterations."""
import functools
import os

import numpy as np
import pytest

import gcr_ref
import line_ref as lr
import pcg_ref
from conftest import ROOT

TOL, CAP = 1e-8, 60


@functools.lru_cache(maxsize=None)
def problem(kind):
    """(A, M, b, hierarchy): 'layers': the layers problem (eps = 1e-2) at 63^2; 'peclet1': upwind convection-diffusion,
    a = (1, 0.5), cell Peclet number 1, at 127^2"""
    L, st5 = (6, lr.aniso_stencil(6, 1e-2, "layers")) if kind == "layers" else (7, gcr_ref.upwind_stencil(7, (1.0, 0.5), 1.0))
    n = (1 << L) - 1
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    h = lr.Hierarchy(lr.LINE_ALT, lr.NumpyOps, st5, L, 3, np.float64, mu1=1, mu2=1)
    return pcg_ref.Operator(st5, np.float64), gcr_ref.cycle_preconditioner(h), b, h


def run(kind, restart, tol=TOL, cap=CAP, **kw):
    A, M, b, _ = problem(kind)
    return gcr_ref.gcr(A, M, b, np.zeros_like(b), tol, cap, restart, **kw)


def test_header_library_and_binding_have_solve_gcr(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "mgx_solve_gcr" in text and "#define MGX_GCR_MAX_RESTART 8" in text
    assert "mgx_solve_gcr" in pkg.EXPORTS and hasattr(pkg.lib(), "mgx_solve_gcr")
    assert callable(pkg.Multigrid.solve_gcr) and pkg.GCR_MAX_RESTART == 8
    assert pkg.lib().mgx_solve_gcr(None, 1e-8, 10, 4, None, None, 0) == 1          # MGX_ERR_INVALID: no handle


@pytest.mark.parametrize("kind", ["layers", "peclet1"])
@pytest.mark.parametrize("restart", [1, 3, 4, 8])
def test_histories_are_monotone_and_the_recursive_residual_is_the_true_one(kind, restart):
    A, _, b, _ = problem(kind)
    x, h, conv, brk = run(kind, restart)
    assert conv and not brk and h[-1] <= TOL * h[0]
    assert np.all(h[1:] <= h[:-1] * (1 + 1e-12)), h
    true = np.sqrt(pcg_ref.dot(b - A(x), b - A(x)))
    assert abs(true - h[-1]) <= 1e-10 * h[-1] + 1e-14 * h[0], (true, h[-1])


def test_a_restart_no_shorter_than_the_solve_is_no_restart():
    x8, h8, conv, _ = run("layers", 8)
    assert conv and len(h8) - 1 <= 8
    x60, h60, _, _ = run("layers", 60)
    assert np.array_equal(h8, h60) and np.array_equal(x8, x60)
    # and a shorter one is the same method up to its first restart
    _, h3, _, _ = run("layers", 3)
    assert np.array_equal(h3[:4], h8[:4]) and not np.array_equal(h3[:5], h8[:5])


def test_iteration_counts_on_the_layers_problem():
    """plain cycles 9, PCG 10, GCR(4) 7, GCR(8) 6"""
    A, M, b, h = problem("layers")
    plain = len(h.solve(b, tol=TOL, max_cycles=CAP)[1]) - 1
    pcg = pcg_ref.pcg(A, M, b, np.zeros_like(b), TOL, CAP)
    counts = [len(run("layers", m)[1]) - 1 for m in (4, 8)]
    assert (plain, len(pcg[1]) - 1, pcg[2]) == (9, 10, True) and counts == [7, 6]
    assert counts[0] <= plain


def test_gcr_converges_on_upwind_convection_where_pcg_does_not():
    """cell Peclet number 1 at 127^2: plain cycles 6, GCR(4) 5; the conjugate gradients of pcg_ref are still above the
    initial residual after 60 iterations"""
    A, M, b, h = problem("peclet1")
    c, n, s, w, e = A.coef
    assert not np.array_equal(w, e) and not np.array_equal(n, s)            # A is not symmetric
    plain = len(h.solve(b, tol=TOL, max_cycles=CAP)[1]) - 1
    _, hp, conv_p, _ = pcg_ref.pcg(A, M, b, np.zeros_like(b), TOL, CAP)
    _, hg, conv_g, brk = run("peclet1", 4)
    assert plain == 6 and conv_g and not brk and len(hg) - 1 == 5
    assert not conv_p and not (hp[-1] <= TOL * hp[0])


def test_the_upwind_stencil():
    c, n, s, w, e = gcr_ref.upwind_stencil(5, (1.0, -0.5), 2.0)
    h = 2.0 ** -5
    eps = h / 2.0
    assert np.all(w == -eps - h) and np.all(e == -eps) and np.all(n == -eps) and np.all(s == -eps - 0.5 * h)
    assert np.all(c == -(n + s + w + e)) and c.shape == (31, 31)
    ax, ay = gcr_ref.recirculating_velocity(5)
    st = gcr_ref.upwind_stencil(5, (ax, ay), 2.0)
    assert all(v.shape == (31, 31) for v in st) and np.all(st[0] > 0) and all(np.all(v < 0) for v in st[1:])
    assert np.ptp(st[3]) > 0                                                # per point


def test_edge_cases_of_the_reference():
    A, M, b, _ = problem("layers")
    z = np.zeros_like(b)
    x, h, conv, brk = gcr_ref.gcr(A, lambda r: np.zeros_like(r), b, z, TOL, CAP, 4)      # M = 0: q' = 0
    assert brk and not conv and len(h) == 1 and not x.any()
    x, h, conv, brk = gcr_ref.gcr(A, M, b, z, TOL, 0, 4)
    assert len(h) == 1 and not conv and not brk
    x, h, conv, brk = gcr_ref.gcr(A, M, z, z, TOL, CAP, 4)
    assert len(h) == 1 and h[0] == 0.0 and conv and not brk
    x, h, conv, brk = gcr_ref.gcr(A, M, b, z, TOL, 2, 4)
    assert len(h) == 3 and not conv


def test_another_summation_order_moves_the_history_by_rounding_only():
    _, h, _, _ = run("layers", 4)
    _, hr, _, _ = run("layers", 4, dot=gcr_ref.dot_reversed)
    assert len(h) == len(hr) and np.all(np.abs(h - hr) <= 1e-9 * h + 1e-14 * h[0])
