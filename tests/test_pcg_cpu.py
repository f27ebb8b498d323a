"""CPU checks of mgx_solve_pcg (conjugate gradients preconditioned by one V-cycle): the entry point is declared,
exported and bound, and the numpy reference of tests/pcg_ref.py - the statement the GPU tests hold the device
to - reproduces the iteration counts measured with the oracle's V-cycle as preconditioner."""
import ctypes as C
import os

import numpy as np
import pytest

import pcg_ref
from conftest import ROOT


def test_header_declares_and_library_exports_solve_pcg(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert "MGX_API int mgx_solve_pcg(mgx_handle h, double tol, int max_iters, mgx_stats* stats," in text
    assert "mgx_solve_pcg" in pkg.EXPORTS
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "mgx_solve_pcg")


def test_binding_has_solve_pcg(pkg):
    assert callable(getattr(pkg.Multigrid, "solve_pcg", None))
    assert pkg.lib().mgx_solve_pcg.argtypes is not None


def test_solve_pcg_without_a_device_is_refused_cleanly(pkg):
    # a NULL handle is an invalid argument, not a crash (no GPU is touched)
    assert pkg.lib().mgx_solve_pcg(None, 1e-8, 10, None, None, 0) == 1


POISSON = dict(finest_level=9, coarsest_level=5, mu1=2, mu2=1, schedule=0)
VAR = dict(finest_level=9, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=1)


def test_reference_reproduces_poisson_iteration_count(po):
    b = po.rhs_sine(9)
    x, h, conv, brk = pcg_ref.run(po, POISSON, b)
    assert conv and not brk
    assert len(h) - 1 == 9
    assert pcg_ref.true_residual(b, x) <= 2e-8 * h[0]
    # plain V-cycles need 15 (the gain the feature is for)
    s = pcg_ref.oracle_solver(po, POISSON)
    _, hv = s.solve(b, None, tol=1e-8, max_cycles=60)
    assert len(hv) - 1 == 15


@pytest.mark.parametrize("contrast,iters", [(10.0, 26), (100.0, 77)])
def test_reference_reproduces_stencil5_iteration_counts(po, contrast, iters):
    b = po.rhs_sine(9)
    a = pcg_ref.contrast_coefficient(9, contrast)
    x, h, conv, brk = pcg_ref.run(po, VAR, b, a_nodes=a)
    assert conv and not brk
    assert len(h) - 1 == iters
    assert pcg_ref.true_residual(b, x, a, 9, po) <= 2e-8 * h[0]
    if contrast == 100.0:
        # plain V-cycles diverge on this operator
        s = pcg_ref.oracle_solver(po, VAR, a)
        _, hv = s.solve(b, None, tol=1e-8, max_cycles=60)
        assert not (hv[-1] <= 1e-8 * hv[0]) and hv[-1] > hv[0]


def test_reference_edge_cases(po):
    n = 31
    cfg = dict(finest_level=5, coarsest_level=3, mu1=2, mu2=1, schedule=0)
    x, h, conv, brk = pcg_ref.run(po, cfg, np.zeros((n, n)))
    assert conv and not brk and len(h) == 1 and h[0] == 0.0 and not x.any()
    b = po.rhs_sine(5)
    u0 = po.fill_uniform((n, n), 7)
    x, h, conv, brk = pcg_ref.run(po, cfg, b, u0, max_iters=0)
    assert len(h) == 1 and np.array_equal(x, u0) and not conv
