"""CPU checks of mgx_solve_refine_gcr (include/mgx.h): the two entry points in the header, the library and the binding;
the claim of the feature on the numpy hierarchies of tests/galerkin_ref.py (restarted GCR in float64 keeps its iteration
counts when its preconditioner is the scaled float32 cycle, tests/refine_gcr_ref.py against tests/gcr_ref.py); and what
the summation order of the dots is worth on the 9..5 configuration of tests/test_gpu_refine_gcr.py's parity test.

The cases are those of tests/test_refine_cpu.py: Jacobi V(2,2), contrast coefficient, b = default_rng(3).uniform(-1, 1),
zero guess, to 1e-11."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import galerkin_ref as gr
import gcr_ref
import refine_gcr_ref as rg
from conftest import ROOT
from pcg_ref import contrast_coefficient

TOL, CAP = 1e-11, 80


def test_header_library_and_binding_have_the_entry_points(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"MGX_API\s+int\s+(mgx_\w+)\s*\(([^;]*)\);", text)}
    assert decl["mgx_solve_refine_gcr"].count(",") == 6 and "mgx_stats" in decl["mgx_solve_refine_gcr"]
    assert decl["mgx_time_refine_gcr_pass"].count(",") == 3 and "mgx_handle" in decl["mgx_time_refine_gcr_pass"]
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "mgx_solve_refine_gcr") and hasattr(L, "mgx_time_refine_gcr_pass")
    assert {"mgx_solve_refine_gcr", "mgx_time_refine_gcr_pass"} <= set(pkg.EXPORTS)
    assert len(pkg.lib().mgx_solve_refine_gcr.argtypes) == 7 and len(pkg.lib().mgx_time_refine_gcr_pass.argtypes) == 4
    assert callable(getattr(pkg.Multigrid, "solve_refine_gcr", None)) and callable(getattr(pkg.Multigrid, "time_refine_gcr_pass", None))
    # a NULL handle is an invalid argument, not a crash (no GPU is touched)
    assert pkg.lib().mgx_solve_refine_gcr(None, 1e-8, 1, 4, None, None, 0) == 1
    assert pkg.lib().mgx_time_refine_gcr_pass(None, 0, 1, None) == 1


@functools.lru_cache(maxsize=None)
def problem(L, Lc, contrast):
    """(A, the fp64 cycle as M, the float32 cycle, b) of the GALERKIN hierarchy L..Lc, Jacobi V(2,2)"""
    from oracle import pyoracle as po
    n = (1 << L) - 1
    st5 = po.stencil_from_nodes(contrast_coefficient(L, contrast), L, L)
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    h64 = gr.Hierarchy(po, st5, L, Lc)
    h32 = gr.Hierarchy(po, [np.asarray(x, dtype=np.float32) for x in st5], L, Lc, dtype=np.float32)
    zero = np.zeros_like(b)

    def A(u):
        return -h64.residual(L, u, zero)            # (the sign flip is exact)
    A.dtype = np.float64

    def cycle32(r32):
        return h32.vcycle(L, np.zeros_like(r32), r32)

    return A, gcr_ref.cycle_preconditioner(h64), cycle32, b


# (finest, coarsest, contrast): fp64 GCR(1) / (4) / (8) iterations to 1e-11
CASES = {(6, 3, 10.0): (16, 12, 12), (7, 4, 100.0): (32, 20, 19), (8, 4, 10.0): (18, 14, 14)}
# the relative gap between the recursively updated residual norm and the true one, ||b - A x||, at the end of these
# solves (at 1e-11 of the first entry): measured 1.2e-4 at the most (7..4, contrast 100, restart 1; the other eight runs
# between 1.6e-5 and 9.7e-5); the bound is 8 times that.  It is the float64 rounding of x += alpha z' (1e-16 of x, seen through A
# by the true residual and not by the recursive one) against a residual that has fallen by eleven orders: 1e-16 / 1e-11 = 1e-5
# per update.  tests/test_gpu_refine_gcr.py holds the device to the same bound at the smaller reduction it runs to
TRUE_GAP = 1e-3


@pytest.mark.parametrize("restart", [1, 4, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_the_mixed_iteration_keeps_the_fp64_counts(po, case, restart):
    L, Lc, contrast = case
    A, M64, cycle32, b = problem(L, Lc, contrast)
    zero = np.zeros_like(b)
    _, h64, conv64, brk64 = gcr_ref.gcr(A, M64, b, zero, TOL, CAP, restart)
    x, h, conv, brk = rg.refine_gcr(A, cycle32, b, zero, TOL, CAP, restart)
    want = CASES[case][{1: 0, 4: 1, 8: 2}[restart]]
    true = po.norm2(b - A(x))
    gap = abs(true - h[-1]) / true
    dev = np.max(np.abs(h - h64[:len(h)]) / h64[:len(h)]) if len(h) <= len(h64) else np.inf
    print(f"L {L}..{Lc}, contrast {contrast:g}, GCR({restart}): fp64 {len(h64) - 1} iterations, mixed {len(h) - 1}; histories differ by "
          f"{dev:.2e} relative; recursive {h[-1]:.6e}, true {true:.6e}: gap {gap:.2e} ({gap / TRUE_GAP:.3g} of the bound {TRUE_GAP:g})")
    assert conv64 and not brk64 and len(h64) - 1 == want
    assert conv and not brk and len(h) == len(h64) and h[-1] <= TOL * h[0]
    assert np.all(h[1:] <= h[:-1]), h
    assert gap <= TRUE_GAP, (true, h[-1])


# ---- what the summation order of the dots is worth ----------------------------------------------------------------------
# the 9..5 case of the GPU parity test (tests/test_gpu_refine_gcr.py imports it): GALERKIN, Jacobi V(2,2), contrast 10, zero
# guess, restart 4, six iterations with tol 0 (slots 0 .. 3 and a wrap)
NINE_FIVE = dict(L=9, Lc=5, contrast=10.0, restart=4, iters=6)
RTOL64, X_TOL64 = 1e-9, 1e-9                      # the GPU test's bounds (tests/test_gpu_pcg.py, tests/test_gpu_gcr.py)
# Measured: over the six iterations the reversed dots move the history by 2.5e-4 of the GPU bound at the most and the iterate
# by 1.4e-7 of its bound; the reference is held to 1e-2 of both, 40 times the larger figure.
# The figure is small only until the first float rounding of r / s_k flips: the two runs then differ by 6e-8 of one entry
# of r32, and the history by more than the bound a few iterations later - run on to 1e-10 (13 iterations) the same pair of
# runs differs by 0.5 of the bound at entry 9 (printed, not asserted).  A flip needs the two residuals to differ by a
# relative 1e-16 .. 1e-14 in an entry that lies that close to a float rounding boundary, one chance in 1e7 per entry, and
# there are 2.6e5 entries per iteration.  That is why the GPU test hands the reference the DEVICE'S summation order
# (refine_gcr_ref.device_dot) and not numpy's: with it nothing is left to chance.
ORDER_FRACTION = 1e-2


def order_movement(h, hr, x, xr):
    return (float(np.max(np.abs(h - hr) / (RTOL64 * h + 1e-14 * h[0]))), float(np.max(np.abs(x - xr)) / np.max(np.abs(x)) / X_TOL64))


def test_another_summation_order_is_a_small_fraction_of_the_gpu_bound():
    c = NINE_FIVE
    A, _, cycle32, b = problem(c["L"], c["Lc"], c["contrast"])
    zero = np.zeros_like(b)
    runs = {}
    for iters, tol in ((c["iters"], 0.0), (40, 1e-10)):
        x, h, _, brk = rg.refine_gcr(A, cycle32, b, zero, tol, iters, c["restart"])
        xr, hr, _, brkr = rg.refine_gcr(A, cycle32, b, zero, tol, iters, c["restart"], dot=gcr_ref.dot_reversed)
        assert not brk and not brkr and len(h) == len(hr)
        runs[iters] = order_movement(h, hr, x, xr)
        print(f"9..5, {len(h) - 1} iterations: the reversed dots move the history by {runs[iters][0]:.3g} of the GPU bound, the iterate by "
              f"{runs[iters][1]:.3g} of its bound")
    dh, dx = runs[c["iters"]]
    assert dh <= ORDER_FRACTION and dx <= ORDER_FRACTION, (dh, dx)


# ---- the scales: invariance under a power of two -----------------------------------------------------------------------------
@pytest.mark.parametrize("dot", [rg.dot, rg.device_dot], ids=["numpy-order", "device-order"])
@pytest.mark.parametrize("loop", ["refine_gcr", "refine"])
def test_the_references_commute_with_a_power_of_two_beyond_float_range(loop, dot):
    """refine_gcr_ref.refine_gcr and refine_ref.refine on (2^e b, 2^e u0), e = -160 and +160, return 2^e x and 2^e hist of the
    unscaled call BIT FOR BIT, with the same iteration count, at tol 0 and run to 1e-10: every float64 operation of the loops
    commutes with a power of two while nothing overflows or goes subnormal (squares reach 2^+-320), and r / s_k is the same
    float32 array for every e.  2^+-160 is beyond float32's range (2^-149 .. 2^128): a loop that skipped the scale would hand
    the cycle zeros or infinities.  tests/test_gpu_refine_gcr.py holds the device to the same statement"""
    import refine_ref as rr
    A, _, cycle32, b = problem(6, 3, 10.0)
    u0 = np.random.default_rng(4).uniform(-1, 1, b.shape)
    if loop == "refine_gcr":
        run = lambda bb, uu, tol, k: rg.refine_gcr(A, cycle32, bb, uu, tol, k, 4, dot=dot)[:2]
    else:
        run = lambda bb, uu, tol, k: rr.refine(lambda u, f: f - A(u), cycle32, bb, uu, tol=tol, max_cycles=k, norm=lambda r: float(np.sqrt(dot(r, r))))
    for tol, k in ((0.0, 6), (1e-10, 60)):
        x, h = run(b, u0, tol, k)
        assert len(h) == 7 if tol == 0.0 else (6 < len(h) - 1 < 60 and h[-1] <= tol * h[0]), h
        for e in (-160, 160):
            xe, he = run(np.ldexp(b, e), np.ldexp(u0, e), tol, k)
            assert np.array_equal(he, np.ldexp(h, e)), (loop, e, he, np.ldexp(h, e))
            assert np.array_equal(xe, np.ldexp(x, e)) and np.isfinite(xe).all(), (loop, e)


@pytest.mark.parametrize("n,rows", [(15, 0), (63, 1), (63, 5), (127, 0), (255, 0), (511, 0), (1023, 0), (2047, 0)])
def test_the_device_order_dot_counts_every_product_once(n, rows):
    """integers: every order gives the same exact sum; and on random data it agrees with numpy's dot to rounding"""
    rng = np.random.default_rng(n)
    a, b = rng.integers(-9, 10, (n, n)).astype(np.float64), rng.integers(-9, 10, (n, n)).astype(np.float64)
    assert rg.device_dot(a, b, rows) == float(np.sum(a * b))
    a, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    want = float(np.dot(a.ravel(), b.ravel()))
    assert abs(rg.device_dot(a, b, rows) - want) <= 1e-13 * float(np.sum(np.abs(a * b)))
    assert rg.device_dot(a, a, rows) > 0.0
