"""CPU checks of mgx_solve_refine (include/mgx.h): the two entry points in the header, the library and the binding; the
convergence claim of the feature on the numpy hierarchies of tests/galerkin_ref.py (fp64 defect correction around a
float32 V-cycle keeps the fp64 hierarchy's cycle counts where the float32 hierarchy alone stalls); and the exactness
of the power-of-two scaling (tests/refine_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import galerkin_ref as gr
import refine_ref as rr
from conftest import ROOT
from pcg_ref import contrast_coefficient


def test_header_library_and_binding_have_the_entry_points(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"MGX_API\s+int\s+(mgx_\w+)\s*\(([^;]*)\);", text)}
    assert decl["mgx_solve_refine"].count(",") == 5 and "mgx_stats" in decl["mgx_solve_refine"]
    assert decl["mgx_time_refine_pass"].count(",") == 2 and "mgx_handle" in decl["mgx_time_refine_pass"]
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "mgx_solve_refine") and hasattr(L, "mgx_time_refine_pass")
    assert {"mgx_solve_refine", "mgx_time_refine_pass"} <= set(pkg.EXPORTS)
    assert len(pkg.lib().mgx_solve_refine.argtypes) == 6 and len(pkg.lib().mgx_time_refine_pass.argtypes) == 3
    assert callable(getattr(pkg.Multigrid, "solve_refine", None)) and callable(getattr(pkg.Multigrid, "time_refine_pass", None))
    # a NULL handle is an invalid argument, not a crash (no GPU is touched)
    assert pkg.lib().mgx_solve_refine(None, 1e-8, 1, None, None, 0) == 1
    assert pkg.lib().mgx_time_refine_pass(None, 1, None) == 1


# (finest, coarsest, contrast, fp64 cycles to 1e-11): Jacobi V(2,2), b = default_rng(3).uniform(-1, 1)
CASES = [(6, 3, 10.0, 22), (7, 4, 100.0, 53), (8, 4, 10.0, 27)]


@pytest.mark.parametrize("L,Lc,contrast,cycles", CASES)
def test_refinement_keeps_the_fp64_cycle_count_where_float32_alone_stalls(po, L, Lc, contrast, cycles):
    n = (1 << L) - 1
    st5 = po.stencil_from_nodes(contrast_coefficient(L, contrast), L, L)
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    h64 = gr.Hierarchy(po, st5, L, Lc)
    h32 = gr.Hierarchy(po, [np.asarray(x, dtype=np.float32) for x in st5], L, Lc, dtype=np.float32)
    _, hist64 = h64.solve(b, tol=1e-11, max_cycles=80)
    assert len(hist64) - 1 == cycles and hist64[-1] <= 1e-11 * hist64[0]

    def cycle32(r32):
        return h32.vcycle(L, np.zeros_like(r32), r32)

    u, hist = rr.refine(lambda u, bb: h64.residual(L, u, bb), cycle32, b, np.zeros_like(b), tol=1e-11, max_cycles=80, norm=po.norm2)
    print(f"L {L}..{Lc}, contrast {contrast:g}: fp64 {len(hist64) - 1} cycles, refine {len(hist) - 1}, "
          f"largest relative difference of the histories {np.max(np.abs(hist - hist64[:len(hist)]) / hist64[:len(hist)]):.2e}")
    # exactly the fp64 hierarchy's count, the history within 1e-3 relative of the fp64 one at every cycle
    assert len(hist) == len(hist64) and hist[-1] <= 1e-11 * hist[0]
    assert np.all(np.abs(hist - hist64) <= 1e-3 * hist64)
    assert po.norm2(h64.residual(L, u, b)) == hist[-1]
    # the float32 hierarchy alone: never below 1e-7 relative in 40 cycles
    _, hist32 = h32.solve(b.astype(np.float32), tol=0.0, max_cycles=40)
    print(f"    float32 alone: best {np.min(hist32) / hist32[0]:.2e}")
    assert len(hist32) == 41 and np.min(hist32) > 1e-7 * hist32[0]


def test_pow2_floor_is_the_power_of_two_at_or_below():
    for x in (1.0, 1.5, 2.0, 3.999, 4.0, 0.75, 1e-300, 3e-17, 6.02e23):
        s = rr.pow2_floor(x)
        assert s <= x < 2.0 * s and np.frexp(s)[0] == 0.5


def test_the_scaling_by_a_power_of_two_is_exact():
    """float32(r / s) * s is float32(r) for every scale the rule can produce: ||r|| / n between the float32 floor of a
    stalled solve and a large right-hand side, the entries of r around that rms (all inside float32's normal range)"""
    rng = np.random.default_rng(11)
    for e in range(-80, 41):
        s = float(np.ldexp(1.0, e))
        assert rr.pow2_floor(s * 1.37) == s
        r = rng.uniform(-8.0, 8.0, 512) * s
        r[:3] = (s, -s * (1.0 + 2.0 ** -30), 0.0)
        scaled = (r / s).astype(np.float32)
        assert np.array_equal(scaled.astype(np.float64) * s, r.astype(np.float32).astype(np.float64)), e
        # the device multiplies by 1 / s: the same float64 as the quotient
        assert np.array_equal(r * (1.0 / s), r / s)
