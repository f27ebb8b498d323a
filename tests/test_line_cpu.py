"""Properties of the numpy statement of the zebra line smoothers (tests/line_ref.py), which tests/test_gpu_line.py
holds the device to: every line solve against scipy's banded solver, the residual a sweep leaves on the lines of its
last colour, the breakdown fixture, and the cycle counts that make the case for the smoother (anisotropic operators on
which point Jacobi does not converge).

THE TOLERANCE RULE of the comparisons (the same in tests/test_gpu_line.py): the rounding error of a Thomas solve grows
with the line's condition number, so a bound is measured per case as the largest difference, relative to max |x|,
between line_ref in the working type and line_ref in np.longdouble, times 4, with a floor of 16 eps of the type (the
measured error is 0 in some double cases)."""
import numpy as np
import pytest
from scipy.linalg import solve_banded

import galerkin_ref as gr
import line_ref as lr
import pcg_ref

TOL, CAP = 1e-8, 60


def operator5(po, L, kind, dt=np.float64):
    if kind == "contrast":
        return [x.astype(dt) for x in po.stencil_from_nodes(pcg_ref.contrast_coefficient(L, 100.0), L, L)]
    eps, k = {"iso": (1.0, "x"), "x1e-2": (1e-2, "x"), "y1e-2": (1e-2, "y"), "x1e-3": (1e-3, "x"), "layers": (1e-2, "layers")}[kind]
    return lr.aniso_stencil(L, eps, k, dt)


def as_type(st9, dt):
    return [np.asarray(a, dtype=dt) for a in st9]


def rule_bound(x_t, x_long):
    """(bound, the reference's own relative error): 4 x |line_ref in T - line_ref in long double| / max |x|, floor 16 eps"""
    err = float(np.max(np.abs(x_t.astype(np.longdouble) - x_long)) / np.max(np.abs(x_long)))
    return max(4.0 * err, 16.0 * float(np.finfo(x_t.dtype).eps)), err


def level_operator(po, L, kind, nine, dt):
    """a five-point operator of level L, or the nine-point R A P of the five-point operator of level L + 1"""
    if not nine:
        return gr.nine(operator5(po, L, kind, dt))
    return gr.rap(gr.nine(operator5(po, L + 1, kind, dt)), 1 << (L + 1))


def scipy_sweep(st9, v, b, nine, direction):
    """the sweep with every line solved by scipy.linalg.solve_banded in double from the assembled tridiagonal matrix"""
    if direction == "y":
        return scipy_sweep(lr.transposed(st9), v.T.copy(), b.T.copy(), nine, "x").T.copy()
    st9 = as_type(st9, np.float64)
    v, b = v.astype(np.float64), b.astype(np.float64)
    n = v.shape[0]
    for first in (0, 1):
        rows = np.arange(first, n, 2)
        rhs = lr.line_rhs(st9, v, b, rows, nine)
        for k, i in enumerate(rows):
            ab = np.zeros((3, n))
            ab[0, 1:] = st9[4][i, :-1]
            ab[1] = st9[0][i]
            ab[2, :-1] = st9[3][i, 1:]
            v[i] = solve_banded((1, 1), ab, rhs[k])
    return v


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nine", [False, True], ids=["five", "nine"])
@pytest.mark.parametrize("kind", ["x1e-3", "layers", "contrast"])
def test_a_sweep_equals_scipy_line_by_line(po, kind, nine, dt):
    L = 5
    st9 = level_operator(po, L, kind, nine, dt)
    n = (1 << L) - 1
    rng = np.random.default_rng(7)
    v, b = rng.uniform(-1, 1, (n, n)).astype(dt), rng.uniform(-1, 1, (n, n)).astype(dt)
    for direction, smoother in (("x", lr.LINE_X), ("y", lr.LINE_Y)):
        got = lr.LevelSmoother(st9, nine, smoother).sweep(v, b)
        exact = lr.LevelSmoother(as_type(st9, np.longdouble), nine, smoother).sweep(v.astype(np.longdouble), b.astype(np.longdouble))
        bound, err = rule_bound(got, exact)
        want = scipy_sweep(st9, v, b, nine, direction)
        diff = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        # scipy's own LU (with pivoting, in double) carries an error of the same kind: its distance to long double joins the bound
        own = float(np.max(np.abs(want - exact)) / np.max(np.abs(exact)))
        assert diff <= bound + own, (kind, nine, direction, f"difference {diff:.3e}, bound {bound:.3e} (reference error {err:.3e}), scipy's own {own:.3e}")
        assert got.dtype == dt


@pytest.mark.parametrize("nine", [False, True], ids=["five", "nine"])
@pytest.mark.parametrize("smoother", [lr.LINE_X, lr.LINE_Y, lr.LINE_ALT])
def test_a_sweep_leaves_no_residual_on_the_lines_of_its_last_colour(po, smoother, nine):
    """... the even grid rows (x) or columns (y, alternating): interior indices 1, 3, ...; the lines of the first colour
    keep one, because their neighbours changed afterwards"""
    L = 5
    st9 = level_operator(po, L, "layers", nine, np.float64)
    n = (1 << L) - 1
    rng = np.random.default_rng(8)
    v, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    r = gr.residual9(lr.LevelSmoother(st9, nine, smoother).sweep(v, b), b, st9)
    if smoother != lr.LINE_X:
        r = r.T
    scale = np.max(np.abs(b))
    assert np.max(np.abs(r[1::2])) <= 1e-13 * scale, np.max(np.abs(r[1::2]))
    assert np.max(np.abs(r[0::2])) > 1e-4 * scale


def test_factor_reports_a_zero_pivot():
    """c = 1, w = e = -1: m_0 = 1, g_0 = -1, and the second pivot is 1 - (-1)(-1) = 0"""
    n = 3
    st9 = gr.nine([np.ones((n, n)), -np.ones((n, n)), -np.ones((n, n)), -np.ones((n, n)), -np.ones((n, n))])
    assert lr.factor(st9)[2] is False
    assert lr.factor_dir(st9, "y")[2] is False
    for smoother, direction in ((lr.LINE_X, "x-line"), (lr.LINE_Y, "y-line"), (lr.LINE_ALT, "x-line")):
        with pytest.raises(lr.Breakdown, match=f"level 2.*{direction}"):
            lr.LevelSmoother(st9, False, smoother, level=2)
    ok = gr.nine(lr.aniso_stencil(2, 1e-2))
    m, g, fine = lr.factor(ok)
    assert fine and np.all(g[:, -1] == 0) and np.all(np.isfinite(m))
    # y-strong only in the middle row: a zero pivot of the x-lines there, none in the y-lines
    bad = [a.copy() for a in ok]
    bad[0][1, :], bad[3][1, :], bad[4][1, :] = 1.0, -1.0, -1.0
    assert lr.factor(bad)[2] is False and lr.factor_dir(bad, "y")[2] is True


# cycles to 1e-8, or None where the run stops at the cap of 60 cycles with a residual ratio not below 1e-3: (x-line,
# y-line, alternating) V(1,1), after Jacobi V(2,2) with omega = 2/3; levels 6..3 and 5..3; right-hand side
# default_rng(3).uniform(-1, 1).  SLOW: the x-line smoother on the layers problem, levels 5..3, where the measured table
# that these counts restate has 2.0e-4 at cycle 60 - stagnation all the same (four orders above the tolerance after ten
# times the cycles the alternating smoother needs), but below the 1e-3 of the other capped runs: held to 1e-4
SLOW = "stops at the cap above 1e-4"
TABLE = {
    6: {"iso": (10, 7, 7, 6), "x1e-2": (None, 7, None, 7), "y1e-2": (None, None, 7, 6), "x1e-3": (None, 5, None, 5), "layers": (None, None, None, 9)},
    5: {"iso": (10, 7, 7, 6), "x1e-2": (None, 6, None, 6), "y1e-2": (None, None, 6, 6), "x1e-3": (None, 3, None, 3), "layers": (None, SLOW, None, 7)},
}
# the same with default_rng(9): no converging line case ends within [0.5, 2] tol (with seed 3 the alternating smoother
# on the y-strong problem, levels 6..3, ends at 0.84 tol); these are the counts tests/test_gpu_line.py asks of the device
SEED_STABLE = 9
TABLE_STABLE = {
    6: {"iso": (7, 7, 6), "x1e-2": (7, None, 7), "y1e-2": (None, 7, 7), "x1e-3": (5, None, 5), "layers": (None, None, 9)},
    5: {"iso": (7, 7, 6), "x1e-2": (6, None, 6), "y1e-2": (None, 6, 6), "x1e-3": (3, None, 3), "layers": (SLOW, None, 7)},
}


def run(h, b):
    hist = h.solve(b, tol=TOL, max_cycles=CAP)[1]
    return len(hist) - 1, hist[-1] / hist[0]


def check(count, ratio, want, what):
    if want is None or want is SLOW:
        assert count == CAP and ratio > (1e-3 if want is None else 1e-4), (what, count, ratio)
    else:
        assert count == want and ratio <= TOL, (what, count, ratio)


@pytest.mark.parametrize("kind", ["iso", "x1e-2", "y1e-2", "x1e-3", "layers"])
@pytest.mark.parametrize("L", [6, 5])
def test_cycle_counts_on_anisotropic_operators(po, L, kind):
    n = (1 << L) - 1
    st5 = operator5(po, L, kind)
    b = np.random.default_rng(3).uniform(-1, 1, (n, n))
    check(*run(gr.Hierarchy(po, st5, L, 3, mu1=2, mu2=2), b), TABLE[L][kind][0], (L, kind, "Jacobi V(2,2)"))
    for k, smoother in enumerate((lr.LINE_X, lr.LINE_Y, lr.LINE_ALT)):
        check(*run(lr.Hierarchy(smoother, po, st5, L, 3, mu1=1, mu2=1), b), TABLE[L][kind][1 + k], (L, kind, smoother))
    b = np.random.default_rng(SEED_STABLE).uniform(-1, 1, (n, n))
    for k, smoother in enumerate((lr.LINE_X, lr.LINE_Y, lr.LINE_ALT)):
        count, ratio = run(lr.Hierarchy(smoother, po, st5, L, 3, mu1=1, mu2=1), b)
        check(count, ratio, TABLE_STABLE[L][kind][k], (L, kind, smoother, "stable seed"))
        if ratio <= TOL:
            assert not 0.5 * TOL <= ratio <= 2.0 * TOL, ("a knife edge", L, kind, smoother, ratio)


def test_the_long_double_statement_follows_the_double_one(po):
    """NumpyOps (the transfers and the norm in numpy, for np.longdouble) against the oracle's: the same solve"""
    L = 5
    st5 = operator5(po, L, "layers")
    b = np.random.default_rng(SEED_STABLE).uniform(-1, 1, ((1 << L) - 1,) * 2)
    h64 = lr.Hierarchy(lr.LINE_ALT, po, st5, L, 3, mu1=1, mu2=1).solve(b, tol=TOL, max_cycles=CAP)[1]
    hld = lr.Hierarchy(lr.LINE_ALT, lr.NumpyOps, as_type(st5, np.longdouble), L, 3, np.longdouble, mu1=1, mu2=1).solve(b, tol=TOL, max_cycles=CAP)[1]
    assert len(h64) == len(hld) and np.allclose(h64, hld.astype(np.float64), rtol=1e-6, atol=0)
    for cycle, cls in ((1, lr.OpdepHierarchy), (2, lr.Hierarchy)):
        a = cls(lr.LINE_ALT, po, st5, L, 3, mu1=1, mu2=1, cycle=cycle).solve(b, tol=TOL, max_cycles=CAP)[1]
        c = cls(lr.LINE_ALT, lr.NumpyOps, as_type(st5, np.longdouble), L, 3, np.longdouble, mu1=1, mu2=1, cycle=cycle).solve(b, tol=TOL, max_cycles=CAP)[1]
        assert len(a) == len(c) <= len(h64) and np.allclose(a, c.astype(np.float64), rtol=1e-6, atol=0)
