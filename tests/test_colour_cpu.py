"""CPU checks of the multicolour Gauss-Seidel smoothers' numpy statement (tests/colour_ref.py), the one the GPU tests hold
the device to: a sweep is the sequential Gauss-Seidel loop colour by colour, the exact solution is a fixed point, the
points of a colour do not read each other, and the V(1,1) cycle with the post-smoothing colours in reverse order is a
symmetric operator while the forward-only one is not.  Plus the interface pins that need no GPU."""
import os
import re

import numpy as np
import pytest

import colour_ref as cf
import galerkin_ref as gr
import line_ref as lr
import nine_ref as nr
from conftest import ROOT


def coefficient_stencil(a):
    """(c, n, s, w, e) of -div(a grad u) from the nodal coefficient a ((N + 1)^2 nodes): a face coefficient is the mean of
    its two nodes (the form of mgx_set_coefficient); w(i, j) = e(i, j - 1) and n(i, j) = s(i - 1, j) bit for bit"""
    ctr = a[1:-1, 1:-1]
    fn, fs = 0.5 * (ctr + a[:-2, 1:-1]), 0.5 * (ctr + a[2:, 1:-1])
    fw, fe = 0.5 * (ctr + a[1:-1, :-2]), 0.5 * (ctr + a[1:-1, 2:])
    return [((fn + fw) + fe) + fs, -fn, -fs, -fw, -fe]


def random_coefficient(L, seed):
    """a = exp(U(0, ln 10)) on the nodes of level L"""
    N = 1 << L
    return np.exp(np.random.default_rng(seed).uniform(0.0, np.log(10.0), (N + 1, N + 1)))


def operator(nine, L, dt, seed=0):
    """a diagonally dominant operator with values in the ring-pointing places too: five-point from a random nodal
    coefficient, nine-point unsymmetric with corners (nine_ref.random_stencil9)"""
    if nine:
        return nr.random_stencil9(L, seed, dt)
    return gr.nine([x.astype(dt) for x in coefficient_stencil(random_coefficient(L, seed))])


def scalar_gauss_seidel(st9, v, b, nine, reverse):
    """the sweep as a sequential loop: the colours in order, within a colour the points row by row, every operation a
    scalar operation of the working type"""
    n = v.shape[0]
    dt = v.dtype.type
    v = v.copy()
    order = list(range(4 if nine else 2))
    for k in (order[::-1] if reverse else order):
        for i in range(n):
            for j in range(n):
                colour = (2 * (i % 2) + (j % 2)) if nine else (i + j) % 2
                if colour != k:
                    continue
                acc = None
                for dy, dx in cf.OFFDIAG:
                    if not nine and dy != 0 and dx != 0:
                        continue
                    inside = 0 <= i + dy < n and 0 <= j + dx < n
                    term = dt(st9[gr.SLOT[dy, dx]][i, j]) * (dt(v[i + dy, j + dx]) if inside else dt(0))
                    acc = term if acc is None else dt(acc + term)
                v[i, j] = dt(dt(b[i, j]) - acc) * (dt(1) / dt(st9[0][i, j]))
    return v


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nine", [False, True], ids=["five", "nine"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_a_sweep_is_the_sequential_loop_colour_by_colour(nine, reverse, dt):
    n = 7
    st9 = operator(nine, 3, dt, seed=11)
    rng = np.random.default_rng(12)
    v, b = rng.uniform(-1, 1, (n, n)).astype(dt), rng.uniform(-1, 1, (n, n)).astype(dt)
    got = cf.sweep(st9, cf.dinv_of(st9), v, b, nine, reverse)
    assert got.dtype == dt
    assert np.array_equal(got, scalar_gauss_seidel(st9, v, b, nine, reverse))
    assert not np.array_equal(got, cf.sweep(st9, cf.dinv_of(st9), v, b, nine, not reverse))


def test_the_colour_orders_are_the_documented_ones():
    """five-point: (grid row + grid column) even first; nine-point: (odd, odd), (odd, even), (even, odd), (even, even) in
    grid parities, the coarse points last.  Interior index k is grid index k + 1"""
    five, nine = cf.colours(5, False), cf.colours(5, True)
    assert five[0][0, 0] and five[1][0, 1] and five[0][1, 1]                     # grid (1, 1): 1 + 1 even
    assert nine[0][0, 0] and nine[1][0, 1] and nine[2][1, 0] and nine[3][1, 1]   # grid (1, 1), (1, 2), (2, 1), (2, 2)
    for masks in (five, nine):
        assert (sum(m.astype(int) for m in masks) == 1).all()


@pytest.mark.parametrize("nine", [False, True], ids=["five", "nine"])
def test_the_exact_solution_is_a_fixed_point(nine):
    """b = A u formed in long double; a sweep in double then moves u by rounding only.  Every update is NQ + 1 rounded
    operations on terms of size at most 2 max|u| (the operators are diagonally dominant), and a later colour reads the
    perturbed values of the earlier ones: at most colours x 2 (NQ + 1) eps max|u|"""
    L, n = 4, 15
    st9 = operator(nine, L, np.float64, seed=21)
    u = np.random.default_rng(22).uniform(-1, 1, (n, n))
    wide = [a.astype(np.longdouble) for a in st9]
    b = gr._apply9(wide, wide[0], u.astype(np.longdouble))              # (a five-point operator carries zero corners)
    nq, ncol = (9, 4) if nine else (5, 2)
    for reverse in (False, True):
        got = cf.sweep(st9, cf.dinv_of(st9), u, b.astype(np.float64), nine, reverse)
        assert np.max(np.abs(got - u)) <= ncol * 2 * (nq + 1) * np.finfo(np.float64).eps * np.max(np.abs(u))


@pytest.mark.parametrize("nine", [False, True], ids=["five", "nine"])
def test_points_of_one_colour_do_not_read_each_other(nine):
    """perturbing a value of colour k changes no value of colour k after that colour's update: the update of a colour is
    a function of the other colours only (so the order within a colour, and a launch that updates it in place, are free)"""
    n = 9
    st9 = operator(nine, 3, np.float64, seed=31)[:]
    st9 = [np.pad(a, 1, mode="edge") for a in st9]                      # 9 x 9 from 7 x 7: any values do
    dinv = cf.dinv_of(st9)
    rng = np.random.default_rng(32)
    v, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    for k, mask in enumerate(cf.colours(n, nine)):
        base = np.where(mask, (b - cf.offdiag_sum(st9, v, nine)) * dinv, v)
        for i, j in np.argwhere(mask)[::3]:
            w = v.copy()
            w[i, j] += 1.0
            moved = np.where(mask, (b - cf.offdiag_sum(st9, w, nine)) * dinv, w)
            assert np.array_equal(moved[mask], base[mask]), (k, i, j)
            assert not np.array_equal(cf.offdiag_sum(st9, w, nine), cf.offdiag_sum(st9, v, nine))      # the others do read it


def symmetry_defect(h, seed):
    """|<M x, y> - <x, M y>| / |<M x, y>| of one cycle M of h from zero"""
    n = (1 << h.L) - 1
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    zero = np.zeros((n, n))
    mx, my = h.vcycle(h.L, zero, x), h.vcycle(h.L, zero, y)
    a, c = float(np.sum(mx * y)), float(np.sum(x * my))
    return abs(a - c) / abs(a)


@pytest.mark.parametrize("nine", [False, True], ids=["five", "nine"])
def test_the_sgs_cycle_is_symmetric_and_the_gs_cycle_is_not(nine):
    """V(1,1) from zero on levels 5..3, bilinear P, R = P^T, exact bottom solve: a symmetric five-point operator (random
    nodal coefficient) and a symmetric nine-point one (the rotated anisotropy of nine_ref, 45 degrees, eps = 0.5)"""
    L, Lc = 5, 3
    if nine:
        op = nr.tensor9(*nr.rotated_tensor(L, 45.0, 0.5))
        cls = cf.NineHierarchy
    else:
        op = coefficient_stencil(random_coefficient(L, 41))
        cls = cf.Hierarchy
    defect = {}
    for smoother in (cf.COLOR_GS, cf.COLOR_SGS):
        h = cls(smoother, lr.NumpyOps, op, L, Lc, np.float64, mu1=1, mu2=1)
        defect[smoother] = max(symmetry_defect(h, seed) for seed in (42, 43))
    print(f"symmetry defect of the V(1,1) cycle: GS {defect[cf.COLOR_GS]:.3e}, SGS {defect[cf.COLOR_SGS]:.3e}")
    assert defect[cf.COLOR_SGS] <= 1e-12
    assert defect[cf.COLOR_GS] > 1e-4


def test_the_bottom_smooth_visit_sweeps_forward_then_in_reverse():
    """bottom = SMOOTH on a one-level 'hierarchy': mu1 forward sweeps, then mu2 reverse ones under COLOR_SGS"""
    L, n = 3, 7
    op = coefficient_stencil(random_coefficient(L, 51))
    st9 = gr.nine(op)
    rng = np.random.default_rng(52)
    v, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    d = cf.dinv_of(st9)
    for smoother, rev in ((cf.COLOR_GS, False), (cf.COLOR_SGS, True)):
        h = cf.Hierarchy(smoother, lr.NumpyOps, op, L, L, np.float64, mu1=2, mu2=1, bottom=gr.SMOOTH)
        want = cf.smooth(st9, d, cf.smooth(st9, d, v, b, 2, False, False), b, 1, False, rev)
        assert np.array_equal(h.vcycle(L, v, b), want)


def test_the_enum_values_are_pinned(pkg):
    """8 and 9: the value 7 stays an invalid smoother (tests/test_gpu_line.py has pinned its refusal on a GALERKIN handle
    since the line smoothers took 4, 5 and 6), as 3 does"""
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert re.search(r"MGX_SMOOTHER_COLOR_GS\s*=\s*8\b", hdr) and re.search(r"MGX_SMOOTHER_COLOR_SGS\s*=\s*9\b", hdr)
    assert re.search(r"MGX_SMOOTHER_RBGS\s*=\s*1\b", hdr) and re.search(r"MGX_SMOOTHER_LINE_ALT\s*=\s*6\b", hdr)
    assert (pkg.SMOOTHER_COLOR_GS, pkg.SMOOTHER_COLOR_SGS) == (8, 9) == (cf.COLOR_GS, cf.COLOR_SGS)


def test_the_plan_refuses_the_smoothers(pkg):
    """mgx_plan_create is host logic: the refusal needs no GPU"""
    for smoother in (8, 9):
        with pytest.raises(pkg.MgxError, match="COLOR_GS"):
            pkg.Plan(2, 0, finest_level=9, coarsest_level=5, smoother=smoother)
    pkg.Plan(2, 0, finest_level=9, coarsest_level=5).close()
