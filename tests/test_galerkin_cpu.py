"""CPU checks of the Galerkin hierarchy (op = MGX_OPERATOR_GALERKIN): the numpy statement the GPU tests hold the
device to (tests/galerkin_ref.py) against scipy's P^T A P, the Poisson coarse stencil, symmetry, the convergence the
feature exists for, and the two entry points in the header, the library and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import galerkin_ref as gr
from conftest import ROOT
from pcg_ref import contrast_coefficient


def coefficient(L, kind):
    N = 1 << L
    if kind == "one":
        return np.ones((N + 1, N + 1))
    if kind == "smooth":
        x = np.linspace(0.0, 1.0, N + 1)
        return 1.0 + 0.5 * np.sin(2 * np.pi * x)[None, :] * np.cos(np.pi * x)[:, None]
    return contrast_coefficient(L, 100.0)


def random_stencil5(L, seed, c_lo=3.0, c_hi=5.0):
    """a seeded non-symmetric five-point operator (c, n, s, w, e): c in [c_lo, c_hi], every off-diagonal drawn on its
    own in [-1, -0.5], so A(i, i+d) != A(i+d, i) and the four directions differ"""
    n = (1 << L) - 1
    rng = np.random.default_rng(seed)
    return [rng.uniform(c_lo, c_hi, (n, n))] + [-rng.uniform(0.5, 1.0, (n, n)) for _ in range(4)]


def with_ring_values(st5, seed, big=1e30):
    """the same operator with the coefficients that point at the Dirichlet ring (n on row 1, s on row n, w on column 1,
    e on column n) overwritten by finite values of mixed sign and magnitudes from 1 to `big` (float32 holds 1e30)"""
    rng = np.random.default_rng(seed)
    out = [np.array(x, copy=True) for x in st5]
    n = out[0].shape[0]

    def junk():
        return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(0.0, np.log10(big), n)
    out[1][0, :], out[2][-1, :], out[3][:, 0], out[4][:, -1] = junk(), junk(), junk(), junk()
    return out


def sparse_of(st9):
    n = st9[0].shape[0]
    idx = np.arange(n * n).reshape(n, n)
    rows, cols, vals = [], [], []
    for (dy, dx), o in gr.SLOT.items():
        ys = slice(max(0, -dy), n - max(0, dy))
        xs = slice(max(0, -dx), n - max(0, dx))
        rows.append(idx[ys, xs].ravel())
        cols.append((idx[ys, xs] + dy * n + dx).ravel())
        vals.append(st9[o][ys, xs].ravel())
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n * n, n * n))


def prolongation(L):
    """bilinear P from level L - 1 to level L: the Kronecker product of the 1-D matrix"""
    nf, nc = (1 << L) - 1, (1 << (L - 1)) - 1
    r, c, v = [], [], []
    for I in range(nc):
        for d, w in ((-1, 0.5), (0, 1.0), (1, 0.5)):
            r.append(2 * I + 1 + d), c.append(I), v.append(w)
    p = sp.csr_matrix((v, (r, c)), shape=(nf, nc))
    return sp.kron(p, p).tocsr()


@pytest.mark.parametrize("L", [5, 6])
@pytest.mark.parametrize("kind", ["one", "smooth", "jump"])
@pytest.mark.parametrize("mode", [gr.CONSISTENT, gr.FW16])
def test_rap_is_scipy_s_triple_product(po, L, kind, mode):
    st = gr.nine(po.stencil_from_nodes(coefficient(L, kind), L, L))
    for lv in (L, L - 1):                       # five-point -> nine-point, then nine-point -> nine-point
        got = gr.rap(st, 1 << lv, mode)
        P = prolongation(lv)
        want = (P.T @ sparse_of(st) @ P).toarray() * (0.25 if mode == gr.FW16 else 1.0)
        scale = np.max(np.abs(want))
        assert np.max(np.abs(gr.dense(got) - want)) <= 1e-12 * scale
        # symmetric within rounding: A_c(I, I+D) = A_c(I+D, -D)
        M = gr.dense(got)
        assert np.max(np.abs(M - M.T)) <= 1e-12 * scale
        st = got


@pytest.mark.parametrize("L", [5, 6])
@pytest.mark.parametrize("mode", [gr.CONSISTENT, gr.FW16])
def test_rap_of_a_non_symmetric_operator_is_scipy_s_triple_product(L, mode):
    """R A P, not a formula that leans on A = A^T: c in [4, 5] against off-diagonals in [-1, -0.5] is diagonally
    dominant, and A(i, i+d) != A(i+d, i) in all four directions"""
    st5 = random_stencil5(L, 40 + L, c_lo=4.0)
    assert np.all(st5[0] >= -(st5[1] + st5[2] + st5[3] + st5[4]))
    A = sparse_of(gr.nine(st5)).toarray()
    assert np.max(np.abs(A - A.T)) > 0.1
    st = gr.nine(st5)
    for lv in (L, L - 1):
        got = gr.rap(st, 1 << lv, mode)
        P = prolongation(lv)
        want = (P.T @ sparse_of(st) @ P).toarray() * (0.25 if mode == gr.FW16 else 1.0)
        scale = np.max(np.abs(want))
        assert np.max(np.abs(gr.dense(got) - want)) <= 1e-12 * scale
        M = gr.dense(got)
        assert np.max(np.abs(M - M.T)) > 1e-3 * scale           # the coarse operator is not symmetric either
        st = got


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("mode", [gr.CONSISTENT, gr.FW16])
def test_rap_ignores_what_the_ring_pointing_coefficients_hold(dt, mode):
    """mgx.h: coefficients that point at the eliminated Dirichlet ring are ignored.  They only ever enter coarse
    coefficients that point at the coarse ring, and those are written as zeros: values up to 1e30 leave no trace"""
    L = 6
    st5 = random_stencil5(L, 7)
    zeroed = [x.copy() for x in st5]
    zeroed[1][0, :], zeroed[2][-1, :], zeroed[3][:, 0], zeroed[4][:, -1] = 0.0, 0.0, 0.0, 0.0
    junk = with_ring_values(st5, 8)
    assert np.max(np.abs(junk[1][0])) > 1e20 and np.isfinite(np.asarray(junk, dtype=dt)).all()
    a = gr.rap(gr.nine([x.astype(dt) for x in zeroed]), 1 << L, mode)
    b = gr.rap(gr.nine([x.astype(dt) for x in junk]), 1 << L, mode)
    for o in range(9):
        assert np.array_equal(a[o], b[o]), gr.SLOTS[o]


def test_fmg_then_v22_converges_on_the_jump_problem(po):
    """schedule = FMG in the reference: one FMG pass, then V(2,2) cycles, L = 7 down to 4, contrast 100.
    Recorded: 44 cycles to 1e-8, the FMG pass counted as the first (plain V(2,2) cycles from zero: 45).  Bound: a third
    over, as for the V-cycle counts below"""
    L = 7
    h = gr.Hierarchy(po, po.stencil_from_nodes(coefficient(L, "jump"), L, L), L, 4)
    u, hist = h.solve(po.rhs_constant(L), tol=1e-8, max_cycles=58, schedule=gr.FMG)
    print(f"FMG + V(2,2), jump, L = 7: {len(hist) - 1} cycles, final {hist[-1] / hist[0]:.3e}")
    assert hist[-1] <= 1e-8 * hist[0] and len(hist) - 1 <= 58
    # the first cycle is the FMG pass, not a V-cycle from the zero guess
    assert not np.isclose(hist[1], h.solve(po.rhs_constant(L), max_cycles=1)[1][1], rtol=1e-3)


@pytest.mark.parametrize("bottom", [gr.EXACT, gr.SMOOTH])
def test_fw16_and_consistent_give_the_same_fmg_iterate(po, bottom):
    """mgx.h: the two modes give coarse operators that differ by an exact factor 4 per level, "and the same
    iterates": the restricted right-hand sides carry the same factor"""
    L = 7
    st5 = po.stencil_from_nodes(coefficient(L, "jump"), L, L)
    b = po.rhs_sine(L)
    u = [gr.Hierarchy(po, st5, L, 4, mode=mode, mu0=1, bottom=bottom).fmg(b) for mode in (gr.CONSISTENT, gr.FW16)]
    assert np.max(np.abs(u[0] - u[1])) <= 1e-12 * np.max(np.abs(u[0]))
    # ... and not a trivial one: the pass reduced the residual of the zero guess
    h = gr.Hierarchy(po, st5, L, 4, mu0=1, bottom=bottom)
    assert po.norm2(h.residual(L, u[0], b)) < po.norm2(b)


def test_bottom_smooth_is_mu1_plus_mu2_sweeps_from_the_guess(po):
    L = 5
    st5 = po.stencil_from_nodes(coefficient(L, "smooth"), L, L)
    h = gr.Hierarchy(po, st5, L, 3, mu1=3, mu2=1, bottom=gr.SMOOTH)
    rng = np.random.default_rng(0)
    v, b = rng.uniform(-1, 1, (7, 7)), rng.uniform(-1, 1, (7, 7))
    assert np.array_equal(h.vcycle(3, v, b), gr.jacobi9(v, b, 4, h.omega, h.jac[3]))


def test_poisson_coarse_stencil_is_3_half_quarter(po):
    L = 6
    st = gr.nine(po.stencil_from_nodes(coefficient(L, "one"), L, L))
    c = gr.rap(st, 1 << L, gr.CONSISTENT)
    q = gr.rap(st, 1 << L, gr.FW16)
    inner = (slice(1, -1), slice(1, -1))
    for o, want in zip(range(9), (3.0, -0.5, -0.5, -0.5, -0.5, -0.25, -0.25, -0.25, -0.25)):
        assert np.all(c[o][inner] == want), gr.SLOTS[o]
        assert np.array_equal(q[o], 0.25 * c[o]), gr.SLOTS[o]
    # coefficients that point at the Dirichlet ring are zero
    assert not c[gr.SLOT[-1, 0]][0].any() and not c[gr.SLOT[1, 1]][:, -1].any() and not c[gr.SLOT[1, 1]][-1].any()


def test_modes_differ_by_an_exact_factor_four_per_level(po):
    L = 6
    st = gr.nine(po.stencil_from_nodes(coefficient(L, "jump"), L, L))
    c1, q1 = gr.rap(st, 1 << L, gr.CONSISTENT), gr.rap(st, 1 << L, gr.FW16)
    c2, q2 = gr.rap(c1, 1 << (L - 1), gr.CONSISTENT), gr.rap(q1, 1 << (L - 1), gr.FW16)
    for o in range(9):
        assert np.array_equal(c1[o], 4.0 * q1[o]) and np.array_equal(c2[o], 16.0 * q2[o])


@pytest.mark.parametrize("contrast,limit", [(100.0, 80), (10.0, 32)])
def test_galerkin_v_cycles_converge_where_rediscretised_ones_do_not(po, contrast, limit):
    """why the feature exists.  scipy statement of the same hierarchy: 61 cycles at contrast 100, 24 at contrast 10
    (bounds: a third over, for rounding-order differences near the threshold)"""
    L = 9
    a = contrast_coefficient(L, contrast)
    b = po.rhs_constant(L)
    h = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, 5)
    u, hist = h.solve(b, tol=1e-8, max_cycles=limit)
    print(f"contrast {contrast:g}: {len(hist) - 1} cycles, final {hist[-1] / hist[0]:.3e}")
    assert hist[-1] <= 1e-8 * hist[0] and len(hist) - 1 <= limit
    if contrast == 100.0:
        s = po.Solver(finest_level=L, coarsest_level=5, mu1=2, mu2=2, schedule=0, op=1)
        s.set_coefficient(a)
        _, hv = s.solve(b, None, tol=1e-8, max_cycles=60)
        assert not (hv[-1] <= 1e-8 * hv[0])


def test_header_library_and_binding_have_the_entry_points(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"MGX_API\s+int\s+(mgx_\w+)\s*\(([^;]*)\);", text)}
    assert decl["mgx_build_galerkin"].count(",") == 0 and "mgx_handle" in decl["mgx_build_galerkin"]
    assert decl["mgx_get_stencil9"].count(",") == 4
    assert re.search(r"MGX_OPERATOR_GALERKIN\s*=\s*%d\b" % pkg.OP_GALERKIN, text)
    L = C.CDLL(pkg.LIB_PATH)
    assert hasattr(L, "mgx_build_galerkin") and hasattr(L, "mgx_get_stencil9")
    assert {"mgx_build_galerkin", "mgx_get_stencil9"} <= set(pkg.EXPORTS)
    assert len(pkg.lib().mgx_build_galerkin.argtypes) == 1 and len(pkg.lib().mgx_get_stencil9.argtypes) == 5
    assert callable(getattr(pkg.Multigrid, "build_galerkin", None)) and callable(getattr(pkg.Multigrid, "get_stencil9", None))
    # a NULL handle is an invalid argument, not a crash (no GPU is touched)
    assert pkg.lib().mgx_build_galerkin(None) == 1 and pkg.lib().mgx_get_stencil9(None, 5, 0, None, 0) == 1
