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
