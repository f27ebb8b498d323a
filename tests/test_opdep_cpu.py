"""CPU checks of the operator-dependent prolongation (mgx_build_galerkin_transfer(h, MGX_TRANSFER_OPERATOR)): the numpy
statement the GPU tests hold the device to (tests/opdep_ref.py) against scipy's P^T A P built from the same weights,
the constant-coefficient case (every weight exactly 1/2 or 1/4), P 1 = 1 where A has zero row sums, the convergence
the feature exists for, and the entry points in the header, the library and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import galerkin_ref as gr
import opdep_ref as od
from conftest import ROOT
from pcg_ref import contrast_coefficient
from test_galerkin_cpu import coefficient, sparse_of


def sparse_p(W):
    """P as a sparse (n_f^2 x n_c^2) matrix from the eight weight grids (and the coincident weight 1)"""
    nc = W[0].shape[0]
    nf = 2 * nc + 1
    I, J = np.meshgrid(np.arange(nc), np.arange(nc), indexing="ij")
    col = (I * nc + J).ravel()
    rows, cols, vals = [((2 * I + 1) * nf + 2 * J + 1).ravel()], [col], [np.ones(nc * nc)]
    for (oy, ox), k in od.WSLOT.items():
        rows.append(((2 * I + 1 + oy) * nf + 2 * J + 1 + ox).ravel())
        cols.append(col)
        vals.append(np.asarray(W[k], dtype=np.float64).ravel())
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nf * nf, nc * nc))


def coarse_entries(M, nc):
    """the nine coefficient grids of a sparse (n_c^2 x n_c^2) matrix, and the largest entry outside the 3 x 3 stencil"""
    idx = np.arange(nc * nc).reshape(nc, nc)
    out = [np.zeros((nc, nc)) for _ in range(9)]
    M = M.tocsr()
    seen = sp.csr_matrix(M.shape)
    for (dy, dx), o in gr.SLOT.items():
        ys, xs = slice(max(0, -dy), nc - max(0, dy)), slice(max(0, -dx), nc - max(0, dx))
        r, c = idx[ys, xs].ravel(), (idx[ys, xs] + dy * nc + dx).ravel()
        out[o][ys, xs] = np.asarray(M[r, c]).reshape(out[o][ys, xs].shape)
        seen = seen + sp.csr_matrix((np.ones(r.size), (r, c)), shape=M.shape)
    outside = abs(M - M.multiply(seen)).max() if M.nnz else 0.0
    return out, outside


KINDS = ["smooth", "jump", "contrast100"]


def nodes(L, kind):
    return contrast_coefficient(L, 100.0) if kind == "contrast100" else coefficient(L, kind)


@pytest.mark.parametrize("finest", [6, 7, 8, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_rap_is_scipy_s_triple_product_on_every_level(po, finest, kind):
    """entrywise within 200 eps (|P|^T |A| |P|): the forward bound of a sum of at most 81 products of three factors
    ((81 + 2) eps to first order, each weight itself carrying a few eps from its own formula on top)"""
    eps = np.finfo(np.float64).eps
    for mode in (gr.CONSISTENT, gr.FW16):
        h = od.Hierarchy(po, po.stencil_from_nodes(nodes(finest, kind), finest, finest), finest, 2, mode=mode)
        c = 0.25 if mode == gr.FW16 else 1.0
        for lv in range(finest, 2, -1):
            nc = (1 << (lv - 1)) - 1
            P, A = sparse_p(h.W[lv]), sparse_of(h.st[lv])
            want, outside = coarse_entries(c * (P.T @ A @ P), nc)
            bound, _ = coarse_entries(c * (abs(P).T @ abs(A) @ abs(P)), nc)
            assert outside <= 1e-9 * abs(A).max(), (lv, "P^T A P is not nine-point")
            for o in range(9):
                assert np.all(np.abs(h.st[lv - 1][o] - want[o]) <= 200 * eps * bound[o]), (kind, mode, lv, gr.SLOTS[o])


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_constant_coefficient_gives_the_bilinear_weights_exactly(po, dt):
    L = 8
    eps = np.finfo(dt).eps
    st5 = po.stencil_from_nodes(coefficient(L, "one"), L, L)
    h = od.Hierarchy(po, st5, L, 2, dt)
    ref = gr.Hierarchy(po, st5, L, 2, dt)
    for lv in range(L, 2, -1):
        for k in range(8):
            assert np.all(h.W[lv][k] == (0.5 if k < 4 else 0.25)), (lv, od.DIRS[k])
        nc = (1 << (lv - 1)) - 1
        P = sparse_p(od.bilinear_weights(nc))
        bound, _ = coarse_entries(abs(P).T @ abs(sparse_of(ref.st[lv])).astype(np.float64) @ abs(P), nc)
        for o in range(9):
            assert np.all(np.abs(h.st[lv - 1][o].astype(np.float64) - ref.st[lv - 1][o]) <= 200 * eps * bound[o]), (lv, gr.SLOTS[o])


@pytest.mark.parametrize("kind", KINDS)
def test_constants_are_interpolated_exactly_where_the_row_sums_vanish(po, kind):
    """-div(a grad u) has zero row sums away from the Dirichlet ring, and so has every Galerkin coarse operator as long
    as P 1 = 1 there: checked on every level, two points away from the ring"""
    L = 8
    h = od.Hierarchy(po, po.stencil_from_nodes(nodes(L, kind), L, L), L, 3)
    for lv in range(L, 3, -1):
        one = od.prolong(np.ones_like(h.W[lv][0]), h.W[lv])
        assert np.max(np.abs(one[2:-2, 2:-2] - 1.0)) <= 1e-14, lv


def cycles_to(h, b, tol, limit):
    u, hist = h.solve(b, tol=tol, max_cycles=limit)
    return len(hist) - 1, hist[-1] <= tol * hist[0], hist[-1] / hist[0]


@pytest.mark.parametrize("contrast", [10.0, 100.0, 1000.0])
def test_operator_dependent_p_needs_fewer_cycles_than_bilinear_p(po, contrast):
    """why the feature exists: contrast_coefficient(9, c), levels 9..5, V(2,2), omega 2/3, constant right-hand side, 1e-8.
    Recorded with this reference: contrast 10: 24 cycles BILINEAR / 20 OPERATOR; 100: 61 / 39; 1000: BILINEAR not converged
    in 120 cycles / OPERATOR 46."""
    L = 9
    st5 = po.stencil_from_nodes(contrast_coefficient(L, contrast), L, L)
    b = po.rhs_constant(L)
    nb, okb, fb = cycles_to(gr.Hierarchy(po, st5, L, 5), b, 1e-8, 120)
    no, oko, fo = cycles_to(od.Hierarchy(po, st5, L, 5), b, 1e-8, 120)
    print(f"contrast {contrast:g}: BILINEAR {nb} cycles (converged {okb}, {fb:.3e}), OPERATOR {no} cycles (converged {oko}, {fo:.3e})")
    assert oko
    if contrast == 1000.0:
        assert not okb
    else:
        assert okb and no < nb


def test_fallback_to_the_bilinear_weight_where_a_denominator_vanishes():
    """mgx.h: a zero or non-finite denominator gives that point the bilinear weight"""
    L = 4
    n = (1 << L) - 1
    st = gr.nine([np.full((n, n), 4.0)] + [np.full((n, n), -1.0) for _ in range(4)])
    st[0][2, 1] = 2.0                  # fine (3, 2): on coarse column 1, between coarse rows 1 and 2: den = w + c + e = 0
    st[0][4, 4] = 0.0                  # fine (5, 5): a cell centre with c = 0
    st[0][6, 3] = np.inf               # fine (7, 4): den not finite
    W = od.weights(st, 1 << L)
    assert all(np.isfinite(w).all() for w in W)
    assert W[od.WSLOT[1, 0]][0, 0] == 0.5 and W[od.WSLOT[-1, 0]][1, 0] == 0.5
    assert W[od.WSLOT[1, 1]][1, 1] == 0.25 and W[od.WSLOT[-1, -1]][2, 2] == 0.25
    assert W[od.WSLOT[1, 0]][2, 1] == 0.5 and W[od.WSLOT[-1, 0]][3, 1] == 0.5


def test_header_library_and_binding_have_the_entry_points(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"MGX_API\s+int\s+(mgx_\w+)\s*\(([^;]*)\);", text)}
    assert decl["mgx_build_galerkin_transfer"].count(",") == 1
    assert decl["mgx_get_transfer"].count(",") == 1
    assert decl["mgx_get_prolongation"].count(",") == 4
    assert re.search(r"MGX_TRANSFER_BILINEAR\s*=\s*0\b", text) and re.search(r"MGX_TRANSFER_OPERATOR\s*=\s*1\b", text)
    assert (pkg.TRANSFER_BILINEAR, pkg.TRANSFER_OPERATOR) == (0, 1)
    L = C.CDLL(pkg.LIB_PATH)
    names = {"mgx_build_galerkin_transfer", "mgx_get_transfer", "mgx_get_prolongation"}
    assert all(hasattr(L, n) for n in names) and names <= set(pkg.EXPORTS)
    assert len(pkg.lib().mgx_build_galerkin_transfer.argtypes) == 2 and len(pkg.lib().mgx_get_prolongation.argtypes) == 5
    assert all(hasattr(pkg.Multigrid, n) for n in ("build_galerkin", "get_prolongation", "transfer"))
    # a NULL handle is an invalid argument, not a crash (no GPU is touched)
    out = C.c_int(7)
    assert pkg.lib().mgx_build_galerkin_transfer(None, 1) == 1
    assert pkg.lib().mgx_get_prolongation(None, 5, 0, None, 0) == 1
    assert pkg.lib().mgx_get_transfer(None, C.byref(out)) == 1 and out.value == 7


def test_struct_sizes_are_unchanged(pkg):
    """no field is added to mgx_config, mgx_slab or mgx_stats (sizes of the release before this entry point)"""
    assert (C.sizeof(pkg.Config), C.sizeof(pkg.Slab), C.sizeof(pkg.Stats)) == (144, 20, 48)
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    for name, fields in (("mgx_config", pkg.Config._fields_), ("mgx_slab", pkg.Slab._fields_), ("mgx_stats", pkg.Stats._fields_)):
        body = re.search(r"typedef struct\s*\{([^}]*)\}\s*%s\s*;" % name, text).group(1)
        body = re.sub(r"/\*.*?\*/|//[^\n]*", "", body, flags=re.S)
        assert len([d for d in body.split(";") if d.strip()]) == len(fields), name


def pointwise_p(st9, N_f):
    """P built fine point by fine point from the wording of include/mgx.h, independently of opdep_ref.weights: a dict
    (fine i, fine j) -> {(coarse I, coarse J): weight} in grid indices, ring coarse points included"""
    q = {name: np.pad(np.asarray(st9[k], dtype=np.float64), 1) for k, name in enumerate(gr.SLOTS)}   # grid-indexed

    def hweights(i, j):                # fine point on a coarse row, between two coarse columns: (west, east)
        den = q["n"][i, j] + q["c"][i, j] + q["s"][i, j]
        return -(q["nw"][i, j] + q["w"][i, j] + q["sw"][i, j]) / den, -(q["ne"][i, j] + q["e"][i, j] + q["se"][i, j]) / den

    def vweights(i, j):                # fine point on a coarse column: (north, south)
        den = q["w"][i, j] + q["c"][i, j] + q["e"][i, j]
        return -(q["nw"][i, j] + q["n"][i, j] + q["ne"][i, j]) / den, -(q["sw"][i, j] + q["s"][i, j] + q["se"][i, j]) / den

    P = {}
    for i in range(1, N_f):
        for j in range(1, N_f):
            if i % 2 == 0 and j % 2 == 0:
                P[i, j] = {(i // 2, j // 2): 1.0}
            elif i % 2 == 0:
                w, e = hweights(i, j)
                P[i, j] = {(i // 2, (j - 1) // 2): w, (i // 2, (j + 1) // 2): e}
            elif j % 2 == 0:
                n, s = vweights(i, j)
                P[i, j] = {((i - 1) // 2, j // 2): n, ((i + 1) // 2, j // 2): s}
            else:
                hWn, hEn = hweights(i - 1, j)          # the north neighbour lies on a coarse row
                hWs, hEs = hweights(i + 1, j)
                vNw, vSw = vweights(i, j - 1)          # the west neighbour lies on a coarse column
                vNe, vSe = vweights(i, j + 1)
                c = q["c"][i, j]
                n, s, w, e = q["n"][i, j], q["s"][i, j], q["w"][i, j], q["e"][i, j]
                I0, I1, J0, J1 = (i - 1) // 2, (i + 1) // 2, (j - 1) // 2, (j + 1) // 2
                P[i, j] = {(I0, J0): -(q["nw"][i, j] + n * hWn + w * vNw) / c, (I0, J1): -(q["ne"][i, j] + n * hEn + e * vNe) / c,
                           (I1, J0): -(q["sw"][i, j] + s * hWs + w * vSw) / c, (I1, J1): -(q["se"][i, j] + s * hEs + e * vSe) / c}
    return P


@pytest.mark.parametrize("kind", ["jump", "nonsymmetric"])
def test_weights_are_the_header_s_definition_fine_point_by_fine_point(po, kind):
    """the eight coarse-point-centred grids of opdep_ref.weights against P assembled per fine point, on a five-point
    level and on the nine-point level below it; 1e-13: a handful of operations on numbers of order one"""
    L = 5
    if kind == "jump":
        st = gr.nine(po.stencil_from_nodes(contrast_coefficient(L, 100.0)[:(1 << L) + 1, :(1 << L) + 1], L, L))
    else:
        from test_galerkin_cpu import random_stencil5
        st = gr.nine(random_stencil5(L, 11))
    for lv in (L, L - 1):
        N_f = 1 << lv
        W = od.weights(st, N_f)
        with np.errstate(all="ignore"):        # (the padded ring's zero stencils divide 0 by 0; those entries are not used)
            P = pointwise_p(st, N_f)
        nc = N_f // 2 - 1
        for (oy, ox), k in od.WSLOT.items():
            want = np.array([[P[2 * I + oy, 2 * J + ox][I, J] for J in range(1, nc + 1)] for I in range(1, nc + 1)])
            assert np.max(np.abs(W[k] - want)) <= 1e-13, (lv, od.DIRS[k])
        st = od.rap(st, W, N_f)
