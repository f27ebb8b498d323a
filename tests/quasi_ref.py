"""numpy statement of mgx_quasi (include/mgx.h, csrc/mgx_quasi.hpp) on top of tests/newton_ref.py: the fused pass operation
by operation (both methods, first evaluation and trial), the Armijo test, and the loop around any linear solve and any
norm.  numpy rounds every elementwise operation on its own, which is what the kernel does, so the pass is meant bit for
bit: the coefficient arithmetic in float64 with one rounding to the working type per coefficient, everything on u in
the working type.

The problem: F(u) = A(u) u - f, A(u) the five-point discretisation of -div(a k(u) grad u) that mgx_set_coefficient forms
from the nodal a k(u), k(u) = k0 + k1 u + k2 u^2, on the interior n x n grid; a_nodes are the (N + 1)^2 nodal values of a,
boundary nodes included; u vanishes on the ring."""
import numpy as np

import galerkin_ref as gr
import newton_ref as nwr
import theta_ref as tr

PICARD, NEWTON = 0, 1
armijo = nwr.armijo
norm2 = nwr.norm2


def quasi_pass(a_nodes, k, f, u, de=None, lam=None, method=PICARD):
    """the pass: v = u (de is None) or u + lam * de in u's dtype; returns (v, b, coefs, picard): b = f - A(v) v, coefs the
    five grids (c, n, s, w, e) the pass writes - A(v) for PICARD, the Jacobian of F at v for NEWTON - and picard the
    five grids of A(v) the residual uses either way, all in u's dtype"""
    dt = u.dtype
    a = np.ascontiguousarray(a_nodes, dtype=np.float64)
    N = a.shape[0] - 1
    assert a.shape == (N + 1, N + 1) and u.shape == (N - 1, N - 1)
    k0, k1, k2 = (np.float64(x) for x in k)
    kk2 = np.float64(2.0 * float(k[2]))
    v = u if de is None else u + dt.type(lam) * np.asarray(de, dtype=dt)
    vd = np.zeros((N + 1, N + 1), dtype=np.float64)          # the ring of v is zero
    vd[1:N, 1:N] = v.astype(np.float64)
    kap = a * ((k2 * vd + k1) * vd + k0)
    P, Nn, S, W, E = (slice(1, N), slice(1, N)), (slice(0, N - 1), slice(1, N)), (slice(2, N + 1), slice(1, N)), \
                     (slice(1, N), slice(0, N - 1)), (slice(1, N), slice(2, N + 1))
    fn, fs = 0.5 * (kap[P] + kap[Nn]), 0.5 * (kap[P] + kap[S])
    fw, fe = 0.5 * (kap[P] + kap[W]), 0.5 * (kap[P] + kap[E])
    ctr = ((fn + fw) + fe) + fs
    picard = [x.astype(dt) for x in (ctr, -fn, -fs, -fw, -fe)]
    q = tr.apply(gr.nine(picard), v)
    b = np.asarray(f, dtype=dt) - q
    if method == PICARD:
        return v, b, [np.array(x, copy=True) for x in picard], picard
    dk = a * (kk2 * vd + k1)
    gN, gS, gW, gE = vd[P] - vd[Nn], vd[P] - vd[S], vd[P] - vd[W], vd[P] - vd[E]
    sg = ((gN + gW) + gE) + gS
    cJ = ctr + (0.5 * dk[P]) * sg
    nJ, sJ = (0.5 * dk[Nn]) * gN - fn, (0.5 * dk[S]) * gS - fs
    wJ, eJ = (0.5 * dk[W]) * gW - fw, (0.5 * dk[E]) * gE - fe
    return v, b, [x.astype(dt) for x in (cJ, nJ, sJ, wJ, eJ)], picard


def residual(a_nodes, k, f, u):
    """-F(u) = f - A(u) u in float64 (for difference quotients)"""
    return quasi_pass(a_nodes, k, np.asarray(f, dtype=np.float64), np.asarray(u, dtype=np.float64))[1]


def quasi(a_nodes, k, f, u0, solve, tol, max_iters, max_backtracks, method=PICARD, norm=norm2):
    """the loop of mgx_quasi: solve(st5, b, k) returns (de, record of the linear solve) for the five grids the pass wrote;
    norm(b) is ||b||_2.  Returns a dict: u (the last accepted iterate), hist, lam (step lengths), lin (the records),
    backtracks (rejected trials), converged, failed (the line search gave up), iterates, ops (the operator of every linear
    solve)"""
    un = np.array(u0, copy=True)
    _, b, nxt, _ = quasi_pass(a_nodes, k, f, un, method=method)
    hist, lams, lin, iterates, ops = [norm(b)], [], [], [un], []
    backtracks, failed = 0, False
    for it in range(max_iters):
        if hist[it] <= tol * hist[0]:
            break
        op = nxt
        ops.append(op)
        de, rec = solve(op, b, it)
        lin.append(rec)
        lam, j = 1.0, 0
        while True:
            ut, b, nxt, _ = quasi_pass(a_nodes, k, f, un, de, lam, method=method)
            r = norm(b)
            if armijo(r, lam, hist[it]):
                break
            backtracks += 1
            j += 1
            if j > max_backtracks:
                failed = True
                break
            lam = lam / 2
        if failed:
            break
        un = ut
        iterates.append(un)
        hist.append(r)
        lams.append(lam)
    return dict(u=un, hist=np.array(hist), lam=np.array(lams), lin=lin, backtracks=backtracks,
                converged=bool(hist[-1] <= tol * hist[0]), failed=failed, iterates=iterates, ops=ops)


def dense_solve(st5, b, it=None):
    """a dense float64 solve with the five-point operator (symmetric or not), rounded to b's dtype"""
    n = b.shape[0]
    M = gr.dense(gr.nine([np.asarray(x, dtype=np.float64) for x in st5]))
    return np.linalg.solve(M, np.asarray(b, dtype=np.float64).ravel()).reshape(n, n).astype(b.dtype), None
