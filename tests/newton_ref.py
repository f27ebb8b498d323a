"""numpy statement of mgx_newton (include/mgx.h, csrc/mgx_newton.hpp) on top of tests/galerkin_ref.py and
tests/theta_ref.py: the fused pass operation by operation, the Armijo test, and the Newton loop around any linear solve
and any norm.  numpy rounds every elementwise operation on its own, which is what the kernel does, so the pass is meant
bit for bit in the operator's dtype.

The problem: F(u) = A0 u + kap phi(u) - f with phi(u) = p1 u + p2 u^2 + p3 u^3 on the interior n x n grid, A0 a list of
nine arrays in the storage order c, n, s, w, e, nw, ne, sw, se (a five-point one: gr.nine(st5)), kap in stencil units."""
import numpy as np

import galerkin_ref as gr
import theta_ref as tr


def poly(p, dtype):
    """(p1, p2, p3, q2, q3) in the working type: the three doubles rounded once, q2 = 2 p2 and q3 = 3 p3 formed in double
    and rounded once"""
    dt = np.dtype(dtype).type
    p1, p2, p3 = (float(x) for x in p)
    return dt(p1), dt(p2), dt(p3), dt(2.0 * p2), dt(3.0 * p3)


def newton_pass(A0, kap, f, p, u, de=None, lam=None):
    """the pass: v = u (de is None) or u + lam * de;  q = A0 v;  ph = ((p3 v + p2) v + p1) v;  dp = (q3 v + q2) v + p1;
    b = f - (q + kap ph);  d = kap dp.  Returns (v, b, d), all in u's dtype"""
    dt = u.dtype
    p1, p2, p3, q2, q3 = poly(p, dt)
    kap, f = np.asarray(kap, dtype=dt), np.asarray(f, dtype=dt)
    v = u if de is None else u + dt.type(lam) * np.asarray(de, dtype=dt)
    q = tr.apply(A0, v)
    ph = ((p3 * v + p2) * v + p1) * v
    dp = (q3 * v + q2) * v + p1
    b = f - (q + kap * ph)
    d = kap * dp
    return v, b, d


def armijo(r, lam, rk):
    """the acceptance test of a trial, in double on the host; a NaN rejects"""
    return bool(float(r) <= (1.0 - 1e-4 * float(lam)) * float(rk))


def norm2(b):
    """||b||_2 in double (the device sums the squares in its own order: the GPU tests pass mgx_residual_norm instead)"""
    return float(np.linalg.norm(np.asarray(b, dtype=np.float64)))


def newton(A0, kap, f, p, u0, solve, tol, max_newton, max_backtracks, norm=norm2):
    """the loop of mgx_newton: solve(S9, b, d, k) returns (de, record of the linear solve) for the Jacobian S9 = A0 +
    diag(d); norm(b) is ||b||_2.  Returns a dict: u (the last accepted iterate), hist, lam (step lengths), lin (the
    records), backtracks (rejected trials), converged, failed (the line search gave up), iterates, ds (the d of every
    linear solve)"""
    un = np.array(u0, copy=True)
    _, b, dn = newton_pass(A0, kap, f, p, un)
    hist, lams, lin, iterates, ds = [norm(b)], [], [], [un], []
    backtracks, failed = 0, False
    for k in range(max_newton):
        if hist[k] <= tol * hist[0]:
            break
        d = dn
        ds.append(d)
        de, rec = solve(tr.shift(A0, d), b, d, k)
        lin.append(rec)
        lam, j = 1.0, 0
        while True:
            ut, b, dn = newton_pass(A0, kap, f, p, un, de, lam)
            r = norm(b)
            if armijo(r, lam, hist[k]):
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
                converged=bool(hist[-1] <= tol * hist[0]), failed=failed, iterates=iterates, ds=ds)


def sparse(st9):
    """the operator as a scipy CSR matrix in float64, unknowns row-major (scipy imported late: only the CPU tests need it)"""
    import scipy.sparse as sp
    n = st9[0].shape[0]
    idx = np.arange(n * n).reshape(n, n)
    rows, cols, vals = [], [], []
    for (dy, dx), o in gr.SLOT.items():
        a = np.asarray(st9[o], dtype=np.float64)
        ys, xs = slice(max(0, -dy), n - max(0, dy)), slice(max(0, -dx), n - max(0, dx))
        rows.append(idx[ys, xs].ravel())
        cols.append((idx[ys, xs] + dy * n + dx).ravel())
        vals.append(a[ys, xs].ravel())
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n * n, n * n))


def direct_solve(S9, b, d=None, k=None):
    """a direct float64 solve of the Jacobian (sparse LU), rounded to b's dtype"""
    import scipy.sparse.linalg as spl
    n = b.shape[0]
    x = spl.spsolve(sparse(S9).tocsc(), np.asarray(b, dtype=np.float64).ravel()).reshape(n, n)
    return x.astype(b.dtype), None


def smallest_eigenvalue(S9):
    """the smallest eigenvalue of a symmetric operator (shift-invert Lanczos about 0)"""
    import scipy.sparse.linalg as spl
    return float(spl.eigsh(sparse(S9).tocsc(), k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])


def poisson_lambda_min(L):
    """the smallest eigenvalue 4 - 4 cos(pi / N) of the Poisson stencil on level L"""
    return 4.0 - 4.0 * np.cos(np.pi / (1 << L))


def backtracking_input(L, dtype=np.float64):
    """(A0, kap, f, p, u0) of the input whose first full Newton step overshoots: A0 = Poisson, kap = 64 / N^2, phi = u^2,
    f = 32 / N^2, u0 = -0.9 lambda_min / (2 kap) - the first Jacobian A0 + 2 kap u0 is SPD with smallest eigenvalue
    0.1 lambda_min"""
    N = 1 << L
    n = N - 1
    kap = 64.0 / N ** 2
    full = lambda v: np.full((n, n), v, dtype=dtype)
    return tr.poisson9(L, dtype), full(kap), full(32.0 / N ** 2), (0.0, 1.0, 0.0), full(-0.9 * poisson_lambda_min(L) / (2.0 * kap))
