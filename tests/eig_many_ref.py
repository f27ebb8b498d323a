"""numpy statement of mgx_eigs_many (include/mgx.h, csrc/mgx_eig_many.hpp): eig_ref's LOBPCG on blocks of at most four
columns, each block constrained to the complement of the pairs locked before it.  Not a bitwise reference.

    Y = {}                                  (locked vectors, orthonormal)
    while |Y| < nev:
        kb = min(4, nev - |Y|);  X = the guesses |Y| .. |Y| + kb - 1
        X <- X - Y (Y^T X), twice           (once per block; skipped when Y is empty)
        eig_ref's iteration on X, with one change: after W_act = M R_act,
            W_act <- W_act - Y (Y^T W_act)  (once per iteration; skipped when Y is empty)
        the block ends as eig_ref.lobpcg ends
        if it did not end converged: stop.   else Y <- [Y, X]
    sort the computed pairs by lambda ascending (stable); vectors, histories and cycle counts follow

The projection is classical Gram-Schmidt: all coefficients from the unmodified W, then the subtraction with i ascending.

block_lobpcg is eig_ref.lobpcg (ap_afresh) with the two projections; without locked vectors it executes the same numpy
operations in the same order and returns the same bits (tests/test_eig_many_cpu.py holds it to that)."""
import numpy as np

import eig_ref as er

BLOCK = 4
EIGS_MAX = 16


def partition(nev):
    """the block sizes: fours, the last one the rest"""
    return [min(BLOCK, nev - d) for d in range(0, nev, BLOCK)]


def project(V, Y):
    """V - Y (Y^T V): the coefficients from the unmodified V, the subtraction over the locked vectors ascending"""
    if Y is None:
        return V
    c = Y.T @ V
    V = V.copy()
    for i in range(Y.shape[1]):
        V -= Y[:, i:i + 1] * c[i][None, :]
    return V


def block_lobpcg(A, M, X0, Y=None, tol=1e-8, max_iters=100):
    """eig_ref.lobpcg on the block X0 (k, n, n) in the complement of the columns of Y ((n^2, m) or None)"""
    X0 = np.asarray(X0, dtype=np.float64)
    nev, n = X0.shape[0], X0.shape[1]
    col = lambda V: V.reshape(V.shape[0], -1).T.copy()
    Aop = lambda S: np.stack([A(S[:, j].reshape(n, n)).ravel() for j in range(S.shape[1])], axis=1)
    out = er.Result()
    out.reason, out.iterations = "", 0
    X = col(X0)
    X = project(project(X, Y), Y)
    first = er.rayleigh_ritz(X, Aop(X), nev)
    if first is None:
        raise ValueError("the guesses are linearly dependent")
    theta, C = first
    X = X @ C
    AX = Aop(X)
    failed = not np.all(np.isfinite(theta) & (theta > 0))
    if failed:
        out.reason = "a Ritz value of the guesses is not a positive finite number"
    P = AP = None
    hist = [[] for _ in range(nev)]
    cycles = [0] * nev
    k = 0
    while True:
        R = AX - X * theta[None, :]
        r = np.sqrt(np.sum(R * R, axis=0))
        for j in range(nev):
            hist[j].append(float(r[j]))
        if failed:
            break
        act = [j for j in range(nev) if not r[j] <= tol * theta[j]]
        if not act or k == max_iters:
            break
        W = np.stack([M(R[:, j].reshape(n, n)).ravel() for j in act], axis=1)
        for j in act:
            cycles[j] += 1
        W = project(W, Y)
        AW = Aop(W)
        S, AS = [X, W] + ([P] if P is not None else []), [AX, AW] + ([AP] if P is not None else [])
        step = er.rayleigh_ritz(np.hstack(S), np.hstack(AS), nev)
        if step is None and P is not None:
            S, AS = S[:2], AS[:2]
            step = er.rayleigh_ritz(np.hstack(S), np.hstack(AS), nev)
        if step is None:
            out.reason = "the basis is rank deficient with and without P"
            break
        th, C = step
        if not np.all(np.isfinite(th) & (th > 0)):
            out.reason, failed = "a Ritz value is not a positive finite number", True
            break
        S, AS = np.hstack(S), np.hstack(AS)
        P = S[:, nev:] @ C[nev:]
        AP = Aop(P)
        X = S @ C
        AX = Aop(X)
        theta = th
        k += 1
    out.iterations = k
    out.theta, out.X = theta, X.T.reshape(nev, n, n).copy()
    out.hist = [np.array(h) for h in hist]
    out.cycles = cycles
    out.converged = [(not failed) and bool(hist[j][-1] <= tol * theta[j]) for j in range(nev)]
    return out


def stable_order(lam):
    """the ranks of mgx_eig_many_plan.hpp's insertion sort: ascending, equal values in the order computed"""
    return [int(i) for i in np.argsort(np.asarray(lam), kind="stable")]


def eigs_many(A, M, X0, tol=1e-8, max_iters=100):
    """X0: (nev, n, n), nev <= 16.  Returns a Result over the `computed` pairs in ascending order (theta, X, hist, cycles,
    converged), with block_iterations (one count per block run), computed, and reason ('' or why the call stopped)"""
    X0 = np.asarray(X0, dtype=np.float64)
    nev, n = X0.shape[0], X0.shape[1]
    assert 1 <= nev <= EIGS_MAX
    Y, done = None, 0
    theta, X, hist, cycles, conv, its, reason = [], [], [], [], [], [], ""
    for b, kb in enumerate(partition(nev)):
        res = block_lobpcg(A, M, X0[done:done + kb], Y, tol, max_iters)
        its.append(res.iterations)
        theta += list(res.theta)
        X += list(res.X)
        hist += res.hist
        cycles += res.cycles
        conv += res.converged
        done += kb
        if not all(res.converged):
            reason = f"block {b}: " + (res.reason or f"did not converge within max_iters = {max_iters} iterations")
            break
        new = res.X.reshape(kb, -1).T
        Y = new if Y is None else np.hstack([Y, new])
    order = stable_order(theta)
    out = er.Result()
    out.theta = np.array([theta[i] for i in order])
    out.X = np.stack([X[i] for i in order])
    out.hist = [hist[i] for i in order]
    out.cycles = [cycles[i] for i in order]
    out.converged = [conv[i] for i in order]
    out.block_iterations, out.iterations, out.computed, out.reason = its, max(its), done, reason
    return out
