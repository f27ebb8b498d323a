"""numpy statement of mgx_eigs (include/mgx.h, csrc/mgx_eig.hpp): LOBPCG with soft locking around one multigrid cycle from
zero.  Not a bitwise reference: the sums run in numpy's order and the small dense problem goes through numpy.linalg.

    X <- guesses;  AX = A X;  (theta, C) = RR([X], [AX]);  X <- X C;  AX <- A X;  P = none
    for k = 0 .. :
        R_j = AX_j - theta_j X_j;  hist_j[k] = ||R_j||                  (all columns, every iteration)
        act = { j : not hist_j[k] <= tol theta_j };  stop if act is empty or k = max_iters
        W_act = M R_act                                                  (one cycle from zero per active column)
        AW = A W
        S = [X, W_act, P], AS = [AX, AW, AP]       (P absent in iteration 0 and after a restart)
        (theta, C) = RR(S, AS)
        P <- S C with the X rows of C zeroed;  X <- S C;  AX <- A X and AP <- A P (both applied afresh)

RR(S, AS): G = S^T S, H = S^T AS, both symmetrised and scaled by 1 / sqrt(diag G); G = L L^T (a pivot that is not
positive and finite or below 64 eps: deficient -> the step is repeated once without P, then the call ends); the standard
problem L^-1 H L^-T; the nev smallest pairs; C = D L^-T Y.

A locked column (residual <= tol theta) gets no cycle and no column of W but stays in X, is rotated by every RR step and
re-enters `act` if its residual rises again.

The preconditioners are the numpy cycles of the suite (nine_ref, opdep_ref, wcycle_ref over line_ref.NumpyOps)."""
import numpy as np

import galerkin_ref as gr
import line_ref as lr
import nine_ref as nr
import wcycle_ref as wr

EPS = np.finfo(np.float64).eps
PIVOT_MIN = 64 * EPS


# ---- operators -----------------------------------------------------------------------------------------------------
def constant_stencil(L, eps, dtype=np.float64):
    """(c, n, s, w, e) of the constant stencil c = 2 (1 + eps), w = e = -1, n = s = -eps on level L"""
    n = (1 << L) - 1
    full = lambda v: np.full((n, n), v, dtype=dtype)
    return [full(2.0 * (1.0 + eps)), full(-eps), full(-eps), full(-1.0), full(-1.0)]


def constant_eigenvalues(L, eps, count):
    """the `count` smallest of 2 (1 - cos p pi / N) + 2 eps (1 - cos q pi / N), p, q = 1 .. N - 1, ascending"""
    N = 1 << L
    t = 2.0 * (1.0 - np.cos(np.arange(1, N) * np.pi / N))
    return np.sort((t[None, :] + eps * t[:, None]).ravel())[:count]


def coefficient_stencil(a_nodes, dtype=np.float64):
    """the nine arrays (corners zero) of what mgx_set_coefficient builds from nodal values"""
    return nr.tensor9(a_nodes, np.zeros_like(a_nodes), a_nodes, dtype)


def apply(st9, v):
    """A v, v of shape (n, n), in float64"""
    st = [np.asarray(a, dtype=np.float64) for a in st9]
    return gr._apply9(st, st[0], np.asarray(v, dtype=np.float64))


def lambda_max_bound(st9):
    """the Gershgorin bound of the spectrum, the scale of the rounding of a row sum"""
    return float(np.max(sum(np.abs(np.asarray(a, dtype=np.float64)) for a in st9)))


class Stencil5Numpy(wr.CycleIndex, gr.Hierarchy):
    """op = STENCIL5 in numpy: every level the caller's five-point operator, Jacobi smoothing, bilinear transfers"""

    def __init__(self, stencils, finest, coarsest, dtype=np.float64, mode=gr.CONSISTENT, omega=2.0 / 3.0, mu1=2, mu2=2):
        self.po, self.L, self.Lc, self.dt, self.mode, self.omega, self.mu1, self.mu2 = lr.NumpyOps, finest, coarsest, dtype, mode, omega, mu1, mu2
        self.mu0, self.bottom_mode = 0, gr.EXACT
        self.st = {lv: gr.nine([np.asarray(x, dtype=dtype) for x in stencils[lv]]) for lv in range(coarsest, finest + 1)}
        self.jac = {lv: gr.build_jacobi9(self.st[lv], omega) for lv in self.st}
        self._inv = None

    def smooth(self, lv, v, b, mu):
        return v if mu == 0 else gr.jacobi9(v, b, mu, self.omega, self.jac[lv])

    def residual(self, lv, v, b):
        return gr.residual9(v, b, self.st[lv])


def hierarchy(op, st, L, Lc, transfer=0, cycle=wr.V):
    """the float64 numpy hierarchy of a handle: op 's5' (st: (c, n, s, w, e) of the finest level, the same constant stencil on
    every level: pass a function level -> stencil) or 'gal' (st: nine arrays of the finest level), V(2,2) Jacobi"""
    if op == "s5":
        h = Stencil5Numpy({lv: st(lv) for lv in range(Lc, L + 1)}, L, Lc)
    elif transfer:
        h = nr.OpdepHierarchy(lr.NumpyOps, st, L, Lc)
    else:
        h = nr.Hierarchy(lr.NumpyOps, st, L, Lc)
    h.cycle = cycle
    return h


def preconditioner(h):
    def M(r):
        return h.vcycle(h.L, np.zeros_like(r), r)
    return M


# ---- the Rayleigh-Ritz step ----------------------------------------------------------------------------------------
def rayleigh_ritz(S, AS, nev):
    """(theta, C) of the nev smallest Ritz pairs of span S (columns), or None if the scaled Gram matrix is deficient"""
    return rayleigh_ritz_dense(S.T @ S, S.T @ AS, nev)


def rayleigh_ritz_dense(G, H, nev):
    """the host part: the nev smallest pairs of H y = theta G y and C with C^T G C = I, or None (deficient)"""
    G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)
    dg = np.diag(G)
    if not np.all(np.isfinite(dg) & (dg > 0)):
        return None
    d = 1.0 / np.sqrt(dg)
    G, H = d[:, None] * G * d[None, :], d[:, None] * H * d[None, :]
    np.fill_diagonal(G, 1.0)
    if not np.all(np.isfinite(G)):
        return None
    try:
        Lc = np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        return None
    piv = np.diag(Lc) ** 2
    if not np.all(np.isfinite(piv) & (piv >= PIVOT_MIN)):
        return None
    M = np.linalg.solve(Lc, H)
    M = np.linalg.solve(Lc, M.T).T
    if not np.all(np.isfinite(M)):
        return np.full(nev, np.nan), np.zeros((G.shape[0], nev))
    w, Y = np.linalg.eigh(0.5 * (M + M.T))
    return w[:nev], d[:, None] * np.linalg.solve(Lc.T, Y[:, :nev])


class Result:
    """theta (nev), X (nev, n, n), hist (list of arrays), cycles (list), iterations (RR steps after the first), converged
    (list of bool), reason ('' or why the call ended early)"""


def lobpcg(A, M, X0, tol=1e-8, max_iters=100, ap_afresh=True):
    """A: (n, n) -> (n, n);  M: residual (n, n) -> one cycle from zero;  X0: (nev, n, n).  ap_afresh = False keeps AP by the
    recurrence AP <- AS C instead: the variant that is not stable (tests/test_eig_cpu.py shows a case)"""
    X0 = np.asarray(X0, dtype=np.float64)
    nev, n = X0.shape[0], X0.shape[1]
    col = lambda V: V.reshape(V.shape[0], -1).T.copy()                 # (k, n, n) -> (n^2, k)
    Aop = lambda S: np.stack([A(S[:, j].reshape(n, n)).ravel() for j in range(S.shape[1])], axis=1)
    out = Result()
    out.reason, out.iterations = "", 0
    X = col(X0)
    first = rayleigh_ritz(X, Aop(X), nev)
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
        AW = Aop(W)
        S, AS = [X, W] + ([P] if P is not None else []), [AX, AW] + ([AP] if P is not None else [])
        step = rayleigh_ritz(np.hstack(S), np.hstack(AS), nev)
        if step is None and P is not None:
            S, AS = S[:2], AS[:2]
            step = rayleigh_ritz(np.hstack(S), np.hstack(AS), nev)
        if step is None:
            out.reason = "the basis is rank deficient with and without P"
            break
        th, C = step
        if not np.all(np.isfinite(th) & (th > 0)):
            out.reason, failed = "a Ritz value is not a positive finite number", True
            break
        S, AS = np.hstack(S), np.hstack(AS)
        P = S[:, nev:] @ C[nev:]
        AP = Aop(P) if ap_afresh else AS[:, nev:] @ C[nev:]
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


def guesses(L, nev, seed=0):
    """the binding's default guesses: uniform(-1, 1) from default_rng(seed)"""
    n = (1 << L) - 1
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (nev, n, n))


def orthonormality_defect(X):
    """max |X^T X - I| of (nev, n, n) vectors, in float64"""
    V = np.asarray(X, dtype=np.float64).reshape(X.shape[0], -1)
    return float(np.max(np.abs(V @ V.T - np.eye(V.shape[0]))))
