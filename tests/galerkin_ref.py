"""numpy statement of the Galerkin hierarchy (op = MGX_OPERATOR_GALERKIN, csrc/mgx_galerkin.hpp): the coarse operator
A_c = R A_f P term by term in the kernel's documented order, the nine-point Jacobi sweep and residual in the kernels'
summation order, the dense coarsest solve in the device's elimination order, and the V-cycle / FMG pass / solve built from them plus the oracle's transfer operators
and five-point finest-level kernels (oracle/pyoracle.py).  numpy's elementwise arithmetic rounds every operation
separately, which is what the kernels do (-ffp-contract=off), so every step is meant bit for bit.

An operator is a list of nine interior n x n arrays in the storage order c, n, s, w, e, nw, ne, sw, se."""
import numpy as np

SLOTS = ("c", "n", "s", "w", "e", "nw", "ne", "sw", "se")
# storage slot of the coefficient that points at (dy, dx)
SLOT = {(0, 0): 0, (-1, 0): 1, (1, 0): 2, (0, -1): 3, (0, 1): 4, (-1, -1): 5, (-1, 1): 6, (1, -1): 7, (1, 1): 8}
ROW_MAJOR = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]       # NW, N, NE, W, C, E, SW, S, SE
CONSISTENT, FW16 = 0, 1
EXACT, SMOOTH = 0, 1                   # cfg.bottom
V, FMG = 0, 1                          # cfg.schedule


def nine(st5):
    """a five-point operator (c, n, s, w, e) as a nine-point one with zero corners"""
    st5 = [np.ascontiguousarray(x) for x in st5]
    return st5 + [np.zeros_like(st5[0]) for _ in range(4)]


def _p1(o):
    return 1.0 - 0.5 * abs(o)


def rap(st9, N_f, mode=CONSISTENT):
    """A_c(I, I+D) = sum_i sum_d R(I, i) A_f(i, i+d) P(i+d, I+D) on the grid with N_f intervals per side (n_f = N_f - 1
    unknowns), R = P^T (CONSISTENT) or P^T / 4 (FW16).  Order: accumulator from +0; i row-major over the 3 x 3 patch
    around 2I; d row-major; structurally zero P(i+d, I+D) skipped; each term is w * A_f with the exact power of two
    w = r P(i, I) P(i+d, I+D).  Offsets that point at the Dirichlet ring get 0."""
    dt = st9[0].dtype
    nf = N_f - 1
    assert st9[0].shape == (nf, nf)
    nc = N_f // 2 - 1
    rscale = dt.type(0.25 if mode == FW16 else 1.0)
    out = [np.zeros((nc, nc), dtype=dt) for _ in range(9)]
    for iy in (-1, 0, 1):
        for ix in (-1, 0, 1):
            wr = _p1(iy) * _p1(ix)
            for dy, dx in ROW_MAJOR:
                # A_f(i, i + d) at i = 2I + (iy, ix), I = 1 .. N_c - 1 (interior index = grid index - 1)
                a = st9[SLOT[dy, dx]][1 + iy::2, 1 + ix::2][:nc, :nc]
                for Dy, Dx in ROW_MAJOR:
                    oy, ox = iy + dy - 2 * Dy, ix + dx - 2 * Dx
                    if abs(oy) > 1 or abs(ox) > 1:
                        continue
                    w = rscale * dt.type(wr * _p1(oy) * _p1(ox))
                    o = SLOT[Dy, Dx]
                    out[o] = out[o] + w * a
    for (Dy, Dx), o in SLOT.items():
        if Dy < 0:
            out[o][0, :] = 0
        if Dy > 0:
            out[o][-1, :] = 0
        if Dx < 0:
            out[o][:, 0] = 0
        if Dx > 0:
            out[o][:, -1] = 0
    return out


def build_jacobi9(st9, omega):
    """(D_inv, [R_n, R_s, R_w, R_e, R_nw, R_ne, R_sw, R_se]): D_inv = 1 / c, R_x = -(omega (D_inv a_x))"""
    dt = st9[0].dtype
    om = dt.type(omega)
    d = dt.type(1) / st9[0]
    return d, [-(om * (d * a)) for a in st9[1:]]


def _apply9(coefs, centre, v):
    """sum in CSR column order NW, N, NE, W, C, E, SW, S, SE; coefs: slot -> array (slots 1..8), centre: array or scalar"""
    P = np.pad(v, 1)
    n = v.shape[0]
    acc = None
    for dy, dx in ROW_MAJOR:
        nb = P[1 + dy:1 + dy + n, 1 + dx:1 + dx + n]
        term = (centre if (dy, dx) == (0, 0) else coefs[SLOT[dy, dx]]) * nb
        acc = term if acc is None else acc + term
    return acc


def jacobi9(v, b, mu, omega, jac):
    """mu sweeps of v <- R_omega v + omega (D_inv b); jac = build_jacobi9(...)"""
    dt = v.dtype
    dinv, r = jac
    coefs = [None] + list(r)
    om = dt.type(omega)
    rc = dt.type(1.0 - float(om))
    for _ in range(mu):
        v = _apply9(coefs, rc, v) + om * (dinv * b)
    return v


def residual9(v, b, st9):
    return b - _apply9(st9, st9[0], v)


def dense(st9):
    """the operator as a dense (n^2 x n^2) float64 matrix, unknowns row-major"""
    n = st9[0].shape[0]
    M = np.zeros((n * n, n * n))
    idx = np.arange(n * n).reshape(n, n)
    for (dy, dx), o in SLOT.items():
        a = np.asarray(st9[o], dtype=np.float64)
        ys = slice(max(0, -dy), n - max(0, dy))
        xs = slice(max(0, -dx), n - max(0, dx))
        rows = idx[ys, xs].ravel()
        cols = (idx[ys, xs] + dy * n + dx).ravel()
        M[rows, cols] = a[ys, xs].ravel()
    return M


def gauss_jordan_inverse(M):
    """dense inverse by Gauss-Jordan elimination without pivoting, every element update its own IEEE operations in the
    order of the device's k_gj_prow / k_gj_elim (and of the oracle's orc_dense_inverse)"""
    M = np.array(M, dtype=np.float64)
    NN = M.shape[0]
    Inv = np.eye(NN)
    for k in range(NN):
        p = M[k, k]
        pm, pi = M[k] / p, Inv[k] / p
        f = M[:, k].copy()
        M -= np.outer(f, pm)
        Inv -= np.outer(f, pi)
        M[k], Inv[k] = pm, pi
    return Inv


def dense_apply(Inv, b):
    """x = Inv b as k_var_dense_solve sums it: one in-order sum per unknown, in double"""
    bb = np.asarray(b, dtype=np.float64).ravel()
    acc = np.zeros(Inv.shape[0])
    for q in range(Inv.shape[1]):
        acc = acc + Inv[:, q] * bb[q]
    return acc


class Hierarchy:
    """finest level: the five-point operator `st5` (oracle kernels); levels below: rap().

    bottom = SMOOTH (vcycle() of mgx.hip at the coarsest level, the oracle's orc_vcycle): no dense solve; the coarsest
    level runs mu1 sweeps and then mu2 sweeps, mu1 + mu2 in all, of its own smoother, starting from the guess it is
    handed: zero inside a V-cycle (the restriction zeroes the coarse guess, PS:613) and in fmg() (PS:630)."""

    def __init__(self, po, st5, finest, coarsest, dtype=np.float64, mode=CONSISTENT, omega=2.0 / 3.0, mu1=2, mu2=2, mu0=0, bottom=EXACT):
        self.po, self.L, self.Lc, self.dt, self.mode, self.omega, self.mu1, self.mu2 = po, finest, coarsest, dtype, mode, omega, mu1, mu2
        self.mu0, self.bottom_mode = mu0, bottom
        self.st = {finest: nine([np.asarray(x, dtype=dtype) for x in st5])}
        for lv in range(finest, coarsest, -1):
            self.st[lv - 1] = rap(self.st[lv], 1 << lv, mode)
        self.jac = {lv: build_jacobi9(self.st[lv], omega) for lv in self.st}
        self.jac5 = po.var_build_jacobi(*self.st[finest][:5], omega=omega)
        self._inv = None                       # dense inverse of the coarsest operator, built on first use

    def smooth(self, lv, v, b, mu):
        if mu == 0:
            return v
        if lv == self.L:
            return self.po.var_jacobi(v, b, mu, self.omega, self.jac5)
        return jacobi9(v, b, mu, self.omega, self.jac[lv])

    def residual(self, lv, v, b):
        if lv == self.L:
            return self.po.var_residual(v, b, self.st[lv][:5])
        return residual9(v, b, self.st[lv])

    def bottom(self, b):
        if self._inv is None:
            self._inv = gauss_jordan_inverse(dense(self.st[self.Lc]))
        return dense_apply(self._inv, b).reshape(b.shape).astype(self.dt)

    def vcycle(self, lv, v, b):
        if lv == self.Lc:
            if self.bottom_mode == EXACT:
                return self.bottom(b)
            return self.smooth(lv, self.smooth(lv, v, b, self.mu1), b, self.mu2)
        v = self.smooth(lv, v, b, self.mu1)
        rc = self.po.restrict(self.residual(lv, v, b), self.mode)
        e = self.vcycle(lv - 1, np.zeros_like(rc), rc)
        v = self.po.prolong_add(v, e)
        return self.smooth(lv, v, b, self.mu2)

    def fmg(self, b):
        """fmg() of mgx.hip / the oracle's orc_fmg: b restricted with the handle's mode down to the coarsest level
        (PS:641); there the dense solve (EXACT) or mu0 + 1 coarsest "V-cycles" from zero (SMOOTH, PS:630-635); then per
        level up to the finest: prolong (PS:645, not added: the level's previous iterate is discarded) and mu0 + 1
        V-cycles with that level's restricted right-hand side (PS:646-648)"""
        rhs = {self.L: np.ascontiguousarray(b, dtype=self.dt)}
        for lv in range(self.L, self.Lc, -1):
            rhs[lv - 1] = self.po.restrict(rhs[lv], self.mode)
        if self.bottom_mode == EXACT:
            v = self.bottom(rhs[self.Lc])
        else:
            v = np.zeros_like(rhs[self.Lc])
            for _ in range(self.mu0 + 1):
                v = self.vcycle(self.Lc, v, rhs[self.Lc])
        for lv in range(self.Lc + 1, self.L + 1):
            v = self.po.prolong(v)
            for _ in range(self.mu0 + 1):
                v = self.vcycle(lv, v, rhs[lv])
        return v

    def solve(self, b, u0=None, tol=1e-8, max_cycles=50, schedule=V):
        """(u, history of ||b - A u||) as the oracle's and the device's solve report it.  schedule = FMG: the first
        cycle is fmg(b), which discards the guess (the history still starts at the guess's residual); V-cycles after"""
        b = np.ascontiguousarray(b, dtype=self.dt)
        u = np.zeros_like(b) if u0 is None else np.array(u0, dtype=self.dt, order="C")
        hist = [self.po.norm2(self.residual(self.L, u, b))]
        for k in range(max_cycles):
            if hist[-1] <= tol * hist[0]:
                break
            u = self.fmg(b) if (k == 0 and schedule == FMG) else self.vcycle(self.L, u, b)
            hist.append(self.po.norm2(self.residual(self.L, u, b)))
        return u, np.array(hist)
