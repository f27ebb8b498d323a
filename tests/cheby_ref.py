"""numpy statement of the Chebyshev smoother (cfg.smoother = MGX_SMOOTHER_CHEBYSHEV, csrc/mgx_cheby.hpp) on top of the
hierarchies of tests/galerkin_ref.py and tests/opdep_ref.py: the bound g_l, the scalars of a block, the block itself,
and hierarchies whose smooth() is the block.  numpy rounds every elementwise operation separately, which is what the
kernels do (-ffp-contract=off), and Python's float arithmetic is the host's double arithmetic, so every step is meant
bit for bit.

    J(v) = one sweep of the level's Jacobi smoother (R_omega v + omega (D_inv b)),   z = J(v) - v
    lmax = omega g,  lmin = lmax / 4,  theta = (lmax + lmin) / 2,  delta = (lmax - lmin) / 2,  sigma = theta / delta
    step 0:       d = c_0 z                c_0 = 1 / theta,                      rho_0 = 1 / sigma
    step k >= 1:  d = (a_k d) + (c_k z)    rho_k = 1 / (2 sigma - rho_{k-1}),  a_k = rho_k rho_{k-1},  c_k = (2 rho_k) / delta
    every step:   v = v + d
with a_k, c_k formed in double and rounded to the working type once."""
import numpy as np

import galerkin_ref as gr
import opdep_ref as od


def lambda_bound(st9, nine=True):
    """g = max over the interior points of 1 + sum_x |D_inv a_x|: x = n, s, w, e (and nw, ne, sw, se when `nine`), D_inv
    = 1 / c in the operator's type, every product and the sum in double, in that order from 1.0; coefficients that point
    at the Dirichlet ring are not counted"""
    dt = st9[0].dtype
    dinv = (dt.type(1) / st9[0]).astype(np.float64)
    n = dinv.shape[0]
    acc = np.ones((n, n))
    for q in range(1, 9 if nine else 5):
        dy, dx = next(k for k, v in gr.SLOT.items() if v == q)
        term = np.abs(dinv * st9[q].astype(np.float64))
        if dy < 0:
            term[0, :] = 0
        if dy > 0:
            term[-1, :] = 0
        if dx < 0:
            term[:, 0] = 0
        if dx > 0:
            term[:, -1] = 0
        acc = acc + term
    return float(acc.max())


def scalars(omega, g, mu):
    """[(a_k, c_k)] of a block of degree mu, Python floats (double)"""
    lmax = omega * g
    lmin = lmax / 4.0
    theta, delta = (lmax + lmin) / 2.0, (lmax - lmin) / 2.0
    sigma = theta / delta
    out, rho = [], 1.0 / sigma
    for k in range(mu):
        if k == 0:
            out.append((0.0, 1.0 / theta))
            continue
        rho_k = 1.0 / (2.0 * sigma - rho)
        out.append((rho_k * rho, (2.0 * rho_k) / delta))
        rho = rho_k
    return out


def block(sweep, v, b, mu, omega, g):
    """a block of degree mu; sweep(v, b): one Jacobi sweep of the level"""
    dt = v.dtype
    d = None
    for k, (a, c) in enumerate(scalars(omega, g, mu)):
        z = sweep(v, b) - v
        if k == 0:
            d = dt.type(c) * z
        else:
            d = (dt.type(a) * d) + (dt.type(c) * z)
        v = v + d
    return v


def cheb_T(k, x):
    """the Chebyshev polynomial T_k(x), x >= 1"""
    return float(np.cosh(k * np.arccosh(x)))


class _Cheby:
    """smooth() of a hierarchy as the Chebyshev block; self.g[lv]: the bound of every level.  A hierarchy's own
    omega only scales z and the interval together (the iterates do not depend on it beyond rounding)"""

    def _bounds(self):
        self.g = {lv: lambda_bound(self.st[lv], nine=(lv != self.L)) for lv in self.st}

    def jacobi_sweep(self, lv, v, b):
        return super().smooth(lv, v, b, 1)

    def smooth(self, lv, v, b, mu):
        if mu == 0:
            return v
        return block(lambda x, f: self.jacobi_sweep(lv, x, f), v, b, mu, self.omega, self.g[lv])


class Hierarchy(_Cheby, gr.Hierarchy):
    """GALERKIN, bilinear transfers"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._bounds()


class OpdepHierarchy(_Cheby, od.Hierarchy):
    """GALERKIN, operator-dependent transfers"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._bounds()


class Stencil5(gr.Hierarchy):
    """op = STENCIL5: every level a five-point operator of the caller's (stencils: level -> (c, n, s, w, e)), the oracle's
    transfer operators, the dense coarsest solve; Jacobi smoothing (Stencil5Cheby: the Chebyshev block)"""

    def __init__(self, po, stencils, finest, coarsest, dtype=np.float64, mode=gr.CONSISTENT, omega=2.0 / 3.0, mu1=2, mu2=2, mu0=0, bottom=gr.EXACT):
        self.po, self.L, self.Lc, self.dt, self.mode, self.omega, self.mu1, self.mu2 = po, finest, coarsest, dtype, mode, omega, mu1, mu2
        self.mu0, self.bottom_mode = mu0, bottom
        self.st = {lv: gr.nine([np.asarray(x, dtype=dtype) for x in stencils[lv]]) for lv in range(coarsest, finest + 1)}
        self.jac5 = {lv: po.var_build_jacobi(*self.st[lv][:5], omega=omega) for lv in self.st}
        self._inv = None

    def smooth(self, lv, v, b, mu):
        if mu == 0:
            return v
        return self.po.var_jacobi(v, b, mu, self.omega, self.jac5[lv])

    def residual(self, lv, v, b):
        return self.po.var_residual(v, b, self.st[lv][:5])


class Stencil5Cheby(_Cheby, Stencil5):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.g = {lv: lambda_bound(self.st[lv], nine=False) for lv in self.st}
