"""numpy statement of GALERKIN hierarchies whose FINEST operator is nine-point (mgx_set_stencil9, mgx_set_tensor):
the discretisation of the full-tensor diffusion problem (k_var_from_tensor) and the hierarchies of galerkin_ref,
opdep_ref, cheby_ref, line_ref and wcycle_ref with the nine-point routines (gr.jacobi9, gr.residual9, gr.rap,
od.weights, od.rap, the line sweeps with corners, the bound over eight off-diagonals) on EVERY level, the finest
included.  The transfers of the bilinear hierarchies stay the oracle's (po.restrict, po.prolong_add, po.prolong).

An operator is a list of nine interior n x n arrays in the storage order c, n, s, w, e, nw, ne, sw, se."""
import numpy as np

import cheby_ref as cr
import galerkin_ref as gr
import line_ref as lr
import opdep_ref as od
import wcycle_ref as wr


def tensor9(axx, axy, ayy, dtype=np.float64):
    """the nine-point operator of -d_x(axx d_x u) - d_y(ayy d_y u) - d_x(axy d_y u) - d_y(axy d_x u), without h^-2, from
    the nodal values on the (N + 1)^2 nodes of a grid (x along a row, y grows with the row index).  All arithmetic in
    double, each coefficient rounded to `dtype` once.  The five-point part is the oracle's stencil_from_nodes with ayy on
    the n / s faces and axx on the w / e faces; a corner is a quarter of the sum of axy at the two edge neighbours it
    lies between, negative towards nw and se"""
    axx, axy, ayy = (np.asarray(a, dtype=np.float64) for a in (axx, axy, ayy))
    assert axx.shape == axy.shape == ayy.shape and axx.shape[0] == axx.shape[1]
    I = slice(1, -1)
    up, dn = slice(0, -2), slice(2, None)              # r - 1 / r + 1 (or c - 1 / c + 1)
    fn = 0.5 * (ayy[I, I] + ayy[up, I])
    fs = 0.5 * (ayy[I, I] + ayy[dn, I])
    fw = 0.5 * (axx[I, I] + axx[I, up])
    fe = 0.5 * (axx[I, I] + axx[I, dn])
    aN, aS, aW, aE = axy[up, I], axy[dn, I], axy[I, up], axy[I, dn]
    out = [((fn + fw) + fe) + fs, -fn, -fs, -fw, -fe,
           -(0.25 * (aW + aN)), 0.25 * (aE + aN), 0.25 * (aW + aS), -(0.25 * (aE + aS))]
    return [np.ascontiguousarray(x.astype(dtype)) for x in out]


def grid_nodes(level):
    """(x, y) of the (N + 1)^2 nodes: x along a row, y down the rows"""
    t = np.linspace(0.0, 1.0, (1 << level) + 1)
    return t[None, :], t[:, None]


def rotated_tensor(level, theta_deg, eps):
    """nodal (axx, axy, ayy) of the constant rotated-anisotropy tensor: principal values 1 (along the direction at angle
    theta to the x axis) and eps"""
    th = np.deg2rad(theta_deg)
    c, s = np.cos(th), np.sin(th)
    shape = ((1 << level) + 1,) * 2
    return (np.full(shape, c * c + eps * s * s), np.full(shape, (1.0 - eps) * s * c), np.full(shape, s * s + eps * c * c))


def smooth_tensor(level):
    """a smooth, variable, uniformly elliptic tensor (axx ayy - axy^2 >= 0.5 * 1.0 - 0.16 > 0)"""
    x, y = grid_nodes(level)
    return (1.0 + 0.5 * np.sin(2 * np.pi * x) * np.cos(np.pi * y), 0.4 * np.sin(np.pi * (x + y)),
            1.5 + 0.5 * np.cos(2 * np.pi * y) + 0.0 * x)


def jump_tensor(level):
    """piecewise constant: another tensor (another principal direction) in the quadrant x, y > 1/2 and in a strip"""
    x, y = grid_nodes(level)
    q = ((x > 0.5) & (y > 0.5)) | ((x < 0.3) & (y > 0.2) & (y < 0.4))
    return (np.where(q, 10.0, 1.0) + 0.0 * y, np.where(q, 2.5, -0.3) + 0.0 * y, np.where(q, 3.0, 2.0) + 0.0 * y)


def zero_ring(st9):
    """the operator with zeros in the coefficients that point at the Dirichlet ring"""
    out = [np.array(a, copy=True) for a in st9]
    for (dy, dx), q in gr.SLOT.items():
        if dy < 0:
            out[q][0, :] = 0
        if dy > 0:
            out[q][-1, :] = 0
        if dx < 0:
            out[q][:, 0] = 0
        if dx > 0:
            out[q][:, -1] = 0
    return out


def random_stencil9(level, seed, dtype=np.float64):
    """a non-symmetric, strictly diagonally dominant nine-point operator with arbitrary finite values in the
    ring-pointing places too"""
    n = (1 << level) - 1
    rng = np.random.default_rng(seed)
    off = [-rng.uniform(0.2, 1.0, (n, n)) for _ in range(4)] + [rng.uniform(-0.3, 0.3, (n, n)) for _ in range(4)]
    c = sum(np.abs(o) for o in off) + rng.uniform(0.05, 0.5, (n, n))
    return [np.ascontiguousarray(x.astype(dtype)) for x in [c] + off]


def with_ring_values9(st9, seed, big=1e30):
    """the same operator with the coefficients that point at the Dirichlet ring overwritten by finite values of mixed
    sign and magnitudes from 1 to `big` (float32 holds 1e30): as test_galerkin_cpu.with_ring_values, for all eight
    off-diagonals (a corner points at the ring on a row AND on a column)"""
    rng = np.random.default_rng(seed)
    out = [np.array(a, copy=True) for a in st9]
    n = out[0].shape[0]

    def junk():
        return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(0.0, np.log10(big), n)
    for (dy, dx), q in gr.SLOT.items():
        if dy < 0:
            out[q][0, :] = junk()
        if dy > 0:
            out[q][-1, :] = junk()
        if dx < 0:
            out[q][:, 0] = junk()
        if dx > 0:
            out[q][:, -1] = junk()
    return out


class Operator9:
    """A of a nine-point finest level for pcg_ref.pcg / gcr_ref.gcr: u -> A u in the order of residual9"""

    def __init__(self, st9, dtype=np.float64):
        self.dtype = dtype
        self.st = [np.asarray(x, dtype=dtype) for x in st9]

    def __call__(self, u):
        return gr._apply9(self.st, self.st[0], u)


class _NineFinest:
    """a hierarchy of galerkin_ref / opdep_ref whose finest operator is the nine-point `st9`: the constructor's second
    argument is that operator (nine arrays) instead of (c, n, s, w, e); every level smooths with jacobi9 and forms
    residual9"""

    def __init__(self, po, st9, finest, coarsest, dtype=np.float64, mode=gr.CONSISTENT, omega=2.0 / 3.0, mu1=2, mu2=2, mu0=0, bottom=gr.EXACT):
        self.po, self.L, self.Lc, self.dt, self.mode, self.omega, self.mu1, self.mu2 = po, finest, coarsest, dtype, mode, omega, mu1, mu2
        self.mu0, self.bottom_mode = mu0, bottom
        assert len(st9) == 9
        self.st = {finest: [np.ascontiguousarray(x, dtype=dtype) for x in st9]}
        self.W = {}
        for lv in range(finest, coarsest, -1):
            if isinstance(self, od.Hierarchy):
                self.W[lv] = od.weights(self.st[lv], 1 << lv)
                self.st[lv - 1] = od.rap(self.st[lv], self.W[lv], 1 << lv, mode)
            else:
                self.st[lv - 1] = gr.rap(self.st[lv], 1 << lv, mode)
        self.jac = {lv: gr.build_jacobi9(self.st[lv], omega) for lv in self.st}
        self.jac5 = None
        self._inv = None

    def smooth(self, lv, v, b, mu):
        return v if mu == 0 else gr.jacobi9(v, b, mu, self.omega, self.jac[lv])

    def residual(self, lv, v, b):
        return gr.residual9(v, b, self.st[lv])

    def apply(self, v):
        """A v on the finest level in the order of residual9 (what k_pcg_direction<T, 2> computes)"""
        return gr._apply9(self.st[self.L], self.st[self.L][0], v)


class Hierarchy(wr.CycleIndex, _NineFinest, gr.Hierarchy):
    """bilinear transfers; .cycle = wr.V / wr.W / wr.F"""


class OpdepHierarchy(wr.CycleIndex, _NineFinest, od.Hierarchy):
    """operator-dependent transfers"""


class _ChebyNine(cr._Cheby):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._bounds()

    def _bounds(self):
        self.g = {lv: cr.lambda_bound(self.st[lv], nine=True) for lv in self.st}

    def jacobi_sweep(self, lv, v, b):
        return _NineFinest.smooth(self, lv, v, b, 1)


class ChebyHierarchy(_ChebyNine, Hierarchy):
    pass


class ChebyOpdepHierarchy(_ChebyNine, OpdepHierarchy):
    pass


class _LineNine(lr._Line):
    """H(smoother, po, st9, finest, coarsest, ...): line sweeps with corners on every level"""

    def __init__(self, smoother, *a, **kw):
        super().__init__(*a, **kw)
        self.smoother = smoother
        self._factor_levels()

    def nine_level(self, lv):
        return True


class LineHierarchy(_LineNine, Hierarchy):
    pass


class LineOpdepHierarchy(_LineNine, OpdepHierarchy):
    pass
