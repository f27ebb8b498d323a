"""numpy statement of the multicolour Gauss-Seidel smoothers (cfg.smoother = MGX_SMOOTHER_COLOR_GS / COLOR_SGS,
csrc/mgx_colour.hpp) on top of the hierarchies of tests/galerkin_ref.py, tests/opdep_ref.py, tests/cheby_ref.py and
tests/nine_ref.py, composed with the cycle index of tests/wcycle_ref.py.

An operator is nine interior n x n arrays in the slot order c, n, s, w, e, nw, ne, sw, se (galerkin_ref); interior index k
is grid row / column k + 1.

THE SWEEP updates the colours of a level one after the other; every point of a colour, from the current state of its
neighbours,

    x_ij = (b_ij - S_ij) * D_inv_ij,     S_ij = the sum of the off-diagonal terms a_k u_k of A, in the CSR order NW, N, NE,
                                         W, E, SW, S, SE (five-point levels: N, W, E, S), the first term starting the sum,
                                         D_inv = 1 / c in the level's type (the stored array of the Jacobi splitting).

Coefficients that point at the Dirichlet ring multiply the ring of the iterate, which is zero (the rule of the residual).

    five-point level, two colours:   colour 0 = (grid row + grid column) even = (i + j) even in interior indices, then odd
    nine-point level, four colours by (grid row parity, grid column parity), in the order
                                     (odd, odd), (odd, even), (even, odd), (even, even)
                                     = interior (i even, j even), (i even, j odd), (i odd, j even), (i odd, j odd):
                                     the coarse points (even, even) last

A REVERSE sweep takes the colours in the opposite order with the same update.  COLOR_GS sweeps forward in every block;
COLOR_SGS sweeps forward in the pre-smoothing blocks (and the first mu1 sweeps of a bottom = SMOOTH visit) and in reverse
in the post-smoothing blocks (and the last mu2 sweeps of that visit).  numpy rounds every elementwise operation
separately, which is what the kernels do (-ffp-contract=off): a sweep is meant bit for bit."""
import numpy as np

import cheby_ref as cr
import galerkin_ref as gr
import nine_ref as nr
import opdep_ref as od
import wcycle_ref as wr

COLOR_GS, COLOR_SGS = 8, 9                               # MGX_SMOOTHER_COLOR_*
NAMES = {COLOR_GS: "gs", COLOR_SGS: "sgs"}
OFFDIAG = [d for d in gr.ROW_MAJOR if d != (0, 0)]       # NW, N, NE, W, E, SW, S, SE


def colours(n, nine):
    """the boolean masks of the colours of an n x n level, in forward order"""
    i, j = np.indices((n, n))
    if not nine:
        return [(i + j) % 2 == 0, (i + j) % 2 == 1]
    return [(i % 2 == 0) & (j % 2 == 0), (i % 2 == 0) & (j % 2 == 1), (i % 2 == 1) & (j % 2 == 0), (i % 2 == 1) & (j % 2 == 1)]


def offdiag_sum(st9, v, nine):
    """S of every point from the state v, one product and one addition per neighbour in the order OFFDIAG"""
    P = np.pad(v, 1)
    n = v.shape[0]
    acc = None
    for dy, dx in OFFDIAG:
        if not nine and dy != 0 and dx != 0:
            continue
        term = st9[gr.SLOT[dy, dx]] * P[1 + dy:1 + dy + n, 1 + dx:1 + dx + n]
        acc = term if acc is None else acc + term
    return acc


def dinv_of(st9):
    return st9[0].dtype.type(1) / st9[0]


def sweep(st9, dinv, v, b, nine, reverse=False):
    """one sweep over all colours, in the type of v"""
    v = np.array(v, copy=True)
    order = colours(v.shape[0], nine)
    with np.errstate(all="ignore"):
        for mask in (order[::-1] if reverse else order):
            v = np.where(mask, (b - offdiag_sum(st9, v, nine)) * dinv, v)
    return v


def smooth(st9, dinv, v, b, mu, nine, reverse=False):
    for _ in range(mu):
        v = sweep(st9, dinv, v, b, nine, reverse)
    return v


class _Colour:
    """smooth() of a hierarchy as mu colour sweeps, and the cycle (V, W or F) with the direction of every block stated:
    pre-smoothing forward, post-smoothing in reverse when the smoother is COLOR_SGS"""
    smoother = COLOR_GS

    def _colour_levels(self):
        self.dinv = {lv: dinv_of(self.st[lv]) for lv in self.st}

    def nine_level(self, lv):
        return lv != self.L

    def smooth(self, lv, v, b, mu, post=False):
        if mu == 0:
            return v
        return smooth(self.st[lv], self.dinv[lv], v, b, mu, self.nine_level(lv), reverse=post and self.smoother == COLOR_SGS)

    def _colour_cycle(self, lv, v, b, kind):
        if lv == self.Lc:
            if self.bottom_mode == gr.EXACT:
                return self.bottom(b)
            return self.smooth(lv, self.smooth(lv, v, b, self.mu1, False), b, self.mu2, True)
        v = self.smooth(lv, v, b, self.mu1, False)
        rc = self._restrict_residual(lv, v, b)
        e = self._colour_cycle(lv - 1, np.zeros_like(rc), rc, kind)
        if kind != wr.V and lv - 1 > self.Lc:
            e = self._colour_cycle(lv - 1, e, rc, wr.V if kind == wr.F else kind)
        v = self._correct(lv, v, e)
        return self.smooth(lv, v, b, self.mu2, True)

    def vcycle(self, lv, v, b):
        return self._colour_cycle(lv, v, b, self.cycle)


def _make(base, nine_finest=None):
    bases = (_Colour, base) if issubclass(base, wr.CycleIndex) else (_Colour, wr.CycleIndex, base)

    class H(*bases):
        def __init__(self, smoother, *a, cycle=wr.V, **kw):
            super().__init__(*a, **kw)
            self.smoother, self.cycle = smoother, cycle
            self._colour_levels()

        if nine_finest is not None:
            def nine_level(self, lv):
                return nine_finest

    H.__name__ = H.__qualname__ = "Colour" + base.__name__
    return H


# H(smoother, po, st5 | stencils | st9, finest, coarsest, dtype, ..., cycle=V | W | F): the constructors of the base
# classes with the smoother in front
Hierarchy = _make(gr.Hierarchy)                          # GALERKIN, five-point finest level, bilinear transfers
OpdepHierarchy = _make(od.Hierarchy)                     # GALERKIN, five-point finest level, operator-dependent transfers
Stencil5 = _make(cr.Stencil5, nine_finest=False)         # STENCIL5: five-point on every level
NineHierarchy = _make(nr.Hierarchy, nine_finest=True)    # GALERKIN, nine-point finest level (mgx_set_stencil9 / mgx_set_tensor)
NineOpdepHierarchy = _make(nr.OpdepHierarchy, nine_finest=True)

