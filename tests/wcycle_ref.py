"""numpy statement of the cycle index (mgx_set_cycle, include/mgx.h): W- and F-cycles on the hierarchies of
tests/galerkin_ref.py, tests/opdep_ref.py and tests/cheby_ref.py.  A mixin in front of one of those classes gives it a
`cycle` attribute; vcycle() - and with it the inherited fmg() and solve() - then runs the recursion

    V: pre-smooth, restrict; cycle(l - 1); correct, post-smooth                                  (the parent's own)
    W: pre-smooth, restrict; cycle(l - 1); if l - 1 > coarsest: cycle(l - 1) again; correct, post-smooth
    F: as W, but the second visit of level l - 1 is a V-cycle

The second visit starts from the coarse iterate the first one left, with the same coarse right-hand side; it is never
a zero guess.  The coarsest level is visited once per descent: with bottom = EXACT a second solve returns the same
vector, and with bottom = SMOOTH the single visit (mu1 + mu2 sweeps) is the definition.  With cycle = V every call goes
to the parent class unchanged, so the bits are the parent's."""
import numpy as np

import cheby_ref as cr
import galerkin_ref as gr
import opdep_ref as od

V, W, F = 0, 1, 2
NAMES = {V: "V", W: "W", F: "F"}


class CycleIndex:
    cycle = V

    @property
    def own_transfers(self):
        """does the hierarchy carry its own restrict() / prolong() (opdep_ref: operator-dependent P), or does it use the
        oracle's full weighting / injection and bilinear prolongation?"""
        return isinstance(self, od.Hierarchy)

    def _restrict_residual(self, lv, v, b):
        r = self.residual(lv, v, b)
        if self.own_transfers:
            return self.restrict(lv, r)
        if self.mode >= 2:                                   # MGX_RESTRICT_INJECT / INJECT4 (MF:122-130), STENCIL5 only
            return self.po.restrict_inject(r, 4.0 if self.mode == 3 else 1.0)
        return self.po.restrict(r, self.mode)

    def _correct(self, lv, v, e):
        return v + self.prolong(lv, e) if self.own_transfers else self.po.prolong_add(v, e)

    def _cycle(self, lv, v, b, kind):
        if lv == self.Lc:
            if self.bottom_mode == gr.EXACT:
                return self.bottom(b)
            return self.smooth(lv, self.smooth(lv, v, b, self.mu1), b, self.mu2)
        v = self.smooth(lv, v, b, self.mu1)
        rc = self._restrict_residual(lv, v, b)
        e = self._cycle(lv - 1, np.zeros_like(rc), rc, kind)
        if kind != V and lv - 1 > self.Lc:
            e = self._cycle(lv - 1, e, rc, V if kind == F else kind)
        v = self._correct(lv, v, e)
        return self.smooth(lv, v, b, self.mu2)

    def vcycle(self, lv, v, b):
        if self.cycle == V:
            return super().vcycle(lv, v, b)
        return self._cycle(lv, v, b, self.cycle)


class Galerkin(CycleIndex, gr.Hierarchy):
    parent = gr.Hierarchy


class Opdep(CycleIndex, od.Hierarchy):
    parent = od.Hierarchy


class ChebyGalerkin(CycleIndex, cr.Hierarchy):
    parent = cr.Hierarchy


class ChebyOpdep(CycleIndex, cr.OpdepHierarchy):
    parent = cr.OpdepHierarchy


class Stencil5(CycleIndex, cr.Stencil5):
    parent = cr.Stencil5


class Stencil5Cheby(CycleIndex, cr.Stencil5Cheby):
    parent = cr.Stencil5Cheby


def with_cycle(cls, cycle, *a, **kw):
    h = cls(*a, **kw)
    h.cycle = cycle
    return h
