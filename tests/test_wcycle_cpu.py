"""CPU checks of the cycle index (mgx_set_cycle / mgx_get_cycle): the entry points in the header, the library and the
binding, and what the feature exists for - the cycle counts of the numpy reference (tests/wcycle_ref.py) on the contrast
problems of tests/pcg_ref.py with V-, W- and F-cycles.  contrast_coefficient(L, c), constant right-hand side, (2,2)
Jacobi sweeps, omega 2/3, exact bottom, tolerance 1e-8."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cheby_ref as cr
import galerkin_ref as gr
import opdep_ref as od
import wcycle_ref as wr
from conftest import ROOT
from pcg_ref import contrast_coefficient

V, W, F = wr.V, wr.W, wr.F
CLS = {"BILINEAR": wr.Galerkin, "OPERATOR": wr.Opdep}
LIMIT = 120


def test_header_library_and_binding_have_the_entry_points(pkg):
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"MGX_API\s+int\s+(mgx_\w+)\s*\(([^;]*)\);", text)}
    assert decl["mgx_set_cycle"].count(",") == 1 and decl["mgx_get_cycle"].count(",") == 1
    for name, value in (("MGX_CYCLE_V", 0), ("MGX_CYCLE_W", 1), ("MGX_CYCLE_F", 2)):
        assert re.search(r"%s\s*=\s*%d\b" % (name, value), text), name
    assert (pkg.CYCLE_V, pkg.CYCLE_W, pkg.CYCLE_F) == (0, 1, 2) == (V, W, F)
    L = C.CDLL(pkg.LIB_PATH)
    names = {"mgx_set_cycle", "mgx_get_cycle"}
    assert all(hasattr(L, n) for n in names) and names <= set(pkg.EXPORTS)
    assert len(pkg.lib().mgx_set_cycle.argtypes) == 2 and len(pkg.lib().mgx_get_cycle.argtypes) == 2
    assert all(hasattr(pkg.Multigrid, n) for n in ("set_cycle", "cycle"))
    # a NULL handle is an invalid argument, not a crash (no GPU is touched)
    out = C.c_int(7)
    for kind in (0, 1, 2, 3, -1):
        assert pkg.lib().mgx_set_cycle(None, kind) == 1
    assert pkg.lib().mgx_get_cycle(None, C.byref(out)) == 1 and out.value == 7


def test_struct_sizes_are_unchanged(pkg):
    """the cycle kind is set by call: no field is added to mgx_config, mgx_slab or mgx_stats"""
    assert (C.sizeof(pkg.Config), C.sizeof(pkg.Slab), C.sizeof(pkg.Stats)) == (144, 20, 48)


def cycles_to(h, b, kind):
    h.cycle = kind
    u, hist = h.solve(b, tol=1e-8, max_cycles=LIMIT)
    assert hist[-1] <= 1e-8 * hist[0], (kind, len(hist) - 1, hist[-1] / hist[0])
    return len(hist) - 1


# (finest, coarsest, transfer, contrast) -> (V, W) as recorded with this reference
COUNTS = {
    (8, 4, "OPERATOR", 10.0): (19, 14), (8, 4, "OPERATOR", 100.0): (36, 20), (8, 4, "OPERATOR", 1000.0): (43, 23),
    (8, 4, "BILINEAR", 10.0): (23, 19), (8, 4, "BILINEAR", 100.0): (53, 37), (8, 4, "BILINEAR", 1000.0): (68, 45),
    (9, 3, "OPERATOR", 100.0): (61, 22),
}
# F-cycles, recorded with this reference when the test was written
F_COUNTS = {
    (8, 4, "OPERATOR", 10.0): 14, (8, 4, "OPERATOR", 100.0): 21, (8, 4, "OPERATOR", 1000.0): 24,
    (8, 4, "BILINEAR", 10.0): 19, (8, 4, "BILINEAR", 100.0): 38, (8, 4, "BILINEAR", 1000.0): 46,
    (9, 3, "OPERATOR", 100.0): 23,
}


@pytest.mark.parametrize("case", list(COUNTS), ids=["-".join(map(str, c)) for c in COUNTS])
def test_w_cycles_need_fewer_cycles_than_v_cycles(po, case):
    finest, coarsest, transfer, contrast = case
    st5 = po.stencil_from_nodes(contrast_coefficient(finest, contrast), finest, finest)
    b = po.rhs_constant(finest)
    h = CLS[transfer](po, st5, finest, coarsest)
    got = {kind: cycles_to(h, b, kind) for kind in (V, W, F)}
    print(f"levels {finest}..{coarsest} {transfer} contrast {contrast:g}: V {got[V]}, W {got[W]}, F {got[F]} cycles to 1e-8")
    assert (got[V], got[W]) == COUNTS[case]
    assert got[W] < got[V]
    assert got[F] == F_COUNTS[case]
    if transfer == "OPERATOR":
        assert got[V] >= got[F] >= got[W]


@pytest.mark.parametrize("name,cls", [("galerkin", wr.Galerkin), ("opdep", wr.Opdep), ("cheby", wr.ChebyGalerkin), ("cheby-opdep", wr.ChebyOpdep)])
def test_cycle_v_is_the_parent_s_bits(po, name, cls):
    L, Lc = 6, 3
    st5 = po.stencil_from_nodes(contrast_coefficient(L, 100.0), L, L)
    b = po.rhs_sine(L)
    u0 = po.fill_uniform(b.shape, seed=5)
    parent = cls.parent
    assert parent in (gr.Hierarchy, od.Hierarchy, cr.Hierarchy, cr.OpdepHierarchy) and issubclass(cls, parent)
    for kw in (dict(), dict(bottom=gr.SMOOTH, mu2=1)):
        mine, theirs = cls(po, st5, L, Lc, **kw), parent(po, st5, L, Lc, **kw)
        assert mine.cycle == V
        assert np.array_equal(mine.vcycle(L, u0, b), theirs.vcycle(L, u0, b))
        assert np.array_equal(mine.fmg(b), theirs.fmg(b))
        for a, c in zip(mine.solve(b, u0, max_cycles=4, schedule=gr.FMG), theirs.solve(b, u0, max_cycles=4, schedule=gr.FMG)):
            assert np.array_equal(a, c)


def test_cycle_v_is_the_parent_s_bits_on_stencil5(po):
    L, Lc = 6, 3
    a = contrast_coefficient(L, 10.0)
    sts = {lv: po.stencil_from_nodes(a, lv, L) for lv in range(Lc, L + 1)}
    b = po.rhs_sine(L)
    for cls in (wr.Stencil5, wr.Stencil5Cheby):
        parent = cls.parent
        assert np.array_equal(cls(po, sts, L, Lc).vcycle(L, np.zeros_like(b), b), parent(po, sts, L, Lc).vcycle(L, np.zeros_like(b), b))


def test_the_recursion_visits_what_the_header_says(po):
    """visits of every level per cycle from level 7 down to 3, counted through smooth() and bottom(): W doubles them per
    level down to coarsest + 1 and visits the coarsest once per descent; F adds one V-cycle per level; and the second
    visit is handed the iterate the first one left, not zeros"""
    L, Lc = 7, 3
    st5 = po.stencil_from_nodes(contrast_coefficient(L, 10.0), L, L)
    b = po.rhs_sine(L)

    class Counting(wr.Opdep):
        def smooth(self, lv, v, b, mu):
            self.seen.append((lv, bool(np.any(v))))
            return super().smooth(lv, v, b, mu)

        def bottom(self, b):
            self.seen.append((self.Lc, False))
            return super().bottom(b)

    h = Counting(po, st5, L, Lc)
    want = {V: {7: 1, 6: 1, 5: 1, 4: 1, 3: 1}, W: {7: 1, 6: 2, 5: 4, 4: 8, 3: 8}, F: {7: 1, 6: 2, 5: 3, 4: 4, 3: 4}}
    for kind in (V, W, F):
        h.cycle, h.seen = kind, []
        h.vcycle(L, np.zeros_like(b), b)
        visits = {lv: sum(1 for s in h.seen if s[0] == lv) // (1 if lv == Lc else 2) for lv in range(Lc, L + 1)}
        assert visits == want[kind], (kind, visits)
        if kind != V:
            # pre-smoothing calls of level 6 alternate: first visit from zeros, second from the first one's iterate
            starts = [nz for lv, nz in h.seen if lv == 6][0::2]
            assert starts == [False, True], starts
