"""numpy statement of the zebra line Gauss-Seidel smoothers (cfg.smoother = MGX_SMOOTHER_LINE_X / LINE_Y / LINE_ALT,
csrc/mgx_line.hpp) on top of the hierarchies of tests/galerkin_ref.py, tests/opdep_ref.py and tests/cheby_ref.py, and
composed with the cycle index of tests/wcycle_ref.py.

An operator is nine interior n x n arrays in the slot order c, n, s, w, e, nw, ne, sw, se (galerkin_ref); interior
index k is grid row / column k + 1, so the ODD grid rows (colour 1, the rows that are not coarse rows) are the interior
indices 0, 2, 4, ... and the EVEN grid rows (colour 2) are 1, 3, 5, ...

THE FACTORS of the tridiagonal matrix T = tridiag(w, c, e) of a grid row, in the level's type, sequentially along the
line (the Thomas recurrences), with p_j the pivot:

    p_0 = c_0                          m_0 = 1 / p_0
    g_{j-1} = e_{j-1} m_{j-1}          p_j = c_j - w_j g_{j-1}          m_j = 1 / p_j            j = 1 .. n - 1
    g_{n-1} = 0                        (e_{n-1} points at the Dirichlet ring and is never read, like w_0)

A pivot that is zero or not finite is a breakdown (factor() reports it).

THE X-LINE ZEBRA SWEEP, per colour (odd grid rows first, then the even ones, which read the rows just written):

    rhs_j = b_ij, then one subtraction per off-line neighbour, in the order  NW, N, NE, SW, S, SE  (five-point levels:
            N, S):  rhs_j = rhs_j - a_x v_x.  A coefficient that points at the Dirichlet ring is never read: that term
            is left out
    y_0 = rhs_0 m_0                    y_j = (rhs_j - w_j y_{j-1}) m_j
    x_{n-1} = y_{n-1}                  x_j = y_j - g_j x_{j+1}
    row i of v = x

No damping.  THE Y-LINE SWEEP is the x-line sweep of the transposed problem (T = tridiag(n, c, s) down a column, odd
grid columns first; off-line order NW, W, SW, NE, E, SE in the original orientation).  THE ALTERNATING SWEEP is one
x-line sweep followed by one y-line sweep.  numpy rounds every elementwise operation separately, which is what the
kernels do (-ffp-contract=off); the device's carries across lanes and chunks are combined in another order, so device
results agree to rounding (tests/test_gpu_line.py derives the bound), the factors bit for bit."""
import numpy as np

import cheby_ref as cr
import galerkin_ref as gr
import opdep_ref as od
import wcycle_ref as wr

LINE_X, LINE_Y, LINE_ALT = 4, 5, 6                       # MGX_SMOOTHER_LINE_*
DIRS = {LINE_X: "x", LINE_Y: "y", LINE_ALT: "xy"}
OFFLINE = [(-1, -1), (-1, 0), (-1, 1), (1, -1), (1, 0), (1, 1)]      # NW, N, NE, SW, S, SE


class Breakdown(ArithmeticError):
    """a zero or non-finite pivot in the factorisation of a line"""


def transposed(st9):
    """the operator of the transposed problem: the coefficient that pointed at (dy, dx) points at (dx, dy)"""
    out = [None] * 9
    for (dy, dx), q in gr.SLOT.items():
        out[gr.SLOT[dx, dy]] = np.ascontiguousarray(st9[q].T)
    return out


def factor(st9):
    """(m, g, ok) of the x-lines (grid rows) of an operator: n x n arrays, ok = no pivot was zero or not finite"""
    c, w, e = st9[0], st9[3], st9[4]
    dt = c.dtype
    n = c.shape[1]
    m, g = np.empty_like(c), np.zeros_like(c)
    with np.errstate(all="ignore"):
        p = c[:, 0]
        bad = ~np.isfinite(p) | (p == 0)
        m[:, 0] = dt.type(1) / p
        for j in range(1, n):
            g[:, j - 1] = e[:, j - 1] * m[:, j - 1]
            p = c[:, j] - w[:, j] * g[:, j - 1]
            bad |= ~np.isfinite(p) | (p == 0)
            m[:, j] = dt.type(1) / p
    return m, g, not bad.any()


def factor_dir(st9, d):
    """the factors of direction d ('x' or 'y') in the level's own orientation (row i, column j)"""
    if d == "x":
        return factor(st9)
    m, g, ok = factor(transposed(st9))
    return np.ascontiguousarray(m.T), np.ascontiguousarray(g.T), ok


def line_rhs(st9, v, b, rows, nine):
    """b - sum of the off-line terms on the interior rows `rows`, one subtraction per neighbour in the order OFFLINE"""
    n = v.shape[0]
    P = np.pad(v, 1)
    rhs = b[rows].copy()
    for dy, dx in OFFLINE:
        if not nine and dx != 0:
            continue
        a = st9[gr.SLOT[dy, dx]][rows]
        term = a * P[rows + 1 + dy, 1 + dx:1 + dx + n]
        # never read: coefficients that point at the ring (first / last row, first / last column)
        ring = ((rows + dy < 0) | (rows + dy > n - 1))[:, None] | np.zeros((1, n), dtype=bool)
        if dx < 0:
            ring[:, 0] = True
        if dx > 0:
            ring[:, -1] = True
        rhs = np.where(ring, rhs, rhs - term)
    return rhs


def solve_lines(m, g, w, rhs):
    """T x = rhs of every row with the factors (m, g) of T and its sub-diagonal w"""
    n = rhs.shape[1]
    y = np.empty_like(rhs)
    y[:, 0] = rhs[:, 0] * m[:, 0]
    for j in range(1, n):
        y[:, j] = (rhs[:, j] - w[:, j] * y[:, j - 1]) * m[:, j]
    x = np.empty_like(rhs)
    x[:, n - 1] = y[:, n - 1]
    for j in range(n - 2, -1, -1):
        x[:, j] = y[:, j] - g[:, j] * x[:, j + 1]
    return x


def sweep_x(st9, fac, v, b, nine):
    """one zebra x-line sweep; fac = factor(st9)[:2]"""
    m, g = fac
    n = v.shape[0]
    v = np.array(v, copy=True)
    with np.errstate(all="ignore"):
        for first in (0, 1):                                  # interior 0, 2, ... = odd grid rows = colour 1
            rows = np.arange(first, n, 2)
            if rows.size:
                v[rows] = solve_lines(m[rows], g[rows], st9[3][rows], line_rhs(st9, v, b, rows, nine))
    return v


def sweep_y(st9, fac_t, v, b, nine):
    """one zebra y-line sweep; fac_t = factor(transposed(st9))[:2]"""
    return np.ascontiguousarray(sweep_x(transposed(st9), fac_t, np.ascontiguousarray(v.T), np.ascontiguousarray(b.T), nine).T)


class LevelSmoother:
    """the line smoother of one level: factors of the directions of `smoother`, sweep(v, b, mu)"""

    def __init__(self, st9, nine, smoother, level=None):
        self.st, self.nine, self.dirs = st9, nine, DIRS[smoother]
        self.fx = self.fy = None
        if "x" in self.dirs:
            *self.fx, ok = factor(st9)
            if not ok:
                raise Breakdown(f"level {level}: zero or non-finite pivot in an x-line")
        if "y" in self.dirs:
            self.stT = transposed(st9)
            *self.fy, ok = factor(self.stT)
            if not ok:
                raise Breakdown(f"level {level}: zero or non-finite pivot in a y-line")

    def sweep(self, v, b, mu=1):
        for _ in range(mu):
            if "x" in self.dirs:
                v = sweep_x(self.st, self.fx, v, b, self.nine)
            if "y" in self.dirs:
                v = np.ascontiguousarray(sweep_x(self.stT, self.fy, np.ascontiguousarray(v.T), np.ascontiguousarray(b.T), self.nine).T)
        return v


class NumpyOps:
    """what the hierarchies take from the oracle (po), in numpy for any float type - np.longdouble, which the oracle's C
    has no build for, is the 'exact' side of the tests' error measurements.  Full weighting R = c P^T of the bilinear P
    (c = 1: CONSISTENT, 1/4: FW16) and the five-point residual; the rounding order is not the oracle's"""

    @staticmethod
    def var_build_jacobi(*a, **kw):
        return None

    @staticmethod
    def restrict(fine, mode=gr.CONSISTENT):
        P = np.pad(fine, 1)
        n = fine.shape[0]
        acc = None
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                t = fine.dtype.type((1 - 0.5 * abs(dy)) * (1 - 0.5 * abs(dx))) * P[2 + dy:1 + n + dy:2, 2 + dx:1 + n + dx:2]
                acc = t if acc is None else acc + t
        return acc * fine.dtype.type(0.25 if mode == gr.FW16 else 1.0)

    @staticmethod
    def prolong(coarse):
        nc = coarse.shape[0]
        P = np.pad(coarse, 1)
        f = np.zeros((2 * nc + 1, 2 * nc + 1), dtype=coarse.dtype)
        h, q = coarse.dtype.type(0.5), coarse.dtype.type(0.25)
        f[1::2, 1::2] = coarse
        f[0::2, 1::2] = h * (P[:-1, 1:-1] + P[1:, 1:-1])
        f[1::2, 0::2] = h * (P[1:-1, :-1] + P[1:-1, 1:])
        f[0::2, 0::2] = q * (P[:-1, :-1] + P[1:, :-1] + P[:-1, 1:] + P[1:, 1:])
        return f

    @classmethod
    def prolong_add(cls, v, coarse):
        return v + cls.prolong(coarse)

    @staticmethod
    def var_residual(v, b, coef):
        return gr.residual9(v, b, gr.nine(list(coef)))

    @staticmethod
    def norm2(x):
        return float(np.sqrt(np.sum(x * x)))


class _Line:
    """smooth() of a hierarchy as mu line sweeps of `smoother`; every level's factors are built with the hierarchy"""
    smoother = LINE_X

    def _factor_levels(self):
        self.line = {lv: LevelSmoother(self.st[lv], self.nine_level(lv), self.smoother, lv) for lv in self.st}

    def nine_level(self, lv):
        return lv != self.L

    def smooth(self, lv, v, b, mu):
        return v if mu == 0 else self.line[lv].sweep(v, b, mu)


def _make(base, five_point=False):
    class H(_Line, wr.CycleIndex, base):
        def __init__(self, smoother, *a, cycle=wr.V, **kw):
            super().__init__(*a, **kw)
            self.smoother, self.cycle = smoother, cycle
            self._factor_levels()

        if five_point:
            def nine_level(self, lv):
                return False

    H.__name__ = H.__qualname__ = "Line" + base.__name__
    return H


# H(smoother, po, st5 | stencils, finest, coarsest, dtype, ..., cycle=V | W | F): the constructors of the base classes
# with the smoother in front
Hierarchy = _make(gr.Hierarchy)                 # GALERKIN, bilinear transfers
OpdepHierarchy = _make(od.Hierarchy)            # GALERKIN, operator-dependent transfers
Stencil5 = _make(cr.Stencil5, five_point=True)  # STENCIL5


def aniso_stencil(level, eps, kind="x", dtype=np.float64):
    """(c, n, s, w, e) of -ex u_xx - ey u_yy on a level: kind 'x': ex = 1, ey = eps (x-strong); 'y': ex = eps, ey = 1;
    'layers': x-strong on the interior rows < n // 2, y-strong from row n // 2 on"""
    n = (1 << level) - 1
    ex, ey = np.empty((n, n)), np.empty((n, n))
    if kind == "x":
        ex[:], ey[:] = 1.0, eps
    elif kind == "y":
        ex[:], ey[:] = eps, 1.0
    else:
        ex[:n // 2], ey[:n // 2] = 1.0, eps
        ex[n // 2:], ey[n // 2:] = eps, 1.0
    return [a.astype(dtype) for a in (2.0 * (ex + ey), -ey, -ey, -ex, -ex)]
