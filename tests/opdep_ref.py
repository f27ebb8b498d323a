"""numpy statement of the operator-dependent ("black box", Alcouffe / Dendy) transfers of the Galerkin hierarchy
(mgx_build_galerkin_transfer(h, MGX_TRANSFER_OPERATOR), csrc/mgx_opdep.hpp): the weights of P read off the operator's
own stencil, P, R = c P^T, the product c P^T A P term by term in the kernel's documented order, and a Hierarchy with
the interface of tests/galerkin_ref.py.  numpy rounds every elementwise operation separately, which is what the
kernels do (-ffp-contract=off), so every step is meant bit for bit.

A set of weights is a list of eight interior n_c x n_c arrays in the order n, s, w, e, nw, ne, sw, se: the weight with
which coarse point (I, J) contributes to fine point (2I + di, 2J + dj).  The coincident weight is 1 and not stored."""
import numpy as np

import galerkin_ref as gr

DIRS = ("n", "s", "w", "e", "nw", "ne", "sw", "se")
OFFS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))
WSLOT = {off: k for k, off in enumerate(OFFS)}
BILINEAR, OPERATOR = 0, 1
_Q = {name: k for k, name in enumerate(gr.SLOTS)}


def weights(st9, N_f):
    """the eight weight grids of P between the level with N_f intervals per side and the next coarser one.

    With the stencil (c, n, s, w, e, nw, ne, sw, se) of the FINE point the weight belongs to:
      n:  fine (2I-1, 2J)    -(((sw + s) + se) / ((w + c) + e))        s:  fine (2I+1, 2J)    -(((nw + n) + ne) / ((w + c) + e))
      w:  fine (2I, 2J-1)    -(((ne + e) + se) / ((n + c) + s))        e:  fine (2I, 2J+1)    -(((nw + w) + sw) / ((n + c) + s))
      nw: fine (2I-1, 2J-1)  -(((se + s * W_w) + e * W_n) / c)         ne: fine (2I-1, 2J+1)  -(((sw + s * W_e) + w * W_n) / c)
      sw: fine (2I+1, 2J-1)  -(((ne + n * W_w) + e * W_s) / c)         se: fine (2I+1, 2J+1)  -(((nw + n * W_e) + w * W_s) / c)
    (W_x: the edge weights of the same coarse point: the edge point between the cell centre and the coarse point's row
    or column interpolates from that coarse point with exactly that weight).  A denominator that is zero or not finite:
    the bilinear weight 1/2 (edges) or 1/4 (centres).  No coefficient that points at the Dirichlet ring is read."""
    dt = st9[0].dtype
    nc = N_f // 2 - 1
    assert st9[0].shape == (N_f - 1, N_f - 1)

    def A(name, oy, ox):                   # coefficient `name` of the fine points (2I + oy, 2J + ox), I, J = 1 .. N_c - 1
        return st9[_Q[name]][1 + oy::2, 1 + ox::2][:nc, :nc]

    def guarded(num, den, fallback):
        w = -(num / den)
        return np.where(np.isfinite(den) & (den != 0), w, dt.type(fallback))

    with np.errstate(all="ignore"):
        den = (A("w", -1, 0) + A("c", -1, 0)) + A("e", -1, 0)
        wn = guarded((A("sw", -1, 0) + A("s", -1, 0)) + A("se", -1, 0), den, 0.5)
        den = (A("w", 1, 0) + A("c", 1, 0)) + A("e", 1, 0)
        ws = guarded((A("nw", 1, 0) + A("n", 1, 0)) + A("ne", 1, 0), den, 0.5)
        den = (A("n", 0, -1) + A("c", 0, -1)) + A("s", 0, -1)
        ww = guarded((A("ne", 0, -1) + A("e", 0, -1)) + A("se", 0, -1), den, 0.5)
        den = (A("n", 0, 1) + A("c", 0, 1)) + A("s", 0, 1)
        we = guarded((A("nw", 0, 1) + A("w", 0, 1)) + A("sw", 0, 1), den, 0.5)
        wnw = guarded((A("se", -1, -1) + A("s", -1, -1) * ww) + A("e", -1, -1) * wn, A("c", -1, -1), 0.25)
        wne = guarded((A("sw", -1, 1) + A("s", -1, 1) * we) + A("w", -1, 1) * wn, A("c", -1, 1), 0.25)
        wsw = guarded((A("ne", 1, -1) + A("n", 1, -1) * ww) + A("e", 1, -1) * ws, A("c", 1, -1), 0.25)
        wse = guarded((A("nw", 1, 1) + A("n", 1, 1) * we) + A("w", 1, 1) * ws, A("c", 1, 1), 0.25)
    return [np.ascontiguousarray(x, dtype=dt) for x in (wn, ws, ww, we, wnw, wne, wsw, wse)]


def bilinear_weights(nc, dt=np.float64):
    return [np.full((nc, nc), 0.5, dtype=dt) for _ in range(4)] + [np.full((nc, nc), 0.25, dtype=dt) for _ in range(4)]


def prolong(e, W):
    """P e.  A fine point on a coarse row: west coarse point first, then east; on a coarse column: north, then south;
    a cell centre: ((NW + NE) + SW) + SE.  Ring coarse points carry e = 0 and the weight 0."""
    dt = e.dtype
    nc = e.shape[0]
    E = np.pad(e, 1)
    n_, s_, w_, e_, nw_, ne_, sw_, se_ = [np.pad(w, 1) for w in W]
    out = np.zeros((2 * nc + 1, 2 * nc + 1), dtype=dt)
    out[1::2, 1::2] = e
    out[1::2, 0::2] = e_[1:-1, :-1] * E[1:-1, :-1] + w_[1:-1, 1:] * E[1:-1, 1:]
    out[0::2, 1::2] = s_[:-1, 1:-1] * E[:-1, 1:-1] + n_[1:, 1:-1] * E[1:, 1:-1]
    acc = se_[:-1, :-1] * E[:-1, :-1] + sw_[:-1, 1:] * E[:-1, 1:]
    acc = acc + ne_[1:, :-1] * E[1:, :-1]
    out[0::2, 0::2] = acc + nw_[1:, 1:] * E[1:, 1:]
    return out


def prolong_add(v, e, W):
    return v + prolong(e, W)


def restrict(r, W, mode=gr.CONSISTENT):
    """c P^T r: the sum over the 3 x 3 fine patch row-major (NW, N, NE, W, C, E, SW, S, SE; the centre's weight 1 is
    not multiplied), then one multiplication by c = 1 (CONSISTENT) or 1/4 (FW16)"""
    dt = r.dtype
    nc = (r.shape[0] + 1) // 2 - 1
    acc = None
    for oy, ox in gr.ROW_MAJOR:
        f = r[1 + oy::2, 1 + ox::2][:nc, :nc]
        term = f if (oy, ox) == (0, 0) else W[WSLOT[oy, ox]] * f
        acc = term if acc is None else acc + term
    return dt.type(0.25 if mode == gr.FW16 else 1.0) * acc


def rap(st9, W, N_f, mode=gr.CONSISTENT):
    """A_c(I, I+D) = sum_i sum_d R(I, i) A_f(i, i+d) P(i+d, I+D) in the order of galerkin_ref.rap (accumulator from +0; i
    row-major over the 3 x 3 patch around 2I; d row-major; D row-major; structurally zero P(i+d, I+D) skipped); each
    term is ((c * P(i, I)) * A_f(i, i+d)) * P(i+d, I+D), the products formed left to right, with the coincident weights
    the constant 1.  Offsets that point at the Dirichlet ring get 0."""
    dt = st9[0].dtype
    nf = N_f - 1
    assert st9[0].shape == (nf, nf)
    nc = N_f // 2 - 1
    rscale = dt.type(0.25 if mode == gr.FW16 else 1.0)
    one = np.ones((nc + 2, nc + 2), dtype=dt)
    Wp = [np.pad(w, 1) for w in W]
    out = [np.zeros((nc, nc), dtype=dt) for _ in range(9)]
    with np.errstate(all="ignore"):
        for iy in (-1, 0, 1):
            for ix in (-1, 0, 1):
                pi = one[1:-1, 1:-1] if (iy, ix) == (0, 0) else W[WSLOT[iy, ix]]
                ri = rscale * pi
                for dy, dx in gr.ROW_MAJOR:
                    a = st9[gr.SLOT[dy, dx]][1 + iy::2, 1 + ix::2][:nc, :nc]
                    ra = ri * a
                    for Dy, Dx in gr.ROW_MAJOR:
                        oy, ox = iy + dy - 2 * Dy, ix + dx - 2 * Dx
                        if abs(oy) > 1 or abs(ox) > 1:
                            continue
                        src = one if (oy, ox) == (0, 0) else Wp[WSLOT[oy, ox]]
                        pj = src[1 + Dy:1 + Dy + nc, 1 + Dx:1 + Dx + nc]
                        o = gr.SLOT[Dy, Dx]
                        out[o] = out[o] + ra * pj
    for (Dy, Dx), o in gr.SLOT.items():
        if Dy < 0:
            out[o][0, :] = 0
        if Dy > 0:
            out[o][-1, :] = 0
        if Dx < 0:
            out[o][:, 0] = 0
        if Dx > 0:
            out[o][:, -1] = 0
    return out


class Hierarchy(gr.Hierarchy):
    """galerkin_ref.Hierarchy with P_l from A_l on every level and A_{l-1} = c P_l^T A_l P_l; smooth, residual, bottom
    and solve are the parent's"""

    def __init__(self, po, st5, finest, coarsest, dtype=np.float64, mode=gr.CONSISTENT, omega=2.0 / 3.0, mu1=2, mu2=2, mu0=0, bottom=gr.EXACT):
        self.po, self.L, self.Lc, self.dt, self.mode, self.omega, self.mu1, self.mu2 = po, finest, coarsest, dtype, mode, omega, mu1, mu2
        self.mu0, self.bottom_mode = mu0, bottom
        self.st = {finest: gr.nine([np.asarray(x, dtype=dtype) for x in st5])}
        self.W = {}
        for lv in range(finest, coarsest, -1):
            self.W[lv] = weights(self.st[lv], 1 << lv)
            self.st[lv - 1] = rap(self.st[lv], self.W[lv], 1 << lv, mode)
        self.jac = {lv: gr.build_jacobi9(self.st[lv], omega) for lv in self.st}
        self.jac5 = po.var_build_jacobi(*self.st[finest][:5], omega=omega)
        self._inv = None

    def restrict(self, lv, r):
        return restrict(r, self.W[lv], self.mode)

    def prolong(self, lv, e):
        return prolong(e, self.W[lv])

    def vcycle(self, lv, v, b):
        if lv == self.Lc:
            if self.bottom_mode == gr.EXACT:
                return self.bottom(b)
            return self.smooth(lv, self.smooth(lv, v, b, self.mu1), b, self.mu2)
        v = self.smooth(lv, v, b, self.mu1)
        rc = self.restrict(lv, self.residual(lv, v, b))
        e = self.vcycle(lv - 1, np.zeros_like(rc), rc)
        v = v + self.prolong(lv, e)
        return self.smooth(lv, v, b, self.mu2)

    def fmg(self, b):
        rhs = {self.L: np.ascontiguousarray(b, dtype=self.dt)}
        for lv in range(self.L, self.Lc, -1):
            rhs[lv - 1] = self.restrict(lv, rhs[lv])
        if self.bottom_mode == gr.EXACT:
            v = self.bottom(rhs[self.Lc])
        else:
            v = np.zeros_like(rhs[self.Lc])
            for _ in range(self.mu0 + 1):
                v = self.vcycle(self.Lc, v, rhs[self.Lc])
        for lv in range(self.Lc + 1, self.L + 1):
            v = self.prolong(lv, v)
            for _ in range(self.mu0 + 1):
                v = self.vcycle(lv, v, rhs[lv])
        return v
