"""numpy statement of mgx_newton_steps (include/mgx.h, csrc/mgx_newton.hpp) on top of tests/newton_ref.py and
tests/theta_ref.py: the pass that forms a theta step's explicit part, the Newton pass with a mass term, Newton's loop
around them and the step loop.  numpy rounds every elementwise operation on its own, which is what the kernels do, so the
two passes are meant bit for bit in the operator's dtype.

One step from the time level u solves  G(v) = A0 v + dm v + kap phi(v) - r = 0  with
r = dm u - c0 (A0 u + kap phi(u)) + g,  c0 = (1 - theta) / theta,  dm = rho h^2 / (theta dt),  g = f / theta; A0 a list
of nine arrays in the storage order c, n, s, w, e, nw, ne, sw, se, everything in stencil units."""
import numpy as np

import newton_ref as nf
import theta_ref as tr


def rhs_pass(A0, kap, dm, g, p, u, theta):
    """the step's explicit part: m = dm u;  theta = 1: r = m;  theta < 1: q = A0 u, ph = ((p3 u + p2) u + p1) u,
    r = m - c0 (q + kap ph);  then + g when g is given.  theta = 1 reads dm, u (and g) only"""
    dt = u.dtype
    m = np.asarray(dm, dtype=dt) * u
    if float(theta) == 1.0:
        r = m
    else:
        p1, p2, p3, _, _ = nf.poly(p, dt)
        c0 = tr.coefficients(theta, dt)[1]
        q = tr.apply(A0, u)
        ph = ((p3 * u + p2) * u + p1) * u
        r = m - c0 * (q + np.asarray(kap, dtype=dt) * ph)
    if g is not None:
        r = r + np.asarray(g, dtype=dt)
    return r


def mass_pass(A0, kap, dm, r, p, u, de=None, lam=None):
    """the Newton pass with a mass term: v = u (de is None) or u + lam * de;  q, ph, dp as newton_ref.newton_pass;
    b = r - ((q + dm v) + kap ph);  d = dm + kap dp.  Returns (v, b, d), all in u's dtype"""
    dt = u.dtype
    p1, p2, p3, q2, q3 = nf.poly(p, dt)
    kap, dm, r = (np.asarray(a, dtype=dt) for a in (kap, dm, r))
    v = u if de is None else u + dt.type(lam) * np.asarray(de, dtype=dt)
    q = tr.apply(A0, v)
    ph = ((p3 * v + p2) * v + p1) * v
    dp = (q3 * v + q2) * v + p1
    b = r - ((q + dm * v) + kap * ph)
    d = dm + kap * dp
    return v, b, d


def newton(A0, kap, dm, r, p, u0, solve, tol, max_newton, max_backtracks, norm=nf.norm2):
    """newton_ref.newton's loop on G: the same iteration, acceptance test and records, around mass_pass"""
    un = np.array(u0, copy=True)
    _, b, dn = mass_pass(A0, kap, dm, r, p, un)
    hist, lams, lin, ds = [norm(b)], [], [], []
    backtracks, failed = 0, False
    for k in range(max_newton):
        if hist[k] <= tol * hist[0]:
            break
        d = dn
        ds.append(d)
        de, rec = solve(tr.shift(A0, d), b, d, k)
        lin.append(rec)
        lam, j = 1.0, 0
        while True:
            ut, b, dn = mass_pass(A0, kap, dm, r, p, un, de, lam)
            rr = norm(b)
            if nf.armijo(rr, lam, hist[k]):
                break
            backtracks += 1
            j += 1
            if j > max_backtracks:
                failed = True
                break
            lam = lam / 2
        if failed:
            break
        un = ut
        hist.append(rr)
        lams.append(lam)
    return dict(u=un, hist=np.array(hist), lam=np.array(lams), lin=lin, backtracks=backtracks,
                converged=bool(hist[-1] <= tol * hist[0]), failed=failed, ds=ds)


def steps(A0, kap, dm, g, p, u0, theta, nsteps, solve, tol, max_newton, max_backtracks, norm=nf.norm2):
    """the step loop of mgx_newton_steps: r from the time level, Newton from the time level as the guess; a step that does
    not converge is the last one.  Returns the list of newton()'s dicts, one per step taken, each with its r"""
    u = np.array(u0, copy=True)
    out = []
    for _ in range(nsteps):
        r = rhs_pass(A0, kap, dm, g, p, u, theta)
        o = newton(A0, kap, dm, r, p, u, solve, tol, max_newton, max_backtracks, norm)
        o["r"] = r
        out.append(o)
        u = o["u"]
        if not o["converged"]:
            break
    return out


def g_norm(A0, kap, dm, g, p, u, v, theta):
    """||G(v)||_2 of the step from u, every term in float64 and summed in another order than the passes' (the diffusion
    through the sparse matrix of newton_ref.sparse): an independent statement"""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    A = nf.sparse(A0)
    p1, p2, p3 = (float(x) for x in p)
    phi = lambda w: p1 * w + p2 * w ** 2 + p3 * w ** 3
    n = u.shape[0]
    op = lambda w: (A @ f64(w).ravel()).reshape(n, n)
    c0 = (1.0 - float(theta)) / float(theta)
    r = f64(dm) * f64(u) - c0 * (op(u) + f64(kap) * phi(f64(u))) + (0.0 if g is None else f64(g))
    G = op(v) + f64(dm) * f64(v) + f64(kap) * phi(f64(v)) - r
    return float(np.sqrt(np.sum(G * G)))
