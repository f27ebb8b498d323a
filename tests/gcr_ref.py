"""numpy statement of mgx_solve_gcr (include/mgx.h, csrc/mgx_krylov.hpp): restarted GCR with right preconditioning
(FGMRES(restart) in exact arithmetic) around one multigrid cycle from zero - the steps of the device in the same order.

Vectors are kept in the working type T (float64 or float32); dots are accumulated in float64; the scalars are float64,
rounded to T once where they are applied; numpy rounds every elementwise operation separately, as the kernels do.

    r = b - A x;  h0 = ||r||;  basis empty
    iteration k:  j = k mod restart;  if j == 0: basis empty
      z = M r                                   (zero-start cycle)
      q = A z
      h_i = (q.Q_i) / s_i   for i < j           (classical Gram-Schmidt: all dots from the unmodified q)
      q' = ((q - h_0 Q_0) - h_1 Q_1) - ... ;  z' = the same combination of z and Z_i
      s_j = q'.q';  rho = r.q';  breakdown unless s_j > 0 and finite;  alpha = rho / s_j
      x += alpha z';  r -= alpha q';  history <- sqrt(r.r);  Z_j = z', Q_j = q'
      stop when ||r|| <= tol h0 or k + 1 == max_iters

The residual norm never increases: alpha minimises ||r - alpha q'|| and q' is orthogonal to the Q_i of this restart
cycle, along which r has already been minimised."""
import numpy as np

from pcg_ref import dot


def gcr(A, M, b, x0, tol=1e-8, max_iters=100, restart=4, dot=dot):
    """A: callable u -> A u with A.dtype;  M: callable r -> one cycle from zero for A z = r;  dot: the inner product
    (float64 result; the tests pass another summation order to measure what that order is worth).
    Returns (x, history, converged, breakdown)."""
    dt = A.dtype
    x = np.array(x0, dtype=dt, copy=True)
    b = np.asarray(b, dtype=dt)
    r = b - A(x)
    h0 = np.sqrt(dot(r, r))
    hist = [h0]
    if h0 <= tol * h0 or max_iters == 0:
        return x, np.array(hist), h0 <= tol * h0, False
    Z, Q, S = [], [], []
    for k in range(max_iters):
        j = k % restart
        if j == 0:
            Z, Q, S = [], [], []
        z = M(r)
        q = A(z)
        h = [dot(q, Q[i]) / S[i] for i in range(j)]
        for i in range(j):
            q = q - dt(h[i]) * Q[i]
            z = z - dt(h[i]) * Z[i]
        s = dot(q, q)
        rho = dot(r, q)
        if not (s > 0) or not np.isfinite(s):
            return x, np.array(hist), False, True
        alpha = rho / s
        x = x + dt(alpha) * z
        r = r - dt(alpha) * q
        rn = np.sqrt(dot(r, r))
        hist.append(rn)
        Z.append(z), Q.append(q), S.append(s)
        if rn <= tol * h0:
            return x, np.array(hist), True, False
    return x, np.array(hist), False, False


def dot_reversed(a, b):
    """the same products summed from the other end (np.dot's blocked order on the reversed arrays)"""
    return float(np.dot(a.ravel()[::-1].astype(np.float64), b.ravel()[::-1].astype(np.float64)))


def cycle_preconditioner(h):
    """M of a reference hierarchy h (galerkin_ref / line_ref / wcycle_ref): r -> one cycle from zero"""
    def M(r):
        return h.vcycle(h.L, np.zeros_like(r), r)
    return M


def upwind_stencil(L, a=(1.0, 0.5), peclet=1.0, dtype=np.float64):
    """(c, n, s, w, e) of first-order upwind convection-diffusion  -eps Lap u + a . grad u  on level L, scaled by h^2:
    h = 2^-L, eps = h |a|_max / Pe (cell Peclet number Pe);
        w = -eps - h max(a_x, 0)     e = -eps - h max(-a_x, 0)
        n = -eps - h max(a_y, 0)     s = -eps - h max(-a_y, 0)       c = -(n + s + w + e)
    (n is the neighbour in row i - 1, the side y decreases towards).  a = (a_x, a_y): two numbers, or two n x n arrays
    for a velocity given per point."""
    n_ = (1 << L) - 1
    h = 2.0 ** -L
    ax = np.broadcast_to(np.asarray(a[0], dtype=np.float64), (n_, n_))
    ay = np.broadcast_to(np.asarray(a[1], dtype=np.float64), (n_, n_))
    eps = h * max(float(np.max(np.abs(ax))), float(np.max(np.abs(ay)))) / peclet
    w = -eps - h * np.maximum(ax, 0.0)
    e = -eps - h * np.maximum(-ax, 0.0)
    n = -eps - h * np.maximum(ay, 0.0)
    s = -eps - h * np.maximum(-ay, 0.0)
    c = -(n + s + w + e)
    return [np.ascontiguousarray(v, dtype=dtype) for v in (c, n, s, w, e)]


def recirculating_velocity(L):
    """a = (sin(pi x) cos(pi y), -cos(pi x) sin(pi y)) on the interior points of level L: one divergence-free cell"""
    n_ = (1 << L) - 1
    t = np.arange(1, n_ + 1) * 2.0 ** -L
    X, Y = np.meshgrid(t, t)
    return np.sin(np.pi * X) * np.cos(np.pi * Y), -np.cos(np.pi * X) * np.sin(np.pi * Y)
