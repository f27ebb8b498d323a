"""numpy statement of mgx_solve_pcg (include/mgx.h): conjugate gradients on the finest level, preconditioned by
one oracle V-cycle from zero, with the Polak-Ribiere beta - the steps of the device in the same order.

Vectors are kept in the handle's working type (float64 or float32); dots are accumulated in float64 and the
scalars (rho, delta, gamma, alpha, beta) are float64, rounded to the working type once where they are applied."""
import numpy as np


def contrast_coefficient(L, contrast):
    """piecewise-constant nodal coefficient: 16 x 16 blocks of 1 or `contrast` (seeded), (N + 1)^2 nodes"""
    N = 1 << L
    rng = np.random.default_rng(1)
    blk = np.where(rng.random((N // 16 + 1, N // 16 + 1)) < 0.5, 1.0, contrast)
    return np.kron(blk, np.ones((16, 16)))[: N + 1, : N + 1].copy()


def oracle_solver(po, cfg, a_nodes=None):
    """the oracle hierarchy mirroring a device configuration.  An exact bottom solve of the Poisson hierarchy uses
    the oracle's sine-transform mode (the device's direct method in the device's operation order) in both
    precisions: the Cholesky solve differs from it by ~6e-15 relative, and PCG amplifies a difference in z by the
    residual reduction of every iteration (1e-9 relative after three RB-GS iterations)."""
    c = dict(cfg)
    if c.get("bottom", 0) == 0 and c.get("op", 0) == 0:
        c["bottom"] = po.BOTTOM_DST
    s = po.Solver(**c)
    if a_nodes is not None:
        s.set_coefficient(a_nodes)
    return s


class Operator:
    """A of the finest level: the constant five-point stencil (coef None) or the five arrays (c, n, s, w, e) of
    po.stencil_from_nodes, in the summation order of the device kernels"""

    def __init__(self, coef=None, dtype=np.float64):
        self.dtype = dtype
        self.coef = None if coef is None else [np.asarray(x, dtype=dtype) for x in coef]

    def __call__(self, u):
        P = np.pad(u, 1)
        up, dn, lf, rt = P[:-2, 1:-1], P[2:, 1:-1], P[1:-1, :-2], P[1:-1, 2:]
        if self.coef is None:
            return -(((up + lf) + rt) + dn) + self.dtype(4) * u
        c, n, s, w, e = self.coef
        acc = n * up
        acc = acc + w * lf
        acc = acc + c * u
        acc = acc + e * rt
        return acc + s * dn


def dot(a, b):
    return float(np.dot(a.ravel().astype(np.float64), b.ravel().astype(np.float64)))


def pcg(A, M, b, x0, tol=1e-8, max_iters=100):
    """A: callable u -> A u;  M: callable r -> one V-cycle from zero for A z = r.
    Returns (x, history, converged, breakdown)."""
    dt = A.dtype
    x = np.array(x0, dtype=dt, copy=True)
    b = np.asarray(b, dtype=dt)
    r = b - A(x)
    h0 = np.sqrt(dot(r, r))
    hist = [h0]
    if h0 <= tol * h0 or max_iters == 0:
        return x, np.array(hist), h0 <= tol * h0, False
    z = M(r)
    rho = dot(r, z)
    p = z
    for k in range(max_iters):
        q = A(p)
        delta = dot(p, q)
        if not (delta > 0) or not np.isfinite(delta):
            return x, np.array(hist), False, True
        alpha = rho / delta
        x = x + dt(alpha) * p
        r = r - dt(alpha) * q
        rn = np.sqrt(dot(r, r))
        hist.append(rn)
        if rn <= tol * h0:
            return x, np.array(hist), True, False
        if k + 1 == max_iters:
            break
        z = M(r)
        rho_new = dot(r, z)
        gamma = dot(z, q)
        beta = -alpha * gamma / rho
        p = z + dt(beta) * p
        rho = rho_new
    return x, np.array(hist), False, False


def run(po, cfg, b, u0=None, a_nodes=None, tol=1e-8, max_iters=100):
    """pcg() with the oracle V-cycle of `cfg` as M and the matching operator; b, u0 in float64 (cast to the
    working type of cfg['dtype'])."""
    L = cfg["finest_level"]
    dt = np.float64 if cfg.get("dtype", 1) == 1 else np.float32
    s = oracle_solver(po, cfg, a_nodes)
    coef = None if a_nodes is None else po.stencil_from_nodes(a_nodes, L, L)
    A = Operator(coef, dt)
    zeros = np.zeros_like(np.asarray(b, dtype=dt))

    def M(r):
        return s.vcycle(L, zeros, r)

    x0 = zeros if u0 is None else np.asarray(u0, dtype=dt)
    try:
        return pcg(A, M, np.asarray(b, dtype=dt), x0, tol=tol, max_iters=max_iters)
    finally:
        s.close()


def true_residual(b, x, a_nodes=None, L=None, po=None):
    """||b - A x|| in float64"""
    coef = None if a_nodes is None else po.stencil_from_nodes(a_nodes, L, L)
    A = Operator(coef, np.float64)
    r = np.asarray(b, dtype=np.float64) - A(np.asarray(x, dtype=np.float64))
    return float(np.sqrt(np.dot(r.ravel(), r.ravel())))
