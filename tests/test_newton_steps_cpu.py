"""CPU checks of tests/newton_steps_ref.py - the numpy statement tests/test_gpu_newton_steps.py holds the device to -
against mathematics (a dense solve zeroes G, kappa = 0 is the linear theta step, the schemes' orders in time), of the
Euler pass's reads, and of the new entry points' argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import galerkin_ref as gr
import newton_ref as nf
import newton_steps_ref as ns
import theta_ref as tr

INVALID = 1                                # MGX_ERR_INVALID
ALLEN_CAHN = (-1.0, 0.0, 1.0)


def operator(kind, L, seed):
    """a random operator, diagonally dominant: five-point (through gr.nine) or nine-point"""
    n = (1 << L) - 1
    rng = np.random.default_rng(seed)
    rand = lambda lo, hi: rng.uniform(lo, hi, (n, n))
    if kind == "five":
        return gr.nine([rand(3.5, 5.0)] + [rand(-0.8, -0.2) for _ in range(4)])
    return [rand(7.0, 9.0)] + [rand(-0.8, -0.2) for _ in range(8)]


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("kind", ["five", "nine"])
@pytest.mark.parametrize("L", [4, 5])
def test_a_step_with_dense_solves_zeroes_g(L, kind, theta):
    """phi = u^3 - u + 0.3 u^2 with kap <= 0.5 and dm >= 1: the Jacobian A0 + dm + kap phi'(v) >= A0 + dm - 0.53 kap is
    positive definite, Newton with newton_ref.direct_solve converges quadratically, and ||G(u+)|| recomputed in float64
    from the sparse matrix (another summation order) is at most 1e-12 of ||G(u)||"""
    n = (1 << L) - 1
    rng = np.random.default_rng(10 * L + (kind == "nine"))
    A0 = operator(kind, L, 3)
    kap, dm, g, u0 = rng.uniform(0.1, 0.5, (n, n)), rng.uniform(1.0, 3.0, (n, n)), rng.uniform(-1, 1, (n, n)), rng.uniform(-2, 2, (n, n))
    p = (-1.0, 0.3, 1.0)
    (o,) = ns.steps(A0, kap, dm, g, p, u0, theta, 1, nf.direct_solve, 1e-14, 20, 8)
    before, after = ns.g_norm(A0, kap, dm, g, p, u0, u0, theta), ns.g_norm(A0, kap, dm, g, p, u0, o["u"], theta)
    print(L, kind, theta, "||G(u)|| =", before, "||G(u+)|| =", after, "Newton steps:", len(o["lam"]))
    assert abs(before - o["hist"][0]) <= 1e-12 * before     # (the reference's own first norm is the independent one but for rounding)
    assert after <= 1e-12 * before, (after, before)


@pytest.mark.parametrize("theta", [1.0, 0.5, 0.75])
def test_kappa_zero_is_the_linear_theta_step(theta):
    """kap = 0: G is linear, one full Newton step with a dense solve is theta_ref's step on S = A0 + diag(dm).  The two
    right-hand sides differ in their association only - c1 m - c0 (S u) against m - c0 (A0 u), with S u = A0 u + dm u and
    c1 = 1 + c0 - a few roundings of terms of size (1 + c0) |dm u| + c0 |A0 u|, and the solves (cond(S) <= 13 / 1) carry
    them over: 64 eps times the magnitude of the vector bounds both"""
    L = 4
    n = (1 << L) - 1
    rng = np.random.default_rng(12)
    A0 = operator("nine", L, 4)
    dm, g, u0 = rng.uniform(1.0, 3.0, (n, n)), rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    kap = np.zeros((n, n))
    S = tr.shift(A0, dm)
    eps = np.finfo(np.float64).eps
    c0 = (1.0 - theta) / theta
    r = ns.rhs_pass(A0, kap, dm, g, ALLEN_CAHN, u0, theta)
    b = tr.rhs_pass(None if theta == 1.0 else tr.apply(S, u0), u0, dm, g, theta)
    scale = np.max((1.0 + c0) * np.abs(dm * u0) + c0 * np.abs(tr.apply(A0, u0)) + np.abs(g))
    assert np.max(np.abs(r - b)) <= 8 * eps * scale, np.max(np.abs(r - b)) / (eps * scale)
    (o,) = ns.steps(A0, kap, dm, g, ALLEN_CAHN, u0, theta, 1, nf.direct_solve, 1e-12, 3, 0)
    (want,) = tr.steps(S, dm, u0, g, theta, 1, tr.dense_solver(S))
    assert len(o["lam"]) == 1 and o["converged"] and not np.asarray(o["ds"][0] - dm).any()
    assert np.max(np.abs(o["u"] - want)) <= 64 * eps * max(scale, np.max(np.abs(want))), np.max(np.abs(o["u"] - want))


def allen_cahn_end(theta, dt, t_end, L=4):
    """u(t_end) of u_t = -A0 u - kap (u^3 - u) (rho = 1, h = 1: time in stencil units) from a two-mode start, by theta
    steps of size dt with direct solves to 1e-13"""
    n = (1 << L) - 1
    A0 = tr.poisson9(L)
    kap = np.full((n, n), 0.05)
    u = 1.5 * tr.sine_mode(L, 1, 1)[0] + 0.5 * tr.sine_mode(L, 2, 3)[0]
    dm = np.full((n, n), 1.0 / (theta * dt))
    out = ns.steps(A0, kap, dm, None, ALLEN_CAHN, u, theta, int(round(t_end / dt)), nf.direct_solve, 1e-13, 30, 8)
    assert all(o["converged"] for o in out)
    return out[-1]["u"]


@pytest.mark.parametrize("theta, order", [(0.5, 2.0), (1.0, 1.0)])
def test_the_order_in_time(theta, order):
    """L = 4, Allen-Cahn with kap = 0.05 on the Poisson operator (lambda_min = 0.077), t_end = 4, dt = 1, 1/2, 1/4 against
    the reference's own Crank-Nicolson run at dt = 1/64 (its error is 1 / 256 of the Crank-Nicolson run at 1/4 and far less
    of the Euler runs').  Observed orders on the numpy reference alone, max-norm errors at t_end:
    theta = 1/2: errors 5.62e-3, 1.40e-3, 3.47e-4, orders 2.010 and 2.007;  theta = 1: errors 5.01e-2, 2.60e-2, 1.33e-2,
    orders 0.945 and 0.973.  The bound: within 0.25 of the scheme's order"""
    t_end = 4.0
    ref = allen_cahn_end(0.5, 1.0 / 64, t_end)
    err = [np.max(np.abs(allen_cahn_end(theta, dt, t_end) - ref)) for dt in (1.0, 0.5, 0.25)]
    orders = [np.log2(err[i] / err[i + 1]) for i in range(2)]
    print("theta =", theta, "errors:", err, "orders:", orders)
    for o in orders:
        assert abs(o - order) <= 0.25, (theta, err, orders)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_passes_operation_by_operation(dtype):
    """rhs_pass and mass_pass against the formulas written out per point in scalars of the working type, on a random
    nine-point operator"""
    L = 4
    n = (1 << L) - 1
    rng = np.random.default_rng(7)
    rand = lambda lo, hi: rng.uniform(lo, hi, (n, n)).astype(dtype)
    A0 = [rand(3.0, 5.0)] + [rand(-1.0, -0.2) for _ in range(8)]
    kap, dm, g, u, de, r = rand(0.1, 2.0), rand(0.5, 3.0), rand(-1.0, 1.0), rand(-1.0, 1.0), rand(-1.0, 1.0), rand(-1.0, 1.0)
    p = (-0.7, 0.3, 1.1)
    T = np.dtype(dtype).type
    p1, p2, p3, q2, q3 = T(p[0]), T(p[1]), T(p[2]), T(2.0 * p[1]), T(3.0 * p[2])
    points = ((0, 0), (3, 7), (n - 1, n - 1))

    def stencil(vv, i, j):
        P = np.pad(vv, 1)
        q = None
        for dy, dx in gr.ROW_MAJOR:
            term = A0[gr.SLOT[dy, dx]][i, j] * P[1 + i + dy, 1 + j + dx]
            q = term if q is None else q + term
        return q

    for theta in (1.0, 0.5, 0.75):
        c0 = T((1.0 - theta) / theta)
        for gg in (None, g):
            out = ns.rhs_pass(A0, kap, dm, gg, p, u, theta)
            assert out.dtype == np.dtype(dtype)
            for i, j in points:
                x = u[i, j]
                m = dm[i, j] * x
                want = m if theta == 1.0 else m - c0 * (stencil(u, i, j) + kap[i, j] * (((p3 * x + p2) * x + p1) * x))
                if gg is not None:
                    want = want + g[i, j]
                assert type(want) is T and out[i, j] == want, (theta, i, j)
    for lam in (None, 0.5):
        v, b, d = ns.mass_pass(A0, kap, dm, r, p, u, None if lam is None else de, lam)
        vv = u if lam is None else (u + T(lam) * de)
        assert np.array_equal(v, vv) and v.dtype == b.dtype == d.dtype == np.dtype(dtype)
        for i, j in points:
            x = vv[i, j]
            ph = ((p3 * x + p2) * x + p1) * x
            dp = (q3 * x + q2) * x + p1
            assert b[i, j] == r[i, j] - ((stencil(vv, i, j) + dm[i, j] * x) + kap[i, j] * ph), (lam, i, j)
            assert d[i, j] == dm[i, j] + kap[i, j] * dp, (lam, i, j)
    # without a mass term the pass is newton_ref's: dm = 0 adds q + 0 v = q and 0 + kap dp = kap dp (no -0 arises from x + 0)
    v0, b0, d0 = nf.newton_pass(A0, kap, r, p, u)
    v1, b1, d1 = ns.mass_pass(A0, kap, np.zeros((n, n), dtype=dtype), r, p, u)
    assert np.array_equal(b0, b1) and np.array_equal(d0, d1)


def test_the_euler_pass_reads_the_mass_and_the_time_level_only():
    """theta = 1 and g = None: NaN in the operator and in kappa does not reach r (the kernel's Euler instance reads no
    coefficient grid), r = dm u exactly, and -0 stays -0 (nothing is added when g is missing)"""
    L = 4
    n = (1 << L) - 1
    rng = np.random.default_rng(8)
    u, dm = rng.uniform(-1, 1, (n, n)), rng.uniform(0.5, 2, (n, n))
    u[2, 3] = -0.0
    nan = np.full((n, n), np.nan)
    r = ns.rhs_pass([nan] * 9, nan, dm, None, ALLEN_CAHN, u, 1.0)
    assert np.array_equal(r, dm * u) and np.signbit(r[2, 3])
    g = rng.uniform(-1, 1, (n, n))
    assert np.array_equal(ns.rhs_pass([nan] * 9, nan, dm, g, ALLEN_CAHN, u, 1.0), dm * u + g)
    assert np.isnan(ns.rhs_pass([nan] * 9, nan, dm, None, ALLEN_CAHN, u, 0.5)).all()        # (the other instance does read them)


def test_null_handles_are_refused_without_a_device(pkg):
    """NULL handle (with and without opt): MGX_ERR_INVALID, every output left alone"""
    lib = pkg.lib()
    B = pkg.binding
    opt = B.NewtonOpts(0.0, 0.0, 1.0, pkg.STEP_SOLVE, 1e-8, 10, 4, 1e-10, 5, 4)
    a = np.ones(9)
    st = (B.NewtonStats * 2)()
    for s in st:
        s.iterations = -7
    hist = np.full(12, -1.0)
    done = C.c_int(7)
    for o in (C.byref(opt), None):
        assert lib.mgx_newton_steps(None, o, 1.0, 2, a.ctypes.data, a.ctypes.data, None, a.size, C.byref(done), st,
                                    hist.ctypes.data_as(C.POINTER(C.c_double)), 6) == INVALID
    assert done.value == 7 and all(s.iterations == -7 for s in st) and (hist == -1.0).all()
    ms = C.c_double(-1.0)
    for which in (0, 1, 2):
        assert lib.mgx_time_newton_step_pass(None, which, 0.5, 1, C.byref(ms)) == INVALID and ms.value == -1.0
