"""GPU tests of mgx_newton and mgx_time_newton_pass (include/mgx.h, csrc/mgx_newton.hpp, csrc/mgx_newton_host.hpp)
against the numpy statement of tests/newton_ref.py, which tests/test_newton_cpu.py pins against mathematics.

Everything is bit for bit: the pass (its right-hand side through the timing entry's R, its d through mgx_get_reaction,
its norm against mgx_residual_norm of (U = 0, B = b)), and whole Newton iterations against the host composition
{pass in numpy, mgx_set_reaction, mgx_build_galerkin_transfer, mgx_set_rhs, zero guess, the same solver call,
mgx_get_solution, u + lam de in numpy, mgx_residual_norm} on the same handle.

Shapes: a wave covers 62 output lanes, 124 columns in double and 248 in float, so the pass runs at L = 4 (one strip, most
points next to the ring) and at L = 8 in double / L = 9 in float (more than one strip)."""
import ctypes as C

import numpy as np
import pytest

import galerkin_ref as gr
import newton_ref as nf
import theta_ref as tr
from test_gpu_galerkin import assert_same, handle, np_dtype
from test_gpu_theta import JACOBI, SGS, finest_slots, rand, run_solver, set_operator, stats_tuple, whole_level

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 5                      # MGX_ERR_INVALID, MGX_ERR_STATE
BILINEAR, OPERATOR = 0, 1                  # MGX_TRANSFER_*
CUBIC, ALLEN_CAHN = (0.0, 0.0, 1.0), (-1.0, 0.0, 1.0)


def base_operator(mg, kind, L):
    """A0 as the device stores it, nine arrays (after a build)"""
    st = finest_slots(mg, kind, L)
    return gr.nine(st) if kind == "five" else st


def device_norm(mg, L, b):
    """||b||_2 as the device sums it: mgx_residual_norm of (U = 0, B = b)"""
    mg.set_rhs(b)
    mg.set_guess(np.zeros_like(b))
    return mg.residual_norm()


def host_newton(pkg, mg, L, A0, kap, f, p, u0, transfer, solver, lin_tol, lin_iters, restart, tol, max_newton, max_backtracks):
    """the Newton loop as the caller composes it on the same handle (newton_ref.newton around the device's linear solver
    and the device's norm)"""
    def solve(S9, b, d, k):
        mg.set_reaction(d)
        mg.build_galerkin(transfer)
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        st, h = run_solver(mg, solver, lin_tol, lin_iters, restart)
        return mg.get_solution(), stats_tuple(st)

    return nf.newton(A0, kap, f, p, u0, solve, tol, max_newton, max_backtracks, norm=lambda b: device_norm(mg, L, b))


def device_newton(mg, kap, f, p, u0, **kw):
    mg.set_rhs(f)
    mg.set_guess(u0)
    return mg.newton(kap, p=p, **kw)


def assert_newton_same(pkg, mg, L, got, want, f, what):
    ns, hist, lin, lam = got
    assert np.array_equal(hist, want["hist"]), (what, hist, want["hist"])
    assert np.array_equal(lam, want["lam"]), (what, lam, want["lam"])
    assert ns.iterations == len(want["lam"]) and ns.history_len == len(want["hist"]) and ns.backtracks == want["backtracks"], what
    assert ns.converged == int(want["converged"]) and ns.initial_residual == want["hist"][0] and ns.final_residual == want["hist"][-1], what
    assert [stats_tuple(s) for s in lin] == want["lin"], what
    assert ns.linear_iterations == sum(s[0] for s in want["lin"]), what
    assert_same(mg.get_solution(), want["u"], (what, "U"))
    assert_same(mg.get_level(L, pkg.VEC_B), f, (what, "B is the caller's f"))


# ---- 1. the pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["five", "nine"])
@pytest.mark.parametrize("dtype, L, Lc", [(1, 4, 3), (1, 8, 5), (0, 4, 3), (0, 9, 5)])
def test_the_pass_is_bit_identical_to_the_reference(pkg, dtype, L, Lc, kind):
    """kappa small against the operator (a nearly linear problem), so that the full step of max_backtracks = 0 passes the
    test; the linear solve runs to 1e-10 (1e-5 in float)"""
    dt = np_dtype(dtype)
    N = 1 << L
    kap, f, u0 = rand(L, 71, dt, 0.05, 0.2), rand(L, 72, dt), rand(L, 73, dt)
    p = (0.25, -0.5, 1.0)
    lin = dict(solver="solve", lin_tol=1e-10 if dtype == 1 else 1e-5, lin_max_iters=40)

    def rings_clean(what):
        for which in (pkg.VEC_U, pkg.VEC_B):
            full = whole_level(pkg, mg, L, which).copy()
            full[1:N, 1:N] = 0
            assert not full.any(), (what, which, "ring or padding written")

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        set_operator(mg, kind, L)
        mg.build_galerkin()
        A0 = base_operator(mg, kind, L)
        v, b0, d0 = nf.newton_pass(A0, kap, f, p, u0)
        r0 = device_norm(mg, L, b0)
        # the first evaluation: max_newton = 0
        ns, hist, _, _ = device_newton(mg, kap, f, p, u0, max_newton=0, tol=0.0, **lin)
        assert ns.iterations == 0 and ns.history_len == 1 and list(hist) == [r0] and ns.converged == (1 if r0 == 0.0 else 0)
        assert np.array_equal(mg.get_solution(), u0) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        rings_clean("first evaluation")
        with pytest.raises(pkg.MgxError, match="no zero-order term"):
            mg.reaction()
        # ... and its right-hand side, through the timing entry's R
        mg.time_newton_pass(0, repeats=1)
        assert_same(mg.get_level(L, pkg.VEC_R), b0, (kind, "b of the first evaluation"))
        # a step: max_newton = 1, max_backtracks = 0
        ns, hist, lstats, lam = device_newton(mg, kap, f, p, u0, max_newton=1, max_backtracks=0, tol=0.0, **lin)
        assert ns.iterations == 1 and ns.backtracks == 0 and list(lam) == [1.0] and hist[0] == r0, (ns.iterations, hist)
        u1 = mg.get_solution()
        assert np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        rings_clean("one step")
        assert_same(mg.reaction(), d0, (kind, "d of the first evaluation"))
        # the trial's right-hand side: the timing entry forms un + 1 * U from the iterate un = u1 and de = U = u1
        mg.time_newton_pass(1, repeats=1)
        assert_same(mg.get_level(L, pkg.VEC_R), nf.newton_pass(A0, kap, f, p, u1, u1, 1.0)[1], (kind, "b of a trial"))
        assert np.array_equal(mg.get_solution(), u1) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        # the host composition of that step on the same handle
        want = host_newton(pkg, mg, L, A0, kap, f, p, u0, BILINEAR, "solve", lin["lin_tol"], 40, 3, 0.0, 1, 0)
        assert not want["failed"] and want["lin"] == [stats_tuple(lstats[0])]
        assert np.array_equal(hist, want["hist"]), (hist, want["hist"])
        assert_same(u1, want["u"], (kind, "U after one step"))


# ---- 2. three steps against the host composition ---------------------------------------------------------------------------
def problem(name, L, dt):
    """(operator kind's coefficient call, kappa, f, p, u0).  cubic: phi = u^3 on a contrast-10 operator, the Jacobian
    A0 + 3 kap u^2 >= A0.  allen-cahn: phi = u^3 - u on the Poisson operator with kap = 0.5 lambda_min, the Jacobian
    A0 + kap (3 u^2 - 1) >= A0 - 0.5 lambda_min is positive definite"""
    n = (1 << L) - 1
    if name == "cubic":
        return rand(L, 81, dt, 0.5, 2.0), rand(L, 82, dt), CUBIC, rand(L, 83, dt)
    u0 = (5.0 * tr.sine_mode(L, 1, 1)[0] + rand(L, 85, dt)).astype(dt)     # (large and smooth: the cubic term matters for several steps)
    return np.full((n, n), 0.5 * nf.poisson_lambda_min(L), dtype=dt), (0.01 * rand(L, 84, dt)).astype(dt), ALLEN_CAHN, u0


def composition_case(pkg, cfg, kind, name, solver, transfer, lin_tol, cycle=None):
    L, Lc = cfg["finest"], cfg["coarsest"]
    dt = np_dtype(cfg.get("dtype", 1))
    kap, f, p, u0 = problem(name, L, dt)
    kw = {k: v for k, v in cfg.items() if k not in ("finest", "coarsest")}
    opts = dict(solver=solver, lin_tol=lin_tol, lin_max_iters=40, restart=3, tol=0.0, max_newton=3, max_backtracks=6)
    with handle(pkg, L, Lc, **kw) as mg:
        if cycle is not None:
            mg.set_cycle(cycle)
        if name == "cubic":
            set_operator(mg, kind, L)
        else:
            mg.set_coefficient(np.ones(((1 << L) + 1,) * 2))
        mg.build_galerkin(transfer)
        A0 = base_operator(mg, kind, L)
        got = device_newton(mg, kap, f, p, u0, **opts)
        u_dev = mg.get_solution()
        assert got[0].iterations == 3, (got[0].iterations, pkg.lib().mgx_last_error(mg._h).decode())
        assert_same(mg.get_level(L, pkg.VEC_B), f, "B is the caller's f")
        want = host_newton(pkg, mg, L, A0, kap, f, p, u0, transfer, solver, lin_tol, 40, 3, 0.0, 3, 6)
        mg.set_guess(u_dev)
        mg.set_rhs(f)
        assert_newton_same(pkg, mg, L, got, want, f, (kind, name, solver, transfer))
        assert want["hist"][-1] < want["hist"][0]
        # once more on the handle the composition left (a term is set: it is replaced), the same bits
        again = device_newton(mg, kap, f, p, u0, **opts)
        assert_newton_same(pkg, mg, L, again, want, f, (kind, name, solver, transfer, "second call"))
        assert_same(mg.reaction(), want["ds"][-1], "d of the last linear solve")


@pytest.mark.parametrize("solver", ["solve", "gcr", "refine_gcr"])
@pytest.mark.parametrize("kind, name, transfer", [("five", "cubic", BILINEAR), ("nine", "cubic", OPERATOR), ("five", "allen-cahn", OPERATOR)])
def test_three_steps_are_the_host_composition_jacobi(pkg, kind, name, transfer, solver):
    composition_case(pkg, dict(finest=6, coarsest=3, **JACOBI), kind, name, solver, transfer, 1e-8)


@pytest.mark.parametrize("kind, name, solver, transfer", [("nine", "cubic", "gcr", BILINEAR), ("five", "allen-cahn", "solve", BILINEAR),
                                                          ("five", "cubic", "refine_gcr", OPERATOR)])
def test_three_steps_are_the_host_composition_colour_sgs(pkg, kind, name, solver, transfer):
    composition_case(pkg, dict(finest=6, coarsest=3, **SGS), kind, name, solver, transfer, 1e-8)


@pytest.mark.parametrize("solver, name", [("solve", "allen-cahn"), ("gcr", "cubic")])
def test_three_steps_with_w_cycles(pkg, solver, name):
    composition_case(pkg, dict(finest=6, coarsest=3, **JACOBI), "five", name, solver, BILINEAR, 1e-8, cycle=pkg.CYCLE_W)


@pytest.mark.parametrize("kind, name, solver, transfer", [("five", "cubic", "solve", BILINEAR), ("five", "allen-cahn", "gcr", OPERATOR)])
def test_three_steps_in_float(pkg, kind, name, solver, transfer):
    composition_case(pkg, dict(finest=6, coarsest=3, dtype=0, **JACOBI), kind, name, solver, transfer, 1e-4)


# ---- 3. the line search ------------------------------------------------------------------------------------------------------
def backtracking_handle(pkg, L, Lc, dtype=1):
    mg = handle(pkg, L, Lc, dtype=dtype, **JACOBI)
    mg.set_coefficient(np.ones(((1 << L) + 1,) * 2))
    mg.build_galerkin()
    return mg


@pytest.mark.parametrize("L, Lc", [(5, 3), (6, 3)])
def test_the_backtracking_input_backtracks_on_the_device(pkg, L, Lc):
    """the input tests/test_newton_cpu.py pins (the first full step overshoots); V(2,2) Jacobi reduces the first system by
    about 0.18 per cycle, so lin_tol = 1e-8 is reached within 20 cycles"""
    A0n, kap, f, p, u0 = nf.backtracking_input(L)
    opts = dict(solver="solve", lin_tol=1e-8, lin_max_iters=20, tol=1e-10, max_newton=10, max_backtracks=8)
    with backtracking_handle(pkg, L, Lc) as mg:
        A0 = base_operator(mg, "five", L)
        assert all(np.array_equal(x, y) for x, y in zip(A0, A0n))
        got = device_newton(mg, kap, f, p, u0, **opts)
        ns, hist, lin, lam = got
        assert ns.converged == 1 and ns.backtracks >= 1 and lam[0] < 1.0 and (lam[1:] == 1.0).all(), (ns.backtracks, lam, hist)
        assert all(s.converged == 1 for s in lin)
        u_dev = mg.get_solution()
        want = host_newton(pkg, mg, L, A0, kap, f, p, u0, BILINEAR, "solve", 1e-8, 20, 3, 1e-10, 10, 8)
        mg.set_guess(u_dev)
        mg.set_rhs(f)
        assert_newton_same(pkg, mg, L, got, want, f, ("backtracking", L))


def test_a_failed_line_search_ends_the_call(pkg):
    L, Lc = 5, 3
    A0n, kap, f, p, u0 = nf.backtracking_input(L)
    with backtracking_handle(pkg, L, Lc) as mg:
        ns, hist, lin, lam = device_newton(mg, kap, f, p, u0, solver="solve", lin_tol=1e-8, lin_max_iters=20, tol=1e-10, max_newton=10,
                                           max_backtracks=2)                  # (MGX_OK: the binding did not raise)
        msg = pkg.lib().mgx_last_error(mg._h).decode()
        assert ns.converged == 0 and ns.iterations == 0 and ns.history_len == 1 and ns.backtracks == 3 and len(lam) == 0
        assert len(lin) == 1 and lin[0].converged == 1 and ns.linear_iterations == lin[0].cycles
        assert "mgx_newton: step 0" in msg and "line search failed" in msg and "0.25" in msg and repr(float(hist[0]))[:12] in msg, msg
        assert np.array_equal(mg.get_solution(), u0) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        # the operator is the Jacobian of the step that failed, built
        assert_same(mg.reaction(), nf.newton_pass(A0n, kap, f, p, u0)[2], "d of the failed step")
        assert mg.solve(tol=1e-8, max_cycles=20)[0].converged == 1


# ---- 4. state ------------------------------------------------------------------------------------------------------------------
def test_zero_iterations_touch_nothing(pkg):
    L, Lc, dt = 6, 3, np.float64
    kap, f, p, u0 = problem("cubic", L, dt)
    d = rand(L, 91, dt, 0.5, 2.0)
    with handle(pkg, L, Lc) as mg:
        set_operator(mg, "five", L)
        mg.build_galerkin(OPERATOR)
        mg.set_rhs(f)
        mg.set_guess(u0)
        mg.solve(tol=0.0, max_cycles=2)                       # (captures graphs)
        graphs = mg.graphs_cached()
        centre = mg.get_stencil(L, 0)
        for kw in (dict(max_newton=0, tol=0.0), dict(max_newton=5, tol=1.0)):       # (hist[0] <= 1.0 * hist[0])
            ns, hist, lin, lam = device_newton(mg, kap, f, p, u0, **kw)
            assert ns.iterations == 0 and ns.history_len == 1 and len(lin) == 0 and ns.converged == (1 if kw["tol"] else 0)
            assert mg.graphs_cached() == graphs and mg.transfer == OPERATOR
            assert np.array_equal(mg.get_stencil(L, 0), centre)
            with pytest.raises(pkg.MgxError, match="no zero-order term"):
                mg.reaction()
            assert np.array_equal(mg.get_solution(), u0) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        # ... and a term that is set stays, with its hierarchy; F is formed with A0, not with A0 + diag(d)
        mg.set_reaction(d)
        mg.build_galerkin(OPERATOR)
        shifted = mg.get_stencil(L, 0)
        r0 = hist[0]
        ns, hist, _, _ = device_newton(mg, kap, f, p, u0, max_newton=0, tol=0.0)
        assert hist[0] == r0
        assert np.array_equal(mg.reaction(), d) and np.array_equal(mg.get_stencil(L, 0), shifted)
        assert mg.solve(tol=1e-8, max_cycles=30)[0].converged == 1          # (still built)


def test_the_state_after_the_call_is_a_set_reaction_and_a_build(pkg):
    L, Lc, dt = 6, 3, np.float64
    kap, f, p, u0 = problem("cubic", L, dt)
    b = rand(L, 92, dt)

    def bits(mg):
        mg.set_rhs(b)
        mg.set_guess(u0)
        st, h = mg.solve(tol=0.0, max_cycles=3)
        return h, mg.get_solution()

    with handle(pkg, L, Lc) as mg:
        set_operator(mg, "five", L)
        mg.build_galerkin()
        A0 = base_operator(mg, "five", L)
        before = bits(mg)
        mg.set_reaction(rand(L, 93, dt, 5.0, 9.0))            # a caller's earlier term: replaced
        mg.build_galerkin()
        ns, hist, lin, lam = device_newton(mg, kap, f, p, u0, max_newton=1, tol=0.0)
        assert ns.iterations == 1
        assert_same(mg.reaction(), nf.newton_pass(A0, kap, f, p, u0)[2], "d_0")
        assert_same(mg.get_stencil(L, 0), A0[0] + mg.reaction(), "centre")
        shifted = bits(mg)                                    # (the hierarchy is built)
        assert not np.array_equal(shifted[0], before[0])
        mg.set_reaction(None)
        mg.build_galerkin()
        after = bits(mg)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def raw_newton(pkg, mg, kap, count=None, **kw):
    B = pkg.binding
    o = dict(p1=0.0, p2=0.0, p3=1.0, solver=0, lin_tol=1e-8, lin_max_iters=20, restart=3, tol=1e-10, max_newton=3, max_backtracks=4)
    o.update(kw)
    opt = B.NewtonOpts(**o)
    return pkg.lib().mgx_newton(mg._h, C.byref(opt), None if kap is None else kap.ctypes.data, kap.size if count is None else count,
                                None, None, None, None, 0)


def test_refused_handles(pkg, po):
    L, Lc = 7, 4
    kap = np.ones(((1 << L) - 1,) * 2)
    small = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, schedule=0)
    b = po.rhs_sine(L)
    lib = pkg.lib()
    ms = C.c_double()

    def all_refuse(mg, word):
        for i, call in enumerate((lambda: raw_newton(pkg, mg, kap), lambda: lib.mgx_time_newton_pass(mg._h, 0, 1, C.byref(ms)))):
            assert call() == STATE, (word, i)
            assert word in lib.mgx_last_error(mg._h).decode(), (i, lib.mgx_last_error(mg._h).decode())

    with pkg.Multigrid(**small) as mg:
        all_refuse(mg, "POISSON")
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=20)[0].converged == 1
    with pkg.Multigrid(n_gpus=2, devices=[0, 0], cut_level=5, **small) as mg:
        all_refuse(mg, "multi-GPU")
        assert raw_newton(pkg, mg, kap, count=3) == INVALID       # (the argument checks come first)
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=20)[0].converged == 1
    with pkg.Multigrid(op=pkg.OPERATOR_STENCIL5, **small) as mg:
        all_refuse(mg, "STENCIL5")
        mg.set_coefficient(np.ones(((1 << L) + 1,) * 2))
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=30)[0].converged == 1


@pytest.mark.parametrize("dtype", [1, 0])
def test_refused_calls_leave_the_handle_usable(pkg, dtype):
    dt = np_dtype(dtype)
    L, Lc = 6, 3
    n = (1 << L) - 1
    lib = pkg.lib()
    kap, f, p, u0 = problem("cubic", L, dt)
    lin_tol = 1e-8 if dtype == 1 else 1e-4
    ms = C.c_double(-1.0)
    nan, inf = float("nan"), float("inf")

    def expect(code, word, call):
        assert call() == code, word
        assert word in lib.mgx_last_error(mg._h).decode(), (word, lib.mgx_last_error(mg._h).decode())

    def reference_bits(m):
        ns, hist, lin, lam = device_newton(m, kap, f, p, u0, solver="gcr", lin_tol=lin_tol, lin_max_iters=20, restart=3, tol=0.0, max_newton=2)
        return ns.iterations, hist, [stats_tuple(s) for s in lin], lam, m.get_solution()

    def same(x, y):
        return x[0] == y[0] == 2 and np.array_equal(x[1], y[1]) and x[2] == y[2] and np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4])

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        set_operator(mg, "five", L)
        mg.build_galerkin()
        want = reference_bits(mg)
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        bad = lambda **kw: (lambda: raw_newton(pkg, mg, kap, **kw))
        # before the finest operator is set, and before the build
        expect(STATE, "finest operator not set", bad())
        expect(STATE, "finest operator not set", lambda: lib.mgx_time_newton_pass(mg._h, 0, 1, C.byref(ms)))
        set_operator(mg, "five", L)
        expect(STATE, "not built", bad())
        expect(STATE, "mgx_newton first", lambda: lib.mgx_time_newton_pass(mg._h, 0, 1, C.byref(ms)))
        mg.build_galerkin()
        expect(STATE, "mgx_newton first", lambda: lib.mgx_time_newton_pass(mg._h, 1, 1, C.byref(ms)))
        assert ms.value == -1.0
        # NULL opt
        assert lib.mgx_newton(mg._h, None, kap.ctypes.data, kap.size, None, None, None, None, 0) == INVALID
        # every INVALID, each with everything after it in the documented order wrong as well
        later = dict()
        chain = [("kappa", dict(), True), ("max_backtracks", dict(max_backtracks=31), False), ("max_newton", dict(max_newton=-1), False),
                 ("tol", dict(tol=nan), False), ("restart", dict(solver=1, restart=9), False), ("lin_max_iters", dict(lin_max_iters=-1), False),
                 ("lin_tol", dict(lin_tol=-1.0), False), ("solver", dict(solver=3), False), ("finite", dict(p2=inf), False)]
        expect(INVALID, "n*n", lambda: raw_newton(pkg, mg, kap, count=n * n - 1))
        null_kappa = False
        for word, kw, is_null in chain:                       # from the last check to the first: each one shadows the earlier ones
            later.update(kw)
            null_kappa = null_kappa or is_null
            expect(INVALID, word, lambda: raw_newton(pkg, mg, None if null_kappa else kap, count=n * n - 1, **later))
        for kw, word in ((dict(p1=nan), "finite"), (dict(p3=-inf), "finite"), (dict(solver=-1), "solver"), (dict(lin_tol=nan), "lin_tol"),
                         (dict(solver=2, restart=0), "restart"), (dict(tol=-1.0), "tol"), (dict(max_backtracks=-1), "max_backtracks")):
            expect(INVALID, word, bad(**kw))
        assert raw_newton(pkg, mg, kap, solver=0, restart=0, max_newton=0) == 0             # (restart is not looked at)
        expect(INVALID, "n*n", lambda: raw_newton(pkg, mg, kap, count=n * n + 1))
        if dtype == 0:
            expect(STATE, "F64", bad(solver=pkg.STEP_REFINE_GCR))
        for step, repeats, out in ((2, 1, C.byref(ms)), (-1, 1, C.byref(ms)), (0, 0, C.byref(ms)), (0, 1, None)):
            expect(INVALID, "mgx_time_newton_pass", lambda: lib.mgx_time_newton_pass(mg._h, step, repeats, out))
        assert ms.value == -1.0
        assert same(reference_bits(mg), want)


# ---- 6. the timing entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["five", "nine"])
def test_timing_the_pass_leaves_u_b_and_the_operator(pkg, kind):
    L, Lc, dt = 8, 5, np.float64
    kap, f, p, u0 = problem("cubic", L, dt)
    with handle(pkg, L, Lc) as mg:
        set_operator(mg, kind, L)
        mg.build_galerkin()
        ns, hist, lin, lam = device_newton(mg, kap, f, p, u0, max_newton=1, tol=0.0, lin_max_iters=10)
        u, d, centre = mg.get_solution(), mg.reaction(), finest_slots(mg, kind, L)[0]
        graphs = mg.graphs_cached()
        for step in (0, 1):
            ms = mg.time_newton_pass(step, repeats=5)
            assert np.isfinite(ms) and ms > 0.0, (step, ms)
            assert np.array_equal(mg.get_solution(), u) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
            assert np.array_equal(mg.reaction(), d) and np.array_equal(finest_slots(mg, kind, L)[0], centre) and mg.graphs_cached() == graphs
        # the next call starts from the iterate it was left with: the same bits as a fresh second step
        got = device_newton(mg, kap, f, p, u, max_newton=1, tol=0.0, lin_max_iters=10)
        assert got[1][0] == hist[1]
