"""GPU tests of mgx_newton_steps and mgx_time_newton_step_pass (include/mgx.h, csrc/mgx_newton.hpp,
csrc/mgx_newton_steps_host.hpp) against the numpy statement of tests/newton_steps_ref.py, which
tests/test_newton_steps_cpu.py pins against mathematics.

Everything but the physical check is bit for bit: the two passes (the step's r through B, the Newton pass's b through the
timing entry's R, its d through mgx_get_reaction, its norm against mgx_residual_norm of (U = 0, B = b)), and whole time
steps against the host composition {r in numpy; per Newton iteration the pass in numpy, mgx_set_reaction,
mgx_build_galerkin_transfer, mgx_set_rhs, zero guess, the same solver call, mgx_get_solution, u + lam de in numpy,
mgx_residual_norm} on the same handle.  Shapes: those of tests/test_gpu_newton.py (the same geometry)."""
import ctypes as C

import numpy as np
import pytest

import newton_ref as nf
import newton_steps_ref as ns
from test_gpu_galerkin import assert_same, handle, np_dtype
from test_gpu_newton import ALLEN_CAHN, BILINEAR, CUBIC, INVALID, OPERATOR, STATE, base_operator, device_norm, problem
from test_gpu_theta import JACOBI, SGS, finest_slots, rand, run_solver, set_operator, stats_tuple, whole_level

pytestmark = pytest.mark.gpu

NSTAT_FIELDS = ("iterations", "converged", "initial_residual", "final_residual", "linear_iterations", "backtracks", "history_len")   # (not seconds)


def nstats_tuple(st):
    return tuple(getattr(st, f) for f in NSTAT_FIELDS)


def host_steps(mg, L, A0, kap, dm, g, p, u0, theta, nsteps, transfer, solver, lin_tol, lin_iters, restart, tol, max_newton, max_backtracks):
    """the time steps as the caller composes them on the same handle (newton_steps_ref.steps around the device's linear
    solver and the device's norm)"""
    def solve(S9, b, d, k):
        mg.set_reaction(d)
        mg.build_galerkin(transfer)
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        st, h = run_solver(mg, solver, lin_tol, lin_iters, restart)
        return mg.get_solution(), stats_tuple(st)

    return ns.steps(A0, kap, dm, g, p, u0, theta, nsteps, solve, tol, max_newton, max_backtracks, norm=lambda b: device_norm(mg, L, b))


def want_tuple(o):
    return (len(o["lam"]), int(o["converged"]), o["hist"][0], o["hist"][-1], sum(s[0] for s in o["lin"]), o["backtracks"], len(o["hist"]))


def assert_steps_same(got, want, what):
    done, stats, hists = got
    assert done == len(want), (what, done, len(want))
    for k, o in enumerate(want):
        assert np.array_equal(hists[k], o["hist"]), (what, k, hists[k], o["hist"])
        assert nstats_tuple(stats[k]) == want_tuple(o), (what, k, nstats_tuple(stats[k]), want_tuple(o))


# ---- 1. the passes ---------------------------------------------------------------------------------------------------------
def overshoot_input(L, dt, theta):
    """(kap, dm, p, u0) whose full Newton step is rejected and whose half step is accepted: phi = u^2, dm = 1e4 .. 2e4 far above
    the operator (centre <= 40), u0 = -alpha dm / (2 kap) per point, so that G' = (1 - alpha) dm and G(u0) = (1 + c0) kap u0^2 up
    to the operator's few per cent; the trial's ||G|| is (1 - lam) + lam^2 / s of ||G(u0)|| with s = 4 (1 - alpha)^2 / ((1 +
    c0) alpha^2) = 0.72 for the alpha below: 1.39 at lam = 1 (rejected), 0.85 at lam = 1/2 (accepted).
    tests/test_newton_steps_cpu.py's reference takes that path on random operators of this size"""
    alpha = 0.702 if theta == 1.0 else 0.625
    kap, dm = rand(L, 61, dt, 0.5, 1.0), rand(L, 62, dt, 1e4, 2e4)
    return kap, dm, (0.0, 1.0, 0.0), (-alpha * dm.astype(np.float64) / (2.0 * kap)).astype(dt)


@pytest.mark.parametrize("with_g", [True, False])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("kind", ["five", "nine"])
@pytest.mark.parametrize("dtype, L, Lc", [(1, 4, 3), (1, 8, 5), (0, 4, 3), (0, 9, 5)])
def test_the_passes_are_bit_identical_to_the_reference(pkg, dtype, L, Lc, kind, theta, with_g):
    """one-step calls: max_newton = 0 leaves r in B and the first evaluation's norm in the history; max_newton = 1 leaves d
    in the reaction term and the trial with lam = 1 in U; the overshoot input's step is the trial with lam = 1/2.  kappa
    small against the operator, so that the full step of max_backtracks = 0 passes the test"""
    dt = np_dtype(dtype)
    N = 1 << L
    kap, dm, u0 = rand(L, 71, dt, 0.05, 0.2), rand(L, 74, dt, 0.5, 2.0), rand(L, 73, dt)
    g = rand(L, 72, dt) if with_g else None
    p = (0.25, -0.5, 1.0)
    lin_tol = 1e-10 if dtype == 1 else 1e-5
    lin = dict(solver="solve", lin_tol=lin_tol, lin_max_iters=40)

    def rings_clean(what):
        for which in (pkg.VEC_U, pkg.VEC_B):
            full = whole_level(pkg, mg, L, which).copy()
            full[1:N, 1:N] = 0
            assert not full.any(), (what, which, "ring or padding written")

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        set_operator(mg, kind, L)
        mg.build_galerkin()
        A0 = base_operator(mg, kind, L)
        r = ns.rhs_pass(A0, kap, dm, g, p, u0, theta)
        v, b0, d0 = ns.mass_pass(A0, kap, dm, r, p, u0)
        # the right-hand-side pass and the first evaluation: max_newton = 0
        mg.set_rhs(rand(L, 75, dt))
        mg.set_guess(u0)
        done, stats, hists = mg.newton_steps(1, dm, kap, p=p, theta=theta, g=g, max_newton=0, tol=0.0, **lin)
        assert done == 1 and stats[0].iterations == 0 and stats[0].history_len == 1
        assert_same(mg.get_level(L, pkg.VEC_B), r, (kind, theta, "r"))
        assert np.array_equal(mg.get_solution(), u0)
        rings_clean("first evaluation")
        with pytest.raises(pkg.MgxError, match="no zero-order term"):
            mg.reaction()
        mg.time_newton_step_pass(1, repeats=1)
        assert_same(mg.get_level(L, pkg.VEC_R), b0, (kind, theta, "b of the first evaluation"))
        assert np.array_equal(mg.get_level(L, pkg.VEC_B), r) and np.array_equal(mg.get_solution(), u0)
        r0 = device_norm(mg, L, b0)
        assert list(hists[0]) == [r0], (hists[0], r0)
        # a step: max_newton = 1, max_backtracks = 0
        mg.set_guess(u0)
        done, stats, hists = mg.newton_steps(1, dm, kap, p=p, theta=theta, g=g, max_newton=1, max_backtracks=0, tol=0.0, **lin)
        assert done == 1 and stats[0].iterations == 1 and stats[0].backtracks == 0 and hists[0][0] == r0, (stats[0].iterations, hists)
        u1 = mg.get_solution()
        assert_same(mg.get_level(L, pkg.VEC_B), r, (kind, theta, "B is the step's r"))
        rings_clean("one step")
        assert_same(mg.reaction(), d0, (kind, theta, "d of the first evaluation"))
        # the trial's right-hand side: the timing entry forms un + 1 * U from the time level un = u1 and de = U = u1
        mg.time_newton_step_pass(2, repeats=1)
        assert_same(mg.get_level(L, pkg.VEC_R), ns.mass_pass(A0, kap, dm, r, p, u1, u1, 1.0)[1], (kind, theta, "b of a trial"))
        # ... and the right-hand-side pass from u1, through the timing entry (it reads the source grid of the last call with one)
        mg.time_newton_step_pass(0, theta=theta, repeats=1)
        if with_g:
            assert_same(mg.get_level(L, pkg.VEC_R), ns.rhs_pass(A0, kap, dm, g, p, u1, theta), (kind, theta, "r through the timing entry"))
        assert np.array_equal(mg.get_solution(), u1) and np.array_equal(mg.get_level(L, pkg.VEC_B), r)
        # the host composition of that step on the same handle
        (want,) = host_steps(mg, L, A0, kap, dm, g, p, u0, theta, 1, BILINEAR, "solve", lin_tol, 40, 3, 0.0, 1, 0)
        assert not want["failed"] and np.array_equal(hists[0], want["hist"]), (hists[0], want["hist"])
        assert nstats_tuple(stats[0]) == want_tuple(want)
        assert_same(u1, want["u"], (kind, theta, "U after one step"))
        # the trial with lam = 1/2
        kap2, dm2, p2, v0 = overshoot_input(L, dt, theta)
        mg.set_guess(v0)
        done, stats, hists = mg.newton_steps(1, dm2, kap2, p=p2, theta=theta, g=g, max_newton=1, max_backtracks=4, tol=0.0, **lin)
        assert done == 1 and stats[0].iterations == 1 and stats[0].backtracks == 1, (stats[0].iterations, stats[0].backtracks, hists)
        v1 = mg.get_solution()
        (want,) = host_steps(mg, L, A0, kap2, dm2, g, p2, v0, theta, 1, BILINEAR, "solve", lin_tol, 40, 3, 0.0, 1, 4)
        assert list(want["lam"]) == [0.5] and np.array_equal(hists[0], want["hist"]), (want["lam"], hists[0], want["hist"])
        assert nstats_tuple(stats[0]) == want_tuple(want)
        assert_same(v1, want["u"], (kind, theta, "U after the half step"))


# ---- 2. two time steps against the host composition ------------------------------------------------------------------------
def composition_case(pkg, cfg, kind, name, solver, transfer, theta, lin_tol, tol, cycle=None):
    L, Lc = cfg["finest"], cfg["coarsest"]
    dt = np_dtype(cfg.get("dtype", 1))
    kap, g, p, u0 = problem(name, L, dt)
    dm = rand(L, 86, dt, 0.5, 2.0)
    kw = {k: v for k, v in cfg.items() if k not in ("finest", "coarsest")}
    opts = dict(p=p, theta=theta, g=g, solver=solver, lin_tol=lin_tol, lin_max_iters=40, restart=3, tol=tol, max_newton=8, max_backtracks=6)
    with handle(pkg, L, Lc, **kw) as mg:
        if cycle is not None:
            mg.set_cycle(cycle)
        if name == "cubic":
            set_operator(mg, kind, L)
        else:
            mg.set_coefficient(np.ones(((1 << L) + 1,) * 2))
        mg.build_galerkin(transfer)
        A0 = base_operator(mg, kind, L)
        mg.set_guess(u0)
        got = mg.newton_steps(2, dm, kap, **opts)
        u_dev, b_dev = mg.get_solution(), mg.get_level(L, pkg.VEC_B)
        what = (kind, name, solver, transfer, theta)
        assert got[0] == 2 and all(s.converged == 1 and s.iterations >= 1 for s in got[1]), (what, pkg.lib().mgx_last_error(mg._h).decode())
        d_dev = mg.reaction()
        want = host_steps(mg, L, A0, kap, dm, g, p, u0, theta, 2, transfer, solver, lin_tol, 40, 3, tol, 8, 6)
        assert_steps_same(got, want, what)
        assert_same(u_dev, want[-1]["u"], (what, "U"))
        assert_same(b_dev, want[-1]["r"], (what, "B is the last step's r"))
        assert_same(d_dev, want[-1]["ds"][-1], (what, "d of the last linear solve"))
        # once more on the handle the composition left (a term is set: it is replaced), the same bits
        mg.set_guess(u0)
        again = mg.newton_steps(2, dm, kap, **opts)
        assert_steps_same(again, want, (what, "second call"))
        assert_same(mg.get_solution(), want[-1]["u"], (what, "U of the second call"))
        assert_same(mg.reaction(), want[-1]["ds"][-1], (what, "d after the second call"))


@pytest.mark.parametrize("solver", ["solve", "gcr", "refine_gcr"])
@pytest.mark.parametrize("kind, name, transfer, theta", [("five", "cubic", BILINEAR, 0.5), ("nine", "cubic", OPERATOR, 1.0),
                                                         ("five", "allen-cahn", OPERATOR, 0.5), ("five", "allen-cahn", BILINEAR, 1.0)])
def test_two_steps_are_the_host_composition_jacobi(pkg, kind, name, transfer, theta, solver):
    composition_case(pkg, dict(finest=6, coarsest=3, **JACOBI), kind, name, solver, transfer, theta, 1e-8, 1e-6)


def test_two_steps_are_the_host_composition_colour_sgs(pkg):
    composition_case(pkg, dict(finest=6, coarsest=3, **SGS), "nine", "cubic", "gcr", BILINEAR, 0.5, 1e-8, 1e-6)


def test_two_steps_with_w_cycles(pkg):
    composition_case(pkg, dict(finest=6, coarsest=3, **JACOBI), "five", "allen-cahn", "solve", BILINEAR, 0.5, 1e-8, 1e-6, cycle=pkg.CYCLE_W)


def test_two_steps_in_float(pkg):
    composition_case(pkg, dict(finest=6, coarsest=3, dtype=0, **JACOBI), "five", "cubic", "gcr", OPERATOR, 0.5, 1e-4, 1e-3)


# ---- 3. a physical check -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, theta", [("five", 0.5), ("nine", 1.0)])
def test_a_step_zeroes_g_recomputed_on_the_host(pkg, kind, theta):
    """F64, L = 5, tol = 1e-8: ||G(u+)|| recomputed in numpy float64 (newton_steps_ref.g_norm: the sparse matrix of the
    stencil the handle returns, nothing of the passes) is at most 2 tol history[0] of the step; the factor 2 covers the
    other summation order of the norm only"""
    L, Lc, dt, tol = 5, 3, np.float64, 1e-8
    kap, g, p, u0 = problem("cubic", L, dt)
    dm = rand(L, 87, dt, 0.5, 2.0)
    with handle(pkg, L, Lc) as mg:
        set_operator(mg, kind, L)
        mg.build_galerkin()
        A0 = base_operator(mg, kind, L)
        mg.set_guess(u0)
        levels = [u0]
        done, stats, hists = mg.newton_steps(2, dm, kap, p=p, theta=theta, g=g, lin_tol=1e-10, lin_max_iters=40, tol=tol, max_newton=10)
        assert done == 2 and all(s.converged == 1 for s in stats)
        last = mg.get_solution()
        # the first step's end: one step from u0 on the handle again
        mg.set_guess(u0)
        mg.newton_steps(1, dm, kap, p=p, theta=theta, g=g, lin_tol=1e-10, lin_max_iters=40, tol=tol, max_newton=10)
        levels += [mg.get_solution(), last]
        for k in range(2):
            gn = ns.g_norm(A0, kap, dm, g, p, levels[k], levels[k + 1], theta)
            print(kind, theta, "step", k, "||G(u+)|| =", gn, "history[0] =", hists[k][0], "device's last norm =", hists[k][-1])
            assert gn <= 2.0 * tol * hists[k][0], (k, gn, hists[k])


# ---- 4. budget and line-search exits -------------------------------------------------------------------------------------------
def raw_steps(pkg, mg, mass, kap, count=None, theta=1.0, nsteps=1, g=None, done=None, stats=None, hist=None, cap=0, **kw):
    B = pkg.binding
    o = dict(p1=0.0, p2=0.0, p3=1.0, solver=0, lin_tol=1e-8, lin_max_iters=20, restart=3, tol=1e-10, max_newton=3, max_backtracks=4)
    o.update(kw)
    opt = B.NewtonOpts(**o)
    ptr = lambda a: None if a is None else a.ctypes.data
    size = (kap if kap is not None else mass).size if count is None else count
    return pkg.lib().mgx_newton_steps(mg._h, C.byref(opt), theta, nsteps, ptr(mass), ptr(kap), ptr(g), size, done, stats,
                                      None if hist is None else hist.ctypes.data_as(C.POINTER(C.c_double)), cap)


def test_a_step_out_of_budget_ends_the_call(pkg):
    L, Lc, dt = 6, 3, np.float64
    kap, g, p, u0 = problem("cubic", L, dt)
    dm = rand(L, 88, dt, 0.5, 2.0)
    B = pkg.binding
    with handle(pkg, L, Lc) as mg:
        set_operator(mg, "five", L)
        mg.build_galerkin()
        A0 = base_operator(mg, "five", L)
        mg.set_guess(u0)
        stats = (B.NewtonStats * 3)()
        for s in stats:
            s.iterations = -7
        hist = np.full((3, 4), -1.0)
        done = C.c_int(-1)
        rc = raw_steps(pkg, mg, dm, kap, theta=0.5, nsteps=3, g=g, done=C.byref(done), stats=stats, hist=hist, cap=4, p1=p[0], p2=p[1], p3=p[2],
                       tol=0.0, max_newton=1)
        msg = pkg.lib().mgx_last_error(mg._h).decode()
        assert rc == 0 and done.value == 1, (rc, done.value, msg)
        assert "mgx_newton_steps: step 0 did not converge" in msg and "later steps were not taken" in msg, msg
        assert stats[0].iterations == 1 and stats[0].converged == 0 and stats[0].history_len == 2
        assert stats[1].iterations == -7 and stats[2].iterations == -7 and (hist[1:] == -1.0).all() and (hist[0, 2:] == -1.0).all()
        u1 = mg.get_solution()
        (want,) = host_steps(mg, L, A0, kap, dm, g, p, u0, 0.5, 3, BILINEAR, "solve", 1e-8, 20, 3, 0.0, 1, 4)
        assert np.array_equal(hist[0, :2], want["hist"]) and np.array_equal(u1, want["u"])


@pytest.mark.parametrize("L, Lc", [(5, 3), (6, 3)])
def test_backtracks_are_counted_as_the_reference_counts_them(pkg, L, Lc):
    """newton_ref.backtracking_input as the time level of an Euler step with dm = 0.01 lambda_min and g = its f: the first
    Jacobian A0 + dm + 2 kap u0 has the smallest eigenvalue 0.11 lambda_min and the first full step overshoots, as on
    the reference alone (five rejected trials at L = 5, four at L = 6 with direct solves)"""
    A0n, kap, f, p, u0 = nf.backtracking_input(L)
    dm = np.full_like(kap, 0.01 * nf.poisson_lambda_min(L))
    opts = dict(p=p, theta=1.0, g=f, solver="solve", lin_tol=1e-8, lin_max_iters=30, tol=1e-10, max_newton=10, max_backtracks=8)
    with handle(pkg, L, Lc, **JACOBI) as mg:
        mg.set_coefficient(np.ones(((1 << L) + 1,) * 2))
        mg.build_galerkin()
        A0 = base_operator(mg, "five", L)
        mg.set_guess(u0)
        got = mg.newton_steps(2, dm, kap, **opts)
        u_dev = mg.get_solution()
        assert got[0] == 2 and got[1][0].backtracks >= 1 and got[1][1].backtracks == 0, [nstats_tuple(s) for s in got[1]]
        want = host_steps(mg, L, A0, kap, dm, f, p, u0, 1.0, 2, BILINEAR, "solve", 1e-8, 30, 3, 1e-10, 10, 8)
        assert_steps_same(got, want, ("backtracking", L))
        assert_same(u_dev, want[-1]["u"], "U")
        # with two halvings the line search of step 0 fails: the call ends there, U is the time level it started from
        mg.set_guess(u0)
        done, stats, hists = mg.newton_steps(2, dm, kap, **dict(opts, max_backtracks=2))
        msg = pkg.lib().mgx_last_error(mg._h).decode()
        assert done == 1 and stats[0].converged == 0 and stats[0].iterations == 0 and stats[0].backtracks == 3, nstats_tuple(stats[0])
        assert "mgx_newton_steps: step 0" in msg and "line search failed" in msg and "later steps were not taken" in msg, msg
        assert np.array_equal(mg.get_solution(), u0)


# ---- 5. state ------------------------------------------------------------------------------------------------------------------
def test_zero_steps_touch_nothing(pkg):
    L, Lc, dt = 6, 3, np.float64
    kap, f, p, u0 = problem("cubic", L, dt)
    dm, d = rand(L, 89, dt, 0.5, 2.0), rand(L, 91, dt, 0.5, 2.0)
    with handle(pkg, L, Lc) as mg:
        set_operator(mg, "five", L)
        mg.build_galerkin(OPERATOR)
        mg.set_rhs(f)
        mg.set_guess(u0)
        mg.solve(tol=0.0, max_cycles=2)                       # (captures graphs)
        u = mg.get_solution()
        graphs, centre = mg.graphs_cached(), mg.get_stencil(L, 0)
        done, stats, hists = mg.newton_steps(0, dm, kap, p=p, theta=0.5, g=f)
        assert done == 0 and stats == [] and mg.graphs_cached() == graphs and mg.transfer == OPERATOR
        assert np.array_equal(mg.get_stencil(L, 0), centre)
        with pytest.raises(pkg.MgxError, match="no zero-order term"):
            mg.reaction()
        assert np.array_equal(mg.get_solution(), u) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        with pytest.raises(pkg.MgxError, match="mgx_newton_steps first"):       # (not even the workspace)
            mg.time_newton_step_pass(0)
        # ... and a term that is set stays, with its hierarchy
        mg.set_reaction(d)
        mg.build_galerkin(OPERATOR)
        shifted, graphs = mg.get_stencil(L, 0), mg.graphs_cached()
        assert mg.newton_steps(0, dm, kap, p=p)[0] == 0
        assert np.array_equal(mg.reaction(), d) and np.array_equal(mg.get_stencil(L, 0), shifted) and mg.graphs_cached() == graphs
        assert np.array_equal(mg.get_solution(), u) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        assert mg.solve(tol=1e-8, max_cycles=30)[0].converged == 1          # (still built)


def test_the_state_after_the_call_is_a_set_reaction_and_a_build(pkg):
    L, Lc, dt = 6, 3, np.float64
    kap, g, p, u0 = problem("cubic", L, dt)
    dm = rand(L, 94, dt, 0.5, 2.0)
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
        mg.set_guess(u0)
        done, stats, hists = mg.newton_steps(1, dm, kap, p=p, theta=0.5, g=g, max_newton=1, tol=0.0)
        assert done == 1 and stats[0].iterations == 1
        d0 = ns.mass_pass(A0, kap, dm, ns.rhs_pass(A0, kap, dm, g, p, u0, 0.5), p, u0)[2]
        assert_same(mg.reaction(), d0, "d_0")
        assert_same(mg.get_stencil(L, 0), A0[0] + d0, "centre")
        shifted = bits(mg)                                    # (the hierarchy is built)
    with handle(pkg, L, Lc) as mg:                            # the composed handle
        set_operator(mg, "five", L)
        mg.set_reaction(d0)
        mg.build_galerkin()
        composed = bits(mg)
        assert np.array_equal(shifted[0], composed[0]) and np.array_equal(shifted[1], composed[1])
        mg.set_reaction(None)
        mg.build_galerkin()
        after = bits(mg)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
        assert not np.array_equal(shifted[0], before[0])


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refused_handles(pkg, po):
    L, Lc = 7, 4
    kap = np.ones(((1 << L) - 1,) * 2)
    small = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, schedule=0)
    b = po.rhs_sine(L)
    lib = pkg.lib()
    ms = C.c_double()

    def all_refuse(mg, word):
        for i, call in enumerate((lambda: raw_steps(pkg, mg, kap, kap), lambda: lib.mgx_time_newton_step_pass(mg._h, 0, 0.5, 1, C.byref(ms)))):
            assert call() == STATE, (word, i)
            assert word in lib.mgx_last_error(mg._h).decode(), (i, lib.mgx_last_error(mg._h).decode())

    with pkg.Multigrid(**small) as mg:
        all_refuse(mg, "POISSON")
        assert raw_steps(pkg, mg, kap, kap, count=3) == INVALID       # (the argument checks come first)
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
    kap, g, p, u0 = problem("cubic", L, dt)
    dm = rand(L, 95, dt, 0.5, 2.0)
    lin_tol = 1e-8 if dtype == 1 else 1e-4
    ms = C.c_double(-1.0)
    nan, inf = float("nan"), float("inf")

    def expect(code, word, call):
        assert call() == code, word
        assert word in lib.mgx_last_error(mg._h).decode(), (word, lib.mgx_last_error(mg._h).decode())

    def reference_bits(m):
        m.set_guess(u0)
        done, stats, hists = m.newton_steps(2, dm, kap, p=p, theta=0.5, g=g, solver="gcr", lin_tol=lin_tol, lin_max_iters=20, restart=3, tol=0.0,
                                            max_newton=1)
        return done, [nstats_tuple(s) for s in stats], hists, m.get_solution()

    def same(x, y):
        return x[0] == y[0] == 1 and x[1] == y[1] and np.array_equal(x[2][0], y[2][0]) and np.array_equal(x[3], y[3])

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        set_operator(mg, "five", L)
        mg.build_galerkin()
        want = reference_bits(mg)
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        bad = lambda **kw: (lambda: raw_steps(pkg, mg, dm, kap, **kw))
        # before the finest operator is set, and before the build
        expect(STATE, "finest operator not set", bad())
        expect(STATE, "finest operator not set", lambda: lib.mgx_time_newton_step_pass(mg._h, 0, 0.5, 1, C.byref(ms)))
        set_operator(mg, "five", L)
        expect(STATE, "not built", bad())
        expect(STATE, "not built", bad(nsteps=0))
        expect(STATE, "mgx_newton_steps first", lambda: lib.mgx_time_newton_step_pass(mg._h, 0, 0.5, 1, C.byref(ms)))
        mg.build_galerkin()
        expect(STATE, "mgx_newton_steps first", lambda: lib.mgx_time_newton_step_pass(mg._h, 2, 0.5, 1, C.byref(ms)))
        assert ms.value == -1.0
        # NULL opt: the outputs are left alone
        done = C.c_int(7)
        assert lib.mgx_newton_steps(mg._h, None, 1.0, 1, dm.ctypes.data, kap.ctypes.data, None, kap.size, C.byref(done), None, None, 0) == INVALID
        assert done.value == 7
        # every INVALID, each with everything after it in the documented order wrong as well
        expect(INVALID, "n*n", bad(count=n * n - 1))
        later = dict(count=n * n - 1)
        chain = [("kappa", dict(kap=None)), ("mass", dict(mass=None)), ("nsteps", dict(nsteps=-1)), ("theta", dict(theta=nan)),
                 ("max_backtracks", dict(max_backtracks=31)), ("max_newton", dict(max_newton=-1)), ("tol", dict(tol=nan)),
                 ("restart", dict(solver=1, restart=9)), ("lin_max_iters", dict(lin_max_iters=-1)), ("lin_tol", dict(lin_tol=-1.0)),
                 ("solver", dict(solver=3)), ("finite", dict(p2=inf))]
        for word, kw in chain:                                # from the last check to the first: each one shadows the earlier ones
            later.update(kw)
            args = dict(later)
            expect(INVALID, word, lambda: raw_steps(pkg, mg, args.pop("mass", dm), args.pop("kap", kap), **args))
        for kw, word in ((dict(theta=0.0), "theta"), (dict(theta=1.5), "theta"), (dict(theta=-0.5), "theta"), (dict(p1=nan), "finite"),
                         (dict(solver=-1), "solver"), (dict(solver=2, restart=0), "restart"), (dict(tol=-1.0), "tol"),
                         (dict(max_backtracks=-1), "max_backtracks"), (dict(count=n * n + 1), "n*n")):
            expect(INVALID, word, bad(**kw))
        done = C.c_int(7)
        assert raw_steps(pkg, mg, dm, kap, nsteps=-1, done=C.byref(done)) == INVALID and done.value == 0
        if dtype == 0:
            expect(STATE, "F64", bad(solver=pkg.STEP_REFINE_GCR))
        for which, theta, repeats, out in ((3, 0.5, 1, C.byref(ms)), (-1, 0.5, 1, C.byref(ms)), (0, 0.0, 1, C.byref(ms)), (0, nan, 1, C.byref(ms)),
                                           (0, 0.5, 0, C.byref(ms)), (0, 0.5, 1, None)):
            expect(INVALID, "mgx_time_newton_step_pass", lambda: lib.mgx_time_newton_step_pass(mg._h, which, theta, repeats, out))
        assert ms.value == -1.0
        assert same(reference_bits(mg), want)


# ---- 7. the timing entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["five", "nine"])
def test_timing_the_passes_leaves_u_b_and_the_operator(pkg, kind):
    L, Lc, dt = 8, 5, np.float64
    kap, g, p, u0 = problem("cubic", L, dt)
    dm = rand(L, 96, dt, 0.5, 2.0)
    opts = dict(p=p, theta=0.5, g=g, max_newton=1, tol=0.0, lin_max_iters=10)
    with handle(pkg, L, Lc) as mg:
        set_operator(mg, kind, L)
        mg.build_galerkin()
        mg.set_guess(u0)
        done, stats, hists = mg.newton_steps(1, dm, kap, **opts)
        u, b, d, centre = mg.get_solution(), mg.get_level(L, pkg.VEC_B), mg.reaction(), finest_slots(mg, kind, L)[0]
        graphs = mg.graphs_cached()
        for which, theta in ((0, 0.5), (0, 1.0), (1, 0.5), (2, 0.5)):
            ms = mg.time_newton_step_pass(which, theta=theta, repeats=5)
            assert np.isfinite(ms) and ms > 0.0, (which, ms)
            assert np.array_equal(mg.get_solution(), u) and np.array_equal(mg.get_level(L, pkg.VEC_B), b)
            assert np.array_equal(mg.reaction(), d) and np.array_equal(finest_slots(mg, kind, L)[0], centre) and mg.graphs_cached() == graphs
        # the next call starts from the time level it was left with: the same bits as the second of two steps
        mg.set_guess(u0)
        two = mg.newton_steps(2, dm, kap, **opts)             # (max_newton = 1, tol = 0: ends after step 0)
        assert two[0] == 1 and np.array_equal(two[2][0], hists[0]) and np.array_equal(mg.get_solution(), u)
