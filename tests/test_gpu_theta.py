"""GPU tests of the zero-order term and the theta steps of GALERKIN handles (mgx_set_reaction, mgx_theta_steps,
mgx_time_theta_rhs; include/mgx.h, csrc/mgx_theta.hpp) against the numpy statement of tests/theta_ref.py, which
tests/test_theta_cpu.py pins against mathematics.

Bit for bit: the shifted centre, the hierarchy built from it against the host path (read back, add, mgx_set_stencil[9]),
removal and replacement of the term, the right-hand-side pass, and whole steps against the host composition
{pass on the host, mgx_set_rhs, the same solver call} on the same handle.  The two tolerances that appear (eigenvalues,
the refine solver's true residual) are derived where they are used.

Shapes: a wave covers 62 output lanes, 124 columns in double and 248 in float, so the pass runs at L = 4 (one strip, most
points next to the ring) and at L = 8 in double / L = 9 in float (more than one strip)."""
import ctypes as C

import numpy as np
import pytest

import eig_ref as er
import galerkin_ref as gr
import hipmem
import nine_ref as nr
import theta_ref as tr
from pcg_ref import contrast_coefficient
from test_gpu_galerkin import assert_same, handle, np_dtype

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 5                      # MGX_ERR_INVALID, MGX_ERR_STATE
OPERATOR = 1                               # MGX_TRANSFER_OPERATOR
STAT_FIELDS = ("cycles", "converged", "initial_residual", "final_residual", "fine_updates", "history_len")   # (not seconds)


def set_operator(mg, kind, L):
    """five: -div(a grad u) with a contrast of 10 (mgx_set_coefficient); nine: the tensor rotated by 45 degrees (mgx_set_tensor)"""
    if kind == "five":
        mg.set_coefficient(contrast_coefficient(L, 10.0))
    else:
        mg.set_tensor(*nr.rotated_tensor(L, 45.0, 0.5))


def finest_slots(mg, kind, L):
    """the finest operator as stored: mgx_get_stencil's five grids, or mgx_get_stencil9's nine (after a build)"""
    if kind == "five":
        return [mg.get_stencil(L, q) for q in range(5)]
    return [mg.get_stencil9(L, q) for q in range(9)]


def rand(L, seed, dt, lo=-1.0, hi=1.0):
    n = (1 << L) - 1
    return np.random.default_rng(seed).uniform(lo, hi, (n, n)).astype(dt)


def stats_tuple(st):
    return tuple(getattr(st, f) for f in STAT_FIELDS)


def whole_level(pkg, mg, L, which):
    """a whole level grid (rows 0 .. N, `pitch` columns) through mgx_get_level_device"""
    dt = mg.level_dtype(L)
    pitch = pkg.lib().mgx_level_pitch(L, mg.cfg.dtype)
    buf = hipmem.zeros(((1 << L) + 1, pitch), dt)
    mg.get_level_device(L, which, buf.data_ptr())
    return buf.numpy()


def run_solver(mg, solver, tol, iters, restart=3):
    if solver == "solve":
        return mg.solve(tol=tol, max_cycles=iters)
    if solver == "gcr":
        return mg.solve_gcr(tol=tol, max_iters=iters, restart=restart)
    return mg.solve_refine_gcr(tol=tol, max_iters=iters, restart=restart)


def host_step(mg, L, u, d, g, theta, solver, tol, iters, restart=3):
    """one step as the caller composes it on the same handle: S u = -residual(L, u, 0), the pass in numpy, mgx_set_rhs, the
    solver from U = u; returns (b, stats, history, the new U)"""
    Su = -mg.residual(L, u, np.zeros_like(u))                # (leaves U = u)
    b = tr.rhs_pass(Su, u, d, g, theta)
    mg.set_rhs(b)
    st, h = run_solver(mg, solver, tol, iters, restart)
    return b, st, h, mg.get_solution()


# ---- 1. the shift ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L, Lc", [(4, 3), (6, 3)])
@pytest.mark.parametrize("kind", ["five", "nine"])
@pytest.mark.parametrize("dtype", [1, 0])
def test_the_centre_is_shifted_in_the_working_type(pkg, dtype, kind, L, Lc):
    dt = np_dtype(dtype)
    d, d2 = rand(L, 1, dt, 0.5, 2.0), rand(L, 2, dt, 0.0, 30.0)
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        set_operator(mg, kind, L)
        mg.build_galerkin()
        base = finest_slots(mg, kind, L)
        with pytest.raises(pkg.MgxError, match="invalid state.*no zero-order term"):
            mg.reaction()
        for term in (d, d2):                                  # the second call replaces the first: c0 + d2, no accumulation
            mg.set_reaction(term)
            assert_same(mg.reaction(), term, "d read back")
            with pytest.raises(pkg.MgxError, match="invalid state.*not built"):
                mg.vcycle()
            mg.build_galerkin()
            got = finest_slots(mg, kind, L)
            assert_same(got[0], base[0] + term, (kind, "shifted centre"))
            for q in range(1, len(base)):
                assert_same(got[q], base[q], (kind, "slot", gr.SLOTS[q]))


# ---- 2. the hierarchy is the host path's ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["five", "nine"])
@pytest.mark.parametrize("dtype", [1, 0])
def test_the_hierarchy_is_that_of_the_host_path(pkg, dtype, kind):
    dt = np_dtype(dtype)
    L, Lc = 6, 3
    d = rand(L, 3, dt, 0.5, 2.0)
    b, u0 = rand(L, 4, dt), rand(L, 5, dt)

    def probe(mg):
        out = {}
        for lv in range(Lc, L + 1):
            out[lv] = [mg.get_stencil9(lv, q) for q in range(10)] + [mg.lambda_max(lv)]
        mg.set_rhs(b)
        mg.set_guess(u0)
        st, h = mg.solve(tol=0.0, max_cycles=10)
        return out, h, mg.get_solution()

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        set_operator(mg, kind, L)
        mg.build_galerkin(OPERATOR)
        base = finest_slots(mg, kind, L)
        mg.set_reaction(d)
        mg.build_galerkin(OPERATOR)
        a_levels, a_hist, a_u = probe(mg)
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        host = [base[0] + d] + base[1:]
        if kind == "five":
            mg.set_stencil(L, *host)
        else:
            mg.set_stencil9(L, *host)
        mg.build_galerkin(OPERATOR)
        b_levels, b_hist, b_u = probe(mg)
    for lv in range(Lc, L + 1):
        for q in range(10):
            assert_same(a_levels[lv][q], b_levels[lv][q], (kind, "level", lv, "grid", q))
        assert a_levels[lv][10] == b_levels[lv][10], (kind, "lambda_max", lv)
    assert len(a_hist) == 11 and np.array_equal(a_hist, b_hist) and np.array_equal(a_u, b_u)


# ---- 3. removal and replacement ---------------------------------------------------------------------------------------
def test_removal_and_replacement_restore_the_bits(pkg):
    L, Lc, dt = 6, 3, np.float64
    a = contrast_coefficient(L, 10.0)
    d = rand(L, 6, dt, 0.5, 2.0)
    b, u0 = rand(L, 7, dt), rand(L, 8, dt)
    bm = np.stack([rand(L, 9, dt), rand(L, 10, dt)])

    def bits(mg):
        out = []
        for run in (lambda: mg.solve(tol=0.0, max_cycles=3), lambda: mg.solve_gcr(tol=0.0, max_iters=3, restart=2)):
            mg.set_rhs(b)
            mg.set_guess(u0)
            st, h = run()
            out += [h, mg.get_solution()]
        st, hs, um = mg.solve_multi(bm, tol=0.0, max_cycles=3)
        return out + hs + [um]

    def same(x, y):
        return len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))

    with handle(pkg, L, Lc) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        before = bits(mg)
        # no term set: removing it is a no-op that keeps the hierarchy and the captured graphs
        graphs = mg.graphs_cached()
        mg.set_reaction(None)
        assert mg.graphs_cached() == graphs
        assert same(bits(mg), before)
        mg.set_reaction(d)
        mg.build_galerkin()
        shifted = bits(mg)
        assert not np.array_equal(shifted[0], before[0])
        mg.set_reaction(None)
        with pytest.raises(pkg.MgxError, match="invalid state.*not built"):
            mg.solve(tol=0.0, max_cycles=1)
        mg.build_galerkin()
        assert_same(mg.get_stencil(L, 0), er.coefficient_stencil(a)[0], "restored centre")
        assert same(bits(mg), before)
        # a new finest operator drops the term
        mg.set_reaction(d)
        mg.set_coefficient(a)
        with pytest.raises(pkg.MgxError, match="invalid state.*no zero-order term"):
            mg.reaction()
        mg.build_galerkin()
        assert same(bits(mg), before)
        # ... and the term can be set again afterwards, on the centre that call gave
        mg.set_reaction(d)
        mg.build_galerkin()
        assert same(bits(mg), shifted)


# ---- 4. the pass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["five", "nine"])
@pytest.mark.parametrize("dtype, L, Lc", [(1, 4, 3), (1, 8, 5), (0, 4, 3), (0, 9, 5)])
def test_the_pass_is_bit_identical_to_the_reference(pkg, dtype, L, Lc, kind):
    dt = np_dtype(dtype)
    N = 1 << L
    d, u, g = rand(L, 11, dt, 0.5, 2.0), rand(L, 12, dt), rand(L, 13, dt)
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        set_operator(mg, kind, L)
        mg.set_reaction(d)
        mg.build_galerkin()
        Su = -mg.residual(L, u, np.zeros_like(u))
        for theta in (1.0, 0.5, 0.75):
            for gg in (None, g):
                mg.set_guess(u)
                done, stats, hists = mg.theta_steps(1, theta=theta, g=gg, solver="solve", tol=0.0, max_iters=0)
                assert done == 1 and stats[0].cycles == 0 and len(hists[0]) == 1
                want = tr.rhs_pass(Su, u, d, gg, theta)
                full = whole_level(pkg, mg, L, pkg.VEC_B)
                assert_same(full[1:N, 1:N], want, (kind, theta, gg is not None))
                assert_same(mg.get_level(L, pkg.VEC_B), want, "B through mgx_get_level")
                ring = full.copy()
                ring[1:N, 1:N] = 0
                assert not ring.any(), (kind, theta, "ring or padding of B written")
                assert np.array_equal(mg.get_solution(), u)


# ---- 5. steps ----------------------------------------------------------------------------------------------------------
def steps_case(pkg, cfg, kind, solver, theta, tol, cycle=None, with_g=True):
    L, Lc = cfg["finest"], cfg["coarsest"]
    dtype = cfg.get("dtype", 1)
    dt = np_dtype(dtype)
    d, u0 = rand(L, 21, dt, 0.5, 2.0), rand(L, 22, dt)
    g = rand(L, 23, dt) if with_g else None
    kw = {k: v for k, v in cfg.items() if k not in ("finest", "coarsest")}
    with handle(pkg, L, Lc, **kw) as mg:
        if cycle is not None:
            mg.set_cycle(cycle)
        set_operator(mg, kind, L)
        mg.set_reaction(d)
        mg.build_galerkin()
        u, want = u0, []
        for k in range(3):
            b, st, h, u = host_step(mg, L, u, d, g, theta, solver, tol, 40)
            assert st.converged == 1, (k, h)
            want.append((b, stats_tuple(st), h, u))
        for ns in (1, 2, 3):
            mg.set_guess(u0)
            done, stats, hists = mg.theta_steps(ns, theta=theta, g=g, solver=solver, tol=tol, max_iters=40, restart=3)
            assert done == ns
            assert_same(mg.get_solution(), want[ns - 1][3], (solver, theta, "U after", ns, "steps"))
            assert_same(mg.get_level(L, pkg.VEC_B), want[ns - 1][0], (solver, theta, "B after", ns, "steps"))
            for k in range(ns):
                assert stats_tuple(stats[k]) == want[k][1], (solver, theta, ns, k)
                assert np.array_equal(hists[k], want[k][2]), (solver, theta, ns, k)


JACOBI = dict(smoother=0, mu1=2, mu2=2)
SGS = dict(smoother=9, mu1=1, mu2=1)


@pytest.mark.parametrize("smoother", ["jacobi", "sgs"])
@pytest.mark.parametrize("L, kind", [(6, "five"), (7, "nine")])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("solver", ["solve", "gcr", "refine_gcr"])
def test_steps_are_the_host_composition_bit_for_bit(pkg, solver, theta, L, kind, smoother):
    cfg = dict(finest=L, coarsest=3, **(JACOBI if smoother == "jacobi" else SGS))
    steps_case(pkg, cfg, kind, solver, theta, 1e-8)


@pytest.mark.parametrize("solver", ["solve", "gcr"])
def test_steps_in_float(pkg, solver):
    steps_case(pkg, dict(finest=7, coarsest=3, dtype=0, **JACOBI), "five", solver, 0.5, 1e-4)


def test_steps_with_w_cycles_and_no_source(pkg):
    steps_case(pkg, dict(finest=6, coarsest=3, **JACOBI), "nine", "gcr", 0.5, 1e-8, cycle=pkg.CYCLE_W, with_g=False)


# ---- 6. a step that does not converge ends the call -------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["solve", "gcr"])
def test_an_unconverged_step_is_the_last(pkg, solver):
    L, Lc, dt = 6, 3, np.float64
    d, u0, g = rand(L, 31, dt, 0.5, 2.0), rand(L, 32, dt), rand(L, 33, dt)
    lib = pkg.lib()
    with handle(pkg, L, Lc) as mg:
        set_operator(mg, "five", L)
        mg.set_reaction(d)
        mg.build_galerkin()
        b, st, h, u1 = host_step(mg, L, u0, d, g, 0.5, solver, 1e-14, 1)
        assert st.converged == 0
        mg.set_guess(u0)
        stats = (pkg.binding.Stats * 3)()
        for s in stats:
            s.cycles, s.history_len = -7, -7
        hist = np.full((3, 2), -1.0)
        done = C.c_int(-1)
        code = pkg.STEP_SOLVERS[solver]
        assert lib.mgx_theta_steps(mg._h, 0.5, 3, g.ctypes.data, code, 1e-14, 1, 3, C.byref(done), stats,
                                   hist.ctypes.data_as(C.POINTER(C.c_double)), 2) == 0
        assert done.value == 1
        assert stats_tuple(stats[0]) == stats_tuple(st) and stats[0].converged == 0
        assert np.array_equal(hist[0], h)
        assert all(s.cycles == -7 and s.history_len == -7 for s in stats[1:]) and (hist[1:] == -1.0).all()
        msg = lib.mgx_last_error(mg._h).decode()
        assert "step 0" in msg and "did not converge" in msg, msg
        assert_same(mg.get_solution(), u1, "U of the unconverged step")
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B of the unconverged step")
        # nsteps = 0: nothing happens
        assert lib.mgx_theta_steps(mg._h, 0.5, 0, None, code, 1e-14, 1, 3, C.byref(done), None, None, 0) == 0
        assert done.value == 0 and np.array_equal(mg.get_solution(), u1) and np.array_equal(mg.get_level(L, pkg.VEC_B), b)


# ---- 7. the rest of the library runs on S -------------------------------------------------------------------------------
def test_eigenvalues_are_shifted(pkg):
    """a = 1, d = 0.5 everywhere: the eigenvalues of S are the closed-form ones of the Poisson stencil plus 0.5.  A
    unit-norm Ritz pair with residual <= tol * theta_j has an eigenvalue error <= tol * theta_j; 1e-12 covers the
    rounding of the Rayleigh quotient (eps * lambda_max * a few)"""
    L, tol = 6, 1e-8
    N = 1 << L
    n = N - 1
    with handle(pkg, L, 3) as mg:
        mg.set_coefficient(np.ones((N + 1, N + 1)))
        mg.set_reaction(np.full((n, n), 0.5))
        mg.build_galerkin()
        lam, X, stats, hists = mg.eigs(2, tol=tol)
        assert all(s.converged == 1 for s in stats)
    want = er.constant_eigenvalues(L, 1.0, 3) + 0.5
    assert abs(lam[0] - want[0]) <= tol * lam[0] + 1e-12, (lam, want)
    assert abs(lam[1] - want[1]) <= tol * lam[1] + 1e-12 and want[1] == want[2], (lam, want)   # (a double eigenvalue)


def test_the_float_shadow_follows_the_term(pkg):
    """mgx_solve_refine_gcr on S reaches 1e-10, and - with a shadow that an earlier call built from A0 - computes the bits of
    a handle that never refined on A0: the float copy was rebuilt from S.  The true residual b - S u in numpy differs
    from the recursively updated one by rounding of O(eps * 9 max|S| max|u| n * iterations) < 1e-11 here, against
    tol * ||r0|| of 1e-9"""
    L, Lc, dt = 7, 3, np.float64
    a = contrast_coefficient(L, 10.0)
    d = rand(L, 41, dt, 20.0, 60.0)
    b = rand(L, 42, dt)
    tol = 1e-10

    def run(mg):
        mg.set_reaction(d)
        mg.build_galerkin()
        mg.set_rhs(b)
        mg.zero_level(L, pkg.VEC_U)
        st, h = mg.solve_refine_gcr(tol=tol, max_iters=30, restart=4)
        return st, h, mg.get_solution()

    with handle(pkg, L, Lc) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_rhs(b)
        st0, h0 = mg.solve_refine_gcr(tol=tol, max_iters=30, restart=4)      # the shadow now holds A0
        st, h, u = run(mg)
    with handle(pkg, L, Lc) as mg:
        mg.set_coefficient(a)
        st2, h2, u2 = run(mg)
    assert st.converged == 1 and h[-1] <= tol * h[0]
    assert np.array_equal(h, h2) and np.array_equal(u, u2)
    assert st0.converged == 1
    S = tr.shift(er.coefficient_stencil(a), d)
    true = np.linalg.norm(b - tr.apply(S, u))
    assert true <= tol * h[0] + 1e-11, (true, h[0])


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def raw_steps(pkg, mg, theta=1.0, nsteps=1, solver=0, tol=1e-8, iters=5, restart=3):
    return pkg.lib().mgx_theta_steps(mg._h, theta, nsteps, None, solver, tol, iters, restart, None, None, None, 0)


def all_refuse(pkg, mg, d, want, word):
    lib = pkg.lib()
    ms = C.c_double()
    out = np.empty_like(d)
    calls = (lambda: lib.mgx_set_reaction(mg._h, d.ctypes.data, d.size), lambda: lib.mgx_get_reaction(mg._h, out.ctypes.data, out.size),
             lambda: raw_steps(pkg, mg), lambda: lib.mgx_time_theta_rhs(mg._h, 1.0, 1, C.byref(ms)))
    for i, call in enumerate(calls):
        assert call() == want, i
        assert word in lib.mgx_last_error(mg._h).decode(), (i, lib.mgx_last_error(mg._h).decode())


def test_refused_handles(pkg, po):
    L, Lc = 7, 4
    d = np.ones(((1 << L) - 1,) * 2)
    small = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, schedule=0)
    b = po.rhs_sine(L)
    with pkg.Multigrid(**small) as mg:
        all_refuse(pkg, mg, d, STATE, "POISSON")
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=20)[0].converged == 1
    with pkg.Multigrid(n_gpus=2, devices=[0, 0], cut_level=5, **small) as mg:
        all_refuse(pkg, mg, d, STATE, "multi-GPU")
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=20)[0].converged == 1
    with pkg.Multigrid(op=pkg.OPERATOR_STENCIL5, **small) as mg:
        all_refuse(pkg, mg, d, STATE, "STENCIL5")
        mg.set_coefficient(np.ones(((1 << L) + 1,) * 2))
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=30)[0].converged == 1


@pytest.mark.parametrize("dtype", [1, 0])
def test_refused_calls_leave_the_handle_usable(pkg, dtype):
    dt = np_dtype(dtype)
    L, Lc = 6, 3
    n = (1 << L) - 1
    lib = pkg.lib()
    d, u0, g = rand(L, 51, dt, 0.5, 2.0), rand(L, 52, dt), rand(L, 53, dt)
    tol = 1e-8 if dtype == 1 else 1e-4
    ms = C.c_double()

    def expect(code, word, call):
        assert call() == code, word
        assert word in lib.mgx_last_error(mg._h).decode(), (word, lib.mgx_last_error(mg._h).decode())

    def reference_bits(m):
        m.set_guess(u0)
        done, stats, hists = m.theta_steps(2, theta=0.5, g=g, solver="gcr", tol=tol, max_iters=20, restart=3)
        return done, [stats_tuple(s) for s in stats], hists, m.get_solution()

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        set_operator(mg, "five", L)
        mg.set_reaction(d)
        mg.build_galerkin()
        want = reference_bits(mg)
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        # before the finest operator is set
        all_refuse(pkg, mg, d, STATE, "finest operator not set")
        set_operator(mg, "five", L)
        # no term set
        expect(STATE, "no zero-order term", lambda: raw_steps(pkg, mg))
        expect(STATE, "no zero-order term", lambda: lib.mgx_time_theta_rhs(mg._h, 0.5, 1, C.byref(ms)))
        expect(INVALID, "n*n", lambda: lib.mgx_set_reaction(mg._h, d.ctypes.data, n * n - 1))
        with pytest.raises(pkg.MgxError, match="no zero-order term"):
            mg.reaction()
        mg.set_reaction(d)
        # before the build
        expect(STATE, "not built", lambda: raw_steps(pkg, mg))
        mg.build_galerkin()
        for theta in (0.0, -1.0, 1.5, float("nan")):
            expect(INVALID, "theta", lambda: raw_steps(pkg, mg, theta=theta))
            expect(INVALID, "theta", lambda: lib.mgx_time_theta_rhs(mg._h, theta, 1, C.byref(ms)))
        expect(INVALID, "nsteps", lambda: raw_steps(pkg, mg, nsteps=-1))
        expect(INVALID, "solver", lambda: raw_steps(pkg, mg, solver=3))
        expect(INVALID, "tol", lambda: raw_steps(pkg, mg, tol=float("nan")))
        expect(INVALID, "max_iters", lambda: raw_steps(pkg, mg, iters=-1))
        for solver in (pkg.STEP_GCR, pkg.STEP_REFINE_GCR):
            for restart in (0, 9):
                expect(INVALID, "restart", lambda: raw_steps(pkg, mg, solver=solver, restart=restart))
        assert raw_steps(pkg, mg, solver=pkg.STEP_SOLVE, restart=0, iters=0) == 0          # (restart is not looked at)
        # the order of the checks: theta before everything else
        expect(INVALID, "theta", lambda: raw_steps(pkg, mg, theta=2.0, nsteps=-1, solver=7))
        if dtype == 0:
            expect(STATE, "F64", lambda: raw_steps(pkg, mg, solver=pkg.STEP_REFINE_GCR))
        expect(INVALID, "n*n", lambda: lib.mgx_set_reaction(mg._h, d.ctypes.data, n * n + 1))
        got = reference_bits(mg)
        assert got[0] == want[0] == 2 and got[1] == want[1]
        assert all(np.array_equal(p, q) for p, q in zip(got[2], want[2])) and np.array_equal(got[3], want[3])


# ---- 9. the timing entry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["five", "nine"])
def test_timing_the_pass_leaves_u_and_b(pkg, kind):
    L, Lc, dt = 8, 5, np.float64
    d, u, b = rand(L, 61, dt, 0.5, 2.0), rand(L, 62, dt), rand(L, 63, dt)
    with handle(pkg, L, Lc) as mg:
        set_operator(mg, kind, L)
        mg.set_reaction(d)                                   # (the pass needs no hierarchy)
        mg.set_guess(u)
        mg.set_rhs(b)
        for theta in (1.0, 0.5):
            ms = mg.time_theta_rhs(theta, repeats=5)
            assert np.isfinite(ms) and ms > 0.0, (theta, ms)
            assert np.array_equal(mg.get_solution(), u) and np.array_equal(mg.get_level(L, pkg.VEC_B), b)
        # what it wrote into R is the pass without a source (the source grid is still zero)
        mg.build_galerkin()
        Su = -mg.residual(L, u, np.zeros_like(u))
        mg.time_theta_rhs(0.5, repeats=1)
        assert_same(mg.get_level(L, pkg.VEC_R), tr.rhs_pass(Su, u, d, np.zeros_like(u), 0.5), "R after the timed pass")
