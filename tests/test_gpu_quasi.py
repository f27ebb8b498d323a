"""GPU tests of mgx_quasi and mgx_time_quasi_pass (include/mgx.h, csrc/mgx_quasi.hpp, csrc/mgx_quasi_host.hpp) against the
numpy statement of tests/quasi_ref.py, which tests/test_quasi_cpu.py pins against mathematics.

Everything is bit for bit: the pass (its right-hand side through the timing entry's R, its five grids through
mgx_get_stencil once an iteration has made them the operator, its norm against mgx_residual_norm of (U = 0, B = b)), and
whole iterations against the host composition {pass in numpy, mgx_set_stencil, mgx_build_galerkin_transfer, mgx_set_rhs,
zero guess, the same solver call, mgx_get_solution, u + lam de in numpy, mgx_residual_norm} on the same handle.

Shapes: a wave covers 62 output lanes, 124 columns in double and 248 in float, so the pass runs at L = 4 (one strip, most
points next to the ring) and at L = 8 in double / L = 9 in float (more than one strip and more than one workgroup).
The rings of the coefficient grids cannot be read through the ABI (mgx_get_stencil returns interiors); the whole-level
checks cover U, B and R."""
import ctypes as C

import numpy as np
import pytest

import quasi_ref as qr
from pcg_ref import contrast_coefficient
from test_gpu_galerkin import assert_same, handle, np_dtype
from test_gpu_theta import JACOBI, SGS, rand, run_solver, stats_tuple, whole_level

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 5                      # MGX_ERR_INVALID, MGX_ERR_STATE
BILINEAR, OPERATOR = 0, 1                  # MGX_TRANSFER_*
K = (1.0, 0.0, 1.0)
METHODS = {"picard": qr.PICARD, "newton": qr.NEWTON}


def smooth_nodes(L):
    """a = 5.5 + 4.5 sin(2 pi x) sin(2 pi y) in [1, 10] on the (N + 1)^2 nodes"""
    x = np.arange((1 << L) + 1) / (1 << L)
    return 5.5 + 4.5 * np.outer(np.sin(2 * np.pi * x), np.sin(2 * np.pi * x))


def smooth_guess(L, dt, amp=0.1):
    x = np.arange(1, 1 << L) / (1 << L)
    return (amp * np.outer(np.sin(np.pi * x), np.sin(2 * np.pi * x))).astype(dt)


def device_norm(mg, b):
    """||b||_2 as the device sums it: mgx_residual_norm of (U = 0, B = b) (any built operator: it meets a zero U)"""
    mg.set_rhs(b)
    mg.set_guess(np.zeros_like(b))
    return mg.residual_norm()


def host_quasi(mg, L, a, k, f, u0, method, transfer, solver, lin_tol, lin_iters, restart, tol, max_iters, max_backtracks):
    """the loop as the caller composes it on the same handle (quasi_ref.quasi around the device's linear solver and the
    device's norm); the result also carries the directions de of the linear solves"""
    des = []

    def solve(op, b, it):
        mg.set_stencil(L, *op)
        mg.build_galerkin(transfer)
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        st, h = run_solver(mg, solver, lin_tol, lin_iters, restart)
        des.append(mg.get_solution())
        return des[-1], stats_tuple(st)

    out = qr.quasi(a, k, f, u0, solve, tol, max_iters, max_backtracks, method=METHODS[method], norm=lambda b: device_norm(mg, b))
    out["des"] = des
    return out


def device_quasi(mg, a, k, f, u0, **kw):
    mg.set_rhs(f)
    mg.set_guess(u0)
    return mg.quasi(a, k, **kw)


def assert_quasi_same(pkg, mg, L, got, want, f, what):
    ns, hist, lin, lam = got
    assert np.array_equal(hist, want["hist"]), (what, hist, want["hist"])
    assert np.array_equal(lam, want["lam"]), (what, lam, want["lam"])
    assert ns.iterations == len(want["lam"]) and ns.history_len == len(want["hist"]) and ns.backtracks == want["backtracks"], what
    assert ns.converged == int(want["converged"]) and ns.initial_residual == want["hist"][0] and ns.final_residual == want["hist"][-1], what
    assert [stats_tuple(s) for s in lin] == want["lin"], what
    assert ns.linear_iterations == sum(s[0] for s in want["lin"]), what
    assert_same(mg.get_solution(), want["u"], (what, "U"))
    assert_same(mg.get_level(L, pkg.VEC_B), f, (what, "B is the caller's f"))


def hierarchy(mg, L, Lc):
    """the operator of every level: the finest level's five grids, nine below it"""
    return [mg.get_stencil(L, q) for q in range(5)] + [mg.get_stencil9(lv, q) for lv in range(L - 1, Lc - 1, -1) for q in range(9)]


# ---- 1. the pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["picard", "newton"])
@pytest.mark.parametrize("dtype, L, Lc", [(1, 4, 3), (1, 8, 5), (0, 4, 3), (0, 9, 5)])
def test_the_pass_is_bit_identical_to_the_reference(pkg, dtype, L, Lc, method):
    """a random nodal a in [1, 10], a guess of a smooth part and noise of 0.01 (a nearly linear problem, so that the full
    step of max_backtracks = 0 passes the test): the first evaluation and a trial with lam = 1.  Then the smooth input whose
    first full step overshoots (f = 250 / N^2: ||F|| grows about fourfold at lam = 1 and falls to about 0.7 at 1/2 with
    exact solves, on every level): a trial with lam = 1/2"""
    dt = np_dtype(dtype)
    N = 1 << L
    m = METHODS[method]
    a = np.random.default_rng(61).uniform(1.0, 10.0, (N + 1, N + 1))
    u0 = (smooth_guess(L, dt) + 0.01 * rand(L, 62, dt)).astype(dt)
    f = ((50.0 / N ** 2) * (1.0 + 0.1 * rand(L, 63, dt))).astype(dt)
    k = (1.25, -0.5, 0.75)
    lin = dict(solver="solve", lin_tol=1e-10 if dtype == 1 else 1e-5, lin_max_iters=40)

    def rings_clean(what, vecs):
        for which in vecs:
            full = whole_level(pkg, mg, L, which).copy()
            full[1:N, 1:N] = 0
            assert not full.any(), (what, which, "ring or padding written")

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        mg.set_coefficient(np.ones((N + 1, N + 1)))
        mg.build_galerkin()
        centre = mg.get_stencil(L, 0)
        _, b0, coefs0, _ = qr.quasi_pass(a, k, f, u0, method=m)
        r0 = device_norm(mg, b0)
        # the first evaluation: max_iters = 0
        ns, hist, _, _ = device_quasi(mg, a, k, f, u0, method=method, max_iters=0, tol=0.0, **lin)
        assert ns.iterations == 0 and ns.history_len == 1 and list(hist) == [r0] and ns.converged == 0
        assert np.array_equal(mg.get_solution(), u0) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        assert np.array_equal(mg.get_stencil(L, 0), centre)
        rings_clean("first evaluation", (pkg.VEC_U, pkg.VEC_B))
        mg.time_quasi_pass(0, method, repeats=1)
        assert_same(mg.get_level(L, pkg.VEC_R), b0, (method, "b of the first evaluation"))
        rings_clean("first evaluation", (pkg.VEC_R,))
        # a step: its operator is what the first evaluation wrote
        ns, hist, lstats, lam = device_quasi(mg, a, k, f, u0, method=method, max_iters=1, max_backtracks=0, tol=0.0, **lin)
        assert ns.iterations == 1 and ns.backtracks == 0 and list(lam) == [1.0] and hist[0] == r0, (ns.iterations, hist)
        for q in range(5):
            assert_same(mg.get_stencil(L, q), coefs0[q], (method, "grid of the first evaluation", q))
        u1 = mg.get_solution()
        assert np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        rings_clean("one step", (pkg.VEC_U, pkg.VEC_B))
        # the trial's right-hand side: the timing entry forms un + 1 * U from the iterate un = u1 and de = U = u1
        mg.time_quasi_pass(1, method, repeats=1)
        assert_same(mg.get_level(L, pkg.VEC_R), qr.quasi_pass(a, k, f, u1, u1, 1.0, m)[1], (method, "b of a trial"))
        rings_clean("trial", (pkg.VEC_R,))
        assert np.array_equal(mg.get_solution(), u1) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        # two steps: the operator of the second is what the accepted trial (lam = 1) of the first wrote
        ns2, hist2, _, lam2 = device_quasi(mg, a, k, f, u0, method=method, max_iters=2, max_backtracks=6, tol=0.0, **lin)
        assert ns2.iterations == 2 and lam2[0] == 1.0 and np.array_equal(hist2[:2], hist)
        trial = [mg.get_stencil(L, q) for q in range(5)]
        # the host composition of the first step on the same handle
        want = host_quasi(mg, L, a, k, f, u0, method, BILINEAR, "solve", lin["lin_tol"], 40, 3, 0.0, 1, 0)
        assert not want["failed"] and want["lin"] == [stats_tuple(lstats[0])]
        assert np.array_equal(hist, want["hist"]), (hist, want["hist"])
        assert_same(u1, want["u"], (method, "U after one step"))
        for q, c in enumerate(qr.quasi_pass(a, k, f, u0, want["des"][0], 1.0, m)[2]):
            assert_same(trial[q], c, (method, "grid of the trial with lam = 1", q))
        # lam = 1/2
        a, u0, f = smooth_nodes(L), smooth_guess(L, dt), np.full((N - 1, N - 1), 250.0 / N ** 2, dtype=dt)
        got1 = device_quasi(mg, a, K, f, u0, method=method, max_iters=1, max_backtracks=4, tol=0.0, **lin)
        assert got1[0].iterations == 1 and list(got1[3]) == [0.5] and got1[0].backtracks == 1, (got1[3], got1[1])
        u1 = mg.get_solution()
        rings_clean("half step", (pkg.VEC_U, pkg.VEC_B))
        got2 = device_quasi(mg, a, K, f, u0, method=method, max_iters=2, max_backtracks=4, tol=0.0, **lin)
        assert got2[0].iterations == 2 and got2[3][0] == 0.5
        trial = [mg.get_stencil(L, q) for q in range(5)]
        want = host_quasi(mg, L, a, K, f, u0, method, BILINEAR, "solve", lin["lin_tol"], 40, 3, 0.0, 1, 4)
        assert np.array_equal(got1[1], want["hist"]) and list(want["lam"]) == [0.5]
        assert_same(u1, want["u"], (method, "U after a half step"))
        for q, c in enumerate(qr.quasi_pass(a, K, f, u0, want["des"][0], 0.5, m)[2]):
            assert_same(trial[q], c, (method, "grid of the trial with lam = 1/2", q))


# ---- 2. three iterations against the host composition ----------------------------------------------------------------------
def problem(L, dt):
    """contrast 10, k = (1, 0, 1), f = 100 / N^2 with 10 % noise, a rough guess of 0.1"""
    N = 1 << L
    return contrast_coefficient(L, 10.0), ((100.0 / N ** 2) * (1.0 + 0.1 * rand(L, 82, dt))).astype(dt), (0.1 * rand(L, 83, dt)).astype(dt)


COMPOSITIONS = [
    (6, "picard", "solve", BILINEAR, "jacobi", None, 1), (6, "picard", "gcr", OPERATOR, "jacobi", None, 1),
    (6, "picard", "refine_gcr", BILINEAR, "jacobi", None, 1), (6, "newton", "solve", OPERATOR, "jacobi", None, 1),
    (6, "newton", "gcr", BILINEAR, "jacobi", None, 1), (6, "newton", "refine_gcr", OPERATOR, "jacobi", None, 1),
    (7, "picard", "solve", OPERATOR, "sgs", None, 1), (7, "newton", "gcr", OPERATOR, "sgs", None, 1),
    (7, "newton", "refine_gcr", BILINEAR, "sgs", None, 1), (7, "picard", "gcr", BILINEAR, "jacobi", "W", 1),
    (7, "newton", "gcr", BILINEAR, "jacobi", "W", 1), (6, "newton", "gcr", OPERATOR, "jacobi", None, 0),
    (7, "picard", "solve", BILINEAR, "jacobi", None, 0),
]


@pytest.mark.parametrize("L, method, solver, transfer, smoother, cycle, dtype", COMPOSITIONS,
                         ids=["-".join(map(str, c)) for c in COMPOSITIONS])
def test_three_iterations_are_the_host_composition(pkg, L, method, solver, transfer, smoother, cycle, dtype):
    Lc, dt = 3, np_dtype(dtype)
    lin_tol = 1e-8 if dtype == 1 else 1e-4
    a, f, u0 = problem(L, dt)
    opts = dict(method=method, solver=solver, transfer=transfer, lin_tol=lin_tol, lin_max_iters=40, restart=3, tol=0.0, max_iters=3,
                max_backtracks=6)
    with handle(pkg, L, Lc, dtype=dtype, **(JACOBI if smoother == "jacobi" else SGS)) as mg:
        if cycle is not None:
            mg.set_cycle(pkg.CYCLE_W)
        got = device_quasi(mg, a, K, f, u0, **opts)           # (no operator and no hierarchy beforehand)
        u_dev = mg.get_solution()
        assert got[0].iterations == 3, (got[0].iterations, pkg.lib().mgx_last_error(mg._h).decode())
        assert_same(mg.get_level(L, pkg.VEC_B), f, "B is the caller's f")
        left = hierarchy(mg, L, Lc)
        want = host_quasi(mg, L, a, K, f, u0, method, transfer, solver, lin_tol, 40, 3, 0.0, 3, 6)
        for x, y in zip(left, hierarchy(mg, L, Lc)):
            assert_same(x, y, "the operator of the last linear solve on every level")
        mg.set_guess(u_dev)
        mg.set_rhs(f)
        assert_quasi_same(pkg, mg, L, got, want, f, (method, solver, transfer))
        assert want["hist"][-1] < want["hist"][0]
        # once more on the handle the composition left, the same bits
        again = device_quasi(mg, a, K, f, u0, **opts)
        assert_quasi_same(pkg, mg, L, again, want, f, (method, solver, transfer, "second call"))


# ---- 3. the line search ------------------------------------------------------------------------------------------------------
def backtracking_input(L):
    N = 1 << L
    n = N - 1
    return contrast_coefficient(L, 10.0), np.full((n, n), 2000.0 / N ** 2), np.zeros((n, n))


@pytest.mark.parametrize("method, iters", [("newton", 5), ("picard", 3)])
def test_the_backtracking_input_backtracks_on_the_device(pkg, method, iters):
    """the input tests/test_quasi_cpu.py pins, at levels 5 .. 3: the first step length is 1/16"""
    L, Lc = 5, 3
    a, f, u0 = backtracking_input(L)
    opts = dict(method=method, solver="solve", lin_tol=1e-8, lin_max_iters=30, tol=1e-10, max_iters=iters, max_backtracks=8)
    with handle(pkg, L, Lc, **JACOBI) as mg:
        got = device_quasi(mg, a, K, f, u0, **opts)
        ns, hist, lin, lam = got
        assert ns.iterations == iters and lam[0] == 1 / 16 and ns.backtracks >= 4, (ns.backtracks, lam, hist)
        if method == "newton":
            assert list(lam[:4]) == [1 / 16, 1 / 8, 1 / 2, 1.0], lam
        u_dev = mg.get_solution()
        want = host_quasi(mg, L, a, K, f, u0, method, BILINEAR, "solve", 1e-8, 30, 3, 1e-10, iters, 8)
        mg.set_guess(u_dev)
        mg.set_rhs(f)
        assert_quasi_same(pkg, mg, L, got, want, f, ("backtracking", method))


@pytest.mark.parametrize("method", ["newton", "picard"])
def test_a_failed_line_search_ends_the_call(pkg, method):
    """one accepted step, then a search that max_backtracks = 2 cannot finish: the operator and the hierarchy are those of
    the last accepted iterate, as a composed handle holds them"""
    L, Lc = 5, 3
    a, f, u0 = backtracking_input(L)
    opts = dict(method=method, solver="solve", transfer=OPERATOR, lin_tol=1e-8, lin_max_iters=30, tol=1e-10)
    with handle(pkg, L, Lc, **JACOBI) as mg, handle(pkg, L, Lc, **JACOBI) as composed:
        ns, hist, lin, lam = device_quasi(mg, a, K, f, u0, max_iters=1, max_backtracks=8, **opts)
        assert ns.iterations == 1 and list(lam) == [1 / 16]
        u1 = mg.get_solution()
        ns, hist, lin, lam = device_quasi(mg, a, K, f, u1, max_iters=10, max_backtracks=2, **opts)     # (MGX_OK: the binding did not raise)
        msg = pkg.lib().mgx_last_error(mg._h).decode()
        assert ns.converged == 0 and ns.iterations == 0 and ns.history_len == 1 and ns.backtracks == 3 and len(lam) == 0
        assert len(lin) == 1 and ns.linear_iterations == lin[0].cycles
        assert "mgx_quasi: step 0" in msg and "line search failed" in msg and "0.25" in msg and repr(float(hist[0]))[:12] in msg, msg
        assert np.array_equal(mg.get_solution(), u1) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        composed.set_stencil(L, *qr.quasi_pass(a, K, f, u1, method=METHODS[method])[2])
        composed.build_galerkin(OPERATOR)
        for x, y in zip(hierarchy(mg, L, Lc), hierarchy(composed, L, Lc)):
            assert_same(x, y, "the operator of the failed step on every level")
        assert mg.transfer == OPERATOR


# ---- 4. state ------------------------------------------------------------------------------------------------------------------
def test_zero_iterations_touch_nothing(pkg):
    L, Lc, dt = 6, 3, np.float64
    a, f, u0 = problem(L, dt)
    with handle(pkg, L, Lc) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin(OPERATOR)
        mg.set_rhs(f)
        mg.set_guess(u0)
        mg.solve(tol=0.0, max_cycles=2)                       # (captures graphs)
        graphs = mg.graphs_cached()
        before = hierarchy(mg, L, Lc)
        for method in ("picard", "newton"):
            for kw in (dict(max_iters=0, tol=0.0), dict(max_iters=5, tol=1.0)):       # (hist[0] <= 1.0 * hist[0])
                ns, hist, lin, lam = device_quasi(mg, a, K, f, u0, method=method, transfer=BILINEAR, **kw)
                assert ns.iterations == 0 and ns.history_len == 1 and len(lin) == 0 and ns.converged == (1 if kw["tol"] else 0)
                assert mg.graphs_cached() == graphs and mg.transfer == OPERATOR
                assert all(np.array_equal(x, y) for x, y in zip(before, hierarchy(mg, L, Lc)))
                assert np.array_equal(mg.get_solution(), u0) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
        assert mg.solve(tol=1e-8, max_cycles=30)[0].converged == 1          # (still built)


@pytest.mark.parametrize("method", ["picard", "newton"])
def test_a_nine_point_level_with_a_reaction_term_ends_in_the_composed_state(pkg, method):
    import nine_ref as nr
    L, Lc, dt = 6, 3, np.float64
    a, f, u0 = problem(L, dt)
    b = rand(L, 92, dt)

    def bits(m):
        m.set_rhs(b)
        m.set_guess(u0)
        st, h = m.solve(tol=0.0, max_cycles=3)
        return h, m.get_solution()

    with handle(pkg, L, Lc) as mg, handle(pkg, L, Lc) as composed:
        mg.set_tensor(*nr.rotated_tensor(L, 45.0, 0.5))
        mg.build_galerkin()
        mg.set_reaction(rand(L, 93, dt, 5.0, 9.0))
        mg.build_galerkin()
        ns, hist, lin, lam = device_quasi(mg, a, K, f, u0, method=method, transfer=OPERATOR, max_iters=1, tol=0.0)
        assert ns.iterations == 1
        composed.set_stencil(L, *qr.quasi_pass(a, K, f, u0, method=METHODS[method])[2])
        composed.build_galerkin(OPERATOR)
        for x, y in zip(hierarchy(mg, L, Lc), hierarchy(composed, L, Lc)):          # (mgx_get_stencil: the level is five-point)
            assert_same(x, y, "operator")
        with pytest.raises(pkg.MgxError, match="no zero-order term"):
            mg.reaction()
        got, want = bits(mg), bits(composed)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def raw_quasi(pkg, mg, a, count=None, **kw):
    B = pkg.binding
    o = dict(k0=1.0, k1=0.0, k2=1.0, method=0, transfer=0, solver=0, lin_tol=1e-8, lin_max_iters=20, restart=3, tol=1e-10, max_iters=3,
             max_backtracks=4)
    o.update(kw)
    opt = B.QuasiOpts(**o)
    return pkg.lib().mgx_quasi(mg._h, C.byref(opt), None if a is None else a.ctypes.data, a.size if count is None else count,
                               None, None, None, None, 0)


def test_refused_handles(pkg, po):
    L, Lc = 7, 4
    a = np.ones(((1 << L) + 1,) * 2)
    small = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, schedule=0)
    b = po.rhs_sine(L)
    lib = pkg.lib()
    ms = C.c_double()

    def all_refuse(mg, word):
        for i, call in enumerate((lambda: raw_quasi(pkg, mg, a), lambda: lib.mgx_time_quasi_pass(mg._h, 0, 0, 1, C.byref(ms)))):
            assert call() == STATE, (word, i)
            assert word in lib.mgx_last_error(mg._h).decode(), (i, lib.mgx_last_error(mg._h).decode())

    with pkg.Multigrid(**small) as mg:
        all_refuse(mg, "POISSON")
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=20)[0].converged == 1
    with pkg.Multigrid(n_gpus=2, devices=[0, 0], cut_level=5, **small) as mg:
        all_refuse(mg, "multi-GPU")
        assert raw_quasi(pkg, mg, a, count=3) == INVALID         # (the argument checks come first)
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=20)[0].converged == 1
    with pkg.Multigrid(op=pkg.OPERATOR_STENCIL5, **small) as mg:
        all_refuse(mg, "STENCIL5")
        mg.set_coefficient(a)
        mg.set_rhs(b)
        assert mg.solve(tol=1e-8, max_cycles=30)[0].converged == 1


@pytest.mark.parametrize("dtype", [1, 0])
def test_refused_calls_leave_the_handle_usable(pkg, dtype):
    dt = np_dtype(dtype)
    L, Lc = 6, 3
    nodes = ((1 << L) + 1) ** 2
    lib = pkg.lib()
    a, f, u0 = problem(L, dt)
    lin_tol = 1e-8 if dtype == 1 else 1e-4
    ms = C.c_double(-1.0)
    nan, inf = float("nan"), float("inf")

    def expect(code, word, call):
        assert call() == code, word
        assert word in lib.mgx_last_error(mg._h).decode(), (word, lib.mgx_last_error(mg._h).decode())

    def reference_bits(m):
        ns, hist, lin, lam = device_quasi(m, a, K, f, u0, method="newton", solver="gcr", lin_tol=lin_tol, lin_max_iters=20, restart=3, tol=0.0,
                                          max_iters=2)
        return ns.iterations, hist, [stats_tuple(s) for s in lin], lam, m.get_solution()

    def same(x, y):
        return x[0] == y[0] == 2 and np.array_equal(x[1], y[1]) and x[2] == y[2] and np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4])

    with handle(pkg, L, Lc, dtype=dtype) as mg:
        want = reference_bits(mg)
    with handle(pkg, L, Lc, dtype=dtype) as mg:
        bad = lambda **kw: (lambda: raw_quasi(pkg, mg, a, **kw))
        expect(STATE, "mgx_quasi first", lambda: lib.mgx_time_quasi_pass(mg._h, 0, 0, 1, C.byref(ms)))
        expect(STATE, "mgx_quasi first", lambda: lib.mgx_time_quasi_pass(mg._h, 1, 1, 1, C.byref(ms)))
        assert ms.value == -1.0
        # NULL opt
        assert lib.mgx_quasi(mg._h, None, a.ctypes.data, a.size, None, None, None, None, 0) == INVALID
        # every INVALID, each with everything after it in the documented order wrong as well
        later = dict()
        chain = [("a_nodes", dict(), True), ("max_backtracks", dict(max_backtracks=31), False), ("mgx_quasi: max_iters", dict(max_iters=-1), False),
                 ("mgx_quasi: tol", dict(tol=nan), False), ("restart", dict(solver=1, restart=9), False),
                 ("lin_max_iters", dict(lin_max_iters=-1), False), ("lin_tol", dict(lin_tol=-1.0), False), ("solver", dict(solver=3), False),
                 ("transfer", dict(transfer=2), False), ("method", dict(method=2), False), ("finite", dict(k1=inf), False)]
        expect(INVALID, "(N + 1)^2", lambda: raw_quasi(pkg, mg, a, count=nodes - 1))
        null_a = False
        for word, kw, is_null in chain:                       # from the last check to the first: each one shadows the earlier ones
            later.update(kw)
            null_a = null_a or is_null
            expect(INVALID, word, lambda: raw_quasi(pkg, mg, None if null_a else a, count=nodes - 1, **later))
        for kw, word in ((dict(k0=nan), "finite"), (dict(k2=-inf), "finite"), (dict(method=-1), "method"), (dict(transfer=-1), "transfer"),
                         (dict(solver=-1), "solver"), (dict(lin_tol=nan), "lin_tol"), (dict(solver=2, restart=0), "restart"),
                         (dict(tol=-1.0), "mgx_quasi: tol"), (dict(max_backtracks=-1), "max_backtracks")):
            expect(INVALID, word, bad(**kw))
        expect(INVALID, "(N + 1)^2", lambda: raw_quasi(pkg, mg, a, count=nodes + 1))
        expect(INVALID, "(N + 1)^2", lambda: raw_quasi(pkg, mg, a, count=((1 << L) - 1) ** 2))
        if dtype == 0:
            expect(STATE, "F64", bad(solver=pkg.STEP_REFINE_GCR))
        expect(STATE, "mgx_quasi first", lambda: lib.mgx_time_quasi_pass(mg._h, 0, 0, 1, C.byref(ms)))      # (no refused call allocated)
        assert raw_quasi(pkg, mg, a, solver=0, restart=0, max_iters=0) == 0                  # (restart is not looked at)
        for step, method, repeats, out in ((2, 0, 1, C.byref(ms)), (-1, 0, 1, C.byref(ms)), (0, 2, 1, C.byref(ms)), (0, -1, 1, C.byref(ms)),
                                           (0, 0, 0, C.byref(ms)), (0, 0, 1, None)):
            expect(INVALID, "mgx_time_quasi_pass", lambda: lib.mgx_time_quasi_pass(mg._h, step, method, repeats, out))
        assert ms.value == -1.0
        assert same(reference_bits(mg), want)


# ---- 6. the timing entry -----------------------------------------------------------------------------------------------------------
def test_timing_the_pass_leaves_u_b_and_the_operator(pkg):
    L, Lc, dt = 8, 5, np.float64
    a, f, u0 = problem(L, dt)
    with handle(pkg, L, Lc) as mg:
        ns, hist, lin, lam = device_quasi(mg, a, K, f, u0, method="newton", max_iters=1, tol=0.0, lin_max_iters=10)
        assert ns.iterations == 1
        u, ops = mg.get_solution(), hierarchy(mg, L, Lc)
        graphs = mg.graphs_cached()
        for method in ("picard", "newton"):
            for step in (0, 1):
                ms = mg.time_quasi_pass(step, method, repeats=5)
                assert np.isfinite(ms) and ms > 0.0, (step, ms)
                assert np.array_equal(mg.get_solution(), u) and np.array_equal(mg.get_level(L, pkg.VEC_B), f)
                assert all(np.array_equal(x, y) for x, y in zip(ops, hierarchy(mg, L, Lc))) and mg.graphs_cached() == graphs
        # the next call starts from the iterate it was left with: the same bits as a fresh second step
        got = device_quasi(mg, a, K, f, u, method="newton", max_iters=1, tol=0.0, lin_max_iters=10)
        assert got[1][0] == hist[1]
