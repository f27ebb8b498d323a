"""GPU checks of mgx_solve_pcg (conjugate gradients preconditioned by one V-cycle from zero; csrc/mgx_krylov.hpp)
against the numpy statement of the same algorithm with the oracle's V-cycle as preconditioner (tests/pcg_ref.py).

Tolerances: the device differs from the reference only in the summation order of the dots (the V-cycle is the
oracle's operation for operation), a relative 1e-16 in each scalar.  An update r - alpha q moves the new residual
by about that times the previous one, and every later iteration divides the entry by its reduction factor, so on
the fast-converging cycles (V(10,10), FW16, RB-GS: 1e-2 .. 1e-3 per iteration) the entries below ~1e-8 ||r0||
differ by a few 1e-9 relative (measured: 9e-9 at 4e-11 ||r0||, an absolute 1e-21; at most 1.2e-15 ||r0|| over
the 15 FW16 iterations).  fp64 entries are held to 1e-9 relative plus 1e-14 ||r0|| (the project's history floor is
1e-13 ||r0||), with the same iteration count;
fp32 entries to 1e-3 with the count within one (perturbing the dots by 1e-7 moves fp32 histories by ~2e-4)."""
import ctypes as C

import numpy as np
import pytest

import pcg_ref

pytestmark = pytest.mark.gpu

RTOL64 = 1e-9
RTOL32 = 1e-3


def dev_cfg(cfg, **extra):
    c = dict(cfg)
    c.update(extra)
    return c


def gpu_pcg(pkg, cfg, b, u0=None, a=None, tol=1e-8, max_iters=100, **extra):
    """one handle: set everything, run solve_pcg; returns (stats, history, U after, B before, B after)"""
    with pkg.Multigrid(**dev_cfg(cfg, **extra)) as mg:
        if a is not None:
            mg.set_coefficient(a)
        mg.set_rhs(b)
        if u0 is not None:
            mg.set_guess(u0)
        L = cfg["finest_level"]
        b_before = mg.get_level(L, pkg.VEC_B)
        st, h = mg.solve_pcg(tol=tol, max_iters=max_iters)
        u = mg.get_solution()
        b_after = mg.get_level(L, pkg.VEC_B)
    return st, h, u, b_before, b_after


def assert_hist(h, ref, rtol, floor=1e-14):
    assert len(h) == len(ref), (len(h), len(ref), h, ref)
    err = np.abs(h - ref)
    assert np.all(err <= rtol * ref + floor * ref[0]), (float((err / ref).max()), h, ref)


P511 = dict(finest_level=9, coarsest_level=5, mu0=0, mu1=2, mu2=1, schedule=0)
CASES64 = {
    "511_V21": P511,
    "511_V11": dev_cfg(P511, mu1=1, mu2=1),
    "511_rbgs_V21": dev_cfg(P511, smoother=1),
    "511_fw16_V21": dev_cfg(P511, restrict_mode=1),
    "511_fma_V10_10": dev_cfg(P511, mu1=10, mu2=10, arith=1),
    "4095_V21": dict(finest_level=12, coarsest_level=7, mu0=0, mu1=2, mu2=1, schedule=0),
    "8191_fma_V10_10": dict(finest_level=13, coarsest_level=7, mu0=0, mu1=10, mu2=10, schedule=0, arith=1),
}


@pytest.mark.parametrize("name", list(CASES64))
def test_fp64_poisson_histories_match_the_reference(pkg, po, name):
    cfg = CASES64[name]
    b = po.rhs_sine(cfg["finest_level"])
    x_ref, h_ref, conv_ref, _ = pcg_ref.run(po, cfg, b)
    st, h, u, b0, b1 = gpu_pcg(pkg, cfg, b)
    assert conv_ref and st.converged == 1 and st.cycles == len(h_ref) - 1
    assert_hist(h, h_ref, RTOL64)
    assert np.max(np.abs(u - x_ref)) <= 1e-9 * np.max(np.abs(x_ref))
    assert np.array_equal(b0, b1)                       # B is the caller's b again, bit for bit
    if name == "511_V21":
        assert st.cycles == 9


@pytest.mark.parametrize("op", [0, 1])
def test_fp32_histories_match_the_reference(pkg, po, op):
    cfg = dict(finest_level=9, coarsest_level=5, mu0=0, mu1=2, mu2=1 if op == 0 else 2, schedule=0, dtype=0, op=op)
    b = po.rhs_sine(9)
    a = pcg_ref.contrast_coefficient(9, 10.0) if op == 1 else None
    _, h_ref, conv_ref, _ = pcg_ref.run(po, cfg, b, a_nodes=a, tol=1e-5)
    st, h, u, b0, b1 = gpu_pcg(pkg, cfg, b, a=a, tol=1e-5)
    assert conv_ref and st.converged == 1
    assert abs(len(h) - len(h_ref)) <= 1, (h, h_ref)
    m = min(len(h), len(h_ref))
    assert np.all(np.abs(h[:m] - h_ref[:m]) <= RTOL32 * h_ref[:m]), (h, h_ref)
    assert np.isfinite(u).all() and np.array_equal(b0, b1)


@pytest.mark.parametrize("L,contrast", [(11, 10.0), (9, 100.0)])
def test_stencil5_converges_where_vcycles_do_not(pkg, po, L, contrast):
    cfg = dict(finest_level=L, coarsest_level=5, mu0=0, mu1=2, mu2=2, schedule=0, op=1)
    b = po.rhs_sine(L)
    a = pcg_ref.contrast_coefficient(L, contrast)
    _, h_ref, conv_ref, _ = pcg_ref.run(po, cfg, b, a_nodes=a)
    st, h, u, b0, b1 = gpu_pcg(pkg, cfg, b, a=a)
    assert conv_ref and st.converged == 1
    if contrast == 10.0:
        assert st.cycles == 35
        assert_hist(h, h_ref, RTOL64)
    else:
        assert abs(st.cycles - (len(h_ref) - 1)) <= 2, (st.cycles, len(h_ref) - 1)
    assert pcg_ref.true_residual(b, u, a, L, po) <= 2 * 1e-8 * h[0]
    assert np.array_equal(b0, b1)
    # plain V-cycles from the same guess do not get there in 60 cycles
    with pkg.Multigrid(**cfg) as mg:
        mg.set_coefficient(a)
        mg.set_rhs(b)
        sv, hv = mg.solve(tol=1e-8, max_cycles=60)
    assert sv.converged == 0 and not (hv[-1] <= 1e-8 * hv[0])


def test_state_after_the_call(pkg, po):
    cfg = P511
    L = 9
    b = po.rhs_sine(L)
    u0 = po.fill_uniform(b.shape, 4242)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.set_guess(u0)
        b0 = mg.get_level(L, pkg.VEC_B)
        st, h = mg.solve_pcg(tol=1e-8, max_iters=50)
        u = mg.get_solution()
        assert np.array_equal(mg.get_level(L, pkg.VEC_B), b0)
        rn = mg.residual_norm()
    want = pcg_ref.true_residual(b, u)
    assert abs(rn - want) <= 1e-12 * want, (rn, want)
    x_ref, h_ref, _, _ = pcg_ref.run(po, cfg, b, u0)
    assert_hist(h, h_ref, RTOL64)
    assert np.max(np.abs(u - x_ref)) <= 1e-9 * np.max(np.abs(x_ref))


def test_solve_pcg_solve_on_one_handle_equals_fresh_handles(pkg, po):
    cfg = P511
    b = po.rhs_sine(9)
    u0 = po.fill_uniform(b.shape, 99)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.set_guess(u0)
        s1, h1 = mg.solve(tol=1e-3, max_cycles=3)
        s2, h2 = mg.solve_pcg(tol=1e-6, max_iters=4)
        s3, h3 = mg.solve(tol=1e-12, max_cycles=4)
        u_one = mg.get_solution()
        graphs = mg.graphs_cached()
    assert graphs >= 2                                   # the solve's and the zero-start cycle's graphs
    u = u0
    hs = []
    for step in ("solve", "pcg", "solve"):
        with pkg.Multigrid(**cfg) as mg:
            mg.set_rhs(b)
            mg.set_guess(u)
            if step == "solve":
                _, hh = mg.solve(tol=1e-3 if not hs else 1e-12, max_cycles=3 if not hs else 4)
            else:
                _, hh = mg.solve_pcg(tol=1e-6, max_iters=4)
            u = mg.get_solution()
            hs.append(hh)
    assert np.array_equal(h1, hs[0]) and np.array_equal(h2, hs[1]) and np.array_equal(h3, hs[2])
    assert np.array_equal(u_one, u)


def test_nonzero_start_and_dirichlet_rhs_match_the_reference(pkg, po):
    cfg = P511
    L = 9
    n = (1 << L) - 1
    b = po.rhs_sine(L)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.fill_guess_random(2024)
        u0 = mg.get_solution()
        st, h = mg.solve_pcg(tol=1e-8, max_iters=50)
    assert np.abs(u0).max() > 0.5
    _, h_ref, _, _ = pcg_ref.run(po, cfg, b, u0)
    assert_hist(h, h_ref, RTOL64)
    N = n + 1
    x = np.linspace(0.0, 1.0, N + 1)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs_dirichlet(b, np.sin(np.pi * x), 1.0 + x, x[1:N] ** 2, np.cos(x[1:N]))
        bd = mg.get_level(L, pkg.VEC_B)
        st, h = mg.solve_pcg(tol=1e-8, max_iters=50)
        assert np.array_equal(mg.get_level(L, pkg.VEC_B), bd)
    _, h_ref, conv, _ = pcg_ref.run(po, cfg, bd)
    assert conv and st.converged == 1
    assert_hist(h, h_ref, RTOL64)


def test_zero_rhs_and_zero_iterations(pkg, po):
    cfg = P511
    n = 511
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(np.zeros((n, n)))
        mg.set_guess(np.zeros((n, n)))
        st, h = mg.solve_pcg(tol=1e-8, max_iters=20)
        u = mg.get_solution()
    assert st.converged == 1 and st.cycles == 0 and len(h) == 1 and h[0] == 0.0
    assert np.isfinite(u).all() and not u.any()
    b = po.rhs_sine(9)
    u0 = po.fill_uniform(b.shape, 5)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.set_guess(u0)
        st, h = mg.solve_pcg(tol=1e-8, max_iters=0)
        assert np.array_equal(mg.get_solution(), u0)
    assert len(h) == 1 and st.cycles == 0 and st.converged == 0


@pytest.mark.parametrize("op", [0, 1])
def test_repeated_calls_and_eager_launches_give_the_same_bits(pkg, po, op):
    cfg = dict(finest_level=9, coarsest_level=5, mu0=0, mu1=2, mu2=2, schedule=0, op=op)
    b = po.rhs_sine(9)
    u0 = po.fill_uniform(b.shape, 31)
    a = pcg_ref.contrast_coefficient(9, 10.0) if op == 1 else None
    out = []
    for profile in (0, 0, 1):
        with pkg.Multigrid(**dev_cfg(cfg, profile=profile)) as mg:
            if a is not None:
                mg.set_coefficient(a)
            mg.set_rhs(b)
            for _ in range(2):                           # two calls from the same state on one handle
                mg.set_guess(u0)
                st, h = mg.solve_pcg(tol=1e-8, max_iters=40)
                out.append((h, mg.get_solution()))
    for h, u in out[1:]:
        assert np.array_equal(h, out[0][0]) and np.array_equal(u, out[0][1])


@pytest.mark.parametrize("seed", [None, 7])
@pytest.mark.parametrize("dtype", [1, 0])
def test_breakdown_exit_and_the_solves_after_it(pkg, po, dtype, seed):
    """The negated operator (nodal coefficient -1): every p.Ap is negative, so the first iteration breaks down whatever
    the guess - arithmetic on finite data.  The reference reports a breakdown, a one-entry history and an untouched x.
    Then the positive operator on the same handle: solve_pcg and solve_gcr(restart 2) from the guess are bit for bit
    those of fresh handles, so the breakdown flag left in the scalar block both methods share stops neither."""
    cfg = dict(finest_level=7, coarsest_level=4, mu0=0, mu1=2, mu2=1, op=1, dtype=dtype)
    L = 7
    tol = 1e-8 if dtype == 1 else 1e-5
    b = po.rhs_sine(L)
    u0 = np.zeros_like(b) if seed is None else po.fill_uniform(b.shape, seed)
    minus, plus = -np.ones((129, 129)), np.ones((129, 129))
    x_ref, h_ref, conv_ref, brk_ref = pcg_ref.run(po, cfg, b, u0, a_nodes=minus, tol=tol)
    assert brk_ref and not conv_ref and len(h_ref) == 1 and np.array_equal(x_ref, u0.astype(x_ref.dtype))

    def after(mg, method):
        """one solve with the positive operator from the guess: (history, U)"""
        mg.set_coefficient(plus)
        mg.set_guess(u0)
        st, h = mg.solve_pcg(tol=tol, max_iters=30) if method == "pcg" else mg.solve_gcr(tol=tol, max_iters=30, restart=2)
        assert st.converged == 1
        return h, mg.get_solution()

    with pkg.Multigrid(**cfg) as mg:
        mg.set_coefficient(minus)
        mg.set_rhs(b)
        mg.set_guess(u0)
        u_before, b_before = mg.get_solution(), mg.get_level(L, pkg.VEC_B)
        st, h = mg.solve_pcg(tol=tol, max_iters=30)          # MGX_OK: anything else raises
        msg = pkg.lib().mgx_last_error(mg._h).decode()
        print(f"dtype {dtype} seed {seed}: history {h} (reference {h_ref}), '{msg}'")
        assert st.converged == 0 and st.cycles == 0 and st.history_len == 1
        assert_hist(h, h_ref, RTOL64 if dtype == 1 else RTOL32)
        assert "PCG breakdown at iteration 1" in msg and "p.Ap" in msg
        assert np.array_equal(u_before, u0.astype(u_before.dtype))
        assert np.array_equal(mg.get_solution(), u_before) and np.array_equal(mg.get_level(L, pkg.VEC_B), b_before)
        same_handle = [after(mg, "pcg"), after(mg, "gcr")]
    for method, (h1, u1) in zip(("pcg", "gcr"), same_handle):
        with pkg.Multigrid(**cfg) as mg:
            mg.set_rhs(b)
            h2, u2 = after(mg, method)
        assert np.array_equal(h1, h2) and np.array_equal(u1, u2), method


def test_refusals_leave_the_handle_usable(pkg, po):
    L = pkg.lib()
    st = pkg.binding.Stats()
    hist = np.zeros(4)
    hp = hist.ctypes.data_as(C.POINTER(C.c_double))
    b = po.rhs_sine(7)
    small = dict(finest_level=7, coarsest_level=4, mu0=0, mu1=2, mu2=1, schedule=0)
    with pkg.Multigrid(**dev_cfg(small, dtype=pkg.DTYPE_MIXED)) as mg:
        mg.set_rhs(b)
        assert L.mgx_solve_pcg(mg._h, 1e-8, 3, C.byref(st), hp, 4) == 5
        assert "MIXED" in L.mgx_last_error(mg._h).decode()
        s, h = mg.solve(tol=1e-8, max_cycles=20)
        assert s.converged == 1
    with pkg.Multigrid(**dev_cfg(small, n_gpus=2, devices=[0, 0], cut_level=5)) as mg:
        mg.set_rhs(b)
        assert L.mgx_solve_pcg(mg._h, 1e-8, 3, C.byref(st), hp, 4) == 5
        s, h = mg.solve(tol=1e-8, max_cycles=20)
        assert s.converged == 1
    with pkg.Multigrid(**small) as mg:
        mg.set_rhs(b)
        assert L.mgx_solve_pcg(mg._h, -1.0, 3, C.byref(st), hp, 4) == 1
        assert L.mgx_solve_pcg(mg._h, 1e-8, -1, C.byref(st), hp, 4) == 1
        s, h = mg.solve_pcg(tol=1e-8, max_iters=30)
        assert s.converged == 1
