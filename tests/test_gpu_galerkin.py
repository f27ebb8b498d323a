"""GPU parity of the Galerkin hierarchy (handles with op = MGX_OPERATOR_GALERKIN; csrc/mgx_galerkin.hpp) against the
numpy statement of tests/galerkin_ref.py (pinned by scipy's P^T A P in tests/test_galerkin_cpu.py).
Bit-exact: the coarse operators R A P on every level, their Jacobi splittings, the nine-point sweep and residual.
Residual histories of whole solves: 1e-10 relative per cycle in double, 1e-6 in float (the dense coarsest solve is the
only step that is not bit for bit).  Convergence where the re-discretised STENCIL5 hierarchy diverges."""
import numpy as np
import pytest

import galerkin_ref as gr
import pcg_ref
from test_galerkin_cpu import coefficient
from test_gpu_solve import hist_close

pytestmark = pytest.mark.gpu


def np_dtype(dtype):
    return np.float64 if dtype == 1 else np.float32


def handle(pkg, finest, coarsest, **kw):
    cfg = dict(finest_level=finest, coarsest_level=coarsest, op=pkg.OP_GALERKIN, mu1=2, mu2=2, schedule=0)
    cfg.update(kw)
    return pkg.Multigrid(**cfg)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("mode", [gr.CONSISTENT, gr.FW16])
@pytest.mark.parametrize("kind", ["one", "smooth", "jump"])
@pytest.mark.parametrize("finest,coarsest", [(9, 5), (7, 3)])
def test_hierarchy_is_bit_identical_to_the_reference(pkg, po, finest, coarsest, kind, mode, dtype):
    dt = np_dtype(dtype)
    a = coefficient(finest, kind)
    omega = 0.8
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, finest, finest), finest, coarsest, dt, mode, omega)
    with handle(pkg, finest, coarsest, dtype=dtype, restrict_mode=mode, omega=omega) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        for lv in range(finest, coarsest - 1, -1):
            dinv, r = ref.jac[lv]
            for q in range(9):
                assert np.array_equal(mg.get_stencil9(lv, q), ref.st[lv][q]), (lv, gr.SLOTS[q])
            assert np.array_equal(mg.get_stencil9(lv, 9), dinv), lv
            for q in range(8):
                assert np.array_equal(mg.get_stencil9(lv, 10 + q), r[q]), (lv, gr.SLOTS[1 + q])
        # the finest level is still a five-point level for mgx_get_stencil; the coarse ones are not
        assert np.array_equal(mg.get_stencil(finest, 0), ref.st[finest][0])
        with pytest.raises(pkg.MgxError, match="mgx_get_stencil9"):
            mg.get_stencil(finest - 1, 0)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("mode", [gr.CONSISTENT, gr.FW16])
def test_nine_point_sweep_and_residual_are_bit_identical(pkg, po, dtype, mode):
    """levels 8 (rows longer than one strip, not a multiple of the wave's column span), 6 (one partial strip) and
    4 (n = 15, the coarsest level: the lane edges)"""
    dt = np_dtype(dtype)
    finest, coarsest, omega = 9, 4, 2.0 / 3.0
    a = coefficient(finest, "jump")
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, finest, finest), finest, coarsest, dt, mode, omega)
    with handle(pkg, finest, coarsest, dtype=dtype, restrict_mode=mode, omega=omega) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        for lv in (8, 6, 4):
            n = (1 << lv) - 1
            rng = np.random.default_rng(lv)
            u = rng.uniform(-1, 1, (n, n)).astype(dt)
            b = rng.uniform(-1, 1, (n, n)).astype(dt)
            for mu in (1, 3):
                assert np.array_equal(mg.jacobirelaxation(lv, u, b, mu), gr.jacobi9(u, b, mu, omega, ref.jac[lv])), (lv, mu)
            want = gr.residual9(u, b, ref.st[lv])
            assert np.array_equal(mg.residual(lv, u, b), want), lv
            rn = mg.residual_norm(lv)
            assert abs(rn - po.norm2(want)) <= 1e-12 * rn
        # the finest level keeps the five-point kernels
        n = (1 << finest) - 1
        u = np.random.default_rng(1).uniform(-1, 1, (n, n)).astype(dt)
        b = np.random.default_rng(2).uniform(-1, 1, (n, n)).astype(dt)
        assert np.array_equal(mg.jacobirelaxation(finest, u, b, 2), ref.smooth(finest, u, b, 2))
        assert np.array_equal(mg.residual(finest, u, b), ref.residual(finest, u, b))


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("mu2", [2, 1])
@pytest.mark.parametrize("contrast", [10.0, 100.0])
def test_histories_match_the_reference(pkg, po, contrast, mu2, dtype):
    dt = np_dtype(dtype)
    L = 9
    a = pcg_ref.contrast_coefficient(L, contrast)
    b = po.rhs_constant(L)
    tol, cycles = (1e-8, 90) if dtype == 1 else (1e-8, 14)      # float cannot reach 1e-8: 14 cycles, as tests/test_gpu_var.py
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, 5, dt, mu1=2, mu2=mu2)
    u_ref, h_ref = ref.solve(b, tol=tol, max_cycles=cycles)
    with handle(pkg, L, 5, dtype=dtype, mu2=mu2) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve(tol=tol, max_cycles=cycles)
        u = mg.get_solution()
        assert mg.graphs_cached() >= 1
    print(f"contrast {contrast:g} V(2,{mu2}) dtype {dtype}: {len(h) - 1} cycles (reference {len(h_ref) - 1}), "
          f"max rel. history difference {np.max(np.abs(h[:len(h_ref)] - h_ref[:len(h)]) / h_ref[:len(h)]):.3e}")
    assert len(h) == len(h_ref)
    if dtype == 1:
        assert h_ref[-1] <= tol * h_ref[0], "the reference itself did not converge"
        assert hist_close(h, h_ref), (h, h_ref)
        assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))
    else:
        assert np.allclose(h, h_ref, rtol=1e-6, atol=0), (h, h_ref)


def test_2047_contrast_10_converges_where_stencil5_diverges(pkg):
    """tests/test_gpu_pcg.py records plain STENCIL5 V-cycles diverging on this problem; the CPU statement of the Galerkin
    hierarchy needs 27 cycles with a random right-hand side"""
    L = 11
    n = (1 << L) - 1
    a = pcg_ref.contrast_coefficient(L, 10.0)
    b = np.random.default_rng(3).standard_normal((n, n))
    with handle(pkg, L, 5) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve(tol=1e-8, max_cycles=40)
    print(f"2047^2 contrast 10: {len(h) - 1} cycles, final {h[-1] / h[0]:.3e}")
    assert st.converged and h[-1] <= 1e-8 * h[0] and len(h) - 1 <= 40


@pytest.mark.parametrize("contrast,stencil5_iters", [(10.0, 26), (100.0, 77)])
def test_pcg_takes_fewer_iterations_than_on_stencil5(pkg, po, contrast, stencil5_iters):
    """tests/test_pcg_cpu.py pins 26 / 77 iterations for the re-discretised hierarchy on the same problem"""
    L = 9
    a = pcg_ref.contrast_coefficient(L, contrast)
    b = po.rhs_sine(L)
    coef = po.stencil_from_nodes(a, L, L)
    ref = gr.Hierarchy(po, coef, L, 5)
    zeros = np.zeros_like(b)
    x_ref, h_ref, conv, brk = pcg_ref.pcg(pcg_ref.Operator(coef, np.float64), lambda r: ref.vcycle(L, zeros, r), b, zeros, tol=1e-8, max_iters=100)
    assert conv and not brk
    with handle(pkg, L, 5) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve_pcg(tol=1e-8, max_iters=100)
        x = mg.get_solution()
    print(f"contrast {contrast:g}: {len(h) - 1} PCG iterations (reference {len(h_ref) - 1}, STENCIL5 {stencil5_iters})")
    assert st.converged and len(h) == len(h_ref)
    assert len(h) - 1 < stencil5_iters
    assert pcg_ref.true_residual(b, x, a, L, po) <= 2e-8 * h[0]


def test_graph_replay_is_deterministic(pkg, po):
    L = 8
    a = coefficient(L, "jump")
    b = po.rhs_sine(L)
    with handle(pkg, L, 4) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        out = []
        for _ in range(2):
            mg.set_rhs(b)
            mg.set_guess(np.zeros_like(b))
            st, h = mg.solve(tol=1e-9, max_cycles=12)
            out.append((h, mg.get_solution()))
        assert mg.graphs_cached() >= 1
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_state_machine(pkg, po):
    L = 7
    n = (1 << L) - 1
    with pytest.raises(pkg.MgxError, match="CONSISTENT or FW16"):
        handle(pkg, L, 4, restrict_mode=pkg.RESTRICT_INJECT)
    for bad in (dict(dtype=2), dict(smoother=1), dict(arith=1), dict(coarsest_level=6)):
        with pytest.raises(pkg.MgxError):
            handle(pkg, **dict(dict(finest=L, coarsest=4), **bad))
    with pkg.Multigrid(finest_level=L, coarsest_level=4, op=pkg.OPERATOR_STENCIL5) as mg:
        with pytest.raises(pkg.MgxError, match="GALERKIN"):
            mg.build_galerkin()
    a1, a2 = coefficient(L, "smooth"), coefficient(L, "jump")
    b = po.rhs_sine(L)
    with handle(pkg, L, 4) as mg:
        with pytest.raises(pkg.MgxError, match="finest operator not set"):
            mg.build_galerkin()
        with pytest.raises(pkg.MgxError, match="finest operator not set"):
            mg.vcycle()
        mg.set_coefficient(a1)
        for call in (mg.vcycle, lambda: mg.smooth(L, 1), lambda: mg.solve(max_cycles=1), lambda: mg.solve_pcg(max_iters=1),
                     lambda: mg.get_stencil9(L - 1, 0)):
            with pytest.raises(pkg.MgxError, match="not built"):
                call()
        with pytest.raises(pkg.MgxError, match="only the finest operator"):
            mg.set_stencil(L - 1, *[np.ones((n // 2, n // 2))] * 5)
        mg.build_galerkin()
        mg.set_rhs(b)
        st1, h1 = mg.solve(tol=1e-9, max_cycles=30)
        # a new finest operator invalidates the hierarchy; the rebuilt one is the new problem's, not a stale graph
        mg.set_stencil(L, *po.stencil_from_nodes(a2, L, L))
        with pytest.raises(pkg.MgxError, match="not built"):
            mg.vcycle()
        mg.build_galerkin()
        ref = gr.Hierarchy(po, po.stencil_from_nodes(a2, L, L), L, 4)
        assert np.array_equal(mg.get_stencil9(L - 2, 5), ref.st[L - 2][5])
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        st2, h2 = mg.solve(tol=1e-9, max_cycles=30)
        u_ref, h_ref = ref.solve(b, tol=1e-9, max_cycles=30)
        assert hist_close(h2, h_ref), (h2, h_ref)
        assert not np.array_equal(h1[:2], h2[:2])


def test_constant_coefficient_agrees_with_the_poisson_handle(pkg, po):
    L = 8
    b = po.rhs_sine(L)
    sols = []
    for op in (pkg.OP_GALERKIN, pkg.OPERATOR_POISSON):
        with pkg.Multigrid(finest_level=L, coarsest_level=4, op=op, mu1=2, mu2=2, schedule=0) as mg:
            if op == pkg.OP_GALERKIN:
                mg.set_coefficient(np.ones(((1 << L) + 1, (1 << L) + 1)))
                mg.build_galerkin()
            mg.set_rhs(b)
            st, h = mg.solve(tol=1e-11, max_cycles=40)
            assert st.converged
            sols.append(mg.get_solution())
    # b is the eigenvector of the smallest eigenvalue, so ||e|| / ||u|| <= ||r|| / ||b|| = 1e-11 for either solve
    assert np.linalg.norm(sols[0] - sols[1]) <= 1e-10 * np.linalg.norm(sols[1])
