"""GPU parity of the Chebyshev smoother (cfg.smoother = MGX_SMOOTHER_CHEBYSHEV, csrc/mgx_cheby.hpp) against the numpy
statement of tests/cheby_ref.py (whose properties tests/test_cheby_cpu.py checks).
Bit-exact: a block of degree 1..4 on a five-point finest level and on nine-point Galerkin levels, the bound g_l on every
level.  Residual histories of whole solves: the tolerances of tests/test_gpu_galerkin.py (hist_close and 1e-10 on the
solution in double, 1e-6 relative in float; the dense coarsest solve is the only step that is not bit for bit), cycle
counts equal.  mgx_solve_pcg, graph replay against eager launches, the refusals."""
import numpy as np
import pytest

import cheby_ref as cr
import galerkin_ref as gr
import hipmem as hm
import opdep_ref as od
import pcg_ref
from test_galerkin_cpu import random_stencil5, with_ring_values
from test_gpu_galerkin import assert_same, np_dtype
from test_gpu_pcg import RTOL64
from test_gpu_solve import hist_close

pytestmark = pytest.mark.gpu

BILINEAR, OPERATOR = od.BILINEAR, od.OPERATOR
REF = {BILINEAR: cr.Hierarchy, OPERATOR: cr.OpdepHierarchy}


def handle(pkg, finest, coarsest, **kw):
    cfg = dict(finest_level=finest, coarsest_level=coarsest, op=pkg.OP_GALERKIN, smoother=pkg.SMOOTHER_CHEBYSHEV, mu1=2, mu2=2, schedule=0)
    cfg.update(kw)
    return pkg.Multigrid(**cfg)


def full_grid(pkg, mg, level, which):
    """a level vector as the library holds it: rows 0..N times the pitch, ring and padding included"""
    N = 1 << level
    pitch = pkg.lib().mgx_level_pitch(level, mg.cfg.dtype)
    out = hm.zeros((N + 1, pitch), mg.level_dtype(level))
    mg.get_level_device(level, which, out.data_ptr())
    return out.numpy()


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR])
def test_a_block_is_bit_identical_to_the_reference(pkg, po, transfer, dtype):
    """(9, 4) from a seeded non-symmetric operator (g_l differs from level to level and from 2): the five-point finest
    level 9, the nine-point levels 8 (rows longer than one strip), 6 (one partial strip) and 4 (n = 15: the lane edges);
    degrees 1..4 end in either buffer of the ping-pong.  The ring and the padding of U stay zero."""
    dt = np_dtype(dtype)
    finest, coarsest, omega = 9, 4, 0.8
    st5 = [x.astype(dt) for x in random_stencil5(finest, 31)]
    ref = REF[transfer](po, st5, finest, coarsest, dt, omega=omega)
    with handle(pkg, finest, coarsest, dtype=dtype, omega=omega) as mg:
        mg.set_stencil(finest, *st5)
        mg.build_galerkin(transfer)
        for lv in (9, 8, 6, 4):
            n = (1 << lv) - 1
            rng = np.random.default_rng(100 + lv)
            u, b = rng.uniform(-1, 1, (n, n)).astype(dt), rng.uniform(-1, 1, (n, n)).astype(dt)
            for mu in (1, 2, 3, 4):
                assert_same(mg.jacobirelaxation(lv, u, b, mu), ref.smooth(lv, u, b, mu), ("transfer", transfer, "level", lv, "degree", mu))
                g = full_grid(pkg, mg, lv, pkg.VEC_U)
                assert not g[0].any() and not g[n + 1].any() and not g[:, 0].any() and not g[:, n + 1:].any(), (lv, mu)


@pytest.mark.parametrize("dtype", [1, 0])
def test_a_block_on_stencil5_levels_is_bit_identical(pkg, po, dtype):
    """op = STENCIL5: every level is a five-point level of the caller's"""
    dt = np_dtype(dtype)
    finest, coarsest = 8, 4
    sts = {lv: [x.astype(dt) for x in random_stencil5(lv, 40 + lv)] for lv in range(coarsest, finest + 1)}
    ref = cr.Stencil5Cheby(po, sts, finest, coarsest, dt)
    with pkg.Multigrid(finest_level=finest, coarsest_level=coarsest, op=pkg.OPERATOR_STENCIL5, smoother=pkg.SMOOTHER_CHEBYSHEV, dtype=dtype) as mg:
        for lv in sts:
            mg.set_stencil(lv, *sts[lv])
        for lv in (8, 5):
            n = (1 << lv) - 1
            rng = np.random.default_rng(lv)
            u, b = rng.uniform(-1, 1, (n, n)).astype(dt), rng.uniform(-1, 1, (n, n)).astype(dt)
            assert mg.lambda_max(lv) == ref.g[lv]
            for mu in (1, 3):
                assert_same(mg.jacobirelaxation(lv, u, b, mu), ref.smooth(lv, u, b, mu), ("level", lv, "degree", mu))


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR])
def test_lambda_max_equals_the_reference_on_every_level(pkg, po, transfer, dtype):
    """... for either smoother, and with values up to 1e30 of mixed sign in the coefficients that point at the ring"""
    dt = np_dtype(dtype)
    finest, coarsest = 9, 4
    st5 = [x.astype(dt) for x in random_stencil5(finest, 51)]
    junk = [x.astype(dt) for x in with_ring_values(st5, 52)]
    ref = REF[transfer](po, st5, finest, coarsest, dt)
    assert len({ref.g[lv] for lv in ref.g}) > 1 and all(g != 2.0 for g in ref.g.values())
    for smoother in (pkg.SMOOTHER_CHEBYSHEV, pkg.SMOOTHER_JACOBI):
        for op in (st5, junk):
            with handle(pkg, finest, coarsest, dtype=dtype, smoother=smoother) as mg:
                mg.set_stencil(finest, *op)
                with pytest.raises(pkg.MgxError, match="not built"):
                    mg.lambda_max(finest)
                mg.build_galerkin(transfer)
                for lv in range(coarsest, finest + 1):
                    assert mg.lambda_max(lv) == ref.g[lv], (smoother, lv, mg.lambda_max(lv), ref.g[lv])
                with pytest.raises(pkg.MgxError, match="out of range"):
                    mg.lambda_max(coarsest - 1)


def test_lambda_max_states_and_the_constant_stencil(pkg, po):
    L = 7
    with pkg.Multigrid(finest_level=L, coarsest_level=4) as mg:
        with pytest.raises(pkg.MgxError, match="POISSON"):
            mg.lambda_max(L)
    with pkg.Multigrid(finest_level=L, coarsest_level=4, op=pkg.OPERATOR_STENCIL5, smoother=pkg.SMOOTHER_CHEBYSHEV) as mg:
        with pytest.raises(pkg.MgxError, match="not set"):
            mg.lambda_max(L)
        mg.set_coefficient(np.ones(((1 << L) + 1, (1 << L) + 1)))
        assert [mg.lambda_max(lv) for lv in range(4, L + 1)] == [2.0] * 4


def test_a_new_operator_changes_lambda_max_and_the_next_solve_is_the_new_problem_s(pkg, po):
    """a cycle captured into a graph holds the Chebyshev scalars of the old g_l: a rebuild must drop it"""
    L, Lc = 8, 4
    n = (1 << L) - 1
    b = np.random.default_rng(1).uniform(-1, 1, (n, n))
    op1, op2 = random_stencil5(L, 61), random_stencil5(L, 62, c_lo=3.5, c_hi=6.0)

    def solve(mg):
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        return mg.solve(tol=1e-9, max_cycles=5)[1]

    with handle(pkg, L, Lc) as fresh:
        fresh.set_stencil(L, *op2)
        fresh.build_galerkin()
        g2 = [fresh.lambda_max(lv) for lv in range(Lc, L + 1)]
        h2 = solve(fresh)
    with handle(pkg, L, Lc) as mg:
        mg.set_stencil(L, *op1)
        mg.build_galerkin()
        g1 = [mg.lambda_max(lv) for lv in range(Lc, L + 1)]
        h1 = solve(mg)
        assert mg.graphs_cached() >= 1
        mg.set_stencil(L, *op2)
        mg.build_galerkin()
        assert [mg.lambda_max(lv) for lv in range(Lc, L + 1)] == g2 and all(x != y for x, y in zip(g1, g2))
        assert np.array_equal(solve(mg), h2) and not np.array_equal(h1[:3], h2[:3])
    # STENCIL5: mgx_set_stencil rebuilds the level at once
    sts1 = {lv: random_stencil5(lv, 70 + lv) for lv in range(Lc, L + 1)}
    sts2 = {lv: random_stencil5(lv, 80 + lv, c_lo=3.5, c_hi=6.0) for lv in range(Lc, L + 1)}
    kw = dict(finest_level=L, coarsest_level=Lc, op=pkg.OPERATOR_STENCIL5, smoother=pkg.SMOOTHER_CHEBYSHEV, mu1=2, mu2=2, schedule=0)
    with pkg.Multigrid(**kw) as fresh:
        for lv in sts2:
            fresh.set_stencil(lv, *sts2[lv])
        h2 = solve(fresh)
    with pkg.Multigrid(**kw) as mg:
        for lv in sts1:
            mg.set_stencil(lv, *sts1[lv])
        g1 = mg.lambda_max(L)
        solve(mg)
        for lv in sts2:
            mg.set_stencil(lv, *sts2[lv])
        assert mg.lambda_max(L) != g1
        assert np.array_equal(solve(mg), h2)


def reference(po, op, transfer, a, L, Lc, dt, mu1, mu2):
    if op == "stencil5":
        return cr.Stencil5Cheby(po, {lv: po.stencil_from_nodes(a, lv, L) for lv in range(Lc, L + 1)}, L, Lc, dt, mu1=mu1, mu2=mu2)
    return REF[transfer](po, po.stencil_from_nodes(a, L, L), L, Lc, dt, mu1=mu1, mu2=mu2)


HISTORY_CASES = [(op, transfer, schedule, mu, contrast, dtype)
                 for dtype in (1, 0) for op, transfer in (("stencil5", None), ("galerkin", BILINEAR), ("galerkin", OPERATOR))
                 for schedule in (gr.V, gr.FMG) for mu in ((2, 2), (3, 1)) for contrast in (10.0, 100.0)]


@pytest.mark.parametrize("op,transfer,schedule,mu,contrast,dtype", HISTORY_CASES,
                         ids=["-".join(map(str, (c[0], c[1], "fmg" if c[2] else "v", *c[3], int(c[4]), "f64" if c[5] else "f32"))) for c in HISTORY_CASES])
def test_histories_match_the_reference(pkg, po, op, transfer, schedule, mu, contrast, dtype):
    """levels 9..5, the contrast problems of tests/pcg_ref.py, to 1e-8 in double, within 90 cycles for GALERKIN as
    tests/test_gpu_galerkin.py and 40 for STENCIL5 (the re-discretised hierarchy does not converge on them, and diverges
    at contrast 100: tests/test_gpu_pcg.py; its history is compared over the 40 cycles all the same); 14 cycles in float
    (which cannot reach 1e-8), as tests/test_gpu_galerkin.py"""
    dt = np_dtype(dtype)
    L, Lc = 9, 5
    a = pcg_ref.contrast_coefficient(L, contrast)
    b = po.rhs_constant(L)
    tol, cycles = (1e-8, 40 if op == "stencil5" else 90) if dtype == 1 else (1e-8, 14)
    ref = reference(po, op, transfer, a, L, Lc, dt, *mu)
    u_ref, h_ref = ref.solve(b, tol=tol, max_cycles=cycles, schedule=schedule)
    kw = dict(dtype=dtype, mu1=mu[0], mu2=mu[1], schedule=schedule, mu0=0)
    if op == "stencil5":
        kw["op"] = pkg.OPERATOR_STENCIL5
    with handle(pkg, L, Lc, **kw) as mg:
        mg.set_coefficient(a)
        if op == "galerkin":
            mg.build_galerkin(transfer)
        mg.set_rhs(b)
        st, h = mg.solve(tol=tol, max_cycles=cycles)
        u = mg.get_solution()
    m = min(len(h), len(h_ref))
    print(f"{op} transfer {transfer} schedule {schedule} V{mu} contrast {contrast:g} dtype {dtype}: {len(h) - 1} cycles (reference "
          f"{len(h_ref) - 1}), final {h[-1] / h[0]:.3e}, max rel. history difference {np.max(np.abs(h[:m] - h_ref[:m]) / h_ref[:m]):.3e}")
    assert len(h) == len(h_ref)
    assert np.isfinite(h_ref).all()
    if dtype == 1:
        assert hist_close(h, h_ref), (h, h_ref)
        assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))
    else:
        assert np.allclose(h, h_ref, rtol=1e-6, atol=0), (h, h_ref)


@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR])
def test_pcg_with_the_chebyshev_cycle(pkg, po, transfer):
    """V(2,2) with mu1 = mu2 is a symmetric preconditioner: contrast 100 at 511^2, tol 1e-8"""
    L = 9
    a = pcg_ref.contrast_coefficient(L, 100.0)
    b = po.rhs_sine(L)
    coef = po.stencil_from_nodes(a, L, L)
    ref = REF[transfer](po, coef, L, 5)
    zeros = np.zeros_like(b)
    x_ref, h_ref, conv, brk = pcg_ref.pcg(pcg_ref.Operator(coef, np.float64), lambda r: ref.vcycle(L, zeros, r), b, zeros, tol=1e-8, max_iters=100)
    assert conv and not brk
    with handle(pkg, L, 5) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin(transfer)
        mg.set_rhs(b)
        st, h = mg.solve_pcg(tol=1e-8, max_iters=100)
        x = mg.get_solution()
    m = min(len(h), len(h_ref))
    print(f"transfer {transfer}: {len(h) - 1} PCG iterations (reference {len(h_ref) - 1}), max rel. history difference "
          f"{np.max(np.abs(h[:m] - h_ref[:m]) / h_ref[:m]):.3e}")
    assert st.converged == 1 and abs(len(h) - len(h_ref)) <= 1, (h, h_ref)
    assert np.all(np.abs(h[:m] - h_ref[:m]) <= RTOL64 * h_ref[:m] + 1e-14 * h_ref[0]), (h, h_ref)
    assert pcg_ref.true_residual(b, x, a, L, po) <= 2e-8 * h[0]


def test_graph_replay_and_eager_launches_give_the_same_bits(pkg, po):
    """profile 0 replays the cycle from a graph, profile 1 launches every kernel eagerly"""
    L = 8
    a = pcg_ref.contrast_coefficient(L, 100.0)
    b = po.rhs_sine(L)
    out = []
    for profile in (0, 0, 1):
        with handle(pkg, L, 4, profile=profile, mu1=3, mu2=2) as mg:
            mg.set_coefficient(a)
            mg.build_galerkin(OPERATOR)
            runs = []
            for _ in range(2):
                mg.set_rhs(b)
                mg.set_guess(np.zeros_like(b))
                st, h = mg.solve(tol=1e-9, max_cycles=12)
                runs.append((h, mg.get_solution()))
            assert mg.graphs_cached() >= 1 if profile == 0 else mg.graphs_cached() == -1
            assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
            out.append(runs[0])
    for h, u in out[1:]:
        assert np.array_equal(h, out[0][0]) and np.array_equal(u, out[0][1])


def test_time_smoother_runs_one_block(pkg, po):
    L = 8
    a = pcg_ref.contrast_coefficient(L, 10.0)
    n = (1 << L) - 1
    rng = np.random.default_rng(3)
    u, b = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    ref = cr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, 4)
    with handle(pkg, L, 4) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_guess(u)
        mg.set_rhs(b)
        assert mg.time_smoother(3) > 0.0
        assert_same(mg.get_solution(), ref.smooth(L, u, b, 3), "mgx_time_smoother(3)")


def test_refusals_name_the_smoother_and_leave_a_jacobi_handle_usable(pkg, po):
    L, Lc = 7, 4
    a = pcg_ref.contrast_coefficient(L, 10.0)
    b = po.rhs_sine(L)
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, Lc)
    u_ref, h_ref = ref.solve(b, tol=1e-9, max_cycles=4)
    cheb = pkg.SMOOTHER_CHEBYSHEV

    def jacobi_still_solves():
        with pkg.Multigrid(finest_level=L, coarsest_level=Lc, op=pkg.OP_GALERKIN, mu1=2, mu2=2, schedule=0) as mg:
            mg.set_coefficient(a)
            mg.build_galerkin()
            mg.set_rhs(b)
            st, h = mg.solve(tol=1e-9, max_cycles=4)
            assert hist_close(h, h_ref), (h, h_ref)

    refused = [
        dict(op=pkg.OPERATOR_POISSON),
        dict(op=pkg.OPERATOR_POISSON, n_gpus=2),
        dict(op=pkg.OP_GALERKIN, n_gpus=2),
        dict(op=pkg.OPERATOR_STENCIL5, n_gpus=2),
        dict(op=pkg.OP_GALERKIN, dtype=pkg.DTYPE_MIXED),
        dict(op=pkg.OPERATOR_STENCIL5, dtype=pkg.DTYPE_MIXED),
        dict(op=pkg.OP_GALERKIN, arith=pkg.ARITH_FMA),
        dict(op=pkg.OPERATOR_STENCIL5, arith=pkg.ARITH_FMA),
    ]
    for bad in refused:
        with pytest.raises(pkg.MgxError, match="invalid argument.*CHEBYSHEV"):
            pkg.Multigrid(finest_level=L, coarsest_level=Lc, smoother=cheb, **bad)
        jacobi_still_solves()
    with pytest.raises(pkg.MgxError, match="invalid argument.*CHEBYSHEV"):
        pkg.Multigrid.rank(0, 2, finest_level=L, coarsest_level=Lc, smoother=cheb)
    with pytest.raises(pkg.MgxError, match="CHEBYSHEV"):
        pkg.Plan(2, 0, finest_level=9, coarsest_level=5, smoother=cheb)
    with pytest.raises(pkg.MgxError):
        pkg.Multigrid(finest_level=L, coarsest_level=Lc, smoother=3, op=pkg.OP_GALERKIN)
    jacobi_still_solves()
    # the slab entry point that takes a smoother argument
    n_rows = (1 << L) + 1
    pitch = pkg.lib().mgx_level_pitch(L, pkg.DTYPE_F64)
    slab = pkg.Slab(L, pkg.DTYPE_F64, n_rows, 0, 0)
    u, f, t = (hm.zeros((n_rows, pitch), np.float64) for _ in range(3))
    rc = pkg.lib().mgx_slab_cycle(slab, u.data_ptr(), f.data_ptr(), t.data_ptr(), 1, n_rows - 1, 2, 2.0 / 3.0, cheb, None, None, None,
                                  0, 0, 0, 0, None, None, None, None)
    assert rc == 1                                   # MGX_ERR_INVALID
    jacobi_still_solves()
