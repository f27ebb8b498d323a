"""GPU parity of the Galerkin hierarchy (handles with op = MGX_OPERATOR_GALERKIN; csrc/mgx_galerkin.hpp) against the
numpy statement of tests/galerkin_ref.py (pinned by scipy's P^T A P in tests/test_galerkin_cpu.py).
Bit-exact: the coarse operators R A P on every level, their Jacobi splittings, the nine-point sweep and residual.
Residual histories of whole solves: 1e-10 relative per cycle in double, 1e-6 in float (the dense coarsest solve is the
only step that is not bit for bit).  Convergence where the re-discretised STENCIL5 hierarchy diverges.
The shapes: a wave covers 62 output lanes, 124 columns in double and 248 in float, so the bit-exact comparisons run up
to finest level 11 (five strips in the first nine-point product R A P, nine in a sweep on level 10) and down to n = 3.
The inputs: non-symmetric user operators, arbitrary values in the ring-pointing coefficients.  The schedules: FMG,
bottom = SMOOTH, V-cycles from an intermediate level, mgx_vcycle_zero, the transfer operators, a seeded fuzz."""
import ctypes as C

import numpy as np
import pytest

import galerkin_ref as gr
import pcg_ref
from test_galerkin_cpu import coefficient, random_stencil5, with_ring_values
from test_gpu_pcg import RTOL32, RTOL64, assert_hist
from test_gpu_solve import hist_close

pytestmark = pytest.mark.gpu


def np_dtype(dtype):
    return np.float64 if dtype == 1 else np.float32


def assert_same(got, want, what):
    """np.array_equal, and on a mismatch the first differing (row, column) in grid indices (interior index + 1) with
    that column modulo the 62 output lanes of a wave (124 columns in double, 248 in float): a strip seam names itself"""
    if np.array_equal(got, want):
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    span = 124 if want.dtype == np.float64 else 248
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    row, col = int(bad[0][0]) + 1, int(bad[0][1]) + 1
    raise AssertionError(f"{what}: {len(bad)} of {got.size} differ, first at (row {row}, column {col}), column % {span} = {col % span}: "
                         f"got {got[row - 1, col - 1]!r}, want {want[row - 1, col - 1]!r}")


def assert_hierarchy(mg, ref, levels, what=()):
    """operators (slots 0..8), D_inv (9) and the off-diagonals of R_omega (10..17) of `levels`, bit for bit"""
    for lv in levels:
        dinv, r = ref.jac[lv]
        for q in range(9):
            assert_same(mg.get_stencil9(lv, q), ref.st[lv][q], (*what, "level", lv, "slot", gr.SLOTS[q]))
        assert_same(mg.get_stencil9(lv, 9), dinv, (*what, "level", lv, "D_inv"))
        for q in range(8):
            assert_same(mg.get_stencil9(lv, 10 + q), r[q], (*what, "level", lv, "R", gr.SLOTS[1 + q]))


def handle(pkg, finest, coarsest, **kw):
    cfg = dict(finest_level=finest, coarsest_level=coarsest, op=pkg.OP_GALERKIN, mu1=2, mu2=2, schedule=0)
    cfg.update(kw)
    return pkg.Multigrid(**cfg)


# (11, 5): the first nine-point product has NC = 512, five strips in double and three in float (middle strips with a
# real neighbour strip on both sides), "jump" and "smooth" only for the time; (10, 4): NC = 256; (6, 2): n = 3 on the
# coarsest level, where every off-centre coefficient of the centre point's neighbours touches the ring; (4, 4): no
# nine-point level at all
HIERARCHY_CASES = [(f, c, kind, mode, dtype)
                   for dtype in (1, 0) for mode in (gr.CONSISTENT, gr.FW16) for kind in ("one", "smooth", "jump")
                   for f, c in [(9, 5), (7, 3), (11, 5), (10, 4), (6, 2), (4, 4)] if (f, c) != (11, 5) or kind != "one"]


@pytest.mark.parametrize("finest,coarsest,kind,mode,dtype", HIERARCHY_CASES, ids=["-".join(map(str, c)) for c in HIERARCHY_CASES])
def test_hierarchy_is_bit_identical_to_the_reference(pkg, po, finest, coarsest, kind, mode, dtype):
    dt = np_dtype(dtype)
    a = coefficient(finest, kind)
    omega = 0.8
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, finest, finest), finest, coarsest, dt, mode, omega)
    with handle(pkg, finest, coarsest, dtype=dtype, restrict_mode=mode, omega=omega) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        assert_hierarchy(mg, ref, range(finest, coarsest - 1, -1))
        # the finest level is still a five-point level for mgx_get_stencil; the coarse ones are not
        assert np.array_equal(mg.get_stencil(finest, 0), ref.st[finest][0])
        if finest > coarsest:
            with pytest.raises(pkg.MgxError, match="mgx_get_stencil9"):
                mg.get_stencil(finest - 1, 0)


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("mode", [gr.CONSISTENT, gr.FW16])
def test_nine_point_sweep_and_residual_are_bit_identical(pkg, po, dtype, mode):
    """(9, 4): levels 8 (rows longer than one strip, not a multiple of the wave's column span), 6 (one partial strip)
    and 4 (n = 15, the coarsest level: the lane edges).  (11, 3): levels 10 (nine strips in double, five in float:
    middle strips), 9, 7, 5 and 3 (n = 7, fewer columns than one float lane pair); mu = 1, 2, 5 ends in either buffer
    of the ping-pong"""
    dt = np_dtype(dtype)
    omega = 2.0 / 3.0
    for finest, coarsest, levels, mus in [(9, 4, (8, 6, 4), (1, 3)), (11, 3, (10, 9, 7, 5, 3), (1, 2, 5))]:
        a = coefficient(finest, "jump")
        ref = gr.Hierarchy(po, po.stencil_from_nodes(a, finest, finest), finest, coarsest, dt, mode, omega)
        with handle(pkg, finest, coarsest, dtype=dtype, restrict_mode=mode, omega=omega) as mg:
            mg.set_coefficient(a)
            mg.build_galerkin()
            for lv in levels:
                n = (1 << lv) - 1
                rng = np.random.default_rng(lv)
                u = rng.uniform(-1, 1, (n, n)).astype(dt)
                b = rng.uniform(-1, 1, (n, n)).astype(dt)
                for mu in mus:
                    assert_same(mg.jacobirelaxation(lv, u, b, mu), gr.jacobi9(u, b, mu, omega, ref.jac[lv]), (finest, "level", lv, "mu", mu))
                want = gr.residual9(u, b, ref.st[lv])
                assert_same(mg.residual(lv, u, b), want, (finest, "level", lv, "residual"))
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
    assert_hist(h, h_ref, RTOL64)
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


# ---- user-supplied finest operators ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("finest", [9, 10])
def test_a_non_symmetric_operator_and_whatever_its_ring_coefficients_hold(pkg, po, finest, dtype):
    """mgx_set_stencil with a seeded non-symmetric operator (c in [3, 5], every off-diagonal on its own in [-1, -0.5]).
    (a) hierarchy, splittings, one sweep per level and a 3-cycle history against the reference;
    (b) the same operator with large finite values of mixed sign (up to 1e30) in the coefficients that point at the
    Dirichlet ring: mgx.h says they are ignored, so every coarse operator and splitting and the iterates are THE SAME
    bits (on the finest level mgx_get_stencil may return what the caller gave)"""
    dt = np_dtype(dtype)
    coarsest = 4
    n = (1 << finest) - 1
    st5 = [x.astype(dt) for x in random_stencil5(finest, 100 + finest)]
    junk = [x.astype(dt) for x in with_ring_values(st5, 200 + finest)]
    assert np.isfinite(junk).all() and np.max(np.abs(junk[1][0])) > 1e20
    b = np.random.default_rng(finest).uniform(-1, 1, (n, n)).astype(dt)
    ref = gr.Hierarchy(po, st5, finest, coarsest, dt)
    u_ref, h_ref = ref.solve(b, tol=0.0, max_cycles=3)
    assert len(h_ref) == 4 and np.all(np.diff(h_ref) < 0), "the reference itself does not reduce the residual"
    out = []
    for name, op in (("natural", st5), ("ring values", junk)):
        with handle(pkg, finest, coarsest, dtype=dtype) as mg:
            mg.set_stencil(finest, *op)
            mg.build_galerkin()
            coarse = {(lv, q): mg.get_stencil9(lv, q) for lv in range(coarsest, finest) for q in range(18)}
            if name == "natural":
                assert_hierarchy(mg, ref, range(finest, coarsest - 1, -1), (name,))
                for lv in range(finest, coarsest - 1, -1):
                    m = (1 << lv) - 1
                    rng = np.random.default_rng(10 * finest + lv)
                    v, f = rng.uniform(-1, 1, (m, m)).astype(dt), rng.uniform(-1, 1, (m, m)).astype(dt)
                    assert_same(mg.jacobirelaxation(lv, v, f, 1), ref.smooth(lv, v, f, 1), (name, "sweep on level", lv))
            mg.set_rhs(b)
            mg.set_guess(np.zeros_like(b))
            st, h = mg.solve(tol=0.0, max_cycles=3)
            out.append((coarse, h, mg.get_solution()))
    (coarse_a, h_a, u_a), (coarse_b, h_b, u_b) = out
    print(f"finest {finest} dtype {dtype}: history {h_a}, reference {h_ref}")
    if dtype == 1:
        assert hist_close(h_a, h_ref), (h_a, h_ref)
        assert np.max(np.abs(u_a - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))
    else:
        assert len(h_a) == len(h_ref) and np.allclose(h_a, h_ref, rtol=1e-6, atol=0), (h_a, h_ref)
    for (lv, q), want in coarse_a.items():
        assert_same(coarse_b[lv, q], want, ("ring values: level", lv, "array", q))
    assert np.array_equal(h_b, h_a), (h_b, h_a)
    assert_same(u_b, u_a, "ring values: solution after 3 cycles")


# ---- schedules and entry points -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("mode", [gr.CONSISTENT, gr.FW16])
def test_transfer_and_bottom_operators_on_nine_point_levels(pkg, po, dtype, mode):
    """mgx_restrict_rhs, mgx_restrict, mgx_prolong, mgx_prolong_add from a nine-point level (7 -> 6) and onto / from the
    coarsest one (5 -> 4), bit for bit; mgx_bottom_solve to the solution tolerance"""
    dt = np_dtype(dtype)
    finest, coarsest = 9, 4
    a = coefficient(finest, "jump")
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, finest, finest), finest, coarsest, dt, mode)
    with handle(pkg, finest, coarsest, dtype=dtype, restrict_mode=mode) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        for lv in (7, 5):
            n, nc = (1 << lv) - 1, (1 << (lv - 1)) - 1
            rng = np.random.default_rng(70 + lv)
            v, f = rng.uniform(-1, 1, (n, n)).astype(dt), rng.uniform(-1, 1, (n, n)).astype(dt)
            e = rng.uniform(-1, 1, (nc, nc)).astype(dt)
            assert_same(mg.restriction2d(lv, f), po.restrict(f, mode), ("restrict_rhs", lv))
            cb, cu = mg.residual_restriction(lv, v, f)
            assert_same(cb, po.restrict(ref.residual(lv, v, f), mode), ("restrict", lv))
            assert not cu.any(), ("the coarse guess is zeroed", lv)
            assert_same(mg.interpolation2d(lv, e), po.prolong(e), ("prolong", lv))
            assert_same(mg.interpolation_add(lv, v, e), po.prolong_add(v, e), ("prolong_add", lv))
        m = (1 << coarsest) - 1
        f = np.random.default_rng(4).uniform(-1, 1, (m, m)).astype(dt)
        x, x_ref = mg.bottom_solve(f), ref.bottom(f)
        if dtype == 1:
            assert np.max(np.abs(x - x_ref)) <= 1e-10 * np.max(np.abs(x_ref))
        else:
            assert np.allclose(x, x_ref, rtol=1e-6, atol=1e-6 * np.max(np.abs(x_ref)))


@pytest.mark.parametrize("mode", [gr.CONSISTENT, gr.FW16])
def test_one_vcycle_from_an_intermediate_nine_point_level(pkg, po, mode):
    finest, coarsest, lv = 9, 4, 7
    a = coefficient(finest, "jump")
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, finest, finest), finest, coarsest, mode=mode, mu1=2, mu2=1)
    n = (1 << lv) - 1
    rng = np.random.default_rng(77)
    v, f = rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n))
    want = ref.vcycle(lv, v, f)
    with handle(pkg, finest, coarsest, restrict_mode=mode, mu2=1) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        got = mg.vcyclemultigrid(lv, v, f)
    assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))
    assert np.max(np.abs(want - v)) > 1e-3 * np.max(np.abs(v))             # the cycle did something


@pytest.mark.parametrize("graph", ["1", "0"])
def test_vcycle_zero_equals_zero_guess_then_vcycle(pkg, po, monkeypatch, graph):
    """the pattern of tests/test_gpu_api.py on a GALERKIN handle"""
    monkeypatch.setenv("MGX_GRAPH", graph)
    L = 8
    n = (1 << L) - 1
    coef = coefficient(L, "jump")
    rng = np.random.default_rng(5)
    with handle(pkg, L, 4, mu2=1) as a, handle(pkg, L, 4, mu2=1) as b:
        for mg in (a, b):
            mg.set_coefficient(coef)
            mg.build_galerkin()
        for it in range(4):
            f = rng.uniform(-1, 1, (n, n))
            a.set_rhs(f)
            a.set_guess(rng.uniform(-1, 1, (n, n)))      # stale data the call must ignore
            a.vcycle_zero()
            b.set_rhs(f)
            b.set_guess(np.zeros((n, n)))
            b.vcycle()
            assert np.array_equal(a.get_solution(), b.get_solution()), it
        if graph == "1":
            assert 1 <= a.graphs_cached() <= 2


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("bottom", [gr.EXACT, gr.SMOOTH])
def test_fmg_matches_the_reference(pkg, po, bottom, dtype):
    """mgx_fmg against Hierarchy.fmg, "jump" at (8, 4), mu0 = 1 (two V-cycles per level)"""
    dt = np_dtype(dtype)
    L = 8
    a = coefficient(L, "jump")
    b = po.rhs_sine(L).astype(dt)
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, 4, dt, mu0=1, bottom=bottom)
    u_ref = ref.fmg(b)
    r_ref = po.norm2(ref.residual(L, u_ref, b))
    assert r_ref < po.norm2(b), "the reference's FMG pass does not reduce the residual"
    with handle(pkg, L, 4, dtype=dtype, mu0=1, bottom=bottom) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_guess(np.ones_like(b))                    # FMG discards the guess (PS:630)
        u = mg.fullmultigrid(b)
        r = mg.residual_norm()
    print(f"FMG bottom {bottom} dtype {dtype}: ||r|| {r:.6e}, reference {r_ref:.6e}, max |u - u_ref| / max |u_ref| {np.max(np.abs(u - u_ref)) / np.max(np.abs(u_ref)):.3e}")
    if dtype == 1:
        assert hist_close([r], [r_ref])
        assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))
    else:
        assert np.allclose(r, r_ref, rtol=1e-6, atol=0)


@pytest.mark.parametrize("dtype", [1, 0])
def test_fmg_schedule_history_matches_the_reference(pkg, po, dtype):
    """schedule = FMG at (9, 5), contrast 10: the first cycle is the FMG pass, V(2,2) cycles after.  Double converges
    (22 cycles in the reference); float runs 14 cycles as test_histories_match_the_reference does"""
    dt = np_dtype(dtype)
    L = 9
    a = pcg_ref.contrast_coefficient(L, 10.0)
    b = po.rhs_constant(L)
    tol, cycles = (1e-8, 40) if dtype == 1 else (1e-8, 14)
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, 5, dt)
    u_ref, h_ref = ref.solve(b, tol=tol, max_cycles=cycles, schedule=gr.FMG)
    with handle(pkg, L, 5, dtype=dtype, schedule=gr.FMG, mu0=0) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve(tol=tol, max_cycles=cycles)
        u = mg.get_solution()
    print(f"FMG schedule dtype {dtype}: {len(h) - 1} cycles (reference {len(h_ref) - 1})")
    if dtype == 1:
        assert h_ref[-1] <= tol * h_ref[0], "the reference itself did not converge"
        assert hist_close(h, h_ref), (h, h_ref)
        assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))
    else:
        assert h_ref[-1] < h_ref[0]
        assert len(h) == len(h_ref) and np.allclose(h, h_ref, rtol=1e-6, atol=0), (h, h_ref)


def test_bottom_smooth_history_matches_the_reference(pkg, po):
    """bottom = SMOOTH at (8, 4): mu1 + mu2 sweeps of the nine-point smoother stand in for the dense solve.  That is a
    weak coarse solve (n = 15), so V(4,4) with omega 0.8 on the "smooth" coefficient: 59 cycles in the reference"""
    L = 8
    a = coefficient(L, "smooth")
    b = po.rhs_sine(L)
    kw = dict(mu1=4, mu2=4, omega=0.8, bottom=gr.SMOOTH)
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, 4, **kw)
    u_ref, h_ref = ref.solve(b, tol=1e-8, max_cycles=80)
    assert h_ref[-1] <= 1e-8 * h_ref[0], "the reference itself did not converge"
    with handle(pkg, L, 4, **kw) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve(tol=1e-8, max_cycles=80)
        u = mg.get_solution()
        with pytest.raises(pkg.MgxError, match="bottom = SMOOTH"):
            mg.bottom_solve(np.zeros((15, 15)))
    print(f"bottom SMOOTH: {len(h) - 1} cycles (reference {len(h_ref) - 1})")
    assert hist_close(h, h_ref), (h, h_ref)
    assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))


def fuzz_cases(po, count=16, seed=20261016):
    """`count` configurations drawn from one seeded stream, each with its reference run.  A draw whose reference does
    not reduce the residual in every one of its cycles is rejected and the stream moves on to the next draw; with
    this seed none of the first 16 draws is rejected (at most 2 rejections are allowed: see the assertion)"""
    rng = np.random.default_rng(seed)
    cases, rejected, draw = [], [], 0
    while len(cases) < count:
        finest = int(rng.integers(5, 10))
        coarsest = int(rng.integers(2, min(5, finest) + 1))
        cfg = dict(finest_level=finest, coarsest_level=coarsest, mu0=int(rng.integers(0, 2)), mu1=int(rng.integers(0, 5)),
                   mu2=int(rng.integers(0, 5)), omega=float(rng.choice([2.0 / 3.0, 0.8, 0.6])), schedule=int(rng.integers(0, 2)),
                   restrict_mode=int(rng.integers(0, 2)), bottom=int(rng.integers(0, 2)))
        if cfg["mu1"] + cfg["mu2"] == 0:
            cfg["mu2"] = 2
        n = (1 << finest) - 1
        x = np.linspace(0.0, 1.0, n + 2)
        a = np.exp(rng.uniform(-0.7, 0.7) * np.sin(rng.integers(1, 4) * np.pi * x)[None, :] * np.cos(rng.integers(1, 4) * np.pi * x)[:, None])
        a = a * (1.0 + 0.1 * rng.random(a.shape))
        b = po.rhs_sine(finest) if draw % 2 else po.rhs_constant(finest)
        u0 = po.fill_uniform((n, n), 500 + draw) if cfg["schedule"] == 0 and draw % 3 == 0 else None
        ref = gr.Hierarchy(po, po.stencil_from_nodes(a, finest, finest), finest, coarsest, np.float64, cfg["restrict_mode"], cfg["omega"],
                           cfg["mu1"], cfg["mu2"], cfg["mu0"], cfg["bottom"])
        u_ref, h_ref = ref.solve(b, u0, tol=1e-9, max_cycles=6, schedule=cfg["schedule"])
        if np.all(np.diff(h_ref) < 0):
            cases.append((draw, cfg, a, b, u0, u_ref, h_ref))
        else:
            rejected.append((draw, cfg, h_ref))
        draw += 1
    assert len(rejected) <= 2, rejected
    return cases, rejected


def test_seeded_fuzz_of_galerkin_configurations(pkg, po):
    """16 random configurations (fixed seed) of the Galerkin path, modelled on the STENCIL5 fuzz of tests/test_gpu_var.py:
    levels (coarsest == finest included), sweeps (0 included), weights, restriction modes, schedules, bottom modes,
    random positive coefficients, a random guess on some V cases - 6 cycles, histories and solutions against
    Hierarchy.solve"""
    cases, rejected = fuzz_cases(po)
    print(f"rejected draws: {[(d, c) for d, c, _ in rejected]}")
    for draw, cfg, a, b, u0, u_ref, h_ref in cases:
        with pkg.Multigrid(op=pkg.OP_GALERKIN, **cfg) as mg:
            mg.set_coefficient(a)
            mg.build_galerkin()
            mg.set_rhs(b)
            if u0 is not None:
                mg.set_guess(u0)
            st, h = mg.solve(tol=1e-9, max_cycles=6)
            u = mg.get_solution()
        print(f"draw {draw} {cfg}: {len(h) - 1} cycles, max rel. history difference "
              f"{np.max(np.abs(h[:len(h_ref)] - h_ref[:len(h)]) / h_ref[:len(h)]):.3e}")
        assert hist_close(h, h_ref), (draw, cfg, h, h_ref)
        assert np.max(np.abs(u - u_ref)) <= 1e-10 * max(np.max(np.abs(u_ref)), 1e-300), (draw, cfg)


@pytest.mark.parametrize("bottom", [gr.EXACT, gr.SMOOTH])
def test_finest_equal_coarsest_has_no_nine_point_level(pkg, po, bottom):
    """one five-point level: a cycle is the dense solve (EXACT: the first cycle ends the solve) or mu1 + mu2 sweeps"""
    L = 4
    a = coefficient(L, "smooth")
    b = po.rhs_sine(L)
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, L, mu1=3, mu2=2, bottom=bottom)
    u_ref, h_ref = ref.solve(b, tol=1e-9, max_cycles=6)
    assert np.all(np.diff(h_ref) < 0) and (bottom == gr.SMOOTH or len(h_ref) == 2)
    with handle(pkg, L, L, mu1=3, mu2=2, bottom=bottom) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve(tol=1e-9, max_cycles=6)
        u = mg.get_solution()
    assert hist_close(h, h_ref), (h, h_ref)
    assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))


def test_pcg_fp32_history_matches_the_reference(pkg, po):
    """the form of test_fp32_histories_match_the_reference in tests/test_gpu_pcg.py, with the Galerkin V-cycle"""
    L = 9
    dt = np.float32
    a = pcg_ref.contrast_coefficient(L, 10.0)
    b = po.rhs_sine(L).astype(dt)
    coef = po.stencil_from_nodes(a, L, L)
    ref = gr.Hierarchy(po, coef, L, 5, dt)
    zeros = np.zeros_like(b)
    _, h_ref, conv_ref, _ = pcg_ref.pcg(pcg_ref.Operator(coef, dt), lambda r: ref.vcycle(L, zeros, r), b, zeros, tol=1e-5, max_iters=100)
    with handle(pkg, L, 5, dtype=0) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        mg.set_rhs(b)
        st, h = mg.solve_pcg(tol=1e-5, max_iters=100)
        u = mg.get_solution()
    print(f"fp32 PCG: {len(h) - 1} iterations (reference {len(h_ref) - 1})")
    assert conv_ref and st.converged == 1
    assert abs(len(h) - len(h_ref)) <= 1, (h, h_ref)
    m = min(len(h), len(h_ref))
    assert np.all(np.abs(h[:m] - h_ref[:m]) <= RTOL32 * h_ref[:m]), (h, h_ref)
    assert np.isfinite(u).all()


def test_refusals_leave_the_handle_usable(pkg, po):
    L, Lc = 7, 4
    n = (1 << L) - 1
    a = coefficient(L, "jump")
    b = po.rhs_sine(L)
    ref = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, Lc)
    u_ref, h_ref = ref.solve(b, tol=1e-9, max_cycles=4)

    def solves(mg):
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        st, h = mg.solve(tol=1e-9, max_cycles=4)
        assert hist_close(h, h_ref), (h, h_ref)

    # a multi-GPU GALERKIN configuration is refused at create, in one process and as a rank
    with pytest.raises(pkg.MgxError, match="one GPU"):
        handle(pkg, L, Lc, n_gpus=2)
    with pytest.raises(pkg.MgxError, match="one GPU"):
        pkg.Multigrid.rank(0, 2, finest_level=L, coarsest_level=Lc, op=pkg.OP_GALERKIN)
    with handle(pkg, L, Lc) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin()
        first = [mg.get_stencil9(lv, q) for lv in range(Lc, L + 1) for q in range(18)]
        mg.build_galerkin()                      # idempotent: the same bits again
        again = [mg.get_stencil9(lv, q) for lv in range(Lc, L + 1) for q in range(18)]
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        solves(mg)
        for lv, which in ((L - 1, -1), (L - 1, 18), (Lc - 1, 0), (L + 1, 0)):
            with pytest.raises(pkg.MgxError, match="out of range"):
                mg.get_stencil9(lv, which)
            solves(mg)
        m = (1 << (L - 1)) - 1
        buf = np.full(m * m + 1, 7.0)
        for lv, which in ((L - 1, 0), (L - 1, 12), (L, 6)):       # (L, 6): a corner of the five-point finest level
            for count in (m * m - 1, m * m + 1, 0):
                rc = pkg.lib().mgx_get_stencil9(mg._h, lv, which, buf.ctypes.data, C.c_size_t(count))
                assert rc != 0, (lv, which, count)
                assert np.all(buf == 7.0), "a refused read wrote to the caller's buffer"
            solves(mg)
