"""Keeps tests/handle_model.py honest (no GPU): the schedules it composes from its own single operators must give
the bits of the references' own schedules - oracle/pyoracle.py's Solver for the constant stencil, the hierarchies of
tests/galerkin_ref.py, tests/opdep_ref.py and tests/cheby_ref.py for the general operators, tests/colour_ref.py for the
colour smoothers and tests/nine_ref.py for nine-point finest levels - and its solves their histories; the coarse levels
must hold afterwards what the documented operator sequence leaves there.  solve_refine is held to tests/refine_ref.py's
loop around an fp64 and an independently built float32 reference hierarchy.  The sequences of
tests/test_gpu_handle_state.py are drawn and walked here without a device: what the generator promises, and the
conditions the Krylov bounds rest on."""
import numpy as np
import pytest

import cheby_ref
import colour_ref as cf
import galerkin_ref as gr
import gcr_ref
import handle_model as hm
import line_ref as lr
import nine_ref as nr
import opdep_ref as od
import pcg_ref
import test_gpu_handle_state as gs
import wcycle_ref as wr
from test_line_cpu import as_type, operator5

LEVELS = [(6, 3), (7, 4)]


def data(po, L, dt, seed):
    n = (1 << L) - 1
    return po.fill_uniform((n, n), seed).astype(dt), po.fill_uniform((n, n), seed + 1).astype(dt)


def oracle(po, cfg):
    """the oracle with the model's bottom method (sine transform: exact like the default Cholesky solve, but in the
    device's operation order - pcg_ref.oracle_solver does the same)"""
    c = dict(cfg)
    if c.get("bottom", 0) == hm.EXACT:
        c["bottom"] = po.BOTTOM_DST
    return po.Solver(**c)


@pytest.mark.parametrize("bottom", [hm.EXACT, hm.SMOOTH])
@pytest.mark.parametrize("mode", [hm.CONSISTENT, hm.FW16])
@pytest.mark.parametrize("smoother", [hm.JACOBI, hm.RBGS])
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32])
@pytest.mark.parametrize("L,Lc", LEVELS)
def test_poisson_vcycle_and_fmg_equal_the_oracle(po, L, Lc, dtype, smoother, mode, bottom):
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=1, mu1=3, mu2=2, smoother=smoother, dtype=dtype, restrict_mode=mode, bottom=bottom)
    dt = np.float64 if dtype == hm.F64 else np.float32
    u, b = data(po, L, dt, 10 * L + smoother)
    ref = oracle(po, cfg)
    m = hm.HandleModel(po, **cfg)
    m.set_guess(u)
    m.set_rhs(b)
    m.vcycle(L)
    assert m.U[L].dtype == dt and np.array_equal(m.U[L], ref.vcycle(L, u, b))
    assert np.array_equal(m.B[L], b)
    # the coarse levels: restricted residuals on the way down, corrections on the way up
    v = po.jacobi(u, b, 3) if smoother == hm.JACOBI else po.rbgs(u, b, 3)
    rc = po.restrict(po.residual(v, b), mode)
    assert np.array_equal(m.B[L - 1], rc)
    assert np.array_equal(m.U[L - 1], ref.vcycle(L - 1, np.zeros_like(rc), rc))
    # a V-cycle from an intermediate level touches nothing above it
    top = m.U[L].copy()
    u1, b1 = data(po, L - 1, dt, 77)
    m.set_level(L - 1, 0, u1)
    m.set_level(L - 1, 1, b1)
    m.vcycle(L - 1)
    assert np.array_equal(m.U[L - 1], ref.vcycle(L - 1, u1, b1)) and np.array_equal(m.U[L], top)
    m.set_rhs(b)
    m.fmg()
    assert np.array_equal(m.U[L], ref.fmg(L, b))
    m.set_guess(u)
    m.vcycle_zero()
    assert np.array_equal(m.U[L], ref.vcycle(L, np.zeros_like(b), b))


def test_poisson_fma_arithmetic_equals_the_oracle(po):
    cfg = dict(finest_level=6, coarsest_level=3, mu0=0, mu1=3, mu2=2, arith=hm.FMA)
    u, b = data(po, 6, np.float64, 5)
    m = hm.HandleModel(po, **cfg)
    m.set_guess(u)
    m.set_rhs(b)
    m.vcycle()
    assert np.array_equal(m.U[6], oracle(po, cfg).vcycle(6, u, b))
    assert not np.array_equal(m.U[6], oracle(po, dict(cfg, arith=hm.SEPARATE)).vcycle(6, u, b))


@pytest.mark.parametrize("schedule", [hm.V, hm.FMG])
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32])
def test_poisson_solve_history_cycles_and_fine_updates(po, dtype, schedule):
    L, Lc = 7, 4
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=1, mu1=2, mu2=1, dtype=dtype, schedule=schedule)
    dt = np.float64 if dtype == hm.F64 else np.float32
    u, b = data(po, L, dt, 3)
    m = hm.HandleModel(po, **cfg)
    m.set_guess(u)
    m.set_rhs(b)
    m.smooth(L, 5)                                      # counted, then forgotten: a solve counts from its own start
    u = m.U[L]
    tol = 1e-3
    st, h = m.solve(tol=tol, max_cycles=12)
    ref = oracle(po, cfg)
    x = u
    want = [po.norm2(po.residual(x, b))]
    for k in range(12):
        if want[-1] <= tol * want[0]:
            break
        x = ref.fmg(L, b) if (k == 0 and schedule == hm.FMG) else ref.vcycle(L, x, b)
        want.append(po.norm2(po.residual(x, b)))
    assert np.array_equal(h, np.array(want)) and np.array_equal(m.U[L], x)
    assert st["cycles"] == len(want) - 1 and st["converged"] == 1 and 1 <= st["cycles"] < 12
    n2 = float((1 << L) - 1) ** 2
    fmg_first = schedule == hm.FMG
    assert st["fine_updates"] == 3.0 * n2 * (st["cycles"] + (1 if fmg_first else 0))     # FMG: mu0 + 1 = 2 finest cycles
    st0, h0 = m.solve(tol=0.5, max_cycles=0)
    assert st0 == dict(cycles=0, converged=0, fine_updates=0.0) and len(h0) == 1


@pytest.mark.parametrize("smoother", [hm.JACOBI, hm.RBGS])
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32])
def test_poisson_solve_pcg_equals_pcg_ref(po, dtype, smoother):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, dtype=dtype, smoother=smoother, schedule=hm.V)
    dt = np.float64 if dtype == hm.F64 else np.float32
    u, b = data(po, L, dt, 21)
    tol = 1e-8 if dtype == hm.F64 else 1e-4
    x_ref, h_ref, conv, _ = pcg_ref.run(po, cfg, b, u, tol=tol, max_iters=30)
    m = hm.HandleModel(po, **cfg)
    m.set_guess(u)
    m.set_rhs(b)
    st, h = m.solve_pcg(tol=tol, max_iters=30)
    assert conv and np.array_equal(h, h_ref) and np.array_equal(m.U[L], x_ref)
    assert np.array_equal(m.B[L], b)                    # B is the caller's b again
    assert st["cycles"] == len(h_ref) - 1 and st["converged"] == 1
    assert st["fine_updates"] == 3.0 * float((1 << L) - 1) ** 2 * st["cycles"]      # a cycle before the loop and after every iteration but the last
    # stopped by the count: the coarse levels hold what the last preconditioner cycle left
    m.set_guess(u)
    st, h = m.solve_pcg(tol=0.0, max_iters=2)
    assert st == dict(cycles=2, converged=0, fine_updates=2 * 3.0 * float((1 << L) - 1) ** 2) and np.array_equal(h, h_ref[:3])
    st, h = m.solve_pcg(tol=0.0, max_iters=0)
    assert st["cycles"] == 0 and len(h) == 1


def contrast(L, c, seed):
    """a nodal coefficient of 1 or c in 8 x 8 blocks"""
    N = 1 << L
    blk = np.where(np.random.RandomState(seed).rand(N // 8 + 1, N // 8 + 1) < 0.5, 1.0, c)
    return np.kron(blk, np.ones((8, 8)))[: N + 1, : N + 1].copy()


def reference_hierarchy(po, cfg, a, transfer):
    L, Lc = cfg["finest_level"], cfg["coarsest_level"]
    dt = np.float64 if cfg["dtype"] == hm.F64 else np.float32
    kw = dict(dtype=dt, mode=cfg["restrict_mode"], omega=2.0 / 3.0, mu1=cfg["mu1"], mu2=cfg["mu2"], mu0=cfg["mu0"], bottom=cfg["bottom"])
    cheb = cfg["smoother"] == hm.CHEBYSHEV
    if cfg["op"] == hm.STENCIL5:
        st = {lv: po.stencil_from_nodes(a, lv, L) for lv in range(Lc, L + 1)}
        return (cheby_ref.Stencil5Cheby if cheb else cheby_ref.Stencil5)(po, st, L, Lc, **kw)
    st5 = po.stencil_from_nodes(a, L, L)
    if transfer == hm.OPERATOR:
        return (cheby_ref.OpdepHierarchy if cheb else od.Hierarchy)(po, st5, L, Lc, **kw)
    return (cheby_ref.Hierarchy if cheb else gr.Hierarchy)(po, st5, L, Lc, **kw)


GENERAL = [(hm.STENCIL5, None), (hm.GALERKIN, hm.BILINEAR), (hm.GALERKIN, hm.OPERATOR)]


@pytest.mark.parametrize("bottom", [hm.EXACT, hm.SMOOTH])
@pytest.mark.parametrize("smoother", [hm.JACOBI, hm.CHEBYSHEV])
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32])
@pytest.mark.parametrize("op,transfer", GENERAL)
@pytest.mark.parametrize("L,Lc", LEVELS)
def test_general_operators_equal_their_references(po, L, Lc, op, transfer, dtype, smoother, bottom):
    mode = hm.FW16 if (L + dtype) % 2 else hm.CONSISTENT
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=3, smoother=smoother, dtype=dtype, restrict_mode=mode,
               bottom=bottom, op=op, schedule=hm.FMG)
    dt = np.float64 if dtype == hm.F64 else np.float32
    a = contrast(L, 10.0, 4)
    ref = reference_hierarchy(po, cfg, a, transfer)
    m = hm.HandleModel(po, **cfg)
    with pytest.raises(RuntimeError):
        m.smooth(L, 1)                                  # no operator yet
    m.set_coefficient(a)
    if op == hm.GALERKIN:
        with pytest.raises(RuntimeError):
            m.vcycle()                                  # set_coefficient invalidates the hierarchy until the build
        m.build_galerkin(transfer)
    u, b = data(po, L, dt, 40 + L)
    m.set_guess(u)
    m.set_rhs(b)
    m.vcycle()
    assert m.U[L].dtype == dt and np.array_equal(m.U[L], ref.vcycle(L, u, b))
    m.fmg()
    assert np.array_equal(m.U[L], ref.fmg(b))
    m.set_guess(u)
    st, h = m.solve(tol=0.0, max_cycles=3)
    u_ref, h_ref = ref.solve(b, u, tol=0.0, max_cycles=3, schedule=gr.FMG)
    assert np.array_equal(h, h_ref) and np.array_equal(m.U[L], u_ref) and st["cycles"] == 3
    assert st["fine_updates"] == 3 * 5.0 * float((1 << L) - 1) ** 2
    if bottom == hm.EXACT:
        # the oracle's dense solve (STENCIL5 model) and the numpy elimination (references) are the same statement
        e, f = data(po, Lc, dt, 9)
        m.set_level(Lc, 1, f)
        m.bottom_solve()
        assert np.array_equal(m.U[Lc], ref.bottom(f))
    else:
        with pytest.raises(RuntimeError):
            m.bottom_solve()
    # single operators between two levels
    e, f = data(po, L - 1, dt, 11)
    m.set_level(L - 1, 0, e)
    m.set_guess(u)
    m.prolong_add(L)
    want = u + ref.prolong(L, e) if transfer == hm.OPERATOR else po.prolong_add(u, e)
    assert np.array_equal(m.U[L], want)
    m.restrict(L)
    r = ref.residual(L, want, b)
    assert np.array_equal(m.B[L - 1], ref.restrict(L, r) if transfer == hm.OPERATOR else po.restrict(r, mode))
    assert not m.U[L - 1].any()


def test_galerkin_rebuilds_switch_the_transfers_and_share_inverses(po):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=2, op=hm.GALERKIN, schedule=hm.V, dtype=hm.F64, smoother=hm.JACOBI,
               restrict_mode=hm.CONSISTENT, bottom=hm.EXACT)
    a1, a2 = contrast(L, 10.0, 1), contrast(L, 100.0, 2)
    u, b = data(po, L, np.float64, 2)
    m = hm.HandleModel(po, **cfg)
    m.set_coefficient(a1)
    out = []
    for transfer, a in ((hm.BILINEAR, None), (hm.OPERATOR, None), (hm.BILINEAR, None), (hm.OPERATOR, None), (hm.BILINEAR, a2)):
        if a is not None:
            m.set_coefficient(a)
        m.build_galerkin(transfer)
        m.set_guess(u)
        m.set_rhs(b)
        m.vcycle()
        out.append(m.U[L])
        ref = reference_hierarchy(po, cfg, a1 if a is None else a, transfer)
        assert np.array_equal(out[-1], ref.vcycle(L, u, b))
    assert np.array_equal(out[0], out[2]) and np.array_equal(out[1], out[3])
    assert not np.array_equal(out[0], out[1]) and not np.array_equal(out[0], out[4])


def test_stencil5_solve_pcg_equals_pcg_ref(po):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=2, op=hm.STENCIL5, schedule=hm.V)
    a = contrast(L, 10.0, 3)
    u, b = data(po, L, np.float64, 8)
    x_ref, h_ref, conv, _ = pcg_ref.run(po, cfg, b, u, a_nodes=a, tol=1e-8, max_iters=40)
    m = hm.HandleModel(po, **cfg)
    m.set_coefficient(a)
    m.set_guess(u)
    m.set_rhs(b)
    st, h = m.solve_pcg(tol=1e-8, max_iters=40)
    assert conv and np.array_equal(h, h_ref) and np.array_equal(m.U[L], x_ref) and st["converged"] == 1


def test_refused_configurations():
    with pytest.raises(ValueError):
        hm.HandleModel(None, dtype=hm.MIXED)
    with pytest.raises(TypeError):
        hm.HandleModel(None, n_gpus=2)


# ---- solve_gcr ----------------------------------------------------------------------------------------------------------
def gcr_with_record(A, M, b, x0, **kw):
    """gcr_ref.gcr, and the residuals it handed to M"""
    seen = []

    def recording(r):
        seen.append(np.array(r, copy=True))
        return M(r)

    return gcr_ref.gcr(A, recording, b, x0, **kw), seen


def assert_gcr_equals(po, m, A, M, u, b, calls):
    """the model's solve_gcr against gcr_ref.gcr around the reference's own cycle M, for every (tol, max_iters, restart) of
    `calls` from the guess u: history, x, B, the statistics, and the coarse levels - those of ONE zero-start cycle on the
    last residual the iteration handed to M (nothing, where it handed none over)"""
    L = m.L
    n2 = float((1 << L) - 1) ** 2
    per = (2 if m.cfg["smoother"] == hm.LINE_ALT else 1) * (m.cfg["mu1"] + m.cfg["mu2"])
    for tol, max_iters, restart in calls:
        (x_ref, h_ref, conv, brk), seen = gcr_with_record(A, M, b, u, tol=tol, max_iters=max_iters, restart=restart)
        m.set_guess(u)
        m.set_rhs(b)
        before = {lv: (m.U[lv].copy(), m.B[lv].copy()) for lv in m.levels() if lv < L}
        st, h = m.solve_gcr(tol=tol, max_iters=max_iters, restart=restart)
        assert np.array_equal(h, h_ref) and np.array_equal(m.U[L], x_ref) and m.U[L].dtype == x_ref.dtype, (tol, max_iters, restart)
        assert np.array_equal(m.B[L], b)                    # B is the caller's b again
        assert st == dict(cycles=len(h_ref) - 1, converged=int(conv and not brk), fine_updates=len(seen) * per * n2), (st, len(seen))
        if seen:
            one = hm.HandleModel(po, **m.cfg)
            one.cycle, one.h, one.transfer = m.cycle, m.h, m.transfer
            one.set_rhs(seen[-1])
            one.vcycle_zero()
            for lv in before:
                assert np.array_equal(m.U[lv], one.U[lv]) and np.array_equal(m.B[lv], one.B[lv]), (lv, tol, max_iters, restart)
        else:
            for lv, (uu, bb) in before.items():
                assert np.array_equal(m.U[lv], uu) and np.array_equal(m.B[lv], bb), lv


def GCR_CALLS(tol):
    """(tol, max_iters, restart): to convergence; stopped by the count after a restart wrap (slots 0, 1, 0, 1); no iteration;
    a basis of one"""
    return [(tol, 30, 4), (0.0, 4, 2), (0.0, 0, 4), (tol, 30, 1)]


@pytest.mark.parametrize("smoother", [hm.JACOBI, hm.RBGS])
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32])
def test_poisson_solve_gcr_equals_gcr_ref(po, dtype, smoother):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, dtype=dtype, smoother=smoother, schedule=hm.V)
    dt = np.float64 if dtype == hm.F64 else np.float32
    u, b = data(po, L, dt, 21)
    s = pcg_ref.oracle_solver(po, cfg)
    zeros = np.zeros_like(b)
    m = hm.HandleModel(po, **cfg)
    try:
        assert_gcr_equals(po, m, pcg_ref.Operator(None, dt), lambda r: s.vcycle(L, zeros, r), u, b, GCR_CALLS(1e-8 if dtype == hm.F64 else 1e-4))
    finally:
        s.close()
    st, h = m.solve_gcr(tol=0.0, max_iters=4, restart=2)
    assert st["cycles"] == 4 and st["converged"] == 0 and len(h) == 5
    assert st["fine_updates"] == 4 * 3.0 * float((1 << L) - 1) ** 2     # counted from zero: one cycle per iteration


def test_stencil5_solve_gcr_equals_gcr_ref(po):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=2, op=hm.STENCIL5, schedule=hm.V)
    a = contrast(L, 10.0, 3)
    u, b = data(po, L, np.float64, 8)
    s = pcg_ref.oracle_solver(po, cfg, a)
    zeros = np.zeros_like(b)
    m = hm.HandleModel(po, **cfg)
    m.set_coefficient(a)
    try:
        assert_gcr_equals(po, m, pcg_ref.Operator(po.stencil_from_nodes(a, L, L), np.float64), lambda r: s.vcycle(L, zeros, r), u, b, GCR_CALLS(1e-8))
    finally:
        s.close()


def test_galerkin_w_cycle_solve_gcr_equals_gcr_ref_around_wcycle_ref(po):
    from test_galerkin_cpu import random_stencil5
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=2, op=hm.GALERKIN, schedule=hm.V)
    st5 = random_stencil5(L, 100 + L)
    u, b = data(po, L, np.float64, 12)
    ref = wr.with_cycle(wr.Galerkin, wr.W, po, st5, L, Lc, np.float64, mu1=2, mu2=2)
    m = hm.HandleModel(po, **cfg)
    m.set_stencil(L, st5)
    m.build_galerkin(hm.BILINEAR)
    m.set_cycle(hm.CYCLE_W)
    assert_gcr_equals(po, m, pcg_ref.Operator(st5, np.float64), gcr_ref.cycle_preconditioner(ref), u, b, GCR_CALLS(1e-10))


def test_line_solve_gcr_equals_gcr_ref_around_line_ref(po):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=1, mu2=1, op=hm.GALERKIN, smoother=hm.LINE_ALT, schedule=hm.V)
    ref = line_reference(po, lr.Hierarchy, hm.LINE_ALT, "layers", L, Lc, np.float64, np.float64, hm.CYCLE_V, mu1=1, mu2=1)
    u, b = data(po, L, np.float64, 14)
    m = hm.HandleModel(po, **cfg)
    m.set_operator("layers")
    assert_gcr_equals(po, m, pcg_ref.Operator(operator5(po, L, "layers", np.float64), np.float64), gcr_ref.cycle_preconditioner(ref), u, b,
                      GCR_CALLS(1e-8))


# POISSON with no smoothing anywhere and bottom = SMOOTH: the zero-start cycle returns exactly zero, M = 0
M0 = dict(finest_level=7, coarsest_level=4, mu0=0, mu1=0, mu2=0, bottom=hm.SMOOTH, schedule=hm.V)


@pytest.mark.parametrize("seed", [None, 7])
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32])
def test_solve_gcr_breaks_down_where_the_cycle_returns_zero(po, dtype, seed):
    """q = A M r = 0, so q'.q' = 0 at iteration 1: gcr_ref around the oracle's cycle reports a breakdown, a history of one
    entry and an untouched x, and so does the model - U the guess, B the caller's b, the coarse levels those of the one
    cycle that ran"""
    L = M0["finest_level"]
    cfg = dict(M0, dtype=dtype)
    dt = np.float64 if dtype == hm.F64 else np.float32
    u, b = data(po, L, dt, 33)
    if seed is None:
        u = np.zeros_like(u)
    s = pcg_ref.oracle_solver(po, cfg)
    zeros = np.zeros_like(b)
    A = pcg_ref.Operator(None, dt)
    try:
        assert not s.vcycle(L, zeros, b).any()
        x_ref, h_ref, conv, brk = gcr_ref.gcr(A, lambda r: s.vcycle(L, zeros, r), b, u, 1e-8, 30, 4)
        assert brk and not conv and len(h_ref) == 1 and np.array_equal(x_ref, u)
        m = hm.HandleModel(po, **cfg)
        assert_gcr_equals(po, m, A, lambda r: s.vcycle(L, zeros, r), u, b, [(1e-8, 30, 4)])
    finally:
        s.close()
    assert np.array_equal(m.U[L], u) and np.array_equal(m.B[L], b)
    assert np.array_equal(m.B[L - 1], po.restrict(b - A(u), hm.CONSISTENT)) and not m.U[L - 1].any()
    st, h = m.solve_pcg(tol=1e-8, max_iters=30)         # p = M r = 0: p.Ap = 0
    assert st == dict(cycles=0, converged=0, fine_updates=0.0) and np.array_equal(h, h_ref) and np.array_equal(m.U[L], u)


# ---- the sequences of tests/test_gpu_handle_state.py ------------------------------------------------------------------
FROZEN = {
    # seed: (length, the first ten calls) of draw_sequence(seed, cfg) before the generator learnt its optional calls
    8501: (48, [('set_u', 5, 1005), ('set_b', 5, 2005), ('set_u', 6, 1006), ('set_b', 6, 2006), ('set_u', 7, 1007), ('set_b', 7, 2007),
                ('set_u', 8, 1008), ('set_b', 8, 2008), ('solve', 0.0, 2), ('vcycle_zero',)]),
    8511: (49, [('set_coefficient', 10.0, 10), ('set_u', 5, 1005), ('set_b', 5, 2005), ('set_u', 6, 1006), ('set_b', 6, 2006),
                ('set_u', 7, 1007), ('set_b', 7, 2007), ('set_u', 8, 1008), ('set_b', 8, 2008), ('solve', 0.01, 3)]),
    8521: (50, [('set_coefficient', 10.0, 10), ('build_galerkin', 0), ('set_u', 5, 1005), ('set_b', 5, 2005), ('set_u', 6, 1006),
                ('set_b', 6, 2006), ('set_u', 7, 1007), ('set_b', 7, 2007), ('set_u', 8, 1008), ('set_b', 8, 2008)]),
}
# sha1 of repr(draw_sequence(seed, cfg)) of every case that existed then: the whole list, not its head
FROZEN_SHA1 = {
    8501: "1ead17fe803eb282c5491a79fcf74850c857588d", 8502: "e77d36c5b83d0d29e5e4fe8f046233e4598638a7",
    8503: "df389ae304f4ee45bb89b741b03b2d31afe54a4f", 8504: "d3dd6f34d14631d79133c7710aac7feca88c1097",
    8505: "0e2344a9df1b2eb2217a708729fa58c2826824a3", 8506: "80e6e1a42d59e51f72693b6e9b2f6bebe0124575",
    8511: "99cbaaf4661cac8be3d0dbdfa9f768b6401cbb59", 8512: "1d9b2aa221966f0f6c6a3c30f0b8a48704f52b6b",
    8513: "6a5955269e7045f5f11cdc8626bf41ed6ac9495f", 8521: "1ea724faecaa8f86dc234518a389962b818269be",
    8522: "319fa09454b5d041b855876f9a6d9475a1257cf3", 8523: "5a7d6e073d720be41539201468df3b1aaffe10fa",
}


def test_the_sequences_of_the_existing_cases_are_call_for_call_what_they_were():
    import hashlib
    cases = dict(gs.POISSON_CASES, **gs.GENERAL_CASES)
    by_seed = {seed: cfg for cfg, seed in cases.values()}
    assert set(by_seed) == set(FROZEN_SHA1)
    for seed, (length, head) in FROZEN.items():
        calls = gs.draw_sequence(seed, by_seed[seed])
        assert len(calls) == length and calls[:10] == head, seed
    for seed, digest in FROZEN_SHA1.items():
        calls = gs.draw_sequence(seed, by_seed[seed])
        assert hashlib.sha1(repr(calls).encode()).hexdigest() == digest, seed
        assert not any(c[0] in ("set_cycle", "set_operator") for c in calls)
    assert "MGX_SMALL_VISIT" in gs.KNOBS and "MGX_LINE_CHUNK" in gs.KNOBS


def test_cycle_and_line_sequences_hold_what_the_generator_promises():
    for cfg, seed, _ in gs.CYCLE_CASES.values():
        calls = gs.draw_sequence(seed, cfg, cycles=True)
        gs.assert_cycle_calls(calls, cfg)
        assert min(sum(1 for c in calls if c[0] == k) for k in gs.GRAPH_USERS) >= 5
        assert gs.small_levels(cfg) == list(range(cfg["coarsest_level"] + 1, 7))
    for cfg, seed, env, options in gs.LINE_CASES.values():
        calls = gs.draw_sequence(seed, cfg, **gs.LINE_OPTIONS, **options)
        if options.get("cycles"):
            gs.assert_cycle_calls(calls, cfg)
        assert calls[0] == ("set_operator", options["operators"][0])
        assert not any(c[0] == "set_coefficient" for c in calls)
        for i, c in enumerate(calls):
            if c[0] in ("solve", "solve_pcg"):
                assert calls[i - 1][0] == "set_guess", (seed, i)
            if c[0] == "vcycle":
                assert calls[i - 1][:2] == ("set_u", c[1]), (seed, i)


def test_gcr_sequences_hold_what_the_generator_promises():
    orders = set()
    for name, (cfg, seed, envs, options, line) in gs.GCR_CASES.items():
        calls = gs.draw_sequence(seed, cfg, gcr=True, **options)
        assert calls == gs.draw_sequence(seed, cfg, gcr=True, **options)
        gs.assert_gcr_calls(calls, cfg, options.get("fresh_guess", False), options.get("deep_iters", 9))
        assert options.get("deep_iters", 9) == 9 or line    # every other double case: nine iterations of GCR(8)
        assert gs.graph_users(calls) == gs.GCR_USERS
        if options.get("cycles"):
            gs.assert_cycle_calls(calls, cfg)
            users = [i for i, c in enumerate(calls) if c[0] in gs.GCR_USERS]
            after = [next(calls[u][0] for u in users if u > i) for i, c in enumerate(calls) if c[0] == "set_cycle"]
            if cfg.get("dtype", hm.F64) == hm.F64:          # where a graph of the old kind would replay under GCR
                assert "solve_gcr" in after, (name, after)
        if cfg.get("op", hm.POISSON) == hm.STENCIL5:
            assert [c[1] for c in calls if c[0] == "set_coefficient"] == [10.0, 100.0, 1000.0]
        if cfg.get("op", hm.POISSON) == hm.GALERKIN and not line:
            assert [c[1] for c in calls if c[0] == "build_galerkin"] == [hm.BILINEAR, hm.OPERATOR, hm.BILINEAR, hm.OPERATOR, hm.BILINEAR]
        if line:
            assert calls[0] == ("set_operator", options["operators"][0]) and not any(c[0] == "set_coefficient" for c in calls)
        orders.add(gs.krylov_order(calls))
    assert orders == {"pcg", "gcr"}                         # the shared workspace allocated by either method first
    assert len({seed for _, seed, _, _, _ in gs.GCR_CASES.values()}) == len(gs.GCR_CASES)
    # the option is off by default, and a sequence drawn without it holds no such call
    for cfg, seed in list(gs.POISSON_CASES.values()) + list(gs.GENERAL_CASES.values()):
        assert not any(c[0] == "solve_gcr" for c in gs.draw_sequence(seed, cfg))


# ---- the cycle index --------------------------------------------------------------------------------------------------
CYCLE_REFS = {
    # name: (reference class, op, transfer, smoother)
    "Galerkin": (wr.Galerkin, hm.GALERKIN, hm.BILINEAR, hm.JACOBI),
    "Opdep": (wr.Opdep, hm.GALERKIN, hm.OPERATOR, hm.JACOBI),
    "ChebyOpdep": (wr.ChebyOpdep, hm.GALERKIN, hm.OPERATOR, hm.CHEBYSHEV),
    "Stencil5": (wr.Stencil5, hm.STENCIL5, None, hm.JACOBI),
    "Stencil5Cheby": (wr.Stencil5Cheby, hm.STENCIL5, None, hm.CHEBYSHEV),
}


@pytest.mark.parametrize("L,Lc", LEVELS)
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32])
@pytest.mark.parametrize("kind", [hm.CYCLE_W, hm.CYCLE_F], ids=["W", "F"])
@pytest.mark.parametrize("name", list(CYCLE_REFS))
def test_w_and_f_compositions_equal_wcycle_ref(po, name, kind, dtype, L, Lc):
    cls, op, transfer, smoother = CYCLE_REFS[name]
    bottom = hm.EXACT if (L + dtype) % 2 == 0 else hm.SMOOTH
    mode = hm.FW16 if dtype == hm.F32 else hm.CONSISTENT
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=1, mu1=2, mu2=1, smoother=smoother, dtype=dtype, restrict_mode=mode, bottom=bottom,
               op=op, schedule=hm.FMG)
    dt = np.float64 if dtype == hm.F64 else np.float32
    a = contrast(L, 10.0, 4)
    kw = dict(dtype=dt, mode=mode, omega=2.0 / 3.0, mu1=2, mu2=1, mu0=1, bottom=bottom)
    if op == hm.STENCIL5:
        ref = cls(po, {lv: po.stencil_from_nodes(a, lv, L) for lv in range(Lc, L + 1)}, L, Lc, **kw)
    else:
        ref = cls(po, po.stencil_from_nodes(a, L, L), L, Lc, **kw)
    ref.cycle = kind
    m = hm.HandleModel(po, **cfg)
    assert m.cycle == hm.CYCLE_V
    early = dtype == hm.F32                             # the kind survives set_coefficient and build_galerkin
    if early:
        m.set_cycle(kind)
    m.set_coefficient(a)
    if op == hm.GALERKIN:
        m.build_galerkin(transfer)
    if not early:
        m.set_cycle(kind)
    assert m.cycle == kind
    u, b = data(po, L, dt, 50 + L)
    m.set_guess(u)
    m.set_rhs(b)
    m.vcycle()
    assert m.U[L].dtype == dt and np.array_equal(m.U[L], ref.vcycle(L, u, b))
    # level L - 1 after the cycle: the restricted residual, and two visits from zero with that right-hand side
    v = ref.smooth(L, u, b, 2)
    rc = ref._restrict_residual(L, v, b)
    e = ref._cycle(L - 1, np.zeros_like(rc), rc, kind)
    e = ref._cycle(L - 1, e, rc, hm.CYCLE_V if kind == hm.CYCLE_F else kind)
    assert np.array_equal(m.B[L - 1], rc) and np.array_equal(m.U[L - 1], e)
    # a cycle started from an intermediate level, from a non-zero U
    top = m.U[L].copy()
    u1, b1 = data(po, L - 1, dt, 78)
    m.set_level(L - 1, 0, u1)
    m.set_level(L - 1, 1, b1)
    m.vcycle(L - 1)
    assert np.array_equal(m.U[L - 1], ref.vcycle(L - 1, u1, b1)) and np.array_equal(m.U[L], top)
    m.set_rhs(b)
    m.fmg()
    assert np.array_equal(m.U[L], ref.fmg(b))
    m.set_guess(u)
    m.vcycle_zero()
    assert np.array_equal(m.U[L], ref.vcycle(L, np.zeros_like(b), b))
    m.set_guess(u)
    st, h = m.solve(tol=0.0, max_cycles=2)
    u_ref, h_ref = ref.solve(b, u, tol=0.0, max_cycles=2, schedule=gr.FMG)
    assert np.array_equal(h, h_ref) and np.array_equal(m.U[L], u_ref) and st["cycles"] == 2
    assert st["fine_updates"] == (2 + 1) * 3.0 * float((1 << L) - 1) ** 2        # FMG: mu0 + 1 = 2 finest cycles, then one
    # back to V: the parent's bits
    m.set_cycle(hm.CYCLE_V)
    m.set_guess(u)
    m.vcycle()
    ref.cycle = hm.CYCLE_V
    assert np.array_equal(m.U[L], ref.vcycle(L, u, b))


def test_a_w_cycle_on_three_levels_by_hand(po):
    """levels 5, 4, 3, GALERKIN with bilinear transfers, double, V(2,1) smoothing, exact bottom: level 4 is visited twice,
    the second time from what the first visit left with the same right-hand side; level 3 once per visit of level 4.
    Afterwards the coarse levels hold the restricted residual and the iterate of the LAST visit"""
    L, Lc = 5, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, op=hm.GALERKIN, schedule=hm.V)
    a = contrast(L, 10.0, 6)
    h = gr.Hierarchy(po, po.stencil_from_nodes(a, L, L), L, Lc, mu1=2, mu2=1)
    u, b = data(po, L, np.float64, 31)
    S, R, A = h.smooth, (lambda r: po.restrict(r, hm.CONSISTENT)), h.residual
    v = S(5, u, b, 2)
    b4 = R(A(5, v, b))
    e4 = S(4, np.zeros_like(b4), b4, 2)                 # first visit of level 4
    b3 = R(A(4, e4, b4))
    e3 = h.bottom(b3)
    e4 = S(4, po.prolong_add(e4, e3), b4, 1)
    e4_first = e4
    e4 = S(4, e4, b4, 2)                                # second visit: from e4, with the same b4
    b3 = R(A(4, e4, b4))
    e3 = h.bottom(b3)
    e4 = S(4, po.prolong_add(e4, e3), b4, 1)
    v = S(5, po.prolong_add(v, e4), b, 1)
    for kind in (hm.CYCLE_W, hm.CYCLE_F):               # on three levels F is W: the second visit of 4 has no level to repeat
        m = hm.HandleModel(po, **cfg)
        m.set_coefficient(a)
        m.build_galerkin(hm.BILINEAR)
        m.set_cycle(kind)
        m.set_guess(u)
        m.set_rhs(b)
        m.vcycle()
        assert np.array_equal(m.U[5], v) and np.array_equal(m.B[5], b)
        assert np.array_equal(m.B[4], b4) and np.array_equal(m.U[4], e4) and not np.array_equal(e4, e4_first)
        assert np.array_equal(m.B[3], b3) and np.array_equal(m.U[3], e3)
    m.set_cycle(hm.CYCLE_V)
    m.set_guess(u)
    m.vcycle()
    assert np.array_equal(m.U[4], e4_first)


def test_set_cycle_refusals(po):
    m = hm.HandleModel(po, finest_level=6, coarsest_level=4)
    for kind in (hm.CYCLE_W, hm.CYCLE_F, hm.CYCLE_V):
        with pytest.raises(RuntimeError):
            m.set_cycle(kind)
    assert m.cycle == hm.CYCLE_V
    m = hm.HandleModel(po, finest_level=6, coarsest_level=4, op=hm.STENCIL5)
    with pytest.raises(ValueError):
        m.set_cycle(3)
    m.set_cycle(hm.CYCLE_F)
    assert m.cycle == hm.CYCLE_F


# ---- the line smoothers -----------------------------------------------------------------------------------------------
LINE_REFS = [(lr.Hierarchy, hm.GALERKIN, hm.BILINEAR), (lr.OpdepHierarchy, hm.GALERKIN, hm.OPERATOR), (lr.Stencil5, hm.STENCIL5, None)]


def line_reference(po, cls, smoother, kind, L, Lc, dt, real, cycle, **kw):
    ops = po if real is dt else lr.NumpyOps
    if cls is lr.Stencil5:
        op = {lv: as_type(operator5(po, lv, kind, dt), real) for lv in range(Lc, L + 1)}
    else:
        op = as_type(operator5(po, L, kind, dt), real)
    return cls(smoother, ops, op, L, Lc, real, cycle=cycle, **kw)


@pytest.mark.parametrize("real", ["working", "longdouble"])
@pytest.mark.parametrize("cycle", [hm.CYCLE_V, hm.CYCLE_W], ids=["V", "W"])
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32])
@pytest.mark.parametrize("cls,op,transfer", LINE_REFS, ids=["Hierarchy", "OpdepHierarchy", "Stencil5"])
def test_line_model_equals_line_ref(po, cls, op, transfer, dtype, cycle, real):
    """both sides are the same numpy statement, in the working type and in long double"""
    L, Lc = 6, 3
    smoother = [hm.LINE_ALT, hm.LINE_X, hm.LINE_Y][(dtype + cycle + (op == hm.STENCIL5)) % 3]
    bottom = hm.SMOOTH if (dtype == hm.F32 and op == hm.STENCIL5) else hm.EXACT
    mode = hm.FW16 if dtype == hm.F32 else hm.CONSISTENT
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=1, mu2=2, smoother=smoother, dtype=dtype, restrict_mode=mode, bottom=bottom,
               op=op, schedule=hm.FMG)
    dt = np.float64 if dtype == hm.F64 else np.float32
    rt = dt if real == "working" else np.longdouble
    kw = dict(mode=mode, mu1=1, mu2=2, mu0=0, bottom=bottom)
    ref = line_reference(po, cls, smoother, "layers", L, Lc, dt, rt, cycle, **kw)
    m = hm.HandleModel(po, real=None if real == "working" else np.longdouble, **cfg)
    with pytest.raises(RuntimeError):
        m.smooth(L, 1)
    m.set_cycle(cycle)
    m.set_operator("x1e-2")
    if op == hm.GALERKIN and transfer == hm.OPERATOR:
        m.build_galerkin(hm.OPERATOR)
    m.set_operator("layers")                            # GALERKIN: rebuilt with the transfer in use
    assert m.transfer == transfer and m.cycle == cycle
    u, b = data(po, L, dt, 60)
    m.set_guess(u)
    m.set_rhs(b)
    assert m.U[L].dtype == rt
    m.smooth(L, 2)
    n2 = float((1 << L) - 1) ** 2
    per = 2 if smoother == hm.LINE_ALT else 1
    assert m.fine_updates == per * 2 * n2
    assert np.array_equal(m.U[L], ref.smooth(L, u.astype(rt), b.astype(rt), 2))
    m.set_guess(u)
    m.vcycle()
    assert m.U[L].dtype == rt and np.array_equal(m.U[L], ref.vcycle(L, u.astype(rt), b.astype(rt)))
    m.fmg()
    assert np.array_equal(m.U[L], ref.fmg(b.astype(rt)))
    m.set_guess(u)
    st, h = m.solve(tol=0.0, max_cycles=2)
    u_ref, h_ref = ref.solve(b.astype(rt), u.astype(rt), tol=0.0, max_cycles=2, schedule=gr.FMG)
    assert np.array_equal(h, h_ref) and np.array_equal(m.U[L], u_ref)
    assert st["fine_updates"] == 2 * per * 3 * n2
    # after set_operator: a fresh model given the new operator
    fresh = hm.HandleModel(po, real=None if real == "working" else np.longdouble, **cfg)
    fresh.set_cycle(cycle)
    if op == hm.GALERKIN:
        fresh.set_stencil(L, operator5(po, L, "x1e-2", dt))
        fresh.build_galerkin(transfer)
    else:
        for lv in range(Lc, L + 1):
            fresh.set_stencil(lv, operator5(po, lv, "x1e-2", dt))
    m.set_operator("x1e-2")
    for x in (m, fresh):
        x.set_guess(u)
        x.set_rhs(b)
        x.vcycle()
    assert all(np.array_equal(m.U[lv], fresh.U[lv]) and np.array_equal(m.B[lv], fresh.B[lv]) for lv in m.levels())
    assert not np.array_equal(m.U[L], ref.vcycle(L, u.astype(rt), b.astype(rt)))


def test_line_model_refusals(po):
    with pytest.raises(ValueError):
        hm.HandleModel(po, smoother=hm.LINE_X)                                   # POISSON
    with pytest.raises(ValueError):
        hm.HandleModel(po, real=np.longdouble, op=hm.GALERKIN)                   # long double: line smoothers only


@pytest.mark.parametrize("name", list(gs.LINE_CASES))
def test_the_bounds_of_the_line_sequences_stay_below_the_cap(po, name):
    """the two models alone, without a device and so without adoption: every bound of THE TOLERANCE RULE that the
    sequence of a LINE_CASES seed uses stays at or below RTOL64 (double) / PCG32_STATE (float), so holding the device
    to it says something.  (A bound above the cap means the iterate has converged into the cancellation regime of
    b - A u: the sequence is changed then, never the cap.)"""
    cfg, seed, env, options = gs.LINE_CASES[name]
    calls = gs.draw_sequence(seed, cfg, **gs.LINE_OPTIONS, **options)
    m, mx = gs.line_models(po, cfg)
    cap = gs.line_cap(cfg)
    worst, held = (0.0, None), 0
    for i, call in enumerate(calls):
        want, far, bounds = gs.line_call(m, mx, cfg, call)
        if call[0] in ("solve", "solve_pcg"):
            assert len(want[1]) == len(far[1]), (i, call, want[1], far[1])
            assert want[0]["cycles"] == far[0]["cycles"] and want[0]["fine_updates"] == far[0]["fine_updates"]
        for key, (bound, scale) in bounds.items():
            held += 1
            if bound > worst[0]:
                worst = (bound, (i, call, key))
    print(f"\n[handle-state] line bounds on the CPU: {name} seed={seed} steps={len(calls)} arrays held to a bound={held} "
          f"largest bound={worst[0]:.3g} at {worst[1]} (cap {cap:g})")
    assert held > 100 and 0.0 < worst[0] <= cap, worst


# ---- the conditions the bounds of GCR_CASES rest on ----------------------------------------------------------------------
def ulp_dot(seed):
    """pcg_ref.dot with every scalar moved independently by up to one float ulp"""
    rng = np.random.RandomState(seed)

    def dot(a, b):
        return pcg_ref.dot(a, b) * (1.0 + 1.2e-7 * rng.uniform(-1.0, 1.0))

    return dot


def sync(dst, src):
    for lv in src.levels():
        dst.set_level(lv, 0, src.U[lv])
        dst.set_level(lv, 1, src.B[lv])
    dst.fine_updates = src.fine_updates


# the GCR cases of NINE_CASES join: (configuration, seed, environments, generator options, through line_step)
GCR_CONDITION_CASES = dict(gs.GCR_CASES, **{k: v + (False,) for k, v in gs.NINE_CASES.items() if v[3].get("gcr")})


@pytest.mark.parametrize("name", list(GCR_CONDITION_CASES))
def test_the_gcr_sequences_meet_the_conditions_their_bounds_rest_on(po, name):
    """the model alone through every GCR_CASES sequence, without a device:
      * double: every solve_gcr and solve_pcg call ends with its last history entry at or above 1e-6 of its first - the
        iterate never sits in the cancellation regime of b - A u, where a bound relative to max |x| means nothing
        (the smoothing of the cases is chosen for this; the sequence is changed if it fails, never the bound);
      * float: PCG32_STATE is fit for solve_gcr.  Every solve_gcr call is run a second time from the same state with
        every scalar moved independently by up to one float ulp (ulp_dot); the largest movement of any array the call
        writes, relative to its largest entry, stays at or below PCG32_STATE / 4;
      * the line case: no bound of THE TOLERANCE RULE above RTOL64"""
    cfg, seed, envs, options, line = GCR_CONDITION_CASES[name]
    calls = gs.draw_sequence(seed, cfg, **dict(options, gcr=True))
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    L = cfg["finest_level"]
    if line:
        m, mx = gs.line_models(po, cfg)
    else:
        m, mx = hm.HandleModel(po, **cfg), (None if f64 else hm.HandleModel(po, **cfg))
    lowest, moved, moved_hist, worst, held, dot = (1.0, None), (0.0, None), 0.0, (0.0, None), 0, ulp_dot(seed)
    for i, call in enumerate(calls):
        if line:
            want, far, bounds = gs.line_call(m, mx, cfg, call)
            for key, (bound, scale) in bounds.items():
                held += 1
                if bound > worst[0]:
                    worst = (bound, (i, call, key))
        elif mx is not None:
            sync(mx, m)
            want = gs.apply_model(m, call, L)
            if call[0] == "solve_gcr":
                st_x, h_x = mx.solve_gcr(tol=call[1], max_iters=call[2], restart=call[3], dot=dot)
                assert len(h_x) == len(want[1]), (i, call, h_x, want[1])
                moved_hist = max(moved_hist, float(np.max(np.abs(h_x - want[1]) / want[1])))
                for lv, which in gs.touched(cfg, call):
                    a, r = mx.get_level(lv, which == "B").astype(np.float64), m.get_level(lv, which == "B").astype(np.float64)
                    d = float(np.max(np.abs(a - r))) / float(np.max(np.abs(r)))
                    if d > moved[0]:
                        moved = (d, (i, call, lv, which))
            else:
                gs.apply_model(mx, call, L)
        else:
            want = gs.apply_model(m, call, L)
        if call[0] in gs.KRYLOV:
            h = want[1]
            if f64 and h[-1] / h[0] < lowest[0]:
                lowest = (float(h[-1] / h[0]), (i, call))
    print(f"\n[handle-state] GCR conditions on the CPU: {name} seed={seed} steps={len(calls)} lowest last/first of a Krylov call={lowest[0]:.3g} "
          f"at {lowest[1]}; one-ulp scalars move a written array by {moved[0]:.3g} at {moved[1]}, a history entry by {moved_hist:.3g}; "
          f"arrays held to a rule bound={held} largest={worst[0]:.3g} at {worst[1]}")
    if f64:
        assert 1e-6 <= lowest[0] < 1.0, lowest
        assert calls[lowest[1][0]][0] in gs.KRYLOV
    else:
        assert 0.0 < moved[0] <= gs.PCG32_STATE / 4, moved
        assert moved_hist <= gs.RTOL32 / 4, moved_hist
    if line:
        assert held > 100 and 0.0 < worst[0] <= gs.line_cap(cfg), worst


# ---- the colour smoothers and nine-point finest levels -----------------------------------------------------------------
def assert_model_equals_reference(po, m, ref, u, b, mu1, mu2, mu0, colour):
    """the model's composed schedules against the reference's own, for the cycle kinds V, W and F: a cycle from (u, b),
    level L - 1 afterwards, a cycle from L - 1 with a non-zero U, fmg, a zero-start cycle, a solve with its statistics"""
    L = m.L
    dt = u.dtype
    n2 = float((1 << L) - 1) ** 2
    for kind in (hm.CYCLE_V, hm.CYCLE_W, hm.CYCLE_F):
        m.set_cycle(kind)
        ref.cycle = kind
        m.set_guess(u)
        m.set_rhs(b)
        m.vcycle()
        assert m.U[L].dtype == dt and np.array_equal(m.U[L], ref.vcycle(L, u, b)), kind
        assert np.array_equal(m.B[L], b)
        v = ref.smooth(L, u, b, mu1, False) if colour else ref.smooth(L, u, b, mu1)
        assert np.array_equal(m.B[L - 1], ref._restrict_residual(L, v, b)), kind
        top = m.U[L].copy()
        u1, b1 = data(po, L - 1, dt, 78)
        m.set_level(L - 1, 0, u1)
        m.set_level(L - 1, 1, b1)
        m.vcycle(L - 1)
        assert np.array_equal(m.U[L - 1], ref.vcycle(L - 1, u1, b1)) and np.array_equal(m.U[L], top), kind
        m.fmg()
        assert np.array_equal(m.U[L], ref.fmg(b)), kind
        m.set_guess(u)
        m.vcycle_zero()
        assert np.array_equal(m.U[L], ref.vcycle(L, np.zeros_like(b), b)), kind
        m.set_guess(u)
        st, h = m.solve(tol=0.0, max_cycles=2)
        u_ref, h_ref = ref.solve(b, u, tol=0.0, max_cycles=2, schedule=gr.FMG)
        assert np.array_equal(h, h_ref) and np.array_equal(m.U[L], u_ref) and st["cycles"] == 2, kind
        assert st["fine_updates"] == (mu0 + 2) * (mu1 + mu2) * n2          # FMG: mu0 + 1 finest cycles, then one; one update per point and sweep
    m.set_cycle(hm.CYCLE_V)


COLOUR_REFS = {
    # name: (reference class, op, transfer)
    "Stencil5": (cf.Stencil5, hm.STENCIL5, None),
    "Hierarchy": (cf.Hierarchy, hm.GALERKIN, hm.BILINEAR),
    "OpdepHierarchy": (cf.OpdepHierarchy, hm.GALERKIN, hm.OPERATOR),
}


@pytest.mark.parametrize("bottom", [hm.EXACT, hm.SMOOTH], ids=["exact", "smooth"])
@pytest.mark.parametrize("dtype", [hm.F64, hm.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("smoother", [hm.COLOR_GS, hm.COLOR_SGS], ids=["gs", "sgs"])
@pytest.mark.parametrize("name", list(COLOUR_REFS))
@pytest.mark.parametrize("L,Lc", LEVELS)
def test_colour_models_equal_colour_ref(po, L, Lc, name, smoother, dtype, bottom):
    cls, op, transfer = COLOUR_REFS[name]
    mode = hm.FW16 if (L + dtype) % 2 else hm.CONSISTENT
    mu0, mu1, mu2 = 1, 2, 1
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=mu0, mu1=mu1, mu2=mu2, smoother=smoother, dtype=dtype, restrict_mode=mode, bottom=bottom,
               op=op, schedule=hm.FMG)
    dt = np.float64 if dtype == hm.F64 else np.float32
    a = contrast(L, 10.0, 4)
    kw = dict(dtype=dt, mode=mode, omega=2.0 / 3.0, mu1=mu1, mu2=mu2, mu0=mu0, bottom=bottom)
    if op == hm.STENCIL5:
        ref = cls(smoother, po, {lv: po.stencil_from_nodes(a, lv, L) for lv in range(Lc, L + 1)}, L, Lc, **kw)
    else:
        ref = cls(smoother, po, po.stencil_from_nodes(a, L, L), L, Lc, **kw)
    m = hm.HandleModel(po, **cfg)
    with pytest.raises(RuntimeError):
        m.smooth(L, 1)
    m.set_coefficient(a)
    if op == hm.GALERKIN:
        m.build_galerkin(transfer)
    u, b = data(po, L, dt, 90 + L)
    # mgx_smooth is forward under either smoother, on the finest level and on a coarse one (nine-point under GALERKIN)
    for lv in (L, L - 1):
        x, f = data(po, lv, dt, 91 + lv)
        m.set_level(lv, 0, x)
        m.set_level(lv, 1, f)
        m.smooth(lv, 3)
        assert np.array_equal(m.U[lv], ref.smooth(lv, x, f, 3, False))
        if smoother == hm.COLOR_SGS:
            assert not np.array_equal(m.U[lv], ref.smooth(lv, x, f, 3, True))
    assert m.fine_updates == 3.0 * float((1 << L) - 1) ** 2
    assert_model_equals_reference(po, m, ref, u, b, mu1, mu2, mu0, True)
    if bottom == hm.EXACT:
        f = data(po, Lc, dt, 9)[1]
        m.set_level(Lc, 1, f)
        m.bottom_solve()
        assert np.array_equal(m.U[Lc], ref.bottom(f))       # the oracle's dense solve (STENCIL5) against the numpy elimination


def nine_reference(po, family, transfer, st9, L, Lc, **kw):
    opdep = transfer == hm.OPERATOR
    if family in (hm.COLOR_GS, hm.COLOR_SGS):
        return (cf.NineOpdepHierarchy if opdep else cf.NineHierarchy)(family, po, st9, L, Lc, **kw)
    if family == hm.CHEBYSHEV:
        return (nr.ChebyOpdepHierarchy if opdep else nr.ChebyHierarchy)(po, st9, L, Lc, **kw)
    return (nr.OpdepHierarchy if opdep else nr.Hierarchy)(po, st9, L, Lc, **kw)


@pytest.mark.parametrize("dtype", [hm.F64, hm.F32], ids=["f64", "f32"])
@pytest.mark.parametrize("transfer", [hm.BILINEAR, hm.OPERATOR], ids=["bilinear", "operator"])
@pytest.mark.parametrize("smoother", [hm.JACOBI, hm.CHEBYSHEV, hm.COLOR_GS, hm.COLOR_SGS], ids=["jacobi", "chebyshev", "gs", "sgs"])
@pytest.mark.parametrize("L,Lc", LEVELS)
def test_nine_point_finest_models_equal_their_references(po, L, Lc, smoother, transfer, dtype):
    """set_tensor (smooth9) and set_stencil9 (random9, unsymmetric) by turns; EXACT and SMOOTH bottoms by turns"""
    tensor = (L + transfer) % 2 == 0
    bottom = hm.EXACT if (L + dtype + smoother) % 2 == 0 else hm.SMOOTH
    mode = hm.FW16 if dtype == hm.F32 else hm.CONSISTENT
    mu0, mu1, mu2 = 0, 2, 1
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=mu0, mu1=mu1, mu2=mu2, smoother=smoother, dtype=dtype, restrict_mode=mode, bottom=bottom,
               op=hm.GALERKIN, schedule=hm.FMG)
    dt = np.float64 if dtype == hm.F64 else np.float32
    st9 = hm.operator9(L, "smooth9" if tensor else "random9", dt)
    ref = nine_reference(po, smoother, transfer, st9, L, Lc, dtype=dt, mode=mode, omega=2.0 / 3.0, mu1=mu1, mu2=mu2, mu0=mu0, bottom=bottom)
    m = hm.HandleModel(po, **cfg)
    if tensor:
        m.set_tensor(*hm.tensor_nodes(L, "smooth9"))
    else:
        m.set_stencil9(L, st9)
    with pytest.raises(RuntimeError):
        m.vcycle()                                          # invalid until the build, as after set_stencil
    m.build_galerkin(transfer)
    assert all(np.array_equal(x, y) and x.dtype == dt for x, y in zip(m.h.st[L], st9)) and len(m.h.st[L]) == 9
    A = m.finest_operator()
    u, b = data(po, L, dt, 95 + L)
    assert isinstance(A, nr.Operator9) and np.array_equal(A(u), ref.apply(u))
    colour = smoother in hm.COLOURS
    assert_model_equals_reference(po, m, ref, u, b, mu1, mu2, mu0, colour)
    # single operators between two levels, with the hierarchy's transfers
    e = data(po, L - 1, dt, 11)[0]
    m.set_level(L - 1, 0, e)
    m.set_guess(u)
    m.prolong_add(L)
    want = u + ref.prolong(L, e) if transfer == hm.OPERATOR else po.prolong_add(u, e)
    assert np.array_equal(m.U[L], want)
    m.restrict(L)
    r = ref.residual(L, want, b)
    assert np.array_equal(m.B[L - 1], ref.restrict(L, r) if transfer == hm.OPERATOR else po.restrict(r, mode)) and not m.U[L - 1].any()


def test_solve_pcg_equals_pcg_ref_around_the_symmetric_colour_cycle(po):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=1, mu2=1, op=hm.GALERKIN, smoother=hm.COLOR_SGS, schedule=hm.V)
    st5 = operator5(po, L, "contrast", np.float64)
    ref = cf.Hierarchy(hm.COLOR_SGS, po, st5, L, Lc, np.float64, mu1=1, mu2=1)
    u, b = data(po, L, np.float64, 16)
    x_ref, h_ref, conv, brk = pcg_ref.pcg(pcg_ref.Operator(st5, np.float64), gcr_ref.cycle_preconditioner(ref), b, u, tol=1e-8, max_iters=40)
    m = hm.HandleModel(po, **cfg)
    m.set_operator("contrast")
    m.set_guess(u)
    m.set_rhs(b)
    st, h = m.solve_pcg(tol=1e-8, max_iters=40)
    assert conv and not brk and np.array_equal(h, h_ref) and np.array_equal(m.U[L], x_ref) and np.array_equal(m.B[L], b)
    assert st == dict(cycles=len(h_ref) - 1, converged=1, fine_updates=(len(h_ref) - 1) * 2.0 * float((1 << L) - 1) ** 2)
    # the forward-only cycle is another preconditioner: the direction is part of what solve_pcg runs
    gs_twin = hm.HandleModel(po, **dict(cfg, smoother=hm.COLOR_GS))
    gs_twin.set_operator("contrast")
    gs_twin.set_guess(u)
    gs_twin.set_rhs(b)
    assert not np.array_equal(gs_twin.solve_pcg(tol=0.0, max_iters=2)[1], h_ref[:3])


@pytest.mark.parametrize("smoother", [hm.COLOR_GS, hm.COLOR_SGS], ids=["gs", "sgs"])
def test_solve_gcr_equals_gcr_ref_around_a_nine_point_colour_hierarchy(po, smoother):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=1, mu2=1, op=hm.GALERKIN, smoother=smoother, schedule=hm.V)
    st9 = hm.operator9(L, "random9", np.float64)
    ref = cf.NineHierarchy(smoother, po, st9, L, Lc, np.float64, mu1=1, mu2=1)
    u, b = data(po, L, np.float64, 18)
    m = hm.HandleModel(po, **cfg)
    m.set_operator("random9")
    assert m.transfer == hm.BILINEAR
    assert_gcr_equals(po, m, nr.Operator9(st9), gcr_ref.cycle_preconditioner(ref), u, b, GCR_CALLS(1e-8))


@pytest.mark.parametrize("op", [hm.STENCIL5, hm.GALERKIN], ids=["stencil5", "galerkin"])
def test_the_direction_of_the_bottom_visit_is_modelled(po, op):
    """COLOR_SGS, bottom = SMOOTH, mu2 >= 1: the coarsest level sweeps mu1 times forward, then mu2 times in reverse.  One
    cycle differs from the COLOR_GS twin's - on the coarsest level already, and with mu1 = 0 and two levels nowhere else:
    the only reverse blocks a zero-start cycle then runs are the bottom's and the finest level's"""
    L, Lc = 5, 3
    out = {}
    for smoother in (hm.COLOR_GS, hm.COLOR_SGS):
        m = hm.HandleModel(po, finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, op=op, smoother=smoother, bottom=hm.SMOOTH, schedule=hm.V)
        m.set_operator("contrast")
        u, b = data(po, L, np.float64, 19)
        m.set_guess(u)
        m.set_rhs(b)
        m.vcycle()
        out[smoother] = {lv: (m.U[lv].copy(), m.B[lv].copy()) for lv in m.levels()}
        # the visit of the coarsest level by hand
        h, f = m.h, m.B[Lc]
        v = h.smooth(Lc, np.zeros_like(f), f, 2, False)
        assert np.array_equal(m.U[Lc], h.smooth(Lc, v, f, 1, True))
        if smoother == hm.COLOR_SGS:
            assert not np.array_equal(m.U[Lc], h.smooth(Lc, v, f, 1, False))
    gs_state, sgs_state = out[hm.COLOR_GS], out[hm.COLOR_SGS]
    for lv in range(Lc, L):
        assert np.array_equal(gs_state[lv][1], sgs_state[lv][1])               # the way down is forward under both
    for lv in range(Lc, L + 1):
        assert not np.array_equal(gs_state[lv][0], sgs_state[lv][0]), lv


@pytest.mark.parametrize("smoother", [hm.JACOBI, hm.COLOR_SGS], ids=["jacobi", "sgs"])
def test_tensor_coefficient_tensor_on_one_model_equals_fresh_models(po, smoother):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=1, mu2=1, op=hm.GALERKIN, smoother=smoother, schedule=hm.V)
    a = contrast(L, 100.0, 5)
    u, b = data(po, L, np.float64, 23)
    changes = [lambda m: m.set_tensor(*hm.tensor_nodes(L, "rot45")), lambda m: m.set_coefficient(a), lambda m: m.set_tensor(*hm.tensor_nodes(L, "jump9"))]

    def state(m):
        m.set_guess(u)
        m.set_rhs(b)
        out = [m.solve(tol=0.0, max_cycles=2)[1], m.solve_pcg(tol=0.0, max_iters=2)[1], m.solve_gcr(tol=0.0, max_iters=3, restart=2)[1]]
        return out + [m.U[lv].copy() for lv in m.levels()] + [m.B[lv].copy() for lv in m.levels()]

    one = hm.HandleModel(po, **cfg)
    got, want, nines = [], [], []
    for change in changes:
        change(one)
        with pytest.raises(RuntimeError):
            one.vcycle()
        one.build_galerkin(hm.OPERATOR if len(got) == 2 else hm.BILINEAR)
        nines.append((one.st9 is not None, isinstance(one.finest_operator(), nr.Operator9), len([x for x in one.h.st[L][5:] if x.any()])))
        got.append(state(one))
        fresh = hm.HandleModel(po, **cfg)
        change(fresh)
        fresh.build_galerkin(hm.OPERATOR if len(want) == 2 else hm.BILINEAR)
        want.append(state(fresh))
    assert nines == [(True, True, 4), (False, False, 0), (True, True, 4)]
    for g, w in zip(got, want):
        assert len(g) == len(w) and all(np.array_equal(x, y) for x, y in zip(g, w))
    assert not np.array_equal(got[0][3 + L - Lc], got[2][3 + L - Lc])


def test_nine_point_refusals(po):
    L = 5
    st9 = hm.operator9(L, "random9", np.float64)
    nodes = hm.tensor_nodes(L, "rot45")
    for op in (hm.STENCIL5, hm.POISSON):                    # the device: MGX_ERR_STATE
        m = hm.HandleModel(po, finest_level=L, coarsest_level=3, op=op)
        with pytest.raises(RuntimeError):
            m.set_stencil9(L, st9)
        with pytest.raises(RuntimeError):
            m.set_tensor(*nodes)
        with pytest.raises(RuntimeError):
            m.set_operator("rot45")
    m = hm.HandleModel(po, finest_level=L, coarsest_level=3, op=hm.GALERKIN)
    with pytest.raises(RuntimeError):
        m.set_stencil9(L - 1, hm.operator9(L - 1, "random9", np.float64))      # a coarse level is R A P
    with pytest.raises(RuntimeError):
        m.build_galerkin()
    for line in hm.LINES:                                   # out of scope, and the message says so
        m = hm.HandleModel(po, finest_level=L, coarsest_level=3, op=hm.GALERKIN, smoother=line)
        with pytest.raises(ValueError, match="out of scope"):
            m.set_tensor(*nodes)
        with pytest.raises(ValueError, match="out of scope"):
            m.set_stencil9(L, st9)
        m.set_operator("layers")                            # five-point: as before
    with pytest.raises(ValueError):
        hm.HandleModel(po, smoother=hm.COLOR_GS)            # POISSON
    assert (hm.COLOR_GS, hm.COLOR_SGS) == (8, 9)


def test_the_named_nine_point_operators():
    L = 5
    for kind in hm.TENSORS:
        st9 = hm.operator9(L, kind, np.float64)
        assert len(st9) == 9 and all(x.shape == (31, 31) and x.dtype == np.float64 for x in st9)
        assert any(x.any() for x in st9[5:])                # corners
        assert np.array_equal(st9[4][:, :-1], st9[3][:, 1:]) and np.array_equal(st9[8][:-1, :-1], st9[5][1:, 1:])      # symmetric
    assert all(np.array_equal(x, y) for x, y in zip(hm.operator9(L, "rot45", np.float32), nr.tensor9(*nr.rotated_tensor(L, 45.0, 0.5), dtype=np.float32)))
    st9 = hm.operator9(L, "random9", np.float64)
    assert np.max(np.abs(st9[4][:, :-1] - st9[3][:, 1:])) > 0.1 and np.max(np.abs(st9[8][:-1, :-1] - st9[5][1:, 1:])) > 0.1    # not symmetric
    assert st9[1][0, :].all() and st9[5][:, 0].all() and st9[8][-1, :].all()            # values in ring-pointing places
    ring = gs.stencil9(L, "random9_ring", np.float64, device=True)
    plain = gs.stencil9(L, "random9_ring", np.float64, device=False)
    assert all(np.array_equal(x, y) for x, y in zip(plain, st9))
    assert all(np.array_equal(x, y) for x, y in zip(nr.zero_ring(ring), nr.zero_ring(st9))) and np.max(np.abs(ring[1][0, :])) > 1e6


# ---- the sequences of COLOUR_CASES, NINE_CASES and the random9 list ------------------------------------------------------
def test_colour_and_nine_sequences_hold_what_the_generator_promises():
    assert "MGX_GS_FUSED" in gs.KNOBS
    seeds = [c[1] for d in (gs.POISSON_CASES, gs.GENERAL_CASES, gs.CYCLE_CASES, gs.LINE_CASES, gs.GCR_CASES, gs.COLOUR_CASES, gs.NINE_CASES) for c in d.values()]
    assert len(set(seeds)) == len(seeds)
    nine_calls = ("set_stencil9", "set_tensor", "set_stencil")
    # every new call kind is off by default: no sequence drawn without the operators option holds one
    for cfg, seed in list(gs.POISSON_CASES.values()) + list(gs.GENERAL_CASES.values()):
        calls = gs.draw_sequence(seed, cfg)
        assert not any(c[0] in nine_calls or (c[0] == "set_operator") for c in calls)
    for name, (cfg, seed, envs, options) in gs.COLOUR_CASES.items():
        calls = gs.draw_sequence(seed, cfg, **options)
        assert calls == gs.draw_sequence(seed, cfg, **options)
        assert set(options) <= {"cycles"} and envs[0] == {}
        users = [i for i, c in enumerate(calls) if c[0] in gs.GRAPH_USERS]
        assert gs.graph_users(calls) == gs.GRAPH_USERS and min(sum(1 for c in calls if c[0] == k) for k in gs.GRAPH_USERS) >= 5
        for lv in range(cfg["coarsest_level"], cfg["finest_level"] + 1):     # an odd-launch smooth on every level between graph users
            assert any(c[0] == "smooth" and c[1] == lv and c[2] % 2 for c in calls[users[0] + 1:users[-1]]), (name, lv)
        if options.get("cycles"):
            gs.assert_cycle_calls(calls, cfg)
        changes = [i for i, c in enumerate(calls) if c[0] in ("set_coefficient", "build_galerkin")]
        if cfg["op"] == hm.STENCIL5:
            assert [calls[i][1] for i in changes] == [10.0, 100.0, 1000.0]
        else:
            assert [calls[i][1] for i in changes if calls[i][0] == "build_galerkin"] == [hm.BILINEAR, hm.OPERATOR, hm.BILINEAR, hm.OPERATOR, hm.BILINEAR]
        for i in changes[2 if cfg["op"] == hm.GALERKIN else 1:]:             # the changes after the first operator: between graph users
            assert users[0] < i < users[-1], (name, i)
        assert not any(c[0] in nine_calls or c[0] == "set_operator" for c in calls)
    # which levels swap (k_gs_rb: five-point, a chunk of 8 rows at least - gs_fused_level of csrc/mgx_colour.hpp) and which
    # sweep in place, as the cases say
    fused = lambda cfg, lv: (cfg["op"] == hm.STENCIL5 or lv == cfg["finest_level"]) and (1 << lv) - 1 >= 8
    c = gs.COLOUR_CASES["stencil5_f64_gs_8_5"][0]
    assert all(fused(c, lv) for lv in range(5, 9)) and c["mu1"] % 2 == 1 and c["mu2"] % 2 == 0 and c["smoother"] == hm.COLOR_GS
    c = gs.COLOUR_CASES["stencil5_f32_sgs_7_3_smooth_bottom_cycles"][0]
    assert [fused(c, lv) for lv in range(3, 8)] == [False, True, True, True, True] and c["bottom"] == hm.SMOOTH and c["mu2"] >= 1 and c["dtype"] == hm.F32
    c = gs.COLOUR_CASES["galerkin_f64_sgs_7_3_cycles"][0]
    assert [fused(c, lv) for lv in range(3, 8)] == [False, False, False, False, True] and c.get("bottom", hm.EXACT) == hm.EXACT
    assert gs.COLOUR_CASES["galerkin_f64_sgs_7_3_cycles"][2] == [{}, {"MGX_SMALL_VISIT": "0"}, {"MGX_GS_FUSED": "0"}]
    assert gs.COLOUR_CASES["stencil5_f64_gs_8_5"][2] == [{}, {"MGX_GS_FUSED": "0"}]
    c = gs.COLOUR_CASES["galerkin_f32_gs_fw16_8_5_smooth_bottom"][0]
    assert c["restrict_mode"] == hm.FW16 and c["bottom"] == hm.SMOOTH and c["dtype"] == hm.F32 and c["smoother"] == hm.COLOR_GS
    orders = set()
    for name, (cfg, seed, envs, options) in gs.NINE_CASES.items():
        calls = gs.draw_sequence(seed, cfg, **options)
        assert calls == gs.draw_sequence(seed, cfg, **options)
        assert cfg["op"] == hm.GALERKIN and cfg["finest_level"] <= 8 and (cfg["coarsest_level"] <= 4 or cfg["bottom"] == hm.SMOOTH)
        gcr = options.get("gcr", False)
        gs.assert_nine_calls(calls, cfg, *options["operators"], krylov=gcr)
        if options.get("cycles"):
            gs.assert_cycle_calls(calls, cfg)
        if gcr:
            gs.assert_gcr_calls(calls, cfg, False, options.get("deep_iters", 9))
            assert gs.graph_users(calls) == gs.GCR_USERS
            orders.add(gs.krylov_order(calls))
        else:
            assert not any(c[0] == "solve_gcr" for c in calls)
        # every operator of a sequence that holds solve_pcg is symmetric
        assert "random9" not in [c[1] for c in calls if c[0] == "set_operator"] and not any(c[0] in ("set_stencil9", "set_stencil") for c in calls)
    assert orders == {"pcg", "gcr"}
    n = gs.NINE_CASES
    assert [c[1] for c in gs.draw_sequence(n["galerkin_f64_jacobi_7_3_nine_cycles"][1], n["galerkin_f64_jacobi_7_3_nine_cycles"][0],
                                           **n["galerkin_f64_jacobi_7_3_nine_cycles"][3]) if c[0] == "set_operator"] == ["rot45", "smooth9", "jump9"]
    assert n["galerkin_f64_sgs_7_3_nine_gcr"][0]["mu1"] == n["galerkin_f64_sgs_7_3_nine_gcr"][0]["mu2"] == 1      # the reverse blocks exist
    c = n["galerkin_f64_gs_8_5_nine_gcr"][0]
    assert (c["mu1"], c["mu2"], c["bottom"]) == (1, 0, hm.SMOOTH)
    # the list written by hand
    calls = list(gs.RANDOM9_CALLS)
    at = gs.flips(calls)
    assert [gs.point_counts(calls)[i] for i in at] == [5, 9] and not any(c[0] == "solve_pcg" for c in calls)
    for part in (calls[:at[0]], calls[at[0]:at[1]], calls[at[1]:]):
        assert {"solve", "solve_gcr"} <= {c[0] for c in part}
    assert calls[at[1]] == ("set_stencil9", "random9_ring")


def walk(po, cfg, calls):
    """the model alone through a sequence: every array of every level finite after every call; the lowest last / first
    history entry of a Krylov call"""
    m = hm.HandleModel(po, **cfg)
    L = cfg["finest_level"]
    lowest = (1.0, None)
    for i, call in enumerate(calls):
        out = gs.apply_model(m, call, L)
        for lv in m.levels():
            assert np.isfinite(m.U[lv]).all() and np.isfinite(m.B[lv]).all(), (i, call, lv)
        if call[0] in gs.SOLVES:
            assert np.isfinite(out[1]).all(), (i, call)
        if call[0] in gs.KRYLOV and out[1][-1] / out[1][0] < lowest[0]:
            lowest = (float(out[1][-1] / out[1][0]), (i, call))
    return lowest


NEW_SEQUENCES = ([(name, c[0], c[1], c[3]) for d in (gs.COLOUR_CASES, gs.NINE_CASES) for name, c in d.items()]
                 + [("random9_" + k, dict(finest_level=6, coarsest_level=3, mu0=0, mu1=1, mu2=1, schedule=hm.V, op=hm.GALERKIN, smoother=s), None, None)
                    for k, s in (("gs", hm.COLOR_GS), ("jacobi", hm.JACOBI))])


@pytest.mark.parametrize("name,cfg,seed,options", NEW_SEQUENCES, ids=[c[0] for c in NEW_SEQUENCES])
def test_the_model_walks_the_colour_and_nine_sequences(po, name, cfg, seed, options):
    """without a device.  Double: every Krylov call ends at or above 1e-6 of its first history entry, the condition RTOL64
    rests on for the arrays such a call writes (test_the_gcr_sequences_meet_the_conditions_their_bounds_rest_on); float:
    at or above 1e-3, where a scalar one float ulp off moves the last residual by 1e-7 / 1e-3 = 1e-4 of itself, a tenth of
    PCG32_STATE.  The sequence is changed if this fails, never the bound"""
    calls = list(gs.RANDOM9_CALLS) if seed is None else gs.draw_sequence(seed, cfg, **options)
    lowest = walk(po, cfg, calls)
    print(f"\n[handle-state] model alone: {name} steps={len(calls)} lowest last/first of a Krylov call={lowest[0]:.3g} at {lowest[1]}")
    assert (1e-6 if cfg.get("dtype", hm.F64) == hm.F64 else 1e-3) <= lowest[0] < 1.0, lowest


# ---- solve_refine ---------------------------------------------------------------------------------------------------------
def f32(st):
    return [np.asarray(x, dtype=np.float32) for x in st]


def refine_references(po, name, L, Lc):
    """(cfg of the model, how the model is given its operator, the fp64 reference hierarchy, the float32 one): the two
    hierarchies are built independently of each other and of the model, the float one IN float32 from the float32 of the
    coefficients - what include/mgx.h says the float copy holds"""
    base = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, schedule=hm.V, dtype=hm.F64)
    a = contrast(L, 10.0, 4)
    kw = dict(mu1=2, mu2=1)
    st5 = po.stencil_from_nodes(a, L, L)
    both = lambda make: (make(np.float64, lambda st: st), make(np.float32, f32))
    if name in ("stencil5-jacobi", "stencil5-chebyshev"):
        cheb = name.endswith("chebyshev")
        cls = cheby_ref.Stencil5Cheby if cheb else cheby_ref.Stencil5
        st = {lv: po.stencil_from_nodes(a, lv, L) for lv in range(Lc, L + 1)}
        refs = both(lambda dt, cast: cls(po, {lv: cast(st[lv]) for lv in st}, L, Lc, dtype=dt, **kw))
        return dict(base, op=hm.STENCIL5, smoother=hm.CHEBYSHEV if cheb else hm.JACOBI), (lambda m: m.set_coefficient(a)), refs
    give5 = lambda transfer: (lambda m: (m.set_coefficient(a), m.build_galerkin(transfer)))
    if name == "galerkin-bilinear":
        return dict(base, op=hm.GALERKIN), give5(hm.BILINEAR), both(lambda dt, cast: gr.Hierarchy(po, cast(st5), L, Lc, dtype=dt, **kw))
    if name == "galerkin-operator":
        return dict(base, op=hm.GALERKIN), give5(hm.OPERATOR), both(lambda dt, cast: od.Hierarchy(po, cast(st5), L, Lc, dtype=dt, **kw))
    if name == "nine-point":
        st9 = hm.operator9(L, "rot45", np.float64)
        return (dict(base, op=hm.GALERKIN), (lambda m: m.set_operator("rot45")),
                both(lambda dt, cast: nr.Hierarchy(po, cast(st9), L, Lc, dtype=dt, **kw)))
    if name == "colour-sgs":
        return (dict(base, op=hm.GALERKIN, smoother=hm.COLOR_SGS), give5(hm.BILINEAR),
                both(lambda dt, cast: cf.Hierarchy(hm.COLOR_SGS, po, cast(st5), L, Lc, dtype=dt, **kw)))
    if name == "w-cycle":
        return (dict(base, op=hm.GALERKIN), (lambda m: (m.set_coefficient(a), m.build_galerkin(hm.BILINEAR), m.set_cycle(hm.CYCLE_W))),
                both(lambda dt, cast: wr.with_cycle(wr.Galerkin, wr.W, po, cast(st5), L, Lc, dtype=dt, **kw)))
    if name == "bottom-smooth":
        return (dict(base, op=hm.GALERKIN, bottom=hm.SMOOTH), give5(hm.BILINEAR),
                both(lambda dt, cast: gr.Hierarchy(po, cast(st5), L, Lc, dtype=dt, bottom=hm.SMOOTH, **kw)))
    raise KeyError(name)


REFINE_REFS = ["stencil5-jacobi", "stencil5-chebyshev", "galerkin-bilinear", "galerkin-operator", "nine-point", "colour-sgs", "w-cycle", "bottom-smooth"]


@pytest.mark.parametrize("name", REFINE_REFS)
def test_solve_refine_equals_refine_ref_around_independent_hierarchies(po, name):
    """iterate and history bit for bit; B and every coarse level untouched; fine_updates those of the float cycle; the
    stop by the tolerance; max_cycles = 0; the scales of a history handed in"""
    import refine_ref as rr
    L, Lc = 6, 3
    cfg, give, (h64, h32) = refine_references(po, name, L, Lc)
    assert all(x.dtype == np.float32 for x in h32.st[L]) and all(x.dtype == np.float64 for x in h64.st[L])
    u, b = data(po, L, np.float64, 61)
    cycle32 = gcr_ref.cycle_preconditioner(h32)
    residual = lambda v, f: h64.residual(L, v, f)
    m = hm.HandleModel(po, **cfg)
    give(m)
    for lv in m.levels():
        if lv < L:
            m.set_level(lv, 0, data(po, lv, np.float64, 70 + lv)[0])
            m.set_level(lv, 1, data(po, lv, np.float64, 80 + lv)[0])
    coarse = {lv: (m.U[lv].copy(), m.B[lv].copy()) for lv in m.levels() if lv < L}
    n2 = float((1 << L) - 1) ** 2
    for tol, k in ((0.0, 4), (1e-2, 30), (0.5, 0)):
        u_ref, h_ref = rr.refine(residual, cycle32, b, u, tol=tol, max_cycles=k, norm=po.norm2)
        m.set_guess(u)
        m.set_rhs(b)
        st, h = m.solve_refine(tol=tol, max_cycles=k)
        assert np.array_equal(h, h_ref) and np.array_equal(m.U[L], u_ref) and m.U[L].dtype == np.float64, (name, tol, k)
        assert np.array_equal(m.B[L], b)
        assert st == dict(cycles=len(h_ref) - 1, converged=int(h_ref[-1] <= tol * h_ref[0]), fine_updates=(len(h_ref) - 1) * 3.0 * n2), st
        for lv, (uu, bb) in coarse.items():
            assert np.array_equal(m.U[lv], uu) and np.array_equal(m.B[lv], bb), lv
    assert len(h) == 1 and np.array_equal(m.U[L], u) and st["converged"] == 0          # max_cycles = 0
    assert np.isfinite(h_ref).all()
    # a history handed in gives the scales and nothing else.  (Scaling by a power of two is exact: the iterate changes only
    # where the scale pushes the float residual out of the normal range - 2^120 too large here)
    _, h4 = m.solve_refine(tol=0.0, max_cycles=4)
    m.set_guess(u)
    far = h4 * 2.0 ** 120
    st, h = m.solve_refine(tol=0.0, max_cycles=4, history=far)
    u_ref, h_ref = rr.refine(residual, cycle32, b, u, history=far, norm=po.norm2)
    assert st["cycles"] == 4 and np.array_equal(m.U[L], u_ref) and np.array_equal(h, h_ref) and not np.array_equal(h, h4)
    m.set_guess(u)
    assert np.array_equal(m.solve_refine(tol=0.0, max_cycles=4, history=h4)[1], h4)       # its own history: the same call


def refined(m, u, b, k=3):
    m.set_guess(u)
    m.set_rhs(b)
    st, h = m.solve_refine(tol=0.0, max_cycles=k)
    return st, h, m.U[m.L].copy()


def test_the_float_model_follows_operator_transfer_and_cycle_changes(po):
    """operator A -> refine -> operator B -> refine -> the other transfer with the same coefficients -> refine ->
    set_cycle(W) -> refine on ONE model: every refine is that of a fresh model in the same state"""
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, op=hm.GALERKIN, schedule=hm.V)
    a1, a2 = contrast(L, 10.0, 1), contrast(L, 100.0, 2)
    u, b = data(po, L, np.float64, 62)
    steps = [lambda m: (m.set_coefficient(a1), m.build_galerkin(hm.BILINEAR)), lambda m: (m.set_coefficient(a2), m.build_galerkin(hm.BILINEAR)),
             lambda m: m.build_galerkin(hm.OPERATOR), lambda m: m.set_cycle(hm.CYCLE_W)]
    one = hm.HandleModel(po, **cfg)
    seen, floats = [], []
    for i, change in enumerate(steps):
        change(one)
        if i == 0:
            with pytest.raises(ValueError):
                one.time_refine_pass(2)                     # before the first solve_refine
        st, h, x = refined(one, u, b)
        floats.append(one.f32)
        fresh = hm.HandleModel(po, **cfg)
        for earlier in steps[:i + 1]:
            if not (i >= 1 and earlier is steps[0]):        # (operator A is overwritten by B)
                earlier(fresh)
        st_f, h_f, x_f = refined(fresh, u, b)
        assert st == st_f and np.array_equal(h, h_f) and np.array_equal(x, x_f), i
        assert all(not np.array_equal(x, y) for y in seen), i
        seen.append(x)
        before = [one.U[lv].copy() for lv in one.levels()] + [one.B[lv].copy() for lv in one.levels()]
        one.time_refine_pass(2)
        assert all(np.array_equal(p, q) for p, q in zip(before, [one.U[lv] for lv in one.levels()] + [one.B[lv] for lv in one.levels()]))
    assert floats[0] is not floats[1] and floats[1] is not floats[2]       # rebuilt after an operator and after a transfer change
    assert floats[2] is floats[3] and one.f32.cycle == hm.CYCLE_W            # set_cycle reaches it at once, nothing is rebuilt
    assert one.f32.cfg["dtype"] == hm.F32 and one.f32.transfer == hm.OPERATOR and all(x.dtype == np.float32 for x in one.f32.h.st[L])


def test_stencil5_float_model_holds_the_float32_of_every_level(po):
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, op=hm.STENCIL5, schedule=hm.V)
    m = hm.HandleModel(po, **cfg)
    m.set_coefficient(contrast(L, 10.0, 1))
    u, b = data(po, L, np.float64, 63)
    x1 = refined(m, u, b)[2]
    m.set_coefficient(contrast(L, 1000.0, 3))
    x2 = refined(m, u, b)[2]
    for lv in m.levels():
        for p, q in zip(m.f32.stencils[lv], m.stencils[lv]):
            assert p.dtype == np.float32 and np.array_equal(p, q.astype(np.float32)), lv
    assert not np.array_equal(x1, x2)


def test_solve_refine_refusals(po):
    L, Lc = 5, 3
    base = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=1, mu2=1, schedule=hm.V)
    a = contrast(L, 10.0, 1)
    for m in (hm.HandleModel(po, **base), hm.HandleModel(po, dtype=hm.F32, **base)):                        # POISSON
        with pytest.raises(ValueError):
            m.solve_refine(1e-8, 3)
        with pytest.raises(ValueError):
            m.time_refine_pass(2)
    m = hm.HandleModel(po, op=hm.STENCIL5, dtype=hm.F32, **base)                                             # F32 (MIXED: no model at all)
    m.set_coefficient(a)
    with pytest.raises(ValueError):
        m.solve_refine(1e-8, 3)
    m = hm.HandleModel(po, op=hm.GALERKIN, **base)
    with pytest.raises(ValueError):
        m.solve_refine(1e-8, 3)                             # unset
    m.set_coefficient(a)
    with pytest.raises(ValueError):
        m.solve_refine(1e-8, 3)                             # unbuilt
    m.build_galerkin()
    m.set_rhs(data(po, L, np.float64, 64)[1])
    assert m.solve_refine(0.0, 1)[0]["cycles"] == 1
    m.set_coefficient(a)
    with pytest.raises(ValueError):
        m.time_refine_pass(2)                               # invalid again until the build
    m = hm.HandleModel(po, op=hm.STENCIL5, **base)
    m.set_stencil(L, operator5(po, L, "layers", np.float64))
    with pytest.raises(ValueError):
        m.solve_refine(1e-8, 3)                             # a STENCIL5 handle with levels missing
    for line in hm.LINES:                                   # not modelled, and the message says so
        for real in (None, np.longdouble):
            m = hm.HandleModel(po, real=real, op=hm.GALERKIN, smoother=line, **base)
            m.set_operator("layers")
            with pytest.raises(ValueError, match="not modelled"):
                m.solve_refine(1e-8, 3)


def test_refine_sequences_hold_what_the_generator_promises():
    seeds = [c[1] for d in (gs.POISSON_CASES, gs.GENERAL_CASES, gs.CYCLE_CASES, gs.LINE_CASES, gs.GCR_CASES, gs.COLOUR_CASES, gs.NINE_CASES, gs.REFINE_CASES)
             for c in d.values()]
    assert len(set(seeds)) == len(seeds)
    # off by default: no sequence drawn without the option holds either call
    for cfg, seed in list(gs.POISSON_CASES.values()) + list(gs.GENERAL_CASES.values()):
        assert not any(c[0] in ("solve_refine", "time_refine_pass") for c in gs.draw_sequence(seed, cfg))
    for name, (cfg, seed, envs, options) in gs.REFINE_CASES.items():
        calls = gs.draw_sequence(seed, cfg, **gs.REFINE_OPTIONS, **options)
        assert calls == gs.draw_sequence(seed, cfg, **gs.REFINE_OPTIONS, **options)
        assert cfg.get("dtype", hm.F64) == hm.F64 and envs[0] == {}
        gcr = options.get("gcr", False)
        gs.assert_refine_calls(calls, cfg, gcr)
        assert gs.graph_users(calls) == (gs.GCR_USERS if gcr else gs.GRAPH_USERS) + ("solve_refine",)
        assert min(sum(1 for c in calls if c[0] == k) for k in gs.graph_users(calls)) >= 5
        # without the option: the same list with the refine stage's calls taken out
        plain = gs.draw_sequence(seed, cfg, **dict(gs.REFINE_OPTIONS, refine=False), **options)
        rest = [c for c in calls if c[0] not in ("solve_refine", "time_refine_pass") and not (c[0] == "set_guess" and 4000 < c[1] < 4100)]
        extra = [("vcycle", next(calls[i + 1][1] for i, c in enumerate(calls) if c[0] == "solve_refine" and calls[i + 1][0] == "vcycle"
                                 and calls[i + 2] == ("restrict", cfg["finest_level"]))), ("restrict", cfg["finest_level"]), ("prolong_add", cfg["finest_level"])]
        assert len(rest) == len(plain) + 3 and sorted(map(repr, rest)) == sorted(map(repr, plain + extra)), name
        if options.get("cycles"):
            gs.assert_cycle_calls(calls, cfg)
        if gcr:
            gs.assert_gcr_calls(calls, cfg)
        if cfg["op"] == hm.STENCIL5:
            assert [c[1] for c in calls if c[0] == "set_coefficient"] == [10.0, 100.0, 1000.0]
        if cfg.get("bottom", hm.EXACT) == hm.EXACT:         # the float dense solve: held by an F32 sequence for STENCIL5 at level 5 only
            assert cfg["op"] == hm.STENCIL5 and cfg["coarsest_level"] == 5 and gs.GENERAL_CASES["stencil5_f32_chebyshev"][0]["dtype"] == hm.F32
    c = gs.REFINE_CASES["galerkin_f64_jacobi_7_3_refine_cycles"]
    calls = gs.draw_sequence(c[1], c[0], **gs.REFINE_OPTIONS, **c[3])
    builds = [i for i, x in enumerate(calls) if x[0] == "build_galerkin"]
    assert [calls[i][1] for i in builds] == [hm.BILINEAR, hm.OPERATOR, hm.BILINEAR, hm.OPERATOR, hm.BILINEAR]
    transfer_only = [i for i in builds[1:] if calls[i - 1][0] != "set_coefficient"]
    assert len(transfer_only) >= 2                          # ... each followed by a refine before any other graph user: (a)
    assert c[2] == [{}, {"MGX_SMALL_VISIT": "0"}, {"MGX_GRAPH": "0"}]
    c = gs.REFINE_CASES["galerkin_f64_sgs_7_3_nine_refine"]
    calls = gs.draw_sequence(c[1], c[0], **gs.REFINE_OPTIONS, **c[3])
    assert [gs.point_counts(calls)[i] for i in gs.flips(calls)] == [5, 9] and c[2] == [{}, {"MGX_GS_FUSED": "0"}]
    c = gs.REFINE_CASES["galerkin_f64_gs_8_5_smooth_bottom_refine_gcr"][0]
    assert (c["mu1"], c["mu2"], c["bottom"], c["smoother"]) == (1, 0, hm.SMOOTH, hm.COLOR_GS)


@pytest.mark.parametrize("name", list(gs.REFINE_CASES))
def test_the_model_walks_the_refine_sequences(po, name):
    """without a device: every array finite after every call (walk); every solve_refine history finite and lower at its end
    than at its start (a call of no cycle aside); every double Krylov call at or above 1e-6 of its first entry"""
    cfg, seed, envs, options = gs.REFINE_CASES[name]
    calls = gs.draw_sequence(seed, cfg, **gs.REFINE_OPTIONS, **options)
    m = hm.HandleModel(po, **cfg)
    lowest, slowest = (1.0, None), (0.0, None)
    for i, call in enumerate(calls):
        before = {lv: (m.U[lv], m.B[lv]) for lv in m.levels()}
        out = gs.apply_model(m, call, cfg["finest_level"])
        for lv in m.levels():
            assert np.isfinite(m.U[lv]).all() and np.isfinite(m.B[lv]).all(), (i, call, lv)
        if call[0] in gs.SOLVES:
            assert np.isfinite(out[1]).all(), (i, call)
        if call[0] == "solve_refine":
            st, h = out
            assert st["cycles"] == len(h) - 1 <= call[2] and (call[1] > 0.0 or st["cycles"] == call[2]), (i, call, st)
            if call[2]:
                assert st["cycles"] >= 1 and h[-1] < h[0], (i, call, h)
                slowest = max(slowest, (float(h[-1] / h[0]), (i, call)))
            for lv in m.levels():                           # only U of the finest level moves
                assert m.B[lv] is before[lv][1] and (lv == m.L or m.U[lv] is before[lv][0]), (i, call, lv)
        if call[0] in gs.KRYLOV and out[1][-1] / out[1][0] < lowest[0]:
            lowest = (float(out[1][-1] / out[1][0]), (i, call))
    print(f"\n[handle-state] model alone: {name} steps={len(calls)} lowest last/first of a Krylov call={lowest[0]:.3g} at {lowest[1]}; "
          f"highest last/first of a solve_refine={slowest[0]:.3g} at {slowest[1]}")
    assert 1e-6 <= lowest[0] < 1.0, lowest


# ---- solve_refine_gcr -----------------------------------------------------------------------------------------------------
REFINE_GCR_REFS = ["stencil5-jacobi", "galerkin-bilinear", "galerkin-operator", "nine-point", "colour-sgs", "w-cycle", "bottom-smooth"]


@pytest.mark.parametrize("name", REFINE_GCR_REFS)
def test_solve_refine_gcr_equals_refine_gcr_ref_around_independent_hierarchies(po, name):
    """iterate and history bit for bit against refine_gcr_ref.refine_gcr over reference hierarchies built independently of
    the model - A from the float64 one's residual (the sign flip is exact), the cycle from the float32 one; B (the same
    array) and every coarse level untouched; fine_updates those of the float cycle; the stop by the tolerance;
    max_iters = 0; a history and a dot handed in are passed through"""
    import refine_gcr_ref as rg
    L, Lc = 6, 3
    cfg, give, (h64, h32) = refine_references(po, name, L, Lc)
    assert all(x.dtype == np.float32 for x in h32.st[L]) and all(x.dtype == np.float64 for x in h64.st[L])
    u, b = data(po, L, np.float64, 61)
    zero = np.zeros_like(b)
    A = lambda v: -h64.residual(L, v, zero)
    cycle32 = gcr_ref.cycle_preconditioner(h32)
    m = hm.HandleModel(po, **cfg)
    give(m)
    for lv in m.levels():
        if lv < L:
            m.set_level(lv, 0, data(po, lv, np.float64, 70 + lv)[0])
            m.set_level(lv, 1, data(po, lv, np.float64, 80 + lv)[0])
    coarse = {lv: (m.U[lv], m.B[lv]) for lv in m.levels() if lv < L}
    n2 = float((1 << L) - 1) ** 2
    for tol, k, restart in ((0.0, 5, 3), (1e-2, 30, 4), (0.0, 3, 1), (0.5, 0, 2)):
        x_ref, h_ref, conv, brk = rg.refine_gcr(A, cycle32, b, u, tol, k, restart)
        m.set_guess(u)
        m.set_rhs(b)
        held = m.B[L]
        st, h = m.solve_refine_gcr(tol=tol, max_iters=k, restart=restart)
        assert not brk and np.array_equal(h, h_ref) and np.array_equal(m.U[L], x_ref) and m.U[L].dtype == np.float64, (name, tol, k, restart)
        assert m.B[L] is held and np.array_equal(m.B[L], b)
        assert st == dict(cycles=len(h_ref) - 1, converged=int(conv), fine_updates=(len(h_ref) - 1) * 3.0 * n2), st
        assert np.all(h[1:] <= h[:-1])
        for lv, (uu, bb) in coarse.items():
            assert m.U[lv] is uu and m.B[lv] is bb, lv
    assert len(h) == 1 and np.array_equal(m.U[L], u) and st["converged"] == 0          # max_iters = 0
    # a history handed in gives the scales, a dot the scalars, and nothing else
    _, h5 = m.solve_refine_gcr(tol=0.0, max_iters=5, restart=3)
    far = h5 * 2.0 ** 120
    for kw in (dict(history=far), dict(dot=gcr_ref.dot_reversed), dict(history=h5, dot=rg.device_dot)):
        m.set_guess(u)
        st, h = m.solve_refine_gcr(tol=0.0, max_iters=5, restart=3, **kw)
        x_ref, h_ref, _, _ = rg.refine_gcr(A, cycle32, b, u, 0.0, 5, 3, **kw)
        assert st["cycles"] == 5 and np.array_equal(m.U[L], x_ref) and np.array_equal(h, h_ref), kw
        assert not np.array_equal(h, h5), kw
    m.set_guess(u)
    assert np.array_equal(m.solve_refine_gcr(tol=0.0, max_iters=5, restart=3, history=h5)[1], h5)       # its own history: the same call


def refined_gcr(m, u, b, k=4, restart=3):
    m.set_guess(u)
    m.set_rhs(b)
    st, h = m.solve_refine_gcr(tol=0.0, max_iters=k, restart=restart)
    return st, h, m.U[m.L].copy()


def test_solve_refine_gcr_follows_operator_transfer_and_cycle_changes_and_shares_the_float_model(po):
    """operator A -> call -> operator B -> call -> the other transfer -> call -> set_cycle(W) -> call on ONE model, a
    solve_refine before every second of them: every call is that of a fresh model in the same state, and the float model
    is one object for both entry points - rebuilt by whichever comes first after a change"""
    L, Lc = 6, 3
    cfg = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=2, mu2=1, op=hm.GALERKIN, schedule=hm.V)
    a1, a2 = contrast(L, 10.0, 1), contrast(L, 100.0, 2)
    u, b = data(po, L, np.float64, 62)
    steps = [lambda m: (m.set_coefficient(a1), m.build_galerkin(hm.BILINEAR)), lambda m: (m.set_coefficient(a2), m.build_galerkin(hm.BILINEAR)),
             lambda m: m.build_galerkin(hm.OPERATOR), lambda m: m.set_cycle(hm.CYCLE_W)]
    one = hm.HandleModel(po, **cfg)
    seen, floats = [], []
    for i, change in enumerate(steps):
        change(one)
        if i % 2:                                           # solve_refine rebuilds the float model, the call finds it current
            refined(one, u, b)
            shared = one.f32
        st, h, x = refined_gcr(one, u, b)
        assert i % 2 == 0 or one.f32 is shared
        floats.append(one.f32)
        fresh = hm.HandleModel(po, **cfg)
        for earlier in steps[:i + 1]:
            if not (i >= 1 and earlier is steps[0]):        # (operator A is overwritten by B)
                earlier(fresh)
        st_f, h_f, x_f = refined_gcr(fresh, u, b)
        assert st == st_f and np.array_equal(h, h_f) and np.array_equal(x, x_f), i
        assert all(not np.array_equal(x, y) for y in seen), i
        seen.append(x)
        # ... and the solve_refine after it is a fresh model's too: the call left the float model as solve_refine needs it
        s2, h2, x2 = refined(one, u, b)
        s2f, h2f, x2f = refined(fresh, u, b)
        assert s2 == s2f and np.array_equal(h2, h2f) and np.array_equal(x2, x2f) and one.f32 is floats[-1], i
    assert floats[0] is not floats[1] and floats[1] is not floats[2]       # rebuilt after an operator and after a transfer change
    assert floats[2] is floats[3] and one.f32.cycle == hm.CYCLE_W            # set_cycle reaches it at once, nothing is rebuilt
    assert one.f32.cfg["dtype"] == hm.F32 and one.f32.transfer == hm.OPERATOR


def test_solve_refine_gcr_and_its_timing_call_refuse_where_the_device_does(po):
    L, Lc = 5, 3
    base = dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=1, mu2=1, schedule=hm.V)
    a = contrast(L, 10.0, 1)
    for m in (hm.HandleModel(po, **base), hm.HandleModel(po, dtype=hm.F32, **base)):                        # POISSON
        with pytest.raises(ValueError):
            m.solve_refine_gcr(1e-8, 3, 2)
        with pytest.raises(ValueError):
            m.time_refine_gcr_pass(0, 2)
    m = hm.HandleModel(po, op=hm.STENCIL5, dtype=hm.F32, **base)
    m.set_coefficient(a)
    with pytest.raises(ValueError):
        m.solve_refine_gcr(1e-8, 3, 2)
    m = hm.HandleModel(po, op=hm.GALERKIN, **base)
    with pytest.raises(ValueError):
        m.solve_refine_gcr(1e-8, 3, 2)                      # unset
    m.set_coefficient(a)
    with pytest.raises(ValueError):
        m.solve_refine_gcr(1e-8, 3, 2)                      # unbuilt
    m.build_galerkin()
    u, b = data(po, L, np.float64, 64)
    m.set_rhs(b)
    m.set_guess(u)
    for kw in (dict(restart=0), dict(restart=9), dict(tol=-1.0), dict(tol=float("nan")), dict(max_iters=-1)):
        with pytest.raises(ValueError, match="MGX_ERR_INVALID"):
            m.solve_refine_gcr(**dict(dict(tol=1e-8, max_iters=3, restart=2), **kw))
    assert np.array_equal(m.U[L], u) and m.f32 is None      # a refused call has touched nothing
    # the timing call: the float model AND slot 0 of the basis - what the device's guard looks at, not which call made them
    with pytest.raises(ValueError):
        m.time_refine_gcr_pass(0, 2)
    m.solve_refine(0.0, 1)
    with pytest.raises(ValueError):
        m.time_refine_gcr_pass(0, 2)                        # the float model alone
    m.solve_gcr(0.0, 1, 1)
    state = lambda: [m.U[lv] for lv in m.levels()] + [m.B[lv] for lv in m.levels()]
    before = state()
    for which in (0, 1):
        m.time_refine_gcr_pass(which, 2)                    # solve_refine + solve_gcr: accepted, as the device does
    assert all(p is q for p, q in zip(before, state()))     # nothing moves
    for which, reps in ((2, 1), (-1, 1), (0, 0)):
        with pytest.raises(ValueError, match="MGX_ERR_INVALID"):
            m.time_refine_gcr_pass(which, reps)
    other = hm.HandleModel(po, op=hm.GALERKIN, **base)
    other.set_coefficient(a)
    other.build_galerkin()
    other.set_rhs(b)
    other.solve_gcr(0.0, 1, 1)
    with pytest.raises(ValueError):
        other.time_refine_gcr_pass(1, 2)                    # the basis alone
    assert other.solve_refine_gcr(0.0, 0, 1)[0]["cycles"] == 0
    other.time_refine_gcr_pass(1, 2)                        # a call of no iteration has created both
    other.set_coefficient(a)
    with pytest.raises(ValueError):
        other.time_refine_gcr_pass(1, 2)                    # invalid again until the build
    for line in hm.LINES:                                   # not modelled, and the message says so
        m = hm.HandleModel(po, op=hm.GALERKIN, smoother=line, **base)
        m.set_operator("layers")
        with pytest.raises(ValueError, match="not modelled"):
            m.solve_refine_gcr(1e-8, 3, 2)


def test_a_breakdown_leaves_the_model_where_the_device_is_left(po):
    """tests/test_gpu_refine_gcr.py's breakdown: no smoothing, full weighting of a checkerboard is zero at every coarse
    point, so the float cycle returns zero and q'.q' = 0 at iteration 1 - one history entry, U the guess, converged 0"""
    L, Lc = 6, 3
    m = hm.HandleModel(po, finest_level=L, coarsest_level=Lc, mu0=0, mu1=0, mu2=0, schedule=hm.V, op=hm.GALERKIN)
    m.set_coefficient(contrast(L, 10.0, 1))
    m.build_galerkin()
    n = m.n(L)
    i = np.arange(n)
    b = np.where((i[:, None] + i[None, :]) % 2 == 0, 1.0, -1.0)
    m.set_rhs(b)
    m.set_guess(np.zeros((n, n)))
    st, h = m.solve_refine_gcr(0.0, 6, 4)
    assert st == dict(cycles=0, converged=0, fine_updates=0.0) and np.array_equal(h, [float(n)]) and not m.U[L].any() and np.array_equal(m.B[L], b)
    m.set_guess(data(po, L, np.float64, 65)[0])             # a residual that is no checkerboard: the exit depends on it alone
    st, h = m.solve_refine_gcr(0.0, 3, 4)
    assert st["cycles"] == 3 and h[-1] < h[0]


def test_refine_gcr_sequences_hold_what_the_generator_promises():
    seeds = [c[1] for d in (gs.POISSON_CASES, gs.GENERAL_CASES, gs.CYCLE_CASES, gs.LINE_CASES, gs.GCR_CASES, gs.COLOUR_CASES, gs.NINE_CASES, gs.REFINE_CASES,
                            gs.REFINE_GCR_CASES) for c in d.values()]
    assert len(set(seeds)) == len(seeds)
    stage = ("solve_refine_gcr", "time_refine_gcr_pass")
    # off by default: no sequence drawn without the option holds either call
    for cfg, seed, envs, options in gs.REFINE_CASES.values():
        assert not any(c[0] in stage for c in gs.draw_sequence(seed, cfg, **gs.REFINE_OPTIONS, **options))
    for name, (cfg, seed, envs, options) in gs.REFINE_GCR_CASES.items():
        calls = gs.draw_sequence(seed, cfg, **gs.REFINE_GCR_OPTIONS, **options)
        assert calls == gs.draw_sequence(seed, cfg, **gs.REFINE_GCR_OPTIONS, **options)
        assert cfg.get("dtype", hm.F64) == hm.F64 and envs[0] == {}
        cycles = options.get("cycles", False)
        gs.assert_refine_gcr_calls(calls, cfg, cycles)
        gs.assert_refine_calls(calls, cfg, True)            # the stage keeps out of what refine_stage promised ...
        gs.assert_gcr_calls(calls, cfg, False, options.get("deep_iters", gs.DEEP_GCR[2]))
        if cycles:
            gs.assert_cycle_calls(calls, cfg)
        assert gs.graph_users(calls) == gs.GCR_USERS + gs.REFINE_USERS
        assert min(sum(1 for c in calls if c[0] == k) for k in gs.graph_users(calls)) >= 5
        # ... and without the option the list is the same with the stage's calls taken out: its calls, their fresh guesses,
        # and the one solve_refine of promise (c)
        plain = gs.draw_sequence(seed, cfg, **dict(gs.REFINE_GCR_OPTIONS, refine_gcr=False), **options)
        mid = [j for j, c in enumerate(calls) if c == ("solve_refine", 0.0, 2) and calls[j - 1][0] == calls[j + 1][0] == "solve_refine_gcr"]
        assert len(mid) == 1
        rest = [c for j, c in enumerate(calls) if j != mid[0] and c[0] not in stage and not (c[0] == "set_guess" and 5000 < c[1] < 6000)]
        assert rest == plain, name
        if cfg["op"] == hm.STENCIL5:
            assert [c[1] for c in calls if c[0] == "set_coefficient"] == [10.0, 100.0, 1000.0]
            far = next(i for i, c in enumerate(calls) if c[0] == "set_coefficient" and c[1] == 1000.0)
            assert all(c[2] <= 2 for c in calls[far:] if c[0] == "solve_refine_gcr")           # short where the cycle diverges
        if cfg.get("bottom", hm.EXACT) == hm.EXACT:         # the float dense solve: held by an F32 sequence for STENCIL5 at level 5 only
            assert cfg["op"] == hm.STENCIL5 and cfg["coarsest_level"] == 5
    c = gs.REFINE_GCR_CASES["galerkin_f64_jacobi_7_3_smooth_bottom_refine_gcr_cycles"]
    assert c[2] == [{}, {"MGX_SMALL_VISIT": "0"}, {"MGX_GRAPH": "0"}] and c[0]["bottom"] == hm.SMOOTH and c[3] == dict(cycles=True)
    c = gs.REFINE_GCR_CASES["galerkin_f64_sgs_7_3_nine_refine_gcr"]
    calls = gs.draw_sequence(c[1], c[0], **gs.REFINE_GCR_OPTIONS, **c[3])
    assert calls[0] == ("set_operator", "rot45") and [gs.point_counts(calls)[i] for i in gs.flips(calls)] == [5, 9]
    assert [x[0] for x in calls if x[0] in ("set_coefficient", "set_stencil9")] == ["set_coefficient", "set_stencil9"]


@pytest.mark.parametrize("name", list(gs.REFINE_GCR_CASES))
def test_the_model_walks_the_refine_gcr_sequences(po, name):
    """without a device (numpy's order of the dots): every array finite after every call; every solve_refine_gcr runs the
    iterations it was asked for, its history never increases and ends below its first entry, and only U of the finest level
    moves; every solve_refine history ends below its first entry; every double Krylov call at or above 1e-6 of its first
    entry.  The sequence is changed if this fails, never a bound"""
    cfg, seed, envs, options = gs.REFINE_GCR_CASES[name]
    calls = gs.draw_sequence(seed, cfg, **gs.REFINE_GCR_OPTIONS, **options)
    m = hm.HandleModel(po, **cfg)
    lowest, slowest = (1.0, None), (0.0, None)
    for i, call in enumerate(calls):
        before = {lv: (m.U[lv], m.B[lv]) for lv in m.levels()}
        out = gs.apply_model(m, call, cfg["finest_level"])
        for lv in m.levels():
            assert np.isfinite(m.U[lv]).all() and np.isfinite(m.B[lv]).all(), (i, call, lv)
        if call[0] in gs.SOLVES:
            assert np.isfinite(out[1]).all(), (i, call)
        if call[0] in gs.REFINE_USERS:
            st, h = out
            if call[0] == "solve_refine_gcr":
                assert st["cycles"] == len(h) - 1 == call[2] and st["converged"] == 0, (i, call, st)
                assert np.all(h[1:] <= h[:-1]), (i, call, h)
            if call[2]:
                assert st["cycles"] >= 1 and h[-1] < h[0], (i, call, h)
                slowest = max(slowest, (float(h[-1] / h[0]), (i, call)))
            for lv in m.levels():
                assert m.B[lv] is before[lv][1] and (lv == m.L or m.U[lv] is before[lv][0]), (i, call, lv)
        if call[0].startswith("time_refine"):
            assert all(m.U[lv] is before[lv][0] and m.B[lv] is before[lv][1] for lv in m.levels()), (i, call)
        if call[0] in gs.KRYLOV and out[1][-1] / out[1][0] < lowest[0]:
            lowest = (float(out[1][-1] / out[1][0]), (i, call))
    print(f"\n[handle-state] model alone: {name} steps={len(calls)} lowest last/first of a Krylov call={lowest[0]:.3g} at {lowest[1]}; "
          f"highest last/first of a refining call={slowest[0]:.3g} at {slowest[1]}")
    assert 1e-6 <= lowest[0] < 1.0, lowest
