"""Keeps tests/handle_model.py honest (no GPU): the schedules it composes from its own single operators must give
the bits of the references' own schedules - oracle/pyoracle.py's Solver for the constant stencil, the hierarchies of
tests/galerkin_ref.py, tests/opdep_ref.py and tests/cheby_ref.py for the general operators - and its solves their
histories; the coarse levels must hold afterwards what the documented operator sequence leaves there."""
import numpy as np
import pytest

import cheby_ref
import galerkin_ref as gr
import handle_model as hm
import opdep_ref as od
import pcg_ref

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
