"""GPU checks of mgx_solve_gcr (restarted GCR around one multigrid cycle from zero; csrc/mgx_krylov.hpp) against the numpy
statement of the same algorithm (tests/gcr_ref.py, pinned by tests/test_gcr_cpu.py) with the reference's cycle as M.

Tolerances.  Where the device cycle is the reference's operation for operation (Jacobi cycles of the POISSON, STENCIL5
and GALERKIN hierarchies) the device differs from the reference only in the summation order of the dots, a relative
1e-16 in each scalar: the argument and the bound of tests/test_gpu_pcg.py, same iteration count and every fp64 entry
within 1e-9 relative plus 1e-14 ||r0||.  (gcr_ref with its dots summed from the other end moves these histories by at
most 4e-10 relative at 5e-12 ||r0||, 1.4e-4 of that bound: tests/test_gcr_cpu.py holds the reference to it.)  fp32: 1e-3
relative with the count within one.  The zebra line sweeps agree with numpy to rounding only (tests/test_gpu_line.py),
so the line cycles are held to counts, monotonicity and the true residual, not entry by entry.

Shapes: 511^2 (four column strips in double, two in float, 64 row chunks: several workgroups and a one-workgroup
reduction over more partials than threads) for the parity cases; 63^2 and 127^2 for the line cycles.

Deep bases (DEEP): GCR(8), nine iterations from a zero guess with tol 0, so both sides run slots 0 .. 7 and a wrap and no
tolerance decides the count; in float at 511^2 on the three hierarchies, in both types at 1023^2 (another strip count, a
masked tail strip) and at 31^2 (one strip, a handful of workgroups: fewer partials than reduction threads).  Every
reference is asserted first to end at or above 1e-4 of its first entry, well above the float floor: measured on the CPU,
POISSON V(1,0) ends at 1.7e-4 (9..5 and 10..6), STENCIL5 contrast 10 V(1,1) at 1.2e-3, GALERKIN V(1,0) with omega = 0.3 at
2.6e-4, POISSON 5..3 V(1,0) with bottom = SMOOTH at 5.1e-3 (DEEP says what the stronger variants reach).
The float iterate is held to X_TOL32 = 1e-4 of the reference's largest entry.  Measured on the CPU, gcr_ref against itself
with every scalar moved independently by up to one float ulp (a factor 1 + 1.2e-7 u, u uniform in (-1, 1); the largest
of three seeds): the iterate moves by 4.6e-6 (POISSON 9..5), 3.4e-6 (STENCIL5), 2.5e-7 (GALERKIN), 5.5e-6 (POISSON 10..6),
3.1e-7 (POISSON 5..3) of its largest entry, the history by at most 3.0e-5 relative (RTOL32 is 33 times that).  1e-4 is 18
times the largest of these figures and 21 times or more the others; it is not raised to make that 20, because it is also
bounded from above: gcr_ref with the update of z' by the last basis vector left out in slots 5 .. 7 moves the iterate
by 8.3e-4 (POISSON 10..6) .. 1.2e-1 (5..3) and the history not at all, so the iterate bound is what catches a skipped
basis vector, with a factor 8 to spare.  In double the bound is this file's 1e-9."""
import ctypes as C
import functools

import numpy as np
import pytest

import galerkin_ref as gr
import gcr_ref
import line_ref as lr
import pcg_ref
import wcycle_ref as wr
from test_galerkin_cpu import random_stencil5
from test_gpu_pcg import RTOL32, RTOL64, assert_hist

pytestmark = pytest.mark.gpu

L9 = 9
BASE = dict(finest_level=9, coarsest_level=5, mu0=0, schedule=0)
CONFIGS = {
    "poisson_V11": dict(BASE, mu1=1, mu2=1),
    "stencil5_V22": dict(BASE, mu1=2, mu2=2, op=1),
    "galerkin_V22": dict(BASE, mu1=2, mu2=2, op=3),
}


def rhs(L, dt=np.float64):
    n = (1 << L) - 1
    return np.random.default_rng(3).uniform(-1, 1, (n, n)).astype(dt)


@functools.lru_cache(maxsize=None)
def operator_of(name):
    """what the configuration's finest operator is made from: nothing, nodal coefficients, five coefficient grids"""
    if name.startswith("stencil5"):
        return pcg_ref.contrast_coefficient(L9, 10.0)
    if name.startswith("galerkin"):
        return random_stencil5(L9, 100 + L9)            # the seeded non-symmetric operator of tests/test_galerkin_cpu.py
    return None


def setup(mg, name):
    op = operator_of(name)
    if name.startswith("stencil5"):
        mg.set_coefficient(op)
    elif name.startswith("galerkin"):
        mg.set_stencil(L9, *op)
        mg.build_galerkin()


@functools.lru_cache(maxsize=None)
def reference(name, restart, tol, cap=40, seed=None):
    """(x, history, converged, breakdown) of gcr_ref on the configuration, from a zero guess (seed None) or a seeded one"""
    from oracle import pyoracle as po
    dt = np.float64
    cfg = CONFIGS[name]
    op = operator_of(name)
    b = rhs(L9, dt)
    zeros = np.zeros_like(b)
    x0 = zeros if seed is None else po.fill_uniform(b.shape, seed).astype(dt)
    if name.startswith("galerkin"):
        M = gcr_ref.cycle_preconditioner(gr.Hierarchy(po, op, L9, 5, dt, mu1=cfg["mu1"], mu2=cfg["mu2"]))
        return gcr_ref.gcr(pcg_ref.Operator(op, dt), M, b, x0, tol, cap, restart)
    s = pcg_ref.oracle_solver(po, cfg, op)
    try:
        coef = None if op is None else po.stencil_from_nodes(op, L9, L9)
        return gcr_ref.gcr(pcg_ref.Operator(coef, dt), lambda r: s.vcycle(L9, zeros, r), b, x0, tol, cap, restart)
    finally:
        s.close()


# ---- history parity where the device cycle is the reference's ------------------------------------------------------------
@pytest.mark.parametrize("restart,tol", [(3, 1e-8), (8, 1e-11)])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_fp64_histories_match_the_reference(pkg, po, name, restart, tol):
    """restart 8 to 1e-11: the reference takes 14 / 30 / 9 iterations, so k_gcr_dots<1..7> and k_gcr_orth<0..7> all run"""
    x_ref, h_ref, conv_ref, brk_ref = reference(name, restart, tol)
    assert conv_ref and not brk_ref
    if restart == 8:
        assert len(h_ref) - 1 >= 9, "the reference does not reach the last basis slot"
    b = rhs(L9)
    with pkg.Multigrid(**CONFIGS[name]) as mg:
        setup(mg, name)
        mg.set_rhs(b)
        b0 = mg.get_level(L9, pkg.VEC_B)
        st, h = mg.solve_gcr(tol=tol, max_iters=40, restart=restart)
        u = mg.get_solution()
        b1 = mg.get_level(L9, pkg.VEC_B)
        assert mg.graphs_cached() >= 1
    k = min(len(h), len(h_ref))
    print(f"{name} GCR({restart}): {len(h) - 1} iterations (reference {len(h_ref) - 1}), largest entry difference "
          f"{float(np.max(np.abs(h[:k] - h_ref[:k]) / (RTOL64 * h_ref[:k] + 1e-14 * h_ref[0]))):.3e} of the bound")
    assert st.converged == 1 and st.cycles == len(h_ref) - 1 and st.history_len == len(h_ref)
    assert_hist(h, h_ref, RTOL64)
    assert np.all(h[1:] <= h[:-1] * (1 + 1e-12)), h
    assert np.max(np.abs(u - x_ref)) <= 1e-9 * np.max(np.abs(x_ref))
    assert np.array_equal(b0, b1)                       # B is the caller's b again, bit for bit
    assert st.initial_residual == h[0] and st.final_residual == h[-1]


def test_fp32_history_matches_the_reference(pkg, po):
    """POISSON 9..5 V(2,1), to 1e-5, restart 4"""
    _, h_ref, conv_ref, _ = reference_fp32()
    cfg = dict(BASE, mu1=2, mu2=1, dtype=0)
    b = rhs(L9, np.float32)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        b0 = mg.get_level(L9, pkg.VEC_B)
        st, h = mg.solve_gcr(tol=1e-5, max_iters=40, restart=4)
        u = mg.get_solution()
        b1 = mg.get_level(L9, pkg.VEC_B)
    print(f"fp32 GCR(4): {len(h) - 1} iterations (reference {len(h_ref) - 1})")
    assert conv_ref and st.converged == 1
    assert abs(len(h) - len(h_ref)) <= 1, (h, h_ref)
    m = min(len(h), len(h_ref))
    assert np.all(np.abs(h[:m] - h_ref[:m]) <= RTOL32 * h_ref[:m]), (h, h_ref)
    assert np.isfinite(u).all() and np.array_equal(b0, b1)


@functools.lru_cache(maxsize=None)
def reference_fp32():
    from oracle import pyoracle as po
    cfg = dict(BASE, mu1=2, mu2=1, dtype=0)
    b = rhs(L9, np.float32)
    zeros = np.zeros_like(b)
    s = pcg_ref.oracle_solver(po, cfg)
    try:
        return gcr_ref.gcr(pcg_ref.Operator(None, np.float32), lambda r: s.vcycle(L9, zeros, r), b, zeros, 1e-5, 40, 4)
    finally:
        s.close()


# ---- deep bases in float, other strip counts, fewer partials than reduction threads ------------------------------------
F32, F64 = np.float32, np.float64
DEEP = {
    # name: (type, operator, finest, coarsest, mu1, mu2): restart 8, nine iterations from a zero guess, tol 0 - slots 0 .. 7
    # and a wrap, so k_gcr_dots<T, 1..7>, k_gcr_orth<T, 0..7> and k_pcg_direction<T, 0 / 1> (first pass) all run with
    # the scalars of a real iteration, and the count does not hang on a tolerance.  Weak smoothing keeps the ninth
    # entry far above the float rounding floor of the first
    "f32_poisson_9_5": (F32, "poisson", 9, 5, 1, 0, {}),
    "f32_stencil5_9_5": (F32, "stencil5", 9, 5, 1, 1, {}),
    # (V(1,1) with omega = 2/3 ends at 1.9e-8 of the first entry, at the float floor, V(1,0) at 1.9e-5; omega = 0.3: 2.6e-4)
    "f32_galerkin_9_5": (F32, "galerkin", 9, 5, 1, 0, dict(omega=0.3)),
    # 1023^2: another strip count than 511^2 and a masked tail strip (columns >= N)
    "f32_poisson_10_6": (F32, "poisson", 10, 6, 1, 0, {}),
    "f64_poisson_10_6": (F64, "poisson", 10, 6, 1, 0, {}),
    # 31^2: one strip, a handful of workgroups - pcg_reduce_sum with far fewer partials than threads.  (With the exact
    # bottom solve on these three levels the ninth entry is 9.1e-5 of the first; bottom = SMOOTH: 5.1e-3)
    "f64_poisson_5_3": (F64, "poisson", 5, 3, 1, 0, dict(bottom=1)),
    "f32_poisson_5_3": (F32, "poisson", 5, 3, 1, 0, dict(bottom=1)),
}
DEEP_ITERS, DEEP_RESTART = 9, 8
X_TOL64 = 1e-9                                  # the iterate in double: this file's bound
X_TOL32 = 1e-4                                  # ... in float: module docstring


def deep_cfg(name):
    dt, kind, L, Lc, mu1, mu2, extra = DEEP[name]
    return dict(finest_level=L, coarsest_level=Lc, mu0=0, mu1=mu1, mu2=mu2, schedule=0, dtype=1 if dt is F64 else 0,
                op={"poisson": 0, "stencil5": 1, "galerkin": 3}[kind], **extra)


def deep_operator(name):
    dt, kind, L = DEEP[name][:3]
    assert kind == "poisson" or L == L9
    return operator_of(kind)


@functools.lru_cache(maxsize=None)
def deep_reference(name, dot=pcg_ref.dot):
    """(x, history, converged, breakdown) of gcr_ref.gcr: GCR(8), nine iterations, zero guess, the reference's cycle as M"""
    from oracle import pyoracle as po
    dt, kind, L, Lc, mu1, mu2, extra = DEEP[name]
    cfg, op = deep_cfg(name), deep_operator(name)
    b = rhs(L, dt)
    zeros = np.zeros_like(b)
    if kind == "galerkin":
        M = gcr_ref.cycle_preconditioner(gr.Hierarchy(po, op, L, Lc, dt, mu1=mu1, mu2=mu2, **extra))
        return gcr_ref.gcr(pcg_ref.Operator(op, dt), M, b, zeros, 0.0, DEEP_ITERS, DEEP_RESTART, dot=dot)
    s = pcg_ref.oracle_solver(po, cfg, op)
    try:
        coef = None if op is None else po.stencil_from_nodes(op, L, L)
        return gcr_ref.gcr(pcg_ref.Operator(coef, dt), lambda r: s.vcycle(L, zeros, r), b, zeros, 0.0, DEEP_ITERS, DEEP_RESTART, dot=dot)
    finally:
        s.close()


@pytest.mark.parametrize("name", list(DEEP))
def test_deep_bases_match_the_reference_entry_by_entry(pkg, po, name):
    dt, kind, L, Lc = DEEP[name][:4]
    x_ref, h_ref, conv_ref, brk_ref = deep_reference(name)
    assert not brk_ref and not conv_ref and len(h_ref) == DEEP_ITERS + 1
    assert h_ref[-1] >= 1e-4 * h_ref[0], h_ref          # well above the float floor: the comparison means something
    b = rhs(L, dt)
    with pkg.Multigrid(**deep_cfg(name)) as mg:
        op = deep_operator(name)
        if kind == "stencil5":
            mg.set_coefficient(op)
        elif kind == "galerkin":
            mg.set_stencil(L, *op)
            mg.build_galerkin()
        mg.set_rhs(b)
        b0 = mg.get_level(L, pkg.VEC_B)
        st, h = mg.solve_gcr(tol=0.0, max_iters=DEEP_ITERS, restart=DEEP_RESTART)
        u = mg.get_solution()
        b1 = mg.get_level(L, pkg.VEC_B)
    rtol, xtol = (RTOL64, X_TOL64) if dt is F64 else (RTOL32, X_TOL32)
    dx = float(np.max(np.abs(u.astype(F64) - x_ref.astype(F64))) / np.max(np.abs(x_ref)))
    k = min(len(h), len(h_ref))
    dh = float(np.max(np.abs(h[:k] - h_ref[:k]) / h_ref[:k]))
    print(f"\n[gcr-deep] {name}: {st.cycles} iterations, last / first {h[-1] / h[0]:.3g} (reference {h_ref[-1] / h_ref[0]:.3g}); largest history "
          f"deviation {dh:.3g} ({dh / rtol:.3g} x {rtol:g}); iterate off by {dx:.3g} of the largest entry ({dx / xtol:.3g} x {xtol:g})")
    assert st.cycles == DEEP_ITERS and st.converged == 0 and st.history_len == DEEP_ITERS + 1
    assert u.dtype == dt
    if dt is F64:
        assert_hist(h, h_ref, RTOL64)
    else:
        assert len(h) == len(h_ref) and np.all(np.abs(h - h_ref) <= RTOL32 * h_ref), (h, h_ref)
    assert np.array_equal(b0, b1) and np.array_equal(b0, b)          # B is the caller's b again, bit for bit
    assert np.all(h[1:] <= h[:-1] * (1 + 1e-12)), h
    assert dx <= xtol, (dx, xtol)


# ---- the breakdown exit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [None, 7])
@pytest.mark.parametrize("dtype", [1, 0])
def test_breakdown_exit_and_the_calls_after_it(pkg, po, dtype, seed):
    """POISSON 7..4 with mu1 = mu2 = 0 and bottom = SMOOTH: the zero-start cycle returns exactly zero (and runs with no
    smoothing pass to synthesise its zero guess), so z = 0, q' = A z = 0 and q'.q' = 0 at iteration 1 - arithmetic on finite
    data.  gcr_ref around the oracle's cycle reports a breakdown, a history of one entry and an untouched x.  The device:
    k_gcr_reduce raises the flag, k_pcg_update skips, the driver returns MGX_OK with the reason, U and B are restored.
    Then solve_pcg on the same handle breaks down too (p = 0: p.Ap = 0), and a smoothing block and a norm afterwards are
    those of a fresh handle.
    (A breakdown at a later basis slot needs q' = 0 after a successful iteration, an input no natural problem provides:
    out of scope here.)"""
    L = 7
    cfg = dict(finest_level=L, coarsest_level=4, mu0=0, mu1=0, mu2=0, bottom=1, schedule=0, dtype=dtype)
    dt = F64 if dtype == 1 else F32
    tol = 1e-8 if dtype == 1 else 1e-5
    rtol = RTOL64 if dtype == 1 else RTOL32
    b = rhs(L, dt)
    u0 = np.zeros_like(b) if seed is None else po.fill_uniform(b.shape, seed).astype(dt)
    zeros = np.zeros_like(b)
    s = pcg_ref.oracle_solver(po, cfg)
    try:
        A = pcg_ref.Operator(None, dt)
        x_ref, h_ref, conv_ref, brk_ref = gcr_ref.gcr(A, lambda r: s.vcycle(L, zeros, r), b, u0, tol, 30, 4)
        xp_ref, hp_ref, convp_ref, brkp_ref = pcg_ref.pcg(A, lambda r: s.vcycle(L, zeros, r), b, u0, tol, 30)
    finally:
        s.close()
    assert brk_ref and not conv_ref and len(h_ref) == 1 and np.array_equal(x_ref, u0)
    assert brkp_ref and not convp_ref and len(hp_ref) == 1 and np.array_equal(xp_ref, u0)

    def state(mg):
        return mg.get_solution(), mg.get_level(L, pkg.VEC_B)

    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.set_guess(u0)
        u_before, b_before = state(mg)
        assert np.array_equal(u_before, u0) and np.array_equal(b_before, b)
        seen = []
        for _ in range(2):                               # the second call: from the flag and the scalars the first one left
            st, h = mg.solve_gcr(tol=tol, max_iters=30, restart=4)          # MGX_OK: anything else raises
            msg = pkg.lib().mgx_last_error(mg._h).decode()
            print(f"dtype {dtype} seed {seed}: history {h} (reference {h_ref}), '{msg}'")
            assert st.converged == 0 and st.cycles == 0 and st.history_len == 1 and len(h) == 1
            assert_hist(h, h_ref, rtol)
            assert "GCR breakdown at iteration 1" in msg and "q'.q'" in msg
            u1, b1 = state(mg)
            assert np.array_equal(u1, u_before), "U is not the guess"
            assert np.array_equal(b1, b_before), "B is not the caller's b"
            seen.append((h, msg))
        assert np.array_equal(seen[0][0], seen[1][0]) and seen[0][1] == seen[1][1]
        st, h = mg.solve_pcg(tol=tol, max_iters=30)
        msg = pkg.lib().mgx_last_error(mg._h).decode()
        assert st.converged == 0 and st.cycles == 0 and st.history_len == 1
        assert_hist(h, hp_ref, rtol)
        assert np.array_equal(h, seen[0][0])             # the same norm kernel on the same data
        assert "PCG breakdown at iteration 1" in msg and "p.Ap" in msg
        u1, b1 = state(mg)
        assert np.array_equal(u1, u_before) and np.array_equal(b1, b_before)
        mg.smooth(L, 2)
        after = state(mg) + (mg.residual_norm(),)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.set_guess(u0)
        mg.smooth(L, 2)
        fresh = state(mg) + (mg.residual_norm(),)
    assert np.array_equal(after[0], fresh[0]) and np.array_equal(after[1], fresh[1]) and after[2] == fresh[2]
    assert not np.array_equal(after[0], u0)


# ---- line cycles -------------------------------------------------------------------------------------------------------
def line_handle(pkg, L, st5, **kw):
    cfg = dict(finest_level=L, coarsest_level=3, op=pkg.OP_GALERKIN, smoother=lr.LINE_ALT, mu1=1, mu2=1, schedule=0)
    cfg.update(kw)
    mg = pkg.Multigrid(**cfg)
    mg.set_stencil(L, *st5)
    mg.build_galerkin()
    return mg


@functools.lru_cache(maxsize=None)
def line_reference(kind):
    """(st5, b, A, M, hierarchy) of LINE_ALT V(1,1), GALERKIN, coarsest level 3: 'layers' at 63^2, 'peclet1' at 127^2"""
    from oracle import pyoracle as po
    L, st5 = (6, lr.aniso_stencil(6, 1e-2, "layers")) if kind == "layers" else (7, gcr_ref.upwind_stencil(7, (1.0, 0.5), 1.0))
    h = lr.Hierarchy(lr.LINE_ALT, po, st5, L, 3, np.float64, mu1=1, mu2=1)
    return L, st5, rhs(L), pcg_ref.Operator(st5, np.float64), gcr_ref.cycle_preconditioner(h), h


def test_the_layers_problem_with_the_alternating_line_cycle(pkg, po):
    tol = 1e-8
    L, st5, b, A, M, _ = line_reference("layers")
    _, h_ref, conv_ref, _ = gcr_ref.gcr(A, M, b, np.zeros_like(b), tol, 60, 4)
    assert conv_ref
    with line_handle(pkg, L, st5) as mg:
        mg.set_rhs(b)
        sv, hv = mg.solve(tol=tol, max_cycles=60)
        mg.set_guess(np.zeros_like(b))
        st, h = mg.solve_gcr(tol=tol, max_iters=60, restart=4)
        rn = mg.residual_norm()
    print(f"layers 63^2: mgx_solve {sv.cycles} cycles, mgx_solve_gcr(4) {st.cycles} iterations (reference {len(h_ref) - 1})")
    assert sv.converged == 1 and st.converged == 1
    assert abs(st.cycles - (len(h_ref) - 1)) <= 1 and st.cycles <= sv.cycles
    assert np.all(h[1:] <= h[:-1] * (1 + 1e-12)), h
    assert rn <= 2 * tol * h[0], (rn, h)
    n = (1 << L) - 1
    assert st.fine_updates == st.cycles * 2 * 2 * n * n          # an alternating sweep is two sweeps; V(1,1)


def test_upwind_convection_converges_with_gcr_and_not_with_pcg(pkg, po):
    tol = 1e-8
    L, st5, b, A, M, _ = line_reference("peclet1")
    zeros = np.zeros_like(b)
    _, h_ref, conv_ref, _ = gcr_ref.gcr(A, M, b, zeros, tol, 60, 4)
    _, hp_ref, conv_p, brk_p = pcg_ref.pcg(A, M, b, zeros, tol, 60)
    assert conv_ref and (not conv_p or brk_p)
    with line_handle(pkg, L, st5) as mg:
        mg.set_rhs(b)
        st, h = mg.solve_gcr(tol=tol, max_iters=60, restart=4)
        rn = mg.residual_norm()
    with line_handle(pkg, L, st5) as mg:
        mg.set_rhs(b)
        sp, hp = mg.solve_pcg(tol=tol, max_iters=60)
    print(f"Peclet 1, 127^2: GCR(4) {st.cycles} iterations (reference {len(h_ref) - 1}); PCG {sp.cycles} iterations, converged {sp.converged}, "
          f"last / first {hp[-1] / hp[0]:.2e}")
    assert st.converged == 1 and abs(st.cycles - (len(h_ref) - 1)) <= 1
    assert np.all(h[1:] <= h[:-1] * (1 + 1e-12)) and rn <= 2 * tol * h[0]
    assert sp.converged == 0


def test_w_cycle_on_a_galerkin_handle(pkg, po):
    L, Lc = 6, 3
    st5 = random_stencil5(L, 100 + L)
    b = rhs(L)
    ref = wr.with_cycle(wr.Galerkin, wr.W, po, st5, L, Lc, np.float64, mu1=2, mu2=2)
    x_ref, h_ref, conv, brk = gcr_ref.gcr(pcg_ref.Operator(st5, np.float64), gcr_ref.cycle_preconditioner(ref), b, np.zeros_like(b), 1e-10, 40, 4)
    assert conv and not brk
    with pkg.Multigrid(finest_level=L, coarsest_level=Lc, op=pkg.OP_GALERKIN, mu0=0, mu1=2, mu2=2, schedule=0) as mg:
        mg.set_stencil(L, *st5)
        mg.build_galerkin()
        mg.set_cycle(wr.W)
        mg.set_rhs(b)
        st, h = mg.solve_gcr(tol=1e-10, max_iters=40, restart=4)
        u = mg.get_solution()
    assert st.converged == 1
    assert_hist(h, h_ref, RTOL64)
    assert np.max(np.abs(u - x_ref)) <= 1e-9 * np.max(np.abs(x_ref))


# ---- state and determinism ---------------------------------------------------------------------------------------------
def test_nonzero_start_state_after_the_call(pkg, po):
    name = "stencil5_V22"
    x_ref, h_ref, _, _ = reference(name, 4, 1e-8, seed=4242)
    b = rhs(L9)
    u0 = po.fill_uniform(b.shape, 4242)
    with pkg.Multigrid(**CONFIGS[name]) as mg:
        setup(mg, name)
        mg.set_rhs(b)
        mg.set_guess(u0)
        b0 = mg.get_level(L9, pkg.VEC_B)
        st, h = mg.solve_gcr(tol=1e-8, max_iters=40, restart=4)
        u = mg.get_solution()
        assert np.array_equal(mg.get_level(L9, pkg.VEC_B), b0)
        rn = mg.residual_norm()
    assert_hist(h, h_ref, RTOL64)
    assert np.max(np.abs(u - x_ref)) <= 1e-9 * np.max(np.abs(x_ref))
    want = pcg_ref.true_residual(b, u, operator_of(name), L9, po)
    assert abs(rn - want) <= 1e-10 * want + 1e-13 * h[0], (rn, want)
    assert rn <= 2 * 1e-8 * h[0]


@pytest.mark.parametrize("name", ["poisson_V11", "galerkin_V22"])
def test_repeated_calls_and_eager_launches_give_the_same_bits(pkg, po, monkeypatch, name):
    b = rhs(L9)
    u0 = po.fill_uniform(b.shape, 31)

    def runs(**kw):
        out = []
        with pkg.Multigrid(**dict(CONFIGS[name], **kw)) as mg:
            setup(mg, name)
            mg.set_rhs(b)
            for _ in range(2):                           # two calls from the same state on one handle
                mg.set_guess(u0)
                st, h = mg.solve_gcr(tol=1e-9, max_iters=12, restart=3)
                out.append((h, mg.get_solution()))
            return out, mg.graphs_cached()

    replay, cached = runs()
    assert cached >= 1 and len(replay[0][0]) > 5
    profiled, _ = runs(profile=1)
    monkeypatch.setenv("MGX_GRAPH", "0")
    eager, cached = runs()
    assert cached <= 0
    for h, u in replay[1:] + profiled + eager:
        assert np.array_equal(h, replay[0][0]) and np.array_equal(u, replay[0][1])


def test_interleaved_entry_points_on_one_handle_equal_fresh_handles(pkg, po):
    """solve_gcr -> solve -> solve_pcg -> solve_gcr(restart 8): the buffers shared with PCG and the basis growing from 2 to 8
    pairs; and callers that never call GCR cache the same graphs as before"""
    cfg = CONFIGS["poisson_V11"]
    b = rhs(L9)
    u0 = po.fill_uniform(b.shape, 99)
    steps = [("gcr", dict(tol=1e-3, max_iters=5, restart=2)), ("solve", dict(tol=1e-5, max_cycles=3)),
             ("pcg", dict(tol=1e-8, max_iters=4)), ("gcr", dict(tol=1e-12, max_iters=10, restart=8))]

    def step(mg, what, kw):
        return {"gcr": mg.solve_gcr, "solve": mg.solve, "pcg": mg.solve_pcg}[what](**kw)[1]

    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.set_guess(u0)
        one = [step(mg, what, kw) for what, kw in steps]
        u_one = mg.get_solution()
        graphs = mg.graphs_cached()
    u = u0
    fresh = []
    for what, kw in steps:
        with pkg.Multigrid(**cfg) as mg:
            mg.set_rhs(b)
            mg.set_guess(u)
            fresh.append(step(mg, what, kw))
            u = mg.get_solution()
    assert len(one[3]) == 11                             # ten iterations: every slot of the grown basis
    for a, c in zip(one, fresh):
        assert np.array_equal(a, c), (a, c)
    assert np.array_equal(u_one, u)
    with pkg.Multigrid(**cfg) as mg:                     # solve -> solve_pcg alone: the same cached graphs
        mg.set_rhs(b)
        mg.set_guess(u0)
        mg.solve(**steps[1][1])
        mg.solve_pcg(**steps[2][1])
        assert mg.graphs_cached() == graphs


def test_pcg_first_then_gcr_and_timed_passes_on_one_handle_equal_fresh_handles(pkg, po):
    """solve_pcg -> solve_gcr(3) -> time_gcr_pass (dots, orth, update) -> solve_pcg -> solve_gcr(2): GCR on the buffers PCG
    allocated, and PCG on the scalar block mgx_time_gcr_pass has just zeroed"""
    cfg = CONFIGS["poisson_V11"]
    b = rhs(L9)
    u0 = po.fill_uniform(b.shape, 99)
    steps = [("pcg", dict(tol=1e-8, max_iters=4)), ("gcr", dict(tol=1e-3, max_iters=5, restart=3)), ("time", None),
             ("pcg", dict(tol=1e-10, max_iters=4)), ("gcr", dict(tol=1e-12, max_iters=6, restart=2))]

    def step(mg, what, kw):
        return (mg.solve_gcr if what == "gcr" else mg.solve_pcg)(**kw)[1]

    one = []
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.set_guess(u0)
        for what, kw in steps:
            if what == "time":
                for which, j in ((1, 1), (1, 2), (2, 0), (2, 2), (0, 2)):
                    assert mg.time_gcr_pass(which, j, 2) > 0.0
            else:
                one.append(step(mg, what, kw))
        u_one = mg.get_solution()
    u = u0
    fresh = []
    for what, kw in steps:
        if what == "time":
            continue
        with pkg.Multigrid(**cfg) as mg:
            mg.set_rhs(b)
            mg.set_guess(u)
            fresh.append(step(mg, what, kw))
            u = mg.get_solution()
    for a, c in zip(one, fresh):
        assert np.array_equal(a, c), (a, c)
    assert np.array_equal(u_one, u)


def test_zero_rhs_and_zero_iterations(pkg, po):
    cfg = CONFIGS["poisson_V11"]
    n = (1 << L9) - 1
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(np.zeros((n, n)))
        mg.set_guess(np.zeros((n, n)))
        st, h = mg.solve_gcr(tol=1e-8, max_iters=20, restart=4)
        u = mg.get_solution()
    assert st.converged == 1 and st.cycles == 0 and len(h) == 1 and h[0] == 0.0
    assert np.isfinite(u).all() and not u.any()
    b = rhs(L9)
    u0 = po.fill_uniform(b.shape, 5)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        mg.set_guess(u0)
        b0 = mg.get_level(L9, pkg.VEC_B)
        st, h = mg.solve_gcr(tol=1e-8, max_iters=0, restart=4)
        assert np.array_equal(mg.get_solution(), u0) and np.array_equal(mg.get_level(L9, pkg.VEC_B), b0)
    assert len(h) == 1 and st.cycles == 0 and st.converged == 0 and st.history_len == 1
    assert abs(h[0] - pcg_ref.true_residual(b, u0)) <= 1e-12 * h[0]


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(pkg, po):
    lib = pkg.lib()
    st = pkg.binding.Stats()
    hist = np.zeros(8)
    hp = hist.ctypes.data_as(C.POINTER(C.c_double))
    INVALID, STATE = 1, 5
    b = po.rhs_sine(7)
    small = dict(finest_level=7, coarsest_level=4, mu0=0, mu1=2, mu2=1, schedule=0)
    assert lib.mgx_solve_gcr(None, 1e-8, 3, 4, C.byref(st), hp, 8) == INVALID
    with pkg.Multigrid(**dict(small, dtype=pkg.DTYPE_MIXED)) as mg:
        mg.set_rhs(b)
        assert lib.mgx_solve_gcr(mg._h, 1e-8, 3, 4, C.byref(st), hp, 8) == STATE
        assert "MIXED" in lib.mgx_last_error(mg._h).decode()
        s, h = mg.solve(tol=1e-8, max_cycles=20)
        assert s.converged == 1
    with pkg.Multigrid(**dict(small, n_gpus=2, devices=[0, 0], cut_level=5)) as mg:
        mg.set_rhs(b)
        assert lib.mgx_solve_gcr(mg._h, 1e-8, 3, 4, C.byref(st), hp, 8) == STATE
        s, h = mg.solve(tol=1e-8, max_cycles=20)
        assert s.converged == 1
    with pkg.Multigrid(**dict(small, op=pkg.OPERATOR_STENCIL5)) as mg:
        mg.set_rhs(b)
        assert lib.mgx_solve_gcr(mg._h, 1e-8, 3, 4, C.byref(st), hp, 8) == STATE          # no stencil set yet
        with pytest.raises(pkg.MgxError):
            mg.solve_gcr()
        mg.set_coefficient(np.ones((129, 129)))
        s, h = mg.solve_gcr(tol=1e-8, max_iters=30, restart=2)
        assert s.converged == 1
    with pkg.Multigrid(**small) as mg:
        mg.set_rhs(b)
        for tol, iters, restart in ((-1.0, 3, 4), (float("nan"), 3, 4), (1e-8, -1, 4), (1e-8, 3, 0), (1e-8, 3, -2),
                                    (1e-8, 3, pkg.GCR_MAX_RESTART + 1)):
            assert lib.mgx_solve_gcr(mg._h, tol, iters, restart, C.byref(st), hp, 8) == INVALID, (tol, iters, restart)
            assert "mgx_solve_gcr" in lib.mgx_last_error(mg._h).decode()
        with pytest.raises(pkg.MgxError, match="restart"):
            mg.solve_gcr(restart=9)
        s, h = mg.solve_gcr(tol=1e-8, max_iters=30, restart=pkg.GCR_MAX_RESTART)
        assert s.converged == 1
        s, h = mg.solve_gcr(tol=1e-8, max_iters=30, restart=1)
        assert s.converged == 1


def test_time_gcr_pass_changes_nothing_and_refuses_what_it_cannot_time(pkg, po):
    """mgx_time_gcr_pass (tools/gcr_bench.py): needs the basis of an earlier solve_gcr; U, B and the next solve keep their bits"""
    cfg = CONFIGS["poisson_V11"]
    b = rhs(L9)
    with pkg.Multigrid(**cfg) as mg:
        mg.set_rhs(b)
        with pytest.raises(pkg.MgxError, match="invalid state.*mgx_solve_gcr"):
            mg.time_gcr_pass(0, 0, 2)
        st, h = mg.solve_gcr(tol=1e-6, max_iters=20, restart=3)
        u, b0 = mg.get_solution(), mg.get_level(L9, pkg.VEC_B)
        for which, j in ((0, 0), (1, 1), (1, 2), (2, 0), (2, 2), (3, 1)):
            assert mg.time_gcr_pass(which, j, 2) > 0.0
        assert np.array_equal(mg.get_solution(), u) and np.array_equal(mg.get_level(L9, pkg.VEC_B), b0)
        with pytest.raises(pkg.MgxError, match="invalid state"):
            mg.time_gcr_pass(2, 3, 2)                    # slot 3 was never allocated
        for which, j, reps in ((1, 0, 2), (4, 0, 2), (-1, 0, 2), (2, 8, 2), (2, -1, 2), (0, 0, 0)):
            with pytest.raises(pkg.MgxError, match="invalid argument"):
                mg.time_gcr_pass(which, j, reps)
        mg.set_guess(np.zeros_like(b))
        st2, h2 = mg.solve_gcr(tol=1e-6, max_iters=20, restart=3)
        assert np.array_equal(h2, h) and np.array_equal(mg.get_solution(), u)
