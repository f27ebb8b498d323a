"""GPU parity of the cycle index (mgx_set_cycle: W- and F-cycles on STENCIL5 and GALERKIN handles) against the numpy
statement of tests/wcycle_ref.py, with the tolerances of tests/test_gpu_galerkin.py and tests/test_gpu_opdep.py: in
double hist_close on residual histories and 1e-10 of max |u| on iterates (the dense coarsest solve is the only step
that is not bit for bit); in float 1e-6 relative on residual norms.

The shapes are the smallest at which the recursion can go wrong:
    levels 7..3   four levels above the coarsest: level 6 is visited twice, 5 four times, 4 eight times by a W-cycle;
                  a 15^2 and a 7^2 level
    levels 8..5   the second visit exists on levels 7 and 6 only; level 6 is coarsest + 1 (its visits never repeat the
                  coarsest level's)
    levels 6..4   one level between the five-point finest level and the coarsest
    levels 5..3   float only, mu1 != mu2
and they are the shapes of the one-workgroup visit kernel (csrc/mgx_small.hpp: nine-point levels with N <= 64, Jacobi):
7..3 runs it on levels 6, 5 and 4 with turns on each and a 15^2 level with more lanes than points; 8..5 runs level 7
through the per-level launches and level 6, the only fused one, next to the coarsest; in 6..4 the finest level is
five-point with N = 64 and must not take the kernel, level 5 does.  Every configuration is run a second time on a handle
created with MGX_SMALL_VISIT=0 (the per-level launches only): the bits of U and of the history must be the same."""
import functools

import numpy as np
import pytest

import galerkin_ref as gr
import opdep_ref as od
import pcg_ref
import wcycle_ref as wr
from test_galerkin_cpu import coefficient
from test_gpu_galerkin import assert_same, handle, np_dtype
from test_gpu_pcg import RTOL64, assert_hist
from test_gpu_solve import hist_close

pytestmark = pytest.mark.gpu

V, W, F = wr.V, wr.W, wr.F
BILINEAR, OPERATOR = od.BILINEAR, od.OPERATOR
REF = {BILINEAR: wr.Galerkin, OPERATOR: wr.Opdep}
MUS = ((1, 1), (2, 2), (2, 1), (0, 2))
PROF_COARSE = 4                         # MGX_PROF_COARSE (include/mgx.h): everything below the finest level


@functools.lru_cache(maxsize=None)
def nodes(L):
    return pcg_ref.contrast_coefficient(L, 100.0)


_refs = {}


def reference(po, finest, coarsest, transfer, dtype, mode, cycle, mu1=2, mu2=2, **kw):
    """one hierarchy (and one dense inverse of its coarsest operator) per configuration, shared by every test of this
    module; mu1, mu2 and the cycle kind are attributes the hierarchy reads per call"""
    key = (finest, coarsest, transfer, dtype, mode, tuple(sorted(kw.items())))
    if key not in _refs:
        _refs[key] = REF[transfer](po, po.stencil_from_nodes(nodes(finest), finest, finest), finest, coarsest, np_dtype(dtype), mode, **kw)
    ref = _refs[key]
    ref.mu1, ref.mu2, ref.cycle = mu1, mu2, cycle
    return ref


def built(pkg, finest, coarsest, transfer, cycle, **kw):
    mg = handle(pkg, finest, coarsest, **kw)
    mg.set_coefficient(nodes(finest))
    mg.build_galerkin(transfer)
    mg.set_cycle(cycle)
    assert mg.cycle == cycle
    return mg


def assert_iterate(po, ref, L, u, u_ref, b, dtype, what):
    r, r_ref = po.norm2(ref.residual(L, u, b)), po.norm2(ref.residual(L, u_ref, b))
    du = np.max(np.abs(u - u_ref)) / np.max(np.abs(u_ref))
    print(f"{what}: max |u - u_ref| / max |u_ref| {du:.3e}, ||r|| {r:.6e}, reference {r_ref:.6e}")
    if dtype == 1:
        assert du <= 1e-10, (what, du)
        assert hist_close([r], [r_ref]), (what, r, r_ref)
    else:
        assert np.allclose(r, r_ref, rtol=1e-6, atol=0), (what, r, r_ref)


SHAPES = [(7, 3), (8, 5), (6, 4), (5, 3)]
CASES = [(f, c, transfer, dtype, mode) for f, c in SHAPES for transfer in (BILINEAR, OPERATOR) for dtype in (1, 0)
         for mode in (gr.CONSISTENT, gr.FW16) if (f, c) != (5, 3) or dtype == 0]


@pytest.mark.parametrize("finest,coarsest,transfer,dtype,mode", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_one_cycle_from_a_random_guess_matches_the_reference(pkg, po, monkeypatch, finest, coarsest, transfer, dtype, mode):
    dt = np_dtype(dtype)
    n = (1 << finest) - 1
    rng = np.random.default_rng(10 * finest + coarsest)
    u0, b = rng.uniform(-1, 1, (n, n)).astype(dt), rng.uniform(-1, 1, (n, n)).astype(dt)
    seen = {}
    for mu1, mu2 in MUS:
        for cycle in (W, F):
            ref = reference(po, finest, coarsest, transfer, dtype, mode, cycle, mu1, mu2)
            want = ref.vcycle(finest, u0, b)
            runs = {}
            for small in ("1", "0"):
                monkeypatch.setenv("MGX_SMALL_VISIT", small)
                with built(pkg, finest, coarsest, transfer, cycle, dtype=dtype, restrict_mode=mode, mu1=mu1, mu2=mu2) as mg:
                    mg.set_rhs(b)
                    mg.set_guess(u0)
                    mg.vcycle()
                    got = mg.get_solution()
                    mg.set_guess(u0)
                    st, h = mg.solve(tol=0.0, max_cycles=3)
                    runs[small] = (got, h, mg.get_solution())
            got = runs["1"][0]
            assert_iterate(po, ref, finest, got, want, b, dtype, (wr.NAMES[cycle], mu1, mu2))
            # the one-workgroup visits against the per-level launches: the same bits
            assert_same(runs["1"][0], runs["0"][0], ("U after one cycle", wr.NAMES[cycle], mu1, mu2))
            assert np.array_equal(runs["1"][1], runs["0"][1]), (wr.NAMES[cycle], mu1, mu2, runs["1"][1], runs["0"][1])
            assert_same(runs["1"][2], runs["0"][2], ("U after a solve of 3 cycles", wr.NAMES[cycle], mu1, mu2))
            seen[cycle, mu1, mu2] = got
        if finest - coarsest >= 3:
            # W and F are different cycles once a level has a level between itself and the coarsest
            assert not np.array_equal(seen[W, mu1, mu2], seen[F, mu1, mu2])


@pytest.mark.parametrize("finest,coarsest,transfer,dtype,mode", CASES, ids=["-".join(map(str, c)) for c in CASES])
@pytest.mark.parametrize("cycle", [W, F], ids=["W", "F"])
def test_solve_histories_match_the_reference(pkg, po, monkeypatch, cycle, finest, coarsest, transfer, dtype, mode):
    """constant right-hand side, zero guess, to 1e-8 in double; float cannot reach it: 10 cycles.  The same solve through
    the per-level launches only (MGX_SMALL_VISIT=0): the same history and iterate, bit for bit"""
    dt = np_dtype(dtype)
    mu1, mu2 = (2, 1) if (finest, coarsest) == (5, 3) else (2, 2)
    b = po.rhs_constant(finest).astype(dt)
    cycles = 40 if dtype == 1 else 10
    ref = reference(po, finest, coarsest, transfer, dtype, mode, cycle, mu1, mu2)
    u_ref, h_ref = ref.solve(b, tol=1e-8, max_cycles=cycles)
    with built(pkg, finest, coarsest, transfer, cycle, dtype=dtype, restrict_mode=mode, mu1=mu1, mu2=mu2) as mg:
        mg.set_rhs(b)
        st, h = mg.solve(tol=1e-8, max_cycles=cycles)
        u = mg.get_solution()
        assert mg.graphs_cached() >= 1
        n = (1 << finest) - 1
        assert st.fine_updates == st.cycles * (mu1 + mu2) * n * n
    monkeypatch.setenv("MGX_SMALL_VISIT", "0")
    with built(pkg, finest, coarsest, transfer, cycle, dtype=dtype, restrict_mode=mode, mu1=mu1, mu2=mu2) as mg:
        mg.set_rhs(b)
        st0, h0 = mg.solve(tol=1e-8, max_cycles=cycles)
        assert np.array_equal(h, h0), (h, h0)
        assert_same(u, mg.get_solution(), "U after the solve")
    m = min(len(h), len(h_ref))
    print(f"{wr.NAMES[cycle]} {finest}..{coarsest} transfer {transfer} dtype {dtype} mode {mode}: {len(h) - 1} cycles (reference {len(h_ref) - 1}), "
          f"max rel. history difference {np.max(np.abs(h[:m] - h_ref[:m]) / h_ref[:m]):.3e}")
    assert len(h) == len(h_ref)
    if dtype == 1:
        assert h_ref[-1] <= 1e-8 * h_ref[0], "the reference itself did not converge"
        assert hist_close(h, h_ref), (h, h_ref)
        assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))
    else:
        assert np.allclose(h, h_ref, rtol=1e-6, atol=0), (h, h_ref)


def coarse_launches(pkg, monkeypatch, small, finest, coarsest, cycle, **kw):
    """launches below the finest level in two eager cycles (cfg.profile = 1), and the iterate"""
    monkeypatch.setenv("MGX_SMALL_VISIT", small)
    with built(pkg, finest, coarsest, OPERATOR, cycle, profile=1, **kw) as mg:
        mg.fill_rhs(0)
        st, h = mg.solve(tol=0.0, max_cycles=2)
        return mg.profile()["launches"][PROF_COARSE], mg.get_solution()


def test_the_visit_kernel_is_engaged_where_the_scope_says(pkg, po, monkeypatch):
    """per W-cycle on 7..3 the per-level path pays 2 + 4 + 8 visits of levels 6, 5, 4 with mu1 + mu2 + 2 counted launches each
    (the sweeps, the restriction, the prolongation);
    the kernel pays 3 launches per pair of visits.  Not in V-cycles, not with the Chebyshev smoother, not on the five-point
    finest level of 6..4 (N = 64), and not with MGX_SMALL_VISIT=0"""
    on, u_on = coarse_launches(pkg, monkeypatch, "1", 7, 3, W)
    off, u_off = coarse_launches(pkg, monkeypatch, "0", 7, 3, W)
    print(f"launches below the finest level in two W-cycles on 7..3: {on} with the visit kernel, {off} without")
    assert np.array_equal(u_on, u_off)
    assert off - on == 2 * (14 * 6 - 7 * 3), (on, off)
    for cycle, kw in ((V, dict()), (W, dict(smoother=pkg.SMOOTHER_CHEBYSHEV))):
        a, ua = coarse_launches(pkg, monkeypatch, "1", 7, 3, cycle, **kw)
        c, uc = coarse_launches(pkg, monkeypatch, "0", 7, 3, cycle, **kw)
        assert a == c and np.array_equal(ua, uc), (cycle, kw, a, c)
    # 6..4: level 5 is the only level between the finest and the coarsest: 2 visits of 6 launches against 3 launches
    on, u_on = coarse_launches(pkg, monkeypatch, "1", 6, 4, W)
    off, u_off = coarse_launches(pkg, monkeypatch, "0", 6, 4, W)
    assert np.array_equal(u_on, u_off) and off - on == 2 * (2 * 6 - 3), (on, off)


@pytest.mark.parametrize("bottom", [gr.EXACT, gr.SMOOTH])
def test_bottom_smooth_is_one_visit_of_the_coarsest_level(pkg, po, bottom):
    finest, coarsest = 7, 3
    b = po.rhs_sine(finest)
    ref = reference(po, finest, coarsest, OPERATOR, 1, gr.CONSISTENT, W, bottom=bottom)
    u_ref, h_ref = ref.solve(b, tol=1e-8, max_cycles=6)
    with built(pkg, finest, coarsest, OPERATOR, W, bottom=bottom) as mg:
        mg.set_rhs(b)
        st, h = mg.solve(tol=1e-8, max_cycles=6)
    assert hist_close(h, h_ref), (h, h_ref)


def test_chebyshev_and_stencil5_handles_run_w_cycles(pkg, po):
    L, Lc = 7, 4
    a = coefficient(L, "smooth")
    b = po.rhs_sine(L)
    st5 = po.stencil_from_nodes(a, L, L)
    sts = {lv: po.stencil_from_nodes(a, lv, L) for lv in range(Lc, L + 1)}
    runs = [("chebyshev galerkin", wr.ChebyOpdep(po, st5, L, Lc), dict(smoother=pkg.SMOOTHER_CHEBYSHEV), OPERATOR),
            ("stencil5 FW", wr.Stencil5(po, sts, L, Lc), dict(op=pkg.OPERATOR_STENCIL5), None),
            ("stencil5 INJECT4", wr.Stencil5(po, sts, L, Lc, mode=3), dict(op=pkg.OPERATOR_STENCIL5, restrict_mode=pkg.RESTRICT_INJECT4), None),
            ("stencil5 chebyshev", wr.Stencil5Cheby(po, sts, L, Lc), dict(op=pkg.OPERATOR_STENCIL5, smoother=pkg.SMOOTHER_CHEBYSHEV), None)]
    for name, ref, kw, transfer in runs:
        ref.cycle = W
        u_ref, h_ref = ref.solve(b, tol=1e-9, max_cycles=5)
        assert np.isfinite(h_ref).all() and h_ref[-1] < h_ref[0], name
        with handle(pkg, L, Lc, **kw) as mg:
            mg.set_coefficient(a)
            if transfer is not None:
                mg.build_galerkin(transfer)
            mg.set_cycle(W)
            mg.set_rhs(b)
            st, h = mg.solve(tol=1e-9, max_cycles=5)
            u = mg.get_solution()
        print(f"{name}: history {h}, reference {h_ref}")
        assert hist_close(h, h_ref), (name, h, h_ref)
        assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref)), name


@pytest.mark.parametrize("cycle", [W, F], ids=["W", "F"])
def test_fmg_and_the_fmg_schedule(pkg, po, cycle):
    finest, coarsest = 7, 3
    b = po.rhs_sine(finest)
    ref = reference(po, finest, coarsest, OPERATOR, 1, gr.CONSISTENT, cycle, mu0=1)
    u_ref = ref.fmg(b)
    with built(pkg, finest, coarsest, OPERATOR, cycle, mu0=1) as mg:
        mg.set_guess(np.ones_like(b))
        u = mg.fullmultigrid(b)
    assert_iterate(po, ref, finest, u, u_ref, b, 1, "fmg")
    v = reference(po, finest, coarsest, OPERATOR, 1, gr.CONSISTENT, V, mu0=1).fmg(b)
    assert np.max(np.abs(u_ref - v)) > 1e-8 * np.max(np.abs(v)), "the inner cycles of FMG did not change with the kind"
    ref = reference(po, finest, coarsest, OPERATOR, 1, gr.CONSISTENT, cycle, mu0=1)
    u_ref, h_ref = ref.solve(b, tol=1e-8, max_cycles=30, schedule=gr.FMG)
    with built(pkg, finest, coarsest, OPERATOR, cycle, mu0=1, schedule=gr.FMG) as mg:
        mg.set_rhs(b)
        st, h = mg.solve(tol=1e-8, max_cycles=30)
        u = mg.get_solution()
    assert h_ref[-1] <= 1e-8 * h_ref[0]
    assert hist_close(h, h_ref), (h, h_ref)
    assert np.max(np.abs(u - u_ref)) <= 1e-10 * np.max(np.abs(u_ref))


def test_pcg_preconditioned_by_a_w_cycle(pkg, po):
    L, Lc = 8, 4
    b = po.rhs_sine(L)
    coef = po.stencil_from_nodes(nodes(L), L, L)
    ref = reference(po, L, Lc, OPERATOR, 1, gr.CONSISTENT, W)
    zeros = np.zeros_like(b)
    x_ref, h_ref, conv, brk = pcg_ref.pcg(pcg_ref.Operator(coef, np.float64), lambda r: ref.vcycle(L, zeros, r), b, zeros, tol=1e-8, max_iters=60)
    assert conv and not brk
    v = reference(po, L, Lc, OPERATOR, 1, gr.CONSISTENT, V)
    _, h_v, _, _ = pcg_ref.pcg(pcg_ref.Operator(coef, np.float64), lambda r: v.vcycle(L, zeros, r), b, zeros, tol=1e-8, max_iters=60)
    with built(pkg, L, Lc, OPERATOR, W) as mg:
        mg.set_rhs(b)
        st, h = mg.solve_pcg(tol=1e-8, max_iters=60)
        x = mg.get_solution()
        assert mg.graphs_cached() >= 1
    print(f"PCG with a W-cycle: {len(h) - 1} iterations (reference {len(h_ref) - 1}; with a V-cycle {len(h_v) - 1})")
    assert st.converged and len(h) == len(h_ref) and len(h_ref) < len(h_v)
    assert_hist(h, h_ref, RTOL64)
    assert pcg_ref.true_residual(b, x, nodes(L), L, po) <= 2e-8 * h[0]


@pytest.mark.parametrize("cycle", [W, F], ids=["W", "F"])
def test_profiled_handles_compute_the_same_bits(pkg, po, cycle):
    """cfg.profile = 1 (every launch eager, between events) and cfg.profile = 2 (the visits of level finest - 1 as one
    graph replay) against cfg.profile = 0 (the whole cycle one graph)"""
    finest, coarsest = 7, 3
    b = po.rhs_sine(finest)
    out = []
    for profile in (0, 1, 2):
        with built(pkg, finest, coarsest, OPERATOR, cycle, profile=profile) as mg:
            mg.set_rhs(b)
            st, h = mg.solve(tol=1e-8, max_cycles=8)
            out.append((h, mg.get_solution()))
            if profile == 2:
                assert mg.graphs_cached() >= 1
                p = mg.profile()
                # per cycle one replay of the coarse part between the finest level's own launches
                assert p["launches"][PROF_COARSE] == st.cycles, p
    for h, u in out[1:]:
        assert np.array_equal(h, out[0][0]) and np.array_equal(u, out[0][1])


def test_switching_the_kind_on_one_handle(pkg, po):
    finest, coarsest = 7, 3
    b = po.rhs_sine(finest)

    def run(mg):
        mg.set_rhs(b)
        mg.set_guess(np.zeros_like(b))
        st, h = mg.solve(tol=1e-8, max_cycles=8)
        return h, mg.get_solution()

    fresh = {}
    for cycle in (V, W, F):
        with built(pkg, finest, coarsest, OPERATOR, cycle) as mg:
            fresh[cycle] = run(mg)
    with handle(pkg, finest, coarsest) as mg:
        mg.set_coefficient(nodes(finest))
        mg.build_galerkin(OPERATOR)
        assert mg.cycle == V
        for cycle in (V, W, V, F, W, V):
            mg.set_cycle(cycle)
            assert mg.graphs_cached() == 0, "the setter drops the cached graphs"
            h, u = run(mg)
            assert np.array_equal(h, fresh[cycle][0]) and np.array_equal(u, fresh[cycle][1]), cycle
            assert mg.graphs_cached() >= 1
        # a rebuild keeps the kind
        mg.set_cycle(W)
        mg.build_galerkin(OPERATOR)
        assert mg.cycle == W
        h, u = run(mg)
        assert np.array_equal(h, fresh[W][0])
    assert not np.array_equal(fresh[V][0][:3], fresh[W][0][:3]) and not np.array_equal(fresh[F][0][:3], fresh[W][0][:3])


def test_refusals(pkg, po):
    L, Lc = 8, 5
    b = po.rhs_sine(L)
    cases = [("POISSON", dict()), ("MIXED", dict(dtype=pkg.DTYPE_MIXED)), ("multi-GPU", dict(n_gpus=2, devices=[0, 0]))]
    for word, kw in cases:
        with pkg.Multigrid(finest_level=L, coarsest_level=Lc, **kw) as mg:
            for cycle in (W, F):
                rc = pkg.lib().mgx_set_cycle(mg._h, cycle)
                assert rc == 5, (word, rc)                     # MGX_ERR_STATE
                assert word in pkg.lib().mgx_last_error(mg._h).decode(), (word, pkg.lib().mgx_last_error(mg._h))
            assert mg.cycle == V
            mg.set_rhs(b)
            st, h = mg.solve(tol=1e-8, max_cycles=3)            # the handle is still usable
            assert h[-1] < h[0]
    with built(pkg, L, Lc, BILINEAR, W) as mg:
        for bad in (3, -1, 17):
            assert pkg.lib().mgx_set_cycle(mg._h, bad) == 1     # MGX_ERR_INVALID
            with pytest.raises(pkg.MgxError, match="MGX_CYCLE"):
                mg.set_cycle(bad)
            assert mg.cycle == W


def test_511_contrast_1000_converges_in_the_reference_s_24_w_cycles(pkg, po):
    """the workload's size: 511^2, levels 9..5, contrast 1000, OPERATOR, double.  tests/test_opdep_cpu.py records 46
    V-cycles for the reference; its W-cycle needs 24"""
    L, Lc = 9, 5
    a = pcg_ref.contrast_coefficient(L, 1000.0)
    b = po.rhs_constant(L)
    ref = wr.Opdep(po, po.stencil_from_nodes(a, L, L), L, Lc)
    ref.cycle = W
    u_ref, h_ref = ref.solve(b, tol=1e-8, max_cycles=120)
    assert len(h_ref) - 1 == 24 and h_ref[-1] <= 1e-8 * h_ref[0]
    with handle(pkg, L, Lc) as mg:
        mg.set_coefficient(a)
        mg.build_galerkin(OPERATOR)
        mg.set_cycle(W)
        mg.set_rhs(b)
        st, h = mg.solve(tol=1e-8, max_cycles=120)
        assert st.converged and len(h) - 1 == 24
        assert hist_close(h, h_ref), (h, h_ref)
        mg.set_cycle(V)
        mg.set_guess(np.zeros_like(b))
        st, hv = mg.solve(tol=1e-8, max_cycles=120)
        assert st.converged and len(hv) - 1 == 46
    print(f"511^2 contrast 1000: W {len(h) - 1} cycles, V {len(hv) - 1}")
