"""GPU tests of mgx_solve_refine (include/mgx.h): fp64 defect correction of a general-operator F64 handle around the
cycle of its float copy of the hierarchy.

The main check is bit for bit against the COMPOSITION OF PUBLIC PIECES (tests/refine_ref.py's loop): the fp64 residual of
an independent F64 handle (mgx_residual), the cycle of an independent F32 handle that was given the float32 of the
parent's coefficients (mgx_vcycle_zero), and the scales recomputed from the history the device returned.  A wrong pass
kernel, a wrong float hierarchy or a wrong scale changes the final iterate; the history then has to agree with numpy's
norms of those residuals to tests/test_gpu_solve.py's HIST_TOL (only the order of the sum differs).

Shapes: a wave of the pass covers 62 output lanes = 124 columns and marches down R rows per chunk, R = clamp(rows / 128,
4, 8) (make_launch) unless MGX_ROWS says otherwise: 4 at every size of CASES.  (4, 3): 15^2 unknowns, a partial strip, four
chunks; (7, 3): 127 columns, two strips, the second a sliver; (8, 4): 255 columns, three strips, 64 chunks per strip and
more than one workgroup per strip.  ROWS_CASES run the other heights: MGX_ROWS 1, 3, 5, 8 and 64 on 63 rows, and level 10
at its own R = 7 (the benchmarked sizes, 2047^2 and 4095^2, run R = 8).
The fallback of launch_refine_pass to taller chunks (more blocks than the partial-sum buffer holds) cannot be entered:
the buffer is sized at creation for a launch of one row per chunk, the largest there is.  No test tries to."""
import ctypes as C

import numpy as np
import pytest

import nine_ref as nr
import refine_ref as rr
from pcg_ref import contrast_coefficient
from test_galerkin_cpu import random_stencil5
from test_gpu_galerkin import assert_same
from test_gpu_solve import HIST_TOL, hist_close

pytestmark = pytest.mark.gpu

BILINEAR, OPERATOR = 0, 1
INVALID, ALLOC, STATE = 1, 4, 5           # MGX_ERR_INVALID, MGX_ERR_ALLOC, MGX_ERR_STATE


def rand(L, seed):
    n = (1 << L) - 1
    return np.random.default_rng(seed).uniform(-1, 1, (n, n))


# ---- operators: how a handle of any dtype is given one, by name -----------------------------------------------------
def give_operator(pkg, mg, kind, L, Lc, transfer):
    galerkin = mg.cfg.op == pkg.OP_GALERKIN
    if kind.startswith("contrast"):
        mg.set_coefficient(contrast_coefficient(L, float(kind[len("contrast"):])))
    elif kind == "rot45":
        mg.set_tensor(*nr.rotated_tensor(L, 45.0, 0.5))
    elif kind == "random5":                 # non-symmetric, diagonally dominant; STENCIL5: one per level
        for lv in ([L] if galerkin else range(Lc, L + 1)):
            mg.set_stencil(lv, *[x.astype(mg.level_dtype(lv)) for x in random_stencil5(lv, 40 + lv, c_lo=4.0)])
    else:
        raise KeyError(kind)
    if galerkin:
        mg.build_galerkin(transfer)


def read_operator(pkg, mg, nine):
    """{level: coefficient arrays} of what the caller of a handle owns: every level (STENCIL5) or the finest (GALERKIN)"""
    L, Lc = mg.cfg.finest_level, mg.cfg.coarsest_level
    if mg.cfg.op == pkg.OP_GALERKIN:
        return {L: [mg.get_stencil9(L, q) for q in range(9)] if nine else [mg.get_stencil(L, q) for q in range(5)]}
    return {lv: [mg.get_stencil(lv, q) for q in range(5)] for lv in range(Lc, L + 1)}


def write_operator(pkg, mg, ops, transfer, dtype):
    for lv, st in ops.items():
        st = [np.asarray(x, dtype=dtype) for x in st]
        if len(st) == 9:
            mg.set_stencil9(lv, *st)
        else:
            mg.set_stencil(lv, *st)
    if mg.cfg.op == pkg.OP_GALERKIN:
        mg.build_galerkin(transfer)


def config(pkg, L, Lc, op, **kw):
    cfg = dict(finest_level=L, coarsest_level=Lc, op=op, mu1=2, mu2=2, schedule=0)
    cfg.update(kw)
    return cfg


def parent(pkg, cfg, kind, transfer=BILINEAR, cycle=None):
    mg = pkg.Multigrid(**cfg)
    give_operator(pkg, mg, kind, cfg["finest_level"], cfg["coarsest_level"], transfer)
    if cycle is not None:
        mg.set_cycle(cycle)
    return mg


def refine(mg, b, u0, tol, max_cycles):
    mg.set_rhs(b)
    mg.set_guess(u0)
    st, hist = mg.solve_refine(tol=tol, max_cycles=max_cycles)
    return st, hist, mg.get_solution()


def composition(pkg, mg, cfg, nine, transfer, cycle, b, u0, hist):
    """refine_ref's loop over two independent handles, the scales from `hist`: (u, history)"""
    L = cfg["finest_level"]
    ops = read_operator(pkg, mg, nine)
    with pkg.Multigrid(**cfg) as r64, pkg.Multigrid(**dict(cfg, dtype=pkg.DTYPE_F32)) as c32:
        write_operator(pkg, r64, ops, transfer, np.float64)
        write_operator(pkg, c32, ops, transfer, np.float32)
        if cycle is not None:
            c32.set_cycle(cycle)

        def cycle32(r32):
            c32.set_rhs(r32)
            c32.vcycle_zero()
            return c32.get_solution()

        return rr.refine(lambda u, bb: r64.residual(L, u, bb), cycle32, b, u0, history=hist)


# ---- 1. bit for bit against the composition of public pieces -------------------------------------------------------
J, CHEB, LINE_ALT, SGS = 0, 2, 6, 9
CASES = {
    # name: (L, Lc, op, cfg, operator, nine, transfer, cycle, random guess)
    "stencil5-4-3": (4, 3, "s5", dict(mu1=2, mu2=1), "contrast10", False, BILINEAR, None, False),
    "stencil5-7-3": (7, 3, "s5", dict(mu1=2, mu2=1), "contrast10", False, BILINEAR, None, True),
    "stencil5-8-4": (8, 4, "s5", dict(mu1=2, mu2=1), "contrast10", False, BILINEAR, None, False),
    "galerkin-bilinear": (7, 3, "gal", dict(), "contrast10", False, BILINEAR, None, False),
    "galerkin-opdep-cheby": (7, 3, "gal", dict(smoother=CHEB), "contrast100", False, OPERATOR, None, False),
    "galerkin-nine-sgs": (8, 4, "gal", dict(smoother=SGS, mu1=1, mu2=1), "rot45", True, BILINEAR, None, True),
    "galerkin-line-alt": (7, 3, "gal", dict(smoother=LINE_ALT, mu1=1, mu2=1), "contrast10", False, BILINEAR, None, False),
    "galerkin-w-cycle": (7, 3, "gal", dict(), "contrast10", False, BILINEAR, 1, False),
    "galerkin-bottom-smooth": (7, 3, "gal", dict(bottom=1), "contrast10", False, BILINEAR, None, False),
    "galerkin-non-symmetric": (7, 3, "gal", dict(), "random5", False, BILINEAR, None, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_refine_is_the_composition_of_public_pieces_bit_for_bit(pkg, name):
    L, Lc, op, extra, kind, nine, transfer, cycle, guess = CASES[name]
    cfg = config(pkg, L, Lc, pkg.OPERATOR_STENCIL5 if op == "s5" else pkg.OP_GALERKIN, **extra)
    b = rand(L, 3)
    u0 = rand(L, 4) if guess else np.zeros_like(b)
    with parent(pkg, cfg, kind, transfer, cycle) as mg:
        st, hist, u = refine(mg, b, u0, 0.0, 6)
        assert st.cycles == 6 and st.history_len == 7 and len(hist) == 7
        assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
        u_ref, hist_ref = composition(pkg, mg, cfg, nine, transfer, cycle, b, u0, hist)
    print(f"{name}: history {hist}, largest relative difference to numpy's norms {np.max(np.abs(hist - hist_ref) / hist_ref):.2e}")
    assert_same(u, u_ref, name)
    assert hist_close(hist, hist_ref, HIST_TOL), (hist, hist_ref)


# ---- 1b. the chunk heights of the pass ------------------------------------------------------------------------------
ROWS_CASES = {
    # name: (MGX_ROWS or None, L, Lc, op, cfg, operator, nine).  63 rows: R = 1: both neighbour rows of every row are
    # recomputed; 3: divides the rows exactly; 5: a last chunk of three rows; 8: the R of the benchmarked sizes; 64: one chunk
    **{f"stencil5-6-3-rows-{r}": (r, 6, 3, "s5", dict(mu1=2, mu2=1), "contrast10", False) for r in (1, 3, 5, 8, 64)},
    **{f"galerkin-nine-6-3-rows-{r}": (r, 6, 3, "gal", dict(), "rot45", True) for r in (3, 8)},
    # 1023 rows, the smallest level at which make_launch leaves R = 4 on its own: R = 7, 147 chunks, the last of one row; nine
    # strips, the last partial; several workgroups per strip.  bottom = SMOOTH (the dense solve stops at level 5)
    "galerkin-10-4-rows-default": (None, 10, 4, "gal", dict(bottom=1), "contrast10", False),
    "galerkin-nine-10-4-rows-default": (None, 10, 4, "gal", dict(bottom=1), "rot45", True),
}


@pytest.mark.parametrize("name", list(ROWS_CASES))
def test_refine_is_the_composition_at_every_chunk_height(pkg, monkeypatch, name):
    """the rolling window of k_refine_pass recomputes the row above and the row below a chunk from u and e: what depends
    on R.  MGX_ROWS is read when a handle is created, so it is set before all three are; random guess, six cycles"""
    rows, L, Lc, op, extra, kind, nine = ROWS_CASES[name]
    if rows is None:
        monkeypatch.delenv("MGX_ROWS", raising=False)
        assert ((1 << L) - 1) // 128 == 7                    # make_launch: R = clamp(rows / 128, 4, 8)
    else:
        monkeypatch.setenv("MGX_ROWS", str(rows))
    cfg = config(pkg, L, Lc, pkg.OPERATOR_STENCIL5 if op == "s5" else pkg.OP_GALERKIN, **extra)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, kind) as mg:
        st, hist, u = refine(mg, b, u0, 0.0, 6)
        assert st.cycles == 6 and len(hist) == 7 and np.isfinite(hist).all() and hist[-1] < hist[0], hist
        u_ref, hist_ref = composition(pkg, mg, cfg, nine, BILINEAR, None, b, u0, hist)
    print(f"{name}: history {hist}, largest relative difference to numpy's norms {np.max(np.abs(hist - hist_ref) / hist_ref):.2e}")
    assert_same(u, u_ref, name)
    assert hist_close(hist, hist_ref, HIST_TOL), (hist, hist_ref)


# ---- 2. contract ---------------------------------------------------------------------------------------------------
def test_contract_b_unchanged_u_the_iterate_stats_and_eager_launches(pkg, monkeypatch):
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg:
        # max_cycles = 0: one entry, U left alone
        st, hist, u = refine(mg, b, u0, 1e-11, 0)
        assert st.cycles == 0 and st.history_len == 1 and len(hist) == 1 and st.converged == 0
        assert_same(u, u0, "U after max_cycles = 0")
        assert hist[0] == pytest.approx(mg.residual_norm(), rel=1e-12)
        st, hist, u = refine(mg, b, u0, 1e-9, 40)
        assert st.converged == 1 and st.cycles == st.history_len - 1 == len(hist) - 1 and 0 < st.cycles < 40
        assert st.initial_residual == hist[0] and st.final_residual == hist[-1] and hist[-1] <= 1e-9 * hist[0]
        assert st.fine_updates == st.cycles * 4 * (mg.n() ** 2)           # V(2,2) of the float cycle
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B after solve_refine")
        # U is the iterate the last history entry belongs to
        assert mg.residual_norm() == pytest.approx(hist[-1], rel=HIST_TOL)
        assert mg.graphs_cached() >= 0
    monkeypatch.setenv("MGX_GRAPH", "0")
    with parent(pkg, cfg, "contrast10") as eager:
        st2, hist2, u2 = refine(eager, b, u0, 1e-9, 40)
        assert eager.graphs_cached() == -1
    assert_same(u2, u, "MGX_GRAPH=0")
    assert np.array_equal(hist2, hist) and st2.cycles == st.cycles


# ---- 3. convergence on the device ------------------------------------------------------------------------------------
def test_refine_converges_like_fp64_where_an_f32_handle_stalls(pkg):
    L, Lc = 8, 4
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b = rand(L, 3)
    with parent(pkg, cfg, "contrast10") as mg:
        mg.set_rhs(b)
        s64, h64 = mg.solve(tol=1e-11, max_cycles=80)
        sr, hr, _ = refine(mg, b, np.zeros_like(b), 1e-11, 80)
    print(f"fp64 solve: {s64.cycles} cycles; solve_refine: {sr.cycles} cycles, final {hr[-1] / hr[0]:.2e}")
    assert s64.converged == 1 and sr.converged == 1
    assert abs(sr.cycles - s64.cycles) <= 1
    with parent(pkg, dict(cfg, dtype=pkg.DTYPE_F32), "contrast10") as f32:
        f32.set_rhs(b.astype(np.float32))
        _, h32 = f32.solve(tol=0.0, max_cycles=40)
    print(f"F32 handle: best relative residual {np.min(h32) / h32[0]:.2e}")
    assert np.min(h32) > 1e-7 * h32[0]


# ---- 4. state model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["s5", "gal"])
def test_a_new_operator_between_two_refines_is_followed(pkg, op):
    L, Lc = 6, 3
    cfg = config(pkg, L, Lc, pkg.OPERATOR_STENCIL5 if op == "s5" else pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast100") as fresh:
        _, h1, u1 = refine(mg, b, u0, 0.0, 4)
        give_operator(pkg, mg, "contrast100", L, Lc, BILINEAR)
        _, h2, u2 = refine(mg, b, u0, 0.0, 4)
        _, hf, uf = refine(fresh, b, u0, 0.0, 4)
    assert not np.array_equal(u1, u2)
    assert_same(u2, uf, "second operator")
    assert np.array_equal(h2, hf)


def test_fp64_solve_after_a_refine_is_that_of_a_handle_that_never_refined(pkg):
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast10") as never:
        for h in (mg, never):
            h.set_rhs(b)
        mg.set_guess(u0)
        mg.solve(tol=0.0, max_cycles=2)                                   # (graphs captured before the refine, too)
        refine(mg, b, u0, 0.0, 3)                                         # an odd number of u <-> tmp swaps
        out = []
        for h in (mg, never):
            h.set_guess(u0)
            st, hist = h.solve(tol=0.0, max_cycles=5)
            u = h.get_solution()
            h.set_guess(u0)
            stp, histp = h.solve_pcg(tol=0.0, max_iters=3)
            out.append((hist, u, histp, h.get_solution()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])
    assert_same(out[0][1], out[1][1], "solve after refine")
    assert_same(out[0][3], out[1][3], "solve_pcg after refine")


def test_set_cycle_between_two_refines_is_honoured(pkg):
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast10", cycle=pkg.CYCLE_W) as fresh:
        _, hv, uv = refine(mg, b, u0, 0.0, 3)
        mg.set_cycle(pkg.CYCLE_W)
        _, hw, uw = refine(mg, b, u0, 0.0, 3)
        _, hf, uf = refine(fresh, b, u0, 0.0, 3)
    assert not np.array_equal(uv, uw) and hw[-1] < hv[-1]
    assert_same(uw, uf, "W after V")
    assert np.array_equal(hw, hf)


def test_nine_point_and_back_to_five_point_is_followed(pkg):
    L, Lc = 6, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "rot45") as nine:
        _, h5, u5 = refine(mg, b, u0, 0.0, 4)
        give_operator(pkg, mg, "rot45", L, Lc, BILINEAR)
        _, h9, u9 = refine(mg, b, u0, 0.0, 4)
        _, hn, un = refine(nine, b, u0, 0.0, 4)
        give_operator(pkg, mg, "contrast10", L, Lc, BILINEAR)
        _, h5b, u5b = refine(mg, b, u0, 0.0, 4)
    assert_same(u9, un, "nine-point after five-point")
    assert np.array_equal(h9, hn)
    assert_same(u5b, u5, "five-point after nine-point")
    assert np.array_equal(h5b, h5)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------
def raw_refine(pkg, mg, tol=1e-8, max_cycles=3):
    rc = pkg.lib().mgx_solve_refine(mg._h, tol, max_cycles, None, None, 0)
    return rc, pkg.lib().mgx_last_error(mg._h).decode()


def still_solves(mg, L, dt=np.float64):
    mg.set_rhs(rand(L, 5).astype(dt))
    st, hist = mg.solve(tol=0.0, max_cycles=2)
    assert np.isfinite(hist).all() and hist[-1] < hist[0]


def test_poisson_and_f32_handles_are_refused_with_the_reason(pkg):
    L, Lc = 6, 3
    base = dict(finest_level=L, coarsest_level=Lc, mu1=2, mu2=2, schedule=0)
    for dtype in (pkg.DTYPE_F64, pkg.DTYPE_MIXED):
        with pkg.Multigrid(dtype=dtype, **base) as mg:
            rc, msg = raw_refine(pkg, mg)
            assert rc == STATE and "POISSON" in msg and "MIXED" in msg, msg
            ms = C.c_double()
            assert pkg.lib().mgx_time_refine_pass(mg._h, 1, C.byref(ms)) == STATE
            still_solves(mg, L)
    with parent(pkg, config(pkg, L, Lc, pkg.OPERATOR_STENCIL5, dtype=pkg.DTYPE_F32), "contrast10") as mg:
        rc, msg = raw_refine(pkg, mg)
        assert rc == STATE and "F64" in msg, msg
        still_solves(mg, L, np.float32)


@pytest.mark.parametrize("kind", ["n_gpus", "rank"])
def test_multi_gpu_and_rank_handles_are_refused_with_the_reason(pkg, kind):
    """(the rank case spends its seconds in ncclCommInitRank: a rank handle cannot be created without it)"""
    kw = dict(finest_level=9, coarsest_level=6, mu1=2, mu2=2, schedule=0, cut_level=7)
    mg = pkg.Multigrid(n_gpus=2, devices=[0, 0], **kw) if kind == "n_gpus" else pkg.Multigrid.rank(0, 1, rccl_id=pkg.rccl_unique_id(), **kw)
    with mg:
        rc, msg = raw_refine(pkg, mg)
        assert rc == STATE and "multi-GPU" in msg, msg
        ms = C.c_double()
        assert pkg.lib().mgx_time_refine_pass(mg._h, 1, C.byref(ms)) == STATE
        still_solves(mg, 9)


def test_unbuilt_hierarchies_and_bad_arguments_are_refused(pkg):
    """a GALERKIN handle before its hierarchy is built: MGX_ERR_STATE; bad arguments on a handle that is ready:
    MGX_ERR_INVALID; the handle solves and refines afterwards"""
    L, Lc = 6, 3
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OP_GALERKIN)) as mg:
        rc, msg = raw_refine(pkg, mg)
        assert rc == STATE and "not set" in msg, msg
        mg.set_coefficient(contrast_coefficient(L, 10.0))
        rc, msg = raw_refine(pkg, mg)
        assert rc == STATE and "not built" in msg, msg
        mg.build_galerkin()
        assert raw_refine(pkg, mg, tol=float("nan"))[0] == INVALID
        assert raw_refine(pkg, mg, tol=-1.0)[0] == INVALID
        assert raw_refine(pkg, mg, max_cycles=-1)[0] == INVALID
        still_solves(mg, L)
        st, hist, _ = refine(mg, rand(L, 3), np.zeros((mg.n(), mg.n())), 1e-10, 60)
        assert st.converged == 1


# ---- 6. mgx_time_refine_pass ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contrast10", "rot45"])
def test_time_refine_pass_times_the_pass_and_changes_nothing(pkg, kind):
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, kind) as mg:
        with pytest.raises(pkg.MgxError, match="invalid state.*mgx_solve_refine first"):
            mg.time_refine_pass(2)
        _, hist, u = refine(mg, b, u0, 0.0, 3)
        ms = mg.time_refine_pass(5)
        assert ms > 0.0
        assert_same(mg.get_solution(), u, "U after time_refine_pass")
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B after time_refine_pass")
        assert mg.residual_norm() == pytest.approx(hist[-1], rel=HIST_TOL)
        # ... and the next refine is the one of a handle that was never timed
        _, hist2, u2 = refine(mg, b, u0, 0.0, 3)
        assert_same(u2, u, "refine after time_refine_pass")
        assert np.array_equal(hist2, hist)
        with pytest.raises(pkg.MgxError, match="invalid argument"):
            mg.time_refine_pass(0)
