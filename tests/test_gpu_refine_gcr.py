"""GPU tests of mgx_solve_refine_gcr (include/mgx.h): restarted GCR in fp64 on the finest level of a general-operator F64
handle, preconditioned by the scaled cycle of the handle's float copy of the hierarchy.

The main check is against the COMPOSITION OF PUBLIC PIECES (tests/refine_gcr_ref.py's loop): A z = -mgx_residual(z, 0) of an
independent F64 handle (the sign flip is exact), the cycle of an independent F32 handle that was given the float32 of the
parent's coefficients (mgx_vcycle_zero), exactly as composition() of tests/test_gpu_refine.py, and the scales from the
history the device returned.  The device then differs from that loop only in the summation order of its dots.  Bounds: the
same iteration count, every history entry within RTOL64 h + 1e-14 h0 (tests/test_gpu_pcg.py), the iterate within 1e-9 of
its largest entry (tests/test_gpu_gcr.py).

What the summation order is worth is NOT small once it has flipped one float rounding of r / s_k: tests/test_refine_gcr_cpu.py
measures numpy's order against the reversed one at 2.5e-4 of the history bound over the six iterations of the 9..5 case
here, and at 0.5 of it when the same pair runs on to 1e-10 - the first flip is a matter of chance (2.6e5 entries per
iteration, each one chance in 1e7).  So the reference is given the DEVICE'S order (refine_gcr_ref.device_dot: the lanes,
waves, workgroups and the one-workgroup reduction of csrc/mgx_krylov.hpp), which leaves nothing to chance: every scalar of
the reference is then the device's, bit for bit, and each test prints the fraction of the bounds it used (measured on an
MI355X: 0 of both bounds in every case below; only hist[0], which the device takes from its residual-norm kernel, is
summed in another order, and it agreed as well).

Shapes (tests/test_gpu_refine.py documents them; the passes here run k_refine_pass's geometry): (4, 3): 15^2, a partial
strip; (7, 3): 127 columns, two strips, the second a sliver; (8, 4): three strips, several workgroups per strip; (9, 5):
five strips, 160 workgroups, the geometry k_gcr_orth<double> is tested at.  Parity runs: restart 4, six iterations with
tol 0 (slots 0 .. 3 and a wrap); deep bases: restart 8, nine iterations (slots 0 .. 7 and a wrap).

Beyond the parity at R = 4 (sections 6 .. 9; times and fractions measured on an MI355X):
  * chunk heights: tests/test_gpu_refine.py's ROWS_CASES under check_parity with the reference's dots at the same height - MGX_ROWS
    1, 3, 5, 8, 64 on 63 rows, 3 and 8 nine-point, level 10 at its own R = 7 five- and nine-point.  0 of both bounds everywhere but
    galerkin-10-4-rows-default, 2.0e-7 of the history bound (its first entry); 0.02 s each, the level-10 cases 0.3 s.  A launch that
    ignores MGX_ROWS in the driver's loop alone stays self-consistent at R = 4 and only sums in another order: it uses up to 3.0e-2 of
    the history and 2.0e-3 of the iterate bound here and passes - the bounds are tests/test_gpu_pcg.py's and are not tightened.
  * the breakdown exit on finite data (V(0,0), checkerboard b, zero guess: history [63.], U and B restored, twice; then random
    data against the composition, 0 of both bounds, 1162.82 -> 1161.21; then mgx_solve_gcr and mgx_solve_refine as on a handle that
    never broke down), 0.04 s; and no breakdown from a random guess, 0.02 s.  k_gcr_reduce sets alpha = 0 with the flag, so an update
    pass that ignored the flag would add 0 z' and 0 q' and rewrite r32 with the bits it holds: no test can tell, and none here does.
  * power-of-two invariance at 2^-160 and 2^+160, beyond float's range, for mgx_solve_refine_gcr and mgx_solve_refine, six
    iterations at tol 0 and to 1e-10 (11 / 8 iterations, 19 / 13 cycles in the numpy statements): bit for bit, 0.02 s each.
  * small exits: b = 0, u = 0; stats = NULL, history = NULL, a short history buffer; mgx_time_refine_gcr_pass on a STENCIL5 handle;
    its guard, which accepts the call after mgx_solve_refine plus mgx_solve_gcr (include/mgx.h says so).  0.03 s at the most."""
import ctypes as C

import numpy as np
import pytest

import refine_gcr_ref as rg
from pcg_ref import contrast_coefficient
from test_gpu_galerkin import assert_same
from test_gpu_pcg import RTOL64, assert_hist
from test_gpu_refine import (BILINEAR, CASES as REFINE_CASES, INVALID, OPERATOR, ROWS_CASES, STATE, config, give_operator, parent, rand, read_operator,
                             refine, write_operator)
from test_refine_gcr_cpu import NINE_FIVE, TRUE_GAP

pytestmark = pytest.mark.gpu

X_TOL64 = 1e-9                                  # tests/test_gpu_gcr.py's bound on the fp64 iterate


@pytest.fixture(autouse=True)
def chunk_height(monkeypatch):
    """MGX_ROWS unset - device_dot(rows_per_chunk = 0) is make_launch's own choice - unless a test asks for a height: the
    fixture's value sets the variable, before the handles are created (it is read there)"""
    monkeypatch.delenv("MGX_ROWS", raising=False)
    return lambda rows: monkeypatch.setenv("MGX_ROWS", str(rows))


def refine_gcr(mg, b, u0, tol, max_iters, restart):
    mg.set_rhs(b)
    mg.set_guess(u0)
    st, hist = mg.solve_refine_gcr(tol=tol, max_iters=max_iters, restart=restart)
    return st, hist, mg.get_solution()


def composition(pkg, mg, cfg, nine, transfer, cycle, b, u0, hist, tol, max_iters, restart, rows=0):
    """refine_gcr_ref's loop over two independent handles, the scales from `hist`, the dots in the device's order at `rows`
    rows per chunk (0: make_launch's own choice): (x, history, converged, breakdown)"""
    L = cfg["finest_level"]
    ops = read_operator(pkg, mg, nine)
    zero = np.zeros_like(b)
    with pkg.Multigrid(**cfg) as r64, pkg.Multigrid(**dict(cfg, dtype=pkg.DTYPE_F32)) as c32:
        write_operator(pkg, r64, ops, transfer, np.float64)
        write_operator(pkg, c32, ops, transfer, np.float32)
        if cycle is not None:
            c32.set_cycle(cycle)

        def A(z):
            return -r64.residual(L, z, zero)

        def cycle32(r32):
            c32.set_rhs(r32)
            c32.vcycle_zero()
            return c32.get_solution()

        return rg.refine_gcr(A, cycle32, b, u0, tol, max_iters, restart, history=hist, dot=lambda p, q: rg.device_dot(p, q, rows))


def used(h, h_ref, u, x_ref):
    """the fractions of the history and the iterate bound that a result uses"""
    k = min(len(h), len(h_ref))
    return (float(np.max(np.abs(h[:k] - h_ref[:k]) / (RTOL64 * h_ref[:k] + 1e-14 * h_ref[0]))),
            float(np.max(np.abs(u - x_ref)) / np.max(np.abs(x_ref)) / X_TOL64))


def check_parity(pkg, name, case, tol, iters, restart, floor=None, rows=0):
    """rows: the MGX_ROWS the handles are created under (the caller has set it), 0 for none"""
    L, Lc, op, extra, kind, nine, transfer, cycle, guess = case
    cfg = config(pkg, L, Lc, pkg.OPERATOR_STENCIL5 if op == "s5" else pkg.OP_GALERKIN, **extra)
    b = rand(L, 3)
    u0 = rand(L, 4) if guess else np.zeros_like(b)
    with parent(pkg, cfg, kind, transfer, cycle) as mg:
        st, hist, u = refine_gcr(mg, b, u0, tol, iters, restart)
        assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
        x_ref, h_ref, conv_ref, brk_ref = composition(pkg, mg, cfg, nine, transfer, cycle, b, u0, hist, tol, iters, restart, rows)
    assert not brk_ref
    if floor is not None:
        assert h_ref[-1] >= floor * h_ref[0], h_ref     # well above the fp64 floor: the comparison means something
    fh, fx = used(hist, h_ref, u, x_ref)
    print(f"\n[refine-gcr] {name}: {st.cycles} iterations (reference {len(h_ref) - 1}), last / first {hist[-1] / hist[0]:.3g}; used {fh:.3g} of the "
          f"history bound, {fx:.3g} of the iterate bound")
    assert st.cycles == len(h_ref) - 1 and st.history_len == len(h_ref) and st.converged == int(conv_ref)
    assert_hist(hist, h_ref, RTOL64)
    assert np.max(np.abs(u - x_ref)) <= X_TOL64 * np.max(np.abs(x_ref))


# ---- 1. parity with the composition of public pieces ---------------------------------------------------------------
# tests/test_gpu_refine.py's cases - (L, Lc, op, cfg, operator, nine, transfer, cycle, random guess): STENCIL5 at (4, 3), (7, 3)
# and (8, 4); GALERKIN with either transfer, Jacobi, Chebyshev, LINE_ALT and COLOR_SGS, a nine-point finest level (rot45),
# the W-cycle, bottom = SMOOTH and the non-symmetric random5 operator; zero and random guesses - and the 9..5 case
CASES = dict(REFINE_CASES)
CASES["galerkin-9-5"] = (NINE_FIVE["L"], NINE_FIVE["Lc"], "gal", dict(), f"contrast{NINE_FIVE['contrast']:g}", False, BILINEAR, None, False)
assert (NINE_FIVE["restart"], NINE_FIVE["iters"]) == (4, 6)


@pytest.mark.parametrize("name", list(CASES))
def test_refine_gcr_is_the_composition_of_public_pieces(pkg, name):
    check_parity(pkg, name, CASES[name], 0.0, 6, 4)


# ---- 2. deep bases -----------------------------------------------------------------------------------------------------
# restart 8, nine iterations, tol 0: slots 0 .. 7 and a wrap, k_gcr_dots<double, 1..7> and k_gcr_orth<double, 0..7> between the
# two mixed passes.  Weak smoothing (V(1,0), omega = 0.3) keeps the ninth entry at 1.2e-3 of the first (measured with the
# numpy hierarchies of tests/galerkin_ref.py at both sizes), far above the fp64 floor
DEEP = {
    "deep-8-4": (8, 4, "gal", dict(mu1=1, mu2=0, omega=0.3), "contrast10", False, BILINEAR, None, False),
    "deep-9-5": (9, 5, "gal", dict(mu1=1, mu2=0, omega=0.3), "contrast10", False, BILINEAR, None, False),
}


@pytest.mark.parametrize("name", list(DEEP))
def test_deep_bases_match_the_composition(pkg, name):
    check_parity(pkg, name, DEEP[name], 0.0, 9, 8, floor=1e-4)


# ---- 3. contract ---------------------------------------------------------------------------------------------------------
def test_contract_b_unchanged_u_the_iterate_stats_and_eager_launches(pkg, monkeypatch):
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg:
        # max_iters = 0: one entry, U left alone
        st, hist, u = refine_gcr(mg, b, u0, 1e-11, 0, 4)
        assert st.cycles == 0 and st.history_len == 1 and len(hist) == 1 and st.converged == 0
        assert_same(u, u0, "U after max_iters = 0")
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B after max_iters = 0")
        assert hist[0] == pytest.approx(mg.residual_norm(), rel=1e-12)
        st, hist, u = refine_gcr(mg, b, u0, 1e-9, 40, 4)
        assert st.converged == 1 and st.cycles == st.history_len - 1 == len(hist) - 1 and 0 < st.cycles < 40
        assert st.initial_residual == hist[0] and st.final_residual == hist[-1] and hist[-1] <= 1e-9 * hist[0]
        assert st.fine_updates == st.cycles * 4 * (mg.n() ** 2)           # V(2,2) of the float cycle
        assert np.all(hist[1:] <= hist[:-1] * (1 + 1e-12)), hist
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B after solve_refine_gcr")
        assert_same(mg.get_solution(), u, "U after solve_refine_gcr")
        # U is the iterate the last history entry belongs to: the true residual against the recursive one
        true = mg.residual_norm()
        print(f"recursive {hist[-1]:.6e}, true {true:.6e}: gap {abs(true - hist[-1]) / true:.2e} (bound {TRUE_GAP:g})")
        assert abs(true - hist[-1]) <= TRUE_GAP * true
        assert mg.graphs_cached() >= 0
    monkeypatch.setenv("MGX_GRAPH", "0")
    with parent(pkg, cfg, "contrast10") as eager:
        st2, hist2, u2 = refine_gcr(eager, b, u0, 1e-9, 40, 4)
        assert eager.graphs_cached() == -1
    assert_same(u2, u, "MGX_GRAPH=0")
    assert np.array_equal(hist2, hist) and st2.cycles == st.cycles


# ---- 4. state model -------------------------------------------------------------------------------------------------------
def raw(pkg, mg, tol=1e-8, max_iters=3, restart=4):
    rc = pkg.lib().mgx_solve_refine_gcr(mg._h, tol, max_iters, restart, None, None, 0)
    return rc, pkg.lib().mgx_last_error(mg._h).decode()


def still_solves(mg, L, dt=np.float64):
    mg.set_rhs(rand(L, 5).astype(dt))
    st, hist = mg.solve(tol=0.0, max_cycles=2)
    assert np.isfinite(hist).all() and hist[-1] < hist[0]


def test_handles_that_cannot_refine_are_refused_with_the_reason(pkg):
    L, Lc = 6, 3
    base = dict(finest_level=L, coarsest_level=Lc, mu1=2, mu2=2, schedule=0)
    ms = C.c_double()
    for dtype in (pkg.DTYPE_F64, pkg.DTYPE_MIXED):
        with pkg.Multigrid(dtype=dtype, **base) as mg:
            rc, msg = raw(pkg, mg)
            assert rc == STATE and "POISSON" in msg and "mgx_solve_refine_gcr" in msg, msg
            assert pkg.lib().mgx_time_refine_gcr_pass(mg._h, 0, 1, C.byref(ms)) == STATE
            still_solves(mg, L)
    with parent(pkg, config(pkg, L, Lc, pkg.OPERATOR_STENCIL5, dtype=pkg.DTYPE_F32), "contrast10") as mg:
        rc, msg = raw(pkg, mg)
        assert rc == STATE and "F64" in msg and "mgx_solve_refine_gcr" in msg, msg
        still_solves(mg, L, np.float32)
    with pkg.Multigrid(n_gpus=2, devices=[0, 0], finest_level=9, coarsest_level=6, mu1=2, mu2=2, schedule=0, cut_level=7) as mg:
        rc, msg = raw(pkg, mg)
        assert rc == STATE and "multi-GPU" in msg, msg
        assert pkg.lib().mgx_time_refine_gcr_pass(mg._h, 0, 1, C.byref(ms)) == STATE
        still_solves(mg, 9)


def test_unbuilt_hierarchies_and_bad_arguments_are_refused(pkg):
    L, Lc = 6, 3
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OP_GALERKIN)) as mg:
        rc, msg = raw(pkg, mg)
        assert rc == STATE and "not set" in msg, msg
        mg.set_coefficient(contrast_coefficient(L, 10.0))
        rc, msg = raw(pkg, mg)
        assert rc == STATE and "not built" in msg, msg
        mg.build_galerkin()
        for kw in (dict(tol=float("nan")), dict(tol=-1.0), dict(max_iters=-1), dict(restart=0), dict(restart=pkg.GCR_MAX_RESTART + 1)):
            rc, msg = raw(pkg, mg, **kw)
            assert rc == INVALID and "mgx_solve_refine_gcr" in msg, (kw, msg)
        assert pkg.GCR_MAX_RESTART + 1 == 9
        still_solves(mg, L)
        st, hist, _ = refine_gcr(mg, rand(L, 3), np.zeros((mg.n(), mg.n())), 1e-10, 60, pkg.GCR_MAX_RESTART)
        assert st.converged == 1
        st, hist, _ = refine_gcr(mg, rand(L, 3), np.zeros((mg.n(), mg.n())), 1e-10, 60, 1)
        assert st.converged == 1


@pytest.mark.parametrize("kind", ["contrast10", "rot45"])
def test_time_refine_gcr_pass_times_the_passes_and_changes_nothing(pkg, kind):
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, kind) as mg:
        with pytest.raises(pkg.MgxError, match="invalid state.*mgx_solve_refine_gcr first"):
            mg.time_refine_gcr_pass(0, 2)
        _, hist, u = refine_gcr(mg, b, u0, 0.0, 3, 2)
        for which in (0, 1, 0):
            assert mg.time_refine_gcr_pass(which, 3) > 0.0
        assert_same(mg.get_solution(), u, "U after time_refine_gcr_pass")
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B after time_refine_gcr_pass")
        # ... and the next solve is the one of a handle that was never timed
        _, hist2, u2 = refine_gcr(mg, b, u0, 0.0, 3, 2)
        assert_same(u2, u, "solve_refine_gcr after time_refine_gcr_pass")
        assert np.array_equal(hist2, hist)
        for which, reps in ((2, 1), (-1, 1), (0, 0)):
            with pytest.raises(pkg.MgxError, match="invalid argument"):
                mg.time_refine_gcr_pass(which, reps)


def test_a_new_operator_or_transfer_between_two_calls_is_followed(pkg):
    """the next call after mgx_set_coefficient, and after a rebuild with the other transfer, is that of a fresh handle: the
    float copy was rebuilt"""
    L, Lc = 6, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast100") as fresh, parent(pkg, cfg, "contrast100", OPERATOR) as fresh_op:
        _, h1, u1 = refine_gcr(mg, b, u0, 0.0, 5, 3)
        give_operator(pkg, mg, "contrast100", L, Lc, BILINEAR)
        _, h2, u2 = refine_gcr(mg, b, u0, 0.0, 5, 3)
        _, hf, uf = refine_gcr(fresh, b, u0, 0.0, 5, 3)
        mg.build_galerkin(OPERATOR)
        _, h3, u3 = refine_gcr(mg, b, u0, 0.0, 5, 3)
        _, ho, uo = refine_gcr(fresh_op, b, u0, 0.0, 5, 3)
    assert not np.array_equal(u1, u2) and not np.array_equal(u2, u3)
    assert_same(u2, uf, "second operator")
    assert np.array_equal(h2, hf)
    assert_same(u3, uo, "other transfer")
    assert np.array_equal(h3, ho)


def test_set_cycle_between_two_calls_reaches_the_float_copy(pkg):
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast10", cycle=pkg.CYCLE_W) as fresh:
        _, hv, uv = refine_gcr(mg, b, u0, 0.0, 3, 4)
        mg.set_cycle(pkg.CYCLE_W)
        _, hw, uw = refine_gcr(mg, b, u0, 0.0, 3, 4)
        _, hf, uf = refine_gcr(fresh, b, u0, 0.0, 3, 4)
    assert not np.array_equal(uv, uw) and hw[-1] < hv[-1]
    assert_same(uw, uf, "W after V")
    assert np.array_equal(hw, hf)


# ---- 5. interleaving -------------------------------------------------------------------------------------------------------
def test_the_other_entry_points_keep_their_bits_around_a_call(pkg):
    """mgx_solve_gcr, mgx_solve_refine, mgx_solve (and mgx_solve_pcg, mgx_vcycle) - one mgx_solve_refine_gcr - the same again:
    the same bits both times, and those of a handle that never made the new call (the Krylov workspace and the float copy are
    shared)"""
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)

    def three(h):
        out = []
        for call in (lambda: h.solve_gcr(tol=0.0, max_iters=5, restart=3), lambda: h.solve_refine(tol=0.0, max_cycles=3),
                     lambda: h.solve(tol=0.0, max_cycles=3), lambda: h.solve_pcg(tol=0.0, max_iters=3)):
            h.set_guess(u0)
            _, hist = call()
            out.append((hist, h.get_solution()))
        h.set_guess(u0)
        h.vcycle()
        out.append((np.array([h.residual_norm()]), h.get_solution()))
        return out

    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast10") as never:
        for h in (mg, never):
            h.set_rhs(b)
        before = three(mg)
        st, hist, _ = refine_gcr(mg, b, u0, 0.0, 5, 3)                     # (an odd number of iterations, a wrap of the basis)
        assert st.cycles == 5 and hist[-1] < hist[0]
        after = three(mg)
        want = three(never)
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B at the end")
    for i, (x, y, z) in enumerate(zip(before, after, want)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[0], z[0]), i
        assert_same(x[1], y[1], f"entry point {i}: before / after")
        assert_same(x[1], z[1], f"entry point {i}: against a handle that never made the call")


# ---- 6. the chunk heights of the two mixed passes ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROWS_CASES))
def test_refine_gcr_is_the_composition_at_every_chunk_height(pkg, chunk_height, name):
    """k_refine_direction recomputes zrow(r0 - 1) above and zrow(r1) below its chunk from z32, and takes the zero ring at
    r1 == N without a load: what depends on R, as k_refine_update's rows and the order of every dot do.  tests/test_gpu_refine.py's
    heights - MGX_ROWS 1, 3, 5, 8, 64 on 63 rows, 3 and 8 nine-point, level 10 at its own R = 7 five- and nine-point -
    with the reference's dots summed at the same height; restart 4, six iterations, tol 0, a random guess.  The height is
    set before all three handles are created.  Measured on an MI355X: see the module docstring"""
    rows, L, Lc, op, extra, kind, nine = ROWS_CASES[name]
    if rows is None:
        assert ((1 << L) - 1) // 128 == 7                    # make_launch: R = clamp(rows / 128, 4, 8)
    else:
        chunk_height(rows)
    check_parity(pkg, name, (L, Lc, op, extra, kind, nine, BILINEAR, None, True), 0.0, 6, 4, rows=rows or 0)


# ---- 7. the breakdown exit, on finite data -------------------------------------------------------------------------------------
def checkerboard(L):
    i = np.arange((1 << L) - 1)
    return np.where((i[:, None] + i[None, :]) % 2 == 0, 1.0, -1.0)


def last_error(pkg, mg):
    return pkg.lib().mgx_last_error(mg._h).decode()


BREAK_CFG = dict(mu1=0, mu2=0)                  # no smoothing: the cycle is P A_c^-1 R, and full weighting of a checkerboard is 4 - 8 + 4 = 0


def test_breakdown_exit_restores_u_and_b_and_leaves_no_flag_behind(pkg):
    """GALERKIN 6..3, V(0,0), exact bottom solve, b = (-1)^(i+j), zero guess: the restricted float residual is exactly zero at
    every coarse point, the float cycle returns exactly zero, z = 0 and q'.q' = 0 at iteration 1 (tests/test_handle_model.py
    holds the numpy statement to that: history [63.], x untouched).  The device: MGX_OK with the reason, nothing updated by
    k_refine_update after the flag, U the guess and B the caller's b bit for bit; the same again on a second call; then a
    call on random data matches the composition (the flag in the scalar block it shares with mgx_solve_gcr and mgx_solve_pcg
    is gone), and mgx_solve_gcr and mgx_solve_refine are those of a handle that never broke down"""
    L, Lc = 6, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN, **BREAK_CFG)
    b, zero = checkerboard(L), np.zeros(((1 << L) - 1,) * 2)
    rb, ru = rand(L, 3), rand(L, 4)

    def others(h):
        out = []
        for call in (lambda: h.solve_gcr(tol=0.0, max_iters=3, restart=2), lambda: h.solve_refine(tol=0.0, max_cycles=2)):
            h.set_rhs(rb)
            h.set_guess(ru)
            _, hist = call()
            out.append((hist, h.get_solution(), h.get_level(L, pkg.VEC_B)))
        return out

    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast10") as never:
        seen = []
        for _ in range(2):                                  # the second call: from the flag and the scalars the first one left
            st, hist, u = refine_gcr(mg, b, zero, 0.0, 6, 4)        # MGX_OK: anything else raises
            msg = last_error(pkg, mg)
            print(f"breakdown: history {hist}, '{msg}'")
            assert st.converged == 0 and st.cycles == 0 and st.history_len == 1 and len(hist) == 1
            assert hist[0] == pytest.approx(63.0, rel=RTOL64)
            assert "GCR breakdown at iteration 1" in msg and "q'.q'" in msg
            assert_same(u, zero, "U after a breakdown")
            assert_same(mg.get_level(L, pkg.VEC_B), b, "B after a breakdown")
            seen.append((hist, msg))
        assert np.array_equal(seen[0][0], seen[1][0]) and seen[0][1] == seen[1][1]
        # random data on the handle that broke down: six iterations of the composition (this cycle makes GCR converge slowly:
        # 36.845 -> 36.780 with the numpy hierarchies)
        st, hist, u = refine_gcr(mg, rb, ru, 0.0, 6, 4)
        assert st.cycles == 6 and np.isfinite(hist).all() and hist[-1] < hist[0], hist
        x_ref, h_ref, conv_ref, brk_ref = composition(pkg, mg, cfg, False, BILINEAR, None, rb, ru, hist, 0.0, 6, 4)
        fh, fx = used(hist, h_ref, u, x_ref)
        print(f"[refine-gcr] after a breakdown: {hist[0]:.6g} -> {hist[-1]:.6g}; used {fh:.3g} of the history bound, {fx:.3g} of the iterate bound")
        assert not brk_ref and len(h_ref) == 7 and st.converged == int(conv_ref) == 0
        assert_hist(hist, h_ref, RTOL64)
        assert np.max(np.abs(u - x_ref)) <= X_TOL64 * np.max(np.abs(x_ref))
        assert_same(mg.get_level(L, pkg.VEC_B), rb, "B after the call that followed")
        refine_gcr(mg, b, zero, 0.0, 6, 4)                  # ... and once more into the exit, directly before the other entry points
        assert "GCR breakdown at iteration 1" in last_error(pkg, mg)
        for i, (x, y) in enumerate(zip(others(mg), others(never))):
            assert np.array_equal(x[0], y[0]), (i, x[0], y[0])
            assert_same(x[1], y[1], f"U of entry point {i} after a breakdown")
            assert_same(x[2], y[2], f"B of entry point {i} after a breakdown")


def test_the_breakdown_depends_on_the_residual_not_on_the_configuration(pkg):
    """the same handle and right-hand side from a random guess: the residual is no checkerboard, nothing breaks down, and
    the six iterations are the composition's"""
    L, Lc = 6, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN, **BREAK_CFG)
    b, u0 = checkerboard(L), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg:
        st, hist, u = refine_gcr(mg, b, u0, 0.0, 6, 4)
        msg = last_error(pkg, mg)
        assert st.cycles == 6 and st.history_len == 7 and "breakdown" not in msg, (st.cycles, msg)
        assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
        x_ref, h_ref, conv_ref, brk_ref = composition(pkg, mg, cfg, False, BILINEAR, None, b, u0, hist, 0.0, 6, 4)
    fh, fx = used(hist, h_ref, u, x_ref)
    print(f"[refine-gcr] checkerboard b, random guess: {hist[0]:.6g} -> {hist[-1]:.6g}; used {fh:.3g} of the history bound, {fx:.3g} of the iterate bound")
    assert not brk_ref and len(h_ref) == 7
    assert_hist(hist, h_ref, RTOL64)
    assert np.max(np.abs(u - x_ref)) <= X_TOL64 * np.max(np.abs(x_ref))


# ---- 8. the scales: invariance under a power of two ---------------------------------------------------------------------------
# Every double operation of both loops commutes with a power of two while nothing overflows or goes subnormal (squares reach
# 2^+-320), and r / s_k is the same float for every e: the scaled call must return ldexp(u, e) and ldexp(hist, e) BIT FOR BIT.
# 2^+-160 lies beyond float's range, 2^-149 .. 2^128: a pass that skips or mis-derives a scale - the separate pass at k = 0,
# the lagged inv_scale_next - hands the float cycle zeros or infinities.  tests/test_refine_gcr_cpu.py holds both numpy
# statements to the same invariance
SCALE_CASES = {"galerkin-7-3": (7, 3, "contrast10"), "galerkin-nine-6-3": (6, 3, "rot45")}
EXPONENTS = (-160, 160)


def stats_of(st):
    return st.cycles, st.converged, st.fine_updates, st.history_len


@pytest.mark.parametrize("entry", ["solve_refine_gcr", "solve_refine"])
@pytest.mark.parametrize("name", list(SCALE_CASES))
def test_a_power_of_two_on_b_and_u_is_a_power_of_two_on_the_result_bit_for_bit(pkg, name, entry):
    L, Lc, kind = SCALE_CASES[name]
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, kind) as mg:
        def run(bb, uu, tol, k):
            return refine_gcr(mg, bb, uu, tol, k, 4) if entry == "solve_refine_gcr" else refine(mg, bb, uu, tol, k)

        for tol, k in ((0.0, 6), (1e-10, 60)):
            st, hist, u = run(b, u0, tol, k)
            assert (st.cycles == 6) if tol == 0.0 else (st.converged == 1 and 6 < st.cycles < 60), (st.cycles, hist)
            for e in EXPONENTS:
                st_e, hist_e, u_e = run(np.ldexp(b, e), np.ldexp(u0, e), tol, k)
                assert stats_of(st_e) == stats_of(st), (e, stats_of(st_e), stats_of(st))
                assert np.array_equal(hist_e, np.ldexp(hist, e)), (e, hist_e, np.ldexp(hist, e))
                assert_same(u_e, np.ldexp(u, e), f"{entry} {name} tol {tol:g} 2^{e}")
                assert np.isfinite(u_e).all() and np.all(hist_e > 0.0)


# ---- 9. small exits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [1e-8, 0.0])
def test_the_zero_problem_converges_at_once_and_divides_nothing(pkg, tol):
    """b = 0, u = 0: h0 <= tol h0 holds for every tol >= 0, one history entry 0.0, converged; the next call is a fresh handle's"""
    L, Lc = 6, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    zero = np.zeros(((1 << L) - 1,) * 2)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast10") as fresh:
        st, hist, u = refine_gcr(mg, zero, zero, tol, 5, 4)
        assert st.converged == 1 and st.cycles == 0 and st.history_len == 1 and len(hist) == 1 and hist[0] == 0.0
        assert st.initial_residual == 0.0 and st.final_residual == 0.0 and st.fine_updates == 0.0
        assert not u.any() and not mg.get_level(L, pkg.VEC_B).any() and np.isfinite(u).all()
        st1, h1, u1 = refine_gcr(mg, b, u0, 0.0, 5, 3)
        st2, h2, u2 = refine_gcr(fresh, b, u0, 0.0, 5, 3)
    assert np.array_equal(h1, h2) and stats_of(st1) == stats_of(st2)
    assert_same(u1, u2, "the call after the zero problem")


def test_null_stats_null_history_and_a_short_history_buffer(pkg):
    L, Lc = 6, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    lib = pkg.lib()
    with parent(pkg, cfg, "contrast10") as mg:
        st, hist, u = refine_gcr(mg, b, u0, 0.0, 5, 4)
        assert len(hist) == 6
        mg.set_guess(u0)
        assert lib.mgx_solve_refine_gcr(mg._h, 0.0, 5, 4, None, None, 0) == 0
        assert_same(mg.get_solution(), u, "U with stats = NULL, history = NULL")
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B with stats = NULL, history = NULL")
        mg.set_guess(u0)
        poison = -7.25
        buf = np.full(5, poison)
        st2 = pkg.Stats()
        assert lib.mgx_solve_refine_gcr(mg._h, 0.0, 5, 4, C.byref(st2), buf.ctypes.data_as(C.POINTER(C.c_double)), 2) == 0
        assert st2.history_len == 6 and st2.cycles == 5
        assert np.array_equal(buf[:2], hist[:2]) and np.all(buf[2:] == poison), buf
        assert st2.final_residual == hist[-1]
        assert_same(mg.get_solution(), u, "U with a short history buffer")
        mg.set_guess(u0)
        assert lib.mgx_solve_refine_gcr(mg._h, 0.0, 5, 4, C.byref(st2), None, 5) == 0 and st2.history_len == 6      # history = NULL with a cap
        assert_same(mg.get_solution(), u, "U with history = NULL")


def test_time_refine_gcr_pass_on_a_stencil5_handle(pkg):
    """both passes on a STENCIL5 handle (7..3: two strips): nothing moves, and the next solve is unchanged"""
    L, Lc = 7, 3
    cfg = config(pkg, L, Lc, pkg.OPERATOR_STENCIL5, mu1=2, mu2=1)
    b, u0 = rand(L, 3), rand(L, 4)
    with parent(pkg, cfg, "contrast10") as mg:
        coarse = [mg.get_level(lv, w) for lv in range(Lc, L) for w in (pkg.VEC_U, pkg.VEC_B)]
        _, hist, u = refine_gcr(mg, b, u0, 0.0, 3, 2)
        for which in (1, 0, 1):
            assert mg.time_refine_gcr_pass(which, 3) > 0.0
        assert_same(mg.get_solution(), u, "U after time_refine_gcr_pass")
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B after time_refine_gcr_pass")
        for x, y in zip(coarse, [mg.get_level(lv, w) for lv in range(Lc, L) for w in (pkg.VEC_U, pkg.VEC_B)]):
            assert_same(y, x, "a coarse level after time_refine_gcr_pass")
        _, hist2, u2 = refine_gcr(mg, b, u0, 0.0, 3, 2)
        assert_same(u2, u, "solve_refine_gcr after time_refine_gcr_pass")
        assert np.array_equal(hist2, hist)


def test_the_timing_guard_looks_at_the_buffers_not_at_which_call_made_them(pkg):
    """mgx_time_refine_gcr_pass needs the float copy and slot 0 of the basis.  mgx_solve_refine alone and mgx_solve_gcr alone
    are refused (MGX_ERR_STATE, the message names mgx_solve_refine_gcr); the two together are accepted without a
    mgx_solve_refine_gcr, as include/mgx.h says: both passes only rewrite buffers that mean nothing between two solves.
    Pinned here: accepted, U and B unchanged, and every entry point that shares those buffers is a fresh handle's afterwards"""
    L, Lc = 6, 3
    cfg = config(pkg, L, Lc, pkg.OP_GALERKIN)
    b, u0 = rand(L, 3), rand(L, 4)
    ms = C.c_double()
    lib = pkg.lib()

    def after(h):
        out = []
        for call in (lambda: h.solve_gcr(tol=0.0, max_iters=3, restart=2), lambda: h.solve_refine(tol=0.0, max_cycles=2),
                     lambda: h.solve_refine_gcr(tol=0.0, max_iters=3, restart=2), lambda: h.solve_pcg(tol=0.0, max_iters=2)):
            h.set_guess(u0)
            _, hist = call()
            out.append((hist, h.get_solution()))
        return out

    with parent(pkg, cfg, "contrast10") as mg, parent(pkg, cfg, "contrast10") as only_gcr, parent(pkg, cfg, "contrast10") as fresh:
        for h in (mg, only_gcr, fresh):
            h.set_rhs(b)
            h.set_guess(u0)
        mg.solve_refine(tol=0.0, max_cycles=2)
        assert lib.mgx_time_refine_gcr_pass(mg._h, 0, 1, C.byref(ms)) == STATE and "mgx_solve_refine_gcr first" in last_error(pkg, mg)
        only_gcr.solve_gcr(tol=0.0, max_iters=2, restart=1)
        assert lib.mgx_time_refine_gcr_pass(only_gcr._h, 1, 1, C.byref(ms)) == STATE
        mg.solve_gcr(tol=0.0, max_iters=2, restart=1)
        u = mg.get_solution()
        for which in (0, 1):
            assert mg.time_refine_gcr_pass(which, 2) > 0.0
        assert_same(mg.get_solution(), u, "U after the timing call")
        assert_same(mg.get_level(L, pkg.VEC_B), b, "B after the timing call")
        for i, (x, y) in enumerate(zip(after(mg), after(fresh))):
            assert np.array_equal(x[0], y[0]), (i, x[0], y[0])
            assert_same(x[1], y[1], f"entry point {i} after the timing call")
