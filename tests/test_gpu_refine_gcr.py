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
tol 0 (slots 0 .. 3 and a wrap); deep bases: restart 8, nine iterations (slots 0 .. 7 and a wrap)."""
import ctypes as C

import numpy as np
import pytest

import refine_gcr_ref as rg
from pcg_ref import contrast_coefficient
from test_gpu_galerkin import assert_same
from test_gpu_pcg import RTOL64, assert_hist
from test_gpu_refine import (BILINEAR, CASES as REFINE_CASES, INVALID, OPERATOR, STATE, config, give_operator, parent, rand, read_operator,
                             write_operator)
from test_refine_gcr_cpu import NINE_FIVE, TRUE_GAP

pytestmark = pytest.mark.gpu

X_TOL64 = 1e-9                                  # tests/test_gpu_gcr.py's bound on the fp64 iterate


@pytest.fixture(autouse=True)
def default_chunk_height(monkeypatch):
    monkeypatch.delenv("MGX_ROWS", raising=False)       # device_dot(rows_per_chunk = 0) is make_launch's own choice


def refine_gcr(mg, b, u0, tol, max_iters, restart):
    mg.set_rhs(b)
    mg.set_guess(u0)
    st, hist = mg.solve_refine_gcr(tol=tol, max_iters=max_iters, restart=restart)
    return st, hist, mg.get_solution()


def composition(pkg, mg, cfg, nine, transfer, cycle, b, u0, hist, tol, max_iters, restart):
    """refine_gcr_ref's loop over two independent handles, the scales from `hist`, the dots in the device's order:
    (x, history, converged, breakdown)"""
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

        return rg.refine_gcr(A, cycle32, b, u0, tol, max_iters, restart, history=hist, dot=rg.device_dot)


def used(h, h_ref, u, x_ref):
    """the fractions of the history and the iterate bound that a result uses"""
    k = min(len(h), len(h_ref))
    return (float(np.max(np.abs(h[:k] - h_ref[:k]) / (RTOL64 * h_ref[:k] + 1e-14 * h_ref[0]))),
            float(np.max(np.abs(u - x_ref)) / np.max(np.abs(x_ref)) / X_TOL64))


def check_parity(pkg, name, case, tol, iters, restart, floor=None):
    L, Lc, op, extra, kind, nine, transfer, cycle, guess = case
    cfg = config(pkg, L, Lc, pkg.OPERATOR_STENCIL5 if op == "s5" else pkg.OP_GALERKIN, **extra)
    b = rand(L, 3)
    u0 = rand(L, 4) if guess else np.zeros_like(b)
    with parent(pkg, cfg, kind, transfer, cycle) as mg:
        st, hist, u = refine_gcr(mg, b, u0, tol, iters, restart)
        assert np.isfinite(hist).all() and hist[-1] < hist[0], hist
        x_ref, h_ref, conv_ref, brk_ref = composition(pkg, mg, cfg, nine, transfer, cycle, b, u0, hist, tol, iters, restart)
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
