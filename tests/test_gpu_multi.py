"""GPU tests of mgx_solve_multi and mgx_time_multi_smoother (include/mgx.h): up to MGX_MAX_RHS right-hand sides per
operator read on general-operator Jacobi handles.

Every comparison is np.array_equal against mgx_solve ON THE SAME HANDLE (mgx_set_rhs, mgx_set_guess, mgx_solve as a plain
cycle loop, schedule = 0), column by column: the iterate, the history, cycles, converged, history_len, both residuals
and fine_updates.  mgx_solve replays its cycle from a graph of the single-column kernels (k_small_visit in W / F cycles);
the block call launches the K-column kernels of csrc/mgx_multi.hpp eagerly - the bits must not know the difference.

Shapes: the kernels run one row per wave (rows_per_chunk = 1: no chunk heights to vary); a strip is 62 lanes = 124 columns
in fp64 and 248 in fp32.  (4, 3): 15^2 unknowns, a partial strip; (7, 3): 127 columns, a second strip that is a sliver in
fp64; (8, 4): 255 columns, three fp64 strips, two fp32 strips, more than one workgroup per strip.  Level 10 (1023^2, fp64,
four columns, 3 cycles): 2304 per-block sums per column, more than 1024 - only there does k_reduce_partials enter its
four-way unrolled loop.

A block of test 1 holds, by construction, columns with different fates: a random column from a zero guess (converges after
several cycles), a zero column (b = 0, guess 0: hist[0] = 0, frozen before the first cycle), a column whose guess is what
40 cycles left of its b (it sits at the rounding floor, cannot gain six digits and runs to max_cycles with converged = 0)
and a second random column from a random guess.  The test asserts from the returned stats that min(nrhs, 3) different
cycle counts occur: without that it could not show that freezing works.

`python tests/test_gpu_multi.py wf-child` is the child process of test 3 (MGX_SMALL_VISIT=0 is read when a handle is created)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_refine import ALLOC, BILINEAR, INVALID, OPERATOR, STATE, config, give_operator, rand  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 3), (7, 3), (8, 4)]
V, W, F = 0, 1, 2
STAT_FIELDS = ("cycles", "converged", "history_len", "initial_residual", "final_residual", "fine_updates")


def np_dtype(pkg, dtype):
    return np.float64 if dtype == pkg.DTYPE_F64 else np.float32


def handle(pkg, L, Lc, op, kind, transfer=BILINEAR, cycle=None, **kw):
    mg = pkg.Multigrid(**config(pkg, L, Lc, pkg.OPERATOR_STENCIL5 if op == "s5" else pkg.OP_GALERKIN, **kw))
    give_operator(pkg, mg, kind, L, Lc, transfer)
    if cycle is not None:
        mg.set_cycle(cycle)
    return mg


def solve_one(mg, b, u0, tol, max_cycles):
    mg.set_rhs(b)
    mg.set_guess(u0)
    st, hist = mg.solve(tol=tol, max_cycles=max_cycles)
    return st, hist, mg.get_solution()


def sequential(mg, b, u0, tol, max_cycles):
    """the reference: one mgx_solve per column on the same handle"""
    return [solve_one(mg, b[j], u0[j], tol, max_cycles) for j in range(len(b))]


def assert_column(got, want, what):
    (st, hist, u), (st0, hist0, u0) = got, want
    for f in STAT_FIELDS:
        assert getattr(st, f) == getattr(st0, f), f"{what}: {f} {getattr(st, f)!r} != {getattr(st0, f)!r}"
    assert np.array_equal(hist, hist0), f"{what}: histories differ\n{hist}\n{hist0}"
    assert u.dtype == u0.dtype and np.array_equal(u, u0), f"{what}: iterates differ in {np.count_nonzero(u != u0)} points"


def assert_block(mg, b, u0, tol, max_cycles, ref, what):
    """solve_multi on the columns of b / u0 against ref (sequential's list); returns the stats"""
    stats, hists, u = mg.solve_multi(b, u0, tol=tol, max_cycles=max_cycles)
    assert len(stats) == len(hists) == len(u) == len(b)
    for j in range(len(b)):
        assert_column((stats[j], hists[j], u[j]), ref[j], f"{what}, column {j} of {len(b)}")
    assert len({st.seconds for st in stats}) == 1 and stats[0].seconds > 0.0
    return stats


def fates(mg, L, dt, seed=3):
    """the block of the module docstring: (b, u0) of shape (4, n, n)"""
    n = (1 << L) - 1
    first = rand(L, seed)
    if dt == np.float32:
        # a float handle cannot gain six digits on a uniformly random b (measured at 127^2: 30 cycles, not converged): the
        # solution is ~N / 20 times as large as b, and the rounding floor of the residual with it.  b = A x of a random x
        # is as random, and its solution x is not larger than b
        first = -mg.residual(L, first.astype(dt), np.zeros((n, n), dtype=dt))
    b = np.stack([first, np.zeros((n, n)), rand(L, seed + 1), rand(L, seed + 2)]).astype(dt)
    u0 = np.zeros_like(b)
    u0[2] = solve_one(mg, b[2], u0[2], 0.0, 40)[2]
    u0[3] = rand(L, seed + 3).astype(dt)
    return b, u0


# ---- 1. bit for bit against mgx_solve, columns with different fates ------------------------------------------------
# (STENCIL5 with a random operator on every level: the operators carry no h^2, so the restriction whose weights sum to one,
# FW16 = 1, is the one that sizes the coarse correction; with the default the cycle diverges)
SWEEP = [("gal", "contrast10", BILINEAR, {}), ("gal", "contrast10", OPERATOR, {}), ("gal", "rot45", BILINEAR, {}), ("gal", "rot45", OPERATOR, {}),
         ("s5", "random5", BILINEAR, dict(restrict_mode=1))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("op,kind,transfer,kw", SWEEP, ids=[f"{o}-{k}-{'opdep' if t else 'bilinear'}" for o, k, t, _ in SWEEP])
def test_every_column_has_the_bits_of_mgx_solve(pkg, op, kind, transfer, kw, dtype, shape):
    L, Lc = shape
    dtype = pkg.DTYPE_F64 if dtype == "f64" else pkg.DTYPE_F32
    dt = np_dtype(pkg, dtype)
    assert pkg.RESTRICT_FW16 == 1
    with handle(pkg, L, Lc, op, kind, transfer, dtype=dtype, **kw) as mg:
        b, u0 = fates(mg, L, dt)
        ref = sequential(mg, b, u0, 1e-6, 30)
        print(f"{op} {kind} transfer {transfer} {dt.__name__} {L}..{Lc}: cycles {[r[0].cycles for r in ref]}, converged "
              f"{[r[0].converged for r in ref]}")
        for nrhs in (1, 2, 3, 4):
            stats = assert_block(mg, b[:nrhs], u0[:nrhs], 1e-6, 30, ref, f"nrhs = {nrhs}")
            counts = [st.cycles for st in stats]
            assert len(set(counts)) >= min(nrhs, 3), f"nrhs = {nrhs}: cycle counts {counts} do not show freezing"
        # the fates themselves
        assert ref[1][0].cycles == 0 and ref[1][0].converged == 1 and ref[1][1][0] == 0.0
        assert ref[2][0].cycles == 30 and ref[2][0].converged == 0
        assert 0 < ref[0][0].cycles < 30 and ref[0][0].converged == 1


def test_level_10_reduces_more_than_1024_sums_per_column(pkg):
    L, Lc = 10, 5
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg:
        b = np.stack([rand(L, 3 + j) for j in range(4)])
        u0 = np.zeros_like(b)
        u0[3] = rand(L, 9)
        ref = sequential(mg, b, u0, 0.0, 3)
        assert_block(mg, b, u0, 0.0, 3, ref, "1023^2")


# ---- 2. the grouping of the columns does not reach the bits ----------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_permuted_columns_give_permuted_results(pkg, dtype):
    L, Lc = 7, 3
    dtype = pkg.DTYPE_F64 if dtype == "f64" else pkg.DTYPE_F32
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR, dtype=dtype) as mg:
        b, u0 = fates(mg, L, np_dtype(pkg, dtype))
        s4, h4, u4 = mg.solve_multi(b, u0, tol=1e-6, max_cycles=12)
        perm = [2, 0, 3, 1]
        sp, hp, up = mg.solve_multi(b[perm], u0[perm], tol=1e-6, max_cycles=12)
        for j, src in enumerate(perm):
            assert_column((sp[j], hp[j], up[j]), (s4[src], h4[src], u4[src]), f"permuted column {j} (was {src})")
        s3, h3, u3 = mg.solve_multi(b[:3], u0[:3], tol=1e-6, max_cycles=12)
        for j in range(3):
            assert_column((s3[j], h3[j], u3[j]), (s4[j], h4[j], u4[j]), f"column {j} of three")


# ---- 3. W and F cycles: mgx_solve visits the small levels through k_small_visit ----------------------------------------
WF = [(cycle, shape, transfer) for cycle in (W, F) for shape in ((7, 3), (6, 3)) for transfer in (BILINEAR, OPERATOR)]


def check_wf(pkg, cycle, shape, transfer):
    L, Lc = shape
    with handle(pkg, L, Lc, "gal", "contrast10", transfer, cycle=cycle) as mg:
        b, u0 = fates(mg, L, np.float64)
        ref = sequential(mg, b, u0, 1e-6, 12)
        assert_block(mg, b, u0, 1e-6, 12, ref, f"cycle {cycle} on {L}..{Lc}, transfer {transfer}")


@pytest.mark.parametrize("cycle,shape,transfer", WF, ids=[f"{'WF'[c - 1]}-{s[0]}-{s[1]}-{'opdep' if t else 'bilinear'}" for c, s, t in WF])
def test_w_and_f_cycles(pkg, cycle, shape, transfer):
    check_wf(pkg, cycle, shape, transfer)


def test_w_and_f_cycles_without_the_visit_kernel():
    """the same in a fresh process whose handles are created with MGX_SMALL_VISIT=0"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "wf-child"], env=dict(os.environ, MGX_SMALL_VISIT="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wf-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- 4. injection, bottom = SMOOTH, one-level hierarchies ------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,kw", [("inject", dict(restrict_mode=2)), ("inject4", dict(restrict_mode=3)), ("bottom-smooth", dict(bottom=1)),
                                     ("inject4-bottom-smooth", dict(restrict_mode=3, bottom=1))])
def test_stencil5_injection_and_smoothed_bottom(pkg, name, kw, dtype):
    L, Lc = 7, 3
    dtype = pkg.DTYPE_F64 if dtype == "f64" else pkg.DTYPE_F32
    assert (pkg.RESTRICT_INJECT, pkg.RESTRICT_INJECT4, pkg.BOTTOM_SMOOTH) == (2, 3, 1)
    with handle(pkg, L, Lc, "s5", "contrast10", dtype=dtype, **kw) as mg:      # -div(a grad u) on every level: h^2 folded in
        b, u0 = fates(mg, L, np_dtype(pkg, dtype))
        ref = sequential(mg, b, u0, 1e-6, 8)
        print(f"{name} {dtype}: cycles {[r[0].cycles for r in ref]}, final {[float(r[1][-1]) for r in ref]}")
        assert_block(mg, b, u0, 1e-6, 8, ref, name)


@pytest.mark.parametrize("op,kind,bottom", [("s5", "random5", 0), ("gal", "contrast10", 0), ("gal", "rot45", 0), ("gal", "rot45", 1)])
def test_one_level_hierarchies_are_one_bottom_solve_per_column(pkg, op, kind, bottom):
    L = 4
    with handle(pkg, L, L, op, kind, bottom=bottom) as mg:
        b, u0 = fates(mg, L, np.float64)
        ref = sequential(mg, b, u0, 1e-6, 5)
        assert_block(mg, b, u0, 1e-6, 5, ref, f"one level, bottom {bottom}")


# ---- 5. the state of the handle ------------------------------------------------------------------------------------------
def snapshot(mg):
    L, Lc = mg.cfg.finest_level, mg.cfg.coarsest_level
    return [mg.get_level(lv, which) for lv in range(Lc, L + 1) for which in (0, 1)], mg.graphs_cached()


def test_the_handle_is_left_as_it_was(pkg):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as fresh:
        assert (pkg.VEC_U, pkg.VEC_B) == (0, 1)
        b, u0 = fates(mg, L, np.float64)
        for h in (mg, fresh):
            solve_one(h, rand(L, 11), rand(L, 12), 0.0, 3)       # every level holds something, the graphs are captured
        grids, graphs = snapshot(mg)
        assert graphs > 0
        mg.solve_multi(b, u0, tol=1e-6, max_cycles=10)
        grids1, graphs1 = snapshot(mg)
        assert graphs1 == graphs
        for a, a1 in zip(grids, grids1):
            assert np.array_equal(a, a1)
        # the handle goes on from its own U and B as one that never made the call
        (st, hist), (st0, hist0) = mg.solve(tol=0.0, max_cycles=3), fresh.solve(tol=0.0, max_cycles=3)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, fresh.get_solution()), "mgx_solve after mgx_solve_multi")


def test_block_calls_record_no_profile(pkg):
    """cfg.profile covers the handle's own cycles: a block cycle and the block smoother timing run the same level
    operations and open no scope, and the scopes of the next mgx_solve are those of a handle that never made the calls"""
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR, profile=1) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR, profile=1) as fresh:
        b = np.stack([rand(L, 3), rand(L, 4)])
        u0 = np.zeros_like(b)
        for h in (mg, fresh):
            h.set_rhs(rand(L, 11))
            h.set_guess(rand(L, 12))
        mg.solve(tol=0.0, max_cycles=2)
        p = mg.profile()
        assert all(x > 0 for x in (sum(p["launches"]), sum(p["sweeps"]), sum(p["ms"]))), p
        mg.profile_reset()
        mg.solve_multi(b, u0, tol=1e-6, max_cycles=3)
        ms = mg.time_multi_smoother(2, 4)
        assert np.isfinite(ms) and ms > 0.0
        p = mg.profile()
        assert not any(p["launches"]) and not any(p["sweeps"]) and not any(p["ms"]), p
        mg.solve(tol=0.0, max_cycles=2)
        fresh.solve(tol=0.0, max_cycles=2)
        p, p0 = mg.profile(), fresh.profile()
        assert sum(p0["launches"]) > 0
        assert p["launches"] == p0["launches"] and p["sweeps"] == p0["sweeps"], (p, p0)


def test_a_new_operator_is_followed_and_the_workspace_grows(pkg):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg:
        b, u0 = fates(mg, L, np.float64)
        ref = sequential(mg, b, u0, 1e-6, 10)
        assert_block(mg, b[:2], u0[:2], 1e-6, 10, ref, "two columns")             # allocates two columns
        assert_block(mg, b, u0, 1e-6, 10, ref, "four columns after two")          # adds two
        give_operator(pkg, mg, "rot45", L, Lc, BILINEAR)                            # nine-point finest level, other transfer
        ref9 = sequential(mg, b, u0, 1e-6, 10)
        assert not np.array_equal(ref9[0][2], ref[0][2])
        assert_block(mg, b, u0, 1e-6, 10, ref9, "after set_tensor and a rebuild")
        from pcg_ref import contrast_coefficient
        mg.set_coefficient(contrast_coefficient(L, 100.0))
        mg.build_galerkin(OPERATOR)
        ref100 = sequential(mg, b, u0, 1e-6, 10)
        assert_block(mg, b, u0, 1e-6, 10, ref100, "after set_coefficient and a rebuild")


def test_a_short_history_slot_is_not_overrun(pkg):
    L, Lc, cap = 6, 3, 3
    with handle(pkg, L, Lc, "gal", "contrast10") as mg:
        b, u0 = fates(mg, L, np.float64)
        ref = sequential(mg, b, u0, 1e-6, 10)
        u = u0.copy()
        stats = (pkg.Stats * 4)()
        flat = np.full(4 * cap + 5, -7.0)                          # column j starts at flat + j * cap; five doubles of margin
        rc = pkg.lib().mgx_solve_multi(mg._h, 4, b.ctypes.data, u.ctypes.data, 1e-6, 10, stats, flat.ctypes.data_as(C.POINTER(C.c_double)), cap)
        assert rc == 0
        for j in range(4):
            want = ref[j][1]
            k = min(cap, len(want))
            assert stats[j].history_len == len(want)
            assert np.array_equal(flat[j * cap: j * cap + k], want[:k])
            assert np.all(flat[j * cap + k: (j + 1) * cap] == -7.0), f"column {j} wrote past its history"
            assert np.array_equal(u[j], ref[j][2])
        assert np.all(flat[4 * cap:] == -7.0)


def test_no_cycles_returns_the_guesses(pkg):
    L, Lc = 6, 3
    with handle(pkg, L, Lc, "gal", "contrast10") as mg:
        b, u0 = fates(mg, L, np.float64)
        ref = sequential(mg, b, u0, 1e-6, 0)
        stats = assert_block(mg, b, u0, 1e-6, 0, ref, "max_cycles = 0")
        assert [st.history_len for st in stats] == [1, 1, 1, 1]


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def raw_multi(pkg, mg, nrhs=2, b=True, u=True, tol=1e-8, max_cycles=2):
    n = mg.n()
    dt = mg.level_dtype(mg.cfg.finest_level)
    bb, uu = np.ones((max(nrhs, 1), n, n), dtype=dt), np.zeros((max(nrhs, 1), n, n), dtype=dt)
    rc = pkg.lib().mgx_solve_multi(mg._h, nrhs, bb.ctypes.data if b else None, uu.ctypes.data if u else None, tol, max_cycles, None, None, 0)
    return rc, pkg.lib().mgx_last_error(mg._h).decode()


def raw_time(pkg, mg, nrhs=1, sweeps=2):
    ms = C.c_double(-1.0)
    rc = pkg.lib().mgx_time_multi_smoother(mg._h, nrhs, sweeps, C.byref(ms))
    return rc, pkg.lib().mgx_last_error(mg._h).decode(), ms.value


def refused(pkg, mg, L, status, word=None, dt=np.float64, **kw):
    """the call is refused with `status` and a reason; the handle solves to the same bits before and after"""
    b = rand(L, 5).astype(dt)
    before = solve_one(mg, b, np.zeros_like(b), 0.0, 2)
    rc, msg = raw_multi(pkg, mg, **kw)
    assert rc == status and msg and (word is None or word in msg), (rc, msg)
    if status == STATE:
        rc, msg, _ = raw_time(pkg, mg)
        assert rc == STATE and msg, (rc, msg)
    assert_column(solve_one(mg, b, np.zeros_like(b), 0.0, 2), before, "mgx_solve after the refusal")


def test_poisson_and_mixed_handles_are_refused_with_the_reason(pkg):
    L, Lc = 6, 3
    base = dict(finest_level=L, coarsest_level=Lc, mu1=2, mu2=2, schedule=0)
    with pkg.Multigrid(**base) as mg:
        refused(pkg, mg, L, STATE, "POISSON")
    with pkg.Multigrid(dtype=pkg.DTYPE_MIXED, **base) as mg:
        refused(pkg, mg, L, STATE)


@pytest.mark.parametrize("kind", ["n_gpus", "rank"])
def test_multi_gpu_and_rank_handles_are_refused_with_the_reason(pkg, kind):
    """(the rank case spends its seconds in ncclCommInitRank: a rank handle cannot be created without it)"""
    kw = dict(finest_level=9, coarsest_level=6, mu1=2, mu2=2, schedule=0, cut_level=7)
    mg = pkg.Multigrid(n_gpus=2, devices=[0, 0], **kw) if kind == "n_gpus" else pkg.Multigrid.rank(0, 1, rccl_id=pkg.rccl_unique_id(), **kw)
    with mg:
        refused(pkg, mg, 9, STATE, "multi-GPU")


@pytest.mark.parametrize("smoother", [2, 4, 5, 6, 8, 9])
def test_other_smoothers_are_refused_as_a_follow_up(pkg, smoother):
    L, Lc = 6, 3
    assert (pkg.SMOOTHER_CHEBYSHEV, pkg.SMOOTHER_LINE_X, pkg.SMOOTHER_LINE_Y, pkg.SMOOTHER_LINE_ALT, pkg.SMOOTHER_COLOR_GS,
            pkg.SMOOTHER_COLOR_SGS) == (2, 4, 5, 6, 8, 9)
    with handle(pkg, L, Lc, "gal", "contrast10", smoother=smoother) as mg:
        refused(pkg, mg, L, STATE, "follow-up")


def test_unbuilt_hierarchies_and_bad_arguments_are_refused(pkg):
    L, Lc = 6, 3
    from pcg_ref import contrast_coefficient
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OP_GALERKIN)) as mg:
        rc, msg = raw_multi(pkg, mg)
        assert rc == STATE and "not set" in msg, msg
        mg.set_coefficient(contrast_coefficient(L, 10.0))
        rc, msg = raw_multi(pkg, mg)
        assert rc == STATE and "not built" in msg, msg
        assert raw_time(pkg, mg)[0] == STATE
        mg.build_galerkin()
        for kw in (dict(nrhs=0), dict(nrhs=-1), dict(nrhs=pkg.MAX_RHS + 1), dict(b=False), dict(u=False), dict(tol=float("nan")),
                   dict(tol=-1.0), dict(max_cycles=-1)):
            refused(pkg, mg, L, INVALID, **kw)
        b, u0 = fates(mg, L, np.float64)
        assert_block(mg, b, u0, 1e-6, 10, sequential(mg, b, u0, 1e-6, 10), "after the refusals")
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OPERATOR_STENCIL5)) as mg:
        rc, msg = raw_multi(pkg, mg)
        assert rc == STATE and "not set" in msg, msg


# ---- 7. mgx_time_multi_smoother ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contrast10", "rot45"])
def test_time_multi_smoother(pkg, kind):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", kind) as mg:
        b, u0 = fates(mg, L, np.float64)
        solve_one(mg, rand(L, 11), rand(L, 12), 0.0, 2)
        rc, msg, _ = raw_time(pkg, mg)
        assert rc == STATE and "mgx_solve_multi" in msg, msg
        first = mg.solve_multi(b[:2], u0[:2], tol=1e-6, max_cycles=10)
        assert raw_time(pkg, mg, nrhs=3)[0] == STATE                # two columns exist
        full = mg.solve_multi(b, u0, tol=1e-6, max_cycles=10)
        grids, graphs = snapshot(mg)
        for nrhs in (1, 2, 3, 4):
            for sweeps in (1, 4):
                ms = mg.time_multi_smoother(nrhs, sweeps)
                assert np.isfinite(ms) and ms > 0.0, (nrhs, sweeps, ms)
        for bad in (dict(nrhs=0), dict(nrhs=5), dict(sweeps=0)):
            rc, msg, _ = raw_time(pkg, mg, **bad)
            assert rc == INVALID and msg
        grids1, graphs1 = snapshot(mg)
        assert graphs1 == graphs and all(np.array_equal(a, a1) for a, a1 in zip(grids, grids1))
        again = mg.solve_multi(b, u0, tol=1e-6, max_cycles=10)
        for j in range(4):
            assert_column((again[0][j], again[1][j], again[2][j]), (full[0][j], full[1][j], full[2][j]), f"column {j} after the timing")
        for j in range(2):
            assert_column((first[0][j], first[1][j], first[2][j]), (full[0][j], full[1][j], full[2][j]), f"column {j} of two")


if __name__ == "__main__":
    assert sys.argv[1:] == ["wf-child"] and os.environ.get("MGX_SMALL_VISIT") == "0"
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    package = ge.load_package()
    for case in WF:
        check_wf(package, *case)
    print("wf-child ok")
