"""GPU tests of mgx_solve_multi_gcr and mgx_time_multi_gcr_direction (include/mgx.h): restarted GCR on up to MGX_MAX_RHS
right-hand sides per operator read, on general-operator Jacobi handles.

Every comparison is np.array_equal / == against mgx_solve_gcr ON THE SAME HANDLE (mgx_set_rhs, mgx_set_guess,
mgx_solve_gcr, mgx_get_solution), column by column: the iterate, the history, cycles, converged, history_len, both
residuals and fine_updates.  mgx_solve_gcr replays its cycle from a graph of the single-column kernels (k_small_visit in
W / F cycles) and runs k_pcg_direction; the block call launches the K-column kernels of csrc/mgx_multi.hpp eagerly,
k_gcr_direction_multi among them, and the coefficient-free Krylov passes once per column on that column's own scalars
and partial sums - the bits must not know the difference.

Shapes: a wave of the Krylov passes covers 62 lanes = 124 columns in fp64 and 248 in fp32 and marches down R rows per
chunk, R = clamp(rows / 128, 4, 8) = 4 at every size here unless MGX_ROWS says otherwise.  (4, 3): 15^2 unknowns, a partial
strip; (7, 3): 127 columns, a second strip that is a sliver in fp64; (8, 4): 255 columns, three fp64 strips, several
workgroups per strip.  Test 3 runs chunks of 5 rows on 127 rows (not a multiple: the last chunk is short) in a child
process: MGX_ROWS is read when a handle is created.

A block of test 1 holds columns with different fates, in this order: a random column from a zero guess (converges after
five to nine iterations), a zero column (b = 0, guess 0: hist[0] = 0, never active), a random column from a random guess
whose b and guess are scaled to the edge of the number format, and a column whose guess is what 40 mgx_solve_gcr
iterations left of its b.  The recursively updated residual of GCR has no rounding floor, so the last column converges
like a fresh one, and every well-scaled right-hand side takes the same five or six iterations on the rotated and the
random operators (measured on an MI355X: nine kinds of b, smooth, rough, a point source, agree to one iteration).  What
does end a column elsewhere is underflow, hence the scaling of the third column: in fp64 by 1e-161, where the squares
of the dots leave the double range after two to five iterations (||r||^2 = 0, or q'.q' = 0: a breakdown of this column
while the others continue); in fp32 by 1e-42, denormal floats whose residual stagnates at a few units of 1.4e-45, so the
column runs on for 8 to 12 iterations and ends with converged = 0.  Measured for every case of test 1 and both restarts,
its count differs from the first column's and from zero.  The test asserts from the sequential reference's stats that
min(nrhs, 3) different iteration counts occur: without that it could not show that freezing works.

`python tests/test_gpu_multi_gcr.py rows-child` is the child process of test 3."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_multi import F, SHAPES, W, assert_column, handle, np_dtype
from test_gpu_refine import BILINEAR, INVALID, OPERATOR, STATE, config, give_operator, rand

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, ITERS = 1e-6, 12


def gcr_one(mg, b, u0, tol, max_iters, restart):
    mg.set_rhs(b)
    mg.set_guess(u0)
    st, hist = mg.solve_gcr(tol=tol, max_iters=max_iters, restart=restart)
    return st, hist, mg.get_solution()


def sequential(mg, b, u0, tol, max_iters, restart):
    """the reference: one mgx_solve_gcr per column on the same handle"""
    return [gcr_one(mg, b[j], u0[j], tol, max_iters, restart) for j in range(len(b))]


def block(mg, b, u0, tol, max_iters, restart):
    stats, hists, u = mg.solve_multi_gcr(b, u0, tol=tol, max_iters=max_iters, restart=restart)
    assert len(stats) == len(hists) == len(u) == len(b)
    return [(stats[j], hists[j], u[j]) for j in range(len(b))]


def assert_block(mg, b, u0, tol, max_iters, restart, ref, what):
    """solve_multi_gcr on the columns of b / u0 against ref (sequential's list); returns the columns"""
    got = block(mg, b, u0, tol, max_iters, restart)
    for j in range(len(b)):
        assert_column(got[j], ref[j], f"{what}, column {j} of {len(b)}")
    assert len({g[0].seconds for g in got}) == 1 and got[0][0].seconds > 0.0
    return got


def fates(mg, L, dt, seed=3):
    """the block of the module docstring: (b, u0) of shape (4, n, n)"""
    n = (1 << L) - 1
    first = rand(L, seed)
    if dt == np.float32:
        # a float handle cannot gain six digits on a uniformly random b (the solution is ~N / 20 times as large as b, and
        # the rounding floor of the residual with it): b = A x of a random x is as random, and x is not larger than b
        first = -mg.residual(L, first.astype(dt), np.zeros((n, n), dtype=dt))
    tiny = 1e-161 if dt == np.float64 else 1e-42                   # (the module docstring)
    b = np.stack([first, np.zeros((n, n)), rand(L, seed + 1) * tiny, rand(L, seed + 2)]).astype(dt)
    u0 = np.zeros_like(b)
    u0[2] = (rand(L, seed + 3) * tiny).astype(dt)
    u0[3] = gcr_one(mg, b[3], u0[3], 0.0, 40, 4)[2]
    return b, u0


# ---- 1. bit for bit against mgx_solve_gcr, columns with different fates ----------------------------------------------
# (STENCIL5 with a random operator on every level: the operators carry no h^2, so the restriction whose weights sum to one,
# FW16 = 1, is the one that sizes the coarse correction)
SWEEP = [("gal", "contrast10", BILINEAR, {}), ("gal", "contrast10", OPERATOR, {}), ("gal", "rot45", BILINEAR, {}), ("gal", "rot45", OPERATOR, {}),
         ("s5", "random5", BILINEAR, dict(restrict_mode=1))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("op,kind,transfer,kw", SWEEP, ids=[f"{o}-{k}-{'opdep' if t else 'bilinear'}" for o, k, t, _ in SWEEP])
def test_every_column_has_the_bits_of_mgx_solve_gcr(pkg, op, kind, transfer, kw, dtype, shape):
    """restart 3 with 12 iterations crosses the restart boundary several times and fills slots 0..2; restart 1 empties the
    basis every iteration (k_gcr_orth<0> alone)"""
    L, Lc = shape
    dtype = pkg.DTYPE_F64 if dtype == "f64" else pkg.DTYPE_F32
    dt = np_dtype(pkg, dtype)
    assert pkg.RESTRICT_FW16 == 1
    with handle(pkg, L, Lc, op, kind, transfer, dtype=dtype, **kw) as mg:
        b, u0 = fates(mg, L, dt)
        for restart in (1, 3):
            ref = sequential(mg, b, u0, TOL, ITERS, restart)
            counts = [r[0].cycles for r in ref]
            print(f"{op} {kind} transfer {transfer} {dt.__name__} {L}..{Lc} restart {restart}: iterations {counts}, converged "
                  f"{[r[0].converged for r in ref]}")
            for nrhs in (1, 2, 3, 4):
                assert len(set(counts[:nrhs])) >= min(nrhs, 3), f"nrhs = {nrhs}: iteration counts {counts[:nrhs]} do not show freezing"
                assert_block(mg, b[:nrhs], u0[:nrhs], TOL, ITERS, restart, ref, f"restart {restart}, nrhs = {nrhs}")
            # the fates themselves
            assert ref[1][0].cycles == 0 and ref[1][0].converged == 1 and ref[1][0].history_len == 1 and ref[1][1][0] == 0.0
            assert 0 < ref[0][0].cycles < ITERS and ref[0][0].converged == 1
            assert 0 < ref[3][0].cycles < ITERS and ref[3][0].converged == 1


# ---- 2. a deep basis: k_gcr_dots<7> / k_gcr_orth<7> per column, with per-column scalars ---------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_deep_basis(pkg, dtype):
    L, Lc = 7, 3
    dtype = pkg.DTYPE_F64 if dtype == "f64" else pkg.DTYPE_F32
    assert pkg.GCR_MAX_RESTART == 8
    with handle(pkg, L, Lc, "gal", "rot45", OPERATOR, dtype=dtype) as mg:
        dt = np_dtype(pkg, dtype)
        b = np.stack([rand(L, 20 + j) for j in range(4)]).astype(dt)
        u0 = np.zeros_like(b)
        u0[3] = rand(L, 29).astype(dt)
        ref = sequential(mg, b, u0, 0.0, 9, 8)
        assert [r[0].cycles for r in ref] == [9, 9, 9, 9]              # slots 0 .. 7, then slot 0 of the second restart cycle
        assert_block(mg, b, u0, 0.0, 9, 8, ref, "restart 8")


# ---- 3. chunk seams of the direction kernel ------------------------------------------------------------------------------
def check_rows(pkg):
    L, Lc = 7, 3
    for kind in ("contrast10", "rot45"):                             # a five- and a nine-point finest level
        with handle(pkg, L, Lc, "gal", kind, OPERATOR) as mg:
            b, u0 = fates(mg, L, np.float64)
            ref = sequential(mg, b, u0, TOL, ITERS, 3)
            assert_block(mg, b, u0, TOL, ITERS, 3, ref, f"MGX_ROWS=5, {kind}")


def test_chunks_of_five_rows_on_127():
    """a fresh process whose handles are created with MGX_ROWS=5: 127 rows are 25 chunks of five and one of two"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "rows-child"], env=dict(os.environ, MGX_ROWS="5"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rows-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- 4. the grouping of the columns does not reach the bits --------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_permuted_columns_give_permuted_results(pkg, dtype):
    L, Lc = 7, 3
    dtype = pkg.DTYPE_F64 if dtype == "f64" else pkg.DTYPE_F32
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR, dtype=dtype) as mg:
        b, u0 = fates(mg, L, np_dtype(pkg, dtype))
        four = block(mg, b, u0, TOL, ITERS, 3)
        perm = [2, 0, 3, 1]
        got = block(mg, b[perm], u0[perm], TOL, ITERS, 3)
        for j, src in enumerate(perm):
            assert_column(got[j], four[src], f"permuted column {j} (was {src})")
        three = block(mg, b[:3], u0[:3], TOL, ITERS, 3)
        for j in range(3):
            assert_column(three[j], four[j], f"column {j} of three")


# ---- 5. W and F cycles: mgx_solve_gcr visits the small levels through k_small_visit, the block call does not ----------------
@pytest.mark.parametrize("cycle", [W, F], ids=["W", "F"])
@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR], ids=["bilinear", "opdep"])
def test_w_and_f_cycles(pkg, cycle, transfer):
    L, Lc = 6, 3
    with handle(pkg, L, Lc, "gal", "contrast10", transfer, cycle=cycle) as mg:
        b, u0 = fates(mg, L, np.float64)
        ref = sequential(mg, b, u0, TOL, ITERS, 3)
        assert_block(mg, b, u0, TOL, ITERS, 3, ref, f"cycle {cycle}, transfer {transfer}")


# ---- 6. breakdown ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_breakdown_of_every_column_and_the_calls_after_it(pkg, dtype):
    """GALERKIN 7..4 with mu1 = mu2 = 0 and bottom = SMOOTH (the construction of test_gpu_gcr.py's breakdown test): the cycle
    from zero returns exactly zero, so z = 0, q' = A z = 0 and q'.q' = 0 at iteration 1 in every column with a residual.
    A breakdown of one column while others continue has no natural input (it needs q' = 0 in one column after the same
    cycle gave the others a direction): the per-column flag handling is read in the driver.  The underflow column of test 1
    enters it in some of its cases (converged = 0 after fewer than max_iters iterations), by measurement, not by design."""
    L, Lc = 7, 4
    dtype = pkg.DTYPE_F64 if dtype == "f64" else pkg.DTYPE_F32
    dt = np_dtype(pkg, dtype)
    kw = dict(mu1=0, mu2=0, bottom=1, dtype=dtype)
    assert pkg.BOTTOM_SMOOTH == 1
    with handle(pkg, L, Lc, "gal", "contrast10", **kw) as mg, handle(pkg, L, Lc, "gal", "contrast10", **kw) as fresh:
        b = np.stack([rand(L, 30 + j) for j in range(4)]).astype(dt)
        u0 = np.zeros_like(b)
        u0[1] = rand(L, 39).astype(dt)
        ref = sequential(fresh, b, u0, TOL, ITERS, 3)
        assert "GCR breakdown at iteration 1" in pkg.lib().mgx_last_error(fresh._h).decode()
        for _ in range(2):                                           # the second call: from the flags and scalars of the first
            got = assert_block(mg, b, u0, TOL, ITERS, 3, ref, "breakdown")       # MGX_OK: anything else raises
            msg = pkg.lib().mgx_last_error(mg._h).decode()
            assert "GCR breakdown at iteration 1" in msg and "column 0" in msg and "q'.q'" in msg, msg
            for j, (st, hist, u) in enumerate(got):
                assert st.converged == 0 and st.cycles == 0 and st.history_len == 1 and len(hist) == 1
                assert np.array_equal(u, u0[j]), f"column {j} is not its guess"
        m, m0 = mg.solve_multi(b, u0, tol=TOL, max_cycles=2), fresh.solve_multi(b, u0, tol=TOL, max_cycles=2)
        for j in range(4):
            assert_column((m[0][j], m[1][j], m[2][j]), (m0[0][j], m0[1][j], m0[2][j]), f"mgx_solve_multi after the breakdown, column {j}")
        assert_column(gcr_one(mg, b[0], u0[0], TOL, ITERS, 3), gcr_one(fresh, b[0], u0[0], TOL, ITERS, 3), "mgx_solve_gcr after the breakdown")


# ---- 7. the state of the handle --------------------------------------------------------------------------------------------
def snapshot(pkg, mg):
    """U, B, R of the finest and one coarse level, and the number of cached graphs"""
    L = mg.cfg.finest_level
    return [mg.get_level(lv, which) for lv in (L, L - 1) for which in (pkg.VEC_U, pkg.VEC_B, pkg.VEC_R)], mg.graphs_cached()


def test_the_handle_is_left_as_it_was(pkg):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as twin:
        for h in (mg, twin):
            # the same calls on both: every level holds something, the graphs of both cycle kinds are captured, the Krylov
            # workspace exists
            b, u0 = fates(h, L, np.float64)
            solve_one(h, rand(L, 11), rand(L, 12), 0.0, 3)
            gcr_one(h, b[0], u0[3], 0.0, 3, 2)
        grids, graphs = snapshot(pkg, mg)
        assert graphs > 0
        block(mg, b, u0, TOL, ITERS, 3)
        grids1, graphs1 = snapshot(pkg, mg)
        assert graphs1 == graphs
        for a, a1 in zip(grids, grids1):
            assert np.array_equal(a, a1)
        grids0, graphs0 = snapshot(pkg, twin)
        assert graphs0 == graphs and all(np.array_equal(a, a0) for a, a0 in zip(grids, grids0))
        # the handle goes on from its own U and B as one that never made the call
        (st, hist), (st0, hist0) = mg.solve(tol=0.0, max_cycles=3), twin.solve(tol=0.0, max_cycles=3)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, twin.get_solution()), "mgx_solve after mgx_solve_multi_gcr")
        (st, hist), (st0, hist0) = mg.solve_gcr(tol=0.0, max_iters=4, restart=4), twin.solve_gcr(tol=0.0, max_iters=4, restart=4)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, twin.get_solution()), "mgx_solve_gcr after mgx_solve_multi_gcr")
        m, m0 = mg.solve_multi(b, u0, tol=TOL, max_cycles=6), twin.solve_multi(b, u0, tol=TOL, max_cycles=6)
        for j in range(4):
            assert_column((m[0][j], m[1][j], m[2][j]), (m0[0][j], m0[1][j], m0[2][j]), f"mgx_solve_multi after mgx_solve_multi_gcr, column {j}")


def test_a_new_operator_is_followed_and_the_workspace_grows(pkg):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as big:
        b, u0 = fates(mg, L, np.float64)
        ref2 = sequential(mg, b, u0, TOL, ITERS, 2)
        ref4 = sequential(mg, b, u0, TOL, ITERS, 4)
        assert_block(mg, b[:2], u0[:2], TOL, ITERS, 2, ref2, "two columns, restart 2")       # allocates 2 columns of 2 pairs
        grown = assert_block(mg, b, u0, TOL, ITERS, 4, ref4, "four columns, restart 4, after 2 / 2")
        started = block(big, b, u0, TOL, ITERS, 4)                                        # a handle that starts at 4 / 4
        for j in range(4):
            assert_column(grown[j], started[j], f"grown against started at 4 / 4, column {j}")
        assert_block(mg, b[:2], u0[:2], TOL, ITERS, 2, ref2, "two columns, restart 2, in the larger workspace")
        give_operator(pkg, mg, "rot45", L, Lc, BILINEAR)                # nine-point finest level, other transfer
        ref9 = sequential(mg, b, u0, TOL, ITERS, 4)
        assert not np.array_equal(ref9[0][2], ref4[0][2])
        assert_block(mg, b, u0, TOL, ITERS, 4, ref9, "after set_tensor and a rebuild")
        from pcg_ref import contrast_coefficient
        mg.set_coefficient(contrast_coefficient(L, 100.0))
        mg.build_galerkin(OPERATOR)
        assert_block(mg, b, u0, TOL, ITERS, 4, sequential(mg, b, u0, TOL, ITERS, 4), "after set_coefficient and a rebuild")


def test_the_three_gcr_users_interleaved_on_one_handle(pkg):
    """mgx_solve_gcr, mgx_solve_multi_gcr and mgx_solve_refine_gcr run the same passes on views of two workspaces (the
    handle's own, the columns'): no call may see the scalars, partial sums or basis slots another one left, in either
    workspace.  Every call on the one handle against the same call on a fresh handle; the bases grow between the calls
    (restart 2, then 4 in the handle's workspace; 4, then 2 on three, then two columns).  63^2: more than one workgroup per
    pass, three levels"""
    L, Lc, iters = 6, 3, 6
    b, u0 = np.stack([rand(L, 50 + j) for j in range(3)]), np.stack([rand(L, 60 + j) for j in range(3)])
    new = lambda: handle(pkg, L, Lc, "gal", "contrast10")

    def single(solve):
        def call(mg):
            mg.set_rhs(b[0])
            mg.set_guess(u0[0])
            st, hist = solve(mg)
            u = mg.get_solution()
            # U = the iterate, B = the caller's b again
            assert np.array_equal(mg.get_level(L, pkg.VEC_U), u) and np.array_equal(mg.get_level(L, pkg.VEC_B), b[0])
            return [(st, hist, u)]
        return call

    def multi(nrhs, restart):
        def call(mg):
            before = mg.get_level(L, pkg.VEC_U), mg.get_level(L, pkg.VEC_B)
            got = block(mg, b[:nrhs], u0[:nrhs], 0.0, iters, restart)
            # U and B are left as they were
            assert np.array_equal(mg.get_level(L, pkg.VEC_U), before[0]) and np.array_equal(mg.get_level(L, pkg.VEC_B), before[1])
            return got
        return call

    calls = [("solve_gcr(restart=2)", single(lambda mg: mg.solve_gcr(tol=0.0, max_iters=iters, restart=2))),
             ("solve_multi_gcr(3 columns, restart=4)", multi(3, 4)),
             ("solve_refine_gcr(restart=3)", single(lambda mg: mg.solve_refine_gcr(tol=0.0, max_iters=iters, restart=3))),
             ("solve_gcr(restart=4)", single(lambda mg: mg.solve_gcr(tol=0.0, max_iters=iters, restart=4))),
             ("solve_multi_gcr(2 columns, restart=2)", multi(2, 2))]
    with new() as mg:
        for what, call in calls:
            got = call(mg)
            with new() as fresh:
                want = call(fresh)
            assert len(got) == len(want)
            for j, (g, w) in enumerate(zip(got, want)):
                assert g[0].cycles == iters, (what, j, g[0].cycles)
                assert_column(g, w, f"{what} on the long-lived handle, column {j}")


# ---- 8. bounds -------------------------------------------------------------------------------------------------------------
def test_a_short_history_slot_is_not_overrun(pkg):
    L, Lc, cap = 6, 3, 3
    with handle(pkg, L, Lc, "gal", "contrast10") as mg:
        b, u0 = fates(mg, L, np.float64)
        ref = sequential(mg, b, u0, TOL, ITERS, 3)
        u = u0.copy()
        stats = (pkg.Stats * 4)()
        flat = np.full(4 * cap + 5, -7.0)                          # column j starts at flat + j * cap; five doubles of margin
        rc = pkg.lib().mgx_solve_multi_gcr(mg._h, 4, b.ctypes.data, u.ctypes.data, TOL, ITERS, 3, stats, flat.ctypes.data_as(C.POINTER(C.c_double)),
                                           cap)
        assert rc == 0
        for j in range(4):
            want = ref[j][1]
            k = min(cap, len(want))
            assert stats[j].history_len == len(want)
            assert np.array_equal(flat[j * cap: j * cap + k], want[:k])
            assert np.all(flat[j * cap + k: (j + 1) * cap] == -7.0), f"column {j} wrote past its history"
            assert np.array_equal(u[j], ref[j][2])
        assert np.all(flat[4 * cap:] == -7.0)


def test_no_iterations_returns_the_guesses(pkg):
    L, Lc = 6, 3
    with handle(pkg, L, Lc, "gal", "contrast10") as mg:
        b, u0 = fates(mg, L, np.float64)
        ref = sequential(mg, b, u0, TOL, 0, 3)
        got = assert_block(mg, b, u0, TOL, 0, 3, ref, "max_iters = 0")
        assert [g[0].history_len for g in got] == [1, 1, 1, 1]
        assert all(np.array_equal(g[2], u0[j]) for j, g in enumerate(got))


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def raw_multi_gcr(pkg, mg, nrhs=2, b=True, u=True, tol=1e-8, max_iters=2, restart=2):
    n = mg.n()
    dt = mg.level_dtype(mg.cfg.finest_level)
    bb, uu = np.ones((max(nrhs, 1), n, n), dtype=dt), np.zeros((max(nrhs, 1), n, n), dtype=dt)
    rc = pkg.lib().mgx_solve_multi_gcr(mg._h, nrhs, bb.ctypes.data if b else None, uu.ctypes.data if u else None, tol, max_iters, restart, None,
                                       None, 0)
    return rc, pkg.lib().mgx_last_error(mg._h).decode()


def raw_time(pkg, mg, nrhs=1, repeats=2):
    ms = C.c_double(-1.0)
    rc = pkg.lib().mgx_time_multi_gcr_direction(mg._h, nrhs, repeats, C.byref(ms))
    return rc, pkg.lib().mgx_last_error(mg._h).decode(), ms.value


def solve_one(mg, b, u0, tol, max_cycles):
    mg.set_rhs(b)
    mg.set_guess(u0)
    st, hist = mg.solve(tol=tol, max_cycles=max_cycles)
    return st, hist, mg.get_solution()


def refused(pkg, mg, L, status, word=None, dt=np.float64, **kw):
    """the call is refused with `status` and a reason; the handle solves to the same bits before and after"""
    b = rand(L, 5).astype(dt)
    before = solve_one(mg, b, np.zeros_like(b), 0.0, 2)
    rc, msg = raw_multi_gcr(pkg, mg, **kw)
    assert rc == status and msg and "mgx_solve_multi_gcr" in msg and (word is None or word in msg), (rc, msg)
    if status == STATE:
        rc, msg, _ = raw_time(pkg, mg)
        assert rc == STATE and msg, (rc, msg)
    assert_column(solve_one(mg, b, np.zeros_like(b), 0.0, 2), before, "mgx_solve after the refusal")


def test_poisson_mixed_and_multi_gpu_handles_are_refused_with_the_reason(pkg):
    L, Lc = 6, 3
    base = dict(finest_level=L, coarsest_level=Lc, mu1=2, mu2=2, schedule=0)
    with pkg.Multigrid(**base) as mg:
        refused(pkg, mg, L, STATE, "POISSON")
    with pkg.Multigrid(dtype=pkg.DTYPE_MIXED, **base) as mg:
        refused(pkg, mg, L, STATE)
    with pkg.Multigrid(n_gpus=2, devices=[0, 0], finest_level=9, coarsest_level=6, mu1=2, mu2=2, schedule=0, cut_level=7) as mg:
        refused(pkg, mg, 9, STATE, "multi-GPU")


@pytest.mark.parametrize("smoother", [2, 4, 5, 6, 8, 9])
def test_other_smoothers_are_refused(pkg, smoother):
    L, Lc = 6, 3
    with handle(pkg, L, Lc, "gal", "contrast10", smoother=smoother) as mg:
        refused(pkg, mg, L, STATE, "MGX_SMOOTHER_JACOBI only")


def test_unbuilt_hierarchies_and_bad_arguments_are_refused(pkg):
    L, Lc = 6, 3
    from pcg_ref import contrast_coefficient
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OP_GALERKIN)) as mg:
        rc, msg = raw_multi_gcr(pkg, mg)
        assert rc == STATE and "not set" in msg, msg
        mg.set_coefficient(contrast_coefficient(L, 10.0))
        rc, msg = raw_multi_gcr(pkg, mg)
        assert rc == STATE and "not built" in msg, msg
        assert raw_time(pkg, mg)[0] == STATE
        mg.build_galerkin()
        for kw, word in ((dict(nrhs=0), "nrhs"), (dict(nrhs=pkg.MAX_RHS + 1), "nrhs"), (dict(restart=0), "restart"),
                         (dict(restart=pkg.GCR_MAX_RESTART + 1), "restart"), (dict(b=False), "NULL"), (dict(u=False), "NULL"),
                         (dict(tol=float("nan")), "tol"), (dict(tol=-1.0), "tol"), (dict(max_iters=-1), "max_iters")):
            refused(pkg, mg, L, INVALID, word, **kw)
        b, u0 = fates(mg, L, np.float64)
        assert_block(mg, b, u0, TOL, ITERS, 3, sequential(mg, b, u0, TOL, ITERS, 3), "after the refusals")


# ---- 10. mgx_time_multi_gcr_direction --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contrast10", "rot45"])
def test_time_multi_gcr_direction(pkg, kind):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", kind) as mg:
        b, u0 = fates(mg, L, np.float64)
        before = solve_one(mg, rand(L, 11), rand(L, 12), 0.0, 2)
        rc, msg, _ = raw_time(pkg, mg)
        assert rc == STATE and "mgx_solve_multi_gcr" in msg, msg
        mg.solve_multi(b, u0, tol=TOL, max_cycles=2)                  # the columns alone are not enough
        assert raw_time(pkg, mg, nrhs=2)[0] == STATE
        first = block(mg, b[:2], u0[:2], TOL, ITERS, 3)
        assert raw_time(pkg, mg, nrhs=3)[0] == STATE                # slot 0 of two columns exists
        full = block(mg, b, u0, TOL, ITERS, 3)
        grids, graphs = snapshot(pkg, mg)
        for nrhs in (1, 2, 3, 4):
            for repeats in (1, 3):
                ms = mg.time_multi_gcr_direction(nrhs, repeats)
                assert np.isfinite(ms) and ms > 0.0, (nrhs, repeats, ms)
        for bad in (dict(nrhs=0), dict(nrhs=5), dict(repeats=0)):
            rc, msg, _ = raw_time(pkg, mg, **bad)
            assert rc == INVALID and msg
        grids1, graphs1 = snapshot(pkg, mg)
        assert graphs1 == graphs and all(np.array_equal(a, a1) for a, a1 in zip(grids, grids1))
        again = block(mg, b, u0, TOL, ITERS, 3)
        for j in range(4):
            assert_column(again[j], full[j], f"column {j} after the timing")
        for j in range(2):
            assert_column(first[j], full[j], f"column {j} of two")
        assert_column(solve_one(mg, rand(L, 11), rand(L, 12), 0.0, 2), before, "mgx_solve after the timing")


if __name__ == "__main__":
    assert sys.argv[1:] == ["rows-child"] and os.environ.get("MGX_ROWS") == "5"
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    check_rows(ge.load_package())
    print("rows-child ok")
