"""GPU tests of mgx_solve_multi_refine_gcr and mgx_time_multi_refine_direction (include/mgx.h): fp64 restarted GCR around
the float block cycle on up to MGX_MAX_RHS right-hand sides per operator read, on general-operator Jacobi F64 handles.

Every comparison is assert_column (== on the stats fields, np.array_equal on history and iterate) against
mgx_solve_refine_gcr ON THE SAME HANDLE (mgx_set_rhs, mgx_set_guess, mgx_solve_refine_gcr, mgx_get_solution), column by
column.  mgx_solve_refine_gcr replays the float cycle of the shadow hierarchy from a graph of the K = 1 kernels and runs
k_refine_direction<NQ, 1> and k_refine_update on the handle's own Krylov workspace; the block call launches the K-column
instances of the same float kernels eagerly on the shadow's columns, k_refine_direction<NQ, K> (csrc/mgx_refine_gcr.hpp)
for the set, and the coefficient-free passes once per column on that column's scalars, partial sums and float right-hand
side, each column scaled by the power of two its own history gives - the bits must not know the difference.

Shapes are tests/test_gpu_multi.py's: (4, 3): 15^2 unknowns, a partial strip; (7, 3): 127 columns, a second fp64 strip
that is a sliver; (8, 4): 255 columns, three strips, several workgroups per strip.  R = 4 rows per chunk at every size here
unless MGX_ROWS says otherwise; test 3 runs chunks of five rows on 127 (25 chunks and one of two rows) in a child process.

The columns are the block of tests/test_gpu_multi_gcr.py's fates() with the guess of the last column produced by 40
iterations of mgx_solve_refine_gcr: a random b from a zero guess; a zero column (never active); a random b and guess scaled
by 1e-161, where the squares of the dots leave the double range after a few iterations (the refinement loop commutes with
powers of two, tests/test_refine_gcr_cpu.py, so only underflow ends it early: ||r||^2 = 0 or a breakdown of this column
while the others go on); and a random b from the guess 40 iterations left, which converges like a fresh one.  The test
asserts from the sequential reference's stats that min(nrhs, 3) different iteration counts occur among the first nrhs
columns: without that it could not show that freezing works.

`python tests/test_gpu_multi_refine_gcr.py rows-child` is the child process of test 3."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_multi_gcr as tg
from test_gpu_multi import F, SHAPES, W, assert_column, handle, solve_one
from test_gpu_refine import BILINEAR, INVALID, OPERATOR, STATE, config, give_operator, rand, refine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL, ITERS = 1e-6, 12
SWEEP = tg.SWEEP


def refine_gcr_one(mg, b, u0, tol, max_iters, restart):
    mg.set_rhs(b)
    mg.set_guess(u0)
    st, hist = mg.solve_refine_gcr(tol=tol, max_iters=max_iters, restart=restart)
    return st, hist, mg.get_solution()


def sequential(mg, b, u0, tol, max_iters, restart):
    """the reference: one mgx_solve_refine_gcr per column on the same handle"""
    return [refine_gcr_one(mg, b[j], u0[j], tol, max_iters, restart) for j in range(len(b))]


def block(mg, b, u0, tol, max_iters, restart):
    stats, hists, u = mg.solve_multi_refine_gcr(b, u0, tol=tol, max_iters=max_iters, restart=restart)
    assert len(stats) == len(hists) == len(u) == len(b)
    return [(stats[j], hists[j], u[j]) for j in range(len(b))]


def assert_block(mg, b, u0, tol, max_iters, restart, ref, what):
    """solve_multi_refine_gcr on the columns of b / u0 against ref (sequential's list); returns the columns"""
    got = block(mg, b, u0, tol, max_iters, restart)
    for j in range(len(b)):
        assert_column(got[j], ref[j], f"{what}, column {j} of {len(b)}")
        assert np.isfinite(got[j][1]).all() and np.isfinite(got[j][2]).all(), f"{what}, column {j}: not finite"   # (NaN != NaN)
    assert len({g[0].seconds for g in got}) == 1 and got[0][0].seconds > 0.0
    return got


def fates(mg, L):
    """the block of test_gpu_multi_gcr.fates(mg, L, float64), the guess of its last column from mgx_solve_refine_gcr"""
    b, u0 = tg.fates(mg, L, np.float64)
    u0[3] = refine_gcr_one(mg, b[3], np.zeros_like(b[3]), 0.0, 40, 4)[2]
    return b, u0


# ---- 1. bit for bit against mgx_solve_refine_gcr, columns with different fates ------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("op,kind,transfer,kw", SWEEP, ids=[f"{o}-{k}-{'opdep' if t else 'bilinear'}" for o, k, t, _ in SWEEP])
def test_every_column_has_the_bits_of_mgx_solve_refine_gcr(pkg, op, kind, transfer, kw, shape):
    """restart 3 with 12 iterations crosses the restart boundary several times; restart 1 empties the basis every iteration"""
    L, Lc = shape
    with handle(pkg, L, Lc, op, kind, transfer, **kw) as mg:
        b, u0 = fates(mg, L)
        for restart in (1, 3):
            ref = sequential(mg, b, u0, TOL, ITERS, restart)
            counts = [r[0].cycles for r in ref]
            print(f"{op} {kind} transfer {transfer} {L}..{Lc} restart {restart}: iterations {counts}, converged "
                  f"{[r[0].converged for r in ref]}")
            for nrhs in (1, 2, 3, 4):
                assert len(set(counts[:nrhs])) >= min(nrhs, 3), f"nrhs = {nrhs}: iteration counts {counts[:nrhs]} do not show freezing"
                assert_block(mg, b[:nrhs], u0[:nrhs], TOL, ITERS, restart, ref, f"restart {restart}, nrhs = {nrhs}")
            # the zero column: never active
            assert ref[1][0].cycles == 0 and ref[1][0].converged == 1 and ref[1][0].history_len == 1 and ref[1][1][0] == 0.0
            assert 0 < ref[0][0].cycles < ITERS and ref[0][0].converged == 1
            assert 0 < ref[3][0].cycles < ITERS and ref[3][0].converged == 1


# ---- 2. a deep basis: k_gcr_dots<7> / k_gcr_orth<7> per column, with per-column scalars and scales -----------------------
def test_deep_basis(pkg):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", "rot45", OPERATOR) as mg:
        b = np.stack([rand(L, 20 + j) for j in range(4)])
        u0 = np.zeros_like(b)
        u0[3] = rand(L, 29)
        ref = sequential(mg, b, u0, 0.0, 9, 8)
        assert [r[0].cycles for r in ref] == [9, 9, 9, 9]              # slots 0 .. 7, then slot 0 of the second restart cycle
        assert_block(mg, b, u0, 0.0, 9, 8, ref, "restart 8")


# ---- 3. chunk seams of the direction kernel --------------------------------------------------------------------------------
def check_rows(pkg):
    L, Lc = 7, 3
    for kind in ("contrast10", "rot45"):                             # a five- and a nine-point finest level
        with handle(pkg, L, Lc, "gal", kind, OPERATOR) as mg:
            b, u0 = fates(mg, L)
            ref = sequential(mg, b, u0, TOL, ITERS, 3)
            for nrhs in (2, 3, 4):
                assert_block(mg, b[:nrhs], u0[:nrhs], TOL, ITERS, 3, ref, f"MGX_ROWS=5, {kind}, nrhs = {nrhs}")


def test_chunks_of_five_rows_on_127():
    """a fresh process whose handles are created with MGX_ROWS=5: 127 rows are 25 chunks of five and one of two"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "rows-child"], env=dict(os.environ, MGX_ROWS="5"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rows-child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- 4. the grouping of the columns does not reach the bits ----------------------------------------------------------------
def test_permuted_columns_give_permuted_results(pkg):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", "rot45", OPERATOR) as mg:
        b, u0 = fates(mg, L)
        four = block(mg, b, u0, TOL, ITERS, 3)
        perm = [2, 0, 3, 1]
        got = block(mg, b[perm], u0[perm], TOL, ITERS, 3)
        for j, src in enumerate(perm):
            assert_column(got[j], four[src], f"permuted column {j} (was {src})")
        three = block(mg, b[:3], u0[:3], TOL, ITERS, 3)
        for j in range(3):
            assert_column(three[j], four[j], f"column {j} of three")


# ---- 5. W and F cycles: the shadow's graph visits the small levels through k_small_visit, the block call does not --------
@pytest.mark.parametrize("cycle", [W, F], ids=["W", "F"])
@pytest.mark.parametrize("transfer", [BILINEAR, OPERATOR], ids=["bilinear", "opdep"])
def test_w_and_f_cycles(pkg, cycle, transfer):
    L, Lc = 6, 3
    with handle(pkg, L, Lc, "gal", "contrast10", transfer, cycle=cycle) as mg:
        b, u0 = fates(mg, L)
        ref = sequential(mg, b, u0, TOL, ITERS, 3)
        assert_block(mg, b, u0, TOL, ITERS, 3, ref, f"cycle {cycle}, transfer {transfer}")


# ---- 6. the bottom -----------------------------------------------------------------------------------------------------------
def test_smoothed_bottom(pkg):
    L, Lc = 7, 3
    assert pkg.BOTTOM_SMOOTH == 1
    with handle(pkg, L, Lc, "gal", "contrast10", bottom=1) as mg:
        b, u0 = fates(mg, L)
        ref = sequential(mg, b, u0, TOL, ITERS, 3)
        assert_block(mg, b, u0, TOL, ITERS, 3, ref, "bottom = SMOOTH")


@pytest.mark.parametrize("kind", ["contrast10", "rot45"])
def test_one_level_hierarchy_with_the_exact_bottom(pkg, kind):
    """finest = coarsest: the float cycle is one dense solve per column, which overwrites the float u (with bottom = SMOOTH the
    block call is defined to start from zero and is not held to the sequential bits: include/mgx.h)"""
    L = 4
    with handle(pkg, L, L, "gal", kind) as mg:
        b, u0 = fates(mg, L)
        ref = sequential(mg, b, u0, TOL, ITERS, 3)
        assert_block(mg, b, u0, TOL, ITERS, 3, ref, "one level, bottom = EXACT")


# ---- 7. breakdown --------------------------------------------------------------------------------------------------------------
def test_breakdown_of_every_column_and_the_calls_after_it(pkg):
    """GALERKIN 7..4 with mu1 = mu2 = 0 and bottom = SMOOTH (tests/test_gpu_multi_gcr.py's construction): the float cycle from
    zero returns exactly zero, so z = 0, q' = A z = 0 and q'.q' = 0 at iteration 1 in every column with a residual"""
    L, Lc = 7, 4
    kw = dict(mu1=0, mu2=0, bottom=1)
    with handle(pkg, L, Lc, "gal", "contrast10", **kw) as mg, handle(pkg, L, Lc, "gal", "contrast10", **kw) as fresh:
        b = np.stack([rand(L, 30 + j) for j in range(4)])
        u0 = np.zeros_like(b)
        u0[1] = rand(L, 39)
        ref = sequential(fresh, b, u0, TOL, ITERS, 3)
        assert "GCR breakdown at iteration 1" in pkg.lib().mgx_last_error(fresh._h).decode()
        for _ in range(2):                                           # the second call: from the flags and scalars of the first
            got = assert_block(mg, b, u0, TOL, ITERS, 3, ref, "breakdown")       # MGX_OK: anything else raises
            msg = pkg.lib().mgx_last_error(mg._h).decode()
            assert "mgx_solve_multi_refine_gcr" in msg and "GCR breakdown at iteration 1" in msg and "column 0" in msg and "q'.q'" in msg, msg
            for j, (st, hist, u) in enumerate(got):
                assert st.converged == 0 and st.cycles == 0 and st.history_len == 1 and len(hist) == 1
                assert np.array_equal(u, u0[j]), f"column {j} is not its guess"
        # the calls after it have a fresh handle's bits
        assert_column(refine_gcr_one(mg, b[0], u0[0], TOL, ITERS, 3), refine_gcr_one(fresh, b[0], u0[0], TOL, ITERS, 3), "mgx_solve_refine_gcr after it")
        assert_column(tg.gcr_one(mg, b[0], u0[0], TOL, ITERS, 3), tg.gcr_one(fresh, b[0], u0[0], TOL, ITERS, 3), "mgx_solve_gcr after it")
        for got, want in zip(tg.block(mg, b, u0, TOL, ITERS, 3), tg.block(fresh, b, u0, TOL, ITERS, 3)):
            assert_column(got, want, "mgx_solve_multi_gcr after it")
        m, m0 = mg.solve_multi(b, u0, tol=TOL, max_cycles=2), fresh.solve_multi(b, u0, tol=TOL, max_cycles=2)
        for j in range(4):
            assert_column((m[0][j], m[1][j], m[2][j]), (m0[0][j], m0[1][j], m0[2][j]), f"mgx_solve_multi after it, column {j}")


# ---- 8. the scales: invariance under a power of two, per column ----------------------------------------------------------------
# (the statement tests/test_gpu_refine_gcr.py holds mgx_solve_refine_gcr to: every double operation commutes with a power of
# two while nothing overflows or goes subnormal, and r / s_k is the same float for every exponent; 2^+-160 lies beyond
# float's range, so a pass that took another column's scale would hand the float cycle zeros or infinities)
@pytest.mark.parametrize("kind", ["contrast10", "rot45"])
def test_a_power_of_two_on_b_and_u_is_a_power_of_two_on_the_result_bit_for_bit(pkg, kind):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", kind) as mg:
        b = np.stack([rand(L, 70 + j) for j in range(4)])
        u0 = np.stack([rand(L, 80 + j) for j in range(4)])
        for tol, k in ((0.0, 6), (1e-10, 40)):
            plain = block(mg, b, u0, tol, k, 4)
            assert all((st.cycles == 6) if tol == 0.0 else (st.converged == 1 and 6 < st.cycles < 40) for st, _, _ in plain)
            # every column by the same power, then each column by its own in one call
            for exps in ((-160,) * 4, (160,) * 4, (-160, 0, 160, 40)):
                e = np.array(exps).reshape(4, 1, 1)
                got = block(mg, np.ldexp(b, e), np.ldexp(u0, e), tol, k, 4)
                for j in range(4):
                    st, hist, u = plain[j]
                    want = (st, np.ldexp(hist, exps[j]), np.ldexp(u, exps[j]))
                    assert got[j][0].cycles == st.cycles and got[j][0].converged == st.converged and got[j][0].fine_updates == st.fine_updates
                    assert np.array_equal(got[j][1], want[1]), (exps, j, got[j][1], want[1])
                    assert np.array_equal(got[j][2], want[2]), (exps, j)
                    assert np.isfinite(got[j][2]).all() and np.all(got[j][1] > 0.0)


# ---- 9. the state of the handle ------------------------------------------------------------------------------------------------
def snapshot(mg):
    """U and B of every level, and the number of cached graphs"""
    L, Lc = mg.cfg.finest_level, mg.cfg.coarsest_level
    return [mg.get_level(lv, which) for lv in range(Lc, L + 1) for which in (0, 1)], mg.graphs_cached()


def test_the_handle_is_left_as_it_was(pkg):
    L, Lc = 7, 3
    assert (pkg.VEC_U, pkg.VEC_B) == (0, 1)
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as twin:
        for h in (mg, twin):
            # the same calls on both: every level holds something, the graphs of the handle and of its float copy are
            # captured, both Krylov workspaces and the columns exist
            b, u0 = fates(h, L)
            solve_one(h, rand(L, 11), rand(L, 12), 0.0, 3)
            tg.gcr_one(h, b[0], u0[3], 0.0, 3, 2)
            refine(h, b[0], u0[3], 0.0, 2)
            refine_gcr_one(h, b[0], u0[3], 0.0, 3, 2)
            tg.block(h, b[:2], u0[:2], 0.0, 2, 2)
        grids, graphs = snapshot(mg)
        assert graphs > 0
        block(mg, b, u0, TOL, ITERS, 3)
        grids1, graphs1 = snapshot(mg)
        assert graphs1 == graphs
        for a, a1 in zip(grids, grids1):
            assert np.array_equal(a, a1)
        grids0, graphs0 = snapshot(twin)
        assert graphs0 == graphs and all(np.array_equal(a, a0) for a, a0 in zip(grids, grids0))
        # the handle goes on from its own U and B as one that never made the call
        (st, hist), (st0, hist0) = mg.solve(tol=0.0, max_cycles=3), twin.solve(tol=0.0, max_cycles=3)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, twin.get_solution()), "mgx_solve after the call")
        (st, hist), (st0, hist0) = mg.solve_gcr(tol=0.0, max_iters=4, restart=4), twin.solve_gcr(tol=0.0, max_iters=4, restart=4)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, twin.get_solution()), "mgx_solve_gcr after the call")
        (st, hist), (st0, hist0) = mg.solve_refine(tol=0.0, max_cycles=3), twin.solve_refine(tol=0.0, max_cycles=3)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, twin.get_solution()), "mgx_solve_refine after the call")
        (st, hist), (st0, hist0) = mg.solve_refine_gcr(tol=0.0, max_iters=4, restart=4), twin.solve_refine_gcr(tol=0.0, max_iters=4, restart=4)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, twin.get_solution()), "mgx_solve_refine_gcr after the call")
        m, m0 = mg.solve_multi(b, u0, tol=TOL, max_cycles=6), twin.solve_multi(b, u0, tol=TOL, max_cycles=6)
        for j in range(4):
            assert_column((m[0][j], m[1][j], m[2][j]), (m0[0][j], m0[1][j], m0[2][j]), f"mgx_solve_multi after the call, column {j}")
        for j, (got, want) in enumerate(zip(tg.block(mg, b, u0, TOL, ITERS, 3), tg.block(twin, b, u0, TOL, ITERS, 3))):
            assert_column(got, want, f"mgx_solve_multi_gcr after the call, column {j}")


# ---- 10. interleaving and growth -------------------------------------------------------------------------------------------------
def test_interleaved_calls_a_growing_workspace_and_a_new_operator(pkg):
    """the call shares the columns' Krylov pieces with mgx_solve_multi_gcr and the columns with mgx_solve_multi: none may see the
    scalars, partial sums, basis slots or swapped grids another one left.  The float copy follows the operator"""
    from test_gpu_multi import sequential as cycles_sequential
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as big:
        b, u0 = fates(mg, L)
        ref2 = sequential(mg, b, u0, TOL, ITERS, 2)
        ref5 = sequential(mg, b, u0, TOL, ITERS, 5)
        assert_block(mg, b[:2], u0[:2], TOL, ITERS, 2, ref2, "two columns, restart 2")       # allocates 2 columns of 2 pairs
        tg.assert_block(mg, b[:3], u0[:3], TOL, ITERS, 3, tg.sequential(mg, b[:3], u0[:3], TOL, ITERS, 3), "mgx_solve_multi_gcr between")
        grown = assert_block(mg, b, u0, TOL, ITERS, 5, ref5, "four columns, restart 5, after 2 / 2")
        started = block(big, b, u0, TOL, ITERS, 5)                                        # a handle that starts at 4 / 5
        for j in range(4):
            assert_column(grown[j], started[j], f"grown against started at 4 / 5, column {j}")
        stats, hists, u = mg.solve_multi(b, u0, tol=TOL, max_cycles=6)
        for j, want in enumerate(cycles_sequential(mg, b, u0, TOL, 6)):
            assert_column((stats[j], hists[j], u[j]), want, f"mgx_solve_multi between, column {j}")
        assert_block(mg, b[:2], u0[:2], TOL, ITERS, 2, ref2, "two columns, restart 2, in the larger workspace")
        from pcg_ref import contrast_coefficient
        mg.set_coefficient(contrast_coefficient(L, 100.0))
        mg.build_galerkin(OPERATOR)
        ref100 = sequential(mg, b, u0, TOL, ITERS, 5)
        assert not np.array_equal(ref100[0][2], ref5[0][2])
        assert_block(mg, b, u0, TOL, ITERS, 5, ref100, "after set_coefficient and a rebuild")
        mg.set_coefficient(contrast_coefficient(L, 30.0))               # this time the block call is the one that rebuilds the float copy
        mg.build_galerkin(OPERATOR)
        got = block(mg, b, u0, TOL, ITERS, 5)
        for j, want in enumerate(sequential(mg, b, u0, TOL, ITERS, 5)):
            assert_column(got[j], want, f"the block call first after a rebuild, column {j}")
        give_operator(pkg, mg, "rot45", L, Lc, BILINEAR)                # nine-point finest level, other transfer
        assert_block(mg, b, u0, TOL, ITERS, 5, sequential(mg, b, u0, TOL, ITERS, 5), "after set_tensor and a rebuild")


# ---- 11. edge arguments ----------------------------------------------------------------------------------------------------------
def test_a_short_history_slot_is_not_overrun(pkg):
    L, Lc, cap = 6, 3, 3
    with handle(pkg, L, Lc, "gal", "contrast10") as mg:
        b, u0 = fates(mg, L)
        ref = sequential(mg, b, u0, TOL, ITERS, 3)
        u = u0.copy()
        stats = (pkg.Stats * 4)()
        flat = np.full(4 * cap + 5, -7.0)                          # column j starts at flat + j * cap; five doubles of margin
        rc = pkg.lib().mgx_solve_multi_refine_gcr(mg._h, 4, b.ctypes.data, u.ctypes.data, TOL, ITERS, 3, stats,
                                                  flat.ctypes.data_as(C.POINTER(C.c_double)), cap)
        assert rc == 0
        for j in range(4):
            want = ref[j][1]
            k = min(cap, len(want))
            assert stats[j].history_len == len(want)
            assert np.array_equal(flat[j * cap: j * cap + k], want[:k])
            assert np.all(flat[j * cap + k: (j + 1) * cap] == -7.0), f"column {j} wrote past its history"
            assert np.array_equal(u[j], ref[j][2])
        assert np.all(flat[4 * cap:] == -7.0)
        # stats = NULL and history = NULL
        u = u0.copy()
        assert pkg.lib().mgx_solve_multi_refine_gcr(mg._h, 4, b.ctypes.data, u.ctypes.data, TOL, ITERS, 3, None, None, 0) == 0
        assert all(np.array_equal(u[j], ref[j][2]) for j in range(4))


def test_no_iterations_returns_the_guesses(pkg):
    L, Lc = 6, 3
    with handle(pkg, L, Lc, "gal", "contrast10") as mg:
        b, u0 = fates(mg, L)
        ref = sequential(mg, b, u0, TOL, 0, 3)
        got = assert_block(mg, b, u0, TOL, 0, 3, ref, "max_iters = 0")
        assert [g[0].history_len for g in got] == [1, 1, 1, 1] and [len(g[1]) for g in got] == [1, 1, 1, 1]
        assert all(np.array_equal(g[2], u0[j]) for j, g in enumerate(got))


# ---- 12. refusals ------------------------------------------------------------------------------------------------------------------
def raw_solve(pkg, mg, nrhs=2, b=True, u=True, tol=1e-8, max_iters=2, restart=2):
    n = mg.n()
    bb, uu = np.ones((max(nrhs, 1), n, n)), np.zeros((max(nrhs, 1), n, n))
    rc = pkg.lib().mgx_solve_multi_refine_gcr(mg._h, nrhs, bb.ctypes.data if b else None, uu.ctypes.data if u else None, tol, max_iters, restart,
                                              None, None, 0)
    return rc, pkg.lib().mgx_last_error(mg._h).decode()


def raw_time(pkg, mg, nrhs=1, repeats=2, ms=True):
    out = C.c_double(-1.0)
    rc = pkg.lib().mgx_time_multi_refine_direction(mg._h, nrhs, repeats, C.byref(out) if ms else None)
    return rc, pkg.lib().mgx_last_error(mg._h).decode(), out.value


def refused(pkg, mg, L, status, word=None, dt=np.float64, **kw):
    """the call is refused with `status` and a reason; the handle solves to the same bits before and after"""
    b = rand(L, 5).astype(dt)
    before = solve_one(mg, b, np.zeros_like(b), 0.0, 2)
    rc, msg = raw_solve(pkg, mg, **kw)
    assert rc == status and msg and (word is None or word in msg), (rc, msg)
    if status == STATE:
        rc, msg, _ = raw_time(pkg, mg)
        assert rc == STATE and msg and (word is None or word in msg), (rc, msg)
    assert_column(solve_one(mg, b, np.zeros_like(b), 0.0, 2), before, "mgx_solve after the refusal")


def test_poisson_f32_and_mixed_handles_are_refused_with_the_reason(pkg):
    L, Lc = 6, 3
    base = dict(finest_level=L, coarsest_level=Lc, mu1=2, mu2=2, schedule=0)
    with pkg.Multigrid(**base) as mg:
        refused(pkg, mg, L, STATE, "POISSON")
    with pkg.Multigrid(dtype=pkg.DTYPE_MIXED, **base) as mg:
        refused(pkg, mg, L, STATE, "POISSON")
    for op, kind in (("gal", "contrast10"), ("s5", "random5")):
        with handle(pkg, L, Lc, op, kind, dtype=pkg.DTYPE_F32) as mg:
            refused(pkg, mg, L, STATE, "F64 handles only", dt=np.float32)


@pytest.mark.parametrize("kind", ["n_gpus", "rank"])
def test_multi_gpu_and_rank_handles_are_refused_with_the_reason(pkg, kind):
    """(the rank case spends its seconds in ncclCommInitRank: a rank handle cannot be created without it)"""
    kw = dict(finest_level=9, coarsest_level=6, mu1=2, mu2=2, schedule=0, cut_level=7)
    mg = pkg.Multigrid(n_gpus=2, devices=[0, 0], **kw) if kind == "n_gpus" else pkg.Multigrid.rank(0, 1, rccl_id=pkg.rccl_unique_id(), **kw)
    with mg:
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
        rc, msg = raw_solve(pkg, mg)
        assert rc == STATE and "not set" in msg, msg
        mg.set_coefficient(contrast_coefficient(L, 10.0))
        rc, msg = raw_solve(pkg, mg)
        assert rc == STATE and "not built" in msg, msg
        assert raw_time(pkg, mg)[0] == STATE
        # the arguments are checked before the guards, in mgx_solve_multi_gcr's order
        rc, msg = raw_solve(pkg, mg, nrhs=0, b=False, restart=0)
        assert rc == INVALID and "nrhs" in msg, msg
        rc, msg = raw_solve(pkg, mg, b=False, tol=-1.0, restart=0)
        assert rc == INVALID and "NULL" in msg, msg
        rc, msg = raw_solve(pkg, mg, tol=-1.0, restart=0)
        assert rc == INVALID and "tol" in msg, msg
        rc, msg = raw_solve(pkg, mg, restart=0)
        assert rc == INVALID and "restart" in msg, msg
        mg.build_galerkin()
        for kw, word in ((dict(nrhs=0), "nrhs"), (dict(nrhs=pkg.MAX_RHS + 1), "nrhs"), (dict(restart=0), "restart"),
                         (dict(restart=pkg.GCR_MAX_RESTART + 1), "restart"), (dict(b=False), "NULL"), (dict(u=False), "NULL"),
                         (dict(tol=float("nan")), "tol"), (dict(tol=-1.0), "tol"), (dict(max_iters=-1), "max_iters")):
            assert pkg.GCR_MAX_RESTART + 1 == 9
            refused(pkg, mg, L, INVALID, word, **kw)
            assert "mgx_solve_multi_refine_gcr" in raw_solve(pkg, mg, **kw)[1]
        b, u0 = fates(mg, L)
        assert_block(mg, b, u0, TOL, ITERS, 3, sequential(mg, b, u0, TOL, ITERS, 3), "after the refusals")
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OPERATOR_STENCIL5)) as mg:
        rc, msg = raw_solve(pkg, mg)
        assert rc == STATE and "not set" in msg, msg


# ---- 13. mgx_time_multi_refine_direction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contrast10", "rot45"])
def test_time_multi_refine_direction(pkg, kind):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", kind) as mg:
        b, u0 = fates(mg, L)                                        # (mgx_solve_gcr and mgx_solve_refine_gcr have run: not enough)
        before = solve_one(mg, rand(L, 11), rand(L, 12), 0.0, 2)
        rc, msg, _ = raw_time(pkg, mg)
        assert rc == STATE and "mgx_solve_multi_refine_gcr" in msg, msg
        tg.block(mg, b, u0, TOL, 2, 3)                              # the fp64 columns and their basis alone are not enough
        assert raw_time(pkg, mg, nrhs=1)[0] == STATE
        first = block(mg, b[:2], u0[:2], TOL, ITERS, 3)
        assert raw_time(pkg, mg, nrhs=3)[0] == STATE                # the float columns of two exist
        full = block(mg, b, u0, TOL, ITERS, 3)
        grids, graphs = snapshot(mg)
        for nrhs in (1, 2, 3, 4):
            for repeats in (1, 3):
                ms = mg.time_multi_refine_direction(nrhs, repeats)
                assert np.isfinite(ms) and ms > 0.0, (nrhs, repeats, ms)
        for bad in (dict(nrhs=0), dict(nrhs=5), dict(repeats=0), dict(ms=False)):
            rc, msg, _ = raw_time(pkg, mg, **bad)
            assert rc == INVALID and msg
        grids1, graphs1 = snapshot(mg)
        assert graphs1 == graphs and all(np.array_equal(a, a1) for a, a1 in zip(grids, grids1))
        again = block(mg, b, u0, TOL, ITERS, 3)
        for j in range(4):
            assert_column(again[j], full[j], f"column {j} after the timing")
        for j in range(2):
            assert_column(first[j], full[j], f"column {j} of two")
        assert_column(refine_gcr_one(mg, b[0], u0[0], TOL, ITERS, 3), full[0], "mgx_solve_refine_gcr after the timing")
        assert_column(solve_one(mg, rand(L, 11), rand(L, 12), 0.0, 2), before, "mgx_solve after the timing")


if __name__ == "__main__":
    assert sys.argv[1:] == ["rows-child"] and os.environ.get("MGX_ROWS") == "5"
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    check_rows(ge.load_package())
    print("rows-child ok")
