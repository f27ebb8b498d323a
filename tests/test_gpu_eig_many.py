"""GPU tests of mgx_eigs_many and mgx_time_eig_project (include/mgx.h): up to 16 smallest eigenpairs by mgx_eigs' LOBPCG on
blocks of four, each block in the complement of the pairs locked before it (csrc/mgx_eig_many.hpp).

The checks are those of tests/test_gpu_eig.py (its `check`), on all nev pairs: r_j = A x_j - theta_j x_j recomputed in numpy
from the returned vectors, and
    |theta_j - lambda_j| <= ||r_j|| + 64 eps lambda_max,      theta_j >= lambda_j - 64 eps lambda_max
against the j-th exact eigenvalue (closed form or numpy.linalg.eigvalsh): together they show that these are the nev SMALLEST
pairs.  |X^T X - I| is measured over all nev vectors; its bound is 16 x the defect of tests/eig_many_ref.py on the same case
(fp32: times eps32 / eps64), that file's rule.  max_iters = 2 x the largest per-block iteration count of eig_many_ref on the
case, and every block has to converge within it.

Shapes (finest, coarsest): (5, 2) the smallest level of the strip kernels; (6, 3) with nev = 16; (8, 3) in fp64 and (9, 3) in
fp32: more than one strip.  fp32 tolerance: test_gpu_eig.py's rule, max(1e-3, 40 x 2^-24 lambda_max / lambda_1)."""
import ctypes as C
import functools

import numpy as np
import pytest

import eig_many_ref as em
import eig_ref as er
from test_gpu_eig import U32, V, W, check, exact_values, fine_stencil, make
from test_gpu_eig import snapshot as snapshot_urb
from test_gpu_multi import assert_column, handle, snapshot, solve_one
from test_gpu_refine import BILINEAR, INVALID, OPERATOR, STATE, config, rand

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("cycles", "converged", "history_len", "initial_residual", "final_residual", "fine_updates")


@functools.lru_cache(maxsize=None)
def reference(op, kind, L, Lc, transfer=BILINEAR, cycle=V, nev=8, tol=1e-8):
    """eig_many_ref on the case, computed once: (fine stencil, result)"""
    fine = fine_stencil(kind, L)
    st = (lambda lv: er.constant_stencil(lv, float(kind[5:]))) if op == "s5" else fine
    h = er.hierarchy(op, st, L, Lc, transfer, cycle)
    res = em.eigs_many(lambda v: er.apply(fine, v), er.preconditioner(h), er.guesses(L, nev), tol, 200)
    assert not res.reason and all(res.converged) and res.computed == nev, (op, kind, L, Lc, res.reason)
    return fine, res


def last_error(pkg, mg):
    return pkg.lib().mgx_last_error(mg._h).decode()


def solve_case(pkg, op, kind, L, Lc, transfer=BILINEAR, cycle=None, nev=8, tol=1e-8, f32=False):
    fine, ref = reference(op, kind, L, Lc, transfer, V if cycle is None else cycle, nev, tol)
    budget = 2 * max(ref.block_iterations)
    with make(pkg, op, kind, L, Lc, transfer, cycle, f32) as mg:
        theta, X, stats, hists = mg.eigs_many(nev, x0=er.guesses(L, nev), tol=tol, max_iters=budget)
    name = f"{op} {kind} {L}..{Lc} transfer {transfer} cycle {cycle} nev {nev} {'f32' if f32 else 'f64'} tol {tol:g}"
    print(f"{name}: iterations per pair {[len(h) - 1 for h in hists]} (eig_many_ref per block {ref.block_iterations}, budget {budget}), "
          f"cycles {[st.cycles for st in stats]}")
    assert all(1 <= len(h) <= budget + 1 for h in hists)
    fine_t = fine_stencil(kind, L, np.float32) if f32 else fine
    check(name, fine_t, theta, X, stats, hists, exact_values(kind, L, nev), tol, er.orthonormality_defect(ref.X), f32)
    return theta, X, stats, hists


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,kind,shape,nev", [("gal", "const1.0", (5, 2), 12), ("gal", "const0.5", (5, 2), 10), ("gal", "const1.0", (6, 3), 16),
                                               ("s5", "const0.5", (6, 3), 9), ("s5", "const1.0", (5, 2), 5), ("gal", "const0.5", (8, 3), 6)])
def test_closed_form_eigenvalues(pkg, op, kind, shape, nev):
    """nev 12 of the Poisson operator at level 5 cuts the degenerate pair 12 / 13; 10, 9, 5 and 6 end in blocks of 2, 1, 1, 2"""
    solve_case(pkg, op, kind, *shape, nev=nev)


# ---- 2. the dense reference at (5, 2) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,transfer,cycle,nev", [("contrast10", BILINEAR, None, 12), ("contrast10", OPERATOR, None, 12),
                                                     ("contrast100", OPERATOR, None, 10), ("rot45", OPERATOR, W, 12)])
def test_against_eigvalsh_at_level_5(pkg, kind, transfer, cycle, nev):
    solve_case(pkg, "gal", kind, 5, 2, transfer, cycle, nev=nev)


# ---- 3. one block is mgx_eigs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nev", [1, 2, 3, 4])
def test_up_to_four_pairs_are_the_bits_of_mgx_eigs(pkg, nev):
    L, Lc = 6, 3
    g = er.guesses(L, nev)
    with make(pkg, "gal", "const0.5", L, Lc) as mg:
        want = mg.eigs(nev, x0=g, tol=1e-8, max_iters=80)
        got = mg.eigs_many(nev, x0=g, tol=1e-8, max_iters=80)
    assert all(st.converged for st in want[2])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for j in range(nev):
        assert np.array_equal(got[3][j], want[3][j])
        for f in STAT_FIELDS:
            assert getattr(got[2][j], f) == getattr(want[2][j], f), (j, f)


# ---- 4. F32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nev", [((5, 2), 10), ((9, 3), 6)], ids=["5-2", "9-3"])
def test_f32(pkg, shape, nev):
    L, Lc = shape
    lam = er.constant_eigenvalues(L, 1.0, 1)[0]
    tol = max(1e-3, 40 * U32 * er.lambda_max_bound(fine_stencil("const1.0", L)) / lam)
    print(f"level {L}: tol {tol:.3g}")
    solve_case(pkg, "gal", "const1.0", L, Lc, nev=nev, tol=tol, f32=True)


# ---- 5. a block that cannot converge -----------------------------------------------------------------------------------------
def test_a_block_that_does_not_converge_ends_the_call(pkg):
    L, Lc, nev = 5, 2, 10
    g = er.guesses(L, nev)
    with make(pkg, "gal", "const0.5", L, Lc) as mg:
        x = g.copy()
        lam = np.full(nev, -1.0)
        stats = (pkg.Stats * nev)()
        for st in stats:
            st.cycles, st.history_len, st.seconds = 7, 7, 7.0
        hist = np.full((nev, 2), -7.0)
        rc = pkg.lib().mgx_eigs_many(mg._h, nev, x.ctypes.data, lam.ctypes.data_as(C.POINTER(C.c_double)), 1e-8, 1, stats,
                                     hist.ctypes.data_as(C.POINTER(C.c_double)), 2)
        msg = last_error(pkg, mg)
        four = mg.eigs(4, x0=g[:4], tol=1e-8, max_iters=1)
    assert rc == 0 and "block 0" in msg and "max_iters" in msg, (rc, msg)
    # the first block is mgx_eigs on the first four guesses, after one iteration
    assert np.array_equal(lam[:4], four[0]) and np.array_equal(x[:4], four[1])
    for j in range(4):
        assert stats[j].history_len == 2 and stats[j].cycles == 1 and stats[j].converged == 0 and np.array_equal(hist[j], four[3][j])
    # the later blocks: the guesses, untouched, behind the computed pairs
    assert np.array_equal(x[4:], g[4:]) and np.all(lam[4:] == 0.0) and np.all(hist[4:] == -7.0)
    for j in range(4, nev):
        st = stats[j]
        assert (st.history_len, st.cycles, st.converged, st.initial_residual, st.final_residual, st.seconds, st.fine_updates) == (0, 0, 0, 0.0, 0.0, 0.0, 0.0)


# ---- 6. determinism, the workspace grows, the handle is left alone -----------------------------------------------------------
def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and all(np.array_equal(h, h1) for h, h1 in zip(a[3], b[3]))
            and all(getattr(s, f) == getattr(s1, f) for s, s1 in zip(a[2], b[2]) for f in STAT_FIELDS))


def test_two_calls_return_the_same_bits_and_the_handle_is_left_as_it_was(pkg):
    L, Lc = 6, 3
    b, u0 = rand(L, 11), rand(L, 12)
    run = lambda h, nev: h.eigs_many(nev, x0=er.guesses(L, nev), tol=1e-8, max_iters=120)
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as fresh:
        for h in (mg, fresh):
            solve_one(h, b, u0, 0.0, 3)                                   # every level holds something, the graphs are captured
        grids, graphs = snapshot(mg)
        urb, _ = snapshot_urb(pkg, mg)
        assert graphs > 0
        six = run(mg, 6)
        twelve = run(mg, 12)                                              # grows from six locked slots to twelve
        again = run(mg, 12)
        assert all(st.converged for st in six[2] + twelve[2])
        assert same(twelve, again) and same(six, run(mg, 6))
        assert same(twelve, run(fresh, 12))                               # a handle that starts at twelve
        assert np.allclose(six[0][:4], twelve[0][:4], rtol=1e-7, atol=0)
        grids1, graphs1 = snapshot(mg)
        urb1, _ = snapshot_urb(pkg, mg)
        assert graphs1 == graphs and all(np.array_equal(a, a1) for a, a1 in zip(grids, grids1))
        assert all((a is None and a1 is None) or np.array_equal(a, a1) for a, a1 in zip(urb, urb1))
    # afterwards mgx_eigs and mgx_solve return the bits of a handle that never made the call
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as never:
        for h in (mg, never):
            solve_one(h, b, u0, 0.0, 3)
        run(mg, 12)
        g = er.guesses(L, 4)
        assert same(mg.eigs(4, x0=g, tol=1e-8, max_iters=80), never.eigs(4, x0=g, tol=1e-8, max_iters=80))
        (st, hist), (st0, hist0) = mg.solve(tol=0.0, max_cycles=3), never.solve(tol=0.0, max_cycles=3)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, never.get_solution()), "mgx_solve after mgx_eigs_many")
        assert_column(solve_one(mg, b, u0, 0.0, 3), solve_one(never, b, u0, 0.0, 3), "a new mgx_solve after mgx_eigs_many")


# ---- 7. refusals and arguments -------------------------------------------------------------------------------------------------
def raw(pkg, mg, nev=6, x=True, lam=True, tol=1e-8, max_iters=2, x0=None):
    n = mg.n()
    L = mg.cfg.finest_level
    k = min(max(nev, 1), 17)
    xx = (er.guesses(L, k) if x0 is None else x0).astype(mg.level_dtype(L))
    ll = np.zeros(k)
    assert xx.shape[1:] == (n, n)
    rc = pkg.lib().mgx_eigs_many(mg._h, nev, xx.ctypes.data if x else None, ll.ctypes.data_as(C.POINTER(C.c_double)) if lam else None, tol,
                                 max_iters, None, None, 0)
    return rc, last_error(pkg, mg)


def refused(pkg, mg, L, status, word=None, **kw):
    b = rand(L, 5).astype(mg.level_dtype(L))
    before = solve_one(mg, b, np.zeros_like(b), 0.0, 2)
    rc, msg = raw(pkg, mg, **kw)
    assert rc == status and msg and (word is None or word in msg), (rc, msg)
    if status == STATE:
        ms = C.c_double(-1.0)
        assert pkg.lib().mgx_time_eig_project(mg._h, 0, 1, 1, 2, C.byref(ms)) == STATE
    assert_column(solve_one(mg, b, np.zeros_like(b), 0.0, 2), before, "mgx_solve after the refusal")


def test_poisson_and_mixed_handles_are_refused(pkg):
    L, Lc = 6, 3
    base = dict(finest_level=L, coarsest_level=Lc, mu1=2, mu2=2, schedule=0)
    with pkg.Multigrid(**base) as mg:
        refused(pkg, mg, L, STATE, "POISSON")
    with pkg.Multigrid(dtype=pkg.DTYPE_MIXED, **base) as mg:
        refused(pkg, mg, L, STATE)


@pytest.mark.parametrize("smoother", [2, 4, 5, 6, 8, 9])
def test_other_smoothers_are_refused(pkg, smoother):
    with handle(pkg, 6, 3, "gal", "contrast10", smoother=smoother) as mg:
        refused(pkg, mg, 6, STATE, "MGX_SMOOTHER_JACOBI only")


def test_unbuilt_hierarchies_bad_arguments_in_their_order_and_dependent_guesses(pkg):
    from pcg_ref import contrast_coefficient
    L, Lc = 6, 3
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OP_GALERKIN)) as mg:
        rc, msg = raw(pkg, mg)
        assert rc == STATE and "not set" in msg, msg
        mg.set_coefficient(contrast_coefficient(L, 10.0))
        rc, msg = raw(pkg, mg)
        assert rc == STATE and "not built" in msg, msg
        assert raw(pkg, mg, nev=0)[0] == INVALID                                     # MGX_ERR_INVALID comes before MGX_ERR_STATE
        mg.build_galerkin()
        # every call below is wrong in the named argument and in all that follow it
        nan = float("nan")
        assert pkg.EIGS_MAX == 16
        for kw, word in ((dict(nev=0, x=False, lam=False, tol=nan, max_iters=-1), "nev"),
                         (dict(nev=17, x=False, lam=False, tol=nan, max_iters=-1), "nev"),
                         (dict(x=False, tol=nan, max_iters=-1), "NULL"), (dict(lam=False, tol=-1.0, max_iters=-1), "NULL"),
                         (dict(tol=nan, max_iters=-1), "tol"), (dict(tol=-1.0, max_iters=-1), "tol"), (dict(max_iters=-1), "max_iters")):
            refused(pkg, mg, L, INVALID, word, **kw)
        # dependent guesses inside the first block, and inside the second (the same two vectors after the projection)
        g = er.guesses(L, 6)
        g[2] = g[0]
        refused(pkg, mg, L, INVALID, "block 0", nev=6, x0=g)
        g = er.guesses(L, 6)
        g[5] = g[4]
        rc, msg = raw(pkg, mg, nev=6, x0=g, max_iters=80)
        assert rc == INVALID and "block 1" in msg and "dependent" in msg, (rc, msg)
        theta, X, stats, hists = mg.eigs_many(6, x0=er.guesses(L, 6), tol=1e-8, max_iters=120)
        assert all(st.converged for st in stats)


def test_a_short_history_slot_is_not_overrun(pkg):
    L, Lc, cap, nev = 6, 3, 3, 6
    with make(pkg, "gal", "const0.5", L, Lc) as mg:
        want = mg.eigs_many(nev, x0=er.guesses(L, nev), tol=1e-8, max_iters=120)
        x = er.guesses(L, nev)
        lam = np.zeros(nev)
        stats = (pkg.Stats * nev)()
        flat = np.full(nev * cap + 5, -7.0)
        rc = pkg.lib().mgx_eigs_many(mg._h, nev, x.ctypes.data, lam.ctypes.data_as(C.POINTER(C.c_double)), 1e-8, 120, stats,
                                     flat.ctypes.data_as(C.POINTER(C.c_double)), cap)
        assert rc == 0 and np.array_equal(lam, want[0]) and np.array_equal(x, want[1])
        for j in range(nev):
            assert stats[j].history_len == len(want[3][j]) > cap
            assert np.array_equal(flat[j * cap: (j + 1) * cap], want[3][j][:cap])
        assert np.all(flat[nev * cap:] == -7.0)


# ---- 8. mgx_time_eig_project -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_time_eig_project(pkg, f32):
    """the workspace columns cannot be read through the API: what is held is the handle's own grids and graphs and the bits of
    the calls that follow (SUB with zeroed coefficients computes W - 0 Y_i, W's own bits)"""
    L, Lc = 7, 3
    tol = max(1e-3, 40 * U32 * er.lambda_max_bound(fine_stencil("const0.5", L)) / er.constant_eigenvalues(L, 0.5, 1)[0]) if f32 else 1e-8
    with make(pkg, "gal", "const0.5", L, Lc, f32=f32) as mg:
        dt = mg.level_dtype(L)
        before = solve_one(mg, rand(L, 11).astype(dt), rand(L, 12).astype(dt), 0.0, 2)
        ms = C.c_double(-1.0)
        assert pkg.lib().mgx_time_eig_project(mg._h, 0, 1, 1, 2, C.byref(ms)) == STATE       # nothing allocated yet
        want = mg.eigs_many(6, x0=er.guesses(L, 6), tol=tol, max_iters=120)
        assert all(st.converged for st in want[2])
        assert pkg.lib().mgx_time_eig_project(mg._h, 0, 4, 4, 2, C.byref(ms)) == STATE       # six slots exist, eight are asked for
        assert mg.time_eig_project(pkg.EIG_PROJECT_DOTS, 2, 4, 2) > 0.0
        mg.eigs_many(13, x0=er.guesses(L, 13), tol=tol, max_iters=1)                         # allocates thirteen slots; ends after block 0
        grids, graphs = snapshot(mg)
        for which in (pkg.EIG_PROJECT_DOTS, pkg.EIG_PROJECT_SUB):
            for m in (4, 9):
                for k in (1, 4):
                    t = mg.time_eig_project(which, m, k, 2)
                    assert np.isfinite(t) and t > 0.0, (which, m, k, t)
        for bad in ((2, 1, 1, 2), (-1, 1, 1, 2), (0, 0, 1, 2), (0, 16, 1, 2), (0, 1, 0, 2), (0, 1, 5, 2), (0, 1, 1, 0)):
            assert pkg.lib().mgx_time_eig_project(mg._h, *bad, C.byref(ms)) == INVALID, bad
        assert pkg.lib().mgx_time_eig_project(mg._h, 0, 1, 1, 2, None) == INVALID
        grids1, graphs1 = snapshot(mg)
        assert graphs1 == graphs and all(np.array_equal(a, a1) for a, a1 in zip(grids, grids1))
        again = mg.eigs_many(6, x0=er.guesses(L, 6), tol=tol, max_iters=120)
        assert same(again, want)
        assert_column(solve_one(mg, rand(L, 11).astype(dt), rand(L, 12).astype(dt), 0.0, 2), before, "mgx_solve after the timing")
