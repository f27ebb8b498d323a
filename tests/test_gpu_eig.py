"""GPU tests of mgx_eigs and mgx_time_eig_pass (include/mgx.h): the smallest eigenpairs of the finest operator by LOBPCG
around the block cycle (csrc/mgx_eig.hpp).

Every case recomputes r_j = A x_j - theta_j x_j in numpy, in double, from the vectors the call returned and the operator the
test handed in, and holds the pair to
    |theta_j - lambda_j| <= ||r_j|| + 64 eps lambda_max      (the residual bound of a symmetric A, plus the rounding of a row)
    theta_j >= lambda_j - 64 eps lambda_max                  (a Ritz value is an upper bound)
with lambda_j the j-th exact eigenvalue (closed form or numpy.linalg.eigvalsh of the dense matrix) and eps the unit
spacing of the handle's type: both together show that these are the SMALLEST pairs.  The device runs with max_iters = 2 x the
iteration count of tests/eig_ref.py on the same case and has to converge within it.

Shapes (finest, coarsest): (5, 2) the smallest level on which the strip kernels run; (6, 3) and (7, 3) as the block-solver
tests; (8, 3) in fp64 and (9, 3) in fp32: more than one strip (124 fp64 / 248 fp32 columns per strip).

|X^T X - I|: the bound is 16 x eig_ref's own defect on the same case (fp32: times eps32 / eps64, the same algorithm at
another unit roundoff), with the recorded figures in profiles/eig_kernel_trace_summary.md.

fp32 tolerances: the attainable ||r|| / theta in float is about u32 lambda_max / lambda_min (u32 = 2^-24); tol = 40 x that or
1e-3, whichever is larger: 1e-3 at level 5 (2.5e-5 x 40), 0.25 at level 9."""
import ctypes as C
import functools

import numpy as np
import pytest

import eig_ref as er
import galerkin_ref as gr
import nine_ref as nr
from pcg_ref import contrast_coefficient
from test_gpu_multi import assert_column, handle, solve_one
from test_gpu_refine import BILINEAR, INVALID, OPERATOR, STATE, config, rand

pytestmark = pytest.mark.gpu

EPS64, EPS32, U32 = np.finfo(np.float64).eps, np.finfo(np.float32).eps, 2.0 ** -24
V, W = 0, 1


# ---- cases: (op, operator, finest, coarsest, transfer, cycle, dtype) -------------------------------------------------
def fine_stencil(kind, L, dt=np.float64):
    """the nine arrays of the finest operator as the handle stores them (type dt), in float64"""
    if kind.startswith("const"):
        st = gr.nine(er.constant_stencil(L, float(kind[5:]), dt))
    elif kind.startswith("contrast"):
        st = er.coefficient_stencil(contrast_coefficient(L, float(kind[8:])), dt)
    else:
        st = nr.tensor9(*nr.rotated_tensor(L, 45.0, 0.5), dtype=dt)
    return [np.asarray(a, dtype=np.float64) for a in st]


def make(pkg, op, kind, L, Lc, transfer=BILINEAR, cycle=None, f32=False, **kw):
    if f32:
        kw["dtype"] = pkg.DTYPE_F32
    if not kind.startswith("const"):
        return handle(pkg, L, Lc, op, "rot45" if kind == "rot45" else kind, transfer, cycle, **kw)
    mg = pkg.Multigrid(**config(pkg, L, Lc, pkg.OPERATOR_STENCIL5 if op == "s5" else pkg.OP_GALERKIN, **kw))
    for lv in (range(Lc, L + 1) if op == "s5" else [L]):
        mg.set_stencil(lv, *er.constant_stencil(lv, float(kind[5:]), mg.level_dtype(lv)))
    if op == "gal":
        mg.build_galerkin(transfer)
    if cycle is not None:
        mg.set_cycle(cycle)
    return mg


@functools.lru_cache(maxsize=None)
def reference(op, kind, L, Lc, transfer=BILINEAR, cycle=V, nev=4, tol=1e-8):
    """eig_ref on the case, computed once: (fine stencil, result)"""
    fine = fine_stencil(kind, L)
    st = (lambda lv: er.constant_stencil(lv, float(kind[5:]))) if op == "s5" else fine
    h = er.hierarchy(op, st, L, Lc, transfer, cycle)
    res = er.lobpcg(lambda v: er.apply(fine, v), er.preconditioner(h), er.guesses(L, nev), tol, 200)
    assert not res.reason and all(res.converged), (op, kind, L, Lc, res.reason)
    return fine, res


@functools.lru_cache(maxsize=None)
def exact_values(kind, L, count=4):
    if kind.startswith("const"):
        return er.constant_eigenvalues(L, float(kind[5:]), count)
    assert L <= 5
    return np.linalg.eigvalsh(gr.dense(fine_stencil(kind, L)))[:count]


def run(mg, L, nev, tol, max_iters, x0=None):
    x0 = er.guesses(L, nev) if x0 is None else x0
    return mg.eigs(nev, x0=x0, tol=tol, max_iters=max_iters)


def check(name, fine, theta, X, stats, hists, exact, tol, ref_defect, f32=False, converged=True):
    """the self-consistency of every case and the two inequalities against the exact eigenvalues; returns the defect"""
    eps = EPS32 if f32 else EPS64
    lmax = er.lambda_max_bound(fine)
    nev = len(theta)
    assert X.dtype == (np.float32 if f32 else np.float64) and X.shape[0] == nev
    assert np.all(np.diff(theta) >= 0), theta
    defect = er.orthonormality_defect(X)
    bound = 16 * ref_defect * (EPS32 / EPS64 if f32 else 1.0)
    print(f"{name}: |X^T X - I| {defect:.2e}, bound {bound:.2e} (eig_ref's own {ref_defect:.2e})")
    assert defect <= bound, (name, defect, bound)
    for j in range(nev):
        x = X[j].astype(np.float64)
        r = float(np.linalg.norm(er.apply(fine, x) - theta[j] * x))
        assert abs(stats[j].final_residual - r) <= (64 * EPS32 * lmax if f32 else 1e-12), (name, j, stats[j].final_residual, r)
        assert stats[j].final_residual == hists[j][-1] and stats[j].initial_residual == hists[j][0] and stats[j].history_len == len(hists[j])
        assert abs(np.linalg.norm(x) - 1.0) <= bound
        if converged:
            assert stats[j].converged == 1 and hists[j][-1] <= tol * theta[j], (name, j, hists[j][-1], theta[j])
        assert abs(theta[j] - exact[j]) <= r + 64 * eps * lmax, (name, j, theta[j], exact[j], r)
        assert theta[j] >= exact[j] - 64 * eps * lmax, (name, j, theta[j], exact[j])
    assert len({st.seconds for st in stats}) == 1 and stats[0].seconds > 0.0
    return defect


def solve_case(pkg, op, kind, L, Lc, transfer=BILINEAR, cycle=None, nev=4, tol=1e-8, f32=False):
    fine, ref = reference(op, kind, L, Lc, transfer, V if cycle is None else cycle, nev, tol)
    with make(pkg, op, kind, L, Lc, transfer, cycle, f32) as mg:
        theta, X, stats, hists = run(mg, L, nev, tol, 2 * ref.iterations)
    its = len(hists[0]) - 1
    name = f"{op} {kind} {L}..{Lc} transfer {transfer} cycle {cycle} nev {nev} {'f32' if f32 else 'f64'} tol {tol:g}"
    print(f"{name}: iterations {its} (eig_ref {ref.iterations}), cycles {[st.cycles for st in stats]} (eig_ref {ref.cycles})")
    assert all(len(h) == its + 1 for h in hists) and its <= 2 * ref.iterations
    fine_t = fine_stencil(kind, L, np.float32) if f32 else fine
    check(name, fine_t, theta, X, stats, hists, exact_values(kind, L, nev), tol, er.orthonormality_defect(ref.X), f32)
    return theta, X, stats, hists, ref


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 2), (6, 3), (7, 3), (8, 3)], ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("op", ["gal", "s5"])
@pytest.mark.parametrize("kind", ["const1.0", "const0.5"])
def test_closed_form_eigenvalues(pkg, kind, op, shape):
    """const1.0 is the Poisson operator: lambda_1 = lambda_2 is a degenerate pair inside the block; const0.5 is simple"""
    solve_case(pkg, op, kind, *shape)


# ---- 2. the dense reference at (5, 2) --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,transfer,cycle", [("contrast10", BILINEAR, None), ("contrast10", OPERATOR, None), ("contrast100", BILINEAR, None),
                                                 ("contrast100", OPERATOR, None), ("rot45", BILINEAR, W), ("rot45", OPERATOR, None)])
def test_against_eigvalsh_at_level_5(pkg, kind, transfer, cycle):
    solve_case(pkg, "gal", kind, 5, 2, transfer, cycle)


# ---- 4. every K instance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nev", [1, 2, 3])
def test_fewer_columns(pkg, nev):
    """nev = 1: the cycle runs the single-column kernels"""
    solve_case(pkg, "gal", "const0.5", 6, 3, nev=nev)


# ---- 6. soft locking -------------------------------------------------------------------------------------------------------
def test_soft_locking(pkg):
    """Poisson at (7, 3): eig_ref locks the four columns in different iterations (tests/test_eig_cpu.py checks that on the
    CPU), so a locked column has had fewer cycles than the call had iterations"""
    _, _, stats, hists, ref = solve_case(pkg, "gal", "const1.0", 7, 3)
    its = len(hists[0]) - 1
    assert min(ref.cycles) < ref.iterations
    assert all(st.cycles <= its for st in stats) and min(st.cycles for st in stats) < its, ([st.cycles for st in stats], its)
    assert all(st.fine_updates == st.cycles * 4 * 127.0 * 127.0 for st in stats)         # V(2,2): four finest sweeps per cycle


# ---- 7. the handle is left alone -------------------------------------------------------------------------------------------
def snapshot(pkg, mg):
    """U and B of every level, R of the levels that have one (None elsewhere), and the number of cached graphs"""
    grids = []
    for lv in range(mg.cfg.coarsest_level, mg.cfg.finest_level + 1):
        for which in (pkg.VEC_U, pkg.VEC_B, pkg.VEC_R):
            try:
                grids.append(mg.get_level(lv, which))
            except pkg.MgxError:
                assert which == pkg.VEC_R
                grids.append(None)
    return grids, mg.graphs_cached()


def same_grids(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))


def test_the_handle_is_left_as_it_was(pkg):
    L, Lc = 6, 3
    b, u0 = rand(L, 11), rand(L, 12)
    bb, uu = np.stack([rand(L, 20 + j) for j in range(3)]), np.stack([rand(L, 30 + j) for j in range(3)])
    with handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as mg, handle(pkg, L, Lc, "gal", "contrast10", OPERATOR) as twin:
        for h in (mg, twin):
            solve_one(h, b, u0, 0.0, 3)
            h.set_rhs(b)
            h.set_guess(u0)
            h.solve_gcr(tol=0.0, max_iters=3, restart=2)
            h.solve_multi_gcr(bb, uu, tol=0.0, max_iters=3, restart=2)
        grids, graphs = snapshot(pkg, mg)
        theta, X, stats, hists = run(mg, L, 4, 1e-8, 60)
        assert all(st.converged for st in stats)
        grids1, graphs1 = snapshot(pkg, mg)
        assert graphs1 == graphs and same_grids(grids, grids1) and sum(g is not None for g in grids) >= 2 * (L - Lc + 1) + 1
        (st, hist), (st0, hist0) = mg.solve(tol=0.0, max_cycles=3), twin.solve(tol=0.0, max_cycles=3)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, twin.get_solution()), "mgx_solve after mgx_eigs")
        m, m0 = mg.solve_multi_gcr(bb, uu, tol=0.0, max_iters=4, restart=3), twin.solve_multi_gcr(bb, uu, tol=0.0, max_iters=4, restart=3)
        for j in range(3):
            assert_column((m[0][j], m[1][j], m[2][j]), (m0[0][j], m0[1][j], m0[2][j]), f"mgx_solve_multi_gcr after mgx_eigs, column {j}")
        (st, hist), (st0, hist0) = mg.solve_gcr(tol=0.0, max_iters=3, restart=2), twin.solve_gcr(tol=0.0, max_iters=3, restart=2)
        assert_column((st, hist, mg.get_solution()), (st0, hist0, twin.get_solution()), "mgx_solve_gcr after mgx_eigs")
        # and the other way round: the eigenpairs do not depend on what the block solver left in the shared columns
        again = run(mg, L, 4, 1e-8, 60)
        assert np.array_equal(again[0], theta) and np.array_equal(again[1], X)


# ---- 8. determinism, and the workspace grows -------------------------------------------------------------------------------
def test_two_calls_return_the_same_bits_and_the_workspace_grows(pkg):
    L, Lc = 6, 3
    with make(pkg, "gal", "rot45", L, Lc, OPERATOR) as mg, make(pkg, "gal", "rot45", L, Lc, OPERATOR) as big:
        two = run(mg, L, 2, 1e-8, 80)
        four = run(mg, L, 4, 1e-8, 80)                                    # grows from two columns to four
        again = run(mg, L, 4, 1e-8, 80)
        fresh = run(big, L, 4, 1e-8, 80)                                  # a handle that starts at four
        for other in (again, fresh):
            assert np.array_equal(four[0], other[0]) and np.array_equal(four[1], other[1])
            assert all(np.array_equal(h, h1) for h, h1 in zip(four[3], other[3]))
            assert [st.cycles for st in four[2]] == [st.cycles for st in other[2]]
        assert all(st.converged for st in two[2] + four[2])
        assert np.allclose(two[0], four[0][:2], rtol=1e-7, atol=0)


# ---- 9. F32 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 2), (9, 3)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_f32(pkg, shape):
    L, Lc = shape
    lam = er.constant_eigenvalues(L, 1.0, 1)[0]
    attainable = U32 * er.lambda_max_bound(fine_stencil("const1.0", L)) / lam
    tol = max(1e-3, 40 * attainable)
    print(f"level {L}: attainable ||r|| / theta in float {attainable:.2e}, tol {tol:.3g}")
    assert (L, tol) in ((5, 1e-3), (9, tol)) and (L == 5 or 0.2 < tol < 0.3)
    solve_case(pkg, "gal", "const1.0", L, Lc, tol=tol, f32=True)


# ---- 10. refusals and edges --------------------------------------------------------------------------------------------------
def raw(pkg, mg, nev=2, x=True, lam=True, tol=1e-8, max_iters=2, x0=None):
    n = mg.n()
    dt = mg.level_dtype(mg.cfg.finest_level)
    xx = (er.guesses(mg.cfg.finest_level, max(nev, 1)) if x0 is None else x0).astype(dt)
    ll = np.zeros(max(nev, 1))
    assert xx.shape[1:] == (n, n)
    rc = pkg.lib().mgx_eigs(mg._h, nev, xx.ctypes.data if x else None, ll.ctypes.data_as(C.POINTER(C.c_double)) if lam else None, tol, max_iters,
                            None, None, 0)
    return rc, pkg.lib().mgx_last_error(mg._h).decode()


def refused(pkg, mg, L, status, word=None, **kw):
    b = rand(L, 5).astype(mg.level_dtype(L))
    before = solve_one(mg, b, np.zeros_like(b), 0.0, 2)
    rc, msg = raw(pkg, mg, **kw)
    assert rc == status and msg and (word is None or word in msg), (rc, msg)
    if status == STATE:
        ms = C.c_double(-1.0)
        assert pkg.lib().mgx_time_eig_pass(mg._h, 0, 1, 2, C.byref(ms)) == STATE
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


def test_unbuilt_hierarchies_and_bad_arguments_in_their_order(pkg):
    L, Lc = 6, 3
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OP_GALERKIN)) as mg:
        rc, msg = raw(pkg, mg)
        assert rc == STATE and "not set" in msg, msg
        mg.set_coefficient(contrast_coefficient(L, 10.0))
        rc, msg = raw(pkg, mg)
        assert rc == STATE and "not built" in msg, msg
        # MGX_ERR_INVALID comes before MGX_ERR_STATE ...
        assert raw(pkg, mg, nev=0)[0] == INVALID
        mg.build_galerkin()
        # ... and in the stated order: every call below is wrong in the named argument and in all that follow it
        nan = float("nan")
        for kw, word in ((dict(nev=0, x=False, lam=False, tol=nan, max_iters=-1), "nev"),
                         (dict(nev=pkg.MAX_RHS + 1, x=False, lam=False, tol=nan, max_iters=-1), "nev"),
                         (dict(x=False, tol=nan, max_iters=-1), "NULL"), (dict(lam=False, tol=-1.0, max_iters=-1), "NULL"),
                         (dict(tol=nan, max_iters=-1), "tol"), (dict(tol=-1.0, max_iters=-1), "tol"), (dict(max_iters=-1), "max_iters")):
            refused(pkg, mg, L, INVALID, word, **kw)
        g = er.guesses(L, 3)
        g[2] = g[0]
        refused(pkg, mg, L, INVALID, "dependent", nev=3, x0=g)
        ms = C.c_double(-1.0)
        assert pkg.lib().mgx_time_eig_pass(mg._h, 0, 4, 2, C.byref(ms)) == STATE           # three columns exist
        theta, X, stats, hists = run(mg, L, 4, 1e-8, 80)
        assert all(st.converged for st in stats)


def test_no_iterations_returns_a_rotation_of_the_orthonormalised_guesses(pkg):
    L, Lc = 6, 3
    g = er.guesses(L, 3)
    with make(pkg, "gal", "const0.5", L, Lc) as mg:
        theta, X, stats, hists = run(mg, L, 3, 1e-8, 0, g)
    assert [len(h) for h in hists] == [1, 1, 1] and [st.cycles for st in stats] == [0, 0, 0] and [st.converged for st in stats] == [0, 0, 0]
    assert er.orthonormality_defect(X) <= 64 * EPS64 and np.all(np.diff(theta) >= 0)
    Q = np.linalg.qr(g.reshape(3, -1).T)[0]
    V3 = X.reshape(3, -1).T
    assert np.max(np.abs(V3 - Q @ (Q.T @ V3))) <= 64 * EPS64                      # in the span of the guesses
    fine = fine_stencil("const0.5", L)
    ritz = np.linalg.eigvalsh(Q.T @ np.stack([er.apply(fine, q.reshape(g.shape[1:])).ravel() for q in Q.T], axis=1))
    assert np.allclose(theta, ritz, rtol=1e-12, atol=0)


def test_a_short_history_slot_is_not_overrun(pkg):
    L, Lc, cap = 6, 3, 3
    with make(pkg, "gal", "const0.5", L, Lc) as mg:
        want = run(mg, L, 4, 1e-8, 60)
        x = er.guesses(L, 4)
        lam = np.zeros(4)
        stats = (pkg.Stats * 4)()
        flat = np.full(4 * cap + 5, -7.0)
        rc = pkg.lib().mgx_eigs(mg._h, 4, x.ctypes.data, lam.ctypes.data_as(C.POINTER(C.c_double)), 1e-8, 60, stats,
                                flat.ctypes.data_as(C.POINTER(C.c_double)), cap)
        assert rc == 0 and np.array_equal(lam, want[0]) and np.array_equal(x, want[1])
        for j in range(4):
            assert stats[j].history_len == len(want[3][j]) > cap
            assert np.array_equal(flat[j * cap: (j + 1) * cap], want[3][j][:cap])
        assert np.all(flat[4 * cap:] == -7.0)


def test_an_indefinite_operator_ends_with_a_reason(pkg):
    """a negative centre at one point: e_i^T A e_i < 0, so the smallest Ritz value turns negative within a few iterations
    (eig_ref: seven) or the cycle's D^-1 breaks the basis - either way MGX_OK, converged = 0 and the reason"""
    L, Lc = 6, 3
    st = er.constant_stencil(L, 1.0)
    st[0][20, 30] = -4.0
    with pkg.Multigrid(**config(pkg, L, Lc, pkg.OP_GALERKIN)) as mg:
        mg.set_stencil(L, *st)
        mg.build_galerkin()
        theta, X, stats, hists = run(mg, L, 4, 1e-8, 100)
        msg = pkg.lib().mgx_last_error(mg._h).decode()
        assert "mgx_eigs" in msg and ("not a positive finite number" in msg or "rank deficient" in msg), msg
        assert not any(st.converged for st in stats) and len(hists[0]) < 100
        # the handle goes on
        mg.set_stencil(L, *er.constant_stencil(L, 1.0))
        mg.build_galerkin()
        assert all(st.converged for st in run(mg, L, 4, 1e-8, 80)[2])


# ---- mgx_time_eig_pass -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contrast10", "rot45"])
def test_time_eig_pass(pkg, kind):
    L, Lc = 7, 3
    with handle(pkg, L, Lc, "gal", kind) as mg:
        before = solve_one(mg, rand(L, 11), rand(L, 12), 0.0, 2)
        want = run(mg, L, 4, 1e-8, 80)
        for which in (pkg.EIG_PASS_GRAM, pkg.EIG_PASS_COMBINE, pkg.EIG_PASS_RESIDUAL, pkg.EIG_PASS_APPLY):
            for nev in (1, 2, 3, 4):
                ms = mg.time_eig_pass(which, nev, 2)
                assert np.isfinite(ms) and ms > 0.0, (which, nev, ms)
        for bad in ((4, 1, 2), (-1, 1, 2), (0, 0, 2), (0, 5, 2), (0, 1, 0)):
            ms = C.c_double(-1.0)
            assert pkg.lib().mgx_time_eig_pass(mg._h, *bad, C.byref(ms)) == INVALID
        again = run(mg, L, 4, 1e-8, 80)
        assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
        assert_column(solve_one(mg, rand(L, 11), rand(L, 12), 0.0, 2), before, "mgx_solve after the timing")
