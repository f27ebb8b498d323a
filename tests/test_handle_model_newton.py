"""Keeps the zero-order term, the theta steps and Newton of tests/handle_model.py honest (no GPU): set_reaction, theta_steps,
newton and newton_steps are held bit for bit to reference hierarchies built INDEPENDENTLY from the shifted operator
(tests/galerkin_ref.py, opdep_ref.py, cheby_ref.py, nine_ref.py, colour_ref.py) with tests/theta_ref.py's steps, tests/newton_ref.py's
newton and tests/newton_steps_ref.py's steps run around them, in double and in float; every refusal and every exit that
touches nothing is entered.  The sequences of tests/test_gpu_handle_newton.py are drawn and walked here without a device:
what the stage promises, and the conditions the GPU bounds rest on."""
import numpy as np
import pytest

import cheby_ref
import colour_ref as cf
import galerkin_ref as gr
import gcr_ref
import handle_model as hm
import newton_ref as nf
import newton_steps_ref as nsr
import nine_ref as nr
import opdep_ref as od
import pcg_ref
import test_gpu_handle_newton as gn
import test_gpu_handle_state as gs
import theta_ref as tr
from test_handle_model import contrast, data

L, LC = 6, 3
KW = dict(mu1=2, mu2=1)
NAMES = ["jacobi-bilinear", "jacobi-operator", "chebyshev-operator", "nine-jacobi", "nine-chebyshev-operator", "colour-sgs"]
DTYPES = [np.float64, np.float32]


def references(po, name, dt):
    """(cfg of the model, how the model is given its operator and hierarchy, make(st) -> a reference hierarchy built from the
    finest operator st - nine arrays, of which a five-point reference takes the first five - in dt)"""
    base = dict(finest_level=L, coarsest_level=LC, mu0=0, mu1=2, mu2=1, schedule=hm.V, op=hm.GALERKIN, dtype=hm.F64 if dt == np.float64 else hm.F32)
    a = contrast(L, 10.0, 4)
    give5 = lambda t: (lambda m: (m.set_coefficient(a), m.build_galerkin(t)))
    give9 = lambda t: (lambda m: (m.set_tensor(*hm.tensor_nodes(L, "rot45")), m.build_galerkin(t)))
    five = lambda cls, *pre: (lambda st: cls(*pre, po, st[:5], L, LC, dtype=dt, **KW))
    nine = lambda cls, *pre: (lambda st: cls(*pre, po, st, L, LC, dtype=dt, **KW))
    if name == "jacobi-bilinear":
        return base, give5(hm.BILINEAR), five(gr.Hierarchy)
    if name == "jacobi-operator":
        return base, give5(hm.OPERATOR), five(od.Hierarchy)
    if name == "chebyshev-operator":
        return dict(base, smoother=hm.CHEBYSHEV), give5(hm.OPERATOR), five(cheby_ref.OpdepHierarchy)
    if name == "nine-jacobi":
        return base, give9(hm.BILINEAR), nine(nr.Hierarchy)
    if name == "nine-chebyshev-operator":
        return dict(base, smoother=hm.CHEBYSHEV), give9(hm.OPERATOR), nine(nr.ChebyOpdepHierarchy)
    if name == "colour-sgs":
        return dict(base, smoother=hm.COLOR_SGS), give5(hm.BILINEAR), five(cf.Hierarchy, hm.COLOR_SGS)
    raise KeyError(name)


def term(n, seed, dt, lo=0.05, hi=0.5):
    return (lo + (hi - lo) * np.random.RandomState(seed).uniform(0.0, 1.0, (n, n))).astype(dt)


def same_hierarchy(h, ref):
    for lv in ref.st:
        assert len(h.st[lv]) == len(ref.st[lv])
        for x, y in zip(h.st[lv], ref.st[lv]):
            assert x.dtype == y.dtype and np.array_equal(x, y), lv


def model(po, name, dt):
    cfg, give, make = references(po, name, dt)
    m = hm.HandleModel(po, **cfg)
    give(m)
    return m, make


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_set_reaction_gives_the_hierarchy_of_the_shifted_operator(po, name, dt):
    """slot 0 is c0 + d rounded once in the working type; the hierarchy is invalid until the build and then that of a fresh
    reference built from the shifted operator, level by level, with its solve; a second call replaces the term; None restores
    c0 bit for bit and invalidates; None with none set changes nothing; an operator change drops the term for good"""
    m, make = model(po, name, dt)
    n, transfer = m.n(L), m.transfer
    A0 = [x.copy() for x in m.base_operator()]
    u, b = data(po, L, dt, 31)
    d1, d2 = term(n, 1, dt), term(n, 2, dt, 0.5, 4.0)
    for d in (d1, d2):                                      # the second call replaces the first
        m.set_reaction(d)
        assert m._finest()[0].dtype == dt and np.array_equal(m._finest()[0], A0[0] + d) and np.array_equal(m.get_reaction(), d)
        assert all(np.array_equal(x, y) for x, y in zip(m.base_operator(), A0))
        assert m.h is None
        with pytest.raises(RuntimeError):
            m.vcycle()
        m.build_galerkin(transfer)
        ref = make(tr.shift(A0, d))
        same_hierarchy(m.h, ref)
        m.set_guess(u)
        m.set_rhs(b)
        st, h = m.solve(tol=0.0, max_cycles=3)
        u_ref, h_ref = ref.solve(b, u, tol=0.0, max_cycles=3)
        assert np.array_equal(m.U[L], u_ref) and np.array_equal(h, h_ref)
    m.set_reaction(None)
    assert m.h is None and m.d is None and np.array_equal(m._finest()[0], A0[0])
    with pytest.raises(RuntimeError):
        m.get_reaction()
    m.build_galerkin(transfer)
    same_hierarchy(m.h, make(A0))
    h = m.h
    m.set_reaction(None)                                    # nothing to remove: the hierarchy stays
    assert m.h is h and m.transfer == transfer
    # an operator change drops the term: a later None is a no-op and brings no old centre back
    m.set_reaction(d1)
    if m.st9 is not None:
        m.set_tensor(*hm.tensor_nodes(L, "smooth9"))
    else:
        m.set_coefficient(contrast(L, 100.0, 5))
    new = m._finest()[0].copy()
    assert m.d is None and m.c0 is None and not np.array_equal(new, A0[0])
    m.set_reaction(None)
    assert np.array_equal(m._finest()[0], new) and np.array_equal(m.base_operator()[0], new)
    with pytest.raises(RuntimeError):
        m.get_reaction()
    m.build_galerkin(transfer)
    same_hierarchy(m.h, make(m.base_operator()))


def test_the_float_model_is_given_the_float_of_the_stored_centre(po):
    """_float_model: float32 of the stored, shifted centre - one rounding of c0 + d in double, then to float - not
    float32(c0) + float32(d); with gs.reaction_term the two differ at more than a quarter of the points, so a float copy
    assembled from the parts would show in the first refine after a set_reaction"""
    m, make = model(po, "jacobi-operator", np.float64)
    c0 = m.base_operator()[0].copy()
    d = gs.reaction_term(c0, 7001)
    assert np.all(d >= 0.04 * c0) and np.all(d <= 0.26 * c0)
    m.set_reaction(d)
    m.build_galerkin(hm.OPERATOR)
    f = m._float_model()
    stored = (c0 + d).astype(np.float32)
    parts = c0.astype(np.float32) + d.astype(np.float32)
    assert np.array_equal(f._finest()[0], stored) and f.d is None
    assert np.mean(stored != parts) >= 0.25, np.mean(stored != parts)
    ref32 = od.Hierarchy(po, [x.astype(np.float32) for x in tr.shift(m.base_operator(), d)[:5]], L, LC, dtype=np.float32, **KW)
    same_hierarchy(f.h, ref32)
    m.set_reaction(None)
    m.build_galerkin(hm.OPERATOR)
    assert np.array_equal(m._float_model()._finest()[0], c0.astype(np.float32))


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_theta_steps_equal_theta_ref_around_an_independent_hierarchy(po, name, dt):
    """iterates, right-hand sides, histories and statistics of theta = 1 / 0.5 with and without a source, bit for bit;
    a step that does not converge is the last one; nsteps = 0 moves nothing"""
    m, make = model(po, name, dt)
    n = m.n(L)
    A0 = [x.copy() for x in m.base_operator()]
    d, transfer = term(n, 3, dt), m.transfer
    m.set_reaction(d)
    m.build_galerkin(transfer)
    S9 = tr.shift(A0, d)
    ref = make(S9)
    u0, g = data(po, L, dt, 41)
    tol = 1e-6 if dt == np.float64 else 1e-3
    for theta, src in ((1.0, g), (0.5, None), (0.5, g)):
        hists = []

        def solve(b, u):
            x, h = ref.solve(b, u, tol=tol, max_cycles=30)
            hists.append(h)
            return x

        want = tr.steps(S9, d, u0, src, theta, 2, solve)
        m.set_guess(u0)
        done, sts, hs = m.theta_steps(theta, 2, src, hm.STEP_SOLVE, tol, 30)
        assert done == 2 and np.array_equal(m.U[L], want[-1]) and m.U[L].dtype == dt
        assert np.array_equal(m.B[L], tr.rhs_pass(None if theta == 1.0 else tr.apply(S9, want[0]), want[0], d, src, theta))
        assert all(np.array_equal(x, y) for x, y in zip(hs, hists)) and all(s["converged"] == 1 and s["cycles"] == len(h) - 1 for s, h in zip(sts, hs))
    # one cycle per step under a tolerance one cycle does not reach: the first step is the last
    m.set_guess(u0)
    done, sts, hs = m.theta_steps(0.5, 3, g, hm.STEP_SOLVE, 1e-12, 1)
    x, h = ref.solve(tr.rhs_pass(tr.apply(S9, u0), u0, d, g, 0.5), u0, tol=1e-12, max_cycles=1)
    assert done == 1 and sts[0]["converged"] == 0 and np.array_equal(m.U[L], x) and np.array_equal(hs[0], h)
    before = (m.U[L], m.B[L], m.h)
    assert m.theta_steps(0.5, 0, g) == (0, [], []) and m.U[L] is before[0] and m.B[L] is before[1] and m.h is before[2]


def test_theta_steps_run_the_krylov_solvers_of_the_model(po):
    """MGX_STEP_GCR: gcr_ref.gcr around the reference's cycle and operator, from the time level; MGX_STEP_REFINE_GCR: the
    model's own solve_refine_gcr from the same state"""
    m, make = model(po, "jacobi-bilinear", np.float64)
    n = m.n(L)
    A0 = [x.copy() for x in m.base_operator()]
    d = term(n, 4, np.float64)
    m.set_reaction(d)
    m.build_galerkin(hm.BILINEAR)
    S9 = tr.shift(A0, d)
    ref = make(S9)
    u0, g = data(po, L, np.float64, 43)
    A, M = pcg_ref.Operator(S9[:5], np.float64), gcr_ref.cycle_preconditioner(ref)
    want = tr.steps(S9, d, u0, g, 0.5, 2, lambda b, u: gcr_ref.gcr(A, M, b, u, tol=1e-6, max_iters=20, restart=3)[0])
    m.set_guess(u0)
    done, sts, hs = m.theta_steps(0.5, 2, g, hm.STEP_GCR, 1e-6, 20, 3)
    assert done == 2 and np.array_equal(m.U[L], want[-1]) and all(s["converged"] for s in sts)
    m.set_guess(u0)
    done, sts, hs = m.theta_steps(0.5, 1, g, hm.STEP_REFINE_GCR, 1e-6, 20, 3)
    b = m.B[L]
    u1 = m.U[L]
    m.set_guess(u0)
    st, h = m.solve_refine_gcr(tol=1e-6, max_iters=20, restart=3)
    assert np.array_equal(b, tr.rhs_pass(tr.apply(S9, u0), u0, d, g, 0.5)) and np.array_equal(m.U[L], u1) and np.array_equal(h, hs[0]) and st == sts[0]


def newton_reference(po, make, A0, kap, f, p, u0, iters, tol, max_newton, max_backtracks, mass=None, theta=None, nsteps=None, g=None):
    """newton_ref.newton (mass None) or newton_steps_ref.steps around a FRESH reference hierarchy per linear solve; also the
    right-hand side of every linear solve"""
    rhs = []

    def solve(S9, b, d, k):
        rhs.append(b)
        return make(S9).solve(b, np.zeros_like(b), tol=0.0, max_cycles=iters)

    if mass is None:
        return nf.newton(A0, kap, f, p, u0, solve, tol, max_newton, max_backtracks, norm=po.norm2), rhs
    return nsr.steps(A0, kap, mass, g, p, u0, theta, nsteps, solve, tol, max_newton, max_backtracks, norm=po.norm2), rhs


def coarse_after(po, name, dt, d, b, iters):
    """the coarse levels of a fresh model after the linear solve of the Jacobian A0 + diag(d) from a zero guess"""
    m, _ = model(po, name, dt)
    t = m.transfer
    m.set_reaction(d)
    m.build_galerkin(t)
    m.set_rhs(b)
    m.solve(tol=0.0, max_cycles=iters)
    return m


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_newton_equals_newton_ref_around_independent_hierarchies(po, name, dt):
    """the iterate, the history, the step lengths, the counts and the records of the linear solves bit for bit; afterwards B
    is the caller's f, the operator A0 + diag(d_k) with its hierarchy built, the coarse levels what the last linear solve
    left; a term set before the call is replaced and is no part of F; the exits without an iteration touch nothing"""
    m, make = model(po, name, dt)
    n, N, transfer = m.n(L), 1 << L, m.transfer
    A0 = [x.copy() for x in m.base_operator()]
    kap, p = np.full((n, n), 50.0 / N ** 2, dtype=dt), (1.0, 0.0, 1.0)
    u0, f = data(po, L, dt, 51)
    k = 4 if dt == np.float64 else 3
    want, rhs = newton_reference(po, make, A0, kap, f, p, u0, 4, 0.0, k, 4)
    assert len(want["hist"]) == k + 1 and want["hist"][-1] < 1e-3 * want["hist"][0]
    for entered_with_a_term in (False, True):
        if entered_with_a_term:
            m.set_reaction(term(n, 5, dt))
            m.build_galerkin(transfer)
        m.set_guess(u0)
        m.set_rhs(f)
        st, h, lin, lam = m.newton(kap, p=p, solver=hm.STEP_SOLVE, lin_tol=0.0, lin_max_iters=4, tol=0.0, max_newton=k, max_backtracks=4)
        assert np.array_equal(m.U[L], want["u"]) and m.U[L].dtype == dt and np.array_equal(m.B[L], f)
        assert np.array_equal(h, want["hist"]) and np.array_equal(lam, want["lam"])
        assert st == dict(iterations=k, converged=0, backtracks=want["backtracks"], linear_iterations=4 * k, failed=False)
        assert len(lin) == k and all(np.array_equal(rec[1], ref_hist) for rec, ref_hist in zip(lin, want["lin"]))
        assert np.array_equal(m.get_reaction(), want["ds"][-1]) and all(np.array_equal(x, y) for x, y in zip(m.base_operator(), A0))
        assert np.array_equal(m._finest()[0], A0[0] + want["ds"][-1]) and m.transfer == transfer
        same_hierarchy(m.h, make(tr.shift(A0, want["ds"][-1])))
        fresh = coarse_after(po, name, dt, want["ds"][-1], rhs[-1], 4)
        for lv in range(LC, L):
            assert np.array_equal(m.U[lv], fresh.U[lv]) and np.array_equal(m.B[lv], fresh.B[lv]), lv
    # no iteration: max_newton = 0, and a tolerance the first norm passes - operator, hierarchy and every level untouched
    for lv in m.levels():
        m.set_level(lv, 0, data(po, lv, dt, 60 + lv)[0])
        m.set_level(lv, 1, data(po, lv, dt, 70 + lv)[0])
    before = ({lv: (m.U[lv], m.B[lv]) for lv in m.levels()}, m.h, m.d, m._finest()[0])
    for tol, k0 in ((0.0, 0), (1.5, 5)):
        st, h, lin, lam = m.newton(kap, p=p, lin_tol=0.0, lin_max_iters=4, tol=tol, max_newton=k0)
        assert st["iterations"] == 0 and st["converged"] == int(tol > 1.0) and len(h) == 1 and not lin and len(lam) == 0
        assert m.h is before[1] and m.d is before[2] and m._finest()[0] is before[3]
        assert all(np.array_equal(m.U[lv], before[0][lv][0]) and np.array_equal(m.B[lv], before[0][lv][1]) for lv in m.levels())


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_a_failed_line_search_leaves_the_last_accepted_iterate(po, dt):
    """newton_ref.backtracking_input with max_backtracks = 0: converged = 0, failed, U the guess, B the caller's f, the operator
    A0 + diag(d_0) built, the coarse levels what the one linear solve left; with halvings allowed the call converges"""
    cfg = dict(finest_level=L, coarsest_level=LC, mu0=0, mu1=2, mu2=1, schedule=hm.V, op=hm.GALERKIN, dtype=hm.F64 if dt == np.float64 else hm.F32)
    A0, kap, f, p, u0 = nf.backtracking_input(L, dt)
    make = lambda st: gr.Hierarchy(po, st[:5], L, LC, dtype=dt, **KW)
    m = hm.HandleModel(po, **cfg)
    m.set_stencil(L, A0[:5])
    m.build_galerkin(hm.BILINEAR)
    want, rhs = newton_reference(po, make, A0, kap, f, p, u0, 6, 1e-10, 5, 0)
    assert want["failed"] and want["backtracks"] == 1 and len(want["hist"]) == 1
    m.set_guess(u0)
    m.set_rhs(f)
    st, h, lin, lam = m.newton(kap, p=p, lin_tol=0.0, lin_max_iters=6, tol=1e-10, max_newton=5, max_backtracks=0)
    assert st == dict(iterations=0, converged=0, backtracks=1, linear_iterations=6, failed=True) and np.array_equal(h, want["hist"]) and len(lin) == 1
    assert np.array_equal(m.U[L], u0) and np.array_equal(m.B[L], f) and np.array_equal(m.get_reaction(), want["ds"][0])
    same_hierarchy(m.h, make(tr.shift(A0, want["ds"][0])))
    fresh = hm.HandleModel(po, **cfg)
    fresh.set_stencil(L, tr.shift(A0, want["ds"][0])[:5])
    fresh.build_galerkin(hm.BILINEAR)
    fresh.set_rhs(rhs[0])
    fresh.solve(tol=0.0, max_cycles=6)
    assert all(np.array_equal(m.U[lv], fresh.U[lv]) and np.array_equal(m.B[lv], fresh.B[lv]) for lv in range(LC, L))
    want, _ = newton_reference(po, make, A0, kap, f, p, u0, 6, 1e-4 if dt == np.float32 else 1e-10, 8, 8)
    m.set_guess(u0)
    st, h, lin, lam = m.newton(kap, p=p, lin_tol=0.0, lin_max_iters=6, tol=1e-4 if dt == np.float32 else 1e-10, max_newton=8, max_backtracks=8)
    assert want["converged"] and want["backtracks"] >= 1 and want["lam"][0] < 1.0
    assert st["converged"] == 1 and np.array_equal(h, want["hist"]) and np.array_equal(lam, want["lam"]) and np.array_equal(m.U[L], want["u"])


@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["jacobi-operator", "nine-chebyshev-operator", "colour-sgs"])
def test_newton_steps_equal_newton_steps_ref_around_independent_hierarchies(po, name, dt):
    """the time levels, r of the last step in B, the histories and the counts of every step bit for bit, theta = 1 and 0.5, with
    and without a source; a step that does not converge is the last one; nsteps = 0 touches nothing, the workspace included"""
    m, make = model(po, name, dt)
    n, N, transfer = m.n(L), 1 << L, m.transfer
    A0 = [x.copy() for x in m.base_operator()]
    kap, p, mass = np.full((n, n), 50.0 / N ** 2, dtype=dt), (1.0, 0.0, 1.0), term(n, 6, dt, 0.25, 1.0)
    u0, g = data(po, L, dt, 53)
    tol = 1e-6 if dt == np.float64 else 1e-3
    assert m.newton_steps(0.5, 0, mass, kap, g, p=p) == (0, [], []) and not m.nwt and not m.nwt_mass
    for theta, src in ((1.0, None), (0.5, g)):
        want, rhs = newton_reference(po, make, A0, kap, None, p, u0, 4, tol, 4, 4, mass=mass, theta=theta, nsteps=2, g=src)
        assert len(want) == 2 and all(o["converged"] for o in want)
        m.set_guess(u0)
        done, sts, hs = m.newton_steps(theta, 2, mass, kap, src, p=p, lin_tol=0.0, lin_max_iters=4, tol=tol, max_newton=4, max_backtracks=4)
        assert done == 2 and np.array_equal(m.U[L], want[-1]["u"]) and np.array_equal(m.B[L], want[-1]["r"]) and m.nwt and m.nwt_mass
        for st, h, o in zip(sts, hs, want):
            assert np.array_equal(h, o["hist"])
            assert st == dict(iterations=len(o["hist"]) - 1, converged=1, backtracks=o["backtracks"], linear_iterations=4 * (len(o["hist"]) - 1), failed=False)
        assert np.array_equal(m.get_reaction(), want[-1]["ds"][-1]) and np.array_equal(m.base_operator()[0], A0[0]) and m.transfer == transfer
        same_hierarchy(m.h, make(tr.shift(A0, want[-1]["ds"][-1])))
    # a budget of one Newton step under that tolerance: the first time step is the last; max_newton = 0: B is r, nothing else moves
    want, _ = newton_reference(po, make, A0, kap, None, p, u0, 4, tol * 1e-3, 1, 4, mass=mass, theta=0.5, nsteps=3, g=g)
    m.set_guess(u0)
    done, sts, hs = m.newton_steps(0.5, 3, mass, kap, g, p=p, lin_tol=0.0, lin_max_iters=4, tol=tol * 1e-3, max_newton=1, max_backtracks=4)
    assert len(want) == 1 and done == 1 and sts[0]["converged"] == 0 and np.array_equal(m.U[L], want[0]["u"]) and np.array_equal(hs[0], want[0]["hist"])
    m.set_guess(u0)
    h, d = m.h, m.d
    done, sts, hs = m.newton_steps(0.5, 3, mass, kap, g, p=p, lin_tol=0.0, lin_max_iters=4, tol=tol, max_newton=0)
    assert done == 1 and sts[0]["iterations"] == 0 and m.h is h and m.d is d and np.array_equal(m.U[L], u0)
    assert np.array_equal(m.B[L], nsr.rhs_pass(A0, kap, mass, g, p, u0, 0.5))


def test_every_refusal_of_the_new_entry_points(po):
    """MGX_ERR_STATE where the device returns it - POISSON, STENCIL5, operator not set, get_reaction and the steps with no term,
    hierarchy not built, the timing calls before their workspace exists, a refining solver on a float handle - and
    MGX_ERR_INVALID on the arguments; a refused call leaves the model as it was"""
    base = dict(finest_level=5, coarsest_level=3, mu0=0, mu1=2, mu2=1, schedule=hm.V)
    n = 31
    d, kap = term(n, 1, np.float64), np.full((n, n), 0.05)
    calls = [lambda m: m.set_reaction(d), lambda m: m.set_reaction(None), lambda m: m.get_reaction(), lambda m: m.theta_steps(0.5, 1),
             lambda m: m.newton(kap), lambda m: m.newton_steps(0.5, 1, d, kap), lambda m: m.time_theta_rhs(0.5, 2),
             lambda m: m.time_newton_pass(0, 2), lambda m: m.time_newton_step_pass(0, 0.5, 2)]
    stencil5 = hm.HandleModel(po, **dict(base, op=hm.STENCIL5))
    stencil5.set_coefficient(contrast(5, 10.0, 1))
    for m in (hm.HandleModel(po, **base), stencil5, hm.HandleModel(po, **dict(base, op=hm.GALERKIN))):   # POISSON, STENCIL5, operator not set
        for call in calls:
            with pytest.raises(RuntimeError):
                call(m)
    m = hm.HandleModel(po, **dict(base, op=hm.GALERKIN))
    m.set_coefficient(contrast(5, 10.0, 1))
    for call in calls[2:]:                                   # no term, no hierarchy, no workspace
        with pytest.raises(RuntimeError):
            call(m)
    m.build_galerkin(hm.BILINEAR)
    for call in (calls[2], calls[3], calls[6], calls[7], calls[8]):
        with pytest.raises(RuntimeError):
            call(m)
    m.set_reaction(d)
    for call in (calls[3], calls[4], calls[5]):              # the term is set, the hierarchy is not built
        with pytest.raises(RuntimeError):
            call(m)
    m.time_theta_rhs(0.5, 2)                                 # (reads the finest operator only: no hierarchy needed, as on the device)
    m.build_galerkin(hm.BILINEAR)
    state = (m.U[5], m.B[5], m.h, m.d)
    bad = [lambda: m.set_reaction(d[:-1]), lambda: m.theta_steps(0.0, 1), lambda: m.theta_steps(1.5, 1), lambda: m.theta_steps(0.5, -1),
           lambda: m.theta_steps(0.5, 1, solver=3), lambda: m.theta_steps(0.5, 1, tol=-1.0), lambda: m.theta_steps(0.5, 1, max_iters=-1),
           lambda: m.theta_steps(0.5, 1, solver=hm.STEP_GCR, restart=9), lambda: m.newton(kap, p=(np.inf, 0.0, 0.0)), lambda: m.newton(kap, solver=-1),
           lambda: m.newton(kap, lin_tol=-1.0), lambda: m.newton(kap, max_newton=-1), lambda: m.newton(kap, max_backtracks=31),
           lambda: m.newton(None), lambda: m.newton(kap[:-1]), lambda: m.newton_steps(0.0, 1, d, kap), lambda: m.newton_steps(0.5, -1, d, kap),
           lambda: m.newton_steps(0.5, 1, None, kap), lambda: m.time_theta_rhs(0.5, 0), lambda: m.time_newton_pass(2, 1),
           lambda: m.time_newton_step_pass(3, 0.5, 1)]
    for call in bad:
        with pytest.raises(ValueError, match="MGX_ERR_INVALID"):
            call()
    assert all(x is y for x, y in zip((m.U[5], m.B[5], m.h, m.d), state))
    m.newton(kap, max_newton=0)                              # allocates the workspace, moves nothing
    m.time_newton_pass(1, 2)
    with pytest.raises(RuntimeError):
        m.time_newton_step_pass(0, 0.5, 2)
    m.newton_steps(0.5, 1, d, kap, max_newton=0)
    m.time_newton_step_pass(2, 0.5, 2)
    f = hm.HandleModel(po, **dict(base, op=hm.GALERKIN, dtype=hm.F32))
    f.set_coefficient(contrast(5, 10.0, 1))
    f.build_galerkin(hm.BILINEAR)
    f.set_reaction(d)
    f.build_galerkin(hm.BILINEAR)
    for call in (lambda: f.theta_steps(0.5, 1, solver=hm.STEP_REFINE_GCR), lambda: f.newton(kap, solver=hm.STEP_REFINE_GCR),
                 lambda: f.newton_steps(0.5, 1, d, kap, solver=hm.STEP_REFINE_GCR)):
        with pytest.raises(ValueError, match="F64 handles only"):
            call()


# ---- the committed GPU sequences on the model alone ------------------------------------------------------------------------
def clone(m):
    """a second model in the state of m (the arrays are never written in place; the lists of the finest operator are)"""
    x = object.__new__(hm.HandleModel)
    x.__dict__ = dict(m.__dict__)
    x.U, x.B, x.R = dict(m.U), dict(m.B), dict(m.R)
    x.st5 = None if m.st5 is None else list(m.st5)
    x.st9 = None if m.st9 is None else list(m.st9)
    return x


def ulp_dot(seed, dt):
    """pcg_ref.dot with every scalar moved independently by up to one ulp of the working type"""
    rng, eps = np.random.RandomState(seed), float(np.finfo(dt).eps)
    return lambda a, b: pcg_ref.dot(a, b) * (1.0 + eps * rng.uniform(-1.0, 1.0))


def decision_margins(norms, tol, max_newton, max_backtracks, runs):
    """the relative margins of every stop and Armijo decision of `runs` Newton iterations in a row, replayed from the norms the
    model formed in their order; also the histories (the caller checks them against the call's)"""
    it, margins, hists = iter(norms), [], []
    rel = lambda a, b: abs(a - b) / b if b > 0.0 else np.inf
    for _ in range(runs):
        h = [next(it)]
        for k in range(max_newton):
            margins.append(rel(h[k], tol * h[0]) if k else (abs(1.0 - tol) / tol if tol > 0.0 else np.inf))
            if h[k] <= tol * h[0]:
                break
            lam, j, accepted = 1.0, 0, False
            while True:
                r = next(it)
                margins.append(rel(r, (1.0 - 1e-4 * lam) * h[k]))
                if nf.armijo(r, lam, h[k]):
                    accepted = True
                    break
                j += 1
                if j > max_backtracks:
                    break
                lam /= 2
            if not accepted:
                break
            h.append(r)
        margins.append(rel(h[-1], tol * h[0]) if len(h) > 1 else np.inf)
        hists.append(h)
    assert next(it, None) is None
    return margins, hists


@pytest.mark.parametrize("name", list(gn.REACTION_CASES))
def test_the_model_walks_the_reaction_sequences_and_meets_the_conditions(po, name):
    """every committed sequence of tests/test_gpu_handle_newton.py on the model alone: the promises of the stages; every call
    does what the stage placed it for (the exits, the second step of (n), the quarter of (i)); and the conditions the GPU
    bounds rest on - never tuned from device output, the data or the seed is changed if one fails:
      1. every Armijo, Newton stop, step stop and inner mgx_solve stop decision of the stage's calls has a relative margin of
         100 x HIST_TOL (double) / 100 x NORM32 (float) at least;
      2. every call with a Krylov solver inside, run a second time from the same state with every scalar of its dots moved by up
         to one ulp of the working type, takes the same decisions and moves an array it writes (and the term it leaves) by at
         most 1/16 of RTOL64 / PCG32_STATE; every double Krylov call of the list ends at or above 1e-6 of its first entry;
      3. no inner history entry of a Newton call with MGX_STEP_REFINE_GCR inside lies, divided by n, within 1e-6 relative of a
         power of two"""
    cfg, seed, envs, options, tol_n, krylov32 = gn.REACTION_CASES[name]
    calls, base = gn.reaction_calls(name)
    gn.assert_base_calls(name, base)
    gn.assert_reaction_calls(calls, cfg)
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    dt = np.float64 if f64 else np.float32
    Lf, Lc = cfg["finest_level"], cfg["coarsest_level"]
    need = 100.0 * (gs.HIST_TOL if f64 else gs.NORM32)
    state_bound = gs.RTOL64 if f64 else gs.PCG32_STATE
    m = hm.HandleModel(po, **cfg)
    dot = ulp_dot(seed, dt)
    low_margin, moved, lowest, near2, quarter = (np.inf, None), (0.0, None), (1.0, None), (np.inf, None), []
    moved_drawn = 0.0
    for i, call in enumerate(calls):
        kind, inner = call[0], gs.inner_solver(call)
        twin = clone(m) if inner not in (None, hm.STEP_SOLVE) or (kind == "solve_gcr" and not f64) else None
        before = (m.h, m.d, dict(m.U), dict(m.B))
        if kind == "set_reaction" and call[1] is not None and f64:
            c0 = m.base_operator()[0]
            d = gs.reaction_term(c0, call[1])
            quarter.append(float(np.mean((c0 + d).astype(np.float32) != c0.astype(np.float32) + d.astype(np.float32))))
        want = gs.apply_model(m, call, Lf)
        same_b = all(np.array_equal(m.B[lv], before[3][lv]) for lv in m.levels())
        untouched = m.h is before[0] and m.d is before[1] and all(np.array_equal(m.U[lv], before[2][lv]) for lv in m.levels())
        margins = []
        if kind == "newton":
            st, h, lin, lam = want
            margins, hists = decision_margins(m.norms, call[5], call[6], call[7], 1)
            assert np.array_equal(hists[0], h)
            assert (st["iterations"] > 0) == gn.iterates(call), (i, call, st)
            if not gn.iterates(call):
                assert untouched and same_b, (i, call)
        elif kind == "newton_steps":
            done, sts, hs = want
            if call[2] > 0:
                margins, hists = decision_margins(m.norms, call[7], call[8], call[9], done)
                assert all(np.array_equal(x, y) for x, y in zip(hists, hs))
            assert (done > 0 and sts[-1]["iterations"] > 0) == gn.iterates(call), (i, call, sts)
            assert done == call[2] or not sts[-1]["converged"]
            if call[2] == 0:
                assert untouched and same_b
            elif not gn.iterates(call):
                assert untouched and done == 1
        elif kind == "theta_steps":
            done, sts, hs = want
            for h in hs:
                margins += [abs(x - call[5] * h[0]) / (call[5] * h[0]) for x in h[1:]]
            if call[2] == 0:
                assert untouched and same_b
            elif call[6] == 1:                             # (n): the first step converges in its one cycle, the second does not
                assert done == 2 and [s["converged"] for s in sts] == [1, 0], (i, call, sts, hs)
            else:
                assert done == call[2] and all(s["converged"] for s in sts), (i, call, sts)
        elif kind in gs.STEP_TIMING or kind in ("get_reaction", "residual_norm") or (kind == "set_reaction" and call[1] is None and before[1] is None):
            assert untouched and same_b
        if margins and min(margins) < low_margin[0]:
            low_margin = (float(min(margins)), (i, call))
        if twin is not None and kind == "solve_gcr":         # the float solve_gcr calls of the drawn list: the existing suite's cap
            twin.solve_gcr(tol=call[1], max_iters=call[2], restart=call[3], dot=dot)
            for lv, x in gs.touched(cfg, call):
                y = m.get_level(lv, x == "B").astype(np.float64)
                dev = float(np.max(np.abs(twin.get_level(lv, x == "B").astype(np.float64) - y))) / float(np.max(np.abs(y)))
                moved_drawn = max(moved_drawn, dev)
        elif twin is not None:                               # condition 2 (and 3)
            a = call[1:]
            if kind == "theta_steps":
                g = None if a[2] is None else gs.field(twin.n(Lf), a[2])
                other = twin.theta_steps(a[0], a[1], g, a[3], a[4], a[5], a[6], dot=dot)
                assert other[0] == want[0] and [s["cycles"] for s in other[1]] == [s["cycles"] for s in want[1]], (i, call)
            elif kind == "newton":
                kap, p = gs.newton_problem(Lf, a[0], twin.wdt)
                other = twin.newton(kap, p=p, solver=a[1], lin_tol=0.0, lin_max_iters=a[2], restart=a[3], tol=a[4], max_newton=a[5], max_backtracks=a[6], dot=dot)
                assert other[0] == want[0] and np.array_equal(other[3], want[3]), (i, call)
            else:
                kap, p = gs.newton_problem(Lf, "cubic", twin.wdt)
                g = None if a[2] is None else gs.field(twin.n(Lf), a[2])
                other = twin.newton_steps(a[0], a[1], np.full_like(kap, gs.STEP_MASS), kap, g, p=p, solver=a[3], lin_tol=0.0, lin_max_iters=a[4],
                                          restart=a[5], tol=a[6], max_newton=a[7], max_backtracks=a[8], dot=dot)
                assert other[0] == want[0] and other[1] == want[1], (i, call)
            pairs = [(twin.get_level(lv, x == "B"), m.get_level(lv, x == "B"), (lv, x)) for lv, x in gs.touched(cfg, call)]
            if kind != "theta_steps":
                pairs.append((twin.d, m.d, "d"))
            for x, y, what in pairs:
                dev = float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64)))) / max(float(np.max(np.abs(y))), 1e-300)
                if dev > moved[0]:
                    moved = (dev, (i, call, what))
            if inner == hm.STEP_REFINE_GCR and kind != "theta_steps":
                for st_lin, h_lin in m.lin:
                    for x in h_lin:
                        mant = np.frexp(x / m.n(Lf))[0]          # in [0.5, 1): a power of two sits at 0.5
                        dist = min(mant / 0.5 - 1.0, 1.0 - mant)
                        if dist < near2[0]:
                            near2 = (float(dist), (i, call))
        if kind in gs.KRYLOV and f64:
            h = want[1]
            if h[-1] / h[0] < lowest[0]:
                lowest = (float(h[-1] / h[0]), (i, call))
    print(f"\n[handle-newton] model alone: {name} calls={len(calls)} (drawn {len(base)}) lowest decision margin={low_margin[0]:.3g} at {low_margin[1]}; "
          f"one-ulp scalars move a written array by {moved[0]:.3g} ({moved[0] / state_bound:.3g} x bound) at {moved[1]}; lowest last/first of a "
          f"double Krylov call={lowest[0]:.3g} at {lowest[1]}; nearest power of two of an inner entry / n={near2[0]:.3g}; "
          f"float32(c0 + d) != float32(c0) + float32(d) at {min(quarter) if quarter else None} of the points at the least")
    assert low_margin[0] >= need, low_margin
    assert moved[0] <= state_bound / 16, moved
    assert moved_drawn <= gs.PCG32_STATE / 4, moved_drawn                      # (tests/test_handle_model.py: the GCR conditions)
    if f64:
        assert 1e-6 <= lowest[0] < 1.0, lowest
        assert near2[0] > 1e-6, near2
        assert quarter and min(quarter) >= 0.25, quarter


def test_the_failed_line_search_list_on_the_model_alone(po):
    """BACKTRACKING_CALLS without a device: the first newton fails its line search at once, the second backtracks and converges;
    both with decision margins of 100 x HIST_TOL at least"""
    cfg, calls = gn.BACKTRACKING_CFG, list(gn.BACKTRACKING_CALLS)
    m = hm.HandleModel(po, **cfg)
    seen = []
    for call in calls:
        want = gs.apply_model(m, call, cfg["finest_level"])
        if call[0] == "newton":
            margins, hists = decision_margins(m.norms, call[5], call[6], call[7], 1)
            assert np.array_equal(hists[0], want[1]) and min(margins) >= 100.0 * gs.HIST_TOL, margins
            seen.append(want)
    (st0, h0, lin0, lam0), (st1, h1, lin1, lam1) = seen
    assert st0 == dict(iterations=0, converged=0, backtracks=1, linear_iterations=6, failed=True) and len(lin0) == 1
    assert st1["converged"] == 1 and st1["backtracks"] >= 1 and lam1[0] < 1.0 and not st1["failed"]
