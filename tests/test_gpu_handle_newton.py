"""One long-lived GALERKIN handle driven through mgx_set_reaction, mgx_theta_steps, mgx_newton, mgx_newton_steps and their
timing entry points BETWEEN the calls of tests/test_gpu_handle_state.py, against the CPU model of a handle
(tests/handle_model.py) after EVERY call.  The features' own tests (test_gpu_theta.py, test_gpu_newton.py,
test_gpu_newton_steps.py) hold a call to the host composition on the same handle: a hierarchy built from a wrongly shifted
centre, a float copy that missed a shift, a base centre kept across an operator change or a source grid read when none was
passed agrees with itself there.  Here the reference is the model, whose hierarchies are built independently
(tests/test_handle_model_newton.py holds its new methods to fresh reference hierarchies bit for bit).

The sequences: a list of tests/test_gpu_handle_state.py's generator (draw_sequence, with its own promises, asserted on that
list) into which reaction_stage places its blocks with a generator of its own, between two plain calls and never between an
operator change or set_cycle and the graph user that follows it.  What every sequence holds by construction is listed in
reaction_stage's docstring, items (a) to (n), and asserted on the final list by assert_reaction_calls; (o), the failed line
search on newton_ref.backtracking_input, is BACKTRACKING_CALLS, a list written by hand for a handle of its own.

What is compared (tests/test_gpu_handle_state.py: step, step_checks):
  * U and B of every level after every call, bit for bit - the setters, the timing calls, and mgx_theta_steps, mgx_newton and
    mgx_newton_steps under MGX_STEP_SOLVE, with steps_done, every iteration count, the step lengths and the backtracks equal;
  * slot 0 of the finest operator as stored (mgx_get_stencil / mgx_get_stencil9) and the term (mgx_get_reaction, or its
    refusal when the model holds none) after every call of the stage, bit for bit;
  * graphs_cached() unchanged over every call the model says moves nothing (set_reaction(None) with no term, the timing
    calls, the zero-iteration exits);
  * histories: those of mgx_solve inside mgx_theta_steps, the Newton histories and the norms of mgx_residual_norm to HIST_TOL /
    HIST_FLOOR (double) and NORM32 (float); with a Krylov solver inside to RTOL64 (+ PCG_FLOOR) / RTOL32;
  * with mgx_solve_gcr or mgx_solve_refine_gcr inside: the arrays the call writes, and the term a Newton call leaves, to RTOL64 /
    PCG32_STATE, after which the model takes over the device's arrays and term (and rebuilds its hierarchy from it).
    mgx_theta_steps with MGX_STEP_REFINE_GCR hands the device's per-step histories to the model for the scales; mgx_newton and
    mgx_newton_steps report no inner history, so a refining solver inside runs on the model's own scales.

The conditions these bounds rest on are asserted on the CPU from the model alone, on the committed lists
(tests/test_handle_model_newton.py::test_the_model_walks_the_reaction_sequences_and_meets_the_conditions): every Armijo, Newton
stop, step stop and inner mgx_solve stop decision has a relative margin of 100 x the norm tolerance of its precision at
least; every call with a Krylov solver inside, run a second time with every scalar of its dots moved by up to one ulp of the
working type, moves the arrays it writes by at most 1/16 of its bound; no inner history entry of a Newton call with a refining
solver inside lies, divided by n, within 1e-6 relative of a power of two.  Float Newton calls are capped at max_newton = 3
(from the fourth step on the iterate sits at the float rounding floor and the Armijo margins shrink to 1e-3).

On the CPU, the model alone, in the order of REACTION_CASES: lowest decision margin 2.3e-2, 4.4e-2, 4.7e-2 (need 1e-8) and 1.3e-2
(float, need 1e-3), each a stop decision of an mgx_solve inside theta_steps - the Armijo and Newton stop margins are above 0.9;
one-ulp scalars move a written array or the term by 1.1e-2, 1.3e-3, 6.4e-4 and (float) 3.3e-2 of its bound (cap 1/16 = 6.3e-2:
the float case keeps its Krylov solvers inside, with the GCR Newton call at two iterations - three moved B of level 5 by 0.11
of the bound); lowest last / first entry of a double Krylov call 1.6e-5, 1.1e-4, 1.4e-5 (the deep solve_gcr, cut to 5, 5 and 4
iterations for this); nearest power of two of an inner history entry / n under a refining Newton call 3.6e-2, 7.6e-3, 9.6e-2
(need 1e-6: the refining solver stays in the Newton calls); float32(c0 + d) != float32(c0) + float32(d) at 0.49 of the points.

Measured on an MI355X, one run, largest deviation as a fraction of its bound, in the order of REACTION_CASES (187, 199, 211 and
158 calls; device and model together 1.08 s - 0.67 s with MGX_GRAPH=0, 0.72 s with MGX_SMALL_VISIT=0, the same final state and
histories - 1.77 s, 0.64 s, 0.28 s; 6, 2, 6 and 5 graphs at the most):
  histories  theta_steps solve / gcr / refine_gcr   2.2e-6 / 2.1e-7 / 1.2e-7;  2.0e-6 / 2.6e-5 / 1.4e-7;  2.1e-6 / 1.1e-6 / 1.5e-7;  2.0e-11 / 1.1e-13 / -
             newton solve / gcr                      2.0e-6 / 8.3e-5;  1.3e-6 / 2.9e-5;  2.0e-6 / 2.1e-5;  2.1e-11 / 0
             newton_steps solve / refine_gcr         1.8e-6 / 4.8e-10;  1.5e-6 / 8.7e-8;  3.0e-10 / 4.6e-9;  1.3e-11 / -
             residual_norm                           0;  0;  1.7e-6;  1.5e-11
  state      theta_steps gcr, newton gcr (the term included)   6.5e-5, 1.8e-3;  9.0e-5, 7.4e-5;  3.2e-5, 5.2e-5;  0, 0 (float: bit for bit)
             theta_steps and newton_steps with refine_gcr inside: 0 in every case - with the device's order of summation the model's
             own scales are the device's and the iterate is the model's bit for bit.
Everything else - every setter, every timing call, every call under MGX_STEP_SOLVE, the stored centre and the term - bit for bit.
The drawn calls there: history of solve / solve_pcg / solve_gcr / solve_refine / solve_refine_gcr at most 2.1e-6 / 7.6e-6 / 2.3e-5 /
2.2e-6 / 2.0e-7, written state after solve_pcg / solve_gcr at most 1.7e-4 / 2.1e-4 of RTOL64.  The failed line search (o): bit
for bit, Newton history 1.6e-6 of its bound.  No defect of the library showed.

Mistakes planted in scratch builds of csrc/ (never committed), the tests that fail with each: reaction_base copying c0 while a term
is set - all four sequences at the second set_reaction (slot 0) and (o) at its second newton; newton_pass taking its centre from
slot 0 - all four at their first newton that iterates (from its second pass on slot 0 carries d), and (o); theta_rhs given the
kept source when the caller passed none - all four at a theta_steps without g; galerkin_invalidate leaving the term's flag
raised - all four and (o) at the first set_reaction(None) with a term set (mgx_get_reaction does not refuse); the float copy
not rebuilt while a term is set - the three double sequences at a refine after a set_reaction, whose float cycle then
diverges.  None goes uncaught."""
import time

import numpy as np
import pytest

import handle_model as hm
import test_gpu_handle_state as gs
from test_gpu_handle_state import (EAGER, GCR_USERS, K_MAX_GRAPHS, NO_VISIT, OPERATOR_CHANGES, REFINE_USERS, STEP_CALLS, STEP_TIMING, all_levels,
                                   apply_device, apply_model, draw_sequence, inner_solver, kinds_at, point_counts, run_sequence, set_knobs,
                                   step)

pytestmark = pytest.mark.gpu

SOLVE, GCR, REFINE_GCR = hm.STEP_SOLVE, hm.STEP_GCR, hm.STEP_REFINE_GCR
PLAIN = ("smooth", "set_u", "set_b", "zero_u", "residual", "restrict_rhs", "prolong", "bottom_solve", "fmg")   # calls no promise ties to a neighbour
USERS = GCR_USERS + REFINE_USERS
TERM_DROPPERS = tuple(k for k in OPERATOR_CHANGES if k != "build_galerkin")


def transfers_at(calls):
    """the transfer of the last build before every call of a list (set_operator rebuilds with the one in use)"""
    out, t = [], hm.BILINEAR
    for c in calls:
        out.append(t)
        if c[0] == "build_galerkin":
            t = c[1]
    return out


def safe_positions(calls):
    """where a block may stand, after the first graph user: so that the nearest graph user, operator change or set_cycle before
    it is a graph user (no earlier stage's 'the next graph user after ...' is taken), and directly after a PLAIN call (no
    stage promises anything about the call after one) or, in a list without refining calls, whose stages promise no
    neighbours, after a graph user"""
    out, first = [], next(i for i, c in enumerate(calls) if c[0] in USERS)
    strict = any(c[0] in REFINE_USERS for c in calls)
    for i in range(first + 1, len(calls)):
        if calls[i - 1][0] in PLAIN or (not strict and calls[i - 1][0] in GCR_USERS):
            back = next(c[0] for c in reversed(calls[:i]) if c[0] in USERS or c[0] in OPERATOR_CHANGES or c[0] == "set_cycle")
            if back in USERS:
                out.append(i)
    return out


def reaction_stage(seed, cfg, out, tol_n, krylov32=True, flips=False):
    """blocks of ("set_reaction", seed | None), ("get_reaction",), ("theta_steps", theta, nsteps, seed of g | None, solver, tol,
    max_iters, restart), ("newton", problem, solver, lin_max_iters, restart, tol, max_newton, max_backtracks), ("newton_steps",
    theta, nsteps, seed of g | None, solver, lin_max_iters, restart, tol, max_newton, max_backtracks), the three timing calls
    and ("residual_norm",) placed INTO a drawn list at safe_positions, in this order, with a generator of its own.  Every
    block rebuilds with the transfer in force where it stands, leaves the hierarchy built and ends with a fresh guess and
    right-hand side.  Held by construction (assert_reaction_calls):
    (a) set_reaction, build, a graph user;  (b) a second set_reaction that replaces the first;  (c) set_reaction(None) with a
    term set;  (d) set_reaction(None) with none set directly between two graph users, the fourth and fifth of five equal ones
    (both pointer assignments of the finest level are cached by then: the fifth replays, or the cache is full);
    (e) an operator change that drops a term, set_reaction(None) - a no-op - a build and later a newton with no set_reaction
    between: the base centre is the new operator's;  (f) newton entered with the caller's term set;  (g) newton directly
    followed by theta_steps, whose mass is then d_k;  (h) theta_steps with g, theta_steps without, newton_steps with g,
    newton_steps without, in a row;  (i, double) solve_refine or solve_refine_gcr directly after set_reaction + build,
    set_reaction(None) + build, newton and newton_steps;  (j) solve_gcr before and directly after a newton;  (k) set_cycle
    between two newton calls, the kind in force put back after;  (l) each timing call directly followed by residual_norm and a
    graph user;  (m) newton with max_newton = 0 and with tol = 2, newton_steps and theta_steps with nsteps = 0, newton_steps
    with max_newton = 0;  (n) a theta_steps of two steps with max_iters = 1 and tol_n: the first step converges in its one
    cycle (a random time level: the cycle smooths it), the second does not.
    Krylov solvers inside: theta_steps with GCR and, double, REFINE_GCR; newton with GCR; double: newton_steps with REFINE_GCR.
    krylov32 = False: a float case whose Krylov calls miss condition 2 runs MGX_STEP_SOLVE only.  flips: the operator change
    of (e) is set_tensor on a five-point finest level (the nine-point case); the double cases run both refining solvers after
    each call of (i) and after (g), five of each in all"""
    rng = np.random.RandomState(seed + 99999)
    L = cfg["finest_level"]
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    count = [0]

    def fresh():
        count[0] += 1
        return [("set_guess", 5000 + count[0]), ("set_rhs", 6000 + count[0])]

    def term():
        count[0] += 1
        return ("set_reaction", 7000 + count[0])

    def source():
        count[0] += 1
        return 8000 + count[0]

    def newton(solver=SOLVE, tol=None, max_newton=None, problem="cubic"):
        k = (3 if not f64 else int(rng.choice([3, 4]))) if max_newton is None else max_newton
        tol = (0.0 if not f64 else float(rng.choice([0.0, 1e-6]))) if tol is None else tol
        lin = (4, 0) if solver == SOLVE else (3, 2)
        return ("newton", problem, solver) + lin + (tol, k, 4)

    def newton_steps(theta, nsteps, g, solver=SOLVE, max_newton=None):
        k = (3 if not f64 else 4) if max_newton is None else max_newton
        lin = (4, 0) if solver == SOLVE else (3, 2)
        return ("newton_steps", theta, nsteps, g, solver) + lin + (1e-3 if not f64 else 1e-6, k, 4)

    def theta_steps(theta, nsteps, g, solver=SOLVE):
        return ("theta_steps", theta, nsteps, g, solver, 1e-3, 40, 0 if solver == SOLVE else 3)

    def refines(first):
        pair = [("solve_refine", 0.0, 2), ("solve_refine_gcr", 0.0, 2, 2)]
        return pair[first:] + pair[:first] if f64 else []

    def b1(T, kind, nine):                                                                                     # (a) (b) (c) (d)
        build, x = ("build_galerkin", T), ("vcycle_zero",)
        return [term(), build, ("solve", 0.0, 2), term(), build, ("get_reaction",), x, ("set_reaction", None), build, x, x, x, x,
                ("set_reaction", None), x] + fresh()

    def b2(T, kind, nine):                                                                                     # (e) (f) (g)
        build = ("build_galerkin", T)
        flip = ("set_tensor", "smooth9") if flips and not nine else ("set_coefficient", 10.0, 21)
        return [term(), build, flip, ("set_reaction", None), build, ("solve", 0.0, 1)] + fresh() + [newton()] + [term(), build] + fresh() + \
            [newton(), theta_steps(0.5, 2, source())] + refines(0) + fresh()

    def b3(T, kind, nine):                                                                                     # (h)
        return [term(), ("build_galerkin", T), theta_steps(1.0, 2, source()), theta_steps(0.5, 2, None), newton_steps(0.5, 2, source()),
                newton_steps(1.0, 1, None)] + fresh()

    def b4(T, kind, nine):                                                                                     # (i): double only
        build = ("build_galerkin", T)
        return [term(), build] + refines(0) + [("set_reaction", None), build] + refines(1) + fresh() + [newton()] + refines(0) + fresh() + \
            [newton_steps(0.5, 1, source())] + refines(1) + fresh()

    def b5(T, kind, nine):                                                                                     # (j) (k)
        other = hm.CYCLE_W if kind != hm.CYCLE_W else hm.CYCLE_F
        return [("solve_gcr", 0.0, 2, 2)] + fresh() + [newton(), ("solve_gcr", 0.0, 3, 3), ("set_cycle", other)] + fresh() + \
            [newton(), ("set_cycle", kind)] + fresh()

    def b6(T, kind, nine):                                                                                     # (l)
        x = ("vcycle_zero",)
        return [term(), ("build_galerkin", T), ("time_theta_rhs", 0.5), ("residual_norm",), ("solve", 0.0, 1), ("time_newton_pass", 1),
                ("residual_norm",), x, ("time_newton_step_pass", 2, 0.5), ("residual_norm",), ("solve", 0.0, 1), ("time_newton_step_pass", 0, 1.0),
                ("residual_norm",), x] + fresh() + [newton()] + fresh()

    def b7(T, kind, nine):                                                                                     # (m) (n)
        return [term(), ("build_galerkin", T)] + fresh() + [newton(max_newton=0), newton(tol=2.0), newton_steps(0.5, 0, None),
                                                             theta_steps(0.5, 0, None), newton_steps(0.5, 2, None, max_newton=0),
                                                             ("solve", 0.0, 1)] + fresh() + [("theta_steps", 1.0, 2, None, SOLVE, tol_n, 1, 0)] + fresh()

    def b8(T, kind, nine):                                                                                     # Krylov solvers inside
        out = [term(), ("build_galerkin", T)] + fresh() + [theta_steps(0.5, 2, source(), GCR)]
        if f64:
            out += [theta_steps(1.0, 2, None, REFINE_GCR)]
        out += fresh() + [newton(GCR, tol=0.0, max_newton=3 if f64 else 2)]
        if f64:
            out += fresh() + [newton_steps(0.5, 1, source(), REFINE_GCR, max_newton=3)]
        return out + fresh()

    makers = [b1, b2, b3] + ([b4] if f64 else []) + [b5, b6, b7] + ([b8] if f64 or krylov32 else [])
    safe = safe_positions(out)
    assert len(safe) >= len(makers), (seed, len(safe))
    at = sorted(int(i) for i in rng.choice(safe, len(makers), replace=False))
    transfers, kinds, counts = transfers_at(out), kinds_at(out), point_counts(out)
    flat, last = [], 0
    for make, i in zip(makers, at):
        flat += out[last:i]
        flat += make(transfers[i], kinds[i - 1], counts[i - 1] == 9)
        last = i
    return flat + out[last:]


def iterates(c):
    """a newton / newton_steps call of a list runs a Newton iteration (the CPU walk asserts that the model agrees)"""
    if c[0] == "newton":
        return c[6] > 0 and c[5] < 1.0
    return c[0] == "newton_steps" and c[2] > 0 and c[8] > 0


def assert_reaction_calls(calls, cfg):
    """what reaction_stage promises, on the final list"""
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    name = lambda i: calls[i][0] if 0 <= i < len(calls) else None
    term, by = [], None                                     # who set the term in force BEFORE every call: None, "caller", "newton"
    for c in calls:
        term.append(by)
        if c[0] == "set_reaction":
            by = None if c[1] is None else "caller"
        elif c[0] in TERM_DROPPERS:
            by = None
        elif iterates(c):
            by = "newton"
    idx = lambda pred: [i for i, c in enumerate(calls) if pred(i, c)]
    sets = idx(lambda i, c: c[0] == "set_reaction" and c[1] is not None)
    nones = idx(lambda i, c: c == ("set_reaction", None))
    newtons = idx(lambda i, c: c[0] == "newton")
    assert any(name(i + 1) == "build_galerkin" and name(i + 2) in USERS for i in sets), "(a)"
    assert any(term[i] == "caller" for i in sets), "(b)"
    assert any(term[i] is not None for i in nones), "(c)"
    assert any(term[i] is None and name(i - 1) in USERS and name(i + 1) in USERS and calls[i - 1] == calls[i + 1] and
               calls[i - 4:i] == [calls[i - 1]] * 4 for i in nones), "(d)"
    ok = False
    for i in idx(lambda i, c: c[0] in TERM_DROPPERS and term[i] is not None):                                  # (e)
        j = next((j for j in range(i + 1, len(calls)) if calls[j][0] == "set_reaction"), None)
        if j is None or calls[j][1] is not None or term[j] is not None:
            continue
        k = next((k for k in newtons if k > j), None)
        between = calls[i + 1:k] if k is not None else []
        ok = ok or (k is not None and iterates(calls[k]) and not any(c[0] in TERM_DROPPERS or (c[0] == "set_reaction" and c[1] is not None) or
                                                                      c[0] == "newton_steps" for c in between))
    assert ok, "(e)"
    assert any(term[i] == "caller" and iterates(calls[i]) for i in newtons), "(f)"
    assert any(iterates(calls[i]) and name(i + 1) == "theta_steps" and calls[i + 1][2] > 0 for i in newtons), "(g)"
    assert any(name(i) == name(i + 1) == "theta_steps" and name(i + 2) == name(i + 3) == "newton_steps" and
               [calls[i + k][3] is None for k in range(4)] == [False, True, False, True] and all(calls[i + k][2] > 0 for k in range(4))
               for i in range(len(calls))), "(h)"
    if f64:                                                                                                    # (i)
        assert any(name(i + 1) == "build_galerkin" and name(i + 2) in REFINE_USERS for i in sets), "(i) set_reaction"
        assert any(term[i] is not None and name(i + 1) == "build_galerkin" and name(i + 2) in REFINE_USERS for i in nones), "(i) set_reaction(None)"
        for kind in ("newton", "newton_steps"):
            assert any(c[0] == kind and iterates(c) and name(i + 1) in REFINE_USERS for i, c in enumerate(calls)), f"(i) {kind}"
    assert any(iterates(calls[i]) and name(i + 1) == "solve_gcr" and any(c[0] == "solve_gcr" for c in calls[:i]) for i in newtons), "(j)"
    ok = False
    for a, b in zip(newtons, newtons[1:]):                                                                     # (k)
        between = [c[0] for c in calls[a + 1:b] if c[0] not in ("set_guess", "set_rhs", "solve_gcr")]
        ok = ok or (between == ["set_cycle"] and iterates(calls[a]) and iterates(calls[b]))
    assert ok, "(k)"
    for kind in STEP_TIMING:                                                                                   # (l)
        assert any(c[0] == kind and name(i + 1) == "residual_norm" and name(i + 2) in USERS for i, c in enumerate(calls)), f"(l) {kind}"
    assert any(calls[i][6] == 0 for i in newtons) and any(calls[i][5] >= 1.0 and calls[i][6] > 0 for i in newtons), "(m) newton"
    assert any(c[0] == "newton_steps" and c[2] == 0 for c in calls) and any(c[0] == "theta_steps" and c[2] == 0 for c in calls), "(m) nsteps = 0"
    assert any(c[0] == "newton_steps" and c[2] > 0 and c[8] == 0 for c in calls), "(m) max_newton = 0"
    assert any(c[0] == "theta_steps" and c[2] >= 2 and c[6] == 1 and c[5] > 0.0 for c in calls), "(n)"


G73 = dict(finest_level=7, coarsest_level=3, mu0=0, mu1=2, mu2=1, schedule=hm.V, op=hm.GALERKIN)
REACTION_CASES = {
    # name: (configuration, seed, environments, options of draw_sequence, tol of (n), Krylov solvers inside).  Level 7 in
    # double is 127 columns: the passes' strip of 124 is crossed once.  Coarsest 3 or 4: Newton rebuilds the dense inverse
    # every iteration
    # V(2,1); the drawn operator changes alternate OPERATOR and BILINEAR builds, set_coefficient 100 at the end; the dense
    # bottom.  Again without graphs and without the visit kernel: the same final state and histories
    "galerkin_f64_jacobi_7_3_operator": (dict(G73), 8611, [{}, EAGER, NO_VISIT], dict(gcr=True, n_steps=50, deep_iters=5), 6e-2, True),
    # nine-point finest level through set_tensor, five-point through set_coefficient and back (the drawn changes and block
    # (e)); W / F cycles
    "galerkin_f64_sgs_7_3_nine_cycles": (
        dict(G73, mu1=1, mu2=1, smoother=hm.COLOR_SGS), 8612, [{}],
        dict(gcr=True, cycles=True, n_steps=50, deep_iters=5,
             operators=("rot45", [[("set_coefficient", 100.0, 11), ("build_galerkin", hm.BILINEAR)], [("set_operator", "smooth9")]])), 0.11, True),
    # bottom = SMOOTH; the refines of refine_stage between the blocks
    "galerkin_f64_chebyshev_7_4_smooth_bottom_refine": (dict(G73, coarsest_level=4, smoother=hm.CHEBYSHEV, bottom=hm.SMOOTH), 8613, [{}],
                                                        dict(gcr=True, refine=True, n_steps=50, deep_iters=4), 3.2e-2, True),
    "galerkin_f32_jacobi_fw16_6_3": (dict(G73, finest_level=6, dtype=hm.F32, restrict_mode=hm.FW16), 8614, [{}], dict(gcr=True, n_steps=50), 6e-2, True),
}


def reaction_calls(name):
    """(the final list, the drawn list it was placed into) of a case"""
    cfg, seed, envs, options, tol_n, krylov32 = REACTION_CASES[name]
    base = draw_sequence(seed, cfg, **options)
    return reaction_stage(seed, cfg, base, tol_n, krylov32, "operators" in options), base


def assert_base_calls(name, base):
    """the promises of the earlier stages, on the list they drew"""
    cfg, seed, envs, options, _, _ = REACTION_CASES[name]
    gs.assert_gcr_calls(base, cfg, False, options.get("deep_iters", gs.DEEP_GCR[2]))
    if options.get("cycles"):
        gs.assert_cycle_calls(base, cfg)
    if options.get("refine"):
        gs.assert_refine_calls(base, cfg, True)


@pytest.mark.parametrize("name", list(REACTION_CASES))
def test_reaction_theta_and_newton_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name):
    """the zero-order term, the theta steps and Newton between the other entry points of ONE handle: U and B of every
    level, the stored centre, the term, the histories, every count and graphs_cached() after every call (module docstring);
    every environment of a case leaves the final state and the histories of the first, bit for bit"""
    cfg, seed, envs, options, _, _ = REACTION_CASES[name]
    calls, base = reaction_calls(name)
    assert_base_calls(name, base)
    assert_reaction_calls(calls, cfg)
    runs = []
    for env in envs:
        set_knobs(monkeypatch, env)
        t0 = time.perf_counter()
        tally = run_sequence(pkg, po, cfg, calls, seed, env)
        print(f"[handle-newton] {name} env={env}: {len(calls)} calls in {time.perf_counter() - t0:.2f} s (device and model)")
        assert tally.graphs == -1 if env == EAGER else 1 <= tally.graphs <= K_MAX_GRAPHS, tally.graphs
        runs.append(tally)
        # (d): the no-op between two equal graph users adds no graph, and neither does the user after it
        for i, c in enumerate(calls):
            if c == ("set_reaction", None) and calls[i - 1] == calls[i + 1] and calls[i - 4:i] == [calls[i - 1]] * 4:
                assert tally.graph_counts[i - 1] == tally.graph_counts[i] == tally.graph_counts[i + 1], (i, tally.graph_counts[i - 1:i + 2])
    for b, env in zip(runs[1:], envs[1:]):
        for x, y in zip(runs[0].final, b.final):
            assert np.array_equal(x, y), env
        assert len(runs[0].histories) == len(b.histories) and all(np.array_equal(x, y) for x, y in zip(runs[0].histories, b.histories)), env


# (o): the failed line search.  Poisson (set_coefficient of a == 1), newton_ref.backtracking_input: the first full Newton step
# overshoots, and with max_backtracks = 0 the call gives up at once - U the guess, B the caller's f, the operator A0 + diag(d_0)
# with its hierarchy built, the coarse levels what the one linear solve left.  Then the same input with the halvings allowed
BACKTRACKING_CFG = dict(finest_level=6, coarsest_level=3, mu0=0, mu1=2, mu2=1, schedule=hm.V, op=hm.GALERKIN)
BACKTRACKING_CALLS = (
    [("set_coefficient", 1.0, 1), ("build_galerkin", hm.BILINEAR)] + [c for lv in range(3, 7) for c in (("set_u", lv, 1000 + lv), ("set_b", lv, 2000 + lv))]
    + [("set_newton_data", "backtracking"), ("newton", "backtracking", SOLVE, 6, 0, 1e-10, 5, 0), ("get_reaction",), ("residual_norm",), ("solve", 0.0, 1),
       ("set_reaction", None), ("build_galerkin", hm.BILINEAR), ("set_newton_data", "backtracking"), ("newton", "backtracking", SOLVE, 6, 0, 1e-10, 8, 8),
       ("get_reaction",), ("vcycle_zero",)])


def test_a_failed_line_search_leaves_what_the_model_holds(pkg, po, monkeypatch):
    """(o) of the module docstring, on a handle of its own: step() after every call"""
    set_knobs(monkeypatch, {})
    cfg, calls = BACKTRACKING_CFG, list(BACKTRACKING_CALLS)
    tally, done = gs.Tally(), []
    where = lambda: f"step {len(done) - 1} of {len(calls)}, calls so far {done}"
    m = hm.HandleModel(po, **cfg)
    with pkg.Multigrid(**cfg) as mg:
        for call in calls:
            done.append(call)
            got = step(pkg, mg, m, cfg, call, tally, where)
            if call[0] == "newton" and call[7] == 0:       # max_backtracks = 0: one rejected trial, no accepted step
                ns = got[0]
                assert (ns.iterations, ns.converged, ns.backtracks) == (0, 0, 1) and len(got[2]) == 1 and b"line search failed" in pkg.lib().mgx_last_error(mg._h)
            elif call[0] == "newton":
                ns = got[0]
                assert ns.converged == 1 and ns.backtracks >= 1 and got[3][0] < 1.0, (ns.iterations, ns.backtracks, got[3])
    print(f"\n[handle-newton] failed line search: histories / bound {tally.steps_hist}")
