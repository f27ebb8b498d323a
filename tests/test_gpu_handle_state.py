"""One long-lived handle driven through interleaved entry points, against the CPU model of a handle
(tests/handle_model.py) after EVERY call: the graph cache of csrc/mgx.hip (cached_graph) is keyed on the u / tmp
pointers of every level, the eager entry points swap those pointers, and a replay repeats the captured body's
bookkeeping from a record - a replay one swap off, a graph that outlives the operator it captured, a fine_updates that
drifts between replay and eager runs or a broken cache-full fallback all return plausible numbers.

What is compared, and how:
  * U and B of every level, after every call.  Bit for bit wherever the per-operator tests hold the operators bit for
    bit (tests/test_gpu_operators.py, test_gpu_var.py, test_gpu_galerkin.py, test_gpu_opdep.py, test_gpu_cheby.py,
    test_gpu_fma.py): every grid operator of the three hierarchies in both precisions and arithmetics, the dense bottom
    solve of the general operators, and so every schedule and solve composed of them.
  * Two operators are held to a tolerance by the existing suite, and calls that run through them here too (relative to
    the largest entry of the model's array): the sine-transform bottom solve of an fp64 POISSON hierarchy with
    bottom = EXACT - 1e-11 (test_gpu_operators.py::test_exact_bottom_solve), a V-cycle / FMG pass through it 1e-12
    (test_gpu_solve.py::test_single_vcycle_and_fmg_entry_points), a solve 1e-11 (test_f64_history_matches_oracle); the
    fp32 POISSON configurations use bottom = SMOOTH and stay bit for bit.  mgx_solve_pcg (dots in another summation
    order): in fp64 the iterate to 1e-9 (test_gpu_pcg.py).  The coarse levels then hold linear images of the last
    residual under the cycle's operators, so they carry that residual's relative deviation, which RTOL64 bounds (it is
    what the history entries are held to): same 1e-9.  In fp32 test_gpu_pcg.py bounds no iterate; the bound here is
    this file's own, PCG32_STATE = 1e-3, from that file's documented sensitivity: a scalar that rounds to the
    neighbouring float (1e-7) moves the fp32 residual, and so its images on the coarse levels, by about 2e-4 of itself;
    the iterate moves far less and is held to the same figure.  The deviations measured are printed.
    Only the arrays such a call writes are compared that way (touched()); every other level stays bit for bit.  After
    such a call the model takes over the device's arrays it compared to a tolerance, so that every later call is again
    compared bit for bit from the state the device really is in (a pointer swap off would still show: it changes the
    arrays read back).
  * histories: mgx_solve to HIST_TOL / HIST_FLOOR of test_gpu_solve.py in fp64 and to the 1e-5 of
    test_gpu_operators.py's fp32 norm; mgx_solve_pcg to RTOL64 (+ 1e-14 ||r0||) / RTOL32 of test_gpu_pcg.py.
  * stats.cycles, stats.converged, stats.fine_updates: equal to the model's.

CYCLE_CASES add the cycle index (mgx_set_cycle, csrc/mgx_small.hpp) to the sequences: the graph key carries no cycle
kind (the setter drops the graphs), k_small_visit updates U in place where the per-level launches swap u / tmp, and a
cycle may start from a small level with a non-zero U.  The model composes W and F from its single operators, so the
state is still held bit for bit, on the coarse levels too; the Jacobi GALERKIN cases run with and without the visit
kernel against the same model.

LINE_CASES add the zebra line smoothers (csrc/mgx_line.hpp: in place, no parity flip; two factor arrays per level and
direction, rebuilt with the operator).  The device joins a line's carries in another order than tests/line_ref.py, so a
call that smooths (SMOOTHING) is held, on every array it writes, to THE TOLERANCE RULE of tests/test_line_cpu.py: 4 x
the difference between the model in the working type and the model in np.longdouble, both run for this one call from
the same state, relative to max |x|, floor 16 eps - against both models, never from device output.  Both models then
take over the device's arrays.  No such bound may exceed RTOL64 / PCG32_STATE ("bound too loose" otherwise;
tests/test_handle_model.py checks the committed seeds on the CPU).  A twin handle created with MGX_GRAPH=0 is held to
the replaying one bit for bit after every call.  Measured on an MI355X, largest bound used / largest deviation of the
device as a fraction of its bound: GALERKIN double LINE_ALT 1.29e-10 / 0.79; GALERKIN float LINE_X 2.69e-4 / 0.44;
GALERKIN double LINE_Y with MGX_LINE_CHUNK=16 6.79e-11 / 0.68; STENCIL5 double LINE_ALT 1.95e-10 / 0.68 (histories: at
most 4e-4 of their bound in double, 0.04 in float).  The dense coarsest solve of the CYCLE_CASES is bit for bit at
levels 3 and 4 as it is at level 5.

GCR_CASES add mgx_solve_gcr (csrc/mgx_krylov_host.hpp) as a fourth graph user: it runs cycle_body through the same graph
cache with lv[L].b repointed at r, on the workspace mgx_solve_pcg shares (one scalar block, one partial-sum buffer, a basis
that grows with the restart asked for), so what it leaves on the coarse levels, a stale graph after mgx_set_cycle or a
rebuild under it, and either method on the buffers the other allocated are held here.  It is compared as mgx_solve_pcg is,
for the same reason (the device differs from the model only in the summation order of the dots): the history through
the solve_pcg branch of history_check, the arrays it writes to RTOL64 / PCG32_STATE, everything else bit for bit.  In
double one call per sequence is DEEP_GCR (nine iterations of GCR(8) after shorter bases: every slot, then a wrap); float
sequences stop at four iterations (after nine the coarse levels hold images of a residual near the float rounding floor
of the first one; deep float bases are held in tests/test_gpu_gcr.py on the history and the iterate).
What these bounds rest on is measured on the CPU, the model against itself, never from device output
(tests/test_handle_model.py::test_the_gcr_sequences_meet_the_conditions_their_bounds_rest_on, which asserts it):
  * PCG32_STATE for solve_gcr: every float solve_gcr call run a second time from the same state with every scalar moved
    independently by up to one float ulp (a factor 1 + 1.2e-7 u, u uniform in (-1, 1)) moves an array the call writes by
    at most 4.6e-6 of its largest entry (POISSON float RB-GS 8..5: B of level 7 after four iterations of GCR(2)) and
    1.6e-5 (GALERKIN float FW16 7..3 with W / F cycles: U of level 6 after four iterations of GCR(2)), a history entry by
    at most 5.0e-7 relative.  The cap there is PCG32_STATE / 4 = 2.5e-4: 16 times the larger figure.
  * no double Krylov call ends below 1e-6 of its first history entry (the iterate stays out of the cancellation regime of
    b - A u): the lowest are 6.0e-5 (POISSON V(1,0) 8..5, the deep call), 1.1e-4 (STENCIL5 Chebyshev, a solve_pcg of three
    iterations), 1.2e-4 (GALERKIN 7..3, the deep call), 5.3e-6 (the line case, whose deep call is shortened to four
    iterations for this: GCR_CASES).  The cases smooth weakly, V(1,0), to get there.
  * the line case: the largest rule bound used is 1.3e-11 (cap 1e-9).
Measured on an MI355X, largest deviation as a fraction of its bound, history of solve_gcr / written state after it:
POISSON double 2.9e-6 / 1.6e-3 (STREAMING: 4.0e-6 / 1.7e-3); STENCIL5 double Chebyshev 7.5e-6 / 3.2e-4; GALERKIN double 7..3
6.7e-6 / 5.3e-5, the same bits with MGX_SMALL_VISIT=0; both float cases: histories 4e-13, state bit for bit (the float
products are exact in the double accumulators, and their sums round to the same floats); the line case 1.7e-4 of the
history bound, 0.55 of the rule bound.

COLOUR_CASES add the multicolour Gauss-Seidel smoothers (csrc/mgx_colour.hpp), the first smoother that mixes both buffer
regimes on one handle - a five-point level with a chunk's worth of rows runs k_gs_rb out of place and swaps u / tmp once per
sweep, a nine-point or smaller level runs k_gs_colour in place - and the first whose blocks depend on their position:
COLOR_SGS reverses the colour order after a correction, in the last mu2 sweeps of a bottom = SMOOTH visit and so in every
second visit of a W / F cycle, a flag that travels through capture, cycle_body under PCG / GCR, mgx_fmg and mgx_vcycle from
any level.  The model hands `post` to tests/colour_ref.py, so everything stays bit for bit, on the coarse levels too.
stencil5_f64_gs_8_5: V(3,2), every level swaps, an odd and an even block; stencil5_f32_sgs_7_3_smooth_bottom_cycles: levels
7..4 swap, level 3 is in place, the bottom visit runs forward then in reverse, W / F second visits, cycles from levels 6, 5,
4; galerkin_f64_sgs_7_3_cycles: only the finest level swaps, the dense solve at level 3, the same bits with
MGX_SMALL_VISIT=0 (the visit kernel is Jacobi's); galerkin_f32_gs_fw16_8_5_smooth_bottom.  The first and the third a second
time with MGX_GS_FUSED=0 (no level swaps): the same final state and histories.
NINE_CASES flip lv[finest].nine between graph users (mgx_set_tensor / mgx_set_stencil9 against mgx_set_coefficient /
mgx_set_stencil): every kernel of that level changes, the Krylov direction kernel on a workspace that survives, and under a
colour smoother whether the level swaps.  galerkin_f64_jacobi_7_3_nine_cycles (rot45 -> OPERATOR -> set_coefficient ->
smooth9 -> jump9, with and without the visit kernel), galerkin_f32_chebyshev_fw16_7_4_nine_smooth_bottom (smooth9 ->
contrast -> rot45), galerkin_f64_sgs_7_3_nine_gcr (V(1,1); solve_pcg and solve_gcr before the first and after the last
flip, each of them once the first Krylov call after a flip), galerkin_f64_gs_8_5_nine_gcr (V(1,0), bottom = SMOOTH).  The
unsymmetric random9 runs through one list written by hand, without solve_pcg, on a COLOR_GS and a Jacobi handle: 9 -> 5
(the unsymmetric five-point operator of tests/test_gpu_colour.py) -> 9 with other ring-pointing values than the model's.
The Krylov calls are held as above; the condition, measured on the CPU from the model alone (tests/test_handle_model.py::
test_the_model_walks_the_colour_and_nine_sequences and the GCR conditions test, which the two new GCR cases join): lowest
last / first history entry of a double Krylov call 8.7e-3 (stencil5 gs), 3.4e-4 (galerkin sgs), 8.3e-4 (jacobi nine), 4.0e-6
(sgs nine gcr: its deep call is five iterations of GCR(8) for this - six end at 3.5e-7), 1.4e-3 (gs nine gcr, the deep call of
nine iterations), 8.1e-5 / 1.5e-3 (random9 gs / jacobi); float: 2.3e-2 at the lowest.  Measured on an MI355X, largest
deviation as a fraction of its bound, history of solve_pcg / of solve_gcr / written state after either: stencil5 gs 1.0e-6 /
- / 4.7e-5; galerkin sgs 1.8e-4 / - / 1.7e-4; jacobi nine 2.4e-5 / - / 1.4e-4; sgs nine gcr 3.9e-6 / 4.8e-6 / 8.5e-5; gs nine
gcr 2.4e-6 / 2.7e-6 / 5.6e-5; random9 - / 6.3e-7 / 2.3e-4 (gs), - / 2.5e-7 / 3.0e-5 (jacobi); the three float cases: histories
4e-13, state bit for bit.  The runs under MGX_SMALL_VISIT=0 and MGX_GS_FUSED=0 give the same figures to the digit.  The
dense coarsest solve stays bit for bit under these operators at levels 3 and 4.

REFINE_CASES add mgx_solve_refine (csrc/mgx.hip, csrc/mgx_refine.hpp) as one more graph user, drawn with refine=True
(refine_stage; what it promises: draw_sequence).  The call hides more state in a handle than any before it: a second solver
(the float copy of the hierarchy, on the parent's stream, with a graph cache of its own) that is rebuilt lazily when the
parent's operator generation has moved and is told the cycle kind by hand; one u <-> tmp swap of the finest level per cycle
under the parent's graph key; and the pass's sums in the partial-sum buffer and the scalar that mgx_solve, mgx_solve_pcg and
mgx_solve_gcr use.  The model (handle_model.HandleModel.solve_refine) keeps a private F32 model beside itself and takes the
scales s_k from the history the device returned; U and B of EVERY level are compared bit for bit after the call - so the
parent's coarse levels are held untouched, which include/mgx.h states - the history through the solve branch of
history_check (the same residual bits, another order of the sum), the statistics for equality.
stencil5_f64_jacobi_8_5_refine and stencil5_f64_chebyshev_8_5_refine (V(3,2); set_coefficient 100 and 1000 rewrite every level of
the float copy; the Chebyshev bounds of the float cycle are arguments of its captured kernels; the float dense solve at level 5
is held by GENERAL_CASES' stencil5_f32_chebyshev); galerkin_f64_jacobi_7_3_refine_cycles (set_cycle through CYCLE_ORDER, two
transfer-only rebuilds between refines; a second and third time with MGX_SMALL_VISIT=0 and with MGX_GRAPH=0: the same final
state and histories, the float copy takes the parent's knobs); galerkin_f64_sgs_7_3_nine_refine (rot45 -> set_coefficient ->
smooth9; again with MGX_GS_FUSED=0); galerkin_f64_gs_8_5_smooth_bottom_refine_gcr (V(1,0), refine between Krylov calls on the
shared workspace).  The three GALERKIN cases use bottom = SMOOTH: no F32 sequence holds the float dense solve of a GALERKIN
hierarchy against the model.  The sequences are 60, 60, 83, 61 and 67 calls long with 9, 9, 13, 9 and 12 refines (n_steps = 30:
the mandatory calls alone, data, graph users, operator changes, set_cycle and the refine stage, come to more than fifty).
Both STENCIL5 cases fill the graph cache (8 graphs; the odd swaps add buffer assignments) and run their last calls through the
eager fallback; the GALERKIN cases reach 4.  On the CPU, the model alone (tests/test_handle_model.py::
test_the_model_walks_the_refine_sequences): every refine history decreases over its call - from the set_coefficient 1000 of
the STENCIL5 cases on, whose re-discretised hierarchy DIVERGES under V(3,2) after a first cycle, by construction of the
sequence (refine_stage) - and the lowest last / first entry of a Krylov call is 1.0e-3, 2.6e-2, 5.5e-4, 1.2e-3, 1.3e-4.
Measured on an MI355X, largest deviation as a fraction of its bound, history of solve_refine / of solve_pcg / written state
after solve_pcg, in the order above: 2.1e-6 / 3.7e-6 / 2.1e-5; 1.3e-6 / 8.3e-6 / 1.7e-5; 1.9e-6 / 1.0e-5 / 1.5e-4; 1.5e-6 / 4.5e-6 /
5.2e-6; 2.0e-6 / 2.2e-6 / 8.3e-7 (solve_gcr there: 2.8e-6 / 1.3e-4); mgx_solve's histories at most 2.2e-6.  The runs under
MGX_SMALL_VISIT=0, MGX_GRAPH=0 and MGX_GS_FUSED=0 give the same figures to the digit.

REFINE_GCR_CASES add mgx_solve_refine_gcr (csrc/mgx_refine_host.hpp: RefineGcrMethod, csrc/mgx_refine_gcr.hpp) and mgx_time_refine_gcr_pass,
drawn with refine_gcr=True on top of refine and gcr (refine_gcr_stage; what it promises: draw_sequence).  The call shares the float
copy of the hierarchy - r32, z32, the cached cycle graphs - with mgx_solve_refine, the Krylov workspace, the scalar block and the
partial sums with mgx_solve_gcr and mgx_solve_pcg, and keeps its residual in B of the finest level for the whole solve.  The model
(handle_model.HandleModel.solve_refine_gcr: tests/refine_gcr_ref.py around the model's fp64 operator and the float model that
solve_refine uses) is given the device's history for the scales and refine_gcr_ref.device_dot for the dots, as
tests/test_gpu_refine_gcr.py's composition is.  touched() is U of the finest level alone, held to RTOL64; B and EVERY other level
stay bit for bit, which is where the call differs from mgx_solve_gcr; the history is held as mgx_solve_gcr's (RTOL64 h + PCG_FLOOR
h0), the statistics for equality; mgx_time_refine_gcr_pass moves nothing.
stencil5_f64_jacobi_8_5_refine_gcr (V(3,2); the first graph user after set_coefficient 100 is a solve_refine, after 1000 a
solve_refine_gcr of one iteration - the calls stay short where the float cycle diverges); galerkin_f64_jacobi_7_3_smooth_bottom_
refine_gcr_cycles (V(1,0); set_cycle through CYCLE_ORDER with a call directly after one of them, the transfer-only rebuilds in
turn through either entry; again with MGX_SMALL_VISIT=0 and with MGX_GRAPH=0: the same final state and histories);
galerkin_f64_sgs_7_3_nine_refine_gcr (V(1,1), bottom = SMOOTH; set_tensor rot45 -> set_coefficient -> set_stencil9 smooth9:
k_refine_direction<9>, <5>, <9> on one workspace).  The sequences are 80, 108 and 83 calls long with 9, 12 and 10 calls of
mgx_solve_refine_gcr and 11, 15 and 11 of mgx_solve_refine.  On the CPU, the model alone with numpy's dots
(tests/test_handle_model.py::test_the_model_walks_the_refine_gcr_sequences): no history of a solve_refine_gcr increases, every one
ends below its first entry (0.81 at the slowest: two iterations of GCR(1) under the diverging STENCIL5 cycle), and the lowest
last / first entry of a Krylov call is 7.6e-4, 1.2e-4, 1.2e-4 (the deep solve_gcr each time).
Measured on an MI355X, in the order above: 2.8 s, 0.7 s (its three environments together), 0.3 s; 8, 4 and 4 graphs (the STENCIL5 case
fills the cache and ends in the eager fallback).  Largest deviation as a fraction of its bound, history of solve_refine_gcr / U of
the finest level after it: 1.3e-7 / 0; 0 / 0; 2.2e-7 / 0 - with the device's order of summation the iterate is the model's bit
for bit, and only the first history entry, which the device takes from its residual-norm kernel, is summed in another order.
The other calls there: history of solve / solve_pcg / solve_gcr / solve_refine at most 2.2e-6 / 1.7e-5 / 3.8e-6 / 2.0e-6, written
state after solve_pcg / solve_gcr at most 3.3e-5 / 3.6e-4 of RTOL64.  The runs under MGX_SMALL_VISIT=0 and MGX_GRAPH=0 give the same
figures to the digit.

The zero-order term, the theta steps and Newton (mgx_set_reaction, mgx_theta_steps, mgx_newton, mgx_newton_steps and their timing
entry points) are drawn, run and described in tests/test_gpu_handle_newton.py; apply_device, apply_model and step know their
calls (apply_model_steps, step_checks), and the committed seeds of this file draw none of them.

A failing sequence is reproduced from the seed, the step index and the calls so far, which the message carries."""
import numpy as np
import pytest

import handle_model as hm
import newton_ref as nf
import nine_ref as nr
from refine_gcr_ref import device_dot
from test_gpu_colour import random5
from test_gpu_line import history_bound
from test_line_cpu import rule_bound

pytestmark = pytest.mark.gpu

HIST_TOL, HIST_FLOOR = 1e-10, 1e-13        # tests/test_gpu_solve.py (fp64 histories)
NORM32 = 1e-5                              # tests/test_gpu_operators.py::test_residual_matches_oracle (fp32 norms)
RTOL64, RTOL32, PCG_FLOOR = 1e-9, 1e-3, 1e-14      # tests/test_gpu_pcg.py (assert_hist)
PCG32_STATE = 1e-3                         # this file's: U and the coarse levels after an fp32 mgx_solve_pcg / mgx_solve_gcr (module docstring)
BOTTOM64, CYCLE64, SOLVE64 = 1e-11, 1e-12, 1e-11   # the POISSON sine-transform bottom solve and what runs through it (see above)
K_MAX_GRAPHS = 8                           # kMaxGraphs of csrc/mgx.hip: the capacity of a handle's graph cache

MUS = (0, 1, 2, 3, 5)
GRAPH_USERS = ("solve", "solve_pcg", "vcycle_zero")
GCR_USERS = GRAPH_USERS + ("solve_gcr",)     # the sequences drawn with gcr=True
SOLVES = ("solve", "solve_pcg", "solve_gcr", "solve_refine", "solve_refine_gcr")  # the calls that return (stats, history)
KRYLOV = ("solve_pcg", "solve_gcr")
REFINE_USERS = ("solve_refine", "solve_refine_gcr")          # the graph users that cycle in the float copy of the hierarchy
OPERATOR_CHANGES = ("set_coefficient", "build_galerkin", "set_stencil", "set_stencil9", "set_tensor", "set_operator")
GCR_RESTARTS = (1, 2, 3)
DEEP_GCR = ("solve_gcr", 0.0, 9, 8)          # nine iterations of GCR(8): every slot of the full basis, then slot 0 again
KNOBS = ("MGX_TILE_MAX_N", "MGX_FUSE_MIN_N", "MGX_PLAN_MIN_N", "MGX_PLAN_PRE", "MGX_PLAN_POST", "MGX_GRAPH", "MGX_FOLD", "MGX_FUSE",
         "MGX_ZERO_IN", "MGX_TILE_K", "MGX_FOLD_KMAX", "MGX_FOLD_KMAX_NOPOST", "MGX_FUSE_ROWS", "MGX_ROWS", "MGX_SMALL_VISIT", "MGX_LINE_CHUNK",
         "MGX_GS_FUSED")
SMOOTHING = ("smooth", "vcycle", "vcycle_zero", "fmg", "solve", "solve_pcg", "solve_gcr")      # the calls that run a smoother
CYCLE_ORDER = (hm.CYCLE_W, hm.CYCLE_F, hm.CYCLE_V, hm.CYCLE_W, hm.CYCLE_F, hm.CYCLE_W, hm.CYCLE_V)
SMALL_MAX_LEVEL = 6                        # kSmallMaxN = 64 of csrc/mgx_small.hpp
# the marching kernels on every level (no register tiles); fused / folded passes from 128^2 up (MGX_FUSE_MIN_N=128, as
# in test_gpu_solve.py::test_tuning_knobs_never_change_a_bit) with explicit pass plans for the folded blocks, V(3,2) as
# [2,1] down and [1,1] up: levels 8 and 7 stream their blocks through folded passes, 6 and 5 take single sweeps
STREAMING = {"MGX_TILE_MAX_N": "0", "MGX_FUSE_MIN_N": "128", "MGX_PLAN_MIN_N": "128", "MGX_PLAN_PRE": "2,1", "MGX_PLAN_POST": "1,1"}


def field(n, seed):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, (n, n))


def coefficient(L, contrast, seed):
    """nodal coefficient of -div(a grad u): 1 or `contrast` in 16 x 16 blocks"""
    N = 1 << L
    blk = np.where(np.random.RandomState(seed).rand(N // 16 + 1, N // 16 + 1) < 0.5, 1.0, contrast)
    return np.kron(blk, np.ones((16, 16)))[: N + 1, : N + 1].copy()


# ---- the generator -------------------------------------------------------------------------------------------------
def small_levels(cfg):
    """the levels above the coarsest with N <= 64: where a W- or F-cycle may run k_small_visit, and from which a cycle
    may start as its top"""
    return list(range(cfg["coarsest_level"] + 1, min(cfg["finest_level"], SMALL_MAX_LEVEL) + 1))


def kinds_at(calls):
    """the cycle kind in force at every call of a drawn list"""
    out, kind = [], hm.CYCLE_V
    for c in calls:
        if c[0] == "set_cycle":
            kind = c[1]
        out.append(kind)
    return out


def graph_users(calls):
    """the kinds of graph user a drawn list holds each five times at least"""
    users = GCR_USERS if any(c[0] == "solve_gcr" for c in calls) else GRAPH_USERS
    return users + tuple(k for k in REFINE_USERS if any(c[0] == k for c in calls))


def refine_stage(seed, cfg, out, gcr):
    """draw_sequence(refine=True): ("solve_refine", tol, max_cycles) and one ("time_refine_pass", 2) placed INTO a drawn list,
    with a generator of its own (the draws of the list itself are untouched).  The list is cut into spans that stay
    together, and whole spans are put between spans, so every promise of draw_sequence's docstring holds by
    construction.  A ("set_guess", seed) stands before a refine wherever the promise does not forbid it: the iterate
    then never sits at the rounding floor of b - A u, where a history cannot decrease"""
    rng = np.random.RandomState(seed + 55555)
    L, Lc = cfg["finest_level"], cfg["coarsest_level"]
    fresh = [0]

    def refine(k=None, tol=None, guess=True):
        k = int(rng.randint(1, 5)) if k is None else k
        tol = float(rng.choice([0.0, 1e-3])) if tol is None else tol
        fresh[0] += 1
        return ([("set_guess", 4000 + fresh[0])] if guess else []) + [("solve_refine", tol, k)]

    spans = []
    for c in out:                                          # (a group of operator changes is one span: set_coefficient + build_galerkin)
        if spans and c[0] in OPERATOR_CHANGES and spans[-1][-1][0] in OPERATOR_CHANGES:
            spans[-1].append(c)
        else:
            spans.append([c])
    at = lambda name: [i for i, s in enumerate(spans) if s[0][0] == name]
    # (c), (d): three of the drawn solves, each with a refine directly before it - tol 0, so that the count is the cycles run
    odd, even, timed = (int(i) for i in rng.choice(at("solve"), 3, replace=False))
    spans[odd] = refine(int(rng.choice([1, 3])), 0.0) + spans[odd]
    spans[even] = refine(int(rng.choice([2, 4])), 0.0) + spans[even]
    spans[timed] = refine() + [("time_refine_pass", 2)] + spans[timed]
    # (e): a drawn solve_pcg and a drawn solve_gcr (not the deep one: a fresh guess stands before that) directly after a refine
    for name in KRYLOV if gcr else KRYLOV[:1]:
        i = int(rng.choice([i for i in at(name) if len(spans[i][0]) < 4 or spans[i][0][3] != DEEP_GCR[3]]))
        spans[i] = refine(int(rng.choice([1, 2])), 0.0) + spans[i]
    # (a): after every group of operator changes, and after a set_cycle that directly follows it; (b): after two more set_cycle
    ends = [i for i, s in enumerate(spans) if s[0][0] in OPERATOR_CHANGES]
    ends =[i + 1 if i + 1 < len(spans) and spans[i + 1][0][0] == "set_cycle" else i for i in ends]
    others = [i for i in at("set_cycle") if i not in ends]
    if others:
        ends += [int(i) for i in rng.choice(others, 2, replace=False)]
    for i in ends:
        spans[i] = spans[i] + refine()
    # (f): a cycle from a coarse level, a restriction of the finest residual and a correction of the finest U between two
    # refines, the second one from what they left; and a call that runs no cycle
    users = [i for i, s in enumerate(spans) if any(c[0] in GCR_USERS for c in s)]
    coarse = int(rng.randint(Lc + 1, L)) if L - 1 > Lc else Lc
    between = refine() + [("vcycle", coarse), ("restrict", L), ("prolong_add", L)] + refine(guess=False)
    for extra in (between, refine(0, 1e-3, guess=False)):
        spans.insert(int(rng.randint(users[0] + 1, users[-1] + 1)), extra)
    # STENCIL5 with the contrast 1000: the cycle of the re-discretised hierarchy DIVERGES (the model alone, V(3,2), Jacobi and
    # Chebyshev: the first cycle from a random guess reduces the residual to 2e-2 .. 4e-2, every later one multiplies it by 5
    # to 20).  From that change on every refine that cycles starts from a fresh guess and runs one cycle for an odd, two for
    # an even count, tol 0 - the histories then still decrease over the call
    flat, diverging = [], False
    for c in (c for s in spans for c in s):
        diverging = diverging or (cfg.get("op") == hm.STENCIL5 and c[0] == "set_coefficient" and c[1] >= 1000.0)
        if diverging and c[0] == "solve_refine" and c[2]:
            flat += refine(2 - c[2] % 2, 0.0, guess=flat[-1][0] != "set_guess")
        else:
            flat.append(c)
    return flat


def assert_refine_calls(calls, cfg, gcr=False):
    """what draw_sequence(refine=True) promises, on the drawn list.  (With refine_gcr=True, which places its calls later and
    keeps out of the pairs promised here, a solve_refine_gcr is not counted as a graph user: assert_refine_gcr_calls says
    which of the two refining calls comes first after an operator change)"""
    L = cfg["finest_level"]
    users = [i for i, c in enumerate(calls) if c[0] in graph_users(calls) and c[0] != "solve_refine_gcr"]
    refines = [i for i, c in enumerate(calls) if c[0] == "solve_refine"]
    assert "solve_refine" in graph_users(calls) and len(refines) >= 5
    counts = [calls[i][2] for i in refines]
    assert all(calls[i][1] in (0.0, 1e-3) and 0 <= calls[i][2] <= 4 for i in refines)
    assert 0 in counts and any(k % 2 for k in counts) and any(k and k % 2 == 0 for k in counts), counts
    timed = [i for i, c in enumerate(calls) if c[0] == "time_refine_pass"]
    assert len(timed) == 1 and calls[timed[0]] == ("time_refine_pass", 2) and timed[0] > refines[0]
    next_user = lambda i: next(calls[u][0] for u in users if u > i)
    changes = [i for i in range(users[0], len(calls)) if calls[i][0] in OPERATOR_CHANGES]
    assert changes and all(next_user(i) == "solve_refine" for i in changes)                                   # (a)
    sets = [i for i, c in enumerate(calls) if c[0] == "set_cycle"]
    assert not sets or sum(1 for i in sets if next_user(i) == "solve_refine") >= 2                             # (b)
    follower = lambda i: calls[i + 1][0] if i + 1 < len(calls) else None
    after = [calls[i][2] for i in refines if calls[i][1] == 0.0 and follower(i) == "solve"]
    assert any(k % 2 for k in after) and any(k and k % 2 == 0 for k in after), after                          # (c)
    assert follower(timed[0]) == "solve"                                                                       # (d)
    for name in KRYLOV if gcr else KRYLOV[:1]:                                                                 # (e)
        assert any(follower(i) == name for i in refines), name
    assert any(len(calls) > i + 4 and calls[i + 1][0] == "vcycle" and calls[i + 1][1] < L and calls[i + 2] == ("restrict", L)
               and calls[i + 3] == ("prolong_add", L) and [c[0] for c in calls[i + 4:i + 6] if c[0] != "set_guess"][:1] == ["solve_refine"]
               for i in refines)                                                                               # (f)


REFINE_GCR_RESTARTS = GCR_RESTARTS + (8,)


def refine_gcr_stage(seed, cfg, out, cycles):
    """draw_sequence(refine_gcr=True): ("solve_refine_gcr", 0.0, max_iters, restart) and the two ("time_refine_gcr_pass", which, 2)
    placed INTO a list that refine_stage has been through (drawn with gcr=True), with a generator of its own.  Calls are put
    between two calls of the list, never between two that a promise of refine_stage keeps together (glued), so those
    promises still hold, and every promise of draw_sequence's docstring for this option holds by construction.
    A ("set_guess", seed) stands before a call wherever the promise does not say "directly after"."""
    rng = np.random.RandomState(seed + 66666)
    L = cfg["finest_level"]
    fresh = [0]

    def call(k=None, restart=None, guess=True):
        k = int(rng.randint(1, 6)) if k is None else k
        restart = int(rng.choice(GCR_RESTARTS)) if restart is None else restart
        fresh[0] += 1
        return ([("set_guess", 5000 + fresh[0])] if guess else []) + [("solve_refine_gcr", 0.0, k, restart)]

    def glued(i):
        """nothing may be put between out[i - 1] and out[i]"""
        a, b = out[i - 1], out[i] if i < len(out) else (None,)
        return (a[0] in ("solve_refine", "time_refine_pass", "set_guess") or (a[0] in OPERATOR_CHANGES and b[0] in OPERATOR_CHANGES)
                or (a[0] == "vcycle" and b == ("restrict", L)) or (a == ("restrict", L) and b == ("prolong_add", L))
                or (a == ("prolong_add", L) and b[0] in ("solve_refine", "set_guess")))

    # between an operator change and the graph user after it nothing is put but (a)'s own call: which call rebuilds the float
    # copy is what (a) decides
    waiting, pending = [], False
    for c in out + [(None,)]:
        waiting.append(pending)
        pending = c[0] in OPERATOR_CHANGES or (pending and c[0] not in GCR_USERS + ("solve_refine",))
    put = {}                                               # position in `out` -> the calls that go in front of it
    free = lambda i: 0 <= i <= len(out) and i not in put and (i == 0 or not glued(i)) and not waiting[i]

    def place(i, calls):
        assert free(i), (seed, i)
        put[i] = calls
        return i

    users = [i for i, c in enumerate(out) if c[0] in GCR_USERS + ("solve_refine",)]
    # STENCIL5: the cycle of the contrast-1000 hierarchy diverges (refine_stage).  GCR does not, but a solve_refine that
    # continues from what a call left would: the pair of (c) stands before that change, and the calls after it are short
    far = [i for i, c in enumerate(out) if cfg.get("op") == hm.STENCIL5 and c[0] == "set_coefficient" and c[1] >= 1000.0]
    limit = far[0] if far else len(out)
    gcrs = [i for i, c in enumerate(out) if c[0] == "solve_gcr"]
    shallow = [i for i in gcrs if out[i][3] != DEEP_GCR[3]]
    deep = [i for i in gcrs if out[i][3] == DEEP_GCR[3]]
    # (b): restart 1 directly before a solve_gcr; restart 8, five iterations, directly after a solve_gcr of a short basis (the
    # call grows the workspace itself; before the diverging change where one stands there); a restart from GCR_RESTARTS, four
    # iterations, directly after the deep solve_gcr (a short basis in the grown workspace, wrapped)
    place(deep[0] + 1, call(4, int(rng.choice(GCR_RESTARTS)), guess=False))
    first = place(next(i for i in shallow if free(i)), call(restart=1))
    grow = [i + 1 for i in shallow if i >= first and free(i + 1)]
    place(next((i for i in grow if i <= limit), grow[0]), call(5, 8, guess=False))
    # (e): both timing passes after the first call; DIRECTION directly before a solve_gcr, UPDATE directly before a call
    place(int(rng.choice([i for i in shallow if i > first and free(i)])), [("time_refine_gcr_pass", 1, 2)])
    later = [i for i in range(first + 1, len(out) + 1) if free(i)]
    place(int(rng.choice(later)), [("set_guess", 5900), ("time_refine_gcr_pass", 0, 2)] + call(guess=False))
    # (d): a drawn solve and a drawn solve_pcg directly after a call
    for name in ("solve", "solve_pcg"):
        if not any(i < len(out) and out[i][0] == name and put[i][-1][0] == "solve_refine_gcr" for i in put):    # (a call of (b), (e) may do)
            place(int(rng.choice([i for i, c in enumerate(out) if c[0] == name and free(i)])), call())
    # (c): a solve_refine between two calls, no set_guess between the three
    early = [i for i in range(users[0] + 1, limit) if free(i)]
    place(int(rng.choice(early)), call(int(rng.choice([2, 3]))) + [("solve_refine", 0.0, 2)] + call(int(rng.choice([2, 3])), guess=False))
    # (f): a call that runs no iteration
    place(int(rng.choice([i for i in range(users[0] + 1, len(out)) if free(i)])), [("solve_refine_gcr", 0.0, 0, 2)])
    # (g): directly after a set_cycle
    if cycles:
        place(int(rng.choice([i + 1 for i, c in enumerate(out) if c[0] == "set_cycle" and free(i + 1)])), call(guess=False))
    # (a): the first graph user after every second group of operator changes (the others: refine_stage's solve_refine)
    ends = [i for i, c in enumerate(out) if c[0] in OPERATOR_CHANGES and (i + 1 == len(out) or out[i + 1][0] not in OPERATOR_CHANGES)]
    for i in ends[1::2]:
        assert (i + 1) not in put and not glued(i + 1), (seed, i)
        put[i + 1] = call()
    for i in sorted(put, reverse=True):
        out = out[:i] + put[i] + out[i:]
    flat, diverging = [], False
    for c in out:
        diverging = diverging or (cfg.get("op") == hm.STENCIL5 and c[0] == "set_coefficient" and c[1] >= 1000.0)
        flat.append(c[:2] + (2 - c[2] % 2,) + c[3:] if diverging and c[0] == "solve_refine_gcr" and c[2] > 2 else c)
    return flat


def assert_refine_gcr_calls(calls, cfg, cycles=False):
    """what draw_sequence(refine_gcr=True) promises, on the drawn list"""
    at = [i for i, c in enumerate(calls) if c[0] == "solve_refine_gcr"]
    assert len(at) >= 5 and all(calls[i][1] == 0.0 and 0 <= calls[i][2] <= 5 and calls[i][3] in REFINE_GCR_RESTARTS for i in at)
    before = lambda i: calls[i - 1]
    after = lambda i: calls[i + 1] if i + 1 < len(calls) else (None,)
    users = [i for i, c in enumerate(calls) if c[0] in graph_users(calls)]
    ends = [i for i in range(users[0], len(calls)) if calls[i][0] in OPERATOR_CHANGES and after(i)[0] not in OPERATOR_CHANGES]
    firsts = [next(calls[u][0] for u in users if u > i) for i in ends]
    assert len(firsts) >= 2 and firsts == [REFINE_USERS[g % 2] for g in range(len(firsts))], firsts                            # (a)
    is_deep = lambda c: c[0] == "solve_gcr" and c[3] == DEEP_GCR[3]
    assert any(after(i)[0] == "solve_gcr" and calls[i][3] == 1 for i in at)                                                   # (b)
    assert any(before(i)[0] == "solve_gcr" and not is_deep(before(i)) and calls[i][3] == 8 for i in at)
    assert any(is_deep(before(i)) and calls[i][3] in GCR_RESTARTS for i in at)
    assert any(c[0] == "solve_refine" and c[2] >= 1 and before(i)[0] == after(i)[0] == "solve_refine_gcr" for i, c in enumerate(calls))   # (c)
    for name in ("solve", "solve_pcg"):                                                                                       # (d)
        assert any(after(i)[0] == name for i in at), name
    timed = [i for i, c in enumerate(calls) if c[0] == "time_refine_gcr_pass"]                                                # (e)
    assert sorted(calls[i][1:] for i in timed) == [(0, 2), (1, 2)] and min(timed) > at[0]
    assert {calls[i][1]: after(i)[0] for i in timed} == {1: "solve_gcr", 0: "solve_refine_gcr"}
    assert sum(1 for i in at if calls[i][2] == 0) == 1                                                                        # (f)
    if cycles:
        assert any(before(i)[0] == "set_cycle" for i in at)                                                                   # (g)
    # a fresh guess wherever no promise says "directly after"
    bare = [i for i in at if before(i)[0] != "set_guess"]
    assert all(before(i)[0] in ("solve_gcr", "solve_refine", "set_cycle", "time_refine_gcr_pass") or calls[i][2] == 0 for i in bare), bare


def draw_sequence(seed, cfg, n_steps=40, cycles=False, operators=None, fresh_guess=False, short_solves=False, without=(), tail=(), gcr=False, deep_iters=DEEP_GCR[2],
                  refine=False, refine_gcr=False):
    """~n_steps calls, every one valid for `cfg` by construction (nothing is filtered afterwards): the three graph
    users (four with gcr) five times each at least, an odd-launch smooth on every level at least once, the rest drawn with weights;
    mu from MUS.  Operator changes of the general hierarchies are placed after every third graph user.

    Off by default (the sequences of the cases that do not ask are call for call what they were):
    cycles       ("set_cycle", kind) after every second graph user, through CYCLE_ORDER, and for every small level a
                 ("vcycle", level) placed while the kind is W and one while it is F
    operators    (first, [change, ...]): ("set_operator", first) instead of set_coefficient (+ build_galerkin) at the
                 start, and the given lists of calls instead of the operator changes
    fresh_guess  a random U of the top level before every call that forms b - A u of what earlier cycles left there:
                 ("set_guess", seed) before solve / solve_pcg, ("set_u", level, seed) before ("vcycle", level).  The
                 iterate then never converges into the cancellation regime of b - A u, where a rounding bound relative
                 to max |x| means nothing
    short_solves one cycle per solve and one iteration per solve_pcg (the float line case: see LINE_CASES)
    without      call kinds left out of the weighted draw
    tail         calls appended after everything else
    gcr          ("solve_gcr", tol, max_iters, restart) as a fourth graph user: tol as for solve_pcg, max_iters 1..4, restart
                 from GCR_RESTARTS (a call with max_iters > restart wraps the basis); the first one of the sequence with
                 restart 2; double: the last one becomes DEEP_GCR after a fresh ("set_guess", 3500) - the basis grows from
                 2 to 8 pairs on a handle the other graph users have run on
    deep_iters   the iterations of that call, where nine take the iterate too far (the line case: see GCR_CASES)
    refine       ("solve_refine", tol, max_cycles) as one more graph user (refine_stage; dtype F64, general operators): five
                 calls at least, tol 0 or 1e-3, max_cycles 0 .. 4 with 0, an odd and an even count among them, and one
                 ("time_refine_pass", 2) after the first of them.  Held by construction (assert_refine_calls):
                 (a) the next graph user after every operator change is a solve_refine (the float copy has to follow);
                 (b) so it is after two set_cycle calls at least;
                 (c) a solve directly follows a solve_refine, once after an odd and once after an even number of cycles
                     (u <-> tmp swaps; sums in the shared partial-sum buffer that are not a smoothing block's);
                 (d) a solve directly follows time_refine_pass;
                 (e) solve_pcg, and with gcr solve_gcr, directly follows a solve_refine once;
                 (f) a ("vcycle", level) from a coarse level, ("restrict", finest) and ("prolong_add", finest) stand between
                     two refines
    refine_gcr   (with refine and gcr) ("solve_refine_gcr", 0.0, max_iters, restart) as one more graph user and
                 ("time_refine_gcr_pass", which, 2) for both passes (refine_gcr_stage): tol 0, so the count is the work done,
                 1 .. 5 iterations, restart from GCR_RESTARTS and 8; a fresh ("set_guess", seed) before a call wherever no
                 promise says "directly".  Held by construction (assert_refine_gcr_calls):
                 (a) the first graph user after the groups of operator changes is in turn a solve_refine and a
                     solve_refine_gcr: the float copy is rebuilt through either entry;
                 (b) a call with restart 1 directly before a solve_gcr; a call with restart 8 directly after a solve_gcr of
                     a short basis (the call grows the workspace); a call with a restart from GCR_RESTARTS directly after
                     the deep solve_gcr (a short basis, wrapped, in the grown workspace);
                 (c) a call directly before and a call directly after one solve_refine, no set_guess between the three
                     (the same r32 / z32 and cycle graphs; the second call starts from what the first two left);
                 (d) a solve and a solve_pcg each directly follow a call once (norm_blocks_ready, the partial sums, the
                     scalar block);
                 (e) both timing passes after the first call: DIRECTION (basis slot 0 rewritten) directly before a
                     solve_gcr, UPDATE (the float right-hand side rewritten, the scalars zeroed) directly before a call;
                 (f) one call with max_iters = 0;
                 (g) with cycles: a call directly after a set_cycle"""
    assert not (refine and fresh_guess) and (not refine_gcr or (refine and gcr))
    rng = np.random.RandomState(seed)
    L, Lc = cfg["finest_level"], cfg["coarsest_level"]
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    exact = cfg.get("bottom", hm.EXACT) == hm.EXACT
    op = cfg.get("op", hm.POISSON)
    user_kinds = GCR_USERS if gcr else GRAPH_USERS

    def one(name):
        lv = int(rng.randint(Lc, L + 1))
        up = int(rng.randint(Lc + 1, L + 1))
        if name == "solve":
            tol, k = float(rng.choice([0.0, 1e-2])), int(rng.randint(1, 4))
            return ("solve", tol, 1 if short_solves else k)
        if name == "solve_pcg":
            tol, k = float(rng.choice([0.0, 1e-3] if f64 else [0.0, 1e-2])), int(rng.randint(1, 4))
            return ("solve_pcg", tol, 1 if short_solves else k)
        if name == "solve_gcr":
            tol, k = float(rng.choice([0.0, 1e-3] if f64 else [0.0, 1e-2])), int(rng.randint(1, 5))
            return ("solve_gcr", tol, 1 if short_solves else k, int(rng.choice(GCR_RESTARTS)))
        if name == "smooth":
            return ("smooth", lv, int(rng.choice(MUS)))
        if name in ("vcycle", "residual", "zero_u"):
            return (name, lv)
        if name in ("restrict", "restrict_rhs", "prolong", "prolong_add"):
            return (name, up)
        if name in ("set_guess", "set_rhs"):
            return (name, int(rng.randint(1 << 30)))
        if name in ("set_u", "set_b"):
            return (name, lv, int(rng.randint(1 << 30)))
        return (name,)

    weights = {"smooth": 8, "vcycle": 3, "restrict": 2, "restrict_rhs": 1, "prolong": 1, "prolong_add": 2, "fmg": 1, "residual": 1,
               "set_guess": 2, "set_rhs": 1, "set_u": 2, "set_b": 1, "zero_u": 1, "solve": 1, "solve_pcg": 1, "vcycle_zero": 1}
    if exact:
        weights["bottom_solve"] = 2
    if gcr:
        weights["solve_gcr"] = 1
    for k in without:
        del weights[k]
    names = sorted(weights)
    p = np.array([weights[k] for k in names], dtype=float)
    calls = [one(k) for k in user_kinds for _ in range(5)]
    between = [("smooth", lv, int(rng.choice([1, 3, 5]))) for lv in range(Lc, L + 1)]
    changes = []
    if op == hm.STENCIL5:
        changes = [[("set_coefficient", 100.0, 11)], [("set_coefficient", 1000.0, 12)]]
    elif op == hm.GALERKIN:
        changes = [[("build_galerkin", hm.OPERATOR)], [("build_galerkin", hm.BILINEAR)], [("build_galerkin", hm.OPERATOR)],
                   [("set_coefficient", 100.0, 11), ("build_galerkin", hm.BILINEAR)]]
    if operators is not None:
        changes = [list(c) for c in operators[1]]
    while len(calls) + len(between) + sum(len(c) for c in changes) < n_steps:
        calls.append(one(names[int(rng.choice(len(names), p=p / p.sum()))]))
    calls = [calls[i] for i in rng.permutation(len(calls))]
    for c in between:                                      # an odd-launch smooth on every level, between two graph users
        users = [i for i, x in enumerate(calls) if x[0] in user_kinds]
        calls.insert(int(rng.randint(users[0] + 1, users[-1] + 1)), c)
    out, users = [], 0
    kinds = list(CYCLE_ORDER) if cycles else []
    for c in calls:
        out.append(c)
        if c[0] in user_kinds:
            users += 1
            if users % 3 == 0 and changes:
                out += changes.pop(0)
            if users % 2 == 0 and kinds:
                out.append(("set_cycle", kinds.pop(0)))
    assert not changes and not kinds
    if cycles:
        # a cycle from every small level as its top, under W and under F: placed inside a span of that kind
        rng2 = np.random.RandomState(seed + 77777)
        for lv in small_levels(cfg):
            for kind in (hm.CYCLE_W, hm.CYCLE_F):
                at = [i for i, k in enumerate(kinds_at(out)) if k == kind]
                out.insert(int(at[rng2.randint(len(at))]) + 1, ("vcycle", lv))
        for lv in small_levels(cfg):
            for kind in (hm.CYCLE_W, hm.CYCLE_F):
                assert any(c == ("vcycle", lv) and k == kind for c, k in zip(out, kinds_at(out))), (seed, lv, kind)
    if gcr:
        first = [i for i, c in enumerate(out) if c[0] == "solve_gcr"]
        out[first[0]] = out[first[0]][:3] + (2,)
        if f64:
            out[first[-1]] = DEEP_GCR[:2] + (deep_iters,) + DEEP_GCR[3:]
            if not fresh_guess:
                out.insert(first[-1], ("set_guess", 3500))
    if refine:
        out = refine_stage(seed, cfg, out, gcr)
    if refine_gcr:
        out = refine_gcr_stage(seed, cfg, out, cycles)
    if fresh_guess:
        fresh = []
        for c in out:
            if c[0] in SOLVES:
                fresh.append(("set_guess", 3000 + len(fresh)))
            elif c[0] == "vcycle":
                fresh.append(("set_u", c[1], 3000 + len(fresh)))
            fresh.append(c)
        out = fresh
    users = [i for i, x in enumerate(out) if x[0] in user_kinds]
    for lv in range(Lc, L + 1):
        assert any(c[0] == "smooth" and c[1] == lv and c[2] % 2 for c in out[users[0] + 1:users[-1]]), (seed, lv)
    # data on every level first, and the operators of the general hierarchies
    pre = []
    if operators is not None:
        pre.append(("set_operator", operators[0]))
    elif op != hm.POISSON:
        pre.append(("set_coefficient", 10.0, 10))
    if op == hm.GALERKIN and operators is None:
        pre.append(("build_galerkin", hm.BILINEAR))
    for lv in range(Lc, L + 1):
        pre += [("set_u", lv, 1000 + lv), ("set_b", lv, 2000 + lv)]
    return pre + out + list(tail)


# ---- one call on the device and on the model -------------------------------------------------------------------
RANDOM5_SEED, RING_SEED = 70, 17


def stencil5(L, kind, dt):
    """("set_stencil", kind): "random5", the unsymmetric five-point operator of tests/test_gpu_colour.py"""
    assert kind == "random5", kind
    return random5(L, RANDOM5_SEED + L, dt)


def stencil9(L, kind, dt, device):
    """("set_stencil9", kind): a nine-point operator of handle_model.operator9.  "random9_ring": the DEVICE is handed
    random9 with other values, up to 1e30, in the places that point at the Dirichlet ring (nine_ref.with_ring_values9),
    the model the plain random9 - those coefficients multiply the zero ring of the iterate and must change no bit"""
    if kind == "random9_ring":
        st9 = hm.operator9(L, "random9", dt)
        return [x.astype(dt) for x in nr.with_ring_values9(st9, RING_SEED)] if device else st9
    return hm.operator9(L, kind, dt)


# the zero-order term, the theta steps and Newton (tests/test_gpu_handle_newton.py draws them; reaction_stage there)
STEP_CALLS = ("theta_steps", "newton", "newton_steps")            # the calls that run a solver per step inside
STEP_TIMING = ("time_theta_rhs", "time_newton_pass", "time_newton_step_pass")
STEP_MASS = 0.5                                # mass = rho h^2 / (theta dt) of every ("newton_steps", ...), a constant grid


def reaction_term(c0, seed):
    """d of ("set_reaction", seed) for the base centre c0: between 0.05 and 0.25 of c0, moved so that c0 + d (one rounding in
    double: the centre as a double handle stores it) lies 2^-10 of a float32 spacing beside the middle of two neighbouring
    float32 values, on a random side.  float32 of the stored centre falls to that side; float32(c0) + float32(d), summed in
    float, falls where the float32 rounding of d - some 2^-4 of that spacing - puts it: a float copy of the hierarchy
    assembled from the parts instead of the stored centre differs at about half of the points"""
    rng = np.random.RandomState(seed)
    c0 = np.asarray(c0, dtype=np.float64)
    s = c0 * (1.05 + 0.2 * rng.uniform(0.0, 1.0, c0.shape))
    lo = s.astype(np.float32)
    hi = np.nextafter(lo, np.float32(np.inf))
    gap = hi.astype(np.float64) - lo.astype(np.float64)
    side = np.where(rng.uniform(0.0, 1.0, c0.shape) < 0.5, -1.0, 1.0)
    target = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64)) + side * gap * 2.0 ** -10
    return target - c0


def newton_problem(L, name, dt):
    """(kappa, p) of ("newton", name, ...): "cubic" kappa = 50 / N^2, phi = u + u^3 (every Newton step from a random
    guess passes the Armijo test with a margin above 0.9: tests/test_handle_model_newton.py asserts it on the committed
    lists); "backtracking" newton_ref.backtracking_input, whose first full step overshoots"""
    n, N = (1 << L) - 1, 1 << L
    if name == "backtracking":
        _, kap, _, p, _ = nf.backtracking_input(L, dt)
        return kap, p
    assert name == "cubic", name
    return np.full((n, n), 50.0 / N ** 2, dtype=dt), (1.0, 0.0, 1.0)


def apply_device(pkg, mg, call, L, transfer=hm.BILINEAR, model=None):
    """transfer: what a GALERKIN set_operator rebuilds with (the model's transfer in use).  model: the model BEFORE the call
    (("set_reaction", seed) places its term beside the base centre, which the model knows).
    The binding (multigrid_nikhil_c-_amd/binding.py) wraps the bare mgx_fmg, mgx_bottom_solve, mgx_residual,
    mgx_restrict*, mgx_prolong* only together with set_level calls, so those go to the C entry points through the
    wrapper's own handle and status check: Multigrid._h and Multigrid._chk - a rename there has to be followed here"""
    lib = pkg.lib()
    name, a = call[0], call[1:]

    def raw(fn, *args):
        mg._chk(getattr(lib, fn)(mg._h, *args), fn)

    if name == "solve":
        return mg.solve(tol=a[0], max_cycles=a[1])
    if name == "solve_pcg":
        return mg.solve_pcg(tol=a[0], max_iters=a[1])
    if name == "solve_gcr":
        return mg.solve_gcr(tol=a[0], max_iters=a[1], restart=a[2])
    if name == "solve_refine":
        return mg.solve_refine(tol=a[0], max_cycles=a[1])
    if name == "solve_refine_gcr":
        return mg.solve_refine_gcr(tol=a[0], max_iters=a[1], restart=a[2])
    dt = mg.level_dtype(L)
    if name == "get_reaction":
        return mg.reaction()
    if name == "residual_norm":
        return mg.residual_norm()
    if name == "theta_steps":                              # (theta, nsteps, seed of g or None, solver, tol, max_iters, restart)
        g = None if a[2] is None else field(mg.n(L), a[2])
        return mg.theta_steps(a[1], theta=a[0], g=g, solver=a[3], tol=a[4], max_iters=a[5], restart=a[6])
    if name == "newton":                                   # (problem, solver, lin_max_iters, restart, tol, max_newton, max_backtracks)
        kap, p = newton_problem(L, a[0], dt)
        return mg.newton(kap, p=p, solver=a[1], lin_tol=0.0, lin_max_iters=a[2], restart=a[3], tol=a[4], max_newton=a[5], max_backtracks=a[6])
    if name == "newton_steps":                             # (theta, nsteps, seed of g or None, solver, lin_max_iters, restart, tol, max_newton, max_backtracks)
        kap, p = newton_problem(L, "cubic", dt)
        g = None if a[2] is None else field(mg.n(L), a[2])
        return mg.newton_steps(a[1], np.full_like(kap, STEP_MASS), kap, p=p, theta=a[0], g=g, solver=a[3], lin_tol=0.0, lin_max_iters=a[4],
                               restart=a[5], tol=a[6], max_newton=a[7], max_backtracks=a[8])
    if name == "set_reaction":
        mg.set_reaction(None if a[0] is None else reaction_term(model.base_operator()[0], a[0]))
    elif name == "set_newton_data":                        # U and B of newton_ref.backtracking_input
        _, _, f, _, u0 = nf.backtracking_input(L, dt)
        mg.set_guess(u0)
        mg.set_rhs(f)
    elif name == "time_theta_rhs":
        assert mg.time_theta_rhs(a[0], 2) > 0.0
    elif name == "time_newton_pass":
        assert mg.time_newton_pass(a[0], 2) > 0.0
    elif name == "time_newton_step_pass":
        assert mg.time_newton_step_pass(a[0], a[1], 2) > 0.0
    elif name == "time_refine_pass":
        assert mg.time_refine_pass(a[0]) > 0.0
    elif name == "time_refine_gcr_pass":
        assert mg.time_refine_gcr_pass(a[0], a[1]) > 0.0
    elif name == "vcycle_zero":
        mg.vcycle_zero()
    elif name == "smooth":
        mg.smooth(a[0], a[1])
    elif name == "vcycle":
        mg.vcycle(a[0])
    elif name == "fmg":
        raw("mgx_fmg")
    elif name == "bottom_solve":
        raw("mgx_bottom_solve")
    elif name == "residual":
        raw("mgx_residual", a[0])
        return mg.get_level(a[0], pkg.VEC_R)
    elif name in ("restrict", "restrict_rhs", "prolong", "prolong_add"):
        raw("mgx_" + name, a[0])
    elif name == "set_guess":
        mg.set_guess(field(mg.n(L), a[0]))
    elif name == "set_rhs":
        mg.set_rhs(field(mg.n(L), a[0]))
    elif name in ("set_u", "set_b"):
        mg.set_level(a[0], pkg.VEC_U if name == "set_u" else pkg.VEC_B, field(mg.n(a[0]), a[1]))
    elif name == "zero_u":
        mg.zero_level(a[0], pkg.VEC_U)
    elif name == "set_coefficient":
        mg.set_coefficient(coefficient(L, a[0], a[1]))
    elif name == "build_galerkin":
        mg.build_galerkin(a[0])
    elif name == "set_cycle":
        mg.set_cycle(a[0])
    elif name == "set_stencil":                           # GALERKIN: the finest level becomes five-point
        mg.set_stencil(L, *stencil5(L, a[0], mg.level_dtype(L)))
    elif name == "set_stencil9":
        mg.set_stencil9(L, *stencil9(L, a[0], mg.level_dtype(L), device=True))
    elif name == "set_tensor":
        mg.set_tensor(*hm.tensor_nodes(L, a[0]))
    elif name == "set_operator" and a[0] in hm.OPERATORS9:
        if a[0] in hm.TENSORS:
            mg.set_tensor(*hm.tensor_nodes(L, a[0]))
        else:
            mg.set_stencil9(L, *hm.operator9(L, a[0], mg.level_dtype(L)))
        mg.build_galerkin(transfer)
    elif name == "set_operator":
        from oracle import pyoracle
        dt = mg.level_dtype(L)
        if mg.cfg.op == hm.STENCIL5:
            for lv in range(mg.cfg.coarsest_level, L + 1):
                mg.set_stencil(lv, *hm.operator5(pyoracle, lv, a[0], dt))
        else:
            mg.set_stencil(L, *hm.operator5(pyoracle, L, a[0], dt))
            mg.build_galerkin(transfer)
    else:
        raise AssertionError(name)
    return None


def inner_solver(call):
    """the solver (hm.STEP_*) a theta_steps / newton / newton_steps call runs inside; None for every other call"""
    return call[{"theta_steps": 4, "newton": 2, "newton_steps": 4}[call[0]]] if call[0] in STEP_CALLS else None


def apply_model_steps(m, call, L, device=None, rows=0):
    """mgx_set_reaction, mgx_theta_steps, mgx_newton, mgx_newton_steps and their timing entry points on the model.  Beside a
    device a refining inner solver sums its dots in the device's order (device_dot), and theta_steps, which reports its
    per-step histories, takes the scales from them, as apply_model does for solve_refine_gcr; mgx_newton and
    mgx_newton_steps report no inner history: the model's own scales"""
    name, a = call[0], call[1:]
    refining = device is not None and inner_solver(call) == hm.STEP_REFINE_GCR
    dot = (lambda p, q: device_dot(p, q, rows)) if refining else None
    n = m.n(L)
    if name == "set_reaction":
        m.set_reaction(None if a[0] is None else reaction_term(m.base_operator()[0], a[0]))
    elif name == "get_reaction":
        return m.get_reaction()
    elif name == "residual_norm":
        return m.residual_norm()
    elif name == "set_newton_data":
        _, _, f, _, u0 = nf.backtracking_input(L, m.wdt)
        m.set_guess(u0)
        m.set_rhs(f)
    elif name == "theta_steps":
        g = None if a[2] is None else field(n, a[2])
        return m.theta_steps(a[0], a[1], g, a[3], a[4], a[5], a[6], histories=device[2] if refining else None, dot=dot)
    elif name == "newton":
        kap, p = newton_problem(L, a[0], m.wdt)
        return m.newton(kap, p=p, solver=a[1], lin_tol=0.0, lin_max_iters=a[2], restart=a[3], tol=a[4], max_newton=a[5], max_backtracks=a[6], dot=dot)
    elif name == "newton_steps":
        kap, p = newton_problem(L, "cubic", m.wdt)
        g = None if a[2] is None else field(n, a[2])
        return m.newton_steps(a[0], a[1], np.full_like(kap, STEP_MASS), kap, g, p=p, solver=a[3], lin_tol=0.0, lin_max_iters=a[4], restart=a[5],
                              tol=a[6], max_newton=a[7], max_backtracks=a[8], dot=dot)
    elif name == "time_theta_rhs":
        m.time_theta_rhs(a[0], 2)
    elif name == "time_newton_pass":
        m.time_newton_pass(a[0], 2)
    elif name == "time_newton_step_pass":
        m.time_newton_step_pass(a[0], a[1], 2)
    else:
        raise AssertionError(name)
    return None


def step_checks(pkg, mg, m, cfg, call, got, want, tally, where, g_before, h_before):
    """what step() holds after a call of the zero-order term, the theta steps and Newton, beside U and B of every level:
    steps_done, every statistic, the step lengths and the backtracks equal; the histories as the solver inside is held
    (history_check: mgx_solve's bound for MGX_STEP_SOLVE and for the Newton norms around it, the Krylov bound otherwise); the
    operator as stored and the term bit for bit (mgx_get_stencil[9] slot 0, mgx_get_reaction) - after a Newton call with a
    Krylov solver inside to the state bound, after which the model takes the device's term over and rebuilds; a call that
    the model says moves nothing leaves graphs_cached() alone.  h_before: the model's hierarchy before the call"""
    name, a = call[0], call[1:]
    L = cfg["finest_level"]
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    inner = inner_solver(call)
    held_as = ("solve",) if inner in (None, hm.STEP_SOLVE) else ("solve_gcr",)
    label = name if inner is None else f"{name}/{('solve', 'gcr', 'refine_gcr')[inner]}"

    def hist(h, ref):
        tally.histories.append(np.array(h))
        ok, frac = history_check(cfg, held_as, h, ref)
        tally.steps_hist[label] = max(tally.steps_hist.get(label, 0.0), frac if np.isfinite(frac) else 0.0)
        assert ok, f"history {frac:.3g} x its bound: {h} vs {ref}; {where()}"

    def same(st, st_m, fields):
        have = tuple(getattr(st, k) for k in fields)
        assert have == tuple(st_m[k] for k in fields), f"stats {have} vs {st_m}; {where()}"

    if name == "get_reaction":
        assert np.array_equal(got, want), where()
    elif name == "residual_norm":
        frac = abs(got - want) / ((HIST_TOL if f64 else NORM32) * want)
        tally.steps_hist[name] = max(tally.steps_hist.get(name, 0.0), frac)
        assert frac <= 1.0, f"residual norm {got!r} vs {want!r}: {frac:.3g} x its bound; {where()}"
    elif name == "theta_steps":
        (done, sts, hs), (done_m, sts_m, hs_m) = got, want
        assert done == done_m, f"steps_done {done} vs {done_m}; {where()}"
        for k in range(done):
            hist(hs[k], hs_m[k])
            same(sts[k], sts_m[k], ("cycles", "converged", "fine_updates"))
    elif name == "newton":
        (ns, h, lin, lam), (st_m, h_m, lin_m, lam_m) = got, want
        same(ns, st_m, ("iterations", "converged", "backtracks", "linear_iterations"))
        assert np.array_equal(lam, lam_m), f"step lengths {lam} vs {lam_m}; {where()}"
        hist(h, h_m)
        assert len(lin) == len(lin_m), where()
        for st, (st_lin, _) in zip(lin, lin_m):
            same(st, st_lin, ("cycles", "converged", "fine_updates"))
    elif name == "newton_steps":
        (done, sts, hs), (done_m, sts_m, hs_m) = got, want
        assert done == done_m, f"steps_done {done} vs {done_m}; {where()}"
        for k in range(done):
            same(sts[k], sts_m[k], ("iterations", "converged", "backtracks", "linear_iterations"))
            hist(hs[k], hs_m[k])
    # the operator as stored (mgx_get_stencil9 waits for the build: a nine-point level is read after it), and the term
    slot0 = mg.get_stencil(L, 0) if m.st9 is None else (mg.get_stencil9(L, 0) if m.h is not None else m.st9[0])
    if m.d is None:
        with pytest.raises(pkg.MgxError, match="no zero-order term"):
            mg.reaction()
    else:
        d = mg.reaction()
        if name in ("newton", "newton_steps") and inner != hm.STEP_SOLVE and m.h is not h_before:
            rtol = state_tolerance(cfg, call)
            dev = float(np.max(np.abs(d.astype(np.float64) - m.d.astype(np.float64)))) / float(np.max(np.abs(m.d)))
            tally.steps_state[label] = max(tally.steps_state.get(label, 0.0), dev / rtol)
            assert dev <= rtol, f"the term off by {dev:.3g} (bound {rtol:g}); {where()}"
            transfer = m.transfer
            m.set_reaction(d)
            m.build_galerkin(transfer)
        assert np.array_equal(d, m.d), f"the term differs at {int(np.sum(d != m.d))} points; {where()}"
    assert np.array_equal(slot0, m._finest()[0]), f"slot 0 of the finest operator differs at {int(np.sum(slot0 != m._finest()[0]))} points; {where()}"
    if m.h is h_before and name != "build_galerkin" and (name in STEP_TIMING or name in ("set_reaction", "get_reaction", "residual_norm", "newton", "newton_steps")):
        assert mg.graphs_cached() == g_before, f"graphs {g_before} -> {mg.graphs_cached()} over a call that moves nothing; {where()}"


def apply_model(m, call, L, device=None, rows=0):
    """device: what apply_device returned for this call.  solve_refine takes its scales s_k from the history the device
    reported (a norm is the one place where the device's order of summation reaches the iterate), as
    tests/test_gpu_refine.py's composition does; everything else about the call is the model's own.  solve_refine_gcr takes
    the scales the same way and, beside a device, sums its dots in the device's order (refine_gcr_ref.device_dot with the
    rows per chunk of the handle, rows: MGX_ROWS when the handle was created, 0 for make_launch's own choice), as
    tests/test_gpu_refine_gcr.py's composition does; without a device numpy's order"""
    name, a = call[0], call[1:]
    if name == "solve_refine":
        return m.solve_refine(tol=a[0], max_cycles=a[1], history=None if device is None else device[1])
    if name == "solve_refine_gcr":
        if device is None:
            return m.solve_refine_gcr(tol=a[0], max_iters=a[1], restart=a[2])
        return m.solve_refine_gcr(tol=a[0], max_iters=a[1], restart=a[2], history=device[1], dot=lambda p, q: device_dot(p, q, rows))
    if name in STEP_CALLS or name in STEP_TIMING or name in ("set_reaction", "get_reaction", "set_newton_data", "residual_norm"):
        return apply_model_steps(m, call, L, device, rows)
    if name == "solve":
        return m.solve(tol=a[0], max_cycles=a[1])
    if name == "solve_pcg":
        return m.solve_pcg(tol=a[0], max_iters=a[1])
    if name == "solve_gcr":
        return m.solve_gcr(tol=a[0], max_iters=a[1], restart=a[2])
    if name == "residual":
        return m.residual(a[0])
    if name == "set_guess":
        m.set_guess(field(m.n(L), a[0]))
    elif name == "set_rhs":
        m.set_rhs(field(m.n(L), a[0]))
    elif name in ("set_u", "set_b"):
        m.set_level(a[0], 0 if name == "set_u" else 1, field(m.n(a[0]), a[1]))
    elif name == "zero_u":
        m.zero_level(a[0], 0)
    elif name == "set_coefficient":
        m.set_coefficient(coefficient(L, a[0], a[1]))
    elif name == "set_stencil":
        m.set_stencil(L, stencil5(L, a[0], m.wdt))
    elif name == "set_stencil9":
        m.set_stencil9(L, stencil9(L, a[0], m.wdt, device=False))
    elif name == "set_tensor":
        m.set_tensor(*hm.tensor_nodes(L, a[0]))
    else:
        getattr(m, name)(*a)
    return None


def state_tolerance(cfg, call):
    """0: bit for bit; else the relative bound of the module docstring for this call"""
    name = call[0]
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    if name in KRYLOV:
        return RTOL64 if f64 else PCG32_STATE
    if name == "solve_refine_gcr":                          # (F64 handles only; U of the finest level: touched)
        return RTOL64
    if name in STEP_CALLS:                                  # the solver inside: mgx_solve bit for bit, the Krylov solvers as themselves
        return 0.0 if inner_solver(call) == hm.STEP_SOLVE else (RTOL64 if f64 else PCG32_STATE)
    sine_bottom = cfg.get("op", hm.POISSON) == hm.POISSON and cfg.get("bottom", hm.EXACT) == hm.EXACT
    if not sine_bottom:
        return 0.0
    assert f64, "fp32 POISSON configurations use bottom = SMOOTH"
    return {"bottom_solve": BOTTOM64, "vcycle": CYCLE64, "vcycle_zero": CYCLE64, "fmg": CYCLE64, "solve": SOLVE64}.get(name, 0.0)


def touched(cfg, call):
    """the (level, 'U' / 'B') arrays a tolerance-held call writes; everything else must not move at all"""
    L, Lc = cfg["finest_level"], cfg["coarsest_level"]
    name = call[0]
    if name == "bottom_solve":
        return {(Lc, "U")}
    if name == "smooth":
        return {(call[1], "U")} if call[2] else set()
    if name == "solve_refine_gcr":                          # the iterate alone: B holds the residual during the solve and the caller's
        return {(L, "U")}                                   # b again after it, the cycle runs in the float copy - bit for bit
    if name in STEP_CALLS:
        # a Krylov solver inside: what it writes, and B of the finest level where a later step forms it from an iterate
        # held to the bound (mgx_newton puts the caller's f back: bit for bit)
        out = {(L, "U")} | (set() if name == "newton" else {(L, "B")})
        if inner_solver(call) == hm.STEP_REFINE_GCR:
            return out
        return out | {(lv, x) for lv in range(Lc, L) for x in ("U", "B")}
    top =call[1] if name == "vcycle" else L                # vcycle_zero, fmg, solve, solve_pcg, solve_gcr: from the finest level
    return {(top, "U")} | {(lv, x) for lv in range(Lc, top) for x in ("U", "B")}


def history_check(cfg, call, h, ref):
    """(ok, largest deviation as a fraction of its bound)"""
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    h, ref = np.asarray(h), np.asarray(ref)
    if len(h) != len(ref):
        return False, np.inf
    if call[0] in ("solve", "solve_refine"):               # (solve_refine: norms of the same residual bits in another order, as solve's)
        bound = HIST_TOL * ref + HIST_FLOOR * ref[0] if f64 else NORM32 * ref
    else:
        bound = RTOL64 * ref + PCG_FLOOR * ref[0] if f64 else RTOL32 * ref
    bound = np.maximum(bound, np.finfo(np.float64).tiny)
    frac = float(np.max(np.abs(h - ref) / bound))
    return frac <= 1.0, frac


class Tally:
    def __init__(self):
        self.executed = 0
        self.graphs = -1
        self.hist = {k: 0.0 for k in SOLVES}               # largest history deviation / bound
        self.state = 0.0                                   # largest relative state deviation through the sine-transform bottom solve
        self.state_pcg = 0.0                               # ... after mgx_solve_pcg
        self.state_gcr = 0.0                               # ... after mgx_solve_gcr
        self.state_refine_gcr = 0.0                        # ... of U[finest] after mgx_solve_refine_gcr
        self.graph_counts = []
        self.histories = []                                # of the device, in call order
        self.final = None                                  # U and B of every level after the last call
        self.steps_hist = {}                               # theta_steps / newton / newton_steps by solver inside: largest history deviation / bound
        self.steps_state = {}                              # ... largest deviation of a written array or the term / bound (Krylov solvers inside)
        self.bound = 0.0                                   # line cases: the largest bound of the tolerance rule used
        self.ratio = 0.0                                   # ... and the largest device deviation / its bound


def step(pkg, mg, m, cfg, call, tally, where, rows=0):
    """one call on both sides, then every level's U and B, the history and the statistics.  rows: MGX_ROWS of the
    environment the handle was created under (apply_model)"""
    L, Lc = cfg["finest_level"], cfg["coarsest_level"]
    g_before, h_before = mg.graphs_cached(), m.h
    got = apply_device(pkg, mg, call, L, hm.BILINEAR if m.transfer is None else m.transfer, m)
    want = apply_model(m, call, L, got, rows)
    tally.executed += 1
    if call[0] == "set_cycle":                             # the graph key carries no kind: the setter has to drop the graphs
        assert mg.cycle == m.cycle == call[1], where()
        assert mg.graphs_cached() == (0 if g_before >= 0 else -1), f"{mg.graphs_cached()} graphs after mgx_set_cycle; {where()}"
    if call[0] in SOLVES:
        (st, h), (st_m, h_m) = got, want
        tally.histories.append(np.array(h))
        ok, frac = history_check(cfg, call, h, h_m)
        tally.hist[call[0]] = max(tally.hist[call[0]], frac if np.isfinite(frac) else 0.0)
        assert ok, f"history {frac:.3g} x its bound: {h} vs {h_m}; {where()}"
        assert (st.cycles, st.converged, st.fine_updates) == (st_m["cycles"], st_m["converged"], st_m["fine_updates"]), \
            f"stats {(st.cycles, st.converged, st.fine_updates)} vs {st_m}; {where()}"
    elif call[0] == "residual":
        assert np.array_equal(got, want), f"R of level {call[1]}; {where()}"
    elif call[0] in STEP_CALLS or call[0] in STEP_TIMING or call[0] in ("set_reaction", "get_reaction", "residual_norm") or \
            (call[0] == "build_galerkin" and m.d is not None):     # (a build under a term: the shifted centre went into the hierarchy)
        step_checks(pkg, mg, m, cfg, call, got, want, tally, where, g_before, h_before)
    rtol = state_tolerance(cfg, call)
    loose = touched(cfg, call) if rtol else set()
    for lv in range(Lc, L + 1):
        for which, name in ((pkg.VEC_U, "U"), (pkg.VEC_B, "B")):
            a, r = mg.get_level(lv, which), m.get_level(lv, 0 if which == pkg.VEC_U else 1)
            assert a.dtype == r.dtype and a.shape == r.shape
            if (lv, name) not in loose:
                if not np.array_equal(a, r):
                    bad = np.argwhere(a != r)
                    raise AssertionError(f"{name} of level {lv} differs at {len(bad)} points, first {tuple(bad[0])}: "
                                         f"{a[tuple(bad[0])]!r} vs {r[tuple(bad[0])]!r}; {where()}")
            else:
                dev = float(np.max(np.abs(a.astype(np.float64) - r.astype(np.float64)))) / max(float(np.max(np.abs(r))), 1e-300)
                if call[0] == "solve_pcg":
                    tally.state_pcg = max(tally.state_pcg, dev)
                elif call[0] == "solve_gcr":
                    tally.state_gcr = max(tally.state_gcr, dev)
                elif call[0] == "solve_refine_gcr":
                    tally.state_refine_gcr = max(tally.state_refine_gcr, dev)
                elif call[0] in STEP_CALLS:
                    label = f"{call[0]}/{('solve', 'gcr', 'refine_gcr')[inner_solver(call)]}"
                    tally.steps_state[label] = max(tally.steps_state.get(label, 0.0), dev / rtol)
                else:
                    tally.state = max(tally.state, dev)
                assert dev <= rtol, f"{name} of level {lv} off by {dev:.3g} (bound {rtol:g}); {where()}"
                m.set_level(lv, 0 if which == pkg.VEC_U else 1, a)
    g = mg.graphs_cached()
    tally.graph_counts.append(g)
    tally.graphs = max(tally.graphs, g)
    return got


def run_sequence(pkg, po, cfg, calls, seed, env=None):
    tally = Tally()
    done = []

    def where():
        return f"seed {seed}, step {len(done) - 1} of {len(calls)}, cfg {cfg}, env {env}, calls so far {done}"

    m = hm.HandleModel(po, **cfg)
    with pkg.Multigrid(**cfg) as mg:
        for call in calls:
            done.append(call)
            step(pkg, mg, m, cfg, call, tally, where, int((env or {}).get("MGX_ROWS", 0)))
        tally.final = all_levels(pkg, mg, cfg["finest_level"], cfg["coarsest_level"])
    assert tally.executed == len(calls)                    # nothing skipped, nothing filtered
    users = {k: sum(1 for c in calls if c[0] == k) for k in graph_users(calls)}
    assert min(users.values()) >= 5, users
    krylov_bound = RTOL64 if cfg.get("dtype", hm.F64) == hm.F64 else PCG32_STATE
    print(f"\n[handle-state] cfg={cfg} env={env} seed={seed} steps={tally.executed} graph_users={users} "
          f"max_graphs={tally.graphs} hist_solve={tally.hist['solve']:.3g}xbound hist_pcg={tally.hist['solve_pcg']:.3g}xbound "
          f"hist_gcr={tally.hist['solve_gcr']:.3g}xbound hist_refine={tally.hist['solve_refine']:.3g}xbound "
          f"hist_refine_gcr={tally.hist['solve_refine_gcr']:.3g}xbound state_dev_bottom={tally.state:.3g} "
          f"state_dev_pcg={tally.state_pcg:.3g} ({tally.state_pcg / krylov_bound:.3g}xbound) state_dev_gcr={tally.state_gcr:.3g} "
          f"({tally.state_gcr / krylov_bound:.3g}xbound) state_dev_refine_gcr={tally.state_refine_gcr:.3g} "
          f"({tally.state_refine_gcr / RTOL64:.3g}xbound) graphs={tally.graph_counts}")
    if tally.steps_hist or tally.steps_state:
        print(f"[handle-state] steps: history / bound {({k: float(f'{v:.3g}') for k, v in sorted(tally.steps_hist.items())})} "
              f"written state / bound {({k: float(f'{v:.3g}') for k, v in sorted(tally.steps_state.items())})}")
    return tally


def set_knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


# ---- 2. seeded call sequences --------------------------------------------------------------------------------------
P85 = dict(finest_level=8, coarsest_level=5, mu0=0, mu1=3, mu2=2, schedule=hm.V)
POISSON_CASES = {
    # name: (configuration, seed)
    "f64_jacobi_V": (dict(P85), 8501),
    "f64_rbgs_V_fw16": (dict(P85, smoother=hm.RBGS, restrict_mode=hm.FW16), 8502),
    "f64_jacobi_FMG_smooth_bottom": (dict(P85, schedule=hm.FMG, mu0=1, bottom=hm.SMOOTH), 8503),
    "f64_jacobi_V_fma": (dict(P85, arith=hm.FMA), 8504),
    "f32_jacobi_V_smooth_bottom": (dict(P85, dtype=hm.F32, bottom=hm.SMOOTH), 8505),
    "f32_rbgs_FMG_fw16_smooth_bottom": (dict(P85, dtype=hm.F32, smoother=hm.RBGS, schedule=hm.FMG, restrict_mode=hm.FW16, bottom=hm.SMOOTH), 8506),
}


@pytest.mark.parametrize("knobs", ["tiles", "streaming"])
@pytest.mark.parametrize("name", list(POISSON_CASES))
def test_poisson_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name, knobs):
    cfg, seed = POISSON_CASES[name]
    env = STREAMING if knobs == "streaming" else {}
    set_knobs(monkeypatch, env)                            # before the handle is created: the knobs are read there
    calls = draw_sequence(seed, cfg)
    tally = run_sequence(pkg, po, cfg, calls, seed, env)
    assert 1 <= tally.graphs <= K_MAX_GRAPHS


GENERAL_CASES = {
    "stencil5_f64_jacobi": (dict(P85, op=hm.STENCIL5), 8511),
    "stencil5_f32_chebyshev": (dict(P85, op=hm.STENCIL5, dtype=hm.F32, smoother=hm.CHEBYSHEV), 8512),
    "stencil5_f64_chebyshev_FMG_fw16": (dict(P85, op=hm.STENCIL5, smoother=hm.CHEBYSHEV, schedule=hm.FMG, restrict_mode=hm.FW16), 8513),
    "galerkin_f64_jacobi": (dict(P85, op=hm.GALERKIN), 8521),
    "galerkin_f64_chebyshev_smooth_bottom": (dict(P85, op=hm.GALERKIN, smoother=hm.CHEBYSHEV, bottom=hm.SMOOTH), 8522),
    # (bottom = SMOOTH: the reference's level-5 inverse takes seconds per operator, and this case has three)
    "galerkin_f32_jacobi_fw16_smooth_bottom": (dict(P85, op=hm.GALERKIN, dtype=hm.F32, restrict_mode=hm.FW16, bottom=hm.SMOOTH), 8523),
}


@pytest.mark.parametrize("name", list(GENERAL_CASES))
def test_general_operator_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name):
    """STENCIL5: two more set_coefficient calls with other contrast fields between graph users.  GALERKIN: rebuilds
    BILINEAR -> OPERATOR -> BILINEAR -> OPERATOR between graph users, then set_coefficient followed by a rebuild.
    A graph that survived one of them would replay the old operator, weights or Chebyshev coefficients."""
    cfg, seed = GENERAL_CASES[name]
    set_knobs(monkeypatch, {})
    calls = draw_sequence(seed, cfg)
    kinds = [c for c in calls if c[0] in ("set_coefficient", "build_galerkin")]
    if cfg["op"] == hm.STENCIL5:
        assert [c[1] for c in kinds] == [10.0, 100.0, 1000.0]
    else:
        assert [c[-1] for c in kinds if c[0] == "build_galerkin"] == [hm.BILINEAR, hm.OPERATOR, hm.BILINEAR, hm.OPERATOR, hm.BILINEAR]
        assert calls[[i for i, c in enumerate(calls) if c[0] == "set_coefficient"][-1] + 1] == ("build_galerkin", hm.BILINEAR)
    tally = run_sequence(pkg, po, cfg, calls, seed)
    assert 1 <= tally.graphs <= K_MAX_GRAPHS


def test_five_level_sequence_matches_the_model_after_every_call(pkg, po, monkeypatch):
    cfg = dict(finest_level=9, coarsest_level=5, mu0=0, mu1=2, mu2=1, schedule=hm.V, smoother=hm.RBGS)
    set_knobs(monkeypatch, {})
    tally = run_sequence(pkg, po, cfg, draw_sequence(9501, cfg), 9501)
    assert 1 <= tally.graphs <= K_MAX_GRAPHS


# ---- 2b. the cycle index ---------------------------------------------------------------------------------------------
G73 = dict(finest_level=7, coarsest_level=3, mu0=0, mu1=3, mu2=2, schedule=hm.V, op=hm.GALERKIN)
CYCLE_CASES = {
    # name: (configuration, seed, also with MGX_SMALL_VISIT=0)
    # levels 6, 5, 4 take k_small_visit, with turns on each; a 15^2 and a 7^2 level; the dense solve at level 3
    "galerkin_f64_jacobi_7_3": (dict(G73), 8531, True),
    # float lanes (1 x 4 vectors), rscale = 1/4
    "galerkin_f32_jacobi_fw16_7_3": (dict(G73, dtype=hm.F32, restrict_mode=hm.FW16, bottom=hm.SMOOTH), 8532, True),
    # level 6 is the only fused level, next to the coarsest; level 7 takes the per-level launches
    "galerkin_f64_jacobi_8_5_smooth_bottom": (dict(P85, op=hm.GALERKIN, bottom=hm.SMOOTH), 8533, True),
    # W / F through the per-level launches only; the dense solve at level 4
    "galerkin_f64_chebyshev_7_4": (dict(G73, coarsest_level=4, smoother=hm.CHEBYSHEV), 8534, False),
    # no nine-point level: never the visit kernel
    "stencil5_f64_jacobi_8_5": (dict(P85, op=hm.STENCIL5), 8535, False),
}


def assert_cycle_calls(calls, cfg):
    """what draw_sequence(cycles=True) promises, on the drawn list"""
    users = [i for i, c in enumerate(calls) if c[0] in graph_users(calls)]
    sets = [i for i, c in enumerate(calls) if c[0] == "set_cycle"]
    assert tuple(calls[i][1] for i in sets) == CYCLE_ORDER
    for k, i in enumerate(sets):                           # after every second graph user (an operator change may stand between;
        assert sum(1 for u in users if u < i and calls[u][0] not in REFINE_USERS) == 2 * (k + 1), (k, i)    # refines are placed later)
    kinds = kinds_at(calls)
    for lv in small_levels(cfg):
        for kind in (hm.CYCLE_W, hm.CYCLE_F):
            assert any(c == ("vcycle", lv) and k == kind for c, k in zip(calls, kinds)), (lv, kind)
    # the first graph user after every change of kind: where a graph of the old kind would replay
    for i in sets:
        assert any(u > i for u in users), i


@pytest.mark.parametrize("name", list(CYCLE_CASES))
def test_cycle_index_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name):
    """set_cycle W, F, V, W, F, W, V between the graph users, besides the operator changes; cycles started from every
    small level under W and under F.  U and B of EVERY level bit for bit after every call (solve_pcg as in
    GENERAL_CASES), so what a W- or F-cycle leaves on levels 6, 5, 4 is held, and the dense coarsest solve at levels 3
    and 4.  The Jacobi GALERKIN cases a second time with MGX_SMALL_VISIT=0 against the same model: the in-place visit
    kernel and the swapping per-level launches leave other buffer assignments behind, and the same bits."""
    cfg, seed, both = CYCLE_CASES[name]
    calls = draw_sequence(seed, cfg, cycles=True)
    assert_cycle_calls(calls, cfg)
    runs = []
    for env in ([{}, {"MGX_SMALL_VISIT": "0"}] if both else [{}]):
        set_knobs(monkeypatch, env)
        tally = run_sequence(pkg, po, cfg, calls, seed, env)
        assert 1 <= tally.graphs <= K_MAX_GRAPHS
        runs.append(tally)
    if both:
        a, b = runs
        for x, y in zip(a.final, b.final):
            assert np.array_equal(x, y)
        assert len(a.histories) == len(b.histories) and all(np.array_equal(x, y) for x, y in zip(a.histories, b.histories))


def test_a_refused_set_cycle_leaves_the_graphs_and_the_next_solve_alone(pkg, po, monkeypatch):
    """POISSON: mgx_set_cycle(W) is MGX_ERR_STATE.  The refusal must come before the setter drops anything: the graphs
    stay, and the next solve is the solve of a handle that never made the call - bits, history, fine_updates"""
    set_knobs(monkeypatch, {})
    cfg = dict(P85)
    L, Lc = 8, 5
    calls = [("set_rhs", 91), ("set_guess", 92), ("solve", 0.0, 2), ("vcycle_zero",), ("smooth", 6, 1), ("solve_pcg", 0.0, 2)]
    with pkg.Multigrid(**cfg) as plain, pkg.Multigrid(**cfg) as mg:
        for call in calls:
            apply_device(pkg, plain, call, L)
            apply_device(pkg, mg, call, L)
        g = mg.graphs_cached()
        assert g >= 1 and plain.graphs_cached() == g
        assert pkg.lib().mgx_set_cycle(mg._h, hm.CYCLE_W) == 5          # MGX_ERR_STATE
        assert mg.graphs_cached() == g and mg.cycle == hm.CYCLE_V
        with pytest.raises(RuntimeError):
            hm.HandleModel(po, **cfg).set_cycle(hm.CYCLE_W)
        for call in [("solve", 0.0, 2), ("vcycle_zero",), ("solve_pcg", 0.0, 1)]:
            a, b = apply_device(pkg, plain, call, L), apply_device(pkg, mg, call, L)
            for x, y in zip(all_levels(pkg, plain, L, Lc), all_levels(pkg, mg, L, Lc)):
                assert np.array_equal(x, y), call
            if a is not None:
                assert np.array_equal(a[1], b[1]), (call, a[1], b[1])
                assert (a[0].cycles, a[0].converged, a[0].fine_updates) == (b[0].cycles, b[0].converged, b[0].fine_updates), call
            assert mg.graphs_cached() == plain.graphs_cached() >= g


# ---- 2c. the line smoothers ------------------------------------------------------------------------------------------
L63 = dict(finest_level=6, coarsest_level=3, mu0=0, mu1=1, mu2=1, schedule=hm.V)
LINE_CASES = {
    # name: (configuration, seed, environment, generator options)
    "galerkin_f64_alt_6_3_cycles": (
        dict(L63, op=hm.GALERKIN, smoother=hm.LINE_ALT), 8541, {},
        dict(cycles=True, operators=("layers", [[("set_operator", "x1e-2")], [("build_galerkin", hm.OPERATOR)], [("set_operator", "contrast")],
                                                [("set_operator", "layers")]]))),
    # float: a zebra x-line sweep all but solves these operators, so every coarse right-hand side is a difference that
    # cancels to 1e-2 .. 1e-3 of its operands and the rule's bound is within a small factor of the cap (PCG32_STATE) after ONE
    # cycle.  Measured on the CPU (the two models alone), x1e-2: one cycle 2.4e-4, one PCG iteration 2e-4, two 7.2e-4, three
    # 1.1e-3, fmg 5e-4 .. 2e-3; x1e-3: one cycle 1.0e-3 .. 1.8e-3, a solve of two cycles 6.8e-2.  The cap stays; the sequence
    # keeps under it by construction: one cycle per solve, one iteration per solve_pcg, no fmg, and the x1e-3 operator at
    # the end, followed by a sweep on every level (the rebuilt factors of every level; the bound of a sweep is 1e-4).
    # Replays after an operator change are the double cases'
    "galerkin_f32_x_fw16_6_3": (
        dict(L63, op=hm.GALERKIN, smoother=hm.LINE_X, dtype=hm.F32, restrict_mode=hm.FW16), 8542, {},
        dict(operators=("x1e-2", []), short_solves=True, without=("fmg",),
             tail=[("set_operator", "x1e-3")] + [("smooth", lv, mu) for lv, mu in ((6, 1), (5, 3), (4, 1), (3, 2))] + [("residual", 6), ("restrict", 6)])),
    # the carries through LDS on levels 7 and 6 (127 and 63 rows in chunks of 16), inside cycles and replays
    "galerkin_f64_y_7_4_chunk16": (
        dict(L63, finest_level=7, coarsest_level=4, op=hm.GALERKIN, smoother=hm.LINE_Y), 8543, {"MGX_LINE_CHUNK": "16"},
        dict(operators=("y1e-2", [[("set_operator", "layers")]]))),
    "stencil5_f64_alt_6_3_smooth_bottom_cycles": (
        dict(L63, op=hm.STENCIL5, smoother=hm.LINE_ALT, bottom=hm.SMOOTH), 8544, {},
        dict(cycles=True, operators=("x1e-2", [[("set_operator", "layers")]]))),
}
LINE_OPTIONS = dict(fresh_guess=True)


def line_cap(cfg):
    return RTOL64 if cfg.get("dtype", hm.F64) == hm.F64 else PCG32_STATE


def line_models(po, cfg):
    """the model in the working type and in np.longdouble"""
    return hm.HandleModel(po, **cfg), hm.HandleModel(po, real=np.longdouble, **cfg)


def line_call(m, mx, cfg, call):
    """one call on both models from the state of `m`.  Returns (want, far, bounds): the two results, and for a call that
    smooths {(level, 'U' / 'B'): (bound, scale)} of THE TOLERANCE RULE for every array it writes; scale = max |x| of
    the long-double array (0: the array is zero in both models, nothing to scale by: bit for bit)"""
    L = cfg["finest_level"]
    for lv in m.levels():
        mx.set_level(lv, 0, m.U[lv])
        mx.set_level(lv, 1, m.B[lv])
    mx.fine_updates = m.fine_updates
    want, far = apply_model(m, call, L), apply_model(mx, call, L)
    bounds = {}
    if call[0] in SMOOTHING:
        for lv, name in touched(cfg, call):
            r, x = m.get_level(lv, 0 if name == "U" else 1), mx.get_level(lv, 0 if name == "U" else 1)
            scale = float(np.max(np.abs(x)))
            if scale == 0.0:
                assert not r.any(), (lv, name, call)
                bounds[lv, name] = (0.0, 0.0)
            else:
                bounds[lv, name] = (rule_bound(r, x)[0], scale)
    return want, far, bounds


def line_history_check(h, h_m, h_x):
    """history_bound of tests/test_gpu_line.py; (ok, deviation / bound)"""
    h, h_m, h_x = np.asarray(h), np.asarray(h_m), np.asarray(h_x, dtype=np.float64)
    if len(h) != len(h_m):
        return False, np.inf
    frac = float(np.max(np.abs(h - h_m)) / np.max(h_m)) / history_bound(h_m, h_x)
    return frac <= 1.0, frac


def line_step(pkg, mg, twin, m, mx, cfg, call, tally, where):
    L, Lc = cfg["finest_level"], cfg["coarsest_level"]
    transfer = hm.BILINEAR if m.transfer is None else m.transfer
    g_before = mg.graphs_cached()
    got, got_t = apply_device(pkg, mg, call, L, transfer), apply_device(pkg, twin, call, L, transfer)
    want, far, bounds = line_call(m, mx, cfg, call)
    tally.executed += 1
    if call[0] == "set_cycle":
        assert mg.cycle == twin.cycle == m.cycle == call[1], where()
        assert mg.graphs_cached() == (0 if g_before >= 0 else -1), f"{mg.graphs_cached()} graphs after mgx_set_cycle; {where()}"
    if call[0] in SOLVES:
        (st, h), (st_t, h_t), (st_m, h_m), (_, h_x) = got, got_t, want, far
        ok, frac = line_history_check(h, h_m, h_x)
        tally.hist[call[0]] = max(tally.hist[call[0]], frac if np.isfinite(frac) else 0.0)
        assert ok, f"history {frac:.3g} x its bound: {h} vs {h_m} (long double {h_x}); {where()}"
        assert (st.cycles, st.converged, st.fine_updates) == (st_m["cycles"], st_m["converged"], st_m["fine_updates"]), \
            f"stats {(st.cycles, st.converged, st.fine_updates)} vs {st_m}; {where()}"
        assert np.array_equal(h, h_t), f"replaying and eager handle: histories {h} vs {h_t}; {where()}"
        assert (st.cycles, st.converged, st.fine_updates) == (st_t.cycles, st_t.converged, st_t.fine_updates), where()
    elif call[0] == "residual":
        assert np.array_equal(got, want) and np.array_equal(got, got_t), f"R of level {call[1]}; {where()}"
    cap = line_cap(cfg)
    for lv in range(Lc, L + 1):
        for which, name in ((pkg.VEC_U, "U"), (pkg.VEC_B, "B")):
            w = 0 if which == pkg.VEC_U else 1
            a, r = mg.get_level(lv, which), m.get_level(lv, w)
            assert a.dtype == r.dtype and a.shape == r.shape
            assert np.array_equal(a, twin.get_level(lv, which)), f"{name} of level {lv}: the replaying and the eager handle differ; {where()}"
            bound, scale = bounds.get((lv, name), (0.0, 0.0))
            if scale == 0.0:
                if not np.array_equal(a, r):
                    bad = np.argwhere(a != r)
                    raise AssertionError(f"{name} of level {lv} differs at {len(bad)} points, first {tuple(bad[0])}: "
                                         f"{a[tuple(bad[0])]!r} vs {r[tuple(bad[0])]!r}; {where()}")
                continue
            assert bound <= cap, f"bound too loose: {bound:.3g} > {cap:g} for {name} of level {lv}; {where()}"
            al = a.astype(np.longdouble)
            dev = max(float(np.max(np.abs(al - r.astype(np.longdouble)))), float(np.max(np.abs(al - mx.get_level(lv, w))))) / scale
            tally.bound = max(tally.bound, bound)
            tally.ratio = max(tally.ratio, dev / bound)
            assert dev <= bound, f"{name} of level {lv} off by {dev:.3g}, {dev / bound:.3g} x its bound {bound:.3g}; {where()}"
            m.set_level(lv, w, a)                          # (mx takes m's state before its next call)
    g = mg.graphs_cached()
    tally.graph_counts.append(g)
    tally.graphs = max(tally.graphs, g)
    assert twin.graphs_cached() == -1


@pytest.mark.parametrize("name", list(LINE_CASES))
def test_line_smoother_sequences_follow_the_models_after_every_call(pkg, po, monkeypatch, name):
    cfg, seed, env, options = LINE_CASES[name]
    calls = draw_sequence(seed, cfg, **LINE_OPTIONS, **options)
    if options.get("cycles"):
        assert_cycle_calls(calls, cfg)
    wanted = [options["operators"][0]] + [c[1] for g in list(options["operators"][1]) + [options.get("tail", [])] for c in g if c[0] == "set_operator"]
    assert [c[1] for c in calls if c[0] == "set_operator"] == wanted
    run_line_sequence(pkg, po, monkeypatch, cfg, calls, seed, env)


def run_line_sequence(pkg, po, monkeypatch, cfg, calls, seed, env):
    """a replaying handle and its MGX_GRAPH=0 twin through `calls`, both models beside them (line_step)"""
    tally = Tally()
    done = []

    def where():
        return f"seed {seed}, step {len(done) - 1} of {len(calls)}, cfg {cfg}, env {env}, calls so far {done}"

    m, mx = line_models(po, cfg)
    set_knobs(monkeypatch, dict(env, MGX_GRAPH="0"))
    twin = pkg.Multigrid(**cfg)
    set_knobs(monkeypatch, env)
    try:
        with pkg.Multigrid(**cfg) as mg:
            assert mg.graphs_cached() == 0 and twin.graphs_cached() == -1
            for call in calls:
                done.append(call)
                line_step(pkg, mg, twin, m, mx, cfg, call, tally, where)
                if len(done) == 1 and "MGX_LINE_CHUNK" in env:
                    chunk = int(env["MGX_LINE_CHUNK"])
                    for lv in (7, 6):                      # the override took effect: more than one chunk on both levels
                        assert mg.line_chunks(lv) == (chunk, -(-((1 << lv) - 1) // chunk)), mg.line_chunks(lv)
    finally:
        twin.close()
    assert tally.executed == len(calls)
    users = {k: sum(1 for c in calls if c[0] == k) for k in graph_users(calls)}
    assert min(users.values()) >= 5, users
    assert 1 <= tally.graphs <= K_MAX_GRAPHS
    print(f"\n[handle-state] line cfg={cfg} env={env} seed={seed} steps={tally.executed} of {len(calls)} drawn graph_users={users} "
          f"max_graphs={tally.graphs} hist_solve={tally.hist['solve']:.3g}xbound hist_pcg={tally.hist['solve_pcg']:.3g}xbound "
          f"hist_gcr={tally.hist['solve_gcr']:.3g}xbound "
          f"largest_bound={tally.bound:.3g} (cap {line_cap(cfg):g}) largest_device_to_bound_ratio={tally.ratio:.3g}")
    return tally


def test_a_line_smoother_keeps_small_levels_off_the_visit_kernel(pkg, po, monkeypatch):
    """k_small_visit is Jacobi's: a W-cycle of a LINE_ALT GALERKIN handle on 6..3 pays the same launches below the finest
    level with MGX_SMALL_VISIT 1 and 0 (cfg.profile = 1: every launch eager and counted), and computes the same bits"""
    cfg = dict(LINE_CASES["galerkin_f64_alt_6_3_cycles"][0], profile=1)
    out = []
    for small in ("1", "0"):
        set_knobs(monkeypatch, {"MGX_SMALL_VISIT": small})
        with pkg.Multigrid(**cfg) as mg:
            for call in [("set_operator", "layers"), ("set_cycle", hm.CYCLE_W), ("set_rhs", 95), ("solve", 0.0, 2)]:
                apply_device(pkg, mg, call, 6)
            out.append((mg.profile()["launches"][4], mg.get_solution()))          # MGX_PROF_COARSE
    assert out[0][0] == out[1][0] > 0, (out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1])


# ---- 2d. mgx_solve_gcr among the graph users -------------------------------------------------------------------------
# Weak smoothing throughout: the deep call (DEEP_GCR) must not take the iterate into the cancellation regime of b - A u,
# where a bound relative to max |x| means nothing - tests/test_handle_model.py walks the model alone through every case
# and holds every fp64 solve_gcr / solve_pcg to a last history entry at or above 1e-6 of its first.
P85_WEAK = dict(P85, mu1=1, mu2=0)
G73_WEAK = dict(G73, mu1=1, mu2=0)
GCR_CASES = {
    # name: (configuration, seed, environments, generator options, through line_step)
    "poisson_f64_jacobi_8_5": (dict(P85_WEAK), 8551, [{}], {}, False),
    "poisson_f64_jacobi_8_5_streaming": (dict(P85_WEAK), 8552, [STREAMING], {}, False),
    "poisson_f32_rbgs_smooth_bottom_8_5": (dict(P85_WEAK, dtype=hm.F32, smoother=hm.RBGS, bottom=hm.SMOOTH), 8558, [{}], {}, False),
    # the two set_coefficient changes between the graph users
    "stencil5_f64_chebyshev_8_5": (dict(P85_WEAK, op=hm.STENCIL5, smoother=hm.CHEBYSHEV), 8554, [{}], {}, False),
    # set_cycle through CYCLE_ORDER and the BILINEAR / OPERATOR rebuilds; with and without k_small_visit against the same model
    "galerkin_f64_jacobi_7_3_cycles": (dict(G73_WEAK), 8555, [{}, {"MGX_SMALL_VISIT": "0"}], dict(cycles=True), False),
    "galerkin_f32_jacobi_fw16_smooth_bottom_7_3_cycles": (dict(G73_WEAK, dtype=hm.F32, restrict_mode=hm.FW16, bottom=hm.SMOOTH), 8556, [{}],
                                                          dict(cycles=True), False),
    # the rule bound against the long-double model, and the MGX_GRAPH=0 twin.  The alternating line cycle V(1,0) reduces the
    # residual by 5e-2 .. 7e-2 per GCR iteration: nine iterations of the deep call end at 4.5e-12 of the first entry with a
    # rule bound of 1.2e-7, six at 2.2e-8, five at 2.8e-7, four at 5.3e-6 (bound 4.9e-13) - measured on the CPU, the two
    # models alone.  So this case's deep call is shortened to four iterations: the basis still grows to eight pairs, slots
    # 0 .. 3 are written; the full basis and its wrap are the other double cases'
    "galerkin_f64_alt_6_3_line": (dict(L63, mu2=0, op=hm.GALERKIN, smoother=hm.LINE_ALT), 8557, [{}],
                                  dict(LINE_OPTIONS, operators=("layers", [[("set_operator", "x1e-2")], [("build_galerkin", hm.OPERATOR)],
                                                                           [("set_operator", "contrast")]]), deep_iters=4), True),
}


def assert_gcr_calls(calls, cfg, fresh_guess=False, deep_iters=DEEP_GCR[2]):
    """what draw_sequence(gcr=True) promises, on the drawn list"""
    f64 = cfg.get("dtype", hm.F64) == hm.F64
    at = [i for i, c in enumerate(calls) if c[0] == "solve_gcr"]
    assert len(at) >= 5 and min(sum(1 for c in calls if c[0] == k) for k in GCR_USERS) >= 5
    assert calls[at[0]][3] == 2                                   # the basis of the first call: two pairs
    deep = [i for i in at if calls[i] == DEEP_GCR[:2] + (deep_iters,) + DEEP_GCR[3:]]
    for i in at:
        tol, iters, restart = calls[i][1:]
        if i in deep:
            continue
        assert tol in ((0.0, 1e-3) if f64 else (0.0, 1e-2)) and 1 <= iters <= 4 and restart in GCR_RESTARTS, calls[i]
        if fresh_guess:
            assert calls[i - 1][0] == "set_guess", i
    if f64:
        assert len(deep) == 1 and deep[0] > at[0] and calls[deep[0] - 1][0] == "set_guess"
        before = {c[0] for c in calls[:deep[0]]}
        assert "solve" in before and "solve_pcg" in before        # the basis grows on a handle the others have used
    else:
        assert not deep and all(c[2] <= 4 for c in calls if c[0] == "solve_gcr")
    assert any(calls[i][2] > calls[i][3] for i in at if i not in deep)          # a wrap of a short basis


def krylov_order(calls):
    """'pcg' / 'gcr': which of the two Krylov solves a sequence runs first (they share one workspace)"""
    return next("pcg" if c[0] == "solve_pcg" else "gcr" for c in calls if c[0] in KRYLOV)


@pytest.mark.parametrize("name", list(GCR_CASES))
def test_gcr_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name):
    """mgx_solve_gcr as a fourth graph user: cycle_body through the graph cache with lv[L].b repointed at r, on the
    workspace mgx_solve_pcg shares (csrc/mgx_krylov_host.hpp).  U and B of every level after every call as for solve_pcg
    (module docstring); the Jacobi GALERKIN case with and without the visit kernel, bit-equal between the two runs; the
    line case through line_step"""
    cfg, seed, envs, options, line = GCR_CASES[name]
    calls = draw_sequence(seed, cfg, gcr=True, **options)
    assert_gcr_calls(calls, cfg, options.get("fresh_guess", False), options.get("deep_iters", DEEP_GCR[2]))
    if options.get("cycles"):
        assert_cycle_calls(calls, cfg)
    runs = []
    for env in envs:
        if line:
            runs.append(run_line_sequence(pkg, po, monkeypatch, cfg, calls, seed, env))
            continue
        set_knobs(monkeypatch, env)
        tally = run_sequence(pkg, po, cfg, calls, seed, env)
        assert 1 <= tally.graphs <= K_MAX_GRAPHS
        runs.append(tally)
    if len(runs) == 2:
        a, b = runs
        for x, y in zip(a.final, b.final):
            assert np.array_equal(x, y)
        assert len(a.histories) == len(b.histories) and all(np.array_equal(x, y) for x, y in zip(a.histories, b.histories))


# ---- 2e. the colour smoothers and nine-point finest levels -----------------------------------------------------------
def run_under(pkg, po, monkeypatch, cfg, calls, seed, envs):
    """the sequence once per environment against a fresh model each; every run leaves the final state and the histories
    of the first one, bit for bit"""
    runs = []
    for env in envs:
        set_knobs(monkeypatch, env)
        tally = run_sequence(pkg, po, cfg, calls, seed, env)
        assert 1 <= tally.graphs <= K_MAX_GRAPHS
        runs.append(tally)
    a = runs[0]
    for b, env in zip(runs[1:], envs[1:]):
        for x, y in zip(a.final, b.final):
            assert np.array_equal(x, y), env
        assert len(a.histories) == len(b.histories) and all(np.array_equal(x, y) for x, y in zip(a.histories, b.histories)), env
    return runs


S73 = dict(G73, op=hm.STENCIL5)
UNFUSED, NO_VISIT = {"MGX_GS_FUSED": "0"}, {"MGX_SMALL_VISIT": "0"}
COLOUR_CASES = {
    # name: (configuration, seed, environments, generator options)
    # V(3,2): every level (N = 256 .. 32) runs k_gs_rb out of place, an odd and an even number of swaps per block; the in-place
    # per-colour form (MGX_GS_FUSED=0) leaves other buffer assignments behind and the same bits
    "stencil5_f64_gs_8_5": (dict(P85, op=hm.STENCIL5, smoother=hm.COLOR_GS), 8561, [{}, UNFUSED], {}),
    # levels 7 .. 4 swap, level 3 (N = 8) runs per colour in place; the bottom visit sweeps forward, then in reverse; W / F
    # pay second visits, whose blocks keep the direction of their position; cycles started from levels 6, 5, 4
    "stencil5_f32_sgs_7_3_smooth_bottom_cycles": (dict(S73, dtype=hm.F32, smoother=hm.COLOR_SGS, bottom=hm.SMOOTH), 8562, [{}], dict(cycles=True)),
    # only the finest level swaps; 6 .. 4 are nine-point, in place; the dense solve at level 3.  MGX_SMALL_VISIT: the
    # visit kernel is Jacobi's and must be bypassed, whatever the knob says
    "galerkin_f64_sgs_7_3_cycles": (dict(G73, smoother=hm.COLOR_SGS), 8563, [{}, NO_VISIT, UNFUSED], dict(cycles=True)),
    "galerkin_f32_gs_fw16_8_5_smooth_bottom": (dict(P85, op=hm.GALERKIN, dtype=hm.F32, smoother=hm.COLOR_GS, restrict_mode=hm.FW16, bottom=hm.SMOOTH),
                                               8564, [{}], {}),
}


@pytest.mark.parametrize("name", list(COLOUR_CASES))
def test_colour_smoother_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name):
    """COLOR_GS / COLOR_SGS (csrc/mgx_colour.hpp): the one smoother that swaps u / tmp on some levels of a handle and not
    on others, and whose blocks depend on their position in the cycle - a flag that travels through graph capture,
    cycle_body under PCG, mgx_fmg and mgx_vcycle(level) from any level.  U and B of EVERY level bit for bit after every
    call (solve_pcg as in GENERAL_CASES)"""
    cfg, seed, envs, options = COLOUR_CASES[name]
    calls = draw_sequence(seed, cfg, **options)
    if options.get("cycles"):
        assert_cycle_calls(calls, cfg)
    run_under(pkg, po, monkeypatch, cfg, calls, seed, envs)


def point_counts(calls):
    """9 / 5 / None: the point count of a GALERKIN handle's finest level after every call of a list"""
    out, count = [], None
    for c in calls:
        if c[0] in ("set_stencil9", "set_tensor") or (c[0] == "set_operator" and c[1] in hm.OPERATORS9):
            count = 9
        elif c[0] in ("set_stencil", "set_coefficient", "set_operator"):
            count = 5
        out.append(count)
    return out


def flips(calls):
    """the indices of the calls that change the finest level's point count"""
    counts = point_counts(calls)
    return [i for i in range(1, len(calls)) if counts[i] != counts[i - 1] and counts[i - 1] is not None]


def assert_nine_calls(calls, cfg, first, changes, krylov=False):
    """what a NINE_CASES sequence promises, on the drawn list: the operator changes in their order, every flip of the point
    count between two graph users - so the first user after it replays, or captures, on the flipped level.  krylov:
    solve_pcg and solve_gcr both run before the first flip and after the last one, and the first of the two after a flip
    is solve_pcg once and solve_gcr once: either method on the workspace the other point count left"""
    users = [i for i, c in enumerate(calls) if c[0] in graph_users(calls)]
    assert calls[0] == ("set_operator", first) and first in hm.OPERATORS9
    assert [c for c in calls[1:] if c[0] in ("set_operator", "set_coefficient", "build_galerkin", "set_tensor", "set_stencil9", "set_stencil")] == \
        [c for g in changes for c in g]
    at = flips(calls)
    assert len(at) >= 2 and {point_counts(calls)[i] for i in at} == {5, 9}, at
    for i in at:
        assert any(u < i for u in users) and any(u > i for u in users), i
    if krylov:
        for part in (calls[:at[0]], calls[at[-1]:]):
            assert {"solve_pcg", "solve_gcr"} <= {c[0] for c in part}
        firsts = [next(c[0] for c in calls[i:] if c[0] in KRYLOV) for i in at]
        assert set(firsts) == set(KRYLOV), firsts


NINE_CASES = {
    # name: (configuration, seed, environments, generator options); options["operators"] = (first, changes)
    # set_tensor; OPERATOR transfers; 9 -> 5 through set_coefficient; 5 -> 9 through set_tensor; another tensor
    "galerkin_f64_jacobi_7_3_nine_cycles": (
        dict(G73), 8571, [{}, NO_VISIT],
        dict(cycles=True, operators=("rot45", [[("build_galerkin", hm.OPERATOR)], [("set_coefficient", 100.0, 11), ("build_galerkin", hm.BILINEAR)],
                                               [("set_operator", "smooth9")], [("set_operator", "jump9")]]))),
    "galerkin_f32_chebyshev_fw16_7_4_nine_smooth_bottom": (
        dict(G73, coarsest_level=4, dtype=hm.F32, smoother=hm.CHEBYSHEV, restrict_mode=hm.FW16, bottom=hm.SMOOTH), 8572, [{}],
        dict(operators=("smooth9", [[("set_operator", "contrast")], [("set_operator", "rot45")]]))),
    # V(1,1): the reverse blocks exist; the finest level flips between in place (nine-point) and swapping (five-point), the
    # Krylov direction kernel between k_pcg_direction<T, 2> and <T, 1> on one workspace
    "galerkin_f64_sgs_7_3_nine_gcr": (
        dict(G73, mu1=1, mu2=1, smoother=hm.COLOR_SGS), 8580, [{}],
        dict(gcr=True, deep_iters=5, operators=("smooth9", [[("set_coefficient", 100.0, 11), ("build_galerkin", hm.BILINEAR)],
                                                            [("set_operator", "rot45")], [("build_galerkin", hm.OPERATOR)]]))),
    "galerkin_f64_gs_8_5_nine_gcr": (
        dict(P85_WEAK, op=hm.GALERKIN, smoother=hm.COLOR_GS, bottom=hm.SMOOTH), 8587, [{}],
        dict(gcr=True, operators=("rot45", [[("set_operator", "contrast")], [("set_operator", "smooth9")]]))),
}


@pytest.mark.parametrize("name", list(NINE_CASES))
def test_nine_point_finest_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name):
    """mgx_set_tensor / mgx_set_stencil9 and back (mgx_set_coefficient, mgx_set_stencil) between the graph users of one
    handle: lv[finest].nine flips, and with it every kernel on that level, the Krylov direction kernel, and under a colour
    smoother whether the level swaps.  U and B of EVERY level bit for bit after every call, the Krylov calls as in
    GCR_CASES (module docstring)"""
    cfg, seed, envs, options = NINE_CASES[name]
    calls = draw_sequence(seed, cfg, **options)
    assert_nine_calls(calls, cfg, *options["operators"], krylov=options.get("gcr", False))
    if options.get("cycles"):
        assert_cycle_calls(calls, cfg)
    if options.get("gcr"):
        assert_gcr_calls(calls, cfg, False, options.get("deep_iters", DEEP_GCR[2]))
    run_under(pkg, po, monkeypatch, cfg, calls, seed, envs)


# "random9" is unsymmetric: no solve_pcg.  One list, written by hand
RANDOM9_CALLS = (
    [("set_stencil9", "random9"), ("build_galerkin", hm.BILINEAR)] + [c for lv in range(3, 7) for c in (("set_u", lv, 1000 + lv), ("set_b", lv, 2000 + lv))]
    + [("solve", 0.0, 2), ("vcycle_zero",), ("smooth", 6, 1), ("solve_gcr", 0.0, 3, 3), ("vcycle", 6),
       ("set_stencil", "random5"), ("build_galerkin", hm.BILINEAR), ("solve", 0.0, 2), ("solve_gcr", 0.0, 3, 3),
       ("set_stencil9", "random9_ring"), ("build_galerkin", hm.BILINEAR), ("solve", 0.0, 2), ("solve_gcr", 0.0, 3, 3)])


@pytest.mark.parametrize("smoother", [hm.COLOR_GS, hm.JACOBI], ids=["gs", "jacobi"])
def test_an_unsymmetric_nine_point_operator_on_one_handle(pkg, po, monkeypatch, smoother):
    """mgx_set_stencil9 with corners, no symmetry and values in the ring-pointing places; then the unsymmetric five-point
    operator of tests/test_gpu_colour.py (9 -> 5); then the nine-point one again with other ring-pointing values, against
    the model that keeps the plain ones.  solve and solve_gcr run on both sides of either flip"""
    cfg = dict(finest_level=6, coarsest_level=3, mu0=0, mu1=1, mu2=1, schedule=hm.V, op=hm.GALERKIN, smoother=smoother)
    calls = list(RANDOM9_CALLS)
    assert not any(c[0] == "solve_pcg" for c in calls) and [point_counts(calls)[i] for i in flips(calls)] == [5, 9]
    set_knobs(monkeypatch, {})
    tally, done = Tally(), []

    def where():
        return f"random9 sequence, step {len(done) - 1} of {len(calls)}, cfg {cfg}, calls so far {done}"

    m = hm.HandleModel(po, **cfg)
    with pkg.Multigrid(**cfg) as mg:
        for call in calls:
            done.append(call)
            step(pkg, mg, m, cfg, call, tally, where)
    assert tally.executed == len(calls) and tally.graphs >= 1
    print(f"\n[handle-state] random9 cfg={cfg} steps={tally.executed} max_graphs={tally.graphs} hist_solve={tally.hist['solve']:.3g}xbound "
          f"hist_gcr={tally.hist['solve_gcr']:.3g}xbound state_dev_gcr={tally.state_gcr:.3g} ({tally.state_gcr / RTOL64:.3g}xbound)")


# ---- 2f. mgx_solve_refine among the graph users ----------------------------------------------------------------------
EAGER = {"MGX_GRAPH": "0"}
REFINE_OPTIONS = dict(refine=True, n_steps=30)             # (few calls drawn by weight: the refine stage adds about twenty-five)
REFINE_CASES = {
    # name: (configuration, seed, environments, generator options).  All double: the handles mgx_solve_refine takes
    # V(3,2); set_coefficient 100 and 1000 rewrite EVERY level of the float copy.  The float dense solve at level 5 of a
    # STENCIL5 handle: held bit for bit by test_general_operator_sequences_match_the_model_after_every_call[stencil5_f32_chebyshev]
    "stencil5_f64_jacobi_8_5_refine": (dict(P85, op=hm.STENCIL5), 8591, [{}], {}),
    # the float lambda bounds are kernel arguments of the float copy's captured cycle
    "stencil5_f64_chebyshev_8_5_refine": (dict(P85, op=hm.STENCIL5, smoother=hm.CHEBYSHEV), 8592, [{}], {}),
    # set_cycle through CYCLE_ORDER; BILINEAR -> OPERATOR -> BILINEAR -> OPERATOR with the same coefficients (the float copy
    # follows a transfer-only rebuild), then set_coefficient + BILINEAR.  The float copy takes the handle's knobs, not the
    # environment's: the same bits without the visit kernel and without graphs.  bottom = SMOOTH: no F32 sequence holds the
    # float dense solve of a GALERKIN hierarchy at level 3 against the model
    "galerkin_f64_jacobi_7_3_refine_cycles": (dict(G73, bottom=hm.SMOOTH), 8593, [{}, NO_VISIT, EAGER], dict(cycles=True)),
    # the finest level flips nine-point (in place) -> five-point (swapping) -> nine-point under the pass and under the float
    # cycle; bottom = SMOOTH for the same reason
    "galerkin_f64_sgs_7_3_nine_refine": (
        dict(G73, smoother=hm.COLOR_SGS, bottom=hm.SMOOTH), 8594, [{}, UNFUSED],
        dict(operators=("rot45", [[("set_coefficient", 100.0, 11), ("build_galerkin", hm.BILINEAR)], [("set_operator", "smooth9")]]))),
    # refine between Krylov calls on the shared workspace (one partial-sum buffer, one scalar block)
    "galerkin_f64_gs_8_5_smooth_bottom_refine_gcr": (dict(P85_WEAK, op=hm.GALERKIN, smoother=hm.COLOR_GS, bottom=hm.SMOOTH), 8595, [{}], dict(gcr=True)),
}


@pytest.mark.parametrize("name", list(REFINE_CASES))
def test_refine_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name):
    """mgx_solve_refine as one more graph user of a long-lived handle: a second solver inside the handle (the float copy,
    with a graph cache of its own, rebuilt lazily from a generation counter and told the cycle kind by hand), one u <-> tmp
    swap of the finest level per cycle under the parent's graph key, and the pass's sums in the partial-sum buffer
    mgx_solve, mgx_solve_pcg and mgx_solve_gcr share.  U and B of EVERY level bit for bit after every refine - so the
    parent's coarse levels are held untouched (the cycle runs in the float copy) - its history as mgx_solve's, its
    statistics equal; the model takes the scales from the device's history (apply_model)"""
    cfg, seed, envs, options = REFINE_CASES[name]
    calls = draw_sequence(seed, cfg, **REFINE_OPTIONS, **options)
    assert_refine_calls(calls, cfg, options.get("gcr", False))
    if options.get("cycles"):
        assert_cycle_calls(calls, cfg)
    if options.get("gcr"):
        assert_gcr_calls(calls, cfg)
    runs = []
    for env in envs:
        set_knobs(monkeypatch, env)
        tally = run_sequence(pkg, po, cfg, calls, seed, env)
        assert tally.graphs == -1 if env == EAGER else 1 <= tally.graphs <= K_MAX_GRAPHS, tally.graphs
        runs.append(tally)
    for b, env in zip(runs[1:], envs[1:]):
        for x, y in zip(runs[0].final, b.final):
            assert np.array_equal(x, y), env
        assert len(runs[0].histories) == len(b.histories) and all(np.array_equal(x, y) for x, y in zip(runs[0].histories, b.histories)), env


# ---- 2g. mgx_solve_refine_gcr among the graph users ------------------------------------------------------------------
REFINE_GCR_OPTIONS = dict(refine=True, gcr=True, refine_gcr=True, n_steps=30)
REFINE_GCR_CASES = {
    # name: (configuration, seed, environments, generator options).  All double.  The deep solve_gcr must stay out of the
    # cancellation regime of b - A u (GCR_CASES): weak smoothing in the GALERKIN cases.  The STENCIL5 case keeps V(3,2), as in
    # REFINE_CASES: its deep call comes after set_coefficient 1000, where GCR converges slowly (7.6e-4 over nine iterations),
    # and under V(1,0) a solve_refine of two cycles there grows from a fresh guess (x 5), which refine_stage relies on not
    # happening.  Every level of the float copy is rewritten by set_coefficient 100 (first user: solve_refine) and 1000
    # (solve_refine_gcr)
    "stencil5_f64_jacobi_8_5_refine_gcr": (dict(P85, op=hm.STENCIL5), 8601, [{}], {}),
    # set_cycle through CYCLE_ORDER, the transfer-only rebuilds; the same bits without the visit kernel and without graphs
    "galerkin_f64_jacobi_7_3_smooth_bottom_refine_gcr_cycles": (dict(G73_WEAK, bottom=hm.SMOOTH), 8602, [{}, NO_VISIT, EAGER], dict(cycles=True)),
    # k_refine_direction<9> -> <5> -> <9> on one workspace: set_tensor, set_coefficient, set_stencil9
    "galerkin_f64_sgs_7_3_nine_refine_gcr": (
        dict(G73, mu1=1, mu2=1, smoother=hm.COLOR_SGS, bottom=hm.SMOOTH), 8603, [{}],
        dict(deep_iters=5, operators=("rot45", [[("set_coefficient", 100.0, 11), ("build_galerkin", hm.BILINEAR)],
                                                [("set_stencil9", "smooth9"), ("build_galerkin", hm.BILINEAR)]]))),
}


@pytest.mark.parametrize("name", list(REFINE_GCR_CASES))
def test_refine_gcr_sequences_match_the_model_after_every_call(pkg, po, monkeypatch, name):
    """mgx_solve_refine_gcr as one more graph user of a long-lived handle.  It shares the float copy of the hierarchy (r32,
    z32, the cached cycle graphs) with mgx_solve_refine, the Krylov workspace, the scalar block and the partial sums with
    mgx_solve_gcr and mgx_solve_pcg, and keeps its residual in B of the finest level while it runs.  After every call U
    of the finest level to RTOL64 against the model (its dots summed in the device's order, its scales from the device's
    history), B and EVERY other level bit for bit - the call moves nothing else, which is where it differs from mgx_solve_gcr -
    the history as mgx_solve_gcr's, the statistics equal; mgx_time_refine_gcr_pass moves nothing"""
    cfg, seed, envs, options = REFINE_GCR_CASES[name]
    calls = draw_sequence(seed, cfg, **REFINE_GCR_OPTIONS, **options)
    assert_refine_calls(calls, cfg, True)
    assert_refine_gcr_calls(calls, cfg, options.get("cycles", False))
    assert_gcr_calls(calls, cfg, False, options.get("deep_iters", DEEP_GCR[2]))
    if options.get("cycles"):
        assert_cycle_calls(calls, cfg)
    runs = []
    for env in envs:
        set_knobs(monkeypatch, env)
        tally = run_sequence(pkg, po, cfg, calls, seed, env)
        assert tally.graphs == -1 if env == EAGER else 1 <= tally.graphs <= K_MAX_GRAPHS, tally.graphs
        runs.append(tally)
    for b, env in zip(runs[1:], envs[1:]):
        for x, y in zip(runs[0].final, b.final):
            assert np.array_equal(x, y), env
        assert len(runs[0].histories) == len(b.histories) and all(np.array_equal(x, y) for x, y in zip(runs[0].histories, b.histories)), env


# ---- 3. the cache bound and its fallback ---------------------------------------------------------------------------
def test_graph_cache_fills_to_its_bound_and_the_fallback_matches_the_model(pkg, po, monkeypatch):
    """more than eight buffer assignments on one handle: each level's parity flipped in turn by smooth(level, 1), the
    three graph users between the flips.  The cache (kMaxGraphs = 8 in csrc/mgx.hip) never shrinks, never exceeds 8,
    reaches 8; the calls after that run eagerly with the capture's bookkeeping left out and still match the model; a
    twin handle with MGX_GRAPH=0 returns the same bits, histories and fine_updates for the same calls."""
    cfg = dict(P85, mu1=2, mu2=1)
    L, Lc = 8, 5
    calls = [c for lv in range(Lc, L + 1) for c in (("set_u", lv, 300 + lv), ("set_b", lv, 400 + lv))]
    flips = [Lc, Lc + 1, Lc, Lc + 2, Lc, Lc + 1, Lc, L, Lc, Lc + 1]          # Gray code: ten more assignments
    for lv in flips:
        calls += [("smooth", lv, 1), ("solve", 0.0, 1), ("vcycle_zero",), ("solve_pcg", 0.0, 1)]
    set_knobs(monkeypatch, {"MGX_GRAPH": "0"})
    twin = pkg.Multigrid(**cfg)
    set_knobs(monkeypatch, {})
    tally = Tally()
    done = []

    def where():
        return f"cache-bound sequence, step {len(done) - 1}, calls so far {done}"

    m = hm.HandleModel(po, **cfg)
    try:
        with pkg.Multigrid(**cfg) as mg:
            assert mg.graphs_cached() == 0 and twin.graphs_cached() == -1
            for call in calls:
                done.append(call)
                out_t = apply_device(pkg, twin, call, L)
                out_g = step(pkg, mg, m, cfg, call, tally, where)
                for lv in range(Lc, L + 1):
                    for which in (pkg.VEC_U, pkg.VEC_B):
                        assert np.array_equal(twin.get_level(lv, which), mg.get_level(lv, which)), (lv, which, where())
                if call[0] in ("solve", "solve_pcg"):
                    (st_g, h_g), (st_t, h_t) = out_g, out_t
                    assert np.array_equal(h_g, h_t), (h_g, h_t, where())
                    assert (st_g.cycles, st_g.converged, st_g.fine_updates) == (st_t.cycles, st_t.converged, st_t.fine_updates), where()
                assert twin.graphs_cached() == -1
    finally:
        twin.close()
    g = tally.graph_counts
    assert all(b >= a for a, b in zip(g, g[1:])), g        # never decreases
    assert max(g) == K_MAX_GRAPHS, g                       # reaches the bound and never exceeds it
    full = g.index(K_MAX_GRAPHS)
    after = [c[0] for c in calls[full + 1:] if c[0] in GRAPH_USERS]
    assert len(after) >= 6 and set(after) == set(GRAPH_USERS), (full, after)     # the fallback really ran, all three bodies
    assert tally.executed == len(calls)
    print(f"\n[handle-state] cache bound: steps={len(calls)} graphs={g} full_at_step={full} graph_users_after={len(after)} "
          f"hist_solve={tally.hist['solve']:.3g}xbound hist_pcg={tally.hist['solve_pcg']:.3g}xbound state_dev_bottom={tally.state:.3g} state_dev_pcg={tally.state_pcg:.3g}")


# ---- 4. the other holders of the cache -----------------------------------------------------------------------------
def all_levels(pkg, mg, L, Lc):
    return [mg.get_level(lv, w) for lv in range(Lc, L + 1) for w in (pkg.VEC_U, pkg.VEC_B)]


def test_split_submission_equals_the_whole_cycle_graph_on_one_handle(pkg, po, monkeypatch):
    """cfg.profile = 2 (the finest level eager, everything below one cached graph, tags 4 / 8) through solve,
    vcycle_zero and solve_pcg with smooth(level, 1) on coarse levels between them: the bits of a profile = 0 handle.
    Histories too: both submissions end in the same post-smoothing pass with its block sums and the same reduction."""
    set_knobs(monkeypatch, {})
    cfg = dict(P85)
    L, Lc = 8, 5
    calls = [("set_rhs", 51), ("set_guess", 52), ("solve", 0.0, 2), ("smooth", 6, 1), ("vcycle_zero",), ("smooth", 5, 1),
             ("solve_pcg", 0.0, 2), ("smooth", 7, 1), ("solve", 0.0, 2), ("vcycle_zero",), ("smooth", 6, 1), ("solve_pcg", 0.0, 2),
             ("set_guess", 53), ("solve", 1e-2, 3)]
    with pkg.Multigrid(profile=0, **cfg) as whole, pkg.Multigrid(profile=2, **cfg) as split:
        for i, call in enumerate(calls):
            a, b = apply_device(pkg, whole, call, L), apply_device(pkg, split, call, L)
            for x, y in zip(all_levels(pkg, whole, L, Lc), all_levels(pkg, split, L, Lc)):
                assert np.array_equal(x, y), (i, call)
            if a is not None:
                assert np.array_equal(a[1], b[1]), (i, call, a[1], b[1])
                assert (a[0].cycles, a[0].converged, a[0].fine_updates) == (b[0].cycles, b[0].converged, b[0].fine_updates), (i, call)
        assert 1 <= whole.graphs_cached() <= K_MAX_GRAPHS and 1 <= split.graphs_cached() <= K_MAX_GRAPHS
    # launches of a capturing and of a replaying call of the same kind from the same data
    with pkg.Multigrid(profile=2, **cfg) as split:
        split.set_rhs(field(255, 51))
        seen = []
        for _ in range(4):
            split.set_guess(field(255, 52))
            g0 = split.graphs_cached()
            split.profile_reset()
            split.solve(tol=0.0, max_cycles=1)
            seen.append((split.graphs_cached() > g0, split.profile()["launches"], split.profile()["sweeps"]))
        assert seen[0][0] and not seen[-1][0], seen        # the first call captures, the last one replays
        for captured, launches, sweeps in seen[1:]:
            assert launches == seen[0][1] and sweeps == seen[0][2], seen
        assert seen[0][1][4] == 1 and seen[0][2][0] == cfg["mu1"] + cfg["mu2"], seen      # one graph launch below the finest level


@pytest.mark.parametrize("P", [2, 4])
def test_slab_handles_keep_their_coarse_cache_across_entry_points(pkg, po, monkeypatch, P):
    """n_gpus = 2 and 4 with every slab on device 0, default cut: solve, vcycle, fmg, set_guess, solve on one handle give
    the single-GPU handle's bits (finest U and B: what a slab handle lets one read); histories to rtol 1e-13 (the slabs'
    partial sums, tests/test_gpu_dist.py); graphs_cached() reports the replicated coarse solver's cache"""
    set_knobs(monkeypatch, {})
    cfg = dict(P85, mu1=2, mu2=1)
    L = 8
    calls = [("set_rhs", 61), ("set_guess", 62), ("solve", 0.0, 2), ("vcycle", L), ("fmg",), ("set_guess", 63), ("solve", 1e-3, 4),
             ("vcycle", L), ("set_guess", 62), ("solve", 0.0, 2)]
    with pkg.Multigrid(**cfg) as one, pkg.Multigrid(n_gpus=P, devices=[0] * P, cut_level=0, **cfg) as many:
        counts = [many.graphs_cached()]
        first, last = None, None
        for i, call in enumerate(calls):
            a, b = apply_device(pkg, one, call, L), apply_device(pkg, many, call, L)
            for w in (pkg.VEC_U, pkg.VEC_B):
                assert np.array_equal(one.get_level(L, w), many.get_level(L, w)), (i, call, w)
            if a is not None:
                assert len(a[1]) == len(b[1]) and np.allclose(a[1], b[1], rtol=1e-13, atol=0), (i, call, a[1], b[1])
                assert (a[0].cycles, a[0].converged, a[0].fine_updates) == (b[0].cycles, b[0].converged, b[0].fine_updates), (i, call)
                first, last = (first or a), a
            counts.append(many.graphs_cached())
        assert np.array_equal(first[1], last[1])           # the same call from the same data, eight calls later
    assert counts[0] == 0 and counts[3] >= 1, counts       # the coarse cycle is captured by the first solve
    assert all(b >= a for a, b in zip(counts, counts[1:])) and max(counts) <= K_MAX_GRAPHS, counts


@pytest.mark.parametrize("schedule", [hm.V, hm.FMG])
def test_mixed_handle_is_unaffected_by_calls_on_its_coarse_levels(pkg, po, monkeypatch, schedule):
    """dtype MIXED: solve, smooth / vcycle on the float levels below the finest, set_guess, solve - the histories and
    solutions of fresh handles given the same finest-level data; no graphs (graphs_cached() == -1) throughout"""
    set_knobs(monkeypatch, {})
    cfg = dict(P85, mu1=2, mu2=1, dtype=hm.MIXED, schedule=schedule)
    L = 8
    b, u0, u1 = field(255, 71), field(255, 72), field(255, 73)
    with pkg.Multigrid(**cfg) as mg:
        seen = [mg.graphs_cached()]
        mg.set_rhs(b)
        mg.set_guess(u0)
        s1, h1 = mg.solve(tol=1e-6, max_cycles=6)
        x1 = mg.get_solution()
        seen.append(mg.graphs_cached())
        for lv, mu in ((7, 1), (6, 3), (5, 1), (7, 2)):
            mg.set_level(lv, pkg.VEC_U, field(mg.n(lv), 80 + lv))
            mg.smooth(lv, mu)
            mg.vcycle(lv)
            seen.append(mg.graphs_cached())
        mg.set_guess(u1)
        s2, h2 = mg.solve(tol=1e-6, max_cycles=6)
        x2 = mg.get_solution()
        mg.set_guess(u0)
        s3, h3 = mg.solve(tol=1e-6, max_cycles=6)
        x3 = mg.get_solution()
        seen.append(mg.graphs_cached())
    assert set(seen) == {-1}, seen
    for u, (s, h, x) in ((u0, (s1, h1, x1)), (u1, (s2, h2, x2)), (u0, (s3, h3, x3))):
        with pkg.Multigrid(**cfg) as fresh:
            fresh.set_rhs(b)
            fresh.set_guess(u)
            sf, hf = fresh.solve(tol=1e-6, max_cycles=6)
            assert np.array_equal(hf, h) and np.array_equal(fresh.get_solution(), x)
            assert (sf.cycles, sf.converged, sf.fine_updates) == (s.cycles, s.converged, s.fine_updates)
            assert fresh.graphs_cached() == -1
