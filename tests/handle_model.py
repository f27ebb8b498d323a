"""CPU model of ONE long-lived mgx handle: U and B of every level as numpy arrays, and every entry point of include/mgx.h
that reads or writes them as its oracle statement.  The single operators come from oracle/pyoracle.py (POISSON) and the
reference hierarchies of tests/galerkin_ref.py, tests/opdep_ref.py and tests/cheby_ref.py (STENCIL5, GALERKIN); the
schedules are COMPOSED from the model's own single operators, so that the coarse levels hold after a schedule what the
documented sequence of operators leaves there; the conjugate-gradient solve is tests/pcg_ref.py's iteration with the
model's zero-start cycle as preconditioner.  tests/test_handle_model.py holds the compositions to the references'
own vcycle / fmg / solve bit for bit; tests/test_gpu_handle_state.py drives a device handle and this model with the
same calls.

Every operator rounds as the device kernels do (the references are written operation by operation), so the state of
the model is meant bit for bit, with two exceptions that are the existing suite's: norms (another summation order) and
the exact bottom solve of the POISSON hierarchy (sine transform: tests/test_gpu_operators.py holds it to 1e-11 / two
float ulps; the model uses the oracle's sine-transform mode, the device's method in the device's order).

fine_updates follows include/mgx.h: finest-level smoother point updates (mu n^2 per block of mu sweeps or of degree
mu, 2 mu n^2 per block of alternating line sweeps), counted from the start of the last solve / solve_pcg / solve_gcr.

The cycle index (mgx_set_cycle) is an attribute the composed vcycle() reads: the recursion of include/mgx.h from the
same single operators, held to tests/wcycle_ref.py bit for bit.  The zebra line smoothers (cfg.smoother 4 / 5 / 6) run
through tests/line_ref.py; the device joins a line's carries in another order, so calls that smooth are compared to a
bound there (tests/test_gpu_handle_state.py), for which the model can be instantiated a second time in np.longdouble
(real=np.longdouble: line_ref.NumpyOps in place of the oracle, the operators cast from the working type).

The multicolour Gauss-Seidel smoothers (cfg.smoother 8 / 9) run through tests/colour_ref.py, bit for bit.  They are the one
smoother whose result depends on the block's position: smooth(level, mu, post) hands `post` to the hierarchy, and the
composed vcycle() sets it where the device does - the block after a correction and the last mu2 sweeps of a
bottom = SMOOTH visit; mgx_smooth itself is always forward.

A GALERKIN handle takes a nine-point finest operator (set_stencil9, set_tensor): the hierarchies of tests/nine_ref.py
(Jacobi, Chebyshev) and colour_ref's Nine* classes; a later set_stencil or set_coefficient makes the level five-point
again.  The line smoothers on a nine-point finest level are not modelled (their tolerance rule is measured for
five-point finest operators only): set_stencil9 / set_tensor refuse there with a ValueError.

solve_refine (mgx_solve_refine) is tests/refine_ref.py's loop around the model's own fp64 residual and the zero-start
cycle of a PRIVATE SECOND MODEL of dtype F32 with the same configuration and cycle index: the statement of
include/mgx.h, "bit for bit what a public F32 handle holds after mgx_set_stencil / mgx_set_stencil9 (and
mgx_build_galerkin_transfer) with the float32 of the handle's coefficients".  The float model is rebuilt by the next
solve_refine after the operator, the hierarchy or the transfer has changed; set_cycle reaches it at once.  Only U of the
finest level moves: the cycle runs on the float model's levels, the model's own coarse levels stay as they were.

solve_refine_gcr (mgx_solve_refine_gcr) is tests/refine_gcr_ref.py's loop around the model's fp64 finest operator and the
cycle of THE SAME float model: a solve_refine and a solve_refine_gcr share it, either one rebuilds it.  The loop's residual
lives in vectors of its own, so B stays the caller's and the coarse levels stay untouched, as for solve_refine; U of the
finest level is x, also after a breakdown.  time_refine_gcr_pass moves nothing and refuses where the device's guard does:
until a float model (solve_refine or solve_refine_gcr) AND a GCR basis (solve_gcr or solve_refine_gcr) exist.

set_reaction / get_reaction (mgx_set_reaction, mgx_get_reaction; GALERKIN handles) keep the base centre c0 and the term d beside
the finest operator, whose slot 0 is tests/theta_ref.py's shift: c0 + d, one rounding in the working type.  A second call
replaces the term; None with a term set restores c0 bit for bit, None with none set changes nothing - the hierarchy stays
valid; set_stencil, set_stencil9, set_coefficient and set_tensor drop the term, so a later None brings no old centre back.
Every call that changes the operator leaves the hierarchy invalid until build_galerkin, as set_stencil does.  The float model
of solve_refine is handed the float32 of the STORED centre - c0 + d rounded in double, then to float - because it copies
slot 0 as it stands.  Refused where the device returns MGX_ERR_STATE (RuntimeError): POISSON, STENCIL5, operator not set,
get_reaction with no term.  The line smoothers are not modelled here (ValueError).

theta_steps (mgx_theta_steps) forms theta_ref.rhs_pass from the model's own S u (minus its residual against a zero right-hand
side) into B of the finest level and runs the model's solve, solve_gcr or solve_refine_gcr from the current U, step by step:
per-step statistics and histories and steps_done; a step with converged = 0 ends the call after that step, nsteps = 0 moves
nothing.  time_theta_rhs moves nothing and is refused while no term is set.

newton and newton_steps (mgx_newton, mgx_newton_steps) run the loops of tests/newton_ref.py and tests/newton_steps_ref.py with
A0 = base_operator() - a caller's term is no part of F - around the model's own linear solve: set_reaction(d), build_galerkin
with the transfer in use, set_rhs(b), a zero U and the chosen solver; the norm is the model's residual norm of (B = b,
U = 0).  On return U is the last accepted iterate and B the caller's f (newton) or the last step's r (newton_steps); the
operator is A0 + diag(d_k) of the last linear solve with its hierarchy built, and the coarse levels hold what that solve
left.  When no iteration runs (max_newton = 0, nsteps = 0, or the first norm passes the tolerance) operator, hierarchy and
every level stay as they were (newton_steps with steps but no iteration leaves r in B).  A failed line search: failed,
converged = 0, U the last accepted iterate.  norms and lin keep every norm and every linear solve's record of the last call:
tests/test_handle_model_newton.py replays the Armijo and stop decisions from them.  time_newton_pass and time_newton_step_pass
move nothing and are refused until a newton (any newton_steps with nsteps > 0) or a newton_steps call has allocated their
workspace, as the guards of csrc/mgx.hip read."""
import numpy as np

import cheby_ref
import colour_ref as cf
import galerkin_ref as gr
import gcr_ref
import line_ref as lr
import newton_ref as nf
import newton_steps_ref as nsr
import nine_ref as nr
import opdep_ref as od
import pcg_ref
import refine_gcr_ref
import refine_ref
import theta_ref as tr

JACOBI, RBGS, CHEBYSHEV = 0, 1, 2
LINE_X, LINE_Y, LINE_ALT = lr.LINE_X, lr.LINE_Y, lr.LINE_ALT
LINES = (LINE_X, LINE_Y, LINE_ALT)
COLOR_GS, COLOR_SGS = cf.COLOR_GS, cf.COLOR_SGS   # 8, 9
COLOURS = (COLOR_GS, COLOR_SGS)
CYCLE_V, CYCLE_W, CYCLE_F = 0, 1, 2            # mgx_set_cycle
F32, F64, MIXED = 0, 1, 2
V, FMG = 0, 1
CONSISTENT, FW16 = 0, 1
EXACT, SMOOTH = 0, 1
SEPARATE, FMA = 0, 1
POISSON, STENCIL5, GALERKIN = 0, 1, 3
BILINEAR, OPERATOR = 0, 1
STEP_SOLVE, STEP_GCR, STEP_REFINE_GCR = 0, 1, 2    # the solver of mgx_theta_steps / mgx_newton / mgx_newton_steps

DEFAULTS = dict(finest_level=10, coarsest_level=7, mu0=30, mu1=10, mu2=10, omega=2.0 / 3.0, smoother=JACOBI, dtype=F64,
                schedule=FMG, restrict_mode=CONSISTENT, bottom=EXACT, arith=SEPARATE, op=POISSON)      # mgx_config_default


class PoissonOps:
    """the constant five-point stencil: the oracle's kernels behind the interface of galerkin_ref.Hierarchy"""

    def __init__(self, po, finest, coarsest, dtype, mode, omega, smoother, arith):
        self.po, self.L, self.Lc, self.dt, self.mode, self.omega = po, finest, coarsest, dtype, mode, omega
        self.smoother, self.arith = smoother, arith
        self._bottom = None

    def smooth(self, lv, v, b, mu):
        if mu == 0:
            return v
        if self.smoother == RBGS:
            return self.po.rbgs(v, b, mu)
        return self.po.jacobi(v, b, mu, self.omega, self.arith)

    def residual(self, lv, v, b):
        return self.po.residual(v, b)

    def bottom(self, b):
        if self._bottom is None:               # the sine-transform solve in the device's operation order
            self._bottom = self.po.Solver(finest_level=self.Lc, coarsest_level=self.Lc, bottom=self.po.BOTTOM_DST,
                                          dtype=F64 if self.dt == np.float64 else F32)
        return self._bottom.bottom_solve(np.ascontiguousarray(b, dtype=self.dt))


class _OracleBottom:
    """bottom() of a STENCIL5 hierarchy through the oracle's own dense solve (orc_dense_inverse: the elimination
    galerkin_ref.gauss_jordan_inverse states, tests/test_gpu_var.py holds the device to it bit for bit), which takes
    a fraction of a second where the numpy statement takes several.  Mixed in BEFORE the reference class, whose
    attributes po, Lc, dt, omega, st and _inv (cheby_ref.Stencil5.__init__) it reads: a change there has to be followed
    here; tests/test_handle_model.py holds this bottom() to the reference's own, bit for bit"""

    def bottom(self, b):
        if self._inv is None:
            s = self.po.Solver(finest_level=self.Lc, coarsest_level=self.Lc, op=self.po.OP_STENCIL5,
                               dtype=F64 if self.dt == np.float64 else F32, omega=self.omega)
            s.set_stencil(self.Lc, *[np.asarray(x, dtype=np.float64) for x in self.st[self.Lc][:5]])
            self._inv = s
        return self._inv.bottom_solve(np.ascontiguousarray(b, dtype=self.dt))


class Stencil5(_OracleBottom, cheby_ref.Stencil5):
    pass


class Stencil5Cheby(_OracleBottom, cheby_ref.Stencil5Cheby):
    pass


class Stencil5Colour(_OracleBottom, cf.Stencil5):
    """H(smoother, po, stencils, finest, coarsest, ...)"""


_INVERSES = {}         # dense inverse of a coarsest nine-point operator, by its bytes: rebuilds and configurations share it


def _shared_inverse(h):
    """galerkin_ref.Hierarchy.bottom builds its inverse on first use (seconds at level 5): the same operator - a
    BILINEAR rebuild after an OPERATOR one, the Chebyshev twin of a Jacobi configuration - takes it from here"""
    if h._inv is None:
        M = gr.dense(h.st[h.Lc])
        key = M.tobytes()
        if key not in _INVERSES:
            _INVERSES[key] = gr.gauss_jordan_inverse(M)
        h._inv = _INVERSES[key]


def operator5(po, level, kind, dt):
    """the five-point operators of tests/test_line_cpu.py by name (imported late: that module needs scipy)"""
    from test_line_cpu import operator5 as op5
    return op5(po, level, kind, dt)


TENSORS = {"rot45": lambda level: nr.rotated_tensor(level, 45.0, 0.5), "smooth9": nr.smooth_tensor, "jump9": nr.jump_tensor}
RANDOM9_SEED = 900                             # "random9": nr.random_stencil9(level, RANDOM9_SEED + level)
OPERATORS9 = tuple(TENSORS) + ("random9",)


def tensor_nodes(level, kind):
    """nodal (axx, axy, ayy) of a tensor kind: what mgx_set_tensor is handed"""
    return tuple(np.ascontiguousarray(np.broadcast_to(a, ((1 << level) + 1,) * 2), dtype=np.float64) for a in TENSORS[kind](level))


def operator9(level, kind, dt):
    """the nine-point finest operators by name, beside operator5: three symmetric ones, discretised from a nodal tensor
    (rot45: the constant anisotropy 1 : 0.5 at 45 degrees; smooth9; jump9), and random9, which is unsymmetric and holds
    values in the places that point at the Dirichlet ring"""
    if kind == "random9":
        return nr.random_stencil9(level, RANDOM9_SEED + level, dt)
    return nr.tensor9(*tensor_nodes(level, kind), dtype=dt)


class HandleModel:
    def __init__(self, po, real=None, **cfg):
        """real: the type the model computes in, when it is not the handle's own (np.longdouble: the 'exact' side of a
        line-smoother comparison; line smoothers only - every other smoother runs through the oracle's C kernels)"""
        unknown = set(cfg) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown configuration fields {sorted(unknown)}")
        c = dict(DEFAULTS, **cfg)
        self.cfg = c
        self.L, self.Lc = c["finest_level"], c["coarsest_level"]
        if c["dtype"] == MIXED:
            raise ValueError("dtype MIXED keeps two finest levels: not modelled")
        self.wdt = np.float64 if c["dtype"] == F64 else np.float32       # the handle's working type
        self.dt = self.wdt if real is None else real
        self.line = c["smoother"] in LINES
        self.colour = c["smoother"] in COLOURS
        if self.colour and c["op"] == POISSON:
            raise ValueError("colour smoothers: STENCIL5 and GALERKIN handles only")
        if self.dt is not self.wdt:
            if not self.line:
                raise ValueError("real= is for the line smoothers: the other smoothers are the oracle's kernels")
        self.oracle = po                       # builds the operators, always in the working type
        self.po = po if self.dt is self.wdt else lr.NumpyOps      # the arithmetic of the transfers, the residual and the norm
        if self.line and c["op"] == POISSON:
            raise ValueError("line smoothers: STENCIL5 and GALERKIN handles only")
        self.op = c["op"]
        self.cycle = CYCLE_V
        self.U = {lv: np.zeros((self.n(lv),) * 2, dtype=self.dt) for lv in self.levels()}
        self.B = {lv: np.zeros((self.n(lv),) * 2, dtype=self.dt) for lv in self.levels()}
        self.R = {}
        self.fine_updates = 0.0
        self.st5 = None                        # GALERKIN: the finest operator, waiting for build_galerkin: five arrays,
        self.st9 = None                        # ... or nine (set_stencil9 / set_tensor); the later call decides
        self.stencils = None                   # STENCIL5: every level's operator
        self.transfer = None
        self.h = None
        self.f32 = None                        # solve_refine: the float model, created by the first call ...
        self.f32_of = None                     # ... and the hierarchy (self.h at the time) whose float copy it holds
        self.basis = False                     # slot 0 of the GCR basis exists: after a solve_gcr or a solve_refine_gcr
        self.c0 = None                         # set_reaction: the base centre (slot 0 of A0) while a term is set ...
        self.d = None                          # ... and the term; None: no term is set (the device's rx.set is lowered)
        self.nwt = False                       # mgx_newton's workspace exists: after a newton or a newton_steps with nsteps > 0
        self.nwt_mass = False                  # ... and its mass grid: after a newton_steps with nsteps > 0
        self.norms = []                        # every norm of the last newton / newton_steps call, in the order formed ...
        self.lin = []                          # ... and (stats, history) of every linear solve it ran
        if self.op == POISSON:
            self.h = PoissonOps(self.po, self.L, self.Lc, self.dt, c["restrict_mode"], c["omega"], c["smoother"], c["arith"])

    # -- plumbing ----------------------------------------------------------------------------------------------
    def n(self, level):
        return (1 << level) - 1

    def levels(self):
        return range(self.Lc, self.L + 1)

    def _ops(self):
        if self.h is None:
            raise RuntimeError("operators not set (set_coefficient / build_galerkin): the device returns MGX_ERR_STATE")
        return self.h

    def _hier_args(self):
        c = self.cfg
        return dict(dtype=self.dt, mode=c["restrict_mode"], omega=c["omega"], mu1=c["mu1"], mu2=c["mu2"], mu0=c["mu0"],
                    bottom=c["bottom"])

    # -- data in and out ---------------------------------------------------------------------------------------
    def set_level(self, level, which, a):
        (self.U if which == 0 else self.B)[level] = np.array(a, dtype=self.dt, order="C").reshape((self.n(level),) * 2)

    def get_level(self, level, which):
        return (self.U if which == 0 else self.B)[level]

    def set_rhs(self, b):
        self.set_level(self.L, 1, b)

    def set_guess(self, u):
        self.set_level(self.L, 0, u)

    def zero_level(self, level, which):
        self.set_level(level, which, np.zeros((self.n(level),) * 2))

    # -- operator changes --------------------------------------------------------------------------------------
    def _w(self, st5):
        return [np.asarray(x, dtype=self.wdt) for x in st5]

    def _stencil5_hierarchy(self):
        """STENCIL5: the hierarchy of self.stencils with the configuration's smoother"""
        c = self.cfg
        if self.line:
            self.h = lr.Stencil5(c["smoother"], self.po, self.stencils, self.L, self.Lc, **self._hier_args())
            if c["bottom"] == EXACT:
                _shared_inverse(self.h)
        elif self.colour:
            self.h = Stencil5Colour(c["smoother"], self.po, self.stencils, self.L, self.Lc, **self._hier_args())
        else:
            cls = Stencil5Cheby if c["smoother"] == CHEBYSHEV else Stencil5
            self.h = cls(self.po, self.stencils, self.L, self.Lc, **self._hier_args())

    def set_coefficient(self, a_nodes):
        """STENCIL5: every level re-discretised from the nodal coefficient.  GALERKIN: the finest level only, and the
        hierarchy is invalid until build_galerkin"""
        a = np.ascontiguousarray(a_nodes, dtype=np.float64)
        if self.op == STENCIL5:
            self.stencils = {lv: self._w(self.oracle.stencil_from_nodes(a, lv, self.L)) for lv in self.levels()}
            self._stencil5_hierarchy()
        elif self.op == GALERKIN:
            self.st5, self.st9 = self._w(self.oracle.stencil_from_nodes(a, self.L, self.L)), None
            self.h = None
            self.transfer = None
            self.c0 = self.d = None             # the term is gone with the centre it was added to
        else:
            raise RuntimeError("op = POISSON: MGX_ERR_STATE")

    def set_stencil(self, level, st5):
        """mgx_set_stencil: STENCIL5 any level (the hierarchy stands once every level has one), GALERKIN the finest only"""
        if self.op == STENCIL5:
            self.stencils = dict(self.stencils or {})
            self.stencils[level] = self._w(st5)
            self.h = None
            if all(lv in self.stencils for lv in self.levels()):
                self._stencil5_hierarchy()
        elif self.op == GALERKIN and level == self.L:
            self.st5, self.st9 = self._w(st5), None
            self.h = None
            self.transfer = None
            self.c0 = self.d = None
        else:
            raise RuntimeError("MGX_ERR_STATE")

    def _nine_finest(self, level, st9):
        if self.op != GALERKIN or level != self.L:
            raise RuntimeError("nine-point operators: the finest level of a GALERKIN handle only: MGX_ERR_STATE")
        if self.line:
            raise ValueError("line smoothers on a nine-point finest level are out of scope: THE TOLERANCE RULE of "
                             "tests/test_line_cpu.py is measured for five-point finest operators")
        assert len(st9) == 9
        self.st5, self.st9 = None, self._w(st9)
        self.h = None
        self.transfer = None
        self.c0 = self.d = None

    def set_stencil9(self, level, st9):
        """mgx_set_stencil9: the finest level of a GALERKIN handle becomes nine-point; invalid until build_galerkin"""
        self._nine_finest(level, st9)

    def set_tensor(self, axx, axy, ayy):
        """mgx_set_tensor: the nine-point discretisation of the nodal tensor (nine_ref.tensor9: double arithmetic, every
        coefficient rounded to the working type once)"""
        self._nine_finest(self.L, nr.tensor9(axx, axy, ayy, dtype=self.wdt))

    def set_operator(self, kind):
        """a named operator of tests/test_line_cpu.py (operator5) or a nine-point one (operator9).  STENCIL5: set_stencil
        on every level.  GALERKIN: set_stencil on the finest level - a tensor kind: set_tensor, random9: set_stencil9 -
        then build_galerkin with the transfer in use (BILINEAR at first)"""
        if kind in OPERATORS9:
            transfer = BILINEAR if self.transfer is None else self.transfer
            if kind in TENSORS:
                self.set_tensor(*tensor_nodes(self.L, kind))
            else:
                self.set_stencil9(self.L, operator9(self.L, kind, self.wdt))
            self.build_galerkin(transfer)
        elif self.op == STENCIL5:
            for lv in self.levels():
                self.set_stencil(lv, operator5(self.oracle, lv, kind, self.wdt))
        elif self.op == GALERKIN:
            transfer = BILINEAR if self.transfer is None else self.transfer
            self.set_stencil(self.L, operator5(self.oracle, self.L, kind, self.wdt))
            self.build_galerkin(transfer)
        else:
            raise RuntimeError("op = POISSON: MGX_ERR_STATE")

    def build_galerkin(self, transfer=BILINEAR):
        if self.op != GALERKIN or (self.st5 is None and self.st9 is None):
            raise RuntimeError("MGX_ERR_STATE")
        cheb = self.cfg["smoother"] == CHEBYSHEV
        opdep = transfer == OPERATOR
        if self.st9 is not None:                # a nine-point finest level: every level through the nine-point routines
            if self.colour:
                self.h = (cf.NineOpdepHierarchy if opdep else cf.NineHierarchy)(self.cfg["smoother"], self.po, self.st9, self.L, self.Lc, **self._hier_args())
            else:
                if opdep:
                    cls = nr.ChebyOpdepHierarchy if cheb else nr.OpdepHierarchy
                else:
                    cls = nr.ChebyHierarchy if cheb else nr.Hierarchy
                self.h = cls(self.po, self.st9, self.L, self.Lc, **self._hier_args())
        elif self.colour:
            self.h = (cf.OpdepHierarchy if opdep else cf.Hierarchy)(self.cfg["smoother"], self.po, self.st5, self.L, self.Lc, **self._hier_args())
        elif self.line:
            cls = lr.OpdepHierarchy if transfer == OPERATOR else lr.Hierarchy
            self.h = cls(self.cfg["smoother"], self.po, self.st5, self.L, self.Lc, **self._hier_args())
        else:
            if transfer == OPERATOR:
                cls = cheby_ref.OpdepHierarchy if cheb else od.Hierarchy
            else:
                cls = cheby_ref.Hierarchy if cheb else gr.Hierarchy
            self.h = cls(self.po, self.st5, self.L, self.Lc, **self._hier_args())
        self.transfer = transfer
        if self.cfg["bottom"] == EXACT:
            _shared_inverse(self.h)

    def set_cycle(self, kind):
        """mgx_set_cycle: the kind of every cycle from here on; it survives build_galerkin and set_coefficient"""
        if self.op == POISSON:
            raise RuntimeError("op = POISSON handles run V-cycles only: MGX_ERR_STATE")
        if kind not in (CYCLE_V, CYCLE_W, CYCLE_F):
            raise ValueError("MGX_ERR_INVALID")
        self.cycle = kind
        if self.f32 is not None:
            self.f32.cycle = kind

    # -- transfers of the current hierarchy --------------------------------------------------------------------
    def _R(self, level, r):
        h = self._ops()
        if self.transfer == OPERATOR:
            return h.restrict(level, r)
        return self.po.restrict(r, self.cfg["restrict_mode"])

    def _P(self, level, e):
        h = self._ops()
        if self.transfer == OPERATOR:
            return h.prolong(level, e)
        return self.po.prolong(e)

    # -- single operators --------------------------------------------------------------------------------------
    def smooth(self, level, mu, post=False):
        """mu Jacobi, red-black Gauss-Seidel, zebra line or colour sweeps, or one Chebyshev block of degree mu.  post: the
        block follows a correction, or is the second one of a bottom = SMOOTH visit (COLOR_SGS sweeps it in reverse colour
        order; no other smoother looks at it).  mgx_smooth is post = False"""
        if self.colour:
            self.U[level] = self._ops().smooth(level, self.U[level], self.B[level], mu, post)
        else:
            self.U[level] = self._ops().smooth(level, self.U[level], self.B[level], mu)
        if level == self.L:
            per_sweep = 2 if self.cfg["smoother"] == LINE_ALT else 1       # an alternating sweep is an x- and a y-sweep
            self.fine_updates += float(per_sweep * mu) * float(self.n(level)) * float(self.n(level))

    def residual(self, level):
        self.R[level] = self._ops().residual(level, self.U[level], self.B[level])
        return self.R[level]

    def residual_norm(self, level=None):
        level = self.L if level is None else level
        return self.po.norm2(self._ops().residual(level, self.U[level], self.B[level]))

    def restrict(self, level):
        """B[l-1] = R (B[l] - A U[l]),  U[l-1] = 0"""
        self.B[level - 1] = self._R(level, self._ops().residual(level, self.U[level], self.B[level]))
        self.U[level - 1] = np.zeros_like(self.B[level - 1])

    def restrict_rhs(self, level):
        self.B[level - 1] = self._R(level, self.B[level])

    def prolong(self, level):
        self.U[level] = self._P(level, self.U[level - 1])

    def prolong_add(self, level):
        if self.transfer == OPERATOR:
            self.U[level] = self.U[level] + self._P(level, self.U[level - 1])
        else:
            self._ops()
            self.U[level] = self.po.prolong_add(self.U[level], self.U[level - 1])

    def bottom_solve(self):
        if self.cfg["bottom"] != EXACT:
            raise RuntimeError("bottom = SMOOTH: MGX_ERR_STATE")
        self.U[self.Lc] = self._ops().bottom(self.B[self.Lc])

    # -- schedules, composed from the operators above ----------------------------------------------------------
    def vcycle(self, level=None, kind=None):
        """one cycle of the handle's kind (include/mgx.h, mgx_set_cycle): pre-smooth, restrict; visit level - 1; W and
        F: if level - 1 is above the coarsest, visit it again (W: a W-cycle, F: a V-cycle) from the U the first visit
        left, with the same B; correct, post-smooth.  The coarsest level is visited once per descent"""
        level = self.L if level is None else level
        kind = self.cycle if kind is None else kind
        c = self.cfg
        if level == self.Lc:
            if c["bottom"] == EXACT:
                self.bottom_solve()
            else:
                self.smooth(level, c["mu1"])
                self.smooth(level, c["mu2"], post=True)
            return
        self.smooth(level, c["mu1"])
        self.restrict(level)
        self.vcycle(level - 1, kind)
        if kind != CYCLE_V and level - 1 > self.Lc:
            self.vcycle(level - 1, CYCLE_V if kind == CYCLE_F else kind)
        self.prolong_add(level)
        self.smooth(level, c["mu2"], post=True)

    def vcycle_zero(self):
        self.zero_level(self.L, 0)
        self.vcycle(self.L)

    def fmg(self):
        c = self.cfg
        for lv in range(self.L, self.Lc, -1):
            self.restrict_rhs(lv)
        if c["bottom"] == EXACT:
            self.bottom_solve()
        else:
            self.zero_level(self.Lc, 0)
            for _ in range(c["mu0"] + 1):
                self.vcycle(self.Lc)
        for lv in range(self.Lc + 1, self.L + 1):
            self.prolong(lv)
            for _ in range(c["mu0"] + 1):
                self.vcycle(lv)

    # -- solves ------------------------------------------------------------------------------------------------
    def solve(self, tol=1e-8, max_cycles=50):
        """(stats, history): cycles until ||r|| <= tol ||r0|| or max_cycles; schedule = FMG: the first cycle is fmg()"""
        self.fine_updates = 0.0
        hist = [self.residual_norm()]
        k = 0
        while k < max_cycles and not hist[k] <= tol * hist[0]:
            if k == 0 and self.cfg["schedule"] == FMG:
                self.fmg()
            else:
                self.vcycle(self.L)
            hist.append(self.residual_norm())
            k += 1
        return dict(cycles=k, converged=int(hist[-1] <= tol * hist[0]), fine_updates=self.fine_updates), np.array(hist)

    def finest_operator(self):
        """A of the finest level as pcg_ref.Operator applies it"""
        if self.op == POISSON:
            return pcg_ref.Operator(None, self.dt)
        if self.st9 is not None:
            return nr.Operator9(self._ops().st[self.L], self.dt)
        return pcg_ref.Operator(self._ops().st[self.L][:5], self.dt)

    def solve_pcg(self, tol=1e-8, max_iters=100):
        """pcg_ref.pcg with this handle's zero-start cycle as M: r lives in B[finest] while a cycle runs, so the coarse
        levels keep what the LAST cycle left; U[finest] = x and B[finest] = b afterwards"""
        self.fine_updates = 0.0
        b = self.B[self.L]

        def M(r):
            self.B[self.L] = np.ascontiguousarray(r, dtype=self.dt)
            self.vcycle_zero()
            return self.U[self.L]

        x, hist, conv, brk = pcg_ref.pcg(self.finest_operator(), M, b, self.U[self.L], tol=tol, max_iters=max_iters)
        self.U[self.L] = np.ascontiguousarray(x, dtype=self.dt)
        self.B[self.L] = b
        return dict(cycles=len(hist) - 1, converged=int(conv and not brk), fine_updates=self.fine_updates), hist

    def solve_gcr(self, tol=1e-8, max_iters=100, restart=4, dot=pcg_ref.dot):
        """gcr_ref.gcr with this handle's zero-start cycle as M, as solve_pcg: r lives in B[finest] while a cycle runs, so
        the coarse levels keep what the LAST cycle left; U[finest] = x and B[finest] = b afterwards, also after a
        breakdown.  dot: the inner product handed to gcr_ref.gcr (the tests measure what another rounding of the scalars
        is worth)"""
        self.fine_updates = 0.0
        b = self.B[self.L]

        def M(r):
            self.B[self.L] = np.ascontiguousarray(r, dtype=self.dt)
            self.vcycle_zero()
            return self.U[self.L]

        self.basis = True
        x, hist, conv, brk = gcr_ref.gcr(self.finest_operator(), M, b, self.U[self.L], tol=tol, max_iters=max_iters, restart=restart, dot=dot)
        self.U[self.L] = np.ascontiguousarray(x, dtype=self.dt)
        self.B[self.L] = b
        return dict(cycles=len(hist) - 1, converged=int(conv and not brk), fine_updates=self.fine_updates), hist

    # -- mgx_solve_refine --------------------------------------------------------------------------------------
    def _refine_guard(self):
        """the handles include/mgx.h refuses (the device: MGX_ERR_STATE), and the line smoothers, which this model leaves
        out: a device handle with a line smoother is held to a tolerance rule between the model in the working type and
        in np.longdouble, not bit for bit, so a refine call there needs a long-double twin of the FLOAT model as well"""
        if self.op == POISSON:
            raise ValueError("mgx_solve_refine: op = POISSON handles refine with dtype MIXED")
        if self.line:
            raise ValueError("solve_refine under a line smoother is not modelled (it needs a long-double float twin)")
        if self.cfg["dtype"] != F64:
            raise ValueError("mgx_solve_refine: dtype F64 handles only")
        if self.h is None:
            raise ValueError("mgx_solve_refine: operators not set / hierarchy not built")

    def _float_model(self):
        """the float copy of the hierarchy as include/mgx.h states it: an F32 model of the same configuration and cycle
        index, given the float32 of the five coefficient arrays of every level (STENCIL5), or of the finest level's five or
        nine arrays and then built in float with the transfer in use (GALERKIN)"""
        if self.f32 is not None and self.f32_of is self.h:
            return self.f32
        f = HandleModel(self.oracle, **dict(self.cfg, dtype=F32))
        f.cycle = self.cycle
        if self.op == STENCIL5:
            for lv in self.levels():
                f.set_stencil(lv, [np.asarray(x, dtype=np.float32) for x in self.stencils[lv][:5]])
        else:
            if self.st9 is not None:
                f.set_stencil9(self.L, [np.asarray(x, dtype=np.float32) for x in self.st9])
            else:
                f.set_stencil(self.L, [np.asarray(x, dtype=np.float32) for x in self.st5[:5]])
            f.build_galerkin(self.transfer)
        self.f32, self.f32_of = f, self.h
        return f

    def solve_refine(self, tol=1e-8, max_cycles=50, history=None):
        """(stats, history): refine_ref.refine with the model's fp64 finest-level residual and the zero-start cycle of the
        float model; fine_updates are the float cycle's.  U[finest] is the iterate afterwards, B and every other level are
        untouched; max_cycles = 0: one history entry, U untouched.  history: the history a device returned for this
        call - the scales s_k are then derived from IT (the norm is the only place where the device's order of summation
        reaches the iterate); the stop decision and the history returned stay the model's own.
        Not modelled: the line smoothers (ValueError, see _refine_guard)"""
        self._refine_guard()
        f = self._float_model()
        f.fine_updates = 0.0
        h, L = self.h, self.L

        def cycle32(r32):
            f.set_rhs(r32)
            f.vcycle_zero()
            return f.U[L]

        u, hist = refine_ref.refine(lambda v, b: h.residual(L, v, b), cycle32, self.B[L], self.U[L], tol=tol, max_cycles=max_cycles,
                                    norm=self.po.norm2, scales=history)
        self.U[L] = np.ascontiguousarray(u, dtype=self.dt)
        self.fine_updates = f.fine_updates
        return dict(cycles=len(hist) - 1, converged=int(hist[-1] <= tol * hist[0]), fine_updates=self.fine_updates), hist

    def time_refine_pass(self, repeats):
        """mgx_time_refine_pass: nothing moves.  Refused where solve_refine is, and until a solve_refine has created the
        float model (the device: MGX_ERR_STATE)"""
        self._refine_guard()
        if repeats < 1:
            raise ValueError("MGX_ERR_INVALID")
        if self.f32 is None:
            raise ValueError("mgx_time_refine_pass: call mgx_solve_refine first")

    # -- mgx_solve_refine_gcr ----------------------------------------------------------------------------------
    def solve_refine_gcr(self, tol=1e-8, max_iters=100, restart=4, history=None, dot=pcg_ref.dot):
        """(stats, history): refine_gcr_ref.refine_gcr with the model's fp64 finest operator as A and the zero-start cycle of
        the float model (solve_refine's: _float_model) as the cycle; fine_updates are the float cycle's.  U[finest] is x
        afterwards, also after a breakdown (converged = 0, the history stops at the entry before it); B and every other
        level are untouched; max_iters = 0: one history entry, U untouched.  history: the history a device returned for
        this call - the scales s_k are derived from IT; dot: the inner product (refine_gcr_ref.device_dot: the device's
        order of summation).  The stop decision and the history returned stay the model's own.
        Refused where solve_refine is (_refine_guard); MGX_ERR_INVALID as the device's"""
        self._refine_guard()
        if not 1 <= restart <= 8 or not tol >= 0.0 or max_iters < 0:
            raise ValueError("MGX_ERR_INVALID")
        f = self._float_model()
        f.fine_updates = 0.0
        L = self.L

        def cycle32(r32):
            f.set_rhs(r32)
            f.vcycle_zero()
            return f.U[L]

        self.basis = True
        x, hist, conv, brk = refine_gcr_ref.refine_gcr(self.finest_operator(), cycle32, self.B[L], self.U[L], tol=tol, max_iters=max_iters,
                                                       restart=restart, history=history, dot=dot)
        self.U[L] = np.ascontiguousarray(x, dtype=self.dt)
        self.fine_updates = f.fine_updates
        return dict(cycles=len(hist) - 1, converged=int(conv and not brk), fine_updates=self.fine_updates), hist

    def time_refine_gcr_pass(self, which, repeats):
        """mgx_time_refine_gcr_pass: nothing moves (both passes rewrite buffers that mean nothing between two solves).
        Refused where solve_refine_gcr is, and - what the device's guard looks at - until the float model AND slot 0 of the
        GCR basis exist: a solve_refine_gcr creates both, so do a solve_refine and a solve_gcr together"""
        if which not in (0, 1) or repeats < 1:
            raise ValueError("MGX_ERR_INVALID")
        self._refine_guard()
        if self.f32 is None or not self.basis:
            raise ValueError("mgx_time_refine_gcr_pass: call mgx_solve_refine_gcr first")

    # -- mgx_set_reaction / mgx_get_reaction -------------------------------------------------------------------
    def _reaction_guard(self):
        """the handles that carry no zero-order term (the device: MGX_ERR_STATE), and the line smoothers, which stay out
        of the model here as under a nine-point finest level"""
        if self.op != GALERKIN:
            raise RuntimeError("zero-order terms: GALERKIN handles only (POISSON, STENCIL5: MGX_ERR_STATE)")
        if self.line:
            raise ValueError("a zero-order term under a line smoother is not modelled")
        if self.st5 is None and self.st9 is None:
            raise RuntimeError("finest operator not set: MGX_ERR_STATE")

    def _finest(self):
        """the finest operator as stored: five or nine arrays, slot 0 the (shifted) centre"""
        return self.st9 if self.st9 is not None else self.st5

    def base_operator(self):
        """A0 as nine arrays: the finest operator without the term (slot 0 is c0 while one is set)"""
        st9 = list(self.st9) if self.st9 is not None else gr.nine(self.st5[:5])
        return st9 if self.d is None else [self.c0] + st9[1:]

    def set_reaction(self, d):
        """mgx_set_reaction: slot 0 of the finest operator becomes c0 + d (theta_ref.shift: one rounding in the working
        type); a second call replaces the term.  None with a term set restores c0, None with none set changes nothing.
        Every call that changes the operator leaves the hierarchy invalid until build_galerkin, as set_stencil does"""
        self._reaction_guard()
        st = self._finest()
        if d is None:
            if self.d is None:
                return                          # nothing to remove: the hierarchy stays valid
            st[0] = self.c0
            self.c0 = self.d = None
        else:
            d = np.array(d, dtype=self.wdt, order="C")
            if d.size != self.n(self.L) ** 2:
                raise ValueError("MGX_ERR_INVALID")
            if self.d is None:
                self.c0 = st[0]
            self.d = d.reshape((self.n(self.L),) * 2)
            st[0] = tr.shift([self.c0], self.d)[0]
        self.h = None
        self.transfer = None

    def get_reaction(self):
        self._reaction_guard()
        if self.d is None:
            raise RuntimeError("mgx_get_reaction: no zero-order term is set: MGX_ERR_STATE")
        return self.d

    # -- mgx_theta_steps ---------------------------------------------------------------------------------------
    def _step_solve(self, solver, tol, max_iters, restart, history=None, dot=None):
        """the solver of a step from the current U: (stats, history)"""
        dot = pcg_ref.dot if dot is None else dot
        if solver == STEP_SOLVE:
            return self.solve(tol=tol, max_cycles=max_iters)
        if solver == STEP_GCR:
            return self.solve_gcr(tol=tol, max_iters=max_iters, restart=restart, dot=dot)
        return self.solve_refine_gcr(tol=tol, max_iters=max_iters, restart=restart, history=history, dot=dot)

    @staticmethod
    def _step_solver_check(solver, tol, max_iters, restart):
        if solver not in (STEP_SOLVE, STEP_GCR, STEP_REFINE_GCR) or not tol >= 0.0 or max_iters < 0:
            raise ValueError("MGX_ERR_INVALID")
        if solver != STEP_SOLVE and not 1 <= restart <= 8:
            raise ValueError("MGX_ERR_INVALID")

    def _built_guard(self, solver):
        if solver == STEP_REFINE_GCR:
            self._refine_guard()
        if self.h is None:
            raise RuntimeError("Galerkin hierarchy not built: MGX_ERR_STATE")

    def theta_steps(self, theta, nsteps, g=None, solver=STEP_SOLVE, tol=1e-8, max_iters=50, restart=4, histories=None, dot=None):
        """mgx_theta_steps: (steps_done, [stats], [history]).  Per step theta_ref.rhs_pass from the model's own S u (minus
        the residual of U against a zero right-hand side) into B of the finest level, then the model's solve, solve_gcr or
        solve_refine_gcr from the current U; a step with converged = 0 is the last one; nsteps = 0 moves nothing.
        histories: the per-step histories a device returned (the scales of solve_refine_gcr); dot: the Krylov solvers'
        inner product"""
        if not 0.0 < theta <= 1.0 or nsteps < 0:
            raise ValueError("MGX_ERR_INVALID")
        self._step_solver_check(solver, tol, max_iters, restart)
        self._reaction_guard()
        if self.d is None:
            raise RuntimeError("mgx_theta_steps: no zero-order term is set: MGX_ERR_STATE")
        self._built_guard(solver)
        L = self.L
        stats, hists = [], []
        for k in range(nsteps):
            u = self.U[L]
            Su = None if float(theta) == 1.0 else -self.h.residual(L, u, np.zeros_like(u))
            self.B[L] = np.ascontiguousarray(tr.rhs_pass(Su, u, self.d, g, theta), dtype=self.dt)
            st, h = self._step_solve(solver, tol, max_iters, restart, None if histories is None or k >= len(histories) else histories[k], dot)
            stats.append(st)
            hists.append(h)
            if not st["converged"]:
                break
        return len(stats), stats, hists

    def time_theta_rhs(self, theta, repeats):
        """mgx_time_theta_rhs: nothing moves (the pass writes the finest R); refused while no term is set"""
        if repeats < 1 or not 0.0 < theta <= 1.0:
            raise ValueError("MGX_ERR_INVALID")
        self._reaction_guard()
        if self.d is None:
            raise RuntimeError("mgx_time_theta_rhs: no zero-order term is set: MGX_ERR_STATE")

    # -- mgx_newton / mgx_newton_steps -------------------------------------------------------------------------
    def _newton_check(self, p, solver, lin_tol, lin_max_iters, restart, tol, max_newton, max_backtracks):
        if not all(np.isfinite(float(x)) for x in p):
            raise ValueError("MGX_ERR_INVALID")
        self._step_solver_check(solver, lin_tol, lin_max_iters, restart)
        if not tol >= 0.0 or max_newton < 0 or not 0 <= max_backtracks <= 30:
            raise ValueError("MGX_ERR_INVALID")

    def _grid(self, a):
        if a is None:
            raise ValueError("MGX_ERR_INVALID")
        a = np.array(a, dtype=self.wdt, order="C")
        if a.size != self.n(self.L) ** 2:
            raise ValueError("MGX_ERR_INVALID")
        return a.reshape((self.n(self.L),) * 2)

    def _newton_parts(self, solver, lin_tol, lin_max_iters, restart, dot):
        """(solve, norm) for newton_ref.newton's loop on this handle: the linear solve is set_reaction(d), build_galerkin
        with the transfer in use, set_rhs(b), a zero U and the chosen solver; the norm is residual_norm of (B = b, U = 0)"""
        L, transfer = self.L, self.transfer
        self.norms, self.lin = [], []

        def solve(S9, b, d, k):
            self.set_reaction(d)
            self.build_galerkin(transfer)
            self.set_rhs(b)
            self.zero_level(L, 0)
            rec = self._step_solve(solver, lin_tol, lin_max_iters, restart, None, dot)
            self.lin.append(rec)
            return self.U[L], rec

        def norm(b):
            b = np.ascontiguousarray(b, dtype=self.dt)
            r = self.po.norm2(self._ops().residual(L, np.zeros_like(b), b))
            self.norms.append(r)
            return r

        return solve, norm

    @staticmethod
    def _newton_stats(o):
        return dict(iterations=len(o["hist"]) - 1, converged=int(o["converged"]), backtracks=o["backtracks"],
                    linear_iterations=sum(rec[0]["cycles"] for rec in o["lin"]), failed=o["failed"])

    def newton(self, kappa, p=(0.0, 0.0, 1.0), solver=STEP_SOLVE, lin_tol=1e-8, lin_max_iters=50, restart=4, tol=1e-10, max_newton=20,
               max_backtracks=8, dot=None):
        """mgx_newton: (stats, history, [(stats, history) of every linear solve], step lengths) - newton_ref.newton's
        loop with A0 = base_operator() (a caller's term is not part of F), f = B and the guess = U of the finest level.
        Afterwards U is the last accepted iterate and B the caller's f; when an iteration ran, the operator is A0 + diag(d_k)
        of the last linear solve with its hierarchy built and the coarse levels hold what that solve left; when none
        ran, nothing has moved.  A failed line search: stats["failed"], converged = 0"""
        self._newton_check(p, solver, lin_tol, lin_max_iters, restart, tol, max_newton, max_backtracks)
        kap = self._grid(kappa)
        self._reaction_guard()
        self._built_guard(solver)
        self.nwt = True
        L = self.L
        f = self.B[L]
        solve, norm = self._newton_parts(solver, lin_tol, lin_max_iters, restart, dot)
        o = nf.newton(self.base_operator(), kap, f, p, self.U[L], solve, tol, max_newton, max_backtracks, norm)
        self.U[L] = np.ascontiguousarray(o["u"], dtype=self.dt)
        self.B[L] = f
        return self._newton_stats(o), o["hist"], o["lin"], o["lam"]

    def newton_steps(self, theta, nsteps, mass, kappa, g=None, p=(0.0, 0.0, 1.0), solver=STEP_SOLVE, lin_tol=1e-8, lin_max_iters=50,
                     restart=4, tol=1e-8, max_newton=20, max_backtracks=8, dot=None):
        """mgx_newton_steps: (steps_done, [stats], [history]) - newton_steps_ref.steps with newton()'s linear solve and
        norm.  Afterwards U is the last time level and B the last step's r; the operator as after newton(); a step that does
        not converge is the last one; nsteps = 0 touches nothing, the workspace included"""
        self._newton_check(p, solver, lin_tol, lin_max_iters, restart, tol, max_newton, max_backtracks)
        if not 0.0 < theta <= 1.0 or nsteps < 0:
            raise ValueError("MGX_ERR_INVALID")
        dm, kap = self._grid(mass), self._grid(kappa)
        self._reaction_guard()
        self._built_guard(solver)
        if nsteps == 0:
            return 0, [], []
        self.nwt = self.nwt_mass = True
        L = self.L
        solve, norm = self._newton_parts(solver, lin_tol, lin_max_iters, restart, dot)
        out = nsr.steps(self.base_operator(), kap, dm, None if g is None else self._grid(g), p, self.U[L], theta, nsteps, solve, tol,
                        max_newton, max_backtracks, norm)
        self.U[L] = np.ascontiguousarray(out[-1]["u"], dtype=self.dt)
        self.B[L] = np.ascontiguousarray(out[-1]["r"], dtype=self.dt)
        return len(out), [self._newton_stats(o) for o in out], [o["hist"] for o in out]

    def time_newton_pass(self, step, repeats):
        """mgx_time_newton_pass: nothing moves (the pass writes the finest R, the trial and the next d of the workspace);
        refused until a newton or a newton_steps call has allocated the workspace"""
        if step not in (0, 1) or repeats < 1:
            raise ValueError("MGX_ERR_INVALID")
        self._reaction_guard()
        if not self.nwt:
            raise RuntimeError("mgx_time_newton_pass: call mgx_newton first: MGX_ERR_STATE")

    def time_newton_step_pass(self, which, theta, repeats):
        """mgx_time_newton_step_pass: nothing moves; refused until a newton_steps call has allocated the mass grid"""
        if which not in (0, 1, 2) or repeats < 1 or not 0.0 < theta <= 1.0:
            raise ValueError("MGX_ERR_INVALID")
        self._reaction_guard()
        if not self.nwt_mass:
            raise RuntimeError("mgx_time_newton_step_pass: call mgx_newton_steps first: MGX_ERR_STATE")
