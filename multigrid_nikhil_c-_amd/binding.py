"""ctypes binding of libmgx.so (include/mgx.h).

The method names follow the reference's free functions so that callers read
like the reference's own driver (PS = Poissons_SYCL.cpp):
    jacobirelaxation   PS:125      restriction2d     PS:531
    interpolation2d    PS:337      vcyclemultigrid   PS:575
    fullmultigrid      PS:629      solve             PS:727 (main's call)

There is no CPU fallback: if libmgx.so is missing or no HIP device is usable
every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MGX_LIBMGX_PATH: another build of the same library (A/B measurements inside one GPU call)
LIB_PATH = os.environ.get("MGX_LIBMGX_PATH") or os.path.join(_HERE, "libmgx.so")

SMOOTHER_JACOBI, SMOOTHER_RBGS = 0, 1
SMOOTHER_CHEBYSHEV = 2      # Chebyshev polynomial smoother of the general-operator hierarchies (mu1 / mu2: degrees)
# zebra line Gauss-Seidel of the general-operator hierarchies: x-lines, y-lines, x then y (3 is not a smoother)
SMOOTHER_LINE_X, SMOOTHER_LINE_Y, SMOOTHER_LINE_ALT = 4, 5, 6
# multicolour point Gauss-Seidel of the general-operator hierarchies: every block forward / post-smoothing blocks in reverse
SMOOTHER_COLOR_GS, SMOOTHER_COLOR_SGS = 8, 9          # (7, like 3, is not a smoother)
DTYPE_F32, DTYPE_F64, DTYPE_MIXED = 0, 1, 2
GCR_MAX_RESTART = 8                       # MGX_GCR_MAX_RESTART
SCHEDULE_V, SCHEDULE_FMG = 0, 1
RESTRICT_CONSISTENT, RESTRICT_FW16, RESTRICT_INJECT, RESTRICT_INJECT4 = 0, 1, 2, 3
OPERATOR_POISSON, OPERATOR_STENCIL5 = 0, 1
OPERATOR_GALERKIN = OP_GALERKIN = 3      # coarse operators R A P (nine-point), built on the device by build_galerkin()
TRANSFER_BILINEAR, TRANSFER_OPERATOR = 0, 1     # P of the Galerkin hierarchy: weights 1/2, 1/4, or read off the operator's stencil
BOTTOM_EXACT, BOTTOM_SMOOTH = 0, 1
CYCLE_V, CYCLE_W, CYCLE_F = 0, 1, 2     # cycle index of a general-operator handle (set_cycle): one or two visits of every coarse level
ARITH_SEPARATE, ARITH_FMA = 0, 1
VEC_U, VEC_B, VEC_R = 0, 1, 2
PROF_SMOOTH_FINE, PROF_RESTRICT_FINE, PROF_PROLONG_FINE, PROF_NORM_FINE, PROF_COARSE, PROF_COUNT = 0, 1, 2, 3, 4, 5

# every symbol include/mgx.h declares (tests check the library exports them all)
EXPORTS = [
    "mgx_config_default", "mgx_create", "mgx_destroy", "mgx_last_error", "mgx_status_string",
    "mgx_level_n", "mgx_set_rhs", "mgx_set_rhs_dirichlet", "mgx_set_guess", "mgx_get_solution", "mgx_set_level",
    "mgx_get_level", "mgx_set_level_device", "mgx_get_level_device", "mgx_zero_level", "mgx_fill_rhs", "mgx_fill_guess_random", "mgx_smooth", "mgx_residual",
    "mgx_restrict", "mgx_restrict_rhs", "mgx_prolong_add", "mgx_prolong", "mgx_bottom_solve",
    "mgx_residual_norm", "mgx_vcycle", "mgx_vcycle_zero", "mgx_fmg", "mgx_solve", "mgx_profile_reset",
    "mgx_profile_get", "mgx_time_smoother", "mgx_synchronize", "mgx_graphs_cached", "mgx_slab_cycle", "mgx_level_pitch",
    "mgx_slab_jacobi", "mgx_slab_rbgs", "mgx_slab_restrict", "mgx_slab_prolong",
    "mgx_slab_residual_sumsq", "mgx_slab_scratch_doubles",
    "mgx_plan_create", "mgx_plan_destroy", "mgx_plan_last_error", "mgx_plan_cut_level", "mgx_plan_level",
    "mgx_plan_cut_share", "mgx_plan_guess_set", "mgx_plan_vcycle", "mgx_plan_norm", "mgx_plan_fmg", "mgx_rccl_unique_id",
    "mgx_create_rank", "mgx_dist_exchanges", "mgx_dist_overlapped", "mgx_memcpy_d2h", "mgx_memcpy_h2d", "mgx_runtime_libs",
    "mgx_set_stencil", "mgx_set_coefficient", "mgx_get_stencil", "mgx_solve_pcg", "mgx_solve_gcr", "mgx_time_gcr_pass",
    "mgx_build_galerkin", "mgx_get_stencil9", "mgx_set_stencil9", "mgx_set_tensor",
    "mgx_build_galerkin_transfer", "mgx_get_transfer", "mgx_get_prolongation", "mgx_get_lambda_max", "mgx_get_line_factor", "mgx_get_line_chunks",
    "mgx_set_cycle", "mgx_get_cycle", "mgx_solve_refine", "mgx_time_refine_pass",
    "mgx_solve_refine_gcr", "mgx_time_refine_gcr_pass", "mgx_solve_multi", "mgx_time_multi_smoother",
    "mgx_solve_multi_gcr", "mgx_time_multi_gcr_direction", "mgx_solve_multi_refine_gcr", "mgx_time_multi_refine_direction",
    "mgx_eigs", "mgx_time_eig_pass", "mgx_eigs_many", "mgx_time_eig_project",
    "mgx_set_reaction", "mgx_get_reaction", "mgx_theta_steps", "mgx_time_theta_rhs",
    "mgx_newton", "mgx_time_newton_pass", "mgx_newton_steps", "mgx_time_newton_step_pass",
    "mgx_quasi", "mgx_time_quasi_pass",
]
QUASI_PICARD, QUASI_NEWTON = 0, 1                    # what the pass of quasi() writes: A(u) or the Jacobian of A(u) u - f
QUASI_METHODS = {"picard": QUASI_PICARD, "newton": QUASI_NEWTON}
STEP_SOLVE, STEP_GCR, STEP_REFINE_GCR = 0, 1, 2      # the solver of a theta step (theta_steps)
STEP_SOLVERS = {"solve": STEP_SOLVE, "gcr": STEP_GCR, "refine_gcr": STEP_REFINE_GCR}
EIG_PASS_GRAM, EIG_PASS_COMBINE, EIG_PASS_RESIDUAL, EIG_PASS_APPLY = 0, 1, 2, 3
EIG_PROJECT_DOTS, EIG_PROJECT_SUB = 0, 1
EIGS_MAX = 16
MAX_RHS = 4
MAX_GPUS = 16
(DOP_EXCHANGE, DOP_ZERO_U, DOP_CYCLE, DOP_SMOOTH, DOP_RESTRICT, DOP_PROLONG, DOP_GATHER_CUT, DOP_COARSE, DOP_SUMSQ,
 DOP_ALLREDUCE_NORM, DOP_RESTRICT_RHS, DOP_PROLONG_SET, DOP_COARSE_FMG) = range(1, 14)


class Config(C.Structure):
    _fields_ = [
        ("finest_level", C.c_int), ("coarsest_level", C.c_int),
        ("mu0", C.c_int), ("mu1", C.c_int), ("mu2", C.c_int),
        ("omega", C.c_double),
        ("smoother", C.c_int), ("dtype", C.c_int), ("schedule", C.c_int),
        ("restrict_mode", C.c_int), ("bottom", C.c_int),
        ("device", C.c_int), ("profile", C.c_int),
        ("n_gpus", C.c_int), ("cut_level", C.c_int), ("devices", C.c_int * MAX_GPUS),
        ("arith", C.c_int), ("op", C.c_int),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("cycles", C.c_int), ("converged", C.c_int),
        ("initial_residual", C.c_double), ("final_residual", C.c_double),
        ("seconds", C.c_double), ("fine_updates", C.c_double), ("history_len", C.c_int),
    ]


class NewtonOpts(C.Structure):
    """mgx_newton_opts"""
    _fields_ = [
        ("p1", C.c_double), ("p2", C.c_double), ("p3", C.c_double),
        ("solver", C.c_int), ("lin_tol", C.c_double), ("lin_max_iters", C.c_int), ("restart", C.c_int),
        ("tol", C.c_double), ("max_newton", C.c_int), ("max_backtracks", C.c_int),
    ]


class QuasiOpts(C.Structure):
    """mgx_quasi_opts"""
    _fields_ = [
        ("k0", C.c_double), ("k1", C.c_double), ("k2", C.c_double),
        ("method", C.c_int), ("transfer", C.c_int),
        ("solver", C.c_int), ("lin_tol", C.c_double), ("lin_max_iters", C.c_int), ("restart", C.c_int),
        ("tol", C.c_double), ("max_iters", C.c_int), ("max_backtracks", C.c_int),
    ]


class NewtonStats(C.Structure):
    """mgx_newton_stats"""
    _fields_ = [
        ("iterations", C.c_int), ("converged", C.c_int),
        ("initial_residual", C.c_double), ("final_residual", C.c_double), ("seconds", C.c_double),
        ("linear_iterations", C.c_int), ("backtracks", C.c_int), ("history_len", C.c_int),
    ]


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * PROF_COUNT), ("launches", C.c_longlong * PROF_COUNT),
                ("sweeps", C.c_longlong * PROF_COUNT)]


class Slab(C.Structure):
    _fields_ = [("level", C.c_int), ("dtype", C.c_int), ("rows", C.c_int), ("row0", C.c_int), ("arith", C.c_int)]


class DistOp(C.Structure):
    """mgx_dist_op: one operation of a slab plan"""
    _fields_ = [("op", C.c_int), ("level", C.c_int), ("which", C.c_int), ("depth", C.c_int),
                ("row_lo", C.c_int), ("row_hi", C.c_int), ("mu", C.c_int), ("pre", C.c_int), ("post", C.c_int),
                ("crow_lo", C.c_int), ("crow_hi", C.c_int), ("coarse_is_cut", C.c_int)]


class DistLevel(C.Structure):
    _fields_ = [("level", C.c_int), ("N", C.c_int), ("own_lo", C.c_int), ("own_hi", C.c_int), ("halo", C.c_int),
                ("row0", C.c_int), ("rows", C.c_int)]


class Xfer(C.Structure):
    _fields_ = [("send", C.c_int), ("peer", C.c_int), ("ptr", C.c_void_p), ("bytes", C.c_size_t)]


SENDRECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(Xfer), C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double))


class Transport(C.Structure):
    """mgx_transport: what moves between the slabs of different processes"""
    _fields_ = [("ctx", C.c_void_p), ("sendrecv", SENDRECV_FN), ("allgather", ALLGATHER_FN), ("allreduce_sum", ALLREDUCE_FN)]


class MgxError(RuntimeError):
    pass


def rccl_unique_id() -> bytes:
    """128 bytes naming a new RCCL communicator (rank 0 calls it, the launcher hands them to every rank)"""
    buf = C.create_string_buffer(128)
    if lib().mgx_rccl_unique_id(buf) != 0:
        raise MgxError("mgx_rccl_unique_id failed")
    return buf.raw


_lib = None


def lib() -> C.CDLL:
    """Load libmgx.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MgxError(
            f"{LIB_PATH} not found: build it with `make -C multigrid_nikhil_c-_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.mgx_config_default.argtypes = [C.POINTER(Config)]
    L.mgx_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.mgx_destroy.argtypes = [vp]
    L.mgx_last_error.argtypes = [vp]
    L.mgx_last_error.restype = C.c_char_p
    L.mgx_status_string.argtypes = [C.c_int]
    L.mgx_status_string.restype = C.c_char_p
    L.mgx_level_n.argtypes = [C.c_int]
    L.mgx_level_pitch.argtypes = [C.c_int, C.c_int]
    L.mgx_level_pitch.restype = C.c_long
    for name in ("mgx_set_rhs", "mgx_set_guess", "mgx_get_solution"):
        getattr(L, name).argtypes = [vp, vp, C.c_size_t]
    L.mgx_set_rhs_dirichlet.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t]
    L.mgx_set_level.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.mgx_get_level.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.mgx_set_level_device.argtypes = [vp, C.c_int, C.c_int, vp]
    L.mgx_get_level_device.argtypes = [vp, C.c_int, C.c_int, vp]
    L.mgx_zero_level.argtypes = [vp, C.c_int, C.c_int]
    L.mgx_fill_rhs.argtypes = [vp, C.c_int, C.c_double]
    L.mgx_fill_guess_random.argtypes = [vp, C.c_uint64]
    L.mgx_smooth.argtypes = [vp, C.c_int, C.c_int]
    for name in ("mgx_residual", "mgx_restrict", "mgx_restrict_rhs", "mgx_prolong_add", "mgx_prolong", "mgx_vcycle"):
        getattr(L, name).argtypes = [vp, C.c_int]
    for name in ("mgx_bottom_solve", "mgx_fmg", "mgx_vcycle_zero", "mgx_profile_reset", "mgx_synchronize", "mgx_graphs_cached"):
        getattr(L, name).argtypes = [vp]
    L.mgx_residual_norm.argtypes = [vp, C.c_int, dp]
    L.mgx_solve.argtypes = [vp, C.c_double, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_solve_pcg.argtypes = [vp, C.c_double, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_solve_gcr.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_solve_refine.argtypes = [vp, C.c_double, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_time_refine_pass.argtypes = [vp, C.c_int, dp]
    L.mgx_solve_refine_gcr.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_time_refine_gcr_pass.argtypes = [vp, C.c_int, C.c_int, dp]
    L.mgx_solve_multi.argtypes = [vp, C.c_int, vp, vp, C.c_double, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_time_multi_smoother.argtypes = [vp, C.c_int, C.c_int, dp]
    L.mgx_solve_multi_gcr.argtypes = [vp, C.c_int, vp, vp, C.c_double, C.c_int, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_time_multi_gcr_direction.argtypes = [vp, C.c_int, C.c_int, dp]
    L.mgx_solve_multi_refine_gcr.argtypes = [vp, C.c_int, vp, vp, C.c_double, C.c_int, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_time_multi_refine_direction.argtypes = [vp, C.c_int, C.c_int, dp]
    L.mgx_eigs.argtypes = [vp, C.c_int, vp, dp, C.c_double, C.c_int, C.POINTER(Stats), dp, C.c_int]
    L.mgx_time_eig_pass.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    L.mgx_eigs_many.argtypes = L.mgx_eigs.argtypes
    L.mgx_time_eig_project.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp]
    L.mgx_profile_get.argtypes = [vp, C.POINTER(Profile)]
    L.mgx_time_smoother.argtypes = [vp, C.c_int, dp]
    L.mgx_time_gcr_pass.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    sp = C.POINTER(Slab)
    L.mgx_slab_jacobi.argtypes = [sp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, ip, vp]
    L.mgx_slab_rbgs.argtypes = [sp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, vp]
    L.mgx_slab_cycle.argtypes = [sp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, sp, vp, vp,
                                 C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, ip, vp]
    L.mgx_slab_restrict.argtypes = [sp, vp, vp, sp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.mgx_slab_prolong.argtypes = [sp, vp, sp, vp, C.c_int, C.c_int, C.c_int, vp]
    L.mgx_slab_residual_sumsq.argtypes = [sp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.mgx_slab_scratch_doubles.argtypes = [sp]
    L.mgx_slab_scratch_doubles.restype = C.c_long
    L.mgx_plan_create.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.mgx_plan_destroy.argtypes = [vp]
    L.mgx_plan_last_error.restype = C.c_char_p
    L.mgx_plan_cut_level.argtypes = [vp]
    L.mgx_plan_level.argtypes = [vp, C.c_int, C.POINTER(DistLevel)]
    L.mgx_plan_cut_share.argtypes = [vp, ip, ip]
    L.mgx_plan_guess_set.argtypes = [vp, C.c_int]
    L.mgx_plan_vcycle.argtypes = [vp, C.POINTER(DistOp), C.c_int]
    L.mgx_plan_norm.argtypes = [vp, C.POINTER(DistOp), C.c_int]
    L.mgx_plan_fmg.argtypes = [vp, C.POINTER(DistOp), C.c_int]
    L.mgx_rccl_unique_id.argtypes = [vp]
    L.mgx_create_rank.argtypes = [C.POINTER(Config), C.c_int, C.c_int, vp, C.POINTER(Transport), C.POINTER(vp)]
    L.mgx_dist_exchanges.argtypes = [vp]
    L.mgx_dist_exchanges.restype = C.c_long
    L.mgx_dist_overlapped.argtypes = [vp]
    L.mgx_dist_overlapped.restype = C.c_long
    L.mgx_memcpy_d2h.argtypes = [vp, vp, C.c_size_t, vp]
    L.mgx_memcpy_h2d.argtypes = [vp, vp, C.c_size_t, vp]
    L.mgx_runtime_libs.argtypes = [C.c_char_p, C.c_size_t]
    L.mgx_set_stencil.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, C.c_size_t]
    L.mgx_set_coefficient.argtypes = [vp, vp, C.c_size_t]
    L.mgx_set_stencil9.argtypes = [vp, C.c_int] + [vp] * 9 + [C.c_size_t]
    L.mgx_set_tensor.argtypes = [vp, vp, vp, vp, C.c_size_t]
    L.mgx_get_stencil.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.mgx_build_galerkin.argtypes = [vp]
    L.mgx_get_stencil9.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.mgx_build_galerkin_transfer.argtypes = [vp, C.c_int]
    L.mgx_get_transfer.argtypes = [vp, ip]
    L.mgx_get_prolongation.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.mgx_get_lambda_max.argtypes = [vp, C.c_int, dp]
    L.mgx_get_line_factor.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t]
    L.mgx_get_line_chunks.argtypes = [vp, C.c_int, ip, ip]
    L.mgx_set_cycle.argtypes = [vp, C.c_int]
    L.mgx_get_cycle.argtypes = [vp, ip]
    L.mgx_set_reaction.argtypes = [vp, vp, C.c_size_t]
    L.mgx_get_reaction.argtypes = [vp, vp, C.c_size_t]
    L.mgx_theta_steps.argtypes = [vp, C.c_double, C.c_int, vp, C.c_int, C.c_double, C.c_int, C.c_int, ip, C.POINTER(Stats), dp, C.c_int]
    L.mgx_time_theta_rhs.argtypes = [vp, C.c_double, C.c_int, dp]
    L.mgx_newton.argtypes = [vp, C.POINTER(NewtonOpts), vp, C.c_size_t, C.POINTER(NewtonStats), C.POINTER(Stats), dp, dp, C.c_int]
    L.mgx_time_newton_pass.argtypes = [vp, C.c_int, C.c_int, dp]
    L.mgx_newton_steps.argtypes = [vp, C.POINTER(NewtonOpts), C.c_double, C.c_int, vp, vp, vp, C.c_size_t, ip, C.POINTER(NewtonStats), dp, C.c_int]
    L.mgx_time_newton_step_pass.argtypes = [vp, C.c_int, C.c_double, C.c_int, dp]
    L.mgx_quasi.argtypes = [vp, C.POINTER(QuasiOpts), vp, C.c_size_t, C.POINTER(NewtonStats), C.POINTER(Stats), dp, dp, C.c_int]
    L.mgx_time_quasi_pass.argtypes = [vp, C.c_int, C.c_int, C.c_int, dp]
    _lib = L
    return L


def runtime_libs() -> list[str]:
    """paths of the ROCm runtime libraries (and libmgx) mapped into this process (mgx_runtime_libs)"""
    buf = C.create_string_buffer(16384)
    if lib().mgx_runtime_libs(buf, len(buf)) < 0:
        return []
    return [p for p in buf.value.decode().splitlines() if p]


def lib_loaded() -> bool:
    """has libmgx.so been loaded into this process yet?"""
    return _lib is not None


def default_config(**kw) -> Config:
    c = Config()
    lib().mgx_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise TypeError(f"unknown mgx_config field {k!r}")
        if k == "devices":
            for i, d in enumerate(v):
                c.devices[i] = int(d)
        else:
            setattr(c, k, v)
    return c


class Plan:
    """mgx_plan_*: the multi-GPU V-cycle of slab `g` of `n_slabs` as a list of operations (host
    logic only: usable without a GPU; the CPU tests execute these plans over numpy and gloo)"""

    def __init__(self, n_slabs, g, fold=True, deep=True, **cfg):
        self.cfg = default_config(**cfg)
        self._h = C.c_void_p()
        st = lib().mgx_plan_create(C.byref(self.cfg), n_slabs, g, 1 if fold else 0, 1 if deep else 0, C.byref(self._h))
        if st != 0:
            raise MgxError(f"mgx_plan_create: {lib().mgx_plan_last_error().decode()}")
        self.cut = lib().mgx_plan_cut_level(self._h)
        r0, rows = C.c_int(), C.c_int()
        lib().mgx_plan_cut_share(self._h, C.byref(r0), C.byref(rows))
        self.c_row0, self.c_rows = r0.value, rows.value

    def level(self, level):
        g = DistLevel()
        if lib().mgx_plan_level(self._h, level, C.byref(g)) != 0:
            raise MgxError("mgx_plan_level: level is not distributed")
        return g

    def guess_set(self, all_rows=True):
        lib().mgx_plan_guess_set(self._h, 1 if all_rows else 0)

    def _emit(self, fn):
        cap = 4096
        buf = (DistOp * cap)()
        n = fn(self._h, buf, cap)
        if n < 0:
            raise MgxError(f"plan longer than {cap} operations")
        return [buf[i] for i in range(n)]

    def fmg(self):
        return self._emit(lib().mgx_plan_fmg)

    def vcycle(self):
        return self._emit(lib().mgx_plan_vcycle)

    def norm(self):
        return self._emit(lib().mgx_plan_norm)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mgx_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Multigrid:
    """One mgx_handle: the grid hierarchy of PS:661-690 plus the operators and
    schedules that act on it.  Vectors cross this boundary as 2-D numpy arrays
    in the reference's interior-only n x n layout (PS:227, 291)."""

    def __init__(self, _rank=None, **cfg):
        self.cfg = default_config(**cfg)
        self._h = C.c_void_p()
        self._keep = None
        if _rank is None:
            st = lib().mgx_create(C.byref(self.cfg), C.byref(self._h))
        else:
            rank, world, rccl_id, transport = _rank
            self._keep = (rccl_id, transport)              # callbacks / id bytes must outlive the handle
            st = lib().mgx_create_rank(C.byref(self.cfg), rank, world, rccl_id,
                                       C.byref(transport) if transport is not None else None, C.byref(self._h))
        if st != 0:
            msg = lib().mgx_last_error(None).decode()
            self._h = C.c_void_p()
            raise MgxError(f"mgx_create: {lib().mgx_status_string(st).decode()}: {msg}")

    @classmethod
    def rank(cls, rank, world, rccl_id=None, transport=None, **cfg):
        """mgx_create_rank: this process owns slab `rank` of `world` (one process per GPU).
        rccl_id: the 128 bytes of rccl_unique_id() from rank 0 (built-in RCCL transport), or
        transport: a Transport of the caller's."""
        idbuf = C.create_string_buffer(bytes(rccl_id), 128) if rccl_id is not None else None
        return cls(_rank=(rank, world, idbuf, transport), **cfg)

    def exchanges(self):
        """halo exchanges a multi-GPU handle has performed"""
        return int(lib().mgx_dist_exchanges(self._h))

    def overlapped(self):
        """... of which ran beside the interior rows of the smoothing pass they feed"""
        return int(lib().mgx_dist_overlapped(self._h))

    # -- plumbing --------------------------------------------------------------
    def _chk(self, st, what):
        if st != 0:
            raise MgxError(f"{what}: {lib().mgx_status_string(st).decode()}: {lib().mgx_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().mgx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def n(self, level=None):
        return (1 << (self.cfg.finest_level if level is None else level)) - 1

    def level_dtype(self, level, which=VEC_U):
        d = self.cfg.dtype
        if d == DTYPE_F64 or (d == DTYPE_MIXED and level == self.cfg.finest_level):
            return np.float64
        return np.float32

    def set_level(self, level, which, a):
        a = np.ascontiguousarray(a, dtype=self.level_dtype(level, which))
        self._chk(lib().mgx_set_level(self._h, level, which, a.ctypes.data, a.size), "mgx_set_level")

    def get_level(self, level, which):
        n = self.n(level)
        a = np.empty((n, n), dtype=self.level_dtype(level, which))
        self._chk(lib().mgx_get_level(self._h, level, which, a.ctypes.data, a.size), "mgx_get_level")
        return a

    def set_level_device(self, level, which, ptr):
        """device-resident input: `ptr` addresses a whole level grid (rows 0..N x pitch)"""
        self._chk(lib().mgx_set_level_device(self._h, level, which, ptr), "mgx_set_level_device")

    def get_level_device(self, level, which, ptr):
        self._chk(lib().mgx_get_level_device(self._h, level, which, ptr), "mgx_get_level_device")

    def zero_level(self, level, which):
        self._chk(lib().mgx_zero_level(self._h, level, which), "mgx_zero_level")

    def set_rhs(self, b):
        self.set_level(self.cfg.finest_level, VEC_B, b)

    def set_rhs_dirichlet(self, b, g_top, g_bottom, g_left, g_right):
        """right-hand side with boundary values folded in: g_top/g_bottom are rows 0 and N
        (N+1 values each), g_left/g_right columns 0 and N on rows 1..N-1"""
        dt = self.level_dtype(self.cfg.finest_level, VEC_B)
        b = np.ascontiguousarray(b, dtype=dt)
        ring = np.ascontiguousarray(np.concatenate([g_top, g_bottom, g_left, g_right]), dtype=dt)
        self._chk(lib().mgx_set_rhs_dirichlet(self._h, b.ctypes.data, b.size, ring.ctypes.data, ring.size),
                  "mgx_set_rhs_dirichlet")

    def set_guess(self, u):
        self.set_level(self.cfg.finest_level, VEC_U, u)

    def get_solution(self):
        return self.get_level(self.cfg.finest_level, VEC_U)

    def get_solution_into(self, a):
        """finest-level U into the caller's n x n array (a rank handle of a multi-GPU job fills the
        rows it owns and leaves the others untouched)"""
        assert a.flags["C_CONTIGUOUS"] and a.dtype == self.level_dtype(self.cfg.finest_level)
        self._chk(lib().mgx_get_solution(self._h, a.ctypes.data, a.size), "mgx_get_solution")
        return a

    # -- general per-level operators (MF:16-41) ---------------------------------------
    def set_stencil(self, level, c, n, s, w, e):
        """ProblemVar::A_sp_dict[level]: five interior n x n coefficient arrays"""
        dt = self.level_dtype(level)
        a = [np.ascontiguousarray(x, dtype=dt) for x in (c, n, s, w, e)]
        self._chk(lib().mgx_set_stencil(self._h, level, *[x.ctypes.data for x in a], a[0].size), "mgx_set_stencil")

    def set_coefficient(self, a_nodes):
        """every level's operator from the nodal coefficient of -div(a grad u) on the finest grid ((N + 1)^2 doubles)"""
        a = np.ascontiguousarray(a_nodes, dtype=np.float64)
        self._chk(lib().mgx_set_coefficient(self._h, a.ctypes.data, a.size), "mgx_set_coefficient")

    def set_stencil9(self, level, c, n, s, w, e, nw, ne, sw, se):
        """a nine-point finest operator of a GALERKIN handle: nine interior n x n coefficient arrays in the slot order
        of get_stencil9 (mgx_set_stencil9); build_galerkin() then builds the hierarchy below it"""
        dt = self.level_dtype(level)
        a = [np.ascontiguousarray(x, dtype=dt) for x in (c, n, s, w, e, nw, ne, sw, se)]
        self._chk(lib().mgx_set_stencil9(self._h, level, *[x.ctypes.data for x in a], a[0].size), "mgx_set_stencil9")

    def set_tensor(self, axx, axy, ayy):
        """the nine-point finest operator of -d_x(axx d_x u) - d_y(ayy d_y u) - d_x(axy d_y u) - d_y(axy d_x u) from the
        nodal values of the three coefficients on the finest grid ((N + 1)^2 doubles each; mgx_set_tensor)"""
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (axx, axy, ayy)]
        assert a[0].size == a[1].size == a[2].size, "axx, axy, ayy must have the same size"
        self._chk(lib().mgx_set_tensor(self._h, *[x.ctypes.data for x in a], a[0].size), "mgx_set_tensor")

    def set_reaction(self, d):
        """the zero-order term of a GALERKIN handle's finest operator: S = A0 + diag(d), d an interior n x n grid without
        h^-2 (mgx_set_reaction); None removes it and restores A0 bit for bit.  build_galerkin() then builds the hierarchy of S"""
        if d is None:
            self._chk(lib().mgx_set_reaction(self._h, None, 0), "mgx_set_reaction")
            return
        a = np.ascontiguousarray(d, dtype=self.level_dtype(self.cfg.finest_level))
        self._chk(lib().mgx_set_reaction(self._h, a.ctypes.data, a.size), "mgx_set_reaction")

    def reaction(self):
        """the zero-order term as set_reaction() stored it (mgx_get_reaction); raises when none is set"""
        n = self.n()
        a = np.empty((n, n), dtype=self.level_dtype(self.cfg.finest_level))
        self._chk(lib().mgx_get_reaction(self._h, a.ctypes.data, a.size), "mgx_get_reaction")
        return a

    def theta_steps(self, nsteps, theta=1.0, g=None, solver="solve", tol=1e-8, max_iters=50, restart=4):
        """nsteps theta steps of M u_t + A0 u = f on the device, from the current U (mgx_theta_steps): the handle's operator
        is A0 + diag(d) with d = M / (theta dt) from set_reaction(), g = f / theta (n x n or None) is constant over the
        steps, solver "solve" | "gcr" | "refine_gcr" (or a STEP_* value) solves every step warm-started with tol, max_iters
        (and restart).  Returns (steps_done, list of stats, list of residual histories) of the completed steps; a step that
        does not converge is the last one (mgx_last_error names it).  A V-schedule handle keeps the warm start under "solve"."""
        dt = self.level_dtype(self.cfg.finest_level)
        ga = None if g is None else np.ascontiguousarray(g, dtype=dt)
        if ga is not None:
            assert ga.size == self.n() ** 2, "g must hold n x n values"
        k = max(int(nsteps), 1)
        st = (Stats * k)()
        cap = max(int(max_iters), 0) + 1
        hist = np.zeros((k, cap), dtype=np.float64)
        done = C.c_int(0)
        code = STEP_SOLVERS[solver] if isinstance(solver, str) else int(solver)
        self._chk(lib().mgx_theta_steps(self._h, theta, nsteps, None if ga is None else ga.ctypes.data, code, tol, max_iters, restart,
                                        C.byref(done), st, hist.ctypes.data_as(C.POINTER(C.c_double)), cap), "mgx_theta_steps")
        stats = []
        for j in range(done.value):
            one = Stats()
            C.memmove(C.byref(one), C.byref(st[j]), C.sizeof(Stats))
            stats.append(one)
        return done.value, stats, [hist[j, : stats[j].history_len].copy() for j in range(done.value)]

    def time_theta_rhs(self, theta, repeats=20):
        """ms per launch of theta_steps' right-hand-side pass (k_theta_rhs) on the handle's own buffers, into the finest R: U
        and B unchanged; after a set_reaction()"""
        ms = C.c_double()
        self._chk(lib().mgx_time_theta_rhs(self._h, theta, repeats, C.byref(ms)), "mgx_time_theta_rhs")
        return ms.value

    def newton(self, kappa, p=(0.0, 0.0, 1.0), solver="solve", lin_tol=1e-8, lin_max_iters=50, restart=4, tol=1e-10, max_newton=20,
               max_backtracks=8):
        """Newton-multigrid for -div(a grad u) + kappa phi(u) = f on the device (mgx_newton): phi(u) = p[0] u + p[1] u^2 +
        p[2] u^3, kappa an interior n x n grid in stencil units (kappa h^2), f the current B, the guess the current U.  Every
        step sets the zero-order term kappa phi'(u), rebuilds the hierarchy with its transfer, solves with solver "solve" |
        "gcr" | "refine_gcr" (or a STEP_* value; lin_tol, lin_max_iters, restart) from a zero guess and backtracks on ||F||
        (at most max_backtracks halvings).  Returns (NewtonStats, history of ||F||, list of the linear solves' Stats, step
        lengths); U holds the iterate (get_solution()), B the caller's f.  A failed line search returns converged = 0
        (mgx_last_error names it)."""
        ka = np.ascontiguousarray(kappa, dtype=self.level_dtype(self.cfg.finest_level))
        code = STEP_SOLVERS[solver] if isinstance(solver, str) else int(solver)
        o = NewtonOpts(float(p[0]), float(p[1]), float(p[2]), code, lin_tol, lin_max_iters, restart, tol, max_newton, max_backtracks)
        k = max(int(max_newton), 1)
        st = (Stats * k)()
        lam = np.zeros(k, dtype=np.float64)
        hist = np.zeros(k + 1, dtype=np.float64)
        ns = NewtonStats()
        self._chk(lib().mgx_newton(self._h, C.byref(o), ka.ctypes.data, ka.size, C.byref(ns), st, lam.ctypes.data_as(C.POINTER(C.c_double)),
                                   hist.ctypes.data_as(C.POINTER(C.c_double)), k + 1), "mgx_newton")
        # one linear solve per accepted step, and one more when the call ended in a failed line search (not converged with
        # steps left): that step's solve ran too
        failed = not ns.converged and ns.iterations < int(max_newton)
        stats = []
        for j in range(ns.iterations + (1 if failed else 0)):
            one = Stats()
            C.memmove(C.byref(one), C.byref(st[j]), C.sizeof(Stats))
            stats.append(one)
        return ns, hist[: ns.history_len].copy(), stats, lam[: ns.iterations].copy()

    def time_newton_pass(self, step, repeats=20):
        """ms per launch of newton()'s pass (k_newton_pass and the reduction of its sums) on the handle's own buffers:
        step 0 the first evaluation, 1 a trial with lam = 1; into the finest R, the trial iterate and the next d: U, B, the
        iterate and the operator unchanged; after a newton()"""
        ms = C.c_double()
        self._chk(lib().mgx_time_newton_pass(self._h, int(step), repeats, C.byref(ms)), "mgx_time_newton_pass")
        return ms.value

    def quasi(self, a_nodes, k, method="picard", solver="solve", transfer=TRANSFER_BILINEAR, lin_tol=1e-8, lin_max_iters=50, restart=4,
              tol=1e-10, max_iters=20, max_backtracks=8):
        """Picard or Newton multigrid for -div(a k(u) grad u) = f on the device (mgx_quasi): a_nodes the (N + 1)^2 nodal
        values of a (set_coefficient's argument), k(u) = k[0] + k[1] u + k[2] u^2, f the current B, the guess the current U.
        Every step makes the pass's five grids the finest operator - A(u) for method "picard", the Jacobian of A(u) u - f
        for "newton" (or a QUASI_* value) - rebuilds the hierarchy with `transfer`, solves with solver "solve" | "gcr" |
        "refine_gcr" (or a STEP_* value; lin_tol, lin_max_iters, restart) from a zero guess and backtracks on ||F|| (at
        most max_backtracks halvings).  Returns (NewtonStats, history of ||F||, list of the linear solves' Stats, step
        lengths); U holds the iterate (get_solution()), B the caller's f.  A failed line search returns converged = 0
        (mgx_last_error names it)."""
        a = np.ascontiguousarray(a_nodes, dtype=np.float64)
        code = STEP_SOLVERS[solver] if isinstance(solver, str) else int(solver)
        meth = QUASI_METHODS[method] if isinstance(method, str) else int(method)
        o = QuasiOpts(float(k[0]), float(k[1]), float(k[2]), meth, int(transfer), code, lin_tol, lin_max_iters, restart, tol, max_iters,
                      max_backtracks)
        m = max(int(max_iters), 1)
        st = (Stats * m)()
        lam = np.zeros(m, dtype=np.float64)
        hist = np.zeros(m + 1, dtype=np.float64)
        ns = NewtonStats()
        self._chk(lib().mgx_quasi(self._h, C.byref(o), a.ctypes.data, a.size, C.byref(ns), st, lam.ctypes.data_as(C.POINTER(C.c_double)),
                                  hist.ctypes.data_as(C.POINTER(C.c_double)), m + 1), "mgx_quasi")
        # one linear solve per accepted step, and one more when the call ended in a failed line search
        failed = not ns.converged and ns.iterations < int(max_iters)
        stats = []
        for j in range(ns.iterations + (1 if failed else 0)):
            one = Stats()
            C.memmove(C.byref(one), C.byref(st[j]), C.sizeof(Stats))
            stats.append(one)
        return ns, hist[: ns.history_len].copy(), stats, lam[: ns.iterations].copy()

    def time_quasi_pass(self, step, method="picard", repeats=20):
        """ms per launch of quasi()'s pass (k_quasi_pass and the reduction of its sums) on the handle's own buffers: step 0
        the first evaluation, 1 a trial with lam = 1 and the current U as de; b goes into the finest R, the coefficients
        into the second set of grids: U, B, the iterate and the operator unchanged; after a quasi()"""
        meth = QUASI_METHODS[method] if isinstance(method, str) else int(method)
        ms = C.c_double()
        self._chk(lib().mgx_time_quasi_pass(self._h, int(step), meth, repeats, C.byref(ms)), "mgx_time_quasi_pass")
        return ms.value

    def newton_steps(self, nsteps, mass, kappa, p=(0.0, 0.0, 1.0), theta=1.0, g=None, solver="solve", lin_tol=1e-8, lin_max_iters=50, restart=4,
                     tol=1e-8, max_newton=20, max_backtracks=8):
        """nsteps theta steps of rho u_t = div(a grad u) - kappa phi(u) + f on the device, from the current U
        (mgx_newton_steps): mass = rho h^2 / (theta dt) and kappa interior n x n grids in stencil units, phi as for newton(),
        g = f / theta (n x n or None) constant over the steps.  Every step forms its explicit part in one pass and runs
        Newton's method from the previous time level with newton()'s options.  Returns (steps_done, list of NewtonStats,
        list of histories of ||G||) of the completed steps; a step whose iteration does not converge is the last one
        (mgx_last_error names it).  U holds the last time level, B the last step's right-hand side."""
        dt = self.level_dtype(self.cfg.finest_level)
        ma, ka = np.ascontiguousarray(mass, dtype=dt), np.ascontiguousarray(kappa, dtype=dt)
        ga = None if g is None else np.ascontiguousarray(g, dtype=dt)
        assert ma.size == ka.size and (ga is None or ga.size == ka.size), "mass, kappa and g must hold n x n values each"
        code = STEP_SOLVERS[solver] if isinstance(solver, str) else int(solver)
        o = NewtonOpts(float(p[0]), float(p[1]), float(p[2]), code, lin_tol, lin_max_iters, restart, tol, max_newton, max_backtracks)
        k = max(int(nsteps), 1)
        cap = max(int(max_newton), 0) + 1
        st = (NewtonStats * k)()
        hist = np.zeros((k, cap), dtype=np.float64)
        done = C.c_int(0)
        self._chk(lib().mgx_newton_steps(self._h, C.byref(o), theta, nsteps, ma.ctypes.data, ka.ctypes.data, None if ga is None else ga.ctypes.data,
                                         ka.size, C.byref(done), st, hist.ctypes.data_as(C.POINTER(C.c_double)), cap), "mgx_newton_steps")
        stats = []
        for j in range(done.value):
            one = NewtonStats()
            C.memmove(C.byref(one), C.byref(st[j]), C.sizeof(NewtonStats))
            stats.append(one)
        return done.value, stats, [hist[j, : stats[j].history_len].copy() for j in range(done.value)]

    def time_newton_step_pass(self, which, theta=0.5, repeats=20):
        """ms per launch of newton_steps()' passes on the handle's own buffers: which = 0 the right-hand-side pass
        (k_newton_step_rhs, theta = 1 its Euler instance), 1 the first evaluation with the mass term, 2 a trial with lam = 1
        (k_newton_pass and the reduction of its sums); into the finest R, the trial iterate and the next d: U, B, the time
        level and the operator unchanged; after a newton_steps()"""
        ms = C.c_double()
        self._chk(lib().mgx_time_newton_step_pass(self._h, int(which), theta, repeats, C.byref(ms)), "mgx_time_newton_step_pass")
        return ms.value

    def get_stencil(self, level, which):
        n = self.n(level)
        a = np.empty((n, n), dtype=self.level_dtype(level))
        self._chk(lib().mgx_get_stencil(self._h, level, which, a.ctypes.data, a.size), "mgx_get_stencil")
        return a

    # -- Galerkin coarse operators (op = OPERATOR_GALERKIN) ------------------------------
    def build_galerkin(self, transfer=None):
        """A_{l-1} = R A_l P below the finest operator (set_stencil / set_coefficient), every level's Jacobi splitting
        and the coarsest operator's dense inverse.  transfer: None / TRANSFER_BILINEAR (P with the weights 1/2, 1/4) or
        TRANSFER_OPERATOR (the operator-dependent P, its weights read off A_l on every level; R = c P^T)"""
        if transfer is None:
            self._chk(lib().mgx_build_galerkin(self._h), "mgx_build_galerkin")
        else:
            self._chk(lib().mgx_build_galerkin_transfer(self._h, int(transfer)), "mgx_build_galerkin_transfer")

    @property
    def transfer(self):
        """TRANSFER_BILINEAR / TRANSFER_OPERATOR: what the Galerkin hierarchy was built with"""
        out = C.c_int()
        self._chk(lib().mgx_get_transfer(self._h, C.byref(out)), "mgx_get_transfer")
        return out.value

    def get_prolongation(self, level, which):
        """weights of P between `level` and level - 1 (TRANSFER_OPERATOR hierarchies): which = 0..7: n, s, w, e, nw,
        ne, sw, se, on the interior of level - 1"""
        n = self.n(level - 1) if level >= 2 else 1
        a = np.empty((n, n), dtype=self.level_dtype(level))
        self._chk(lib().mgx_get_prolongation(self._h, level, which, a.ctypes.data, a.size), "mgx_get_prolongation")
        return a

    def lambda_max(self, level):
        """g_l: the Gershgorin bound of the spectrum of D^-1 A of the level's current operator (mgx_get_lambda_max)"""
        out = C.c_double()
        self._chk(lib().mgx_get_lambda_max(self._h, level, C.byref(out)), "mgx_get_lambda_max")
        return out.value

    def line_factor(self, level, dir, which):
        """a factor of the level's tridiagonal line systems (mgx_get_line_factor): dir 0 x-lines, 1 y-lines; which 0 m
        (reciprocal pivots), 1 g; n x n in the level's working type"""
        n = (1 << level) - 1
        a = np.empty((n, n), dtype=self.level_dtype(level))
        self._chk(lib().mgx_get_line_factor(self._h, level, dir, which, a.ctypes.data, a.size), "mgx_get_line_factor")
        return a

    def line_chunks(self, level):
        """(rows per chunk, chunks) of the y-line kernel's columns on a level (mgx_get_line_chunks)"""
        rows, chunks = C.c_int(), C.c_int()
        self._chk(lib().mgx_get_line_chunks(self._h, level, C.byref(rows), C.byref(chunks)), "mgx_get_line_chunks")
        return rows.value, chunks.value

    def set_cycle(self, cycle):
        """CYCLE_V / CYCLE_W / CYCLE_F: the kind of every cycle the handle runs from here on (vcycle, vcycle_zero, solve,
        fmg, solve_pcg).  W visits every level below the finest twice per visit of the level above, F makes the second
        visit a V-cycle; the coarsest level is visited once per descent.  STENCIL5 and GALERKIN handles only"""
        self._chk(lib().mgx_set_cycle(self._h, int(cycle)), "mgx_set_cycle")

    @property
    def cycle(self):
        out = C.c_int()
        self._chk(lib().mgx_get_cycle(self._h, C.byref(out)), "mgx_get_cycle")
        return out.value

    def get_stencil9(self, level, which):
        """which = 0..8: c, n, s, w, e, nw, ne, sw, se;  9: D_inv;  10..17: the off-diagonals of R_omega (n .. se)"""
        n = self.n(level)
        a = np.empty((n, n), dtype=self.level_dtype(level))
        self._chk(lib().mgx_get_stencil9(self._h, level, which, a.ctypes.data, a.size), "mgx_get_stencil9")
        return a

    def fill_rhs(self, kind=0, f=4.0):
        self._chk(lib().mgx_fill_rhs(self._h, kind, f), "mgx_fill_rhs")

    def fill_guess_random(self, seed=12345):
        self._chk(lib().mgx_fill_guess_random(self._h, seed), "mgx_fill_guess_random")

    # -- the reference's operators ------------------------------------------------
    def jacobirelaxation(self, level, v, f, mu):
        """PS:125-147: returns v after `mu` smoother sweeps with right-hand side f."""
        self.set_level(level, VEC_U, v)
        self.set_level(level, VEC_B, f)
        self._chk(lib().mgx_smooth(self._h, level, mu), "mgx_smooth")
        return self.get_level(level, VEC_U)

    def residual(self, level, v, f):
        """PS:604-607."""
        self.set_level(level, VEC_U, v)
        self.set_level(level, VEC_B, f)
        self._chk(lib().mgx_residual(self._h, level), "mgx_residual")
        return self.get_level(level, VEC_R)

    def restriction2d(self, level, vec_h):
        """PS:531-546 applied to a fine vector of `level`; returns the level-1 vector."""
        self.set_level(level, VEC_B, vec_h)
        self._chk(lib().mgx_restrict_rhs(self._h, level), "mgx_restrict_rhs")
        return self.get_level(level - 1, VEC_B)

    def residual_restriction(self, level, v, f):
        """PS:604-611 fused: restriction2d(f - A v)."""
        self.set_level(level, VEC_U, v)
        self.set_level(level, VEC_B, f)
        self._chk(lib().mgx_restrict(self._h, level), "mgx_restrict")
        return self.get_level(level - 1, VEC_B), self.get_level(level - 1, VEC_U)

    def interpolation2d(self, level, vec_2h):
        """PS:337-425: coarse vector of level-1 -> fine vector of `level`."""
        self.set_level(level - 1, VEC_U, vec_2h)
        self._chk(lib().mgx_prolong(self._h, level), "mgx_prolong")
        return self.get_level(level, VEC_U)

    def interpolation_add(self, level, vec_h, vec_2h):
        """PS:620-624: vec_h + interpolation2d(vec_2h)."""
        self.set_level(level, VEC_U, vec_h)
        self.set_level(level - 1, VEC_U, vec_2h)
        self._chk(lib().mgx_prolong_add(self._h, level), "mgx_prolong_add")
        return self.get_level(level, VEC_U)

    def bottom_solve(self, f):
        """MF:63-72 / MF:137-139 on the coarsest level."""
        lo = self.cfg.coarsest_level
        self.set_level(lo, VEC_B, f)
        self._chk(lib().mgx_bottom_solve(self._h), "mgx_bottom_solve")
        return self.get_level(lo, VEC_U)

    def vcyclemultigrid(self, level, vec_h, f_h):
        """PS:575-627."""
        self.set_level(level, VEC_U, vec_h)
        self.set_level(level, VEC_B, f_h)
        self._chk(lib().mgx_vcycle(self._h, level), "mgx_vcycle")
        return self.get_level(level, VEC_U)

    def fullmultigrid(self, f_h):
        """PS:629-650 on the finest level."""
        L = self.cfg.finest_level
        self.set_level(L, VEC_B, f_h)
        self._chk(lib().mgx_fmg(self._h), "mgx_fmg")
        return self.get_level(L, VEC_U)

    def residual_norm(self, level=None):
        out = C.c_double()
        lvl = self.cfg.finest_level if level is None else level
        self._chk(lib().mgx_residual_norm(self._h, lvl, C.byref(out)), "mgx_residual_norm")
        return out.value

    def vcycle(self, level=None):
        self._chk(lib().mgx_vcycle(self._h, self.cfg.finest_level if level is None else level), "mgx_vcycle")

    def vcycle_zero(self):
        """one V-cycle from the finest level for A e = b, starting from e = 0"""
        self._chk(lib().mgx_vcycle_zero(self._h), "mgx_vcycle_zero")

    def smooth(self, level, mu):
        self._chk(lib().mgx_smooth(self._h, level, mu), "mgx_smooth")

    def solve(self, tol=1e-8, max_cycles=50):
        """PS:727 run to a tolerance; returns (stats, residual history)."""
        st = Stats()
        hist = np.zeros(max_cycles + 1, dtype=np.float64)
        self._chk(lib().mgx_solve(self._h, tol, max_cycles, C.byref(st), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                  hist.size), "mgx_solve")
        return st, hist[: st.history_len].copy()

    def solve_pcg(self, tol=1e-8, max_iters=100):
        """conjugate gradients preconditioned by one V-cycle from zero per iteration, from the current
        guess; returns (stats, residual history) as solve() does (stats.cycles = iterations)."""
        st = Stats()
        hist = np.zeros(max_iters + 1, dtype=np.float64)
        self._chk(lib().mgx_solve_pcg(self._h, tol, max_iters, C.byref(st), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                      hist.size), "mgx_solve_pcg")
        return st, hist[: st.history_len].copy()

    def solve_gcr(self, tol=1e-8, max_iters=100, restart=4):
        """restarted GCR (FGMRES(restart) in exact arithmetic) around one cycle from zero per iteration, from the
        current guess: for operators and cycles that are not symmetric, 1 <= restart <= GCR_MAX_RESTART; returns
        (stats, residual history) as solve_pcg() does (stats.cycles = iterations)."""
        st = Stats()
        hist = np.zeros(max(max_iters, 0) + 1, dtype=np.float64)
        self._chk(lib().mgx_solve_gcr(self._h, tol, max_iters, restart, C.byref(st), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                      hist.size), "mgx_solve_gcr")
        return st, hist[: st.history_len].copy()

    def solve_refine(self, tol=1e-8, max_cycles=50):
        """iterative refinement of a general-operator F64 handle: the fp64 residual and iterate around one cycle from
        zero of a float copy of the hierarchy (mgx_solve_refine), from the current guess; returns (stats, history of the
        true fp64 residual norm) as solve() does."""
        st = Stats()
        hist = np.zeros(max(max_cycles, 0) + 1, dtype=np.float64)
        self._chk(lib().mgx_solve_refine(self._h, tol, max_cycles, C.byref(st), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                         hist.size), "mgx_solve_refine")
        return st, hist[: st.history_len].copy()

    def solve_refine_gcr(self, tol=1e-8, max_iters=100, restart=4):
        """solve_gcr's iteration in fp64 around the float cycle of solve_refine (mgx_solve_refine_gcr): general-operator F64
        handles, from the current guess; returns (stats, history of the recursively updated fp64 residual norm) as
        solve_gcr() does (stats.cycles = iterations = float cycles)."""
        st = Stats()
        hist = np.zeros(max(max_iters, 0) + 1, dtype=np.float64)
        self._chk(lib().mgx_solve_refine_gcr(self._h, tol, max_iters, restart, C.byref(st), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                             hist.size), "mgx_solve_refine_gcr")
        return st, hist[: st.history_len].copy()

    def _solve_block(self, name, b, u0, tol, iters, *extra):
        """the block entry point `name` (b, u, tol, iters, *extra, stats, history, cap) on k <= MAX_RHS columns: (list of
        stats, list of residual histories, u of shape (k, n, n))"""
        dt = self.level_dtype(self.cfg.finest_level)
        n = self.n()
        b = np.ascontiguousarray(b, dtype=dt).reshape(-1, n, n)
        k = b.shape[0]
        u = np.zeros_like(b) if u0 is None else np.array(u0, dtype=dt, order="C").reshape(k, n, n)
        st = (Stats * max(k, 1))()
        cap = max(iters, 0) + 1
        hist = np.zeros((max(k, 1), cap), dtype=np.float64)
        self._chk(getattr(lib(), name)(self._h, k, b.ctypes.data, u.ctypes.data, tol, iters, *extra, st,
                                       hist.ctypes.data_as(C.POINTER(C.c_double)), cap), name)
        stats = []
        for j in range(k):
            one = Stats()
            C.memmove(C.byref(one), C.byref(st[j]), C.sizeof(Stats))
            stats.append(one)
        return stats, [hist[j, : stats[j].history_len].copy() for j in range(k)], u

    def solve_multi(self, b, u0=None, tol=1e-8, max_cycles=50):
        """k <= MAX_RHS right-hand sides b[j] (k x n x n) for the handle's operator in one call, every coefficient grid read
        once per pass for the columns still iterating (mgx_solve_multi): general-operator Jacobi handles, F64 or F32.  u0:
        the initial guesses (None: zero).  Returns (list of stats, list of residual histories, u of shape (k, n, n)); column
        j is bit for bit what set_rhs(b[j]); set_guess(u0[j]); solve(tol, max_cycles) returns as a plain cycle loop."""
        return self._solve_block("mgx_solve_multi", b, u0, tol, max_cycles)

    def solve_multi_gcr(self, b, u0=None, tol=1e-8, max_iters=50, restart=4):
        """solve_gcr's iteration on k <= MAX_RHS right-hand sides b[j] (k x n x n) in one call, the cycle and the direction
        pass reading every coefficient grid once for the columns still iterating (mgx_solve_multi_gcr): general-operator
        Jacobi handles, F64 or F32.  u0: the initial guesses (None: zero).  Returns (list of stats, list of residual
        histories, u of shape (k, n, n)) like solve_multi(); column j is bit for bit what set_rhs(b[j]); set_guess(u0[j]);
        solve_gcr(tol, max_iters, restart); get_solution() returns."""
        return self._solve_block("mgx_solve_multi_gcr", b, u0, tol, max_iters, restart)

    def solve_multi_refine_gcr(self, b, u0=None, tol=1e-8, max_iters=50, restart=4):
        """solve_refine_gcr's iteration on k <= MAX_RHS right-hand sides b[j] (k x n x n) in one call: fp64 GCR around the
        float block cycle, the cycle and the direction pass reading every coefficient grid once for the columns still
        iterating (mgx_solve_multi_refine_gcr): general-operator Jacobi F64 handles.  u0: the initial guesses (None: zero).
        Returns (list of stats, list of residual histories, u of shape (k, n, n)) like solve_multi_gcr(); column j is bit for
        bit what set_rhs(b[j]); set_guess(u0[j]); solve_refine_gcr(tol, max_iters, restart); get_solution() returns."""
        return self._solve_block("mgx_solve_multi_refine_gcr", b, u0, tol, max_iters, restart)

    # -- measurement -----------------------------------------------------------------
    def eigs(self, nev, x0=None, tol=1e-8, max_iters=100, seed=0):
        """the nev <= MAX_RHS smallest eigenpairs of the finest-level operator (as stored: no h^-2) by LOBPCG around the block
        cycle (mgx_eigs): general-operator Jacobi handles, F64 or F32, a symmetric positive definite operator.  x0: the
        guesses (nev x n x n); None: uniform(-1, 1) vectors of numpy's default_rng(seed).  Returns (theta, X, stats,
        history): theta ascending, X of shape (nev, n, n) with unit 2-norm, a list of stats (cycles = preconditioner cycles
        of the column) and a list of histories of ||A x_j - theta_j x_j||."""
        return self._eigs("mgx_eigs", nev, x0, tol, max_iters, seed)

    def eigs_many(self, nev, x0=None, tol=1e-8, max_iters=100, seed=0):
        """the nev <= EIGS_MAX smallest eigenpairs: eigs()' iteration on blocks of at most MAX_RHS columns, each block in the
        complement of the pairs found before it (mgx_eigs_many).  Arguments and return value as eigs(); max_iters is the
        budget of each block.  A block that does not converge ends the call: the pairs of the later blocks come back as the
        guesses with theta = 0 and empty histories, behind the computed ones, and mgx_last_error names the block.  nev <=
        MAX_RHS returns what eigs() returns, bit for bit."""
        return self._eigs("mgx_eigs_many", nev, x0, tol, max_iters, seed)

    def _eigs(self, fn, nev, x0, tol, max_iters, seed):
        dt = self.level_dtype(self.cfg.finest_level)
        n = self.n()
        if x0 is None:
            x = np.random.default_rng(seed).uniform(-1.0, 1.0, (max(nev, 1), n, n)).astype(dt)
        else:
            x = np.array(x0, dtype=dt, order="C").reshape(-1, n, n)
            assert x.shape[0] == nev, "x0 must hold nev vectors"
        theta = np.zeros(max(nev, 1), dtype=np.float64)
        st = (Stats * max(nev, 1))()
        cap = max(max_iters, 0) + 1
        hist = np.zeros((max(nev, 1), cap), dtype=np.float64)
        self._chk(getattr(lib(), fn)(self._h, nev, x.ctypes.data, theta.ctypes.data_as(C.POINTER(C.c_double)), tol, max_iters, st,
                                     hist.ctypes.data_as(C.POINTER(C.c_double)), cap), fn)
        stats = []
        for j in range(nev):
            one = Stats()
            C.memmove(C.byref(one), C.byref(st[j]), C.sizeof(Stats))
            stats.append(one)
        return theta[:nev], x, stats, [hist[j, : stats[j].history_len].copy() for j in range(nev)]

    def time_eig_pass(self, which, nev, repeats=20):
        """ms per launch of pass `which` (EIG_PASS_GRAM / COMBINE / RESIDUAL / APPLY) of eigs() on its first nev workspace
        columns; after an eigs() with at least nev columns"""
        ms = C.c_double(0.0)
        self._chk(lib().mgx_time_eig_pass(self._h, which, nev, repeats, C.byref(ms)), "mgx_time_eig_pass")
        return ms.value

    def time_eig_project(self, which, m, k, repeats=20):
        """ms per launch of pass `which` (EIG_PROJECT_DOTS / EIG_PROJECT_SUB) of eigs_many()'s projection of the first k
        workspace columns against the first m locked vectors; after an eigs_many() with nev >= m + k"""
        ms = C.c_double(0.0)
        self._chk(lib().mgx_time_eig_project(self._h, which, m, k, repeats, C.byref(ms)), "mgx_time_eig_project")
        return ms.value

    def profile_reset(self):
        self._chk(lib().mgx_profile_reset(self._h), "mgx_profile_reset")

    def profile(self):
        p = Profile()
        self._chk(lib().mgx_profile_get(self._h, C.byref(p)), "mgx_profile_get")
        return {"ms": list(p.ms), "launches": list(p.launches), "sweeps": list(p.sweeps)}

    def time_smoother(self, sweeps):
        ms = C.c_double()
        self._chk(lib().mgx_time_smoother(self._h, sweeps, C.byref(ms)), "mgx_time_smoother")
        return ms.value

    def time_gcr_pass(self, which, j, repeats=20):
        """ms per launch of one pass of solve_gcr at basis slot j: which = 0 k_pcg_update, 1 k_gcr_dots<j>, 2 k_gcr_orth<j>,
        3 k_pcg_direction; after a solve_gcr with restart > j"""
        ms = C.c_double()
        self._chk(lib().mgx_time_gcr_pass(self._h, which, j, repeats, C.byref(ms)), "mgx_time_gcr_pass")
        return ms.value

    def time_refine_pass(self, repeats=20):
        """ms per launch of solve_refine's fp64 update + residual pass (k_refine_pass) on the handle's own buffers, U and B
        unchanged; after a solve_refine"""
        ms = C.c_double()
        self._chk(lib().mgx_time_refine_pass(self._h, repeats, C.byref(ms)), "mgx_time_refine_pass")
        return ms.value

    def time_refine_gcr_pass(self, which, repeats=20):
        """ms per launch of one mixed pass of solve_refine_gcr: which = 0 k_refine_update, 1 k_refine_direction; U and B
        unchanged; after a solve_refine_gcr"""
        ms = C.c_double()
        self._chk(lib().mgx_time_refine_gcr_pass(self._h, which, repeats, C.byref(ms)), "mgx_time_refine_gcr_pass")
        return ms.value

    def time_multi_smoother(self, nrhs, sweeps):
        """ms of `sweeps` finest-level Jacobi sweeps on the first nrhs workspace columns of solve_multi (k_jacobi_var<T, NQ, nrhs>;
        nrhs = 1 is the yardstick); after a solve_multi with at least nrhs columns"""
        ms = C.c_double()
        self._chk(lib().mgx_time_multi_smoother(self._h, nrhs, sweeps, C.byref(ms)), "mgx_time_multi_smoother")
        return ms.value

    def time_multi_gcr_direction(self, nrhs, repeats=20):
        """ms per launch of solve_multi_gcr's direction pass on the first nrhs workspace columns (nrhs = 1: k_pcg_direction,
        the yardstick); after a solve_multi_gcr with at least nrhs columns"""
        ms = C.c_double()
        self._chk(lib().mgx_time_multi_gcr_direction(self._h, nrhs, repeats, C.byref(ms)), "mgx_time_multi_gcr_direction")
        return ms.value

    def time_multi_refine_direction(self, nrhs, repeats=20):
        """ms per launch of solve_multi_refine_gcr's direction pass on the first nrhs workspace columns (k_refine_direction<NQ,
        nrhs>; nrhs = 1 is the yardstick); after a solve_multi_refine_gcr with at least nrhs columns"""
        ms = C.c_double()
        self._chk(lib().mgx_time_multi_refine_direction(self._h, nrhs, repeats, C.byref(ms)), "mgx_time_multi_refine_direction")
        return ms.value

    def graphs_cached(self):
        """hipGraphs captured by solve() for its loop body (-1: graph replay off)"""
        return lib().mgx_graphs_cached(self._h)

    def synchronize(self):
        self._chk(lib().mgx_synchronize(self._h), "mgx_synchronize")
