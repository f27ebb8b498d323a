"""mgx — MI355X-native geometric multigrid for the 2-D Poisson problem.

Drop-in for the hot path of nikhilTkur/Multigrid_Nikhil_C- (smoother, residual,
restriction, prolongation, V-cycle / FMG schedules).  The product
is libmgx.so (C-ABI: include/mgx.h) built from csrc/; this package is the thin
ctypes view of it plus the multi-GPU slab driver.  The directory name carries
the reference's name, so import it through __graft_entry__.load_package()
(registered as `multigrid_nikhil_c_amd`).
"""
from .binding import (  # noqa: F401
    ARITH_FMA, ARITH_SEPARATE, BOTTOM_EXACT, BOTTOM_SMOOTH, CYCLE_F, CYCLE_V, CYCLE_W,
    DTYPE_F32, DTYPE_F64, DTYPE_MIXED, EIG_PASS_APPLY, EIG_PASS_COMBINE, EIG_PASS_GRAM, EIG_PASS_RESIDUAL, EIG_PROJECT_DOTS, EIG_PROJECT_SUB, EIGS_MAX, EXPORTS, GCR_MAX_RESTART, LIB_PATH, MAX_RHS,
    OP_GALERKIN, OPERATOR_GALERKIN, OPERATOR_POISSON, OPERATOR_STENCIL5, RESTRICT_CONSISTENT, RESTRICT_FW16, RESTRICT_INJECT, RESTRICT_INJECT4, SCHEDULE_FMG, SCHEDULE_V, SMOOTHER_CHEBYSHEV, SMOOTHER_COLOR_GS, SMOOTHER_COLOR_SGS, SMOOTHER_JACOBI, SMOOTHER_LINE_ALT, SMOOTHER_LINE_X, SMOOTHER_LINE_Y,
    QUASI_METHODS, QUASI_NEWTON, QUASI_PICARD, SMOOTHER_RBGS, STEP_GCR, STEP_REFINE_GCR, STEP_SOLVE, STEP_SOLVERS, TRANSFER_BILINEAR, TRANSFER_OPERATOR, VEC_B, VEC_R, VEC_U, Config, DistLevel, DistOp, MgxError, Multigrid, Plan, Slab, Stats, Transport, Xfer,
    default_config, lib, rccl_unique_id, runtime_libs,
)
