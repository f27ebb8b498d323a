/*
 * mgx.h — C-ABI of libmgx: MI355X-native geometric multigrid for the 2-D
 * Poisson problem, the drop-in for the hot path of nikhilTkur/Multigrid_Nikhil_C-.
 *
 * The reference exposes no FFI: its interface is a set of C++ free functions
 * in one translation unit called from main().  Each entry point
 * below names the reference function or block it replaces
 * (PS = Poissons_SYCL.cpp, MF = Multigrid_functions.cpp).  A header-only C++
 * wrapper with the reference's own names and std::vector signatures is in
 * include/mgx_reference_api.hpp; INTEGRATION.md shows the binding a maintainer
 * would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types, never throws.
 *   - every function returns an mgx_status (0 = ok); mgx_last_error() gives text.
 *   - host vectors use the reference's layout: interior-only, row-major,
 *     n x n with n = 2^L - 1 (PS:227-233, PS:291, PS:662-664); element type is
 *     double for dtype F64 and MIXED, float for dtype F32.
 *   - device memory is owned by the handle; one host thread per handle; calls
 *     block until the result is available unless the name ends in _async.
 *   - there is no CPU fallback: creation fails with MGX_ERR_NO_DEVICE when no
 *     gfx950 device is usable.
 */
#ifndef MGX_H
#define MGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_API __attribute__((visibility("default")))

typedef enum {
    MGX_OK = 0,
    MGX_ERR_INVALID = 1,      /* bad argument / configuration */
    MGX_ERR_NO_DEVICE = 2,    /* no usable HIP device */
    MGX_ERR_HIP = 3,          /* a HIP runtime call failed */
    MGX_ERR_ALLOC = 4,
    MGX_ERR_STATE = 5         /* call not valid in the handle's current state */
} mgx_status;

enum { MGX_SMOOTHER_JACOBI = 0, MGX_SMOOTHER_RBGS = 1,
       /* CHEBYSHEV: a Chebyshev polynomial in omega D^-1 A on the interval [lmax / 4, lmax], lmax = omega g_l with g_l the
        * Gershgorin bound of the level's D^-1 A (mgx_get_lambda_max); csrc/mgx_cheby.hpp states the iteration.  mu1 / mu2
        * (and the mu of mgx_smooth, the sweeps of mgx_time_smoother) are then the DEGREES of the pre- / post-smoothing
        * blocks: a block of degree k is k launches and damps [lmax / 4, lmax] by 1 / T_k(5/3) (0.22, 0.074, 0.025 for
        * k = 2, 3, 4 against (2/3)^k of Jacobi with omega = 2/3); every block starts afresh; degree 0 is no smoothing.
        * The iterates do not depend on omega beyond rounding.  Handles with op = MGX_OPERATOR_STENCIL5 or
        * MGX_OPERATOR_GALERKIN only, dtype F64 or F32, arith SEPARATE, one GPU; with op = MGX_OPERATOR_POISSON, in
        * mgx_create_rank, mgx_plan_create and mgx_slab_cycle it is MGX_ERR_INVALID.  One more array per level (the
        * direction d) and 10 / 14 sizeof(T) per point and step on five- / nine-point levels (Jacobi: 8 / 12). */
       MGX_SMOOTHER_CHEBYSHEV = 2,
       /* LINE_X / LINE_Y / LINE_ALT: zebra line Gauss-Seidel (csrc/mgx_line.hpp states the sweep).  An x-line sweep solves
        * the tridiagonal system of every grid row exactly - the odd grid rows first, then the even ones, which read the rows
        * just written - with the off-line terms on the right-hand side; a y-line sweep does the same down the columns; an
        * alternating sweep is an x-sweep followed by a y-sweep.  The smoother for anisotropic operators (strong coupling
        * along x, along y, or either in different parts of the grid), where point smoothers do not converge.  No damping:
        * omega is validated but not used.  mu1 / mu2 (the mu of mgx_smooth, the sweeps of mgx_time_smoother) count
        * sweeps; a sweep is two launches per direction and updates the iterate in place; mgx_stats.fine_updates counts
        * one update per point and x- or y-sweep (an alternating sweep: two).  The tridiagonal factors are built with the
        * operator (mgx_get_line_factor); a zero or non-finite pivot makes mgx_set_stencil / mgx_set_coefficient / the
        * Galerkin builds return MGX_ERR_INVALID.  Handles with op = MGX_OPERATOR_STENCIL5 or MGX_OPERATOR_GALERKIN only,
        * dtype F64 or F32, arith SEPARATE, one GPU; with op = MGX_OPERATOR_POISSON, in mgx_create_rank, mgx_plan_create and
        * mgx_slab_cycle they are MGX_ERR_INVALID.  Two more arrays per level and direction; 11 / 15 sizeof(T) per point
        * and sweep direction on five- / nine-point levels (15 / 19 for y-lines on levels cut into chunks).
        * (The value 3 stays an invalid smoother: mgx_create has always refused it and the suite pins that.) */
       MGX_SMOOTHER_LINE_X = 4, MGX_SMOOTHER_LINE_Y = 5, MGX_SMOOTHER_LINE_ALT = 6,
       /* COLOR_GS / COLOR_SGS: multicolour point Gauss-Seidel (csrc/mgx_colour.hpp states the sweep).  A sweep updates the
        * colours of a level one after the other, every point x_ij = (b_ij - S_ij) * D_inv_ij from the current state of
        * its neighbours: S the sum of the off-diagonal terms a_k u_k of A in CSR order (NW, N, NE, W, E, SW, S, SE;
        * five-point levels N, W, E, S), the first term starting the accumulator, every product and sum rounded on its
        * own; D_inv the level's stored 1 / c (mgx_get_stencil which 5, mgx_get_stencil9 which 9).  Five-point levels have
        * two colours: (grid row + grid column) even first, then odd.  Nine-point levels have four, by (row parity, column
        * parity): (odd, odd), (odd, even), (even, odd), (even, even) - the coarse points last.  Coefficients that point
        * at the Dirichlet ring multiply the ring of the iterate, which is zero.  A reverse sweep takes the colours in the
        * opposite order.  COLOR_GS: every block sweeps forward.  COLOR_SGS: the blocks before a restriction, mgx_smooth,
        * mgx_time_smoother and the first mu1 sweeps of a bottom = SMOOTH visit sweep forward, the blocks after a
        * correction and the last mu2 sweeps of a bottom = SMOOTH visit in reverse (in W- and F-cycles each block by its
        * position: before the descent or after the ascent) - with mu1 = mu2 that cycle is a symmetric preconditioner
        * for mgx_solve_pcg, which the forward-only one is not.  mu1 / mu2 (the mu of mgx_smooth) count sweeps; omega
        * is validated but not used; mgx_stats.fine_updates counts one update per point and sweep.  A five-point level of
        * N >= 16 sweeps both colours in one launch, out of place like a Jacobi pass (8 sizeof(T) per point; with
        * MGX_GS_FUSED=0 in the environment at mgx_create: one launch per colour, in place, as on nine-point and smaller
        * levels) - the same bits either way.  Nothing is allocated beyond what a Jacobi handle has.  Handles with op =
        * MGX_OPERATOR_STENCIL5 or MGX_OPERATOR_GALERKIN only, dtype F64 or F32, arith SEPARATE, one GPU; with op =
        * MGX_OPERATOR_POISSON (which has RBGS), in mgx_create_rank, mgx_plan_create and mgx_slab_cycle they are
        * MGX_ERR_INVALID.  (The value 1, RBGS, stays refused on general-operator handles.  The value 7 stays an invalid smoother, like 3:
        * mgx_create has always refused it and the suite pins that.) */
       MGX_SMOOTHER_COLOR_GS = 8, MGX_SMOOTHER_COLOR_SGS = 9 };
enum { MGX_DTYPE_F32 = 0, MGX_DTYPE_F64 = 1, MGX_DTYPE_MIXED = 2 };
enum { MGX_SCHEDULE_V = 0, MGX_SCHEDULE_FMG = 1 };
enum { MGX_RESTRICT_CONSISTENT = 0, MGX_RESTRICT_FW16 = 1,
       MGX_RESTRICT_INJECT = 2,    /* MF:122-130 restriction2D as written: the fine value at the coincident node */
       MGX_RESTRICT_INJECT4 = 3 }; /* 4 x injection: the h^2-consistent weight for operators that carry no h^-2 (cf. D4) */
/* Operator of the hierarchy.  POISSON: the constant five-point stencil of PS (matrix-free, fused kernels).
 * STENCIL5: the data model of the reference's second draft (MF:16-41 ProblemVar) on the structured grid - one
 * general five-point operator PER LEVEL (A_sp_dict[level]) given by the caller as five coefficient grids
 * (mgx_set_stencil) or re-discretised from a nodal coefficient a(x, y) of -div(a grad u) (mgx_set_coefficient),
 * smoothed in MF's form  v <- R_omega v + omega D^-1 b  (MF:86-93), residual b - A v (MF:150-153), direct solve of
 * the coarsest operator (MF:63-72: dense inverse; coarsest_level <= 5).  dtype F64 / F32, Jacobi, Chebyshev, a line smoother or multicolour Gauss-Seidel, one GPU.
 * Algorithmic bytes per point and sweep: 8 sizeof(T) (v, b, D_inv, four R arrays in; v' out). */
enum { MGX_OPERATOR_POISSON = 0, MGX_OPERATOR_STENCIL5 = 1,
       /* GALERKIN: the variational hierarchy.  The finest level is a general five-point operator given as for STENCIL5,
        * or a general NINE-point operator (mgx_set_stencil9, mgx_set_tensor: mixed derivatives, rotated anisotropy, Q1
        * stiffness matrices, compact fourth-order stencils); every coarser level is the NINE-point operator
        * A_{l-1} = R A_l P built on the device by mgx_build_galerkin (P: the bilinear prolongation, R: the handle's full
        * weighting; csrc/mgx_galerkin.hpp).  Same restrictions as STENCIL5, and restrict_mode CONSISTENT or FW16 only.
        * Nine-point levels move 12 sizeof(T) per point and sweep (v, b, D_inv, eight R arrays in; v' out); a five-point
        * finest level keeps 8 sizeof(T).
        * (The value 2 stays an invalid operator: mgx_create has always refused it and the suite pins that.) */
       MGX_OPERATOR_GALERKIN = 3 };
enum { MGX_BOTTOM_EXACT = 0, MGX_BOTTOM_SMOOTH = 1 };
/* Arithmetic of the weighted-Jacobi update  v' = (1-w) v + (w/4) b + (w/4)(N+W+E+S)  (PS:138-142):
 *   SEPARATE: the reference's five library calls as five roundings per point, in its order
 *             (t = c0 v + c1 b ; v' = t + c1 nb) - bit-identical to the CPU oracle's default mode;
 *   FMA:      the same expression with its two multiply-adds contracted, v' = fma(c1, nb, fma(c0, v, c1 b)):
 *             what oneMKL's fused kernels would be free to do; two roundings fewer per point, bit-identical
 *             to the oracle's FMA mode and within 1e-10 of the SEPARATE residual histories (north_star's
 *             tolerance; tests/test_gpu_fma.py).  Every other operator (residual, transfers, red-black
 *             Gauss-Seidel, bottom solve) performs the same operations in both modes. */
enum { MGX_ARITH_SEPARATE = 0, MGX_ARITH_FMA = 1 };
#define MGX_MAX_GPUS 16

/* The reference's compile-time globals as run-time fields.
 * PS:17-22 (finest_level, coarsest_level, mu0, mu1, mu2), PS:127 (omega);
 * MF:43-48 holds the draft's values of the same names. */
typedef struct {
    int finest_level;     /* PS:17  */
    int coarsest_level;   /* PS:18; >= 2, and <= 8 with bottom = EXACT (the dense sine-transform
                             solve holds (2^L - 1)^2 matrices: 255^2 at level 8; PS:18 uses 7) */
    int mu0;              /* PS:20  FMG runs mu0+1 V-cycles per level (PS:646) */
    int mu1;              /* PS:21  pre-smoothing sweeps  (smoother = CHEBYSHEV: degree of the pre-smoothing block) */
    int mu2;              /* PS:22  post-smoothing sweeps (smoother = CHEBYSHEV: degree of the post-smoothing block) */
    double omega;         /* PS:127 Jacobi weight */
    int smoother;         /* MGX_SMOOTHER_*  (RBGS: BASELINE config 3) */
    int dtype;            /* MGX_DTYPE_*     (PS is f32, MF is f64; MIXED: config 5) */
    int schedule;         /* MGX_SCHEDULE_*  (PS:727 calls fullmultigrid = FMG) */
    int restrict_mode;    /* MGX_RESTRICT_*   */
    int bottom;           /* MGX_BOTTOM_*    (EXACT: MF:137-139; SMOOTH: PS:581-587, D8) */
    int device;           /* HIP device ordinal (n_gpus <= 1) */
    int profile;          /* 1: HIP events around each operator class, every launch eager (no graph replay);
                             2: events around the finest level's passes, launched one by one, and around ONE
                                graph replay of everything below it (what bench.py times: mgx_solve's own
                                execution, less the two kernel boundaries a whole-cycle graph saves) */
    /* ---- multi-GPU (the reference has one sycl::queue, PS:659) -------------
     * n_gpus > 1: the levels above cut_level are split into n_gpus row slabs, slab g on device
     * devices[g]; one stream pair per slab, halo rows moved device to device between the
     * smoothing blocks (hipMemcpyPeerAsync inside one process, RCCL send/recv between the
     * processes of mgx_create_rank), levels <= cut_level solved redundantly per device
     * ("the bottom solve stays on one GPU").  Several slabs may share a device (devices[g] all 0
     * runs the whole slab plan on one GPU: how the 1-GPU tests check n_gpus = 2, 4, 8 bit for bit
     * against n_gpus = 1).  Multi-GPU handles: dtype F64 or F32, both schedules. */
    int n_gpus;           /* 0 or 1: single GPU */
    int cut_level;        /* 0: chosen from the grid and n_gpus */
    int devices[MGX_MAX_GPUS];   /* -1 entries: slab g on device g modulo the device count */
    int arith;            /* MGX_ARITH_*     (PS:138-142: how the Jacobi update is rounded) */
    int op;               /* MGX_OPERATOR_*  (MF:16-41: per-level general operators) */
} mgx_config;

typedef struct mgx_solver* mgx_handle;

/* Fills the reference's defaults (PS:17-22, 127): levels 10..7, mu 30/10/10,
 * omega 2/3, Jacobi, FMG; dtype F64, consistent restriction, exact bottom. */
MGX_API int mgx_config_default(mgx_config* cfg);

/* Grid-hierarchy constructor: replaces the per-level loop of main()
 * (PS:661-690: globalstiffenssmatrix + coo_to_csr + init_matrix_handle +
 * set_csr_data filling jacobi_matrices[level - coarsest_level], PS:33).
 * Matrix-free: allocates per-level device arrays instead of CSR handles. */
MGX_API int mgx_create(const mgx_config* cfg, mgx_handle* out);
MGX_API int mgx_destroy(mgx_handle h);
MGX_API const char* mgx_last_error(mgx_handle h);   /* h may be NULL: last create error */
MGX_API const char* mgx_status_string(int status);

/* Interior points per side at `level`, n = 2^level - 1 (PS:662-664). */
MGX_API int mgx_level_n(int level);

/* ---- data in / out (host buffers, reference layout) ---------------------- */
/* which: vector selector for level-wise access */
enum { MGX_VEC_U = 0, MGX_VEC_B = 1, MGX_VEC_R = 2 };

/* Right-hand side of the finest level: replaces globalforcefunction()'s
 * output handed to fullmultigrid (PS:725-727).  count must be n*n. */
MGX_API int mgx_set_rhs(mgx_handle h, const void* b, size_t count);
/* Right-hand side with non-homogeneous Dirichlet data folded in (the general
 * input path of SURVEY §8f: the reference hard-wires u = 0 on the boundary by
 * eliminating the boundary nodes, PS:188-198, 224).  `ring` holds the boundary
 * node values g in the order: row 0 (columns 0..N), row N (columns 0..N),
 * column 0 (rows 1..N-1), column N (rows 1..N-1); ring_count = 4 N, N = n + 1.
 * Because every off-diagonal of A is -1, eliminating a boundary neighbour moves
 * +g to the right-hand side: b_ij += sum of its boundary neighbours' g.  The
 * solve then returns the interior of the solution of  A u = b,  u = g on the ring. */
MGX_API int mgx_set_rhs_dirichlet(mgx_handle h, const void* b, size_t count, const void* ring, size_t ring_count);
/* Initial guess / result of the finest level (PS:630 starts from zero). */
MGX_API int mgx_set_guess(mgx_handle h, const void* u, size_t count);
MGX_API int mgx_get_solution(mgx_handle h, void* u, size_t count);
/* Level-wise access for operator tests.  Element type: the level's working
 * type (float for F32; double for F64; for MIXED the finest-level U/B/R are
 * double and everything else float). */
MGX_API int mgx_set_level(mgx_handle h, int level, int which, const void* src, size_t count);
MGX_API int mgx_get_level(mgx_handle h, int level, int which, void* dst, size_t count);
/* Device-resident variants (inputs already in HBM): `grid` is a device pointer
 * to a whole level in the library's own layout, rows 0..N times
 * mgx_level_pitch(level, dtype) elements, Dirichlet ring and padding zero.
 * Device-to-device copies on the handle's stream; block until done. */
MGX_API int mgx_set_level_device(mgx_handle h, int level, int which, const void* grid);
MGX_API int mgx_get_level_device(mgx_handle h, int level, int which, void* grid);
/* zero a level vector (PS:613 / PS:630 initial guesses) */
MGX_API int mgx_zero_level(mgx_handle h, int level, int which);
/* Built-in right-hand sides, generated on the device:
 * kind 0: b = f h^2, the reference's load vector (PS:283-335, f = 4 at PS:123)
 * kind 1: b = h^2 8 pi^2 sin(2 pi x) sin(2 pi y)   (`f` ignored). */
MGX_API int mgx_fill_rhs(mgx_handle h, int kind, double f);
/* u ~ U(-1,1) from a counter-based generator keyed on (seed, index). */
MGX_API int mgx_fill_guess_random(mgx_handle h, uint64_t seed);

/* ---- general per-level operators: ProblemVar (MF:16-41), handles with op = MGX_OPERATOR_STENCIL5 -----------
 * A_sp_dict[level] (MF:19; csr_matrix_elements MF:33-41) as five coefficient grids in the host layout of every
 * vector (interior n x n, row-major, element type = the handle's working type):
 *     (A u)_ij = c u_ij + n u_(i-1)j + s u_(i+1)j + w u_i(j-1) + e u_i(j+1)
 * (coefficients that point at the eliminated Dirichlet ring are ignored, PS:188-198).  The call also builds
 * A_jacobi_sp_dict[level] = {D_inv, R_omega = I - omega D^-1 A} (MF:20, 28-32) and, on the coarsest level, the
 * direct solver of coarsest_level_matrix (MF:18, 63-72).  Every level must be given before a schedule runs
 * (MGX_ERR_STATE otherwise): as in MF, coarse operators are the caller's (the Python front-end of MF:1-3). */
MGX_API int mgx_set_stencil(mgx_handle h, int level, const void* c, const void* n, const void* s, const void* w,
                            const void* e, size_t count);
/* All levels at once from the nodal coefficient a >= a_min > 0 of  -div(a grad u)  on the finest grid's
 * (N + 1)^2 nodes (double, row-major, boundary nodes included): each level samples a at its own nodes and takes
 * face values as the mean of the two nodes (w = -(a_ij + a_i,j-1)/2 ..., c = -(n + s + w + e)): the re-discretised
 * hierarchy of MF:184.  a = 1 gives the Poisson stencil. */
MGX_API int mgx_set_coefficient(mgx_handle h, const double* a_nodes, size_t count);
/* read back: which = 0..4 the operator (c, n, s, w, e), 5..9 its Jacobi splitting (D_inv, R_n, R_s, R_w, R_e) */
MGX_API int mgx_get_stencil(mgx_handle h, int level, int which, void* dst, size_t count);

/* ---- Galerkin coarse operators: handles with op = MGX_OPERATOR_GALERKIN -------------------------------------
 * mgx_set_stencil (finest level only; a coarser level: MGX_ERR_STATE) or mgx_set_coefficient (samples the finest
 * level only) give the finest operator and invalidate the hierarchy; mgx_build_galerkin then builds
 *     A_{l-1} = R A_l P   for l = finest .. coarsest + 1,
 * the Jacobi splitting {D_inv, R_omega} of every level and the dense inverse of the coarsest operator.  R is the
 * handle's restriction: CONSISTENT -> R = P^T (weights 1, 1/2, 1/4), FW16 -> R = P^T / 4; all weights are powers of
 * two, so the two modes give coarse operators that differ by an exact factor 4 per level, and the same iterates.
 * Schedules and operators return MGX_ERR_STATE until it has run.  MGX_ERR_STATE when the finest operator has not
 * been given or the handle's op is not GALERKIN. */
MGX_API int mgx_build_galerkin(mgx_handle h);
/* read back (after mgx_build_galerkin): which = 0..8 the level's operator (c, n, s, w, e, nw, ne, sw, se; the corners
 * are zero on a five-point finest level), 9 = D_inv, 10..17 = the off-diagonals of R_omega in the same order (n .. se).
 * mgx_get_stencil keeps its meaning on a five-point finest level and returns MGX_ERR_STATE for the nine-point levels
 * (a nine-point finest level among them). */
MGX_API int mgx_get_stencil9(mgx_handle h, int level, int which, void* dst, size_t count);

/* ---- nine-point finest operators: handles with op = MGX_OPERATOR_GALERKIN ----------------------------------------
 * The finest operator as nine coefficient grids, in the layout and slot order of mgx_get_stencil9 (interior n x n,
 * row-major, the handle's working type):
 *     (A u)_ij = nw u_(i-1)(j-1) + n u_(i-1)j + ne u_(i-1)(j+1) + w u_i(j-1) + c u_ij + e u_i(j+1)
 *              + sw u_(i+1)(j-1) + s u_(i+1)j + se u_(i+1)(j+1)        (summed in this order, as on every nine-point level).
 * The operator need not be symmetric.  `level` must be the finest (a coarser one: MGX_ERR_STATE, as in mgx_set_stencil);
 * MGX_ERR_STATE on handles whose op is not GALERKIN (STENCIL5 re-discretises every level as a five-point operator,
 * POISSON has no coefficients); MGX_ERR_INVALID for a NULL pointer or count != n * n.  The call invalidates the
 * hierarchy exactly as mgx_set_stencil does (schedules return MGX_ERR_STATE until mgx_build_galerkin[_transfer] has
 * run; cached graphs are dropped) and makes the finest level a nine-point level: every smoother, transfer, cycle and
 * solver (mgx_solve_pcg and mgx_solve_gcr included) then runs the nine-point kernels there, mgx_get_stencil9 returns
 * its nine grids, D_inv and the eight off-diagonals of R_omega, and mgx_get_stencil returns MGX_ERR_STATE on it.  In
 * W- and F-cycles the finest level always keeps the per-level launches, whatever its size.
 * A later mgx_set_stencil or mgx_set_coefficient makes the finest level five-point again; the handle then computes
 * the bits of a handle that never saw a nine-point operator.  The first of mgx_set_stencil9 / mgx_set_tensor allocates
 * the finest level's eight corner arrays (before anything else is done: MGX_ERR_ALLOC leaves the previous operator
 * and hierarchy usable); they are kept, unread on a five-point level, until mgx_destroy.
 * Coefficients that point at the eliminated Dirichlet ring (n on the first row, nw on the first row and the first
 * column, ...) are ignored: every result is that of the same operator with zeros there.  They are STORED AS GIVEN, as
 * mgx_set_stencil stores them: mgx_get_stencil9 returns the caller's values in those places of the finest operator
 * (and the R_omega entries computed from them); the coarse operators hold zeros there. */
MGX_API int mgx_set_stencil9(mgx_handle h, int level, const void* c, const void* n, const void* s, const void* w, const void* e,
                             const void* nw, const void* ne, const void* sw, const void* se, size_t count);
/* The finest operator of the full-tensor diffusion problem
 *     - d_x(axx d_x u) - d_y(ayy d_y u) - d_x(axy d_y u) - d_y(axy d_x u)
 * from the nodal values of axx, axy, ayy on the finest grid's (N + 1)^2 nodes (double, row-major, boundary nodes
 * included, as for mgx_set_coefficient; x runs along a row, y grows with the row index), discretised on the device
 * (k_var_from_tensor), all arithmetic in double, each coefficient rounded to the working type once.  At node (r, c),
 * with aN, aS, aW, aE = axy at (r-1, c), (r+1, c), (r, c-1), (r, c+1):
 *     fn = 0.5 (ayy(r,c) + ayy(r-1,c)),  fs = 0.5 (ayy(r,c) + ayy(r+1,c)),
 *     fw = 0.5 (axx(r,c) + axx(r,c-1)),  fe = 0.5 (axx(r,c) + axx(r,c+1)),
 *     c = ((fn + fw) + fe) + fs,   n = -fn,  s = -fs,  w = -fw,  e = -fe      (mgx_set_coefficient's five-point part),
 *     nw = -(0.25 (aW + aN)),  ne = 0.25 (aE + aN),  sw = 0.25 (aW + aS),  se = -(0.25 (aE + aS)).
 * Like mgx_set_coefficient it carries no h^-2.  The four corners of a point sum to zero, so the row sum is that of the
 * five-point part; the assembled operator is symmetric bit for bit (e(i,j) = w(i,j+1), se(i,j) = nw(i+1,j+1),
 * ne(i,j) = sw(i-1,j+1)) and exact on quadratics.  It is a central discretisation of the mixed term: for strong
 * mixed terms it is not an M-matrix (no upwinding).  axy = 0 and axx = ayy = a give mgx_set_coefficient(a)'s operator.
 * State model, errors and ring-pointing coefficients as for mgx_set_stencil9; count != (N + 1)^2: MGX_ERR_INVALID. */
MGX_API int mgx_set_tensor(mgx_handle h, const double* axx, const double* axy, const double* ayy, size_t count);

/* ---- a zero-order term on the finest operator: handles with op = MGX_OPERATOR_GALERKIN (csrc/mgx_theta.hpp) ----------
 * The finest operator becomes S = A0 + diag(d): A0 is what the last of mgx_set_stencil / mgx_set_coefficient /
 * mgx_set_stencil9 / mgx_set_tensor gave, d an interior n x n grid (row-major, the handle's working type).  Like those
 * operators d carries no h^-2: pass kappa h^2 for -div(a grad u) + kappa u, or rho h^2 / (theta dt) for a time step
 * (mgx_theta_steps).  On the device c = c0 + d, one rounding in the working type, into slot 0 of the finest level
 * (k_reaction_shift); the handle keeps the base centre c0 and d as two more finest-level grids, allocated by the first
 * call before anything else is touched (MGX_ERR_ALLOC leaves operator and hierarchy usable) and freed by mgx_destroy.
 * State model: a second call with d2 gives A0 + diag(d2), not an accumulation.  d = NULL while a term is set restores
 * c0 bit for bit - the handle then computes the bits of one that never had a term; d = NULL with none set is MGX_OK and
 * changes nothing (hierarchy and graphs kept; count is not looked at).  A later mgx_set_stencil / mgx_set_stencil9 /
 * mgx_set_coefficient / mgx_set_tensor drops the term: the operator is what that call gave.  A call that changes the
 * operator invalidates the hierarchy exactly as mgx_set_stencil does (schedules return MGX_ERR_STATE until
 * mgx_build_galerkin[_transfer] has run; cached graphs are dropped; the float copy of the refine solvers is rebuilt by
 * their next call).  Nothing else changes: R S P, the splittings, lambda bounds, line factors and the dense bottom inverse
 * come from the build, mgx_get_stencil / mgx_get_stencil9 return the shifted centre in slot 0 (the operator as stored),
 * and every solver, smoother, transfer and cycle runs on S.  Positivity of c0 + d is the caller's duty, as for
 * mgx_set_stencil (the line smoothers report a zero pivot at the build).
 * MGX_ERR_STATE with the reason on POISSON handles, STENCIL5 handles (their caller owns every level's stencil and adds the
 * term there), multi-GPU and rank handles, and before the finest operator is set; MGX_ERR_INVALID for count != n * n or
 * a NULL handle.  mgx_get_reaction reads d back; MGX_ERR_STATE when none is set. */
MGX_API int mgx_set_reaction(mgx_handle h, const void* d, size_t count);
MGX_API int mgx_get_reaction(mgx_handle h, void* dst, size_t count);

/* ---- the prolongation of the Galerkin hierarchy (csrc/mgx_opdep.hpp) ------------------------------------------
 * BILINEAR: the weights 1, 1/2, 1/4 on every level.  OPERATOR: the operator-dependent ("black box", Alcouffe / Dendy)
 * prolongation, its weights read off the stencil (c, n, s, w, e, nw, ne, sw, se) of the fine point they belong to:
 *   a fine point on a coarse row, between two coarse columns: the stencil collapsed in y, den = n + c + s, from the
 *     west coarse point -(nw + w + sw) / den, from the east one -(ne + e + se) / den;
 *   a fine point on a coarse column: the same with x and y exchanged (den = w + c + e);
 *   a cell centre: its row of A solved for the centre value, the four edge neighbours replaced by their own formula
 *     above, e.g. from the north-west coarse point -(nw + n hW + w vN) / c with hW / vN the west / north weights of
 *     its north / west neighbour;
 *   a denominator (den, or c at a centre) that is zero or not finite: that weight is the bilinear one (1/2, 1/4).
 * Coefficients that point at the Dirichlet ring are never read.  For the constant Poisson stencil and its Galerkin
 * coarse operators the weights are exactly 1/2 and 1/4.  The hierarchy keeps eight weight grids per coarse level (two
 * more words per fine point for each transfer); restriction and prolongation of every general-operator level, in
 * every schedule and stand-alone entry point, then use them (R = c P^T, c = 1 for CONSISTENT, 1/4 for FW16).
 * The weight grids are allocated by the first OPERATOR build, kept (unused) through a later BILINEAR build so that
 * switching back allocates nothing, and freed by mgx_destroy. */
enum { MGX_TRANSFER_BILINEAR = 0, MGX_TRANSFER_OPERATOR = 1 };
/* mgx_build_galerkin with a choice of P.  BILINEAR: exactly mgx_build_galerkin (same bits).  OPERATOR: on every
 * level l = finest .. coarsest + 1 first the weights of P_l from A_l, then A_{l-1} = R_l A_l P_l with R_l = c P_l^T.
 * Handles with op = MGX_OPERATOR_GALERKIN only (others: MGX_ERR_STATE); other values of `transfer`: MGX_ERR_INVALID. */
MGX_API int mgx_build_galerkin_transfer(mgx_handle h, int transfer);
/* 0 / 1: what the hierarchy was built with; MGX_ERR_STATE before a build and on a handle whose op is not GALERKIN */
MGX_API int mgx_get_transfer(mgx_handle h, int* transfer);
/* read back the weights of P between `level` (fine) and level - 1: eight grids in the host layout of level - 1
 * (n_c x n_c interior, row-major, the handle's working type), which = 0..7 in the order n, s, w, e, nw, ne, sw, se:
 * the weight with which coarse point (I, J) contributes to fine point (2I + di, 2J + dj).  The coincident weight is 1
 * and is not stored.  MGX_ERR_STATE on a BILINEAR hierarchy or before a build. */
MGX_API int mgx_get_prolongation(mgx_handle h, int level, int which, void* dst, size_t count);

/* ---- the eigenvalue bound of a general-operator level (csrc/mgx_cheby.hpp) --------------------------------------
 * g_l = max over the level's interior points of  1 + sum_x |D_inv a_x|  (x: the four off-diagonals n, s, w, e of a
 * five-point level, the eight n, s, w, e, nw, ne, sw, se of a nine-point one; accumulated in double in that order;
 * coefficients that point at the Dirichlet ring are not counted): the Gershgorin bound of the spectrum of D^-1 A, which
 * the Chebyshev smoother uses as lmax / omega.  Computed on the device whenever the level's operator is (re)built
 * (mgx_set_stencil, mgx_set_coefficient, mgx_build_galerkin, mgx_build_galerkin_transfer), for either smoother.
 * 2 exactly for the constant Poisson stencil.  MGX_ERR_STATE before the level's operator exists (before mgx_set_stencil
 * on a STENCIL5 level, before the build on a GALERKIN handle) and on a handle with op = MGX_OPERATOR_POISSON. */
MGX_API int mgx_get_lambda_max(mgx_handle h, int level, double* out);

/* ---- the tridiagonal factors of a line smoother (csrc/mgx_line.hpp) ----------------------------------------------
 * dir = 0: the x-lines (grid rows, T = tridiag(w, c, e)), 1: the y-lines (grid columns, T = tridiag(n, c, s));
 * which = 0: m, the reciprocal pivots  m_0 = 1 / c_0, m_j = 1 / (c_j - w_j g_{j-1});  1: g_j = e_j m_j (0 at the line's last
 * point).  Host layout of the level (n x n interior, row-major, element (i, j) belongs to grid point (i + 1, j + 1) in
 * either direction), the handle's working type.  Built on the device whenever the level's operator is (re)built.
 * MGX_ERR_STATE before the level's operator exists, on a handle whose smoother has no lines in that direction and on
 * handles without a line smoother. */
MGX_API int mgx_get_line_factor(mgx_handle h, int level, int dir, int which, void* dst, size_t count);
/* how the y-line kernel cuts the columns of `level`: rows per chunk (max(64, ceil((N - 1) / 16)) unless MGX_LINE_CHUNK=<rows>
 * was set when the handle was created; never fewer than ceil((N - 1) / 16)) and the number of chunks, ceil((N - 1) / rows);
 * one chunk: the plain recurrence.  All chunks of a 64-column strip run in one workgroup (at most 16).  MGX_ERR_STATE on
 * handles whose smoother has no y-lines. */
MGX_API int mgx_get_line_chunks(mgx_handle h, int level, int* rows, int* chunks);

/* ---- grid operators (one call = the reference function named) ------------
 * On a dtype MIXED handle the finest level holds double data for the accessors above and a
 * float correction / residual pair for the inner cycle, so the operators and schedules below
 * return MGX_ERR_STATE when asked to act on the finest level (use mgx_solve there, or a F64 /
 * F32 handle); the coarser levels of a MIXED handle are ordinary float levels. */
/* jacobirelaxation(q, a_lu, size, v, f, mu)  PS:125-147 / MF:75-96; with
 * smoother = RBGS: mu red-black Gauss-Seidel sweeps; smoother = CHEBYSHEV: one block of degree mu.  Acts on U,B of `level`. */
MGX_API int mgx_smooth(mgx_handle h, int level, int mu);
/* residual block of vcyclemultigrid  PS:591-608 / MF:145-153:  R = B - A U. */
MGX_API int mgx_residual(mgx_handle h, int level);
/* restriction2d(residual)  PS:531-546, 611:  B[level-1] = R(B[level] - A U[level]),
 * residual fused in; also zeroes U[level-1] (PS:613). */
MGX_API int mgx_restrict(mgx_handle h, int level);
/* restriction2d(f_h)  PS:641: B[level-1] = R(B[level])  (FMG right-hand sides). */
MGX_API int mgx_restrict_rhs(mgx_handle h, int level);
/* interpolation2d + vm::add  PS:620-624:  U[level] += P U[level-1]. */
MGX_API int mgx_prolong_add(mgx_handle h, int level);
/* interpolation2d  PS:337-425, 645:  U[level] = P U[level-1]. */
MGX_API int mgx_prolong(mgx_handle h, int level);
/* coarsest-level solve U = A^-1 B  (MF:63-72 direct_solver, MF:137-139). */
MGX_API int mgx_bottom_solve(mgx_handle h);
/* ||B - A U||_2 on `level` (the report D10 says the reference lacks). */
MGX_API int mgx_residual_norm(mgx_handle h, int level, double* out);

/* ---- schedules ------------------------------------------------------------- */
/* vcyclemultigrid(q, a_h, vec_h, f_h) from `level` down  PS:575-627 / MF:132-173 */
MGX_API int mgx_vcycle(mgx_handle h, int level);
/* fullmultigrid(q, a_h, f_h)  PS:629-650 / MF:175-191 on the finest level. */
MGX_API int mgx_fmg(mgx_handle h);
/* One V-cycle from the finest level for A e = b starting from e = 0 (PS:613, 617: the
 * coarse-grid correction of a caller that owns the finer levels, e.g. the multi-GPU driver).
 * The zero guess is synthesised by the first smoothing pass where possible (nobody writes or
 * reads it), and with profiling off the cycle is replayed from a hipGraph. */
MGX_API int mgx_vcycle_zero(mgx_handle h);

/* ---- cycle index: V-, W- and F-cycles (absent in the reference) ------------------------------------------------
 * The kind of every cycle the handle runs: mgx_vcycle, mgx_vcycle_zero, the loop body of mgx_solve, the inner cycles
 * of mgx_fmg and of an FMG-schedule solve, the preconditioner of mgx_solve_pcg.  From a level l above the coarsest:
 *   V: pre-smooth, restrict; cycle(l - 1); correct, post-smooth                       (PS:575-627; the default)
 *   W: pre-smooth, restrict; cycle(l - 1); if l - 1 > coarsest: cycle(l - 1) again; correct, post-smooth
 *   F: as W, but the second visit of level l - 1 is a V-cycle
 * The second visit starts from the iterate the first one left on level l - 1, with the same right-hand side (it is
 * never a zero guess).  The coarsest level is visited once per descent: with bottom = EXACT a second solve would return
 * the same vector, and with bottom = SMOOTH it is one visit (mu1 + mu2 sweeps) by definition.  The finest level is still
 * smoothed mu1 + mu2 times per cycle (mgx_stats.fine_updates is that of a V-cycle); level l is visited 2^(finest - l)
 * times by a W-cycle.  With MGX_CYCLE_V every entry point computes the bits it computed before this call existed.
 * The setter drops the handle's cached graphs (the next cycle is captured anew).  cfg.profile = 2: the coarse part
 * (one graph replay between two events) is all the visits of level finest - 1.
 * In W- and F-cycles a visit of a nine-point level below the finest with N <= 64 (level <= 6) of a GALERKIN handle with
 * the Jacobi smoother is one launch of one workgroup (csrc/mgx_small.hpp: the iterate in LDS, the coefficients in registers),
 * bit-identical to the per-level launches it replaces; every other level, smoother and operator runs W and F through
 * the per-level launches, and so does everything when the environment holds MGX_SMALL_VISIT=0 at mgx_create.
 * (The one-workgroup visit is Jacobi only: MGX_SMOOTHER_COLOR_GS / COLOR_SGS smooth those levels through their per-level
 * launches like the Chebyshev and line smoothers.)
 * Handles with op = MGX_OPERATOR_STENCIL5 or MGX_OPERATOR_GALERKIN (single GPU, dtype F64 or F32, either smoother);
 * MGX_ERR_STATE on POISSON, MIXED and multi-GPU / rank handles, which run V-cycles only; MGX_ERR_INVALID for a NULL
 * handle or another value.  mgx_get_cycle(NULL, ..) returns MGX_ERR_INVALID and leaves *cycle alone. */
enum { MGX_CYCLE_V = 0, MGX_CYCLE_W = 1, MGX_CYCLE_F = 2 };
MGX_API int mgx_set_cycle(mgx_handle h, int cycle);
MGX_API int mgx_get_cycle(mgx_handle h, int* cycle);

typedef struct {
    int cycles;                 /* cycles run (an FMG pass counts as cycle 1) */
    int converged;              /* 1 if ||r|| <= tol ||r0|| */
    double initial_residual;    /* ||b - A u0||_2 */
    double final_residual;
    double seconds;             /* wall time of the solve, device-synchronised */
    double fine_updates;        /* finest-level smoother point updates performed */
    int history_len;            /* entries written to `history` (cycles + 1) */
} mgx_stats;

/* main()'s call `fullmultigrid(q, jacobi_matrices.back(), f_global)` PS:727 /
 * multigrid_solver(ProblemVar&) MF:193-197, run to a tolerance: cycles until
 * ||r||_2 <= tol ||r0||_2 or max_cycles.  history (may be NULL) receives
 * ||r||_2 before the first cycle and after each one; capacity history_cap. */
MGX_API int mgx_solve(mgx_handle h, double tol, int max_cycles, mgx_stats* stats,
                      double* history, int history_cap);

/* Conjugate gradients on the finest level, preconditioned by one V(mu1, mu2) cycle from zero
 * (mgx_vcycle_zero), run to ||r||_2 <= tol ||r0||_2 or max_iters iterations (absent in the reference).
 * Starts from the current U; B is not modified.  On return U holds the iterate.  stats / history as for
 * mgx_solve: history[0] = ||b - A u0||, then the norm of the (recursively updated) residual after each
 * iteration; stats->cycles = iterations = V-cycles applied.  cfg.schedule is ignored.
 * Flexible PCG (Polak-Ribiere beta: the V-cycle need not be symmetric, e.g. RB-GS or mu1 != mu2); the
 * scalars are doubles computed on the device, dots accumulated in double also for F32 handles; results are
 * deterministic (fixed-order reductions).  A breakdown (p.Ap not a positive finite number) stops the
 * iteration with stats->converged = 0, MGX_OK and the reason in mgx_last_error.
 * Single-GPU handles of dtype F64 or F32, op POISSON or STENCIL5; MGX_ERR_STATE on multi-GPU handles and
 * dtype MIXED (an fp64 CG around the float cycle is a follow-up); MGX_ERR_INVALID for tol < 0 or
 * max_iters < 0. */
MGX_API int mgx_solve_pcg(mgx_handle h, double tol, int max_iters, mgx_stats* stats,
                          double* history, int history_cap);

/* Restarted GCR with right preconditioning (FGMRES(restart) in exact arithmetic) on the finest level, around one
 * cycle from zero (mgx_vcycle_zero: any smoother, cycle kind, transfer and bottom of the handle), run to
 * ||r||_2 <= tol ||r0||_2 or max_iters iterations (absent in the reference).  Neither the operator nor the cycle
 * need be symmetric; the residual norm never increases.  Per iteration k, j = k mod restart (the basis is emptied
 * when j = 0):  z = M r;  q = A z;  h_i = (q.Q_i) / s_i for i < j (classical Gram-Schmidt, all dots from the
 * unmodified q);  q' = ((q - h_0 Q_0) - h_1 Q_1) - ..., z' the same combination of z and Z_i;  s_j = q'.q',
 * rho = r.q', alpha = rho / s_j;  x += alpha z', r -= alpha q';  Z_j = z', Q_j = q'.
 * The contract of mgx_solve_pcg: starts from the current U; on return U holds the iterate (also after a breakdown)
 * and B the caller's b, bit for bit; history[0] = ||b - A u0||, then the norm of the recursively updated residual
 * after each iteration; stats->cycles = iterations = cycles applied; max_iters = 0 writes one history entry.
 * Vectors in the working type, dots accumulated in double, scalars doubles on the device; deterministic
 * (fixed-order reductions, no atomics; graph replay and MGX_GRAPH=0 give the same bits).  A breakdown (q'.q' not a
 * positive finite number) stops the iteration with stats->converged = 0, MGX_OK and the reason in mgx_last_error.
 * The first call allocates 2 restart vectors of the finest level (a later, larger restart adds the difference).
 * Single-GPU handles of dtype F64 or F32, op POISSON, STENCIL5 or GALERKIN; MGX_ERR_STATE on multi-GPU and rank
 * handles, dtype MIXED and before the operators are set / built; MGX_ERR_INVALID for tol not >= 0, max_iters < 0,
 * restart < 1 or restart > MGX_GCR_MAX_RESTART. */
#define MGX_GCR_MAX_RESTART 8
MGX_API int mgx_solve_gcr(mgx_handle h, double tol, int max_iters, int restart, mgx_stats* stats,
                          double* history, int history_cap);

/* Iterative refinement (defect correction) on the finest level of a general-operator handle: residual and iterate in
 * fp64 around one cycle from zero of a FLOAT copy of the hierarchy (absent in the reference; what dtype MIXED is for
 * the Poisson operator), run to ||r||_2 <= tol ||r0||_2 or max_cycles cycles:
 *     u += s_k * M32( (b - A u) / s_k ),   s_k = 2^floor(log2( hist[max(k - 1, 0)] / n )),  n = 2^finest_level - 1,
 * M32 the cycle mgx_vcycle_zero runs on an F32 handle (every smoother, the cycle kind of mgx_set_cycle, either transfer,
 * either bottom, a five- or nine-point finest level), the scaling by a power of two exact.  Per cycle one fp64 pass
 * (k_refine_pass: the update, the residual of the new iterate, its norm and the scaled float residual; 72 B per point
 * on a five-point, 104 B on a nine-point finest level) and the float cycle, at about half the bytes of the fp64 one.
 * The contract of mgx_solve_pcg: starts from the current U; on return U holds the fp64 iterate and B the caller's b,
 * bit for bit; history[0] = ||b - A u0||, then the TRUE fp64 residual norm after each cycle; stats as for mgx_solve,
 * stats->cycles = history_len - 1, fine_updates those of the float cycle; max_cycles = 0 writes one history entry and
 * leaves U alone.  U and B of the levels below the finest are left as they were (the cycle runs in the float copy).
 * cfg.schedule is ignored.  Deterministic (fixed-order reductions, no atomics; graph replay and
 * MGX_GRAPH=0 give the same bits).  The handle's own mgx_solve / mgx_vcycle / mgx_solve_pcg / mgx_solve_gcr compute,
 * before and after a call, the bits of a handle that never refined.
 * The float copy: the first call creates, inside the handle, an F32 solver of the same cfg and knobs on the handle's
 * stream (it does not read the environment again; cfg.profile does not extend to it) - about half the device memory
 * the handle already holds, freed by mgx_destroy.  Its operator is the handle's, rounded once to float on the device:
 * the five coefficient grids of every level (STENCIL5), or the finest level's five or nine grids, the coarse operators
 * then built in float with the handle's transfer (GALERKIN); splittings, lambda bounds, line factors and the dense
 * bottom inverse come from the F32 build - bit for bit what a public F32 handle holds after mgx_set_stencil /
 * mgx_set_stencil9 (and mgx_build_galerkin_transfer) with the float32 of the handle's coefficients.  It is rebuilt by
 * the next call after the handle's operator or hierarchy has changed; mgx_set_cycle reaches it at once.
 * Single-GPU handles of dtype F64, op STENCIL5 or GALERKIN.  MGX_ERR_STATE (reason in mgx_last_error) on POISSON handles
 * (use dtype MIXED), F32 and MIXED handles, multi-GPU and rank handles and before the operators are set / built;
 * MGX_ERR_INVALID for tol not >= 0 or max_cycles < 0; MGX_ERR_ALLOC when the float copy cannot be allocated, and the
 * F32 build's error when its line factors break down in float - the fp64 state stays usable in both cases. */
MGX_API int mgx_solve_refine(mgx_handle h, double tol, int max_cycles, mgx_stats* stats, double* history, int history_cap);

/* mgx_solve_gcr's iteration in fp64 around the FLOAT cycle of mgx_solve_refine: restarted GCR with right preconditioning
 * on the finest level of a general-operator F64 handle, the preconditioner one cycle from zero of the handle's float copy
 * of the hierarchy (the one mgx_solve_refine creates and shares), scaled by mgx_solve_refine's power of two (absent in the
 * reference).  Run to ||r||_2 <= tol ||r0||_2 or max_iters iterations:
 *     r = b - A x;  hist[0] = ||r||;  n = 2^finest_level - 1
 *     iteration k, j = k mod restart (the basis is emptied when j = 0):
 *       s_k = 2^floor(log2( hist[max(k - 1, 0)] / n ))
 *       z = s_k * (double) M32( (float)(r / s_k) );  q = A z          (fp64, the handle's finest operator)
 *       h_i, q', z', s_j = q'.q', rho = r.q', alpha = rho / s_j       (exactly mgx_solve_gcr's passes on double vectors)
 *       x += alpha z';  r -= alpha q';  hist[k + 1] = ||r||;  Z_j = z', Q_j = q'
 * M32 is the cycle mgx_vcycle_zero runs on an F32 handle (any smoother, cycle kind, transfer, bottom, a five- or
 * nine-point finest level); the scaling is exact.  Two passes sit on the precision boundary: k_refine_direction
 * (z from the float correction and q = A z: 60 B per point on a five-point, 92 B on a nine-point finest level) and
 * k_refine_update (mgx_solve_gcr's update plus the scaled float residual of the next cycle: 52 B per point); the
 * orthogonalisation passes and reductions are mgx_solve_gcr's.
 * The contract of mgx_solve_gcr: starts from the current U; on return U holds the fp64 iterate (also after a breakdown)
 * and B the caller's b, bit for bit; history[0] = ||b - A u0||, then the norm of the recursively updated fp64 residual
 * after each iteration; stats->cycles = iterations = float cycles applied, fine_updates those of the float cycle (as for
 * mgx_solve_refine); max_iters = 0 writes one history entry and leaves U alone.  A breakdown (q'.q' not a positive
 * finite number) stops the iteration with stats->converged = 0, MGX_OK and the reason in mgx_last_error.  Deterministic
 * (fixed-order reductions, no atomics; graph replay and MGX_GRAPH=0 give the same bits); one host synchronisation per
 * iteration.  The handle's own mgx_solve / mgx_vcycle / mgx_solve_pcg / mgx_solve_gcr / mgx_solve_refine compute, before
 * and after a call, the bits of a handle that never made it.
 * Memory: the float copy (shared with mgx_solve_refine, rebuilt by the next call after the handle's operator or
 * hierarchy has changed; mgx_set_cycle reaches it at once) and mgx_solve_gcr's workspace, shared with it: x, b and
 * 2 restart fp64 vectors of the finest level.
 * MGX_ERR_STATE exactly where mgx_solve_refine returns it (POISSON, F32 and MIXED handles, multi-GPU and rank handles,
 * before the operators are set / built); MGX_ERR_INVALID for tol not >= 0, max_iters < 0, restart < 1 or
 * restart > MGX_GCR_MAX_RESTART; MGX_ERR_ALLOC, and the F32 build's error from the float copy - the fp64 state stays
 * usable in both cases. */
MGX_API int mgx_solve_refine_gcr(mgx_handle h, double tol, int max_iters, int restart, mgx_stats* stats,
                                 double* history, int history_cap);

/* Up to MGX_MAX_RHS right-hand sides for one operator: solves A u_j = b_j, j < nrhs, on the finest level with the
 * handle's cycle, every coefficient grid read once per pass for all the columns still iterating (a Jacobi sweep moves
 * (NQ + 3 nrhs) sizeof(T) per point instead of nrhs (NQ + 3); the transfer weights and the dense coarsest inverse are
 * read once as well).  b: nrhs host vectors back to back, each n * n in the reference layout and the handle's working
 * type; u: the same shape, the initial guesses on entry, the iterates on return; stats: NULL or nrhs entries;
 * history: NULL or nrhs slots of history_cap doubles, column j from history + j * history_cap.
 * What column j returns - iterate, history, cycles, converged, initial_residual, final_residual, history_len,
 * fine_updates - is bit for bit what mgx_set_rhs(b_j); mgx_set_guess(u_j); mgx_solve(h, tol, max_cycles, ..) returns
 * on the same handle as a plain cycle loop: cfg.schedule is ignored (as in mgx_solve_pcg; no FMG).  A column is frozen
 * as soon as its history meets hist[k] <= tol * hist[0]: no later launch reads or writes it; the call ends when every
 * column is frozen or after max_cycles.  stats[j].seconds is the wall time of the whole call in every entry;
 * max_cycles = 0 writes one history entry per column and returns the guesses.  Deterministic; one host
 * synchronisation per cycle; launched eagerly (cfg.profile does not extend to the call).
 * The handle's own U, B, R of every level and its cached graphs are left as they were, and every other entry point
 * computes, before and after, the bits of a handle that never made the call.  Memory: the first call allocates, inside
 * the handle, nrhs copies of each level's u, tmp, b, r, per-column partial sums and the pinned sums; a later call with
 * a larger nrhs adds the difference; mgx_destroy frees it.  The workspace holds no copy of the operator: a call after
 * mgx_set_* and a rebuild uses the new operator.
 * Single-GPU handles of dtype F64 or F32, op STENCIL5 or GALERKIN, smoother JACOBI: every cycle kind (W and F through
 * the per-level launches, whose bits k_small_visit shares), either transfer, every restriction mode the handle
 * accepts, either bottom, a five- or nine-point finest level.  MGX_ERR_STATE (reason in mgx_last_error) on POISSON
 * handles (their kernels read no coefficient grids: nothing to share), MIXED handles, multi-GPU and rank handles, every
 * other smoother (multi-column Chebyshev, line and colour smoothers are a follow-up) and before the operators are set
 * / built; MGX_ERR_INVALID for nrhs < 1 or nrhs > MGX_MAX_RHS, NULL b or u, tol not >= 0, max_cycles < 0;
 * MGX_ERR_ALLOC leaves the handle (and the columns that existed) usable. */
#define MGX_MAX_RHS 4
MGX_API int mgx_solve_multi(mgx_handle h, int nrhs, const void* b, void* u, double tol, int max_cycles,
                            mgx_stats* stats, double* history, int history_cap);

/* mgx_solve_gcr's iteration on up to MGX_MAX_RHS right-hand sides for one operator: restarted GCR with right
 * preconditioning on the finest level, the preconditioner mgx_solve_multi's cycle from zero on the columns still
 * iterating (every coefficient grid, transfer weight and the dense coarsest inverse read once per pass for all of them),
 * the direction pass Z_j = z, Q_j = A z one launch of k_gcr_direction_multi for the set ((NQ + 3 nrhs) sizeof(T) per point
 * instead of nrhs (NQ + 3)).  The orthogonalisation, update and reduction passes read no coefficients and run once per
 * column, in mgx_solve_gcr's geometry, on that column's own scalars and partial sums; all columns share the iteration
 * index k and so the basis slot k mod restart.  Arguments as for mgx_solve_multi: b and u are nrhs host vectors back to
 * back (u the guesses on entry, the iterates on return), stats NULL or nrhs entries, history NULL or nrhs slots of
 * history_cap doubles.
 * What column j returns - iterate, history, cycles, converged, initial_residual, final_residual, history_len,
 * fine_updates - is bit for bit what mgx_set_rhs(b_j); mgx_set_guess(u_j); mgx_solve_gcr(h, tol, max_iters, restart, ..);
 * mgx_get_solution returns on the same handle.  stats[j].seconds is the wall time of the whole call in every entry.
 * A column leaves the active set for good - no later launch reads or writes it - when hist[0] <= tol * hist[0] or
 * max_iters = 0 (one history entry, the guess returned), when ||r|| <= tol * hist[0] after an iteration, or on its own
 * breakdown (q'.q' not a positive finite number: converged = 0, its x as before that iteration; the call still returns
 * MGX_OK and mgx_last_error names the first such column and iteration).  The call ends when the set is empty or after
 * max_iters.  Deterministic; one device-to-host copy and one host synchronisation per iteration serve all columns;
 * launched eagerly (cfg.profile does not extend to the call).
 * The handle's own U, B, R of every level, its mgx_solve_pcg / mgx_solve_gcr workspace, its cached graphs and its
 * fine_updates are left as they were, and every other entry point computes, before and after, the bits of a handle that
 * never made the call.  Memory: mgx_solve_multi's columns and, per column, x, 2 restart vectors of the finest level, the
 * partial sums of a pass and a block of scalars (all blocks in one device buffer with one pinned mirror); a later call
 * with a larger nrhs or restart adds the difference; mgx_destroy frees it.
 * MGX_ERR_STATE exactly where mgx_solve_multi returns it (POISSON, MIXED, multi-GPU and rank handles, every smoother but
 * JACOBI, before the operators are set / built); MGX_ERR_INVALID for nrhs < 1 or nrhs > MGX_MAX_RHS, NULL b or u, tol not
 * >= 0, max_iters < 0, restart < 1 or restart > MGX_GCR_MAX_RESTART; MGX_ERR_ALLOC leaves the handle (and what existed of
 * the workspace) usable. */
MGX_API int mgx_solve_multi_gcr(mgx_handle h, int nrhs, const void* b, void* u, double tol, int max_iters, int restart,
                                mgx_stats* stats, double* history, int history_cap);

/* mgx_solve_refine_gcr's iteration on up to MGX_MAX_RHS right-hand sides for one operator: fp64 restarted GCR on the
 * finest level, the preconditioner mgx_solve_multi's float cycle from zero on the columns of the float copy of the
 * hierarchy still iterating (a sweep moves 4 (NQ + 3 nrhs) bytes per point where nrhs fp64 solves move 8 nrhs (NQ + 3)),
 * the direction pass Z_j = z = s (double) z32, Q_j = A z one launch of k_refine_direction<NQ, nrhs> for the set (8 NQ + 20 nrhs
 * bytes per point instead of nrhs (8 NQ + 20); every instance, the nine-point one on four columns included, runs without
 * scratch: four nine-point columns are one launch).  The orthogonalisation, the mixed update and the reductions read no
 * coefficients and run once per column, in mgx_solve_refine_gcr's geometry, on that column's own scalars and partial sums;
 * all columns share the iteration index k and so the basis slot k mod restart.  Arguments as for mgx_solve_multi_gcr: b
 * and u are nrhs host vectors of doubles back to back (u the guesses on entry, the iterates on return), stats NULL or
 * nrhs entries, history NULL or nrhs slots of history_cap doubles.
 * What column j returns - iterate, history, cycles, converged, initial_residual, final_residual, history_len,
 * fine_updates (those of the float cycle) - is bit for bit what mgx_set_rhs(b_j); mgx_set_guess(u_j);
 * mgx_solve_refine_gcr(h, tol, max_iters, restart, ..); mgx_get_solution returns on the same handle.  The scale of
 * iteration k of column j comes from that column's own history: pow2_floor(hist_j[max(k - 1, 0)] / n).
 * stats[j].seconds is the wall time of the whole call in every entry.  A column leaves the active set for good - no
 * later launch reads or writes it - under mgx_solve_multi_gcr's rules: hist[0] <= tol * hist[0] or max_iters = 0 (one
 * history entry, the guess returned), ||r|| <= tol * hist[0] after an iteration, or its own breakdown (converged = 0,
 * its x as before that iteration; the call still returns MGX_OK and mgx_last_error names the first such column and
 * iteration).  Deterministic; one device-to-host copy and one host synchronisation per iteration serve all columns;
 * launched eagerly (cfg.profile does not extend to the call).
 * One configuration is defined differently and not held to the sequential bits: on a one-level hierarchy (finest =
 * coarsest) with bottom = SMOOTH, mgx_solve_refine_gcr starts its float cycle from whatever the float copy's U held
 * before; this call zeroes the column's float u before every cycle.  (With bottom = EXACT the dense solve overwrites it,
 * and the contract holds.)
 * The handle's own U, B, R of every level, its mgx_solve_pcg / mgx_solve_gcr workspace, its cached graphs and its
 * fine_updates, and the float copy's own vectors and graphs, are left as they were; every other entry point -
 * mgx_solve_refine, mgx_solve_refine_gcr, mgx_solve_multi and mgx_solve_multi_gcr included - computes, before and after,
 * the bits of a handle that never made the call.  Memory: the float copy of the hierarchy (shared with
 * mgx_solve_refine and mgx_solve_refine_gcr); mgx_solve_multi's columns of the float copy (float u, tmp, b, r of every
 * level per column); the handle's mgx_solve_multi_gcr workspace, shared with that call (per column x, r, scratch,
 * restart pairs Z, Q, the partial sums and a block of scalars) - its coarse fp64 columns are allocated and not used by
 * this call: the price of one workspace.  A later call with a larger nrhs or restart adds the difference.
 * Single-GPU handles of dtype F64, op STENCIL5 or GALERKIN, smoother JACOBI: every cycle kind, either transfer, every
 * restriction mode the handle accepts, either bottom, a five- or nine-point finest level.  MGX_ERR_STATE (reason in
 * mgx_last_error) on POISSON, F32, MIXED, multi-GPU and rank handles, every other smoother and before the operators are
 * set / built; MGX_ERR_INVALID, checked first and in this order, for nrhs < 1 or nrhs > MGX_MAX_RHS, NULL b or u, tol
 * not >= 0, max_iters < 0, restart < 1 or restart > MGX_GCR_MAX_RESTART; MGX_ERR_ALLOC and the F32 build's error from
 * the float copy leave the fp64 state and what existed of the workspaces usable. */
MGX_API int mgx_solve_multi_refine_gcr(mgx_handle h, int nrhs, const void* b, void* u, double tol, int max_iters, int restart,
                                       mgx_stats* stats, double* history, int history_cap);

/* The nev <= MGX_MAX_RHS smallest eigenpairs A x_j = lambda_j x_j of the finest-level operator A of a general-operator
 * handle, by LOBPCG (locally optimal block preconditioned conjugate gradients) whose preconditioner is
 * mgx_solve_multi's cycle from zero, every coefficient grid read once per pass for the block (csrc/mgx_eig.hpp states
 * the iteration operation by operation).  A must be symmetric positive definite: mgx_set_coefficient, mgx_set_tensor, or
 * symmetric mgx_set_stencil / mgx_set_stencil9 input; symmetry is the caller's duty and is not checked.  A is the
 * stencil AS STORED: it carries no h^-2 (multiply lambda by N^2 for the differential operator on the unit square).
 * x: nev host vectors back to back, each n*n, in the handle's working type (mgx_solve_multi's layout); on entry the
 * guesses, on return the Ritz vectors with unit 2-norm ordered by ascending lambda[j], sign unspecified.  stats: NULL
 * or nev entries; history: NULL or nev slots of history_cap doubles.  hist_j[k] = ||A x_j - theta_j x_j||_2 after
 * iteration k, entry 0 after the initial Rayleigh-Ritz step on the guesses; A x is applied afresh in every iteration, so
 * these are the residuals of the pair returned, not of a recurrence.  stats[j]: cycles = preconditioner cycles applied
 * to column j, initial_residual / final_residual = first and last history entry, converged = the last entry <= tol *
 * theta_j, fine_updates as mgx_solve_multi counts them, seconds = the whole call, the same in every entry.  max_iters =
 * 0 does the initial Rayleigh-Ritz step and writes one history entry.
 * Soft locking: a column whose residual meets tol * theta_j gets no cycle and no search direction, but it stays in the
 * block, is still rewritten by every Ritz rotation and iterates again if its residual rises above the tolerance - not
 * the "frozen for good" rule of the block solvers.
 * A Rayleigh-Ritz step whose basis [X, W, P] is numerically rank deficient (a Cholesky pivot of the scaled Gram matrix
 * not positive and finite, or below 64 eps) is repeated once without the directions P; if it still is, the call ends:
 * the columns still iterating report converged = 0, mgx_last_error holds the reason, the return value is MGX_OK (as for a
 * GCR breakdown).  A Ritz value that is not a positive finite number ends the call the same way with converged = 0 in
 * every column.  Linearly dependent guesses: MGX_ERR_INVALID.
 * Deterministic (every sum in a fixed order, no atomics); two device-to-host copies and host synchronisations per
 * iteration (the residual norms, the Gram sums); launched eagerly (cfg.profile does not extend to the call).
 * The handle's own U, B, R of every level, its Krylov workspaces, its cached graphs and its fine_updates are left as
 * they were; every other entry point computes, before and after, the bits of a handle that never made the call.
 * Memory: mgx_solve_multi's columns (shared with that call) and five finest-level vectors per column (X, AX, AW, P,
 * AP; W is the column's finest u, the residual its finest b), allocated on first use, grown for a larger nev, freed by
 * mgx_destroy.
 * Accepted and refused handles: exactly mgx_solve_multi's (MGX_ERR_STATE with the reason on POISSON, MIXED, multi-GPU
 * and rank handles, every smoother but JACOBI, before the operators are set / built).  MGX_ERR_INVALID, checked first
 * and in this order: nev < 1 or nev > MGX_MAX_RHS, NULL x or lambda, tol not >= 0, max_iters < 0.  MGX_ERR_ALLOC leaves
 * the handle and what existed of the workspaces usable. */
MGX_API int mgx_eigs(mgx_handle h, int nev, void* x, double* lambda, double tol, int max_iters, mgx_stats* stats,
                     double* history, int history_cap);

/* Up to MGX_EIGS_MAX smallest eigenpairs: mgx_eigs' iteration on blocks of at most MGX_MAX_RHS columns, each block
 * iterating in the complement of the pairs found before it (deflation by locking; csrc/mgx_eig_many.hpp states it
 * operation by operation).  The arguments and their layout are mgx_eigs', with nev up to MGX_EIGS_MAX:
 *     Y = {}                                  (locked vectors, device resident, orthonormal)
 *     while |Y| < nev:
 *         kb = min(MGX_MAX_RHS, nev - |Y|);  X = the caller's guesses |Y| .. |Y| + kb - 1
 *         X <- X - Y (Y^T X), twice           (once per block; skipped when Y is empty)
 *         mgx_eigs' iteration on X, with one change: after W_act = M R_act,
 *             W_act <- W_act - Y (Y^T W_act)  (once per iteration; skipped when Y is empty)
 *         the block ends as mgx_eigs ends: every column meets hist <= tol theta, or after max_iters iterations, or
 *         on its failures
 *         if it did not end converged: stop.   else Y <- [Y, X]
 *     sort the computed pairs by lambda ascending (stable); vectors, stats and history slots follow
 * The projection: c_ij = Y_i . W_j in double, every sum in a fixed order, all from the unmodified W (classical
 * Gram-Schmidt); then W_j = ((W_j - c_0j Y_0) - c_1j Y_1) - ..., i ascending over all locked vectors, c_ij rounded to the
 * working type once, every product and difference rounded in it.  The coefficients stay on the device: two host
 * synchronisations per iteration, as in mgx_eigs.
 * max_iters is the budget of EACH block.  Per pair: hist_j[k] = ||A x_j - theta_j x_j|| after iteration k of the pair's
 * own block, A applied afresh; stats[j] as in mgx_eigs, counted within that block; seconds = the whole call, the same in
 * every computed entry.  nev <= MGX_MAX_RHS is one block without a constraint and returns, bit for bit, what mgx_eigs
 * returns.
 * A block that ends unconverged ends the call: its pairs come back as they stand (converged per column as in mgx_eigs),
 * the pairs of the later blocks are not computed - x_j stays the caller's guess, lambda[j] = 0, stats[j] all zero with
 * history_len = 0, their history slots untouched - and they stay behind the computed ones; the return value is MGX_OK
 * and mgx_last_error names the block and the reason.  Guesses that are linearly dependent after the projection:
 * MGX_ERR_INVALID, naming the block (nothing is written to x, lambda, stats or history).
 * What deflation cannot promise: a block converges to the smallest pairs of the complement of Y THAT ITS GUESSES REACH,
 * and the final order is that of the computed values - no Rayleigh-Ritz step over all nev vectors is made.  A tight
 * cluster of eigenvalues that straddles a block boundary converges slowly (the gap behind a block is the cluster's
 * width); an exactly degenerate pair cut by a boundary does not: the part of the eigenspace that is locked is gone from
 * the complement, and what remains of it there is separated from the next eigenvalue by an ordinary gap.  The locked vectors are as orthonormal as the
 * blocks' Ritz rotations leave them (|X^T X - I| of a few units of roundoff times the iteration count).
 * Accepted and refused handles: mgx_solve_multi's.  MGX_ERR_INVALID, checked first and in this order: nev < 1 or
 * nev > MGX_EIGS_MAX, NULL x or lambda, tol not >= 0, max_iters < 0.  The handle is left as it was: its own U, B, R, its
 * Krylov workspaces, graphs and fine_updates are unchanged and every other entry point, mgx_eigs included, computes the
 * same bits before and after.  Memory: mgx_eigs' workspace of one block, plus nev finest-level vectors Y, the table of
 * their pointers and MGX_EIGS_MAX x MGX_MAX_RHS coefficients with their partial sums; allocated on first use, grown for
 * a larger nev, freed by mgx_destroy; MGX_ERR_ALLOC leaves everything usable.  Deterministic; launched eagerly. */
#define MGX_EIGS_MAX 16
MGX_API int mgx_eigs_many(mgx_handle h, int nev, void* x, double* lambda, double tol, int max_iters,
                          mgx_stats* stats, double* history, int history_cap);

/* ---- implicit time stepping: theta steps of  M u_t + A0 u = f  on the device (csrc/mgx_theta.hpp; absent in the
 * reference) -----------------------------------------------------------------------------------------------------------
 * The handle's operator is S = A0 + diag(d) with d = M / (theta dt) (mass over step, in stencil units: mgx_set_reaction).
 * One step is
 *     S u+ = (1 / theta) d.u - ((1 - theta) / theta) S u + g,        g = f / theta in stencil units,
 * theta = 1 implicit Euler, theta = 1/2 Crank-Nicolson.  g: host, n * n, the working type, constant over the call's
 * steps, may be NULL; it is uploaded once per call into a grid the handle keeps (MGX_ERR_ALLOC leaves the handle usable).
 * Per step one launch of k_theta_rhs writes B of the finest level from U, d, g and the finest coefficients, then the
 * chosen solver runs from the current U (the previous time level) with the caller's tol, max_iters and restart (ignored
 * for MGX_STEP_SOLVE): mgx_solve, mgx_solve_gcr or mgx_solve_refine_gcr.  Nothing but that solver's own scalars crosses
 * the bus between steps.  The pass, every product and sum rounded on its own in the working type T:
 *     m = d_p * u_p
 *     theta = 1:  b_p = m, then + g_p if g is given                       (reads no coefficient grid)
 *     theta < 1:  q = (S u)_p, the sum of mgx_residual (CSR order, centre included, ring-pointing coefficients times the
 *                 zero ring);  b_p = c1 * m - c0 * q, then + g_p;  c1 = (T)(1 / theta), c0 = (T)((1 - theta) / theta)
 *                 formed in double and rounded once.
 * Ring and padding of B stay zero.  What step k leaves in U, stats[k] and history slot k are bit for bit what the caller
 * gets from  b = the pass on the host (S u = -mgx_residual with B = 0);  mgx_set_rhs(b);  the same solver call  on the
 * same handle.  stats: NULL or nsteps entries; history: NULL or nsteps slots of history_cap doubles; *steps_done (may be
 * NULL) counts the completed steps.  A step whose solve ends with converged = 0 (budget or breakdown) ends the call after
 * that step: MGX_OK, *steps_done includes it, U is its iterate, the later stats and history slots are untouched and
 * mgx_last_error names the step and the reason.  nsteps = 0 does nothing.  On return B holds the last step's right-hand
 * side.  cfg.schedule is whatever the chosen solver makes of it: under MGX_STEP_SOLVE an FMG handle discards U in its
 * first cycle - a V-schedule handle is what keeps the warm start there; the Krylov solvers ignore the schedule.
 * MGX_ERR_INVALID, checked first and in this order: theta not in (0, 1] (NaN included), nsteps < 0, unknown solver, tol
 * not >= 0, max_iters < 0, and for the GCR solvers restart outside 1 .. MGX_GCR_MAX_RESTART.  MGX_ERR_STATE where
 * mgx_set_reaction returns it, when no term is set (there is no mass term to step with), before the hierarchy is built,
 * and with MGX_STEP_REFINE_GCR wherever mgx_solve_refine_gcr returns it (F32 handles).  A time-dependent g: one call
 * with nsteps = 1 per step. */
enum { MGX_STEP_SOLVE = 0, MGX_STEP_GCR = 1, MGX_STEP_REFINE_GCR = 2 };
MGX_API int mgx_theta_steps(mgx_handle h, double theta, int nsteps, const void* g, int solver, double tol, int max_iters,
                            int restart, int* steps_done, mgx_stats* stats, double* history, int history_cap);

/* ---- Newton-multigrid for the semilinear problem  -div(a grad u) + kappa(x) phi(u) = f,  u = 0 on the boundary, on the
 * device (csrc/mgx_newton.hpp; absent in the reference) -----------------------------------------------------------------
 * Handles with op = MGX_OPERATOR_GALERKIN, on the finest level.  A0 is the finest operator without a zero-order term (what
 * the last of mgx_set_stencil / mgx_set_coefficient / mgx_set_stencil9 / mgx_set_tensor gave), kappa an interior n x n
 * grid in stencil units (host, row-major, the working type T: pass kappa h^2, as for mgx_set_reaction),
 * phi(u) = p1 u + p2 u^2 + p3 u^3 with the three doubles rounded to T once, q2 = (T)(2 p2) and q3 = (T)(3 p3) formed in
 * double and rounded once, f the finest B at entry, the guess the finest U at entry:  F(u) = A0 u + kappa phi(u) - f.
 * The pass (k_newton_pass, one launch and one reduction; every product and sum rounded on its own in T):
 *     v   = u                       the first evaluation
 *     v   = u + lam * de            a trial: lam = 2^-j, de the linear solve's result
 *     q   = (A0 v)_p                the sum of mgx_residual (CSR order, centre included, ring-pointing coefficients times
 *                                   the zero ring)
 *     ph  = ((p3 * v + p2) * v + p1) * v
 *     dp  = (q3 * v + q2) * v + p1
 *     b_p = f_p - (q + kap_p * ph)          d_p = kap_p * dp
 * and ||F(v)||_2 = sqrt(sum b_p^2), the sum formed as mgx_residual_norm forms it: bit for bit its value for B = b, U = 0.
 * The iteration, hist[0] = ||F(U)||, for k = 0 .. max_newton - 1 while !(hist[k] <= tol * hist[0]):
 *     the operator becomes A0 + diag(d) (as mgx_set_reaction(d) does) and the hierarchy is rebuilt with the transfer it
 *     was last built with;  B = b, U = 0, the chosen solver runs with lin_tol, lin_max_iters and restart (ignored for
 *     MGX_STEP_SOLVE): lin_stats[k];  de = U;  trials lam = 1, 1/2, ... until
 *         ||F(u + lam de)|| <= (1 - 1e-4 lam) hist[k]          (in double on the host; a NaN rejects)
 *     at most max_backtracks halvings (0: plain Newton, every full step must pass the test);  u = u + lam de,
 *     hist[k + 1] = its norm, step_lengths[k] = lam.
 * A linear solve that ends with converged = 0 (budget or breakdown) does not end the call: it is an inexact Newton step
 * that the line search guards, and lin_stats[k] reports it.  An error status of the solver ends the call with that
 * status, mgx_last_error prefixed "mgx_newton: step k:".  A failed line search ends the call with MGX_OK and converged =
 * 0, U the last accepted iterate; mgx_last_error names the step, the smallest lam tried and the two norms.
 * After every accepted step the iterate, hist, lin_stats, step_lengths and the backtrack count are bit for bit what the
 * caller gets on the same handle from: the pass on the host; mgx_set_reaction(d); mgx_build_galerkin_transfer(t);
 * mgx_set_rhs(b), a zero guess, the same solver call, mgx_get_solution; u + lam de on the host and its norm through
 * mgx_residual_norm with U = 0.
 * On return U holds the iterate and B the caller's f bit for bit.  The handle's operator is A0 + diag(d_k) of the last
 * linear solve with its hierarchy built: mgx_get_reaction returns d_k and mgx_set_reaction(h, NULL, 0) restores A0,
 * exactly as after a caller's own mgx_set_reaction + build; a term set before the call is replaced, as a second
 * mgx_set_reaction does.  When no iteration runs (max_newton = 0, or hist[0] <= tol * hist[0]) the operator, the
 * hierarchy and the graphs are untouched.  Positivity of c0 + d is the caller's duty, as for mgx_set_reaction.
 * nstats may be NULL; lin_stats and step_lengths: NULL or max_newton entries; history: NULL or history_cap doubles, the
 * first min(history_len, history_cap) are written.
 * Workspace: five finest-level grids (the iterate, the trial, f, kappa, the next d) and mgx_set_reaction's two, allocated
 * before anything is touched (MGX_ERR_ALLOC leaves operator and hierarchy usable) and freed by mgx_destroy.
 * MGX_ERR_INVALID, checked first and in this order: NULL handle or opt (outputs left alone), a p that is not finite,
 * unknown solver, lin_tol not >= 0, lin_max_iters < 0, for the GCR solvers restart outside 1 .. MGX_GCR_MAX_RESTART, tol
 * not >= 0, max_newton < 0, max_backtracks outside 0 .. 30, NULL kappa, count != n * n.  MGX_ERR_STATE with the reason
 * where mgx_set_reaction returns it (POISSON, STENCIL5, multi-GPU and rank handles; finest operator not set), before the
 * hierarchy has been built (that is how the transfer is known), and with MGX_STEP_REFINE_GCR wherever
 * mgx_solve_refine_gcr returns it (F32 handles).  Every smoother, cycle kind, transfer, bottom and a five- or nine-point
 * finest level are accepted: the call runs the public solvers. */
typedef struct {
    double p1, p2, p3;      /* phi(u) = p1 u + p2 u^2 + p3 u^3 */
    int solver;             /* MGX_STEP_SOLVE / MGX_STEP_GCR / MGX_STEP_REFINE_GCR (the enum of mgx_theta_steps) */
    double lin_tol;         /* the linear solver's tol, ... */
    int lin_max_iters;      /* ... max_iters ... */
    int restart;            /* ... and restart (GCR solvers) */
    double tol;             /* stop when ||F|| <= tol * ||F(guess)|| */
    int max_newton;         /* at most this many Newton steps */
    int max_backtracks;     /* halvings per step; 0: plain Newton, every full step must pass the test */
} mgx_newton_opts;
typedef struct {
    int iterations;         /* accepted Newton steps */
    int converged;          /* hist[last] <= tol * hist[0] */
    double initial_residual, final_residual, seconds;
    int linear_iterations;  /* sum of lin_stats[k].cycles */
    int backtracks;         /* rejected trials over all steps */
    int history_len;        /* iterations + 1 */
} mgx_newton_stats;
MGX_API int mgx_newton(mgx_handle h, const mgx_newton_opts* opt, const void* kappa, size_t count, mgx_newton_stats* nstats,
                       mgx_stats* lin_stats, double* step_lengths, double* history, int history_cap);

/* ---- implicit time stepping of the semilinear problem  rho u_t = div(a grad u) - kappa(x) phi(u) + f,  u = 0 on the
 * boundary, on the device (csrc/mgx_newton.hpp, csrc/mgx_newton_steps_host.hpp; absent in the reference) ---------------
 * Handles with op = MGX_OPERATOR_GALERKIN, on the finest level; A0, kappa, phi, p1 .. p3, q2, q3 as for mgx_newton,
 * everything in stencil units.  mass = dm = rho h^2 / (theta dt) and kappa are interior n x n grids (host, row-major, the
 * working type T); g = f / theta in stencil units, constant over the call's steps, may be NULL.  All three are uploaded once
 * per call into grids the handle keeps.  One theta step from the time level u (the finest U at entry) to u+ solves
 *     G(v) = A0 v + dm.v + kappa.phi(v) - r = 0,      r = dm.u - c0 (A0 u + kappa.phi(u)) + g,
 * c0 = (T)((1 - theta) / theta) formed in double and rounded once; theta = 1 implicit Euler, theta = 1/2 Crank-Nicolson.
 * Per step one launch of k_newton_step_rhs writes r, every product and sum rounded on its own in T:
 *     m = dm_p * u_p
 *     theta = 1:  r_p = m, then + g_p if g is given                      (reads no neighbour and no coefficient grid)
 *     theta < 1:  q = (A0 u)_p as in mgx_newton's pass;  ph = ((p3 * u + p2) * u + p1) * u;
 *                 r_p = m - c0 * (q + kap_p * ph), then + g_p
 * then Newton's method runs on G from u as the guess (warm start) exactly as mgx_newton runs it on F, with opt's tol,
 * max_newton, max_backtracks, solver, lin_tol, lin_max_iters and restart; its pass is mgx_newton's with a mass term
 * (k_newton_pass, MASS instances; v, q, ph, dp as there):
 *     b_p = r_p - ((q + dm_p * v) + kap_p * ph)          d_p = dm_p + kap_p * dp
 * so the Jacobian is A0 + diag(dm + kappa phi'(v)), and ||G(v)||_2 is bit for bit mgx_residual_norm of (B = b, U = 0).
 * Between steps nothing but the solvers' own scalars and the pass norms crosses the bus.
 * step_stats: NULL or nsteps entries, step_stats[k] what mgx_newton reports for the iteration of step k (seconds = the
 * step's); history: NULL or nsteps slots of history_cap doubles, slot k the norms ||G|| of step k; *steps_done (may be
 * NULL) counts the completed steps.  After every step U, step_stats[k] (all fields but seconds) and history slot k are
 * bit for bit what the caller gets on the same handle from the host composition: the right-hand-side pass on the host;
 * then per Newton iteration the MASS pass on the host, mgx_set_reaction(d), mgx_build_galerkin_transfer(t),
 * mgx_set_rhs(b), a zero guess, the same solver call, mgx_get_solution; the trial u + lam de on the host and its norm
 * through mgx_residual_norm with U = 0.
 * A step whose Newton iteration ends with converged = 0 (budget or failed line search) ends the call after that step:
 * MGX_OK, *steps_done includes it, U holds its last accepted iterate, the later slots are untouched and mgx_last_error
 * names the step and the reason.  An error status of a solver ends the call with that status, mgx_last_error prefixed
 * "mgx_newton_steps: step k:".  nsteps = 0 touches nothing: operator, hierarchy, graphs, U and B stay as they are.
 * On return U is the last time level and B holds the last step's r.  The handle's operator is A0 + diag(d) of the last
 * linear solve with its hierarchy built: mgx_get_reaction returns that d and mgx_set_reaction(h, NULL, 0) restores A0; a
 * term set before the call is replaced.  (When no step ran a Newton iteration the operator is untouched, as for
 * mgx_newton.)  Positivity of c0 + d is the caller's duty.  A time-dependent g: one call with nsteps = 1 per step.
 * Workspace: mgx_newton's grids, the mass term and, with the first g, the source, allocated before anything is touched
 * (MGX_ERR_ALLOC leaves operator and hierarchy usable) and freed by mgx_destroy.
 * MGX_ERR_INVALID, checked first and in this order: NULL handle or opt (outputs left alone), mgx_newton's checks on opt in
 * its order, theta not in (0, 1] (NaN included), nsteps < 0, NULL mass, NULL kappa, count != n * n.  MGX_ERR_STATE exactly
 * where mgx_newton returns it.  A refused call leaves the handle usable with its bits. */
MGX_API int mgx_newton_steps(mgx_handle h, const mgx_newton_opts* opt, double theta, int nsteps, const void* mass,
                             const void* kappa, const void* g, size_t count, int* steps_done, mgx_newton_stats* step_stats,
                             double* history, int history_cap);

/* ---- Picard and Newton multigrid for the quasilinear problem  -div(a(x) k(u) grad u) = f,  u = 0 on the boundary, on the
 * device (csrc/mgx_quasi.hpp, csrc/mgx_quasi_host.hpp; absent in the reference) ---------------------------------------------
 * Handles with op = MGX_OPERATOR_GALERKIN, on the finest level.  a_nodes is the nodal coefficient on the (N + 1)^2 nodes,
 * N = 2^finest_level (host, double, row-major, boundary nodes included: the argument of mgx_set_coefficient);
 * k(u) = k0 + k1 u + k2 u^2 with the three doubles as given; f the finest B at entry in stencil units, the guess the
 * finest U at entry:  F(u) = A(u) u - f,  A(u) the five-point operator mgx_set_coefficient forms from the nodal a k(u).
 * The pass (k_quasi_pass, one launch and one reduction).  All coefficient arithmetic is in double whatever T is, one
 * rounding to T per coefficient; everything on u is in T; every product and sum rounded on its own.  At the interior
 * point p and its neighbours x = N, S, W, E, the ring of v being zero:
 *     v     = u                          the first evaluation
 *     v     = u + lam * de               a trial: lam = 2^-j (rounded to T), de the linear solve's result
 *     vd_x  = (double)v_x;   kap_x = a_x * ((k2 * vd_x + k1) * vd_x + k0)
 *     fn    = 0.5 * (kap_p + kap_N), fs, fw, fe alike
 *     cP    = (T)(((fn + fw) + fe) + fs);   nP = (T)(-fn), sP = (T)(-fs), wP = (T)(-fw), eP = (T)(-fe)
 *     q     = cP, nP, sP, wP, eP applied to v in T: the sum of mgx_residual (CSR order N, W, C, E, S; ring-pointing
 *             coefficients times the zero ring);   b_p = f_p - q
 * and ||F(v)||_2 = sqrt(sum b_p^2), the sum formed as mgx_residual_norm forms it: bit for bit its value for B = b, U = 0.
 * MGX_QUASI_PICARD: the operator of the next linear solve is (cP, nP, sP, wP, eP) = A(v).  MGX_QUASI_NEWTON: it is the
 * Jacobian of F, five-point and not symmetric, with kk2 = 2.0 * k2 formed in double:
 *     dk_x  = a_x * (kk2 * vd_x + k1);   gN = vd_p - vd_N, gS, gW, gE alike;   sg = ((gN + gW) + gE) + gS
 *     cJ    = (T)((((fn + fw) + fe) + fs) + (0.5 * dk_p) * sg)
 *     nJ    = (T)((0.5 * dk_N) * gN - fn), sJ, wJ, eJ alike
 * (the residual uses the Picard coefficients either way).  Coefficients that point at the ring are stored as computed.
 * The iteration, hist[0] = ||F(U)||, for k = 0 .. max_iters - 1 while !(hist[k] <= tol * hist[0]):
 *     the finest operator becomes what the pass wrote for u_k (as mgx_set_stencil does) and the hierarchy is rebuilt with
 *     opt.transfer;  B = b, U = 0, the chosen solver runs with lin_tol, lin_max_iters and restart (ignored for
 *     MGX_STEP_SOLVE): lin_stats[k];  de = U;  trials lam = 1, 1/2, ... until
 *         ||F(u + lam de)|| <= (1 - 1e-4 lam) hist[k]          (in double on the host; a NaN rejects)
 *     at most max_backtracks halvings (0: every full step must pass the test);  u = u + lam de, hist[k + 1] = its norm,
 *     step_lengths[k] = lam.  The accepted trial's pass output is the next iteration's operator and right-hand side.
 * A linear solve that ends with converged = 0 (budget or breakdown) does not end the call: it is an inexact step that the
 * line search guards, and lin_stats[k] reports it.  An error status of the solver ends the call with that status,
 * mgx_last_error prefixed "mgx_quasi: step k:".  A failed line search ends the call with MGX_OK and converged = 0, U the
 * last accepted iterate; mgx_last_error names the step, the smallest lam tried and the two norms.
 * After every accepted step the iterate, hist, lin_stats (all but seconds), step_lengths and the backtrack count are bit
 * for bit what the caller gets on the same handle from: the pass on the host; mgx_set_stencil(finest, the five grids);
 * mgx_build_galerkin_transfer(transfer); mgx_set_rhs(b), a zero guess, the same solver call, mgx_get_solution; u + lam de
 * on the host and its norm through mgx_residual_norm with B = the trial's b and U = 0.
 * On return U holds the iterate and B the caller's f bit for bit.  The handle is in the state those mgx_set_stencil +
 * build calls leave: the finest level is five-point whatever it was before, a zero-order term set earlier is dropped,
 * and mgx_get_stencil / mgx_get_stencil9 return the operator of the last linear solve on every level (a rejected or a
 * last accepted trial writes a second set of grids, never the operator).  When no iteration runs (max_iters = 0, or
 * hist[0] <= tol * hist[0]) the operator, the hierarchy and the graphs are untouched.  The call needs no operator or
 * hierarchy beforehand.  Positivity of a k(u) at every iterate, and for MGX_QUASI_NEWTON solvability of the Jacobian, are
 * the caller's duty, as positivity of c0 + d is for mgx_newton.
 * nstats may be NULL; lin_stats and step_lengths: NULL or max_iters entries; history: NULL or history_cap doubles, the
 * first min(history_len, history_cap) are written.
 * Workspace: eight finest-level grids (the iterate, the trial, f, the five coefficient grids of the next operator; b is
 * the level's B) and the nodal a as doubles in the level's rows and pitch, allocated before anything is touched
 * (MGX_ERR_ALLOC leaves the handle usable) and freed by mgx_destroy.
 * MGX_ERR_INVALID, checked first and in this order: NULL handle or opt (outputs left alone), a k that is not finite,
 * unknown method, unknown transfer, unknown solver, lin_tol not >= 0, lin_max_iters < 0, for the GCR solvers restart
 * outside 1 .. MGX_GCR_MAX_RESTART, tol not >= 0, max_iters < 0, max_backtracks outside 0 .. 30, NULL a_nodes,
 * count != (N + 1)^2.  MGX_ERR_STATE with the reason on POISSON, STENCIL5, multi-GPU and rank handles, and with
 * MGX_STEP_REFINE_GCR wherever mgx_solve_refine_gcr returns it (F32 handles).  A refused call leaves the handle's bits
 * alone.  Every smoother, cycle kind and bottom are accepted: the call runs the public solvers. */
enum { MGX_QUASI_PICARD = 0, MGX_QUASI_NEWTON = 1 };
typedef struct {
    double k0, k1, k2;      /* k(u) = k0 + k1 u + k2 u^2 */
    int method;             /* MGX_QUASI_PICARD = 0, MGX_QUASI_NEWTON = 1 */
    int transfer;           /* MGX_TRANSFER_BILINEAR / MGX_TRANSFER_OPERATOR */
    int solver;             /* MGX_STEP_SOLVE / MGX_STEP_GCR / MGX_STEP_REFINE_GCR (the enum of mgx_theta_steps) */
    double lin_tol;         /* the linear solver's tol, ... */
    int lin_max_iters;      /* ... max_iters ... */
    int restart;            /* ... and restart (GCR solvers) */
    double tol;             /* stop when ||F|| <= tol * ||F(guess)|| */
    int max_iters;          /* at most this many nonlinear steps */
    int max_backtracks;     /* halvings per step; 0: every full step must pass the test */
} mgx_quasi_opts;
MGX_API int mgx_quasi(mgx_handle h, const mgx_quasi_opts* opt, const double* a_nodes, size_t count, mgx_newton_stats* stats,
                      mgx_stats* lin_stats, double* step_lengths, double* history, int history_cap);

/* ---- measurement ------------------------------------------------------------ */
enum {
    MGX_PROF_SMOOTH_FINE = 0,   /* finest-level smoother launches */
    MGX_PROF_RESTRICT_FINE = 1, /* finest-level fused residual+restriction */
    MGX_PROF_PROLONG_FINE = 2,  /* finest-level prolongation+correction */
    MGX_PROF_NORM_FINE = 3,     /* finest-level residual norm */
    MGX_PROF_COARSE = 4,        /* everything below the finest level */
    MGX_PROF_COUNT = 5
};
typedef struct {
    double ms[MGX_PROF_COUNT];        /* accumulated HIP-event time */
    long long launches[MGX_PROF_COUNT]; /* kernel launches inside those intervals */
    long long sweeps[MGX_PROF_COUNT];   /* smoother sweeps those launches performed (a fused
                                           launch does several; 0 for non-smoother classes) */
} mgx_profile;
/* Valid when cfg.profile = 1 or 2; events are recorded on the handle's stream. */
MGX_API int mgx_profile_reset(mgx_handle h);
MGX_API int mgx_profile_get(mgx_handle h, mgx_profile* out);
/* `sweeps` finest-level smoother sweeps bracketed by HIP events on the
 * handle's stream; returns the elapsed milliseconds. */
MGX_API int mgx_time_smoother(mgx_handle h, int sweeps, double* ms);
/* Milliseconds per launch of one streaming pass of mgx_solve_gcr at basis slot j, `repeats` launches between two
 * events on the handle's own buffers (tools/gcr_bench.py).  The scalars are zeroed first, so the passes leave U, B
 * and the saved iterate unchanged (DIRECTION rewrites basis slot j from U; the basis has no meaning between two
 * mgx_solve_gcr calls).  UPDATE is k_pcg_update (6 sizeof(T) per point, the yardstick),
 * DOTS k_gcr_dots<j> (j >= 1), ORTH k_gcr_orth<j>, DIRECTION k_pcg_direction (4 sizeof(T) per point plus the coefficient
 * grids of the finest operator: none for POISSON, 5 on a five-point, 9 on a nine-point finest level).  MGX_ERR_STATE until a mgx_solve_gcr
 * call with restart > j has allocated the basis. */
enum { MGX_GCR_PASS_UPDATE = 0, MGX_GCR_PASS_DOTS = 1, MGX_GCR_PASS_ORTH = 2, MGX_GCR_PASS_DIRECTION = 3 };
MGX_API int mgx_time_gcr_pass(mgx_handle h, int pass, int j, int repeats, double* ms);
/* ms per launch of the fp64 update + residual pass of mgx_solve_refine (k_refine_pass<NQ, true> and its k_reduce_partials)
 * on the handle's own buffers, `repeats` launches between two events (tools/refine_bench.py).  Scale 0, and the updated
 * iterate stays in the scratch grid: U and B are unchanged bit for bit; the float residual of the shadow is rewritten (it has
 * no meaning between two mgx_solve_refine calls).  MGX_ERR_STATE where mgx_solve_refine is, and until a mgx_solve_refine
 * call has created the float copy; MGX_ERR_INVALID for repeats < 1. */
MGX_API int mgx_time_refine_pass(mgx_handle h, int repeats, double* ms);
/* ms per launch of one of mgx_solve_refine_gcr's two mixed passes on the handle's own buffers, `repeats` launches between
 * two events (tools/refine_gcr_bench.py): UPDATE is k_refine_update, DIRECTION k_refine_direction<5 | 9, 1> with scale 1.  The
 * scalars are zeroed first, so U, B and the saved iterate are unchanged bit for bit; the float residual of the shadow
 * (UPDATE) and basis slot 0 (DIRECTION) are rewritten - neither has a meaning between two solves.  MGX_ERR_STATE where
 * mgx_solve_refine_gcr is, and until the float copy and basis slot 0 exist: a mgx_solve_refine_gcr call creates both, and
 * so do a mgx_solve_refine and a mgx_solve_gcr call between them - the call is accepted after those two as well, and is as
 * harmless there; MGX_ERR_INVALID for another pass or repeats < 1. */
enum { MGX_REFINE_GCR_PASS_UPDATE = 0, MGX_REFINE_GCR_PASS_DIRECTION = 1 };
MGX_API int mgx_time_refine_gcr_pass(mgx_handle h, int pass, int repeats, double* ms);
/* `sweeps` finest-level Jacobi sweeps on the first nrhs workspace columns of mgx_solve_multi between two events; returns
 * the elapsed milliseconds (tools/multi_bench.py).  nrhs = 1 runs k_jacobi_var<T, NQ, 1> on a workspace column - the yardstick,
 * in the same run; nrhs = 2..4 one launch of k_jacobi_var<T, NQ, nrhs> per sweep.  The handle's own vectors are untouched.
 * MGX_ERR_STATE where mgx_solve_multi returns it, and until a mgx_solve_multi call with at least that nrhs has
 * allocated the columns; MGX_ERR_INVALID for sweeps < 1, nrhs < 1 or nrhs > MGX_MAX_RHS. */
MGX_API int mgx_time_multi_smoother(mgx_handle h, int nrhs, int sweeps, double* ms);
/* ms per launch of the direction pass of mgx_solve_multi_gcr on its first nrhs workspace columns, from the finest u of
 * each column into its basis slot 0, `repeats` launches between two events (tools/multi_gcr_bench.py).  nrhs = 1 runs
 * k_pcg_direction on a workspace column - the yardstick, in the same run; nrhs = 2..4 one launch of k_gcr_direction_multi.
 * The handle's own vectors are untouched (slot 0 has no meaning between two solves).  MGX_ERR_STATE where
 * mgx_solve_multi_gcr returns it, and until a mgx_solve_multi_gcr call with at least that nrhs has allocated slot 0;
 * MGX_ERR_INVALID for repeats < 1, nrhs < 1 or nrhs > MGX_MAX_RHS. */
MGX_API int mgx_time_multi_gcr_direction(mgx_handle h, int nrhs, int repeats, double* ms);
/* ms per launch of the direction pass of mgx_solve_multi_refine_gcr with scale 1 on its first nrhs columns, from the
 * finest float u of each column of the float copy into basis slot 0 of the handle's column, `repeats` launches between
 * two events (tools/multi_refine_gcr_bench.py).  nrhs = 1 runs k_refine_direction<NQ, 1> on a workspace column - the
 * yardstick, in the same run; nrhs = 2..4 one launch of k_refine_direction<NQ, nrhs>.  The handle's own vectors are untouched (slot 0
 * has no meaning between two solves).  MGX_ERR_STATE where mgx_solve_multi_refine_gcr returns it, and until a
 * mgx_solve_multi_refine_gcr call with at least that nrhs has allocated the pieces; MGX_ERR_INVALID for repeats < 1,
 * nrhs < 1 or nrhs > MGX_MAX_RHS, NULL ms. */
MGX_API int mgx_time_multi_refine_direction(mgx_handle h, int nrhs, int repeats, double* ms);
/* ms per launch of one of mgx_eigs' four passes on its first nev workspace columns, `repeats` launches between two
 * events (tools/eig_bench.py; the yardstick is mgx_time_gcr_pass, UPDATE, in the same run).  Per point and launch:
 * GRAM k_eig_gram<T, nev, nev> of X against [P, AP] with the reduction of its sums, 3 nev words read; COMBINE
 * k_eig_combine<T, 3 nev, nev>, X <- [X, W, P] with the identity on X (X keeps its bits), 3 nev read and nev written;
 * RESIDUAL k_eig_residual<T, nev> with theta = 1 and its reductions, 2 nev read and nev written; APPLY
 * k_apply_var_multi<T, NQ, nev>, AX <- A X, NQ + 2 nev.  The handle's own vectors are untouched (the workspace has no
 * meaning between two calls).  MGX_ERR_STATE where mgx_eigs returns it, and until a mgx_eigs call with at least that
 * nev has allocated the columns; MGX_ERR_INVALID for another pass, repeats < 1, nev < 1 or nev > MGX_MAX_RHS, NULL ms. */
enum { MGX_EIG_PASS_GRAM = 0, MGX_EIG_PASS_COMBINE = 1, MGX_EIG_PASS_RESIDUAL = 2, MGX_EIG_PASS_APPLY = 3 };
MGX_API int mgx_time_eig_pass(mgx_handle h, int pass, int nev, int repeats, double* ms);
/* ms per launch of one pass of mgx_eigs_many's projection of the first k workspace columns (their finest u, where the cycle
 * leaves W) against the first m locked slots, `repeats` launches between two events (tools/eig_many_bench.py; the
 * yardstick is mgx_time_gcr_pass, UPDATE, in the same run).  DOTS: k_eig_project_dots over all chunks of eight locked
 * vectors with the reduction of their sums, m + k ceil(m / 8) words read per point; SUB: k_eig_project_sub, one launch, m + k
 * read and k written, with the coefficient buffer zeroed, so W keeps its bits.  The handle's own vectors are untouched.
 * MGX_ERR_STATE where mgx_eigs_many returns it, and until a mgx_eigs_many call with nev >= m + k has allocated the
 * pieces; MGX_ERR_INVALID for another pass, repeats < 1, m outside 1 .. MGX_EIGS_MAX - 1, k outside 1 .. MGX_MAX_RHS,
 * NULL ms. */
enum { MGX_EIG_PROJECT_DOTS = 0, MGX_EIG_PROJECT_SUB = 1 };
MGX_API int mgx_time_eig_project(mgx_handle h, int pass, int m, int k, int repeats, double* ms);
/* ms per launch of mgx_theta_steps' right-hand-side pass on the handle's own buffers, `repeats` launches between two
 * events (tools/theta_bench.py; the yardstick is k_residual_var<T, NQ, 0, 1>, one word per point fewer, through mgx_residual
 * in the same run): k_theta_rhs<T, 5 | 9, false> for theta < 1 (NQ + 3 words in, 1 out), k_theta_rhs<T, 5, true> for
 * theta = 1 (3 in, 1 out), with a source grid (zeros until a mgx_theta_steps call gave one).  The pass writes into the
 * finest R: U and B keep their bits.  MGX_ERR_STATE where mgx_set_reaction returns it and when no term is set;
 * MGX_ERR_INVALID for theta outside (0, 1], repeats < 1, NULL ms. */
MGX_API int mgx_time_theta_rhs(mgx_handle h, double theta, int repeats, double* ms);
/* ms per launch of mgx_newton's pass (with the reduction of its sums) on the handle's own buffers, `repeats` launches
 * between two events (tools/newton_bench.py; the yardstick is k_residual_var<T, NQ, 0, 1> through mgx_residual in the same
 * run): step = 0 times k_newton_pass<T, NQ, false, false> (NQ + 3 words in, 2 out), step = 1 <T, NQ, true, false> with lam = 1
 * (NQ + 4 in, 3 out), on the iterate, f, kappa and polynomial the last mgx_newton call left and the current U as de.  The pass
 * writes into the finest R, the trial iterate and the next d: U, B, the iterate and the operator keep their bits.
 * MGX_ERR_STATE where mgx_set_reaction returns it and until a mgx_newton call has allocated the workspace;
 * MGX_ERR_INVALID for another step, repeats < 1, NULL ms. */
MGX_API int mgx_time_newton_pass(mgx_handle h, int step, int repeats, double* ms);
/* ms per launch of mgx_newton_steps' passes on the handle's own buffers, `repeats` launches between two events
 * (tools/newton_steps_bench.py; the yardstick is k_residual_var<T, NQ, 0, 1> through mgx_residual in the same run):
 * pass = 0 times k_newton_step_rhs (theta < 1: <T, NQ, false>, NQ + 4 words in, 1 out; theta = 1: <T, 5, true>, 3 in, 1
 * out) with a source grid (zeros until a mgx_newton_steps call gave one); pass = 1 k_newton_pass<T, NQ, false, true> with
 * its reduction (NQ + 4 in, 2 out); pass = 2 <T, NQ, true, true> with lam = 1 (NQ + 5 in, 3 out); theta is read by pass 0
 * only.  They run on the time level, r, mass, kappa and polynomial the last mgx_newton_steps call left and the current U
 * as de, and write into the finest R, the trial iterate and the next d: U, B, the time level and the operator are
 * unchanged.  MGX_ERR_STATE where mgx_set_reaction returns it and until a mgx_newton_steps call has allocated the
 * workspace; MGX_ERR_INVALID for pass outside 0 .. 2, theta outside (0, 1], repeats < 1, NULL ms. */
MGX_API int mgx_time_newton_step_pass(mgx_handle h, int pass, double theta, int repeats, double* ms);
/* ms per launch of mgx_quasi's pass (with the reduction of its sums) on the handle's own buffers, `repeats` launches
 * between two events (tools/quasi_bench.py; the yardstick is k_residual_var<T, 5, 0, 1> through mgx_residual in the same
 * run): step = 0 times k_quasi_pass<T, false, NEWTON> (u, f and the nodal a in - a counts two words in float - five
 * coefficients and b out), step = 1 <T, true, NEWTON> with lam = 1 (de in and the trial out as well); method selects NEWTON.
 * It runs on the iterate, f, nodal a and k the last mgx_quasi call left and the current U as de, and writes b into the
 * finest R, the trial iterate and the second set of coefficient grids: U, B, the iterate and the operator are unchanged.
 * MGX_ERR_STATE where mgx_quasi returns it and until a mgx_quasi call has allocated the workspace; MGX_ERR_INVALID for
 * step outside 0 .. 1, an unknown method, repeats < 1, NULL ms. */
MGX_API int mgx_time_quasi_pass(mgx_handle h, int step, int method, int repeats, double* ms);
MGX_API int mgx_synchronize(mgx_handle h);
/* Number of hipGraphs mgx_solve has captured for its loop body ("one V-cycle +
 * residual norm", PS:727 run to a tolerance): 0 until the first graph cycle,
 * -1 when graph replay is off (cfg.profile = 1, mixed precision, MGX_GRAPH=0,
 * or a failed capture). */
MGX_API int mgx_graphs_cached(mgx_handle h);

/* =============================================================================
 * Slab-level operators on caller-owned device memory.  These are what the
 * multi-GPU driver (one process per GPU, RCCL halo exchange between calls)
 * composes; the single-GPU handle above uses the same kernels.
 *
 * A slab is `rows` consecutive grid rows of one level stored with the level's
 * pitch (mgx_level_pitch), columns 0..N as in the handle (Dirichlet columns
 * and padding must be zero).  Row indices are local to the slab.  `stream` is
 * a hipStream_t passed as void* (NULL = default stream).  dtype is
 * MGX_DTYPE_F32 or MGX_DTYPE_F64.  Calls are asynchronous on `stream`.
 * ===========================================================================*/
typedef struct {
    int level;        /* grid level L: N = 2^L, columns 0..N */
    int dtype;        /* MGX_DTYPE_F32 / MGX_DTYPE_F64 */
    int rows;         /* rows allocated in the slab */
    int row0;         /* global row index of local row 0 */
    int arith;        /* MGX_ARITH_* of the smoother calls (mgx_config.arith) */
} mgx_slab;

/* elements per row for (level, dtype); bytes per row = pitch * sizeof(type) */
MGX_API long mgx_level_pitch(int level, int dtype);

/* mu Jacobi sweeps (PS:125-147) on local rows [row_lo,row_hi), ping-ponging
 * u <-> tmp; with shrink = 1 the range shrinks by one row per sweep at each
 * end that is not a global boundary (deep-halo communication avoidance): the
 * first sweep then covers [row_lo - (mu-1), row_hi + (mu-1)) clipped to the
 * unknown rows.  *result_in_tmp is set to 1 when the block made an odd number of
 * launches: sweeps may be fused, so a block of 10 sweeps run as one pass leaves
 * the result in tmp. */
MGX_API int mgx_slab_jacobi(const mgx_slab* s, void* u, const void* b, void* tmp,
                            int row_lo, int row_hi, int mu, double omega, int shrink,
                            int* result_in_tmp, void* stream);
/* same for red-black Gauss-Seidel; a sweep consumes two halo rows per side */
MGX_API int mgx_slab_rbgs(const mgx_slab* s, void* u, const void* b, void* tmp,
                          int row_lo, int row_hi, int mu, int shrink,
                          int* result_in_tmp, void* stream);
/* mu smoother sweeps (PS:125-147 / red-black GS) on local rows [row_lo,row_hi) with the
 * deep-halo shrinking of mgx_slab_jacobi(shrink = 1) and the V-cycle's transfer operators
 * folded into the passes, as the single-GPU handle does (one pass over the slab per 5 sweeps
 * instead of separate transfer kernels):
 *   coarse_e != NULL : the input is u + P e (PS:620-624), e on the coarse slab `c`;
 *   coarse_b != NULL : the residual of the result is restricted (PS:604-611) into coarse_b,
 *                      local coarse rows [crow_lo,crow_hi) of `c` (row_lo + row0 must be odd);
 *   sum_dev  != NULL : sum over [row_lo,row_hi) of (b - A u)^2 of the result -> *sum_dev
 *                      (scratch as for mgx_slab_residual_sumsq).
 * At most one of coarse_b / sum_dev.  The rows the passes read must hold valid data:
 * per*mu rows beyond the range, +2 with coarse_b, +1 with sum_dev (per = 1 Jacobi, 2 RB-GS),
 * and with coarse_e the coarse rows around them.
 * zero_in != 0 : the input iterate is known to be all zero (PS:613: the guess of a coarse-grid correction) and
 *                is NOT read - nobody has to write those zeros first; u is then scratch for the passes' ping-pong.
 *                Not with coarse_e; MGX_ERR_INVALID when the first pass cannot synthesise its input (mu = 1).
 * smoother: MGX_SMOOTHER_JACOBI or MGX_SMOOTHER_RBGS; restrict_mode: MGX_RESTRICT_CONSISTENT or MGX_RESTRICT_FW16
 * (the injection modes are single-GPU only) - any other value is MGX_ERR_INVALID. */
MGX_API int mgx_slab_cycle(const mgx_slab* f, void* u, const void* b, void* tmp,
                           int row_lo, int row_hi, int mu, double omega, int smoother,
                           const mgx_slab* c, const void* coarse_e, void* coarse_b,
                           int crow_lo, int crow_hi, int restrict_mode, int zero_in,
                           double* scratch, double* sum_dev, int* result_in_tmp, void* stream);
/* fused residual + restriction (PS:604-611) of fine slab `f` into coarse slab
 * `c`, coarse local rows [crow_lo,crow_hi); zero_u (may be NULL) is the coarse
 * solution slab to zero on the same rows (PS:613).  restrict_mode as for
 * mgx_slab_cycle: CONSISTENT or FW16, anything else is MGX_ERR_INVALID. */
MGX_API int mgx_slab_restrict(const mgx_slab* f, const void* u, const void* b,
                              const mgx_slab* c, void* cb, void* zero_u,
                              int crow_lo, int crow_hi, int restrict_mode, int fused, void* stream);
/* u[fine rows row_lo..row_hi) (+)= P e  (PS:337-425, 620-624) */
MGX_API int mgx_slab_prolong(const mgx_slab* f, void* u, const mgx_slab* c, const void* e,
                             int row_lo, int row_hi, int add, void* stream);
/* sum over rows [row_lo,row_hi) of (b - A u)^2 -> *partial_sum_dev (device
 * double, written asynchronously); scratch must hold mgx_slab_scratch_doubles(). */
MGX_API int mgx_slab_residual_sumsq(const mgx_slab* s, const void* u, const void* b,
                                    int row_lo, int row_hi, double* scratch, double* sum_dev, void* stream);
MGX_API long mgx_slab_scratch_doubles(const mgx_slab* s);


/* =============================================================================
 * Multi-GPU: the slab plan as data, ranks, transports.
 *
 * mgx_create with cfg.n_gpus > 1 drives every slab from ONE process (one host thread, a stream
 * pair per device).  mgx_create_rank is the one-process-per-GPU form (torch.distributed.run /
 * mpirun launch `world` processes): this process owns slab `rank` and talks to its neighbours
 * through `transport` - NULL selects the built-in RCCL transport, which needs the 128-byte
 * ncclUniqueId of rank 0 (mgx_rccl_unique_id) handed to every rank by the launcher.
 * On such handles: mgx_set_rhs / mgx_set_guess / mgx_get_solution (whole-grid host vectors; each
 * slab takes / returns its rows), mgx_fill_rhs, mgx_fill_guess_random, mgx_residual_norm (finest
 * level), mgx_vcycle (finest level), mgx_fmg, mgx_solve, mgx_synchronize, mgx_destroy; everything
 * else returns MGX_ERR_STATE.
 * ===========================================================================*/
enum {
    MGX_DOP_EXCHANGE = 1,       /* fill `depth` halo rows of `which` (U / B) of `level` from both neighbours */
    MGX_DOP_ZERO_U = 2,         /* zero the coarse guess slab of `level` (PS:613) */
    MGX_DOP_CYCLE = 3,          /* mgx_slab_cycle: mu sweeps on [row_lo,row_hi) with folded transfers (pre / post) */
    MGX_DOP_SMOOTH = 4,         /* mgx_slab_jacobi / _rbgs, shrink = 1 */
    MGX_DOP_RESTRICT = 5,       /* mgx_slab_restrict, fused residual, coarse rows [crow_lo,crow_hi) */
    MGX_DOP_PROLONG = 6,        /* mgx_slab_prolong, add = 1, fine rows [row_lo,row_hi) */
    MGX_DOP_GATHER_CUT = 7,     /* all-gather the slabs' shares of the cut level's right-hand side */
    MGX_DOP_COARSE = 8,         /* one V-cycle from e = 0 on levels cut..coarsest (replicated) */
    MGX_DOP_SUMSQ = 9,          /* sum of (b - A u)^2 over rows [row_lo,row_hi) of the finest level */
    MGX_DOP_ALLREDUCE_NORM = 10,/* sum the slabs' sums of squares; the norm is its square root */
    /* fullmultigrid on slabs (PS:629-650) */
    MGX_DOP_RESTRICT_RHS = 11,  /* B[level-1] = R B[level] (PS:641), coarse rows [crow_lo,crow_hi) */
    MGX_DOP_PROLONG_SET = 12,   /* U[level] = P U[level-1] (PS:645) on fine rows [row_lo,row_hi) */
    MGX_DOP_COARSE_FMG = 13     /* fullmultigrid on levels cut..coarsest from the gathered right-hand side (replicated) */
};
typedef struct {
    int op, level;
    int which, depth;           /* EXCHANGE */
    int row_lo, row_hi, mu;     /* CYCLE / SMOOTH / PROLONG / SUMSQ: local rows of the slab of `level` */
    int pre;                    /* CYCLE: 1 = the input is u + P e (PS:620-624) */
    int post;                   /* CYCLE: 1 = restrict the residual of the result (PS:604-611), 2 = sum its squares */
    int crow_lo, crow_hi;       /* CYCLE post 1 / RESTRICT: local coarse rows produced */
    int coarse_is_cut;          /* the level below is the cut level (this slab's share / the gathered grid) */
} mgx_dist_op;
typedef struct {
    int level, N;               /* N = 2^level: rows 0..N */
    int own_lo, own_hi;         /* global rows owned: [own_lo, own_hi) */
    int halo;                   /* halo rows allocated per side */
    int row0, rows;             /* global row of local row 0, rows allocated */
} mgx_dist_level;

/* The plan of slab `g` of `n_slabs` for cfg (cfg.n_gpus is ignored, cfg.cut_level 0 = default):
 * pure host logic, no device needed - the CPU tests run these plans over numpy and gloo. */
typedef struct mgx_dist_planner* mgx_plan_handle;
MGX_API int mgx_plan_create(const mgx_config* cfg, int n_slabs, int g, int fold, int deep, mgx_plan_handle* out);
MGX_API int mgx_plan_destroy(mgx_plan_handle p);
MGX_API const char* mgx_plan_last_error(void);
MGX_API int mgx_plan_cut_level(mgx_plan_handle p);
/* geometry of the slab of `level` (cut < level <= finest) */
MGX_API int mgx_plan_level(mgx_plan_handle p, int level, mgx_dist_level* out);
/* this slab's share of the cut level: rows [row0, row0 + rows) */
MGX_API int mgx_plan_cut_share(mgx_plan_handle p, int* row0, int* rows);
/* the caller refilled u of the finest level: all rows incl. halos (all_rows = 1) or owned rows only */
MGX_API int mgx_plan_guess_set(mgx_plan_handle p, int all_rows);
/* operations of one V-cycle / of the residual norm, in order; returns the count (< 0: cap too small) */
MGX_API int mgx_plan_vcycle(mgx_plan_handle p, mgx_dist_op* ops, int cap);
MGX_API int mgx_plan_norm(mgx_plan_handle p, mgx_dist_op* ops, int cap);
/* operations of fullmultigrid (PS:629-650): right-hand sides restricted down to the cut level, FMG on
 * the replicated levels, then per slab level prolongation + mu0 + 1 V-cycles */
MGX_API int mgx_plan_fmg(mgx_plan_handle p, mgx_dist_op* ops, int cap);

/* what moves between slabs of different processes */
typedef struct { int send; int peer; void* ptr; size_t bytes; } mgx_xfer;   /* send = 1: ptr -> peer; 0: peer -> ptr */
typedef struct {
    void* ctx;
    /* every transfer of one halo exchange; device pointers; must be complete, or ordered on `stream`
     * (a hipStream_t), when the call returns */
    int (*sendrecv)(void* ctx, int n, const mgx_xfer* x, void* stream);
    /* recv[r * bytes .. ) = rank r's send[0 .. bytes); device pointers, same completion rule */
    int (*allgather)(void* ctx, const void* send, void* recv, size_t bytes, void* stream);
    /* *value = sum over ranks of *value (host double) */
    int (*allreduce_sum)(void* ctx, double* value);
} mgx_transport;
/* 128 bytes identifying a new RCCL communicator (ncclGetUniqueId); rank 0 calls it, the launcher
 * distributes the bytes */
MGX_API int mgx_rccl_unique_id(void* out128);
/* One rank of `world` (one process per GPU).  transport = NULL: built-in RCCL (rccl_id = the 128
 * bytes of mgx_rccl_unique_id from rank 0); otherwise the caller's transport (rccl_id ignored).
 * cfg.op must be MGX_OPERATOR_POISSON (MGX_ERR_INVALID otherwise: the general operators are single-GPU). */
MGX_API int mgx_create_rank(const mgx_config* cfg, int rank, int world, const void* rccl_id,
                            const mgx_transport* transport, mgx_handle* out);
/* number of halo exchanges a multi-GPU handle has performed (tests: communication plan) */
MGX_API long mgx_dist_exchanges(mgx_handle h);
/* how many of them ran on the slab's second stream beside the rows of the following smoothing pass that
 * need no halo (the pass then finishes with its two edge bands).  Opt-in, MGX_DIST_OVERLAP=1: a band is a
 * 10-level launch of ~50 us however thin it is, more than a halo message of this size takes */
MGX_API long mgx_dist_overlapped(mgx_handle h);
/* The ROCm runtime libraries this process has mapped (libamdhip64, libhsa-runtime64, librccl, libmgx ...), one
 * path per line, from /proc/self/maps.  libmgx is built against /opt/rocm (RUNPATH); a host application that
 * loaded another copy with the same SONAME first - the torch wheel bundles its own - would run this library on
 * that stack.  bench.py reports the list (`runtime_libs`); MGX_LOG_RUNTIME_LIBS=1 prints it at every
 * mgx_create / mgx_create_rank.  Returns the bytes written (without the terminator), < 0 on error. */
MGX_API int mgx_runtime_libs(char* buf, size_t cap);
/* plain copies for callers that implement a transport without a HIP binding of their own */
MGX_API int mgx_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
MGX_API int mgx_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGX_H */
