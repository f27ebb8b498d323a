// mgx.hip — libmgx: solver handle, V-cycle / FMG schedules and the C-ABI
// (include/mgx.h) over the gfx950 kernels of mgx_kernels.hpp and their launch wrappers /
// pass planner of mgx_launch.hpp.
//
// Reference map (PS = Poissons_SYCL.cpp, MF = Multigrid_functions.cpp):
//   Solver / Level      PS:24-33 matrix_elements_for_jacobi + jacobi_matrices[],
//                       MF:16-26 ProblemVar   (matrix-free: arrays, no CSR)
//   Solver::vcycle      PS:575-627 vcyclemultigrid / MF:132-173
//   Solver::fmg         PS:629-650 fullmultigrid   / MF:175-191
//   mgx_solve           PS:727 (main's call) / MF:193-197 multigrid_solver
//   mgx_solve_pcg       (absent in the reference) CG preconditioned by one V-cycle, mgx_krylov.hpp
//   mgx_solve_gcr       (absent in the reference) restarted GCR around one cycle, mgx_krylov.hpp
//   mgx_solve_refine    (absent in the reference) fp64 defect correction around the cycle of a float copy of the
//                       hierarchy, mgx_refine.hpp
//   mgx_solve_refine_gcr  (absent in the reference) fp64 restarted GCR around that float cycle, mgx_refine_gcr.hpp
//   mgx_solve_multi     (absent in the reference) mgx_solve's cycle loop on up to four right-hand sides per operator
//                       read, mgx_multi.hpp
//   mgx_solve_multi_gcr (absent in the reference) mgx_solve_gcr's iteration on those columns, around that cycle
//   mgx_solve_multi_refine_gcr  (absent in the reference) mgx_solve_refine_gcr's iteration on those columns, around the
//                       float block cycle
// The host side of the last seven is in mgx_krylov_host.hpp (the Krylov passes, driver and entry-point body of all that
// iterate), mgx_refine_host.hpp, mgx_multi_host.hpp and mgx_multi_refine_host.hpp; only their extern "C" entry points
// are here.
// There is no CPU fallback anywhere in this file.

#include "../../include/mgx.h"
#include "mgx_bottom.hpp"
#include "mgx_kernels.hpp"
#include "mgx_launch.hpp"
#include "mgx_var.hpp"
#include "mgx_galerkin.hpp"
#include "mgx_opdep.hpp"
#include "mgx_cheby.hpp"
#include "mgx_line.hpp"
#include "mgx_colour.hpp"
#include "mgx_small.hpp"
#include "mgx_krylov.hpp"
#include "mgx_refine.hpp"
#include "mgx_refine_gcr.hpp"
#include "mgx_multi.hpp"
#include "mgx_eig.hpp"
#include "mgx_eig_many.hpp"
#include "mgx_theta.hpp"
#include "mgx_newton.hpp"
#include "mgx_quasi.hpp"
#include "mgx_dist_plan.hpp"

#include <chrono>
#include <unistd.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

using namespace mgx;

thread_local std::string g_create_error;

// MGX_LOG_RUNTIME_LIBS=1: print the mapped ROCm runtime libraries when a handle is created (mgx_runtime_libs)
void log_runtime_libs(const char* where)
{
    if (env_int("MGX_LOG_RUNTIME_LIBS", 0) == 0) return;
    char buf[8192];
    if (mgx_runtime_libs(buf, sizeof buf) >= 0)
        std::fprintf(stderr, "[mgx] runtime libraries mapped at %s (pid %d):\n%s", where, (int)getpid(), buf);
}

struct Level {
    int L = 0, N = 0, rows = 0;
    long pitch = 0;
    size_t bytes = 0;
    bool f64 = true;
    void *u = nullptr, *b = nullptr, *tmp = nullptr, *r = nullptr;
    // MGX_OPERATOR_STENCIL5 / GALERKIN (mgx_var.hpp), in the slot order c, n, s, w, e, nw, ne, sw, se: the operator A
    // [ProblemVar::A_sp_dict, MF:19] and its Jacobi splitting J = (D_inv, R_n, R_s, ..., R_se)  [A_jacobi_sp_dict, MF:20,
    // 28-32].  The corner slots 5..8 exist on the levels below the finest GALERKIN level (R A P) and, from the first
    // mgx_set_stencil9 / mgx_set_tensor on, on the finest one; `nine`: the level's current operator is nine-point (the
    // NQ = 5 instances never read slots 5..8)
    void* A[9] = {};
    void* J[9] = {};
    // MGX_TRANSFER_OPERATOR (mgx_opdep.hpp): the eight weight grids (n, s, w, e, nw, ne, sw, se) of P between level
    // L + 1 and this level, allocated by the first OPERATOR build
    void* wt[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool nine = false;
    bool stencil_set = false;
    // MGX_SMOOTHER_CHEBYSHEV (mgx_cheby.hpp): the direction d of a smoothing block (allocated at create for that smoother
    // only) and, for either smoother, the bound g_l of the spectrum of D^-1 A of the level's current operator
    void* cheb = nullptr;
    double lambda_g = 0.0;
    // MGX_SMOOTHER_LINE_* (mgx_line.hpp): the Thomas factors m, g of the level's x-lines [0] and y-lines [1] and the
    // homogeneous factors hf, hb of k_line_y's chunks of line_R rows; allocated at create for the directions the handle
    // smooths in, rebuilt with the operator (line_update)
    void *line_m[2] = {nullptr, nullptr}, *line_g[2] = {nullptr, nullptr}, *line_hf = nullptr, *line_hb = nullptr;
    int line_R = 0;
    size_t esize() const { return f64 ? 8 : 4; }
};

struct EventPair { hipEvent_t a, b; int cls; long long launches; long long sweeps; hipEvent_t a_use; };   // a_use: the event the span starts at (a, or the previous span's b)

} // namespace

struct mgx_solver {
    mgx_config cfg{};
    hipStream_t stream = nullptr;
    std::vector<Level> lv;          // working hierarchy, index = level (only [coarsest..finest] valid)
    Level fine64;                   // MIXED only: double u, b (and r) on the finest level
    bool mixed = false;
    bool work_f64 = true;           // element type of the working hierarchy
    BottomDST bottom;
    double* partial = nullptr;      // per-block partial sums
    long partial_cap = 0;
    double* sum_dev = nullptr;      // reduced sum (device)
    double* sum_host = nullptr;     // pinned
    std::string err;
    int rows_per_chunk = 0;         // 0 = auto (MGX_ROWS env overrides)
    FuseCfg fuse{10, 0, 256, 10, 10, 1024, 10, 10};   // temporal fusion knobs (MGX_FUSE, MGX_FUSE_ROWS, MGX_FUSE_MIN_N, MGX_FOLD_KMAX[_BIG])
    // profiling
    std::vector<EventPair> ev_used, ev_free;
    double prof_ms[MGX_PROF_COUNT] = {0};
    long long prof_launches[MGX_PROF_COUNT] = {0};
    long long prof_sweeps[MGX_PROF_COUNT] = {0};
    int last_smooth_launches = 0;   // launches made by the most recent smoothing block
    int fold = 1;                   // fold transfers / norm into smoother passes (MGX_FOLD)
    int use_zero_in = 1;            // let first passes synthesise a known-zero iterate (MGX_ZERO_IN)
    int norm_blocks_ready = 0;      // > 0: partial[] holds that many sums of r^2 for the current U
    double fine_updates = 0.0;
    // hipGraph replay of "one V-cycle + residual norm" (profiling off) or of the cycle below the finest level
    // (cfg.profile = 2): one cache, cached_graph()
    struct CycleGraph {
        std::vector<void*> before, after;   // u / tmp of every level before and after the cycle
        hipGraphExec_t exec = nullptr;
        double fine_updates = 0.0;
    };
    std::vector<CycleGraph> graphs;
    int use_graph = 1;              // MGX_GRAPH
    bool prof_mute = false;         // inside a stream capture: no events (they carry no time stamps there)
    // cfg.profile = 2: the spans of one cycle follow one another with nothing enqueued in between, so the end event of a span is
    // the start of the next (an event record costs ~4 us of GPU time: 8 per cycle were 2.5 % of it, 5 are 1.6 %)
    bool prof_chain = false;
    hipEvent_t chain_ev = nullptr;
    int mixed_fuse = 1;             // mixed precision: u += s e and the residual in one pass (MGX_MIXED_FUSE)
    // general per-level operators: dense inverse of the coarsest one (MF:18 coarsest_level_matrix, MF:63-72)
    double *var_M = nullptr, *var_inv = nullptr, *var_pm = nullptr, *var_pi = nullptr;
    bool var = false;               // cfg.op == MGX_OPERATOR_STENCIL5 or MGX_OPERATOR_GALERKIN
    bool galerkin = false;          // cfg.op == MGX_OPERATOR_GALERKIN: coarse operators are R A P (mgx_build_galerkin)
    bool gal_built = false;         // ... and have been built from the current finest operator
    int cycle = MGX_CYCLE_V;        // cycle index of every cycle the handle runs (mgx_set_cycle): V, W or F
    int small_visit = 1;            // W / F: one-workgroup visits of the small nine-point levels (MGX_SMALL_VISIT, mgx_small.hpp)
    int small_max_n = kSmallMaxN;   // ... of the levels with N <= this
    int line_dirs = 0;              // MGX_SMOOTHER_LINE_*: bit 0 x-lines, bit 1 y-lines (0: another smoother)
    int colour = 0;                 // MGX_SMOOTHER_COLOR_GS: 1, COLOR_SGS: 2 (post-smoothing blocks in reverse colour order); 0: another smoother
    int gs_fused = 1;               // ... five-point levels sweep both colours in one launch of k_gs_rb (MGX_GS_FUSED, mgx_colour.hpp)
    int* line_flag = nullptr;       // device: bit d raised by k_line_factor on a zero or non-finite pivot in direction d
    int transfer = MGX_TRANSFER_BILINEAR;   // ... with this prolongation (mgx_build_galerkin_transfer)
    // mgx_solve_pcg and mgx_solve_gcr (mgx_krylov_host.hpp): one workspace, every piece allocated by the first call
    // that needs it.  Both methods run on the one scalar block, PCG on its first kPcgScalars slots, and neither
    // depends on what the other left there: GCR zeroes the block before it starts; PCG's kPcgInit reduction writes
    // rho, beta and the breakdown flag before anything reads them; alpha and ||r||^2 are written before they are
    // read in every iteration; mgx_time_gcr_pass zeroes the block and leaves it zeroed.
    struct KrylovWs {
        void *x = nullptr, *b = nullptr;            // the iterate; the caller's b while r occupies lv[finest].b
        void *p[2] = {nullptr, nullptr}, *q = nullptr;               // PCG: the directions p / p' (ping-pong), q = A p
        void *Z[kGcrMaxRestart] = {}, *Q[kGcrMaxRestart] = {};       // GCR: the basis pairs Z_i, Q_i = A Z_i (restart of them)
        double* part = nullptr;                     // per-block partials of one pass, sized for the widest (k_gcr_dots<T, 7>)
        long part_cap = 0;
        double *sc = nullptr, *sc_host = nullptr;   // kGcrScalars device scalars (mgx_krylov.hpp) and their pinned host copy
        int vecs(mgx_solver* s, std::initializer_list<void**> vs, size_t bytes);
        int shared(mgx_solver* s, size_t bytes, int blocks);
        void free();
    } kry;
    struct mgx_dist* dist = nullptr; // multi-GPU handle (cfg.n_gpus > 1 / mgx_create_rank): mgx_dist.hpp; no levels of its own
    // mgx_solve_refine: the float copy of a general-operator F64 handle's hierarchy, an F32 solver of the same cfg and
    // knobs on the parent's stream (own_stream = false there), created by the first call.  op_gen counts the changes of
    // the handle's operator or hierarchy (operator_changed); the shadow holds the operator of generation shadow_gen and
    // is rebuilt when the two differ (< 0: never built)
    mgx_solver* shadow = nullptr;
    long long op_gen = 0, shadow_gen = -1;
    bool own_stream = true;
    // mgx_solve_multi: MGX_MAX_RHS columns of u, tmp, b, r on every level (index = level, then column), each column's
    // per-block sums of r^2 and the reduced sums with their pinned copy; columns [0, cols) exist.  Allocated by the first
    // call, grown by a call with more columns, freed by mgx_destroy.  No copy of the operator: nothing to invalidate
    struct MultiWs {
        struct Grids { void *u[MGX_MAX_RHS] = {}, *tmp[MGX_MAX_RHS] = {}, *b[MGX_MAX_RHS] = {}, *r[MGX_MAX_RHS] = {}; };
        std::vector<Grids> lv;
        double* part[MGX_MAX_RHS] = {};
        double *sums = nullptr, *sums_host = nullptr;
        int cols = 0;
        // mgx_solve_multi_gcr, per column beyond the above: the iterate x, the basis pairs Z_i, Q_i = A Z_i of the finest
        // level (as many as the largest restart so far), the partial sums of one Krylov pass (sized like KrylovWs::part)
        // and a block of kGcrScalars doubles - the blocks of all columns contiguous in gsc, one pinned mirror gsc_host
        void* x[MGX_MAX_RHS] = {};
        void *Z[MGX_MAX_RHS][kGcrMaxRestart] = {}, *Q[MGX_MAX_RHS][kGcrMaxRestart] = {};
        double* gpart[MGX_MAX_RHS] = {};
        double *gsc = nullptr, *gsc_host = nullptr;
    } multi;
    // mgx_eigs (mgx_eig_host.hpp), per column beyond mgx_solve_multi's: X, AX, AW, P, AP of the finest level (W is the
    // column's finest u, R its finest b); the per-block sums of one Gram pair and the sums of the six pairs of an
    // iteration with their pinned copy.  Columns [0, cols) exist; allocated by the first call, grown by a larger nev,
    // freed by mgx_destroy
    struct EigWs {
        void *X[MGX_MAX_RHS] = {}, *AX[MGX_MAX_RHS] = {}, *AW[MGX_MAX_RHS] = {}, *P[MGX_MAX_RHS] = {}, *AP[MGX_MAX_RHS] = {};
        double *gpart = nullptr, *gsum = nullptr, *gsum_host = nullptr;
        int cols = 0;
    } eig;
    // mgx_eigs_many (mgx_eig_many_host.hpp), beyond mgx_eigs' workspace: the locked vectors Y of the finest level, the
    // device table of their pointers, the MGX_EIGS_MAX x MGX_MAX_RHS coefficients of a projection and the per-block sums
    // of one chunk of its dots.  Slots [0, slots) exist; allocated by the first call, grown by a larger nev, freed by
    // mgx_destroy
    struct EigManyWs {
        void* Y[MGX_EIGS_MAX] = {};
        void** ytab = nullptr;
        double *coef = nullptr, *part = nullptr;
        int slots = 0;
    } eigm;
    // mgx_set_reaction / mgx_theta_steps (mgx_theta_host.hpp), grids of the finest level with ring and padding zero: c0
    // the centre of the finest operator as the last operator call gave it, d the zero-order term (A[0] = c0 + d while
    // `set`), g the source of the theta steps.  c0 and d are allocated by the first mgx_set_reaction, g by the first
    // mgx_theta_steps with a source; kept until mgx_destroy
    struct ReactionWs {
        void *c0 = nullptr, *d = nullptr, *g = nullptr;
        bool set = false;
    } rx;
    // mgx_newton (mgx_newton_host.hpp), grids of the finest level with ring and padding zero: the iterate un and the trial
    // ut (swapped when a trial is accepted), the caller's f while B holds the step's right-hand side, kappa, and the
    // Jacobian's diagonal term dn the pass writes (swapped with rx.d before a step's shift); p1..p3 of the last call for
    // mgx_time_newton_pass.  Allocated by the first mgx_newton, kept until mgx_destroy.  mgx_newton_steps
    // (mgx_newton_steps_host.hpp) runs on the same grids - un the time level, f the step's r - and adds the mass term dm
    // and, with its first source, g
    struct NewtonWs {
        void *un = nullptr, *ut = nullptr, *f = nullptr, *kap = nullptr, *dn = nullptr, *dm = nullptr, *g = nullptr;
        double p1 = 0.0, p2 = 0.0, p3 = 0.0;
    } nwt;
    // mgx_quasi (mgx_quasi_host.hpp), grids of the finest level with ring and padding zero: the iterate un and the trial ut
    // (swapped when a trial is accepted), the caller's f while B holds the step's right-hand side, the five coefficient
    // grids A2 the pass writes (swapped with the level's A[0 .. 4] when an iteration makes them the operator), and the
    // nodal coefficient an, doubles in the level's rows and pitch with the boundary nodes; k0 .. k2 of the last call for
    // mgx_time_quasi_pass.  Allocated by the first mgx_quasi, kept until mgx_destroy
    struct QuasiWs {
        void *un = nullptr, *ut = nullptr, *f = nullptr, *A2[5] = {};
        double* an = nullptr;
        double k0 = 0.0, k1 = 0.0, k2 = 0.0;
    } qsi;

    int fail(int code, const std::string& m) { err = m; return code; }
};

namespace {

#define HIPCHK(h, expr)                                                                  \
    do {                                                                                 \
        hipError_t e__ = (expr);                                                         \
        if (e__ != hipSuccess)                                                           \
            return (h)->fail(MGX_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

// ---- profiling scopes ---------------------------------------------------------
struct Prof {
    mgx_solver* s; int idx = -1;
    // on = false: no scope (cfg.profile covers the handle's own column, not a block call's columns)
    Prof(mgx_solver* s_, int cls, long long launches, bool on = true) : s(s_)
    {
        static const bool mute_all = env_int("MGX_PROF_MUTE", 0) != 0;      // experiment: the split submission of cfg.profile = 2 without its events
        if (!on || !s->cfg.profile || s->prof_mute || mute_all) return;
        EventPair p;
        if (!s->ev_free.empty()) { p = s->ev_free.back(); s->ev_free.pop_back(); }
        else {
            // timing only: no system-scope fence when the event completes (MGX_PROF_EVENT_FLAGS=0: plain events)
            static const unsigned flags = env_int("MGX_PROF_EVENT_FLAGS", 1) ? hipEventDisableSystemFence : hipEventDefault;
            if (hipEventCreateWithFlags(&p.a, flags) != hipSuccess || hipEventCreateWithFlags(&p.b, flags) != hipSuccess) return;
        }
        p.cls = cls; p.launches = launches; p.sweeps = 0;
        p.a_use = p.a;
        if (s->prof_chain && s->chain_ev) p.a_use = s->chain_ev;
        else (void)hipEventRecord(p.a, s->stream);
        s->ev_used.push_back(p);
        idx = (int)s->ev_used.size() - 1;
    }
    void set(long long launches, long long sweeps)
    {
        if (idx >= 0) { s->ev_used[idx].launches = launches; s->ev_used[idx].sweeps = sweeps; }
    }
    ~Prof()
    {
        if (idx < 0) return;
        (void)hipEventRecord(s->ev_used[idx].b, s->stream);
        if (s->prof_chain) s->chain_ev = s->ev_used[idx].b;
    }
};

int prof_collect(mgx_solver* s)
{
    if (s->ev_used.empty()) return MGX_OK;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    for (auto& p : s->ev_used) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a_use, p.b) == hipSuccess) {
            s->prof_ms[p.cls] += ms;
            s->prof_launches[p.cls] += p.launches;
            s->prof_sweeps[p.cls] += p.sweeps;
        }
        s->ev_free.push_back(p);
    }
    s->ev_used.clear();
    s->chain_ev = nullptr;
    return MGX_OK;
}

// ---- device-side fills -------------------------------------------------------------
template <typename T>
__global__ void k_fill_rhs(T* b, int N, long pitch, int kind, double f)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c > N || r > N) return;
    const double h = 1.0 / (double)N;
    double v = 0.0;
    if (r >= 1 && r < N && c >= 1 && c < N) {
        if (kind == 0) v = f * h * h;                                   // PS:283-335 (sign: D1)
        else v = h * h * 8.0 * 9.869604401089358 * sinpi(2.0 * c * h) * sinpi(2.0 * r * h);
    }
    b[(long)r * pitch + c] = (T)v;
}

__device__ inline uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

template <typename T>
__global__ void k_fill_random(T* u, int N, long pitch, uint64_t seed)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (c > N || r > N) return;
    double v = 0.0;
    if (r >= 1 && r < N && c >= 1 && c < N) {
        const uint64_t idx = (uint64_t)(r - 1) * (uint64_t)(N - 1) + (uint64_t)(c - 1);  // PS:227 numbering
        const uint64_t x = splitmix64(seed ^ splitmix64(idx));
        v = (double)(x >> 11) * (1.0 / 4503599627370496.0) - 1.0;
    }
    u[(long)r * pitch + c] = (T)v;
}

// ---- level helpers ------------------------------------------------------------------
int alloc_level(mgx_solver* s, Level& l, int level, bool f64)
{
    l.L = level;
    l.N = 1 << level;
    l.rows = l.N + 1;
    l.f64 = f64;
    l.pitch = level_pitch(level, f64 ? MGX_DTYPE_F64 : MGX_DTYPE_F32);
    l.bytes = (size_t)l.rows * (size_t)l.pitch * l.esize();
    for (void** p : {&l.u, &l.b, &l.tmp}) {
        if (hipMalloc(p, l.bytes) != hipSuccess) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for level arrays");
        HIPCHK(s, hipMemsetAsync(*p, 0, l.bytes, s->stream));
    }
    return MGX_OK;
}

void free_level(Level& l)
{
    std::vector<void**> all = {&l.u, &l.b, &l.tmp, &l.r, &l.cheb, &l.line_m[0], &l.line_m[1], &l.line_g[0], &l.line_g[1], &l.line_hf, &l.line_hb};
    for (int q = 0; q < 9; ++q) { all.push_back(&l.A[q]); all.push_back(&l.J[q]); }
    for (void*& w : l.wt) all.push_back(&w);
    for (void** p : all) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

int ensure_r(mgx_solver* s, Level& l)
{
    if (l.r) return MGX_OK;
    if (hipMalloc(&l.r, l.bytes) != hipSuccess) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for residual array");
    HIPCHK(s, hipMemsetAsync(l.r, 0, l.bytes, s->stream));
    return MGX_OK;
}

bool level_ok(const mgx_solver* s, int level)
{
    return level >= s->cfg.coarsest_level && level <= s->cfg.finest_level;
}

// interior (n x n, reference layout) <-> padded grid
int copy_in(mgx_solver* s, Level& l, void* dst_grid, const void* src, size_t count)
{
    const size_t n = (size_t)l.N - 1;
    if (count != n * n) return s->fail(MGX_ERR_INVALID, "vector length must be n*n with n = 2^level - 1");
    const size_t es = l.esize();
    char* d = reinterpret_cast<char*>(dst_grid) + ((size_t)l.pitch + 1) * es;   // (row 1, col 1)
    HIPCHK(s, hipMemcpy2DAsync(d, (size_t)l.pitch * es, src, n * es, n * es, n, hipMemcpyHostToDevice, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return MGX_OK;
}

int copy_out(mgx_solver* s, Level& l, const void* src_grid, void* dst, size_t count)
{
    const size_t n = (size_t)l.N - 1;
    if (count != n * n) return s->fail(MGX_ERR_INVALID, "vector length must be n*n with n = 2^level - 1");
    const size_t es = l.esize();
    const char* p = reinterpret_cast<const char*>(src_grid) + ((size_t)l.pitch + 1) * es;
    HIPCHK(s, hipMemcpy2DAsync(dst, n * es, p, (size_t)l.pitch * es, n * es, n, hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return MGX_OK;
}

// ---- operators on the working hierarchy -----------------------------------------------
inline bool tile_level(const mgx_solver* s, const Level& l) { return s->fuse.tile_max_n > 0 && l.N <= s->fuse.tile_max_n; }

// the plan request of a smoothing block on a whole level: the slab of all its rows, register tiles for levels of
// N <= tile_max_n
BlockReq level_req(const mgx_solver* s, const Level& l, int mu, bool pre, int post, bool zero_in, int rpc)
{
    BlockReq q{s->cfg.smoother, l.f64, l.N, 0, l.rows, 1, l.N, mu, pre, post, zero_in};
    q.tile_points = (long)(s->fuse.tile_max_n - 1) * s->fuse.tile_max_n;
    q.rpc = rpc;
    return q;
}

// ---- general per-level operators (cfg.op = MGX_OPERATOR_STENCIL5; kernels in mgx_var.hpp) ---------------
int var_alloc_level(mgx_solver* s, Level& l)
{
    for (int q = 0; q < (l.nine ? 9 : 5); ++q)
        for (void** p : {&l.A[q], &l.J[q]}) {
            if (hipMalloc(p, l.bytes) != hipSuccess)
                return s->fail(MGX_ERR_ALLOC, q < 5 ? "hipMalloc failed for the operator's coefficient arrays"
                                                    : "hipMalloc failed for the nine-point operator's corner arrays");
            HIPCHK(s, hipMemsetAsync(*p, 0, l.bytes, s->stream));
        }
    return MGX_OK;
}

// the corner arrays A[5..8], J[5..8] of the finest GALERKIN level, allocated and zeroed by the first nine-point finest
// operator and kept until mgx_destroy.  Nothing is launched before all eight exist: a failure leaves the level's
// operator, `nine` and the hierarchy as they were (arrays already allocated stay for the next attempt)
int finest_corners(mgx_solver* s, Level& l)
{
    for (int q = 5; q < 9; ++q)
        for (void** p : {&l.A[q], &l.J[q]}) {
            if (*p) continue;
            if (hipMalloc(p, l.bytes) != hipSuccess) { *p = nullptr; return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for the nine-point operator's corner arrays"); }
            HIPCHK(s, hipMemsetAsync(*p, 0, l.bytes, s->stream));         // the ring and the padding stay zero from here on
        }
    return MGX_OK;
}

// dense inverse of the NN x NN matrix in var_M (k_var_dense_fill wrote it) into var_inv
void gj_invert(mgx_solver* s, int NN)
{
    for (int k = 0; k < NN; ++k) {
        hipLaunchKernelGGL(k_gj_prow, dim3((NN + 255) / 256), dim3(256), 0, s->stream, s->var_M, s->var_inv, s->var_pm, s->var_pi, NN, k);
        hipLaunchKernelGGL(k_gj_elim, dim3(NN), dim3(256), 0, s->stream, s->var_M, s->var_inv, s->var_pm, s->var_pi, NN, k);
    }
}

void drop_graphs(mgx_solver* s)
{
    for (auto& g : s->graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    s->graphs.clear();
}

// the handle's operator or hierarchy is no longer what it was: captured cycles are cycles of the old problem, and the
// float copy of mgx_solve_refine is stale
void operator_changed(mgx_solver* s)
{
    ++s->op_gen;
    drop_graphs(s);
}

template <typename T> Op9<T> op9_of(const Level& l)
{
    Op9<T> o;
    for (int q = 0; q < 9; ++q) o.a[q] = (const T*)l.A[q];
    return o;
}
template <typename T> Op9<T> jac9_of(const Level& l)      // slot 0 is D_inv (the diagonal of R_omega is a scalar)
{
    Op9<T> o;
    for (int q = 0; q < 9; ++q) o.a[q] = (const T*)l.J[q];
    return o;
}
template <typename T> Op9Out<T> out9(const Op9<T>& o)
{
    Op9Out<T> w;
    for (int q = 0; q < 9; ++q) w.a[q] = const_cast<T*>(o.a[q]);
    return w;
}

template <typename T> VarLevel<T> var_level(const Level& l)
{
    return VarLevel<T>{op9_of<T>(l), jac9_of<T>(l), (const T*)l.J[0], l.nine, l.N, l.rows, l.pitch};
}

// g_l of the operator and splitting just built on level l (k_lambda_partials, k_reduce_max): one 8-byte copy to the
// host per level, at set-up only
int lambda_update(mgx_solver* s, Level& l)
{
    if (l.f64) launch_lambda_max<double>(var_level<double>(l), s->partial, s->partial_cap, s->sum_dev, s->stream);
    else launch_lambda_max<float>(var_level<float>(l), s->partial, s->partial_cap, s->sum_dev, s->stream);
    HIPCHK(s, hipGetLastError());
    HIPCHK(s, hipMemcpyAsync(s->sum_host, s->sum_dev, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    l.lambda_g = *s->sum_host;
    return MGX_OK;
}

template <typename T> LineLevel<T> line_level(const Level& l)
{
    return LineLevel<T>{op9_of<T>(l), l.nine, l.N, l.pitch, (T*)l.line_m[0], (T*)l.line_g[0], (T*)l.line_m[1], (T*)l.line_g[1],
                        (T*)l.line_hf, (T*)l.line_hb, l.line_R};
}

// the line factors of the operator just written into l.A[] (handles with a line smoother; nothing otherwise).  A zero
// or non-finite pivot: MGX_ERR_INVALID, naming the level and the direction
int line_update(mgx_solver* s, Level& l)
{
    if (!s->line_dirs) return MGX_OK;
    HIPCHK(s, hipMemsetAsync(s->line_flag, 0, sizeof(int), s->stream));
    for (int d = 0; d < 2; ++d) {
        if (!(s->line_dirs & (1 << d))) continue;
        if (l.f64) launch_line_factor<double>(line_level<double>(l), d, s->line_flag, s->stream);
        else launch_line_factor<float>(line_level<float>(l), d, s->line_flag, s->stream);
    }
    HIPCHK(s, hipGetLastError());
    int flag = 0;
    HIPCHK(s, hipMemcpyAsync(&flag, s->line_flag, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    if (flag)
        return s->fail(MGX_ERR_INVALID, "MGX_SMOOTHER_LINE: zero or non-finite pivot in the tridiagonal factorisation of level " +
                                            std::to_string(l.L) + ", direction " + ((flag & 1) ? "x" : "y"));
    return MGX_OK;
}

// {D_inv, R_omega} of the operator in l.A[] (MF:28-32)
template <typename T>
void build_splitting(mgx_solver* s, const Level& l)
{
    const dim3 blk(256), grd((l.N + 1 + 255) / 256, l.N + 1);
    with_point_count(l.nine, [&](auto nq) {
        hipLaunchKernelGGL((k_var_build_jacobi<T, decltype(nq)::value>), grd, blk, 0, s->stream, op9_of<T>(l), out9(jac9_of<T>(l)), l.N, l.pitch,
                           (T)s->cfg.omega);
    });
}
// the dense inverse of the coarsest operator, for the exact bottom solve (MF:63-72)
template <typename T>
void build_bottom_inverse(mgx_solver* s, const Level& l)
{
    const int n = l.N - 1, NN = n * n;
    with_point_count(l.nine, [&](auto nq) {
        hipLaunchKernelGGL((k_var_dense_fill<T, decltype(nq)::value>), dim3((NN + 255) / 256, NN), dim3(256), 0, s->stream, s->var_M, s->var_inv,
                           op9_of<T>(l), n, l.pitch);
    });
    gj_invert(s, NN);
}

// the level's operator has been written into l.A[]: build its splitting and, on the coarsest level with an exact
// bottom solve, the dense inverse
template <typename T>
int var_build_t(mgx_solver* s, Level& l)
{
    build_splitting<T>(s, l);
    if (l.L == s->cfg.coarsest_level && s->cfg.bottom == MGX_BOTTOM_EXACT) build_bottom_inverse<T>(s, l);
    HIPCHK(s, hipGetLastError());
    HIPCHK(s, hipStreamSynchronize(s->stream));
    if (int rc = lambda_update(s, l)) return rc;
    if (int rc = line_update(s, l)) { l.stencil_set = false; operator_changed(s); return rc; }
    l.stencil_set = true;
    // the kernels' coefficient pointers are unchanged, but a new operator is a new problem, and the Chebyshev scalars
    // (from g_l) are kernel arguments of a captured cycle: recapture
    operator_changed(s);
    return MGX_OK;
}
int var_build(mgx_solver* s, Level& l) { return l.f64 ? var_build_t<double>(s, l) : var_build_t<float>(s, l); }

// ---- Galerkin hierarchy (cfg.op = MGX_OPERATOR_GALERKIN; kernels in mgx_galerkin.hpp) ---------------------
template <typename T> Wt8<T> wt8_of(const Level& c)
{
    Wt8<T> w;
    for (int x = 0; x < 8; ++x) w.w[x] = (const T*)c.wt[x];
    return w;
}
template <typename T> Wt8Out<T> wt8_out(const Level& c)
{
    Wt8Out<T> w;
    for (int x = 0; x < 8; ++x) w.w[x] = (T*)c.wt[x];
    return w;
}

// the hierarchy in use has operator-dependent transfers (mgx_opdep.hpp)
inline bool opdep(const mgx_solver* s) { return s->galerkin && s->gal_built && s->transfer == MGX_TRANSFER_OPERATOR; }

// A_{l-1} = R A_l P for l = finest .. coarsest + 1 (transfer = OPERATOR: the weights of P_l from A_l first), then
// {D_inv, R_omega} of every level and the dense inverse of the coarsest operator
template <typename T>
int galerkin_build_t(mgx_solver* s, int transfer)
{
    const int lo = s->cfg.coarsest_level, hi = s->cfg.finest_level;
    const T rscale = (s->cfg.restrict_mode == MGX_RESTRICT_FW16) ? (T)0.25 : (T)1;
    // every allocation before the first launch: a failure here leaves the previous hierarchy, gal_built and transfer as
    // they were (grids already allocated stay for the next attempt; mgx_destroy frees them)
    if (transfer == MGX_TRANSFER_OPERATOR)
        for (int lv = lo; lv < hi; ++lv)
            for (void*& p : s->lv[lv].wt) {
                if (p) continue;
                if (hipMalloc(&p, s->lv[lv].bytes) != hipSuccess) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for the prolongation's weight arrays");
                HIPCHK(s, hipMemsetAsync(p, 0, s->lv[lv].bytes, s->stream));      // the ring and the padding stay zero from here on
            }
    for (int lv = hi; lv > lo; --lv) {
        const Level& f = s->lv[lv];
        const Level& c = s->lv[lv - 1];
        const Launch g = make_launch(c.N, VecOf<T>::W, c.N - 1, 1);
        const dim3 grd(g.blocks), blk(kBlock);
        with_point_count(f.nine, [&](auto nq) {
            constexpr bool CORNERS = decltype(nq)::value == 9;
            if (transfer == MGX_TRANSFER_OPERATOR) {
                hipLaunchKernelGGL((k_opdep_weights<T, CORNERS>), grd, blk, 0, s->stream, op9_of<T>(f), wt8_out<T>(c), c.N, f.pitch, c.pitch, g.strips);
                hipLaunchKernelGGL((k_galerkin_rap_opdep<T, CORNERS>), grd, blk, 0, s->stream, op9_of<T>(f), wt8_of<T>(c), out9(op9_of<T>(c)), c.N,
                                   f.pitch, c.pitch, g.strips, rscale);
            }
            else hipLaunchKernelGGL((k_galerkin_rap<T, CORNERS>), grd, blk, 0, s->stream, op9_of<T>(f), out9(op9_of<T>(c)), c.N, f.pitch, c.pitch,
                                    g.strips, rscale);
        });
    }
    for (int lv = lo; lv <= hi; ++lv) build_splitting<T>(s, s->lv[lv]);
    if (s->cfg.bottom == MGX_BOTTOM_EXACT) build_bottom_inverse<T>(s, s->lv[lo]);
    HIPCHK(s, hipGetLastError());
    HIPCHK(s, hipStreamSynchronize(s->stream));
    for (int lv = lo; lv <= hi; ++lv)
        if (int rc = lambda_update(s, s->lv[lv])) return rc;
    for (int lv = lo; lv <= hi; ++lv)
        if (int rc = line_update(s, s->lv[lv])) {             // as after a new finest operator: nothing below it is usable
            for (int c = lo; c < hi; ++c) s->lv[c].stencil_set = false;
            s->gal_built = false;
            operator_changed(s);
            return rc;
        }
    for (int lv = lo; lv <= hi; ++lv) s->lv[lv].stencil_set = true;
    s->gal_built = true;
    s->transfer = transfer;
    operator_changed(s);     // the buffers have not moved, but a new hierarchy (or another P) is a new problem: recapture
    return MGX_OK;
}

// a new finest operator of a GALERKIN handle: the coarse operators and every splitting are stale.  The operator is what
// the call gave: a zero-order term of mgx_set_reaction is gone with the centre it was added to (mgx_set_reaction itself
// raises the flag again after this)
void galerkin_invalidate(mgx_solver* s)
{
    s->rx.set = false;
    for (int lv = s->cfg.coarsest_level; lv < s->cfg.finest_level; ++lv) s->lv[lv].stencil_set = false;
    s->lv[s->cfg.finest_level].stencil_set = true;
    s->gal_built = false;
    operator_changed(s);
}

// every level's operator must have been given before a schedule or operator runs
int var_ready(mgx_solver* s, int lo, int hi)
{
    if (!s->var) return MGX_OK;
    if (s->galerkin && !s->gal_built)
        return s->fail(MGX_ERR_STATE, s->lv[s->cfg.finest_level].stencil_set ? "Galerkin hierarchy not built (mgx_build_galerkin)"
                                                                             : "finest operator not set (mgx_set_stencil / mgx_set_coefficient / mgx_set_stencil9 / mgx_set_tensor)");
    for (int l = lo; l <= hi; ++l)
        if (!s->lv[l].stencil_set)
            return s->fail(MGX_ERR_STATE, "operator of level " + std::to_string(l) + " not set (mgx_set_stencil / mgx_set_coefficient)");
    return MGX_OK;
}

// ---- the columns a cycle works on ------------------------------------------------------------------------------------
// The level operations and the walk below run on a set of columns: act[0 .. m), m >= 1, ascending.  Column c >= 0 is
// column c of s->multi (mgx_multi_host.hpp); the handle's own grids are one more column, kOwn, which comes alone: the
// set kOwnSet.  What exists for the own column only - Prof scopes, the constant stencil's kernels, the smoothers other
// than Jacobi, the folded passes and the one-workgroup visits - asks own(a).
struct MultiSet { int act[MGX_MAX_RHS]; int m; };
constexpr int kOwn = -1;
constexpr MultiSet kOwnSet{{kOwn}, 1};
inline bool own(const MultiSet& a) { return a.act[0] == kOwn; }

inline MultiSet multi_all(int nrhs)
{
    MultiSet a{};
    for (int j = 0; j < nrhs; ++j) a.act[a.m++] = j;
    return a;
}

// the pointer slot `which` of column c on a level, the storage itself: a sweep swaps u and tmp through it
enum Slot { kU, kTmp, kB, kR };
inline void*& slot(mgx_solver* s, int level, int c, Slot which)
{
    if (c == kOwn) {
        Level& l = s->lv[level];
        void** const own_slots[] = {&l.u, &l.tmp, &l.b, &l.r};
        return *own_slots[which];
    }
    auto& w = s->multi.lv[level];
    void** const columns[] = {w.u, w.tmp, w.b, w.r};
    return columns[which][c];
}

// one slot of the set's columns as a host array of m pointers (T may be const), what the launch_* helpers take
template <typename T> struct SetPtrs { T* p[MGX_MAX_RHS]; };
template <typename T> SetPtrs<T> set_ptrs(mgx_solver* s, int level, const MultiSet& a, Slot which)
{
    SetPtrs<T> o{};
    for (int j = 0; j < a.m; ++j) o.p[j] = (T*)slot(s, level, a.act[j], which);
    return o;
}

// MF:75-96: mu sweeps, one launch each for the set, u <-> tmp
template <typename T>
void smooth_var_t(mgx_solver* s, int level, const MultiSet& a, int mu)
{
    const T om = (T)s->cfg.omega;
    const T rc = (T)(1.0 - (double)om);
    const VarLevel<T> v = var_level<T>(s->lv[level]);
    for (int i = 0; i < mu; ++i) {
        launch_jacobi_var<T>(v, a.m, set_ptrs<const T>(s, level, a, kU).p, set_ptrs<const T>(s, level, a, kB).p, set_ptrs<T>(s, level, a, kTmp).p,
                             rc, om, s->stream);
        for (int j = 0; j < a.m; ++j) std::swap(slot(s, level, a.act[j], kU), slot(s, level, a.act[j], kTmp));
    }
    s->last_smooth_launches = mu;
}

// a Chebyshev block of degree mu (mgx_cheby.hpp), one launch per step, u <-> tmp; every block starts afresh (step 0
// overwrites the level's d)
template <typename T>
void smooth_cheby_t(mgx_solver* s, Level& l, int mu)
{
    const T om = (T)s->cfg.omega;
    const T rc = (T)(1.0 - (double)om);
    const std::vector<ChebyStep> st = cheby_scalars(s->cfg.omega, l.lambda_g, mu);
    const VarLevel<T> cl = var_level<T>(l);
    for (int i = 0; i < mu; ++i) {
        launch_cheby<T>(cl, (const T*)l.u, (const T*)l.b, (T*)l.tmp, (T*)l.cheb, i == 0, rc, om, (T)st[i].a, (T)st[i].c, s->stream);
        std::swap(l.u, l.tmp);
    }
    s->last_smooth_launches = mu;
}

// mu zebra line sweeps (mgx_line.hpp), two launches per sweep and direction, u in place: no swap
template <typename T>
void smooth_line_t(mgx_solver* s, Level& l, int mu)
{
    const LineLevel<T> ll = line_level<T>(l);
    int launches = 0;
    for (int i = 0; i < mu; ++i) launches += launch_line_sweep<T>(ll, (T*)l.u, (const T*)l.b, s->line_dirs, s->stream);
    s->last_smooth_launches = launches;
}

// mu multicolour Gauss-Seidel sweeps (mgx_colour.hpp), the colours in reverse order if `reverse`.  A five-point level
// with a chunk's worth of rows: one launch per sweep, u <-> tmp; otherwise one launch per colour, u in place
template <typename T>
void smooth_colour_t(mgx_solver* s, Level& l, int mu, bool reverse)
{
    const ColourLevel<T> cl{op9_of<T>(l), (const T*)l.J[0], l.nine, l.N, l.pitch};
    const bool fused = s->gs_fused && !l.nine && gs_fused_level(l.N);
    int launches = 0;
    for (int i = 0; i < mu; ++i) {
        if (fused) {
            launch_gs_rb<T>(cl, (const T*)l.u, (const T*)l.b, (T*)l.tmp, reverse, s->stream);
            std::swap(l.u, l.tmp);
            ++launches;
        } else {
            launches += launch_gs_colours<T>(cl, (T*)l.u, (const T*)l.b, reverse, s->stream);
        }
    }
    s->last_smooth_launches = launches;
}

// the level smoother of a general-operator handle; post: the block follows a correction (MGX_SMOOTHER_COLOR_SGS sweeps
// it in reverse colour order; nothing else looks at it).  The Jacobi block runs on the set; the other smoothers exist for
// the own column only (multi_guard refuses them for a block)
void smooth_var(mgx_solver* s, int level, const MultiSet& a, int mu, bool post = false)
{
    Level& l = s->lv[level];
    if (s->colour) {
        const bool reverse = s->colour == 2 && post;
        if (l.f64) smooth_colour_t<double>(s, l, mu, reverse); else smooth_colour_t<float>(s, l, mu, reverse);
    }
    else if (s->line_dirs) { if (l.f64) smooth_line_t<double>(s, l, mu); else smooth_line_t<float>(s, l, mu); }
    else if (s->cfg.smoother == MGX_SMOOTHER_CHEBYSHEV) { if (l.f64) smooth_cheby_t<double>(s, l, mu); else smooth_cheby_t<float>(s, l, mu); }
    else if (l.f64) smooth_var_t<double>(s, level, a, mu);       // MF:75-96
    else smooth_var_t<float>(s, level, a, mu);
}

// MF:150-153 on m grid pairs of level l, one per column of the set: out_j = b_j - A u_j (MODE 0), or the per-block sums
// of its squares into the column's partials, each reduced by k_reduce_partials in its own order into the column's sum
// (MODE 1; out may be null): s->partial and s->sum_dev for the own column, multi.part[c] and multi.sums + c for column c
template <typename T, int MODE>
void residual_var_t(mgx_solver* s, const Level& l, const MultiSet& a, const T* const* u, const T* const* b, T* const* out)
{
    double *part[MGX_MAX_RHS] = {}, *sums[MGX_MAX_RHS] = {};
    for (int j = 0; j < a.m; ++j) {
        const int c = a.act[j];
        part[j] = c == kOwn ? s->partial : s->multi.part[c];
        sums[j] = c == kOwn ? s->sum_dev : s->multi.sums + c;
    }
    launch_residual_var<T, MODE>(var_level<T>(l), a.m, u, b, out, part, sums, s->stream);
}

// ... of the u and b of the set's columns, MODE 0 into their r
template <typename T, int MODE>
void residual_set(mgx_solver* s, int level, const MultiSet& a)
{
    residual_var_t<T, MODE>(s, s->lv[level], a, set_ptrs<const T>(s, level, a, kU).p, set_ptrs<const T>(s, level, a, kB).p,
                            MODE ? nullptr : set_ptrs<T>(s, level, a, kR).p);
}

// the same of whichever operator the handle has, on a grid pair of level l (the own column's, or the Krylov and fp64
// vectors that stand in for them): the general operator's kernel or the constant stencil's (which takes the partial-sum
// capacity for MODE 1 only)
template <int MODE>
void residual_level(mgx_solver* s, const Level& l, const void* u, const void* b, void* out)
{
    with_float_type(l.f64, [&](auto tag) {
        using T = decltype(tag);
        const T* const uu = (const T*)u;
        const T* const bb = (const T*)b;
        T* const oo = (T*)out;
        if (s->var) residual_var_t<T, MODE>(s, l, kOwnSet, &uu, &bb, &oo);
        else launch_residual<T, MODE>((const T*)u, (const T*)b, out, MODE ? 0 : l.pitch, MODE ? s->partial : nullptr, MODE ? s->sum_dev : nullptr,
                                      1.0, l.N, l.pitch, 1, l.N, s->rows_per_chunk, s->stream, MODE ? s->partial_cap : -1, l.rows);
    });
}

// ---- the executor of smoothing blocks ----------------------------------------------------------------
// Runs the plan of q (fold_plan) on u <-> tmp, the arrays of the window q.row0 .. q.row0 + q.rows - 1 (a whole level:
// row0 = 0, rows = N + 1).  c (may be null): the coarse window; coarse_e: the correction of q.pre; post 1: the residual
// restricted into coarse rows [crow_lo, crow_hi) of coarse_b, zeroed in coarse_zero (may be null); post 2: per-block sums
// of r^2 in `partial`.  Returns the number of those sums (0 unless post 2), < 0 when the block cannot run as asked (then
// before any launch); *flips = launches made (the result is in tmp when odd).
template <typename T, int SM, int AR>
int fold_block(const FuseCfg& fc, const BlockReq& q, T* u, const T* b, T* tmp, long pitch, double omega, const mgx_slab* c,
               const T* coarse_e, T* coarse_b, T* coarse_zero, int crow_lo, int crow_hi, int restrict_mode, double* partial,
               hipStream_t st, int* flips)
{
    std::vector<Pass> plan;
    if (!fold_plan(fc, q, &plan)) return -1;
    const int N = q.N, row0 = q.row0;
    const JacobiCoef<T> jc = jacobi_coef<T>(omega);
    FoldArgs fa;
    fa.restrict_mode = restrict_mode;
    fa.partial = partial;
    fa.win.row_first = std::max(row0, 0);
    fa.win.row_last = std::min(row0 + q.rows - 1, N);
    fa.win.crow_first = 0; fa.win.crow_last = -1; fa.win.emit_lo = 0; fa.win.emit_hi = 0;
    if (c) {
        fa.cpitch = level_pitch(c->level, c->dtype);
        fa.win.crow_first = std::max(c->row0, 0);
        fa.win.crow_last = std::min(c->row0 + c->rows - 1, N / 2);
        fa.win.emit_lo = std::max(c->row0 + crow_lo, 1);
        fa.win.emit_hi = std::min(c->row0 + crow_hi, N / 2);
        // base pointers moved back so that GLOBAL coarse rows index them (never dereferenced outside the window)
        const long cback = (long)c->row0 * fa.cpitch;
        if (coarse_e) fa.coarse_e = coarse_e - cback;
        if (coarse_b) fa.coarse_b = coarse_b - cback;
        if (coarse_zero) fa.coarse_zero = coarse_zero - cback;
    }
    const long back = (long)row0 * pitch;
    T* src = u; T* dst = tmp;
    int blocks = 0;
    for (const Pass& p : plan) {
        if (p.hi > p.lo) {
            const int lo = p.lo - row0, hi = p.hi - row0;             // local rows
            fa.row_lo = p.lo; fa.row_hi = p.hi;
            fa.zero_in = p.zero_in ? 1 : 0;                           // PS:613: the first pass synthesises the zero guess
            int rc = 0;
            if (p.kind == PASS_JACOBI)
                rc = launch_jacobi<T>(src, b, dst, N, pitch, lo, hi, omega, p.R, st, q.rows, AR) ? -1 : 0;
            else if (p.kind == PASS_RBGS)
                launch_rbgs<T>(src, b, dst, N, pitch, lo, hi, row0 & 1, -row0, N - row0, p.R, st);
            else if (p.kind == PASS_FUSED)
                rc = launch_fused<T, SM, AR>(p.K, src, b, dst, N, pitch, lo, hi, jc.c0, jc.c1, -row0, N - row0, row0 & 1, p.R, st,
                                             q.rows, fa.zero_in) ? 0 : -1;
            else if (p.kind == PASS_FOLDED)
                rc = with_stages(p.pre, p.post, [&](auto s) {
                    using S = decltype(s);
                    if constexpr (S::PRE || S::POST)
                        return launch_cycle<T, S::PRE, S::POST, SM, AR>(p.K, src - back, b - back, dst - back, fa, N, pitch, jc.c0, jc.c1, p.R, st);
                    else
                        return -1;
                });
            else
                rc = launch_tile_pass<T, SM, AR>(src - back, b - back, dst - back, fa, N, pitch, jc.c0, jc.c1, p.K, p.R, p.pre, p.post, st);
            if (rc < 0) return -1;                                    // (the plan rules these out)
            if (p.post == 2) blocks = rc;
        }
        std::swap(src, dst);
    }
    *flips = (int)plan.size();
    return blocks;
}

// May a whole level run this block with folded stages?  Decided before any launch (a `false` never leaves a half-done
// block): the handle's settings, then whether a plan exists.
bool fold_eligible(const mgx_solver* s, const Level& l, int mu, bool pre = false, int post = 1, bool zero_in = false)
{
    if (!s->fold || mu < 1 || mu > 64) return false;
    // general operators have no fused / folded kernels; the folded restriction is full weighting
    if (s->var || (post == 1 && s->cfg.restrict_mode >= MGX_RESTRICT_INJECT)) return false;
    const int per = (s->cfg.smoother == MGX_SMOOTHER_RBGS) ? 2 : 1;
    if (!tile_level(s, l) && (l.N < s->fuse.min_n || s->fuse.kmax < per)) return false;
    std::vector<Pass> plan;
    return fold_plan(s->fuse, level_req(s, l, mu, pre, post, zero_in, 0), &plan);
}

// May the pre-smoothing of `level` start from an implicit zero iterate (the producer then
// skips the zero fill)?  Only when its plan's first pass is a kernel that honours zero_in: a folded,
// fused or tile pass, not a stand-alone single sweep.
bool zero_in_ok(const mgx_solver* s, int level)
{
    if (!s->use_zero_in || level <= s->cfg.coarsest_level) return false;
    return fold_eligible(s, s->lv[level], s->cfg.mu1, false, 1, true);
}

// mu sweeps on a whole level with the prolongation+correction applied while loading (pre) and/or the
// residual restriction (post = 1) or the residual norm (post = 2) produced by the last pass.  Returns
// false when this level / configuration is not eligible (the caller then uses the stand-alone kernels).
// zero_in: this level's iterate is an implicit zero;  coarse_zero_in: so is the coarse guess of post = 1.
bool smooth_folded(mgx_solver* s, int level, int mu, bool pre, int post, bool zero_in = false, bool coarse_zero_in = false)
{
    Level& l = s->lv[level];
    if (!fold_eligible(s, l, mu, pre, post)) return false;
    const bool fine = (level == s->cfg.finest_level);
    const bool rbgs = (s->cfg.smoother == MGX_SMOOTHER_RBGS);
    // float: the 10-level pass with BOTH the correction stage and the norm stage does not fit its registers (mgx_pass_plan.hpp,
    // cycle_k_supported) and a block of 10 would run as two passes of 5 (8192^2: 223 + 190 us); one 10-level pass without
    // the norm stage and the stand-alone norm kernel are 216 + ~110 us.  (The same for the restriction stage of the
    // separately rounded mode - 10 levels + the stand-alone residual / restriction instead of 8 + 2 - was measured and is
    // worse: mixed cycle 1.54 -> 1.72 ms, the stand-alone transfer alone is 0.15 ms.)
    if (!l.f64 && !rbgs && mu == 10 && l.N > s->fuse.tile_max_n && post == 2 && pre &&
        cycle_k_supported(mu, false, false, 0, pre, s->fuse.arith) && !cycle_k_supported(mu, false, false, post, pre, s->fuse.arith))
        post = 0;
    {
        Prof p(s, fine ? MGX_PROF_SMOOTH_FINE : MGX_PROF_COARSE, mu);
        // the level below is the coarse window of the whole level; the restriction stage zeroes
        // the coarse guess (PS:613) unless that level's first pre-smoothing pass synthesises it
        const Level& c = s->lv[level - 1];
        const int dt = l.f64 ? MGX_DTYPE_F64 : MGX_DTYPE_F32;
        const mgx_slab cs{level - 1, dt, c.rows, 0, s->cfg.arith};
        void* czero = (post == 1 && coarse_zero_in) ? nullptr : c.u;
        const BlockReq q = level_req(s, l, mu, pre, post, zero_in, env_int("MGX_ROWS", 0));
        int launches = 0;
        const int nb = with_kernel_set(l.f64, s->cfg.smoother, s->fuse.arith, [&](auto k) {
            using K = decltype(k);
            using T = typename K::T;
            return fold_block<T, K::SM, K::AR>(s->fuse, q, (T*)l.u, (const T*)l.b, (T*)l.tmp, l.pitch, s->cfg.omega, &cs,
                                               pre ? (const T*)c.u : nullptr, post == 1 ? (T*)c.b : nullptr, (T*)czero, 1, c.N,
                                               s->cfg.restrict_mode, s->partial, s->stream, &launches);
        });
        if (nb < 0) return false;
        if (launches & 1) std::swap(l.u, l.tmp);
        p.set(launches, mu);
        if (post == 2) s->norm_blocks_ready = nb;
    }
    // (the norm stage left out: mgx_solve's residual_norm_grid finds norm_blocks_ready == 0 and runs the norm kernel)
    if (fine) s->fine_updates += (double)mu * (double)(l.N - 1) * (double)(l.N - 1);
    return true;
}

// mu sweeps on a whole level, no folded stage
void smooth_t(mgx_solver* s, Level& l, int mu)
{
    int launches = 0;
    with_kernel_set(l.f64, s->cfg.smoother, s->fuse.arith, [&](auto k) {
        using K = decltype(k);
        using T = typename K::T;
        (void)fold_block<T, K::SM, K::AR>(s->fuse, level_req(s, l, mu, false, 0, false, s->rows_per_chunk), (T*)l.u, (const T*)l.b,
                                          (T*)l.tmp, l.pitch, s->cfg.omega, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr,
                                          s->stream, &launches);
    });
    s->last_smooth_launches = launches;
    if (launches & 1) std::swap(l.u, l.tmp);
}

// one smoothing block of the set on a level.  fu (may be null): the fine_updates of a block call's columns, fu[c] for
// column c; the own column counts into s->fine_updates
void smooth(mgx_solver* s, int level, int mu, bool post = false, const MultiSet& a = kOwnSet, double* fu = nullptr)
{
    if (mu <= 0) return;
    Level& l = s->lv[level];
    const bool fine = (level == s->cfg.finest_level);
    Prof p(s, fine ? MGX_PROF_SMOOTH_FINE : MGX_PROF_COARSE, mu, own(a));
    if (s->var) smooth_var(s, level, a, mu, post);
    else smooth_t(s, l, mu);
    p.set(s->last_smooth_launches, mu);
    if (!fine) return;
    // one update per point and sweep; an alternating line sweep is an x- and a y-sweep
    const double updates = (double)(s->line_dirs == 3 ? 2 * mu : mu) * (double)(l.N - 1) * (double)(l.N - 1);
    if (own(a)) s->fine_updates += updates;
    else if (fu) for (int j = 0; j < a.m; ++j) fu[a.act[j]] += updates;
}

// B[level-1] = R (B - A U)[level]  (fused = true)  or  R B[level]  (fused = false) of the set's columns; zero_guess: and
// U[level-1] = 0.  A block call restricts fused with zero_guess; the unfused form and the constant stencil are the own
// column's
void restrict_level(mgx_solver* s, int level, bool fused, bool zero_guess, const MultiSet& a = kOwnSet)
{
    Level& f = s->lv[level];
    Level& c = s->lv[level - 1];
    const bool fine = (level == s->cfg.finest_level);
    Prof p(s, fine ? MGX_PROF_RESTRICT_FINE : MGX_PROF_COARSE, 1, own(a));
    const int rpc = s->rows_per_chunk;
    const int mode = s->cfg.restrict_mode;
    with_float_type(f.f64, [&](auto tag) {
        using T = decltype(tag);
        const SetPtrs<const T> uf = set_ptrs<const T>(s, level, a, kU), bf = set_ptrs<const T>(s, level, a, kB);
        const SetPtrs<T> cb = set_ptrs<T>(s, level - 1, a, kB);
        const SetPtrs<T> cz = zero_guess ? set_ptrs<T>(s, level - 1, a, kU) : SetPtrs<T>{};
        if (opdep(s)) {
            // B_c = c P^T (B - A U) or c P^T B with the hierarchy's own weights, the residual formed in the same pass
            const Launch g = make_launch(c.N, VecOf<T>::W, c.N - 1, 1);
            const T rscale = (mode == MGX_RESTRICT_FW16) ? (T)0.25 : (T)1;
            const dim3 grd(g.blocks), blk(kBlock);
            if (!fused) hipLaunchKernelGGL((k_restrict_opdep<T, 0>), grd, blk, 0, s->stream, uf.p[0], bf.p[0], op9_of<T>(f), wt8_of<T>(c), cb.p[0],
                                           cz.p[0], c.N, f.pitch, c.pitch, g.strips, rscale);
            else with_point_count(f.nine, [&](auto nq) {
                constexpr int MODE = decltype(nq)::value == 9 ? 2 : 1;
                // one column: mgx_solve's kernel, not the K = 1 instance of the K-column one.  The two bodies differ
                // (k_restrict_opdep loads the five u rows once and keeps three residual rows live, 216 / 256 VGPRs in double /
                // float, two waves per SIMD; k_restrict_opdep_multi reloads three u rows per fine row so that K = 3, 4 do not
                // spill, 112 / 118 VGPRs at K = 1, four waves) and which is faster has not been measured: replacing one
                // with the other would change the speed of mgx_solve or of a block solve's last column
                if (a.m == 1) hipLaunchKernelGGL((k_restrict_opdep<T, MODE>), grd, blk, 0, s->stream, uf.p[0], bf.p[0], op9_of<T>(f), wt8_of<T>(c),
                                                 cb.p[0], cz.p[0], c.N, f.pitch, c.pitch, g.strips, rscale);
                else with_count<kMultiMax, 2>(a.m, [&](auto kc) {
                    constexpr int K = decltype(kc)::value;
                    hipLaunchKernelGGL((k_restrict_opdep_multi<T, MODE, K>), grd, blk, 0, s->stream, columns_in<K>(uf.p), columns_in<K>(bf.p),
                                       op9_of<T>(f), wt8_of<T>(c), columns_out<K>(cb.p), columns_out<K>(cz.p), c.N, f.pitch, c.pitch, g.strips, rscale);
                });
            });
            return;
        }
        // general operator and / or injection (MF:122-130): the residual is formed first as a grid (MF:150-153; f.r
        // was allocated with the handle; the operator's grids read once for the set), then each column's is restricted
        // by full weighting (PS:531-546) or injected, with the coefficient-free single-column kernel.  The constant
        // stencil with full weighting forms it inside launch_restrict (fused) and reads B itself
        const bool grid_residual = fused && (s->var || mode >= MGX_RESTRICT_INJECT);
        if (grid_residual) {
            if (s->var) residual_set<T, 0>(s, level, a);
            else residual_level<0>(s, f, f.u, f.b, f.r);
        }
        const SetPtrs<const T> src = grid_residual ? set_ptrs<const T>(s, level, a, kR) : bf;
        for (int j = 0; j < a.m; ++j) {
            if (mode >= MGX_RESTRICT_INJECT) {
                const double w = (mode == MGX_RESTRICT_INJECT4) ? 4.0 : 1.0;
                const dim3 blk(256), grd((c.N + 255) / 256, c.N - 1);
                hipLaunchKernelGGL((k_restrict_inject<T>), grd, blk, 0, s->stream, src.p[j], cb.p[j], cz.p[j], c.N, f.pitch, c.pitch, (T)w);
            } else {
                launch_restrict<T>(uf.p[j], src.p[j], cb.p[j], cz.p[j], f.N, f.pitch, c.pitch, 1, c.N, 0, mode, fused && !grid_residual, rpc, s->stream);
            }
        }
    });
}

// U[level] += P U[level-1] (add) or U[level] = P U[level-1] of the set's columns
void prolong_level(mgx_solver* s, int level, bool add, const MultiSet& a = kOwnSet)
{
    Level& f = s->lv[level];
    Level& c = s->lv[level - 1];
    const bool fine = (level == s->cfg.finest_level);
    Prof p(s, fine ? MGX_PROF_PROLONG_FINE : MGX_PROF_COARSE, 1, own(a));
    with_float_type(f.f64, [&](auto tag) {
        using T = decltype(tag);
        const SetPtrs<T> v = set_ptrs<T>(s, level, a, kU);
        const SetPtrs<const T> e = set_ptrs<const T>(s, level - 1, a, kU);
        if (opdep(s)) launch_prolong_opdep<T>(a.m, add, v.p, e.p, wt8_of<T>(c), c.N, f.pitch, c.pitch, s->stream);
        else for (int j = 0; j < a.m; ++j) launch_prolong<T>(v.p[j], e.p[j], f.N, f.pitch, c.pitch, 1, f.N, 0, add, s->rows_per_chunk, s->stream);
    });
}

// the exact solve of the set's columns on the coarsest level (the constant stencil's is the own column's)
void bottom_solve(mgx_solver* s, const MultiSet& a = kOwnSet)
{
    const int level = s->cfg.coarsest_level;
    Level& l = s->lv[level];
    Prof p(s, (l.L == s->cfg.finest_level) ? MGX_PROF_SMOOTH_FINE : MGX_PROF_COARSE, 4, own(a));
    const int n = l.N - 1;
    with_float_type(l.f64, [&](auto tag) {
        using T = decltype(tag);
        const SetPtrs<const T> b = set_ptrs<const T>(s, level, a, kB);
        const SetPtrs<T> u = set_ptrs<T>(s, level, a, kU);
        if (s->var) launch_var_dense_solve<T>(s->var_inv, a.m, b.p, u.p, n, l.pitch, s->stream);     // MF:63-72: x = A^-1 b, A^-1 built at set-up
        else s->bottom.solve<T>(b.p[0], u.p[0], l.pitch, s->stream);
    });
}

// U[level] = 0 of the set's columns, one fill each
int zero_u(mgx_solver* s, int level, const MultiSet& a = kOwnSet)
{
    for (int j = 0; j < a.m; ++j) HIPCHK(s, hipMemsetAsync(slot(s, level, a.act[j], kU), 0, s->lv[level].bytes, s->stream));
    return MGX_OK;
}

// The two halves of a V-cycle on a level above the coarsest (PS:575-627 / MF:132-173).
// descend: PS:581 pre-smoothing + PS:604-613 residual, restriction, zero coarse guess - one set of passes when the
// level is eligible for folding.  zero_in_here: this level's iterate is a known zero that nobody has written.
// Returns whether the coarse guess is one: if the coarse level's first pass can synthesise it, nobody writes or
// reads those zeros.
// The walk runs on a set of columns (a; fu as for smooth).  Its shortcuts - the folded passes with their implicit zeros
// and norm stage (smooth_folded, zero_in_ok, post = 2) and the one-workgroup visits (small_level) - are the own column's:
// each asks own(a), and a block call runs the per-level launches on every level
bool descend(mgx_solver* s, int level, bool zero_in_here, const MultiSet& a = kOwnSet, double* fu = nullptr)
{
    const bool zin_next = own(a) && zero_in_ok(s, level - 1);
    if (!own(a) || !smooth_folded(s, level, s->cfg.mu1, false, 1, zero_in_here, zin_next)) {
        if (zero_in_here) (void)zero_u(s, level, a);          // cannot happen (zero_in_ok planned this block); stay correct
        smooth(s, level, s->cfg.mu1, false, a, fu);           // PS:581
        restrict_level(s, level, true, !zin_next, a);         // PS:604-613
    }
    return zin_next;
}

// ascend: PS:620-624 correction + PS:625 post-smoothing; post = 2: the last pass also sums r^2 per block (the
// cycle's residual norm), else 0
void ascend(mgx_solver* s, int level, int post, const MultiSet& a = kOwnSet, double* fu = nullptr)
{
    if (!own(a) || !smooth_folded(s, level, s->cfg.mu2, true, post)) {
        prolong_level(s, level, true, a);                     // PS:620-624
        smooth(s, level, s->cfg.mu2, true, a, fu);            // PS:625
    }
}

void vcycle(mgx_solver* s, int level, bool zero_in_here = false, int post_top = 0, int kind = -1, const MultiSet& a = kOwnSet,
            double* fu = nullptr);

// Is a visit of `level` one launch of k_small_visit (mgx_small.hpp)?  Only in the W- and F-cycles of a GALERKIN handle
// with the Jacobi smoother, on nine-point levels above the coarsest and below the finest with N <= 64: the V-cycle keeps
// its launches and its bits, and everything else - a nine-point FINEST level too, whatever its size: it is visited once
// per cycle, by the cycle's own entry and exit, and the columns of a block call, whose results are bit-identical to the
// kernel's - runs W and F through the per-level launches
bool small_level(const mgx_solver* s, int level, const MultiSet& a)
{
    if (!own(a) || !s->small_visit || s->cycle == MGX_CYCLE_V || !s->galerkin || !s->gal_built) return false;
    if (s->cfg.smoother != MGX_SMOOTHER_JACOBI) return false;
    if (level <= s->cfg.coarsest_level || level >= s->cfg.finest_level) return false;
    const Level& l = s->lv[level];
    return l.nine && l.N <= s->small_max_n;
}

// one form of the visit kernel on a small level: ascend (U += P e, mu2 sweeps), descend (mu1 sweeps, the residual
// restricted into the coarse B, the coarse U zeroed) or, with both, the turn between two sub-cycles.  U is updated
// in place: no u <-> tmp swap
void small_visit(mgx_solver* s, int level, bool ascend, bool descend)
{
    Level& f = s->lv[level];
    Level& c = s->lv[level - 1];
    Prof p(s, MGX_PROF_COARSE, 1);
    with_float_type(f.f64, [&](auto tag) {
        using T = decltype(tag);
        SmallVisit<T> a;
        a.u = (T*)f.u; a.b = (const T*)f.b;
        a.a = op9_of<T>(f); a.r = jac9_of<T>(f); a.dinv = (const T*)f.J[0];
        a.cu = (T*)c.u; a.cb = (T*)c.b;
        a.w = wt8_of<T>(c);
        a.N = f.N; a.pitch = f.pitch; a.cpitch = c.pitch;
        a.ascend = ascend; a.descend = descend; a.mu1 = s->cfg.mu1; a.mu2 = s->cfg.mu2;
        a.opdep = opdep(s);
        a.omega = (T)s->cfg.omega;
        a.rc = (T)(1.0 - (double)a.omega);
        const bool fw16 = s->cfg.restrict_mode == MGX_RESTRICT_FW16;
        a.rscale = fw16 ? (T)0.25 : (T)1;
        a.wgt = fw16 ? (T)0.0625 : (T)0.25;
        launch_small_visit<T>(a, s->stream);
    });
    p.set(1, (ascend ? s->cfg.mu2 : 0) + (descend ? s->cfg.mu1 : 0));
}

// every visit a cycle of `kind` pays to `level` between the descend and the ascend of the level above: one (V), or two
// on a level above the coarsest (W: both of kind W; F: the second a V-cycle).  The second visit starts from the iterate
// the first one left, with the same right-hand side - never from an implicit zero.  The coarsest level is visited
// once per descent: a second exact solve would return the same vector, and bottom = SMOOTH is one visit by definition.
// On a small level (small_level) the ascend of the first visit and the descend of the second are one launch, the turn
void coarse_visits(mgx_solver* s, int level, bool zero_in_here, int kind, const MultiSet& a = kOwnSet, double* fu = nullptr)
{
    const bool twice = kind != MGX_CYCLE_V && level > s->cfg.coarsest_level;
    const int second = kind == MGX_CYCLE_F ? MGX_CYCLE_V : kind;
    if (twice && small_level(s, level, a)) {
        small_visit(s, level, false, true);
        coarse_visits(s, level - 1, false, kind);
        small_visit(s, level, true, true);
        coarse_visits(s, level - 1, false, second);
        small_visit(s, level, true, false);
        return;
    }
    vcycle(s, level, zero_in_here, 0, kind, a, fu);           // PS:617
    if (twice) vcycle(s, level, false, 0, second, a, fu);
}

// zero_in_here as for descend; post_top: `post` of this level's ascend (the levels below never report the norm);
// kind: MGX_CYCLE_*, < 0: the handle's (mgx_set_cycle)
void vcycle(mgx_solver* s, int level, bool zero_in_here, int post_top, int kind, const MultiSet& a, double* fu)
{
    if (kind < 0) kind = s->cycle;
    if (level == s->cfg.coarsest_level) {
        if (s->cfg.bottom == MGX_BOTTOM_EXACT) {
            bottom_solve(s, a);                               // MF:137-139
        } else {
            smooth(s, level, s->cfg.mu1, false, a, fu);       // PS:581
            smooth(s, level, s->cfg.mu2, true, a, fu);        // PS:585
        }
        return;
    }
    if (small_level(s, level, a)) {                              // (general operators: zero_in_here is never set, post_top is 0)
        small_visit(s, level, false, true);
        coarse_visits(s, level - 1, false, kind);
        small_visit(s, level, true, false);
        return;
    }
    const bool zin_next = descend(s, level, zero_in_here, a, fu);
    coarse_visits(s, level - 1, zin_next, kind, a, fu);
    ascend(s, level, post_top, a, fu);
}

// PS:629-650 / MF:175-191 on the working hierarchy (B[finest] must be set)
int fmg(mgx_solver* s)
{
    const int lo = s->cfg.coarsest_level, hi = s->cfg.finest_level;
    for (int l = hi; l > lo; --l) restrict_level(s, l, false, false);        // PS:641
    if (s->cfg.bottom == MGX_BOTTOM_EXACT) {
        bottom_solve(s);                                                     // MF:178-181
    } else {
        int rc = zero_u(s, lo);                                              // PS:630
        if (rc) return rc;
        for (int i = 0; i <= s->cfg.mu0; ++i) vcycle(s, lo);                 // PS:635
    }
    for (int l = lo + 1; l <= hi; ++l) {
        prolong_level(s, l, false);                                          // PS:645
        for (int i = 0; i <= s->cfg.mu0; ++i) vcycle(s, l);                  // PS:646-648
    }
    return MGX_OK;
}

// ||B - A U||^2 of an arbitrary grid pair (double or float) -> sum_host, enqueued only
int enqueue_norm(mgx_solver* s, const Level& l, const void* u, const void* b, int cls)
{
    if (s->norm_blocks_ready > 0 && u == s->lv[s->cfg.finest_level].u && !s->mixed) {
        // the last post-smoothing pass already summed (b - A u)^2 per block
        Prof p(s, cls, 1);
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, s->stream, s->partial, s->norm_blocks_ready,
                           s->sum_dev);
    } else {
        Prof p(s, cls, 2);
        residual_level<1>(s, l, u, b, nullptr);
    }
    s->norm_blocks_ready = 0;
    HIPCHK(s, hipMemcpyAsync(s->sum_host, s->sum_dev, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    return MGX_OK;
}

int residual_norm_grid(mgx_solver* s, const Level& l, const void* u, const void* b, double* out, int cls)
{
    int rc = enqueue_norm(s, l, u, b, cls);
    if (rc) return rc;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    *out = std::sqrt(*s->sum_host);
    return MGX_OK;
}

// ---- the graph cache ------------------------------------------------------------------------
// A V-cycle is about 30 launches, the small levels launch-bound: what can be is captured once into a hipGraph and
// replayed.  A W-cycle visits level l 2^(finest - l) times, so its graph over n levels holds about 2^n times the
// nodes of the coarsest visit (9..5 through the per-level launches: ~250 nodes; with k_small_visit three launches
// per visit of a small level); capture time grows with it, once per buffer assignment.
// The cycle swaps each level's u / tmp buffers on the host, so a graph is keyed by the buffer
// assignment it was captured with (and a tag: the kind of body) and carries the assignment it leaves behind (a
// cycle with an odd number of passes on some level alternates between two graphs).
constexpr size_t kMaxGraphs = 8;

std::vector<void*> buffer_state(const mgx_solver* s)
{
    std::vector<void*> v;
    for (int l = s->cfg.coarsest_level; l <= s->cfg.finest_level; ++l) { v.push_back(s->lv[l].u); v.push_back(s->lv[l].tmp); }
    return v;
}

void set_buffer_state(mgx_solver* s, const std::vector<void*>& v)
{
    size_t i = 0;
    for (int l = s->cfg.coarsest_level; l <= s->cfg.finest_level; ++l) { s->lv[l].u = v[i++]; s->lv[l].tmp = v[i++]; }
}

// The graph of `enqueue` (it returns a status) for the current buffer assignment, the host-side bookkeeping of the
// body (u / tmp, fine_updates) done: the caller launches it.  Null when the caller has to run `enqueue` itself: the
// cache is full, or the capture or the instantiation failed - then the bookkeeping of the body that did not run is
// undone, so that the eager launches compute the same bits, and the handle stays off graphs for good.
template <typename Body>
hipGraphExec_t cached_graph(mgx_solver* s, unsigned tag, Body&& enqueue)
{
    std::vector<void*> key = buffer_state(s);
    key.push_back(reinterpret_cast<void*>((uintptr_t)tag));
    for (auto& c : s->graphs)
        if (c.before == key) {
            set_buffer_state(s, c.after);
            s->fine_updates += c.fine_updates;
            return c.exec;
        }
    if (s->graphs.size() >= kMaxGraphs) return nullptr;
    const double fu0 = s->fine_updates;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        // nothing executes while capturing; the host-side bookkeeping does.  No events: they carry no time stamps there
        s->prof_mute = true;
        const int rc = enqueue();
        s->prof_mute = false;
        e = hipStreamEndCapture(s->stream, &graph);
        if (e == hipSuccess && rc != MGX_OK) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_buffer_state(s, key);                             // (the tag at its end is not read)
        s->fine_updates = fu0;
        s->use_graph = 0;
        return nullptr;
    }
    s->graphs.push_back({key, buffer_state(s), exec, s->fine_updates - fu0});
    return exec;
}

// cfg.profile = 2: the finest level's passes are launched one by one between HIP events (they are
// long: the host runs ahead of them) and everything below the finest level is ONE graph replay
// between two events.  Events recorded inside a captured graph carry no time stamps on this runtime
// (hipEventElapsedTime: invalid resource handle - tools/probe/graph_events.hip), so this is how the
// dominant kernel is timed with HIP events while the cycle still runs the way mgx_solve runs it
// (cfg.profile = 1, every launch eager: 1.62 instead of 1.52 ms per cycle at 8192^2).
int coarse_part_graph(mgx_solver* s, int level, bool zero_in_here)
{
    auto body = [&] { coarse_visits(s, level, zero_in_here, s->cycle); return MGX_OK; };
    const hipGraphExec_t exec = cached_graph(s, 4u | (zero_in_here ? 8u : 0u), body);
    if (!exec) return body();
    Prof p(s, MGX_PROF_COARSE, 1);
    HIPCHK(s, hipGraphLaunch(exec, s->stream));
    return MGX_OK;
}

// ---- one V-cycle from the finest level (+ the residual norm): the loop body of mgx_solve, the preconditioner of
// mgx_solve_pcg, mgx_vcycle_zero ---------------------------------------------------------------------------
// A cycle that starts from u = 0 (PS:613; the correction cycle of a coarse-grid solver), three cases in order:
//  1. the finest level's first pass can synthesise the zero (*implicit): nothing is enqueued, nobody writes or reads it;
//  2. a one-level hierarchy outside the MIXED solve: nothing is enqueued either, the cycle is the bottom solve alone;
//  3. otherwise (the MIXED solve's one-level correction included) u is zero-filled.
int zero_start_u(mgx_solver* s, bool* implicit)
{
    const int L = s->cfg.finest_level;
    const bool one_level = L == s->cfg.coarsest_level;
    *implicit = zero_in_ok(s, L);
    if (*implicit) return MGX_OK;                             // 1
    if (one_level && !s->mixed) return MGX_OK;                // 2
    return zero_u(s, L);                                      // 3
}

// enqueues the cycle; want_norm: and ||b - A u||^2 of its result with the copy to sum_host.  split: the submission
// of cfg.profile = 2 (coarse_part_graph), its spans sharing their boundary events (mgx_solver::prof_chain)
int enqueue_cycle(mgx_solver* s, bool want_norm, bool zero_start, bool split)
{
    struct Chain {
        mgx_solver* s;
        Chain(mgx_solver* s_, bool on) : s(s_) { s->prof_chain = on && env_int("MGX_PROF_CHAIN", 1) != 0; s->chain_ev = nullptr; }
        ~Chain() { s->prof_chain = false; s->chain_ev = nullptr; }
    } chain(s, split);
    const int L = s->cfg.finest_level;
    const int post = want_norm ? 2 : 0;
    s->norm_blocks_ready = 0;
    bool zin = false;
    if (zero_start)
        if (int rc = zero_start_u(s, &zin)) return rc;
    if (split) {
        const bool zin_next = descend(s, L, zin);
        if (int rc = coarse_part_graph(s, L - 1, zin_next)) return rc;       // PS:617
        ascend(s, L, post);
    } else {
        vcycle(s, L, zin, post);
    }
    return want_norm ? enqueue_norm(s, s->lv[L], s->lv[L].u, s->lv[L].b, MGX_PROF_NORM_FINE) : MGX_OK;
}

// With profiling off the whole body is one cached graph (tag: want_norm | zero_start << 1), the host synchronisation
// that reads the norm outside it; cfg.profile = 2 splits it; cfg.profile = 1, MIXED and MGX_GRAPH=0 launch eagerly.
int cycle_body(mgx_solver* s, bool want_norm, bool zero_start, double* r)
{
    const bool split = s->cfg.profile == 2 && s->use_graph && !s->mixed && s->cfg.finest_level > s->cfg.coarsest_level;
    const bool whole = s->use_graph && !s->cfg.profile && !s->mixed;
    auto body = [&] { return enqueue_cycle(s, want_norm, zero_start, split); };
    const hipGraphExec_t exec = whole ? cached_graph(s, (want_norm ? 1u : 0u) | (zero_start ? 2u : 0u), body) : nullptr;
    if (exec) {
        s->norm_blocks_ready = 0;
        HIPCHK(s, hipGraphLaunch(exec, s->stream));
    } else if (int rc = body()) {
        return rc;
    }
    if (!want_norm) return MGX_OK;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    *r = std::sqrt(*s->sum_host);
    return MGX_OK;
}

// the common end of the solve entry points (the stream is idle): the statistics and the residual history
void finish_solve(mgx_stats* stats, double* history, int history_cap, const std::vector<double>& hist, int cycles, bool converged,
                  std::chrono::steady_clock::time_point t0, double fine_updates)
{
    if (stats) {
        stats->cycles = cycles;
        stats->initial_residual = hist.front();
        stats->final_residual = hist.back();
        stats->converged = converged ? 1 : 0;
        stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        stats->fine_updates = fine_updates;
        stats->history_len = (int)hist.size();
    }
    if (history)
        for (int i = 0; i < (int)hist.size() && i < history_cap; ++i) history[i] = hist[i];
}

double pow2_floor(double x)
{
    int e;
    (void)std::frexp(x, &e);
    return std::ldexp(1.0, e - 1);
}

Level* pick(mgx_solver* s, int level, int which, void** grid)
{
    Level* l = &s->lv[level];
    if (s->mixed && level == s->cfg.finest_level) l = &s->fine64;
    switch (which) {
        case MGX_VEC_U: *grid = l->u; break;
        case MGX_VEC_B: *grid = l->b; break;
        case MGX_VEC_R: *grid = l->r; break;
        default: *grid = nullptr;
    }
    return l;
}

// non-homogeneous Dirichlet data: b_ij += g of the boundary neighbours (mgx_set_rhs_dirichlet)
template <typename T>
void fold_ring(std::vector<T>& b, const T* ring, size_t n)
{
    const size_t N = n + 1;
    const T* top = ring;                 // row 0, columns 0..N
    const T* bot = ring + (N + 1);       // row N, columns 0..N
    const T* lef = ring + 2 * (N + 1);   // column 0, rows 1..N-1
    const T* rig = lef + (N - 1);        // column N, rows 1..N-1
    for (size_t j = 0; j < n; ++j) {
        b[j] += top[j + 1];                          // interior row 1 touches boundary row 0
        b[(n - 1) * n + j] += bot[j + 1];            // interior row N-1 touches boundary row N
    }
    for (size_t i = 0; i < n; ++i) {
        b[i * n] += lef[i];                          // interior column 1 touches boundary column 0
        b[i * n + (n - 1)] += rig[i];
    }
}

// the milliseconds the GPU spends on what `enqueue` puts on the handle's stream, between two events that are
// destroyed on every path
template <typename Enqueue>
int time_on_stream(mgx_solver* s, double* ms, Enqueue enqueue)
{
    hipEvent_t a = nullptr, b = nullptr;
    auto timed = [&]() -> int {
        HIPCHK(s, hipEventCreate(&a));
        HIPCHK(s, hipEventCreate(&b));
        HIPCHK(s, hipEventRecord(a, s->stream));
        enqueue();
        HIPCHK(s, hipEventRecord(b, s->stream));
        HIPCHK(s, hipEventSynchronize(b));
        HIPCHK(s, hipGetLastError());
        float f = 0.f;
        HIPCHK(s, hipEventElapsedTime(&f, a, b));
        *ms = f;
        return MGX_OK;
    };
    const int rc = timed();
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    return rc;
}

} // namespace

#include "mgx_dist.hpp"

// entry points that make no sense on a multi-GPU handle
#define NO_DIST(s)                                                                        \
    if ((s)->dist) return (s)->fail(MGX_ERR_STATE, "not available on a multi-GPU handle (see mgx.h, Multi-GPU)");

#include "mgx_krylov_host.hpp"
#include "mgx_multi_host.hpp"

// mgx_create behind its argument list (below): refine_shadow creates the float copy with it
static int create_solver(const mgx_config* cfg, const mgx_solver* like, mgx_handle* out);

#include "mgx_refine_host.hpp"
#include "mgx_multi_refine_host.hpp"
#include "mgx_eig_host.hpp"
#include "mgx_eig_many_host.hpp"
#include "mgx_theta_host.hpp"
#include "mgx_newton_host.hpp"
#include "mgx_newton_steps_host.hpp"
#include "mgx_quasi_host.hpp"

// =====================================================================================
// C-ABI
// =====================================================================================
extern "C" {

int mgx_config_default(mgx_config* c)
{
    if (!c) return MGX_ERR_INVALID;
    c->finest_level = 10;      // PS:17
    c->coarsest_level = 7;     // PS:18
    c->mu0 = 30;               // PS:20
    c->mu1 = 10;               // PS:21
    c->mu2 = 10;               // PS:22
    c->omega = 2.0 / 3.0;      // PS:127
    c->smoother = MGX_SMOOTHER_JACOBI;
    c->dtype = MGX_DTYPE_F64;
    c->schedule = MGX_SCHEDULE_FMG;   // PS:727
    c->restrict_mode = MGX_RESTRICT_CONSISTENT;
    c->bottom = MGX_BOTTOM_EXACT;
    c->device = 0;
    c->profile = 0;
    c->n_gpus = 0;             // PS:659: one queue
    c->cut_level = 0;
    for (int i = 0; i < MGX_MAX_GPUS; ++i) c->devices[i] = -1;
    c->arith = MGX_ARITH_SEPARATE;
    c->op = MGX_OPERATOR_POISSON;
    return MGX_OK;
}

const char* mgx_status_string(int st)
{
    switch (st) {
        case MGX_OK: return "ok";
        case MGX_ERR_INVALID: return "invalid argument";
        case MGX_ERR_NO_DEVICE: return "no usable HIP device";
        case MGX_ERR_HIP: return "HIP runtime error";
        case MGX_ERR_ALLOC: return "device allocation failed";
        case MGX_ERR_STATE: return "invalid state";
        default: return "unknown status";
    }
}

const char* mgx_last_error(mgx_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int mgx_level_n(int level) { return (level >= 1 && level < 31) ? (1 << level) - 1 : -1; }

long mgx_level_pitch(int level, int dtype)
{
    if (level < 1 || level > 20 || (dtype != MGX_DTYPE_F32 && dtype != MGX_DTYPE_F64)) return -1;
    return level_pitch(level, dtype);
}

// mgx_create.  like (may be null): the handle whose float copy this one is (mgx_solve_refine) - its stream and its knobs
// instead of a stream of its own and the environment's
static int create_solver(const mgx_config* cfg, const mgx_solver* like, mgx_handle* out)
{
    if (!cfg || !out) { g_create_error = "null argument"; return MGX_ERR_INVALID; }
    *out = nullptr;
    // level 2 (N = 4) is the smallest grid whose rows hold whole 16-byte vectors
    // in both precisions; level 8 (255^2) bounds the dense sine-transform solve.
    if (cfg->coarsest_level < 2 || cfg->finest_level < cfg->coarsest_level || cfg->finest_level > 15 ||
        cfg->mu0 < 0 || cfg->mu1 < 0 || cfg->mu2 < 0 || !(cfg->omega > 0.0 && cfg->omega < 2.0) ||
        cfg->smoother < 0 || cfg->smoother > MGX_SMOOTHER_COLOR_SGS || cfg->smoother == 3 || cfg->smoother == 7 || cfg->dtype < 0 || cfg->dtype > 2 ||
        cfg->schedule < 0 || cfg->schedule > 1 || cfg->restrict_mode < 0 || cfg->restrict_mode > MGX_RESTRICT_INJECT4 ||
        cfg->bottom < 0 || cfg->bottom > 1 || cfg->arith < 0 || cfg->arith > 1 || (cfg->op != MGX_OPERATOR_POISSON && cfg->op != MGX_OPERATOR_STENCIL5 && cfg->op != MGX_OPERATOR_GALERKIN)) {
        g_create_error = "invalid configuration";
        return MGX_ERR_INVALID;
    }
    const bool galerkin = (cfg->op == MGX_OPERATOR_GALERKIN);
    const bool var = (cfg->op == MGX_OPERATOR_STENCIL5) || galerkin;
    if (cfg->bottom == MGX_BOTTOM_EXACT && cfg->coarsest_level > (var ? 5 : 8)) {
        g_create_error = var ? "exact bottom solve of a general operator (dense inverse) supports coarsest_level <= 5"
                             : "exact bottom solve supports coarsest_level <= 8";
        return MGX_ERR_INVALID;
    }
    const bool cheby = (cfg->smoother == MGX_SMOOTHER_CHEBYSHEV);
    if (cheby && !var) {
        g_create_error = "MGX_SMOOTHER_CHEBYSHEV: op = MGX_OPERATOR_STENCIL5 or MGX_OPERATOR_GALERKIN only (the constant stencil has its fused and folded passes)";
        return MGX_ERR_INVALID;
    }
    const bool line = (cfg->smoother >= MGX_SMOOTHER_LINE_X && cfg->smoother <= MGX_SMOOTHER_LINE_ALT);
    const bool colour = (cfg->smoother == MGX_SMOOTHER_COLOR_GS || cfg->smoother == MGX_SMOOTHER_COLOR_SGS);
    if (colour && (!var || cfg->dtype == MGX_DTYPE_MIXED || cfg->arith != MGX_ARITH_SEPARATE || cfg->n_gpus > 1)) {
        g_create_error = "MGX_SMOOTHER_COLOR_GS / COLOR_SGS: op = MGX_OPERATOR_STENCIL5 or MGX_OPERATOR_GALERKIN, dtype F64 or F32, arith SEPARATE, one GPU";
        return MGX_ERR_INVALID;
    }
    if (line && (!var || cfg->dtype == MGX_DTYPE_MIXED || cfg->arith != MGX_ARITH_SEPARATE || cfg->n_gpus > 1)) {
        g_create_error = "MGX_SMOOTHER_LINE_X / LINE_Y / LINE_ALT: op = MGX_OPERATOR_STENCIL5 or MGX_OPERATOR_GALERKIN, dtype F64 or F32, arith SEPARATE, one GPU";
        return MGX_ERR_INVALID;
    }
    if (var && (cfg->dtype == MGX_DTYPE_MIXED || cfg->smoother == MGX_SMOOTHER_RBGS || cfg->arith != MGX_ARITH_SEPARATE || cfg->n_gpus > 1)) {
        g_create_error = cheby ? "MGX_SMOOTHER_CHEBYSHEV: dtype F64 or F32, arith SEPARATE, one GPU"
                       : galerkin ? "MGX_OPERATOR_GALERKIN: dtype F64 or F32, Jacobi or Chebyshev, arith SEPARATE, one GPU"
                                  : "MGX_OPERATOR_STENCIL5: dtype F64 or F32, Jacobi (MF:75-96) or Chebyshev, arith SEPARATE, one GPU";
        return MGX_ERR_INVALID;
    }
    if (galerkin && cfg->restrict_mode >= MGX_RESTRICT_INJECT) {
        g_create_error = "MGX_OPERATOR_GALERKIN: restrict_mode CONSISTENT or FW16 (R A P needs R = c P^T; injection has no variational meaning)";
        return MGX_ERR_INVALID;
    }
    if (cfg->restrict_mode >= MGX_RESTRICT_INJECT && (cfg->n_gpus > 1 || cfg->dtype == MGX_DTYPE_MIXED)) {
        g_create_error = "injection restriction (MF:122-130): single-GPU handles of dtype F64 or F32";
        return MGX_ERR_INVALID;
    }
    if (cfg->n_gpus > 1) return mgx_create_rank(cfg, -1, 1, nullptr, nullptr, out);
    log_runtime_libs("mgx_create");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        g_create_error = "no usable HIP device (libmgx has no CPU fallback)";
        return MGX_ERR_NO_DEVICE;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return MGX_ERR_HIP; }

    mgx_solver* s = new (std::nothrow) mgx_solver();
    if (!s) { g_create_error = "out of host memory"; return MGX_ERR_ALLOC; }
    s->cfg = *cfg;
    s->mixed = (cfg->dtype == MGX_DTYPE_MIXED);
    s->var = var;
    s->galerkin = galerkin;
    s->work_f64 = (cfg->dtype == MGX_DTYPE_F64);
    s->rows_per_chunk = like ? like->rows_per_chunk : env_int("MGX_ROWS", 0);
    s->fuse = like ? like->fuse : fuse_cfg();
    s->fuse.arith = cfg->arith;
    s->fold = like ? like->fold : env_int("MGX_FOLD", 1);
    s->use_zero_in = like ? like->use_zero_in : env_int("MGX_ZERO_IN", 1);
    s->use_graph = like ? like->use_graph : env_int("MGX_GRAPH", 1);
    s->small_visit = like ? like->small_visit : env_int("MGX_SMALL_VISIT", 1);
    s->colour = cfg->smoother == MGX_SMOOTHER_COLOR_GS ? 1 : cfg->smoother == MGX_SMOOTHER_COLOR_SGS ? 2 : 0;
    s->gs_fused = like ? like->gs_fused : env_int("MGX_GS_FUSED", 1);
    s->line_dirs = cfg->smoother == MGX_SMOOTHER_LINE_X ? 1 : cfg->smoother == MGX_SMOOTHER_LINE_Y ? 2 : cfg->smoother == MGX_SMOOTHER_LINE_ALT ? 3 : 0;
    int rc = MGX_OK;
    auto bail = [&](int code) { g_create_error = s->err; mgx_destroy(s); return code; };
    if (like) { s->stream = like->stream; s->own_stream = false; }
    else if (hipStreamCreate(&s->stream) != hipSuccess) { s->err = "hipStreamCreate failed"; return bail(MGX_ERR_HIP); }
    s->lv.resize(cfg->finest_level + 1);
    for (int l = cfg->coarsest_level; l <= cfg->finest_level; ++l)
        if ((rc = alloc_level(s, s->lv[l], l, s->work_f64)) != MGX_OK) return bail(rc);
    if (s->mixed && (rc = alloc_level(s, s->fine64, cfg->finest_level, true)) != MGX_OK) return bail(rc);
    if (var || cfg->restrict_mode >= MGX_RESTRICT_INJECT) {
        // these cycles form the residual as a grid (MF:150-153) before restricting it: allocate it now (nothing may be
        // allocated while a cycle is being captured into a graph)
        for (int l = cfg->coarsest_level + 1; l <= cfg->finest_level; ++l)
            if ((rc = ensure_r(s, s->lv[l])) != MGX_OK) return bail(rc);
    }
    if (galerkin && s->small_visit) {
        // k_small_visit's 64 KB of LDS at N = 64 in double: an attribute of the function, set outside any capture
        if (small_visit_prepare<double>() != hipSuccess || small_visit_prepare<float>() != hipSuccess) {
            s->err = "hipFuncSetAttribute failed for k_small_visit";
            return bail(MGX_ERR_HIP);
        }
    }
    if (var) {
        for (int l = cfg->coarsest_level; l <= cfg->finest_level; ++l) {
            s->lv[l].nine = galerkin && l < cfg->finest_level;
            if ((rc = var_alloc_level(s, s->lv[l])) != MGX_OK) return bail(rc);
            if (cheby) {
                // the direction d of the Chebyshev blocks; zeroed once: its ring and padding are never written
                Level& lv = s->lv[l];
                if (hipMalloc(&lv.cheb, lv.bytes) != hipSuccess) { s->err = "hipMalloc failed for the Chebyshev direction array"; return bail(MGX_ERR_ALLOC); }
                if (hipMemsetAsync(lv.cheb, 0, lv.bytes, s->stream) != hipSuccess) { s->err = "hipMemsetAsync failed"; return bail(MGX_ERR_HIP); }
            }
            if (line) {
                // the line factors; zeroed once: their ring and padding are never written.  hf / hb: k_line_y's levels of
                // more than one chunk only (MGX_LINE_CHUNK=<rows> overrides the launcher's rows per chunk)
                Level& lv = s->lv[l];
                lv.line_R = like ? like->lv[l].line_R : line_chunk_rows(lv.N, env_int("MGX_LINE_CHUNK", 0));
                std::vector<void**> arrays;
                for (int d = 0; d < 2; ++d)
                    if (s->line_dirs & (1 << d)) { arrays.push_back(&lv.line_m[d]); arrays.push_back(&lv.line_g[d]); }
                if ((s->line_dirs & 2) && line_chunks(lv.N, lv.line_R) > 1) { arrays.push_back(&lv.line_hf); arrays.push_back(&lv.line_hb); }
                for (void** p : arrays) {
                    if (hipMalloc(p, lv.bytes) != hipSuccess) { s->err = "hipMalloc failed for the line smoother's factor arrays"; return bail(MGX_ERR_ALLOC); }
                    if (hipMemsetAsync(*p, 0, lv.bytes, s->stream) != hipSuccess) { s->err = "hipMemsetAsync failed"; return bail(MGX_ERR_HIP); }
                }
            }
        }
        if (line && hipMalloc(&s->line_flag, sizeof(int)) != hipSuccess) { s->err = "hipMalloc failed for the line smoother's breakdown flag"; return bail(MGX_ERR_ALLOC); }
        if (cfg->bottom == MGX_BOTTOM_EXACT) {
            const size_t NN = (size_t)((1 << cfg->coarsest_level) - 1) * ((1 << cfg->coarsest_level) - 1);
            if (hipMalloc(&s->var_M, NN * NN * sizeof(double)) != hipSuccess || hipMalloc(&s->var_inv, NN * NN * sizeof(double)) != hipSuccess ||
                hipMalloc(&s->var_pm, NN * sizeof(double)) != hipSuccess || hipMalloc(&s->var_pi, NN * sizeof(double)) != hipSuccess) {
                s->err = "allocation of the coarsest operator's dense inverse failed";
                return bail(MGX_ERR_ALLOC);
            }
        }
    }
    s->mixed_fuse = like ? like->mixed_fuse : env_int("MGX_MIXED_FUSE", 1);
    // fine64.tmp: the out-of-place target of the fused update + residual pass
    if (s->mixed && !s->mixed_fuse) { (void)hipFree(s->fine64.tmp); s->fine64.tmp = nullptr; }
    // partial sums: the largest launch any norm kernel can make on the finest level
    {
        const int N = 1 << cfg->finest_level;
        long cap = 0;
        for (int rpc : {s->rows_per_chunk, 1}) {
            cap = std::max(cap, sumsq_blocks<double>(N, N, rpc));
            cap = std::max(cap, sumsq_blocks<float>(N, N, rpc));
        }
        if (N <= s->fuse.tile_max_n) cap = std::max(cap, (long)((N + 31) / 32) * ((N + 39) / 40));   // tiles >= 32 x 40
        s->partial_cap = cap + 8;
        if (hipMalloc(&s->partial, s->partial_cap * sizeof(double)) != hipSuccess ||
            hipMalloc(&s->sum_dev, sizeof(double)) != hipSuccess ||
            hipHostMalloc(&s->sum_host, sizeof(double)) != hipSuccess) {
            s->err = "allocation of reduction buffers failed";
            return bail(MGX_ERR_ALLOC);
        }
    }
    if (cfg->bottom == MGX_BOTTOM_EXACT && !var) {
        if (s->bottom.init((1 << cfg->coarsest_level) - 1) != hipSuccess) {
            s->err = "bottom solver allocation failed";
            return bail(MGX_ERR_ALLOC);
        }
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess) { s->err = "device initialisation failed"; return bail(MGX_ERR_HIP); }
    *out = s;
    return MGX_OK;
}

int mgx_create(const mgx_config* cfg, mgx_handle* out) { return create_solver(cfg, nullptr, out); }

int mgx_destroy(mgx_handle s)
{
    if (!s) return MGX_OK;
    if (s->shadow) { mgx_destroy(s->shadow); s->shadow = nullptr; }
    if (s->dist) { dist_free(s->dist); s->dist = nullptr; }
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (auto& l : s->lv) free_level(l);
    free_level(s->fine64);
    s->bottom.destroy();
    if (s->partial) (void)hipFree(s->partial);
    if (s->sum_dev) (void)hipFree(s->sum_dev);
    if (s->line_flag) (void)hipFree(s->line_flag);
    if (s->sum_host) (void)hipHostFree(s->sum_host);
    for (double* p : {s->var_M, s->var_inv, s->var_pm, s->var_pi}) if (p) (void)hipFree(p);
    s->kry.free();
    multi_free(s->multi);
    eig_free(s->eig);
    eig_many_free(s->eigm);
    reaction_free(s->rx);
    newton_free(s->nwt);
    quasi_free(s->qsi);
    drop_graphs(s);
    for (auto& p : s->ev_used) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto& p : s->ev_free) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    if (s->stream && s->own_stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return MGX_OK;
}

int mgx_graphs_cached(mgx_handle s)
{
    if (!s) return MGX_ERR_INVALID;
    if (s->dist) {
        // the replicated coarse levels of the first local slab replay their cycle from a graph
        mgx_handle c = s->dist->slabs[0].coarse;
        return (c && c->use_graph) ? (int)c->graphs.size() : -1;
    }
    if (!s->use_graph || s->cfg.profile == 1 || s->mixed) return -1;
    return (int)s->graphs.size();
}

int mgx_synchronize(mgx_handle s)
{
    if (!s) return MGX_ERR_INVALID;
    if (s->dist) return dist_sync(s, s->dist);
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return MGX_OK;
}

// ---- data ---------------------------------------------------------------------------
int mgx_set_level(mgx_handle s, int level, int which, const void* src, size_t count)
{
    if (!s || !src) return MGX_ERR_INVALID;
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    if (s->dist) {
        if (level != s->cfg.finest_level || (which != MGX_VEC_U && which != MGX_VEC_B))
            return s->fail(MGX_ERR_STATE, "multi-GPU handles exchange U and B of the finest level only");
        return dist_set(s, s->dist, which, src, count);
    }
    void* grid = nullptr;
    Level* l = pick(s, level, which, &grid);
    if (which == MGX_VEC_R) {
        int rc = ensure_r(s, *l);
        if (rc) return rc;
        grid = l->r;
    }
    if (!grid) return s->fail(MGX_ERR_INVALID, "unknown vector selector");
    return copy_in(s, *l, grid, src, count);
}

int mgx_get_level(mgx_handle s, int level, int which, void* dst, size_t count)
{
    if (!s || !dst) return MGX_ERR_INVALID;
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    if (s->dist) {
        if (level != s->cfg.finest_level || (which != MGX_VEC_U && which != MGX_VEC_B))
            return s->fail(MGX_ERR_STATE, "multi-GPU handles exchange U and B of the finest level only");
        return dist_get(s, s->dist, which, dst, count);
    }
    void* grid = nullptr;
    Level* l = pick(s, level, which, &grid);
    if (!grid) return s->fail(MGX_ERR_STATE, "vector not available (call mgx_residual first for MGX_VEC_R)");
    return copy_out(s, *l, grid, dst, count);
}

int mgx_set_level_device(mgx_handle s, int level, int which, const void* grid)
{
    if (!s || !grid) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    void* dst = nullptr;
    Level* l = pick(s, level, which, &dst);
    if (which == MGX_VEC_R) {
        int rc = ensure_r(s, *l);
        if (rc) return rc;
        dst = l->r;
    }
    if (!dst) return s->fail(MGX_ERR_INVALID, "unknown vector selector");
    HIPCHK(s, hipMemcpyAsync(dst, grid, l->bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return MGX_OK;
}

int mgx_get_level_device(mgx_handle s, int level, int which, void* grid)
{
    if (!s || !grid) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    void* src = nullptr;
    Level* l = pick(s, level, which, &src);
    if (!src) return s->fail(MGX_ERR_STATE, "vector not available");
    HIPCHK(s, hipMemcpyAsync(grid, src, l->bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return MGX_OK;
}

int mgx_zero_level(mgx_handle s, int level, int which)
{
    if (!s) return MGX_ERR_INVALID;
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    if (s->dist) {
        if (level != s->cfg.finest_level || which != MGX_VEC_U) return s->fail(MGX_ERR_STATE, "multi-GPU handles: only U of the finest level");
        return dist_zero_u(s, s->dist);
    }
    void* dst = nullptr;
    Level* l = pick(s, level, which, &dst);
    if (!dst) return s->fail(MGX_ERR_STATE, "vector not available");
    HIPCHK(s, hipMemsetAsync(dst, 0, l->bytes, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return MGX_OK;
}

int mgx_set_rhs(mgx_handle s, const void* b, size_t count) { return s ? mgx_set_level(s, s->cfg.finest_level, MGX_VEC_B, b, count) : MGX_ERR_INVALID; }
int mgx_set_rhs_dirichlet(mgx_handle s, const void* b, size_t count, const void* ring, size_t ring_count)
{
    if (!s || !b || !ring) return MGX_ERR_INVALID;
    const int L = s->cfg.finest_level;
    const size_t n = (size_t)((1 << L) - 1);
    if (count != n * n) return s->fail(MGX_ERR_INVALID, "vector length must be n*n with n = 2^level - 1");
    if (ring_count != 4 * (n + 1)) return s->fail(MGX_ERR_INVALID, "ring must hold 4 N boundary values, N = n + 1");
    const bool f64 = (s->cfg.dtype != MGX_DTYPE_F32);
    if (f64) {
        std::vector<double> t((const double*)b, (const double*)b + count);
        fold_ring<double>(t, (const double*)ring, n);
        return mgx_set_level(s, L, MGX_VEC_B, t.data(), count);
    }
    std::vector<float> t((const float*)b, (const float*)b + count);
    fold_ring<float>(t, (const float*)ring, n);
    return mgx_set_level(s, L, MGX_VEC_B, t.data(), count);
}

int mgx_set_guess(mgx_handle s, const void* u, size_t count) { return s ? mgx_set_level(s, s->cfg.finest_level, MGX_VEC_U, u, count) : MGX_ERR_INVALID; }
int mgx_get_solution(mgx_handle s, void* u, size_t count) { return s ? mgx_get_level(s, s->cfg.finest_level, MGX_VEC_U, u, count) : MGX_ERR_INVALID; }

int mgx_fill_rhs(mgx_handle s, int kind, double f)
{
    if (!s) return MGX_ERR_INVALID;
    if (kind < 0 || kind > 1) return s->fail(MGX_ERR_INVALID, "unknown rhs kind");
    if (s->dist) return dist_fill(s, s->dist, MGX_VEC_B, kind, f, 0);
    void* grid = nullptr;
    Level* l = pick(s, s->cfg.finest_level, MGX_VEC_B, &grid);
    const dim3 blk(256), grd((l->N + 1 + 255) / 256, l->N + 1);
    if (l->f64) hipLaunchKernelGGL(k_fill_rhs<double>, grd, blk, 0, s->stream, (double*)grid, l->N, l->pitch, kind, f);
    else hipLaunchKernelGGL(k_fill_rhs<float>, grd, blk, 0, s->stream, (float*)grid, l->N, l->pitch, kind, f);
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return MGX_OK;
}

int mgx_fill_guess_random(mgx_handle s, uint64_t seed)
{
    if (!s) return MGX_ERR_INVALID;
    if (s->dist) return dist_fill(s, s->dist, MGX_VEC_U, 0, 0.0, seed);
    void* grid = nullptr;
    Level* l = pick(s, s->cfg.finest_level, MGX_VEC_U, &grid);
    const dim3 blk(256), grd((l->N + 1 + 255) / 256, l->N + 1);
    if (l->f64) hipLaunchKernelGGL(k_fill_random<double>, grd, blk, 0, s->stream, (double*)grid, l->N, l->pitch, seed);
    else hipLaunchKernelGGL(k_fill_random<float>, grd, blk, 0, s->stream, (float*)grid, l->N, l->pitch, seed);
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return MGX_OK;
}

// ---- general per-level operators (MF:16-41) ---------------------------------------------------
int mgx_set_stencil(mgx_handle s, int level, const void* c, const void* n, const void* so, const void* w, const void* e, size_t count)
{
    if (!s || !c || !n || !so || !w || !e) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->var) return s->fail(MGX_ERR_STATE, "handle was created with op = MGX_OPERATOR_POISSON (the constant stencil needs no coefficients)");
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    if (s->galerkin && level != s->cfg.finest_level)
        return s->fail(MGX_ERR_STATE, "MGX_OPERATOR_GALERKIN: only the finest operator is the caller's (coarse levels are R A P: mgx_build_galerkin)");
    Level& l = s->lv[level];
    const void* src[5] = {c, n, so, w, e};
    for (int q = 0; q < 5; ++q) {
        int rc = copy_in(s, l, l.A[q], src[q], count);
        if (rc) return rc;
    }
    if (s->galerkin) { l.nine = false; galerkin_invalidate(s); return MGX_OK; }     // (corner arrays of an earlier nine-point operator: kept, not read)
    return var_build(s, l);
}

// the guards mgx_set_stencil9 and mgx_set_tensor share; nullptr: the handle takes a nine-point finest operator
static const char* nine_finest_refusal(const mgx_solver* s)
{
    if (!s->galerkin)
        return "nine-point finest operators need op = MGX_OPERATOR_GALERKIN (STENCIL5 and POISSON hierarchies are five-point on every level)";
    return nullptr;
}

int mgx_set_stencil9(mgx_handle s, int level, const void* c, const void* n, const void* so, const void* w, const void* e, const void* nw,
                     const void* ne, const void* sw, const void* se, size_t count)
{
    if (!s || !c || !n || !so || !w || !e || !nw || !ne || !sw || !se) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (const char* why = nine_finest_refusal(s)) return s->fail(MGX_ERR_STATE, why);
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    if (level != s->cfg.finest_level)
        return s->fail(MGX_ERR_STATE, "MGX_OPERATOR_GALERKIN: only the finest operator is the caller's (coarse levels are R A P: mgx_build_galerkin)");
    Level& l = s->lv[level];
    const size_t nn = (size_t)l.N - 1;
    if (count != nn * nn) return s->fail(MGX_ERR_INVALID, "vector length must be n*n with n = 2^level - 1");
    if (int rc = finest_corners(s, l)) return rc;
    const void* src[9] = {c, n, so, w, e, nw, ne, sw, se};
    for (int q = 0; q < 9; ++q)
        if (int rc = copy_in(s, l, l.A[q], src[q], count)) return rc;
    l.nine = true;
    galerkin_invalidate(s);
    return MGX_OK;
}

int mgx_set_tensor(mgx_handle s, const double* axx, const double* axy, const double* ayy, size_t count)
{
    if (!s || !axx || !axy || !ayy) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (const char* why = nine_finest_refusal(s)) return s->fail(MGX_ERR_STATE, why);
    Level& l = s->lv[s->cfg.finest_level];
    if (count != (size_t)(l.N + 1) * (size_t)(l.N + 1)) return s->fail(MGX_ERR_INVALID, "every tensor component must hold (N + 1)^2 nodal values, N = 2^finest_level");
    double* dev = nullptr;
    if (hipMalloc(&dev, 3 * count * sizeof(double)) != hipSuccess) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for the nodal tensor");
    int rc = finest_corners(s, l);
    const double* src[3] = {axx, axy, ayy};
    for (int k = 0; k < 3 && rc == MGX_OK; ++k)
        if (hipMemcpyAsync(dev + k * count, src[k], count * sizeof(double), hipMemcpyHostToDevice, s->stream) != hipSuccess)
            rc = s->fail(MGX_ERR_HIP, "copy of the nodal tensor failed");
    if (rc == MGX_OK) {
        const dim3 blk(256), grd((l.N + 1 + 255) / 256, l.N + 1);
        with_float_type(l.f64, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL((k_var_from_tensor<T>), grd, blk, 0, s->stream, dev, dev + count, dev + 2 * count, out9(op9_of<T>(l)), l.N, l.pitch);
        });
        if (hipGetLastError() != hipSuccess) rc = s->fail(MGX_ERR_HIP, "launch of the tensor discretisation failed");
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess && rc == MGX_OK) rc = s->fail(MGX_ERR_HIP, "discretising the nodal tensor failed");
    (void)hipFree(dev);
    if (rc == MGX_OK) { l.nine = true; galerkin_invalidate(s); }
    return rc;
}

int mgx_set_coefficient(mgx_handle s, const double* a_nodes, size_t count)
{
    if (!s || !a_nodes) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->var) return s->fail(MGX_ERR_STATE, "handle was created with op = MGX_OPERATOR_POISSON");
    const int Lf = s->cfg.finest_level, Nf = 1 << Lf;
    if (count != (size_t)(Nf + 1) * (size_t)(Nf + 1)) return s->fail(MGX_ERR_INVALID, "coefficient must hold (N + 1)^2 nodal values, N = 2^finest_level");
    double* dev = nullptr;
    if (hipMalloc(&dev, count * sizeof(double)) != hipSuccess) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for the nodal coefficient");
    int rc = MGX_OK;
    if (hipMemcpyAsync(dev, a_nodes, count * sizeof(double), hipMemcpyHostToDevice, s->stream) != hipSuccess) rc = s->fail(MGX_ERR_HIP, "copy of the nodal coefficient failed");
    for (int lv = s->galerkin ? Lf : s->cfg.coarsest_level; lv <= Lf && rc == MGX_OK; ++lv) {
        Level& l = s->lv[lv];
        const dim3 blk(256), grd((l.N + 1 + 255) / 256, l.N + 1);
        const int q = 1 << (Lf - lv);
        with_float_type(l.f64, [&](auto tag) {
            using T = decltype(tag);
            hipLaunchKernelGGL((k_var_from_nodes<T>), grd, blk, 0, s->stream, dev, Nf, q, out9(op9_of<T>(l)), l.N, l.pitch);
        });
        if (!s->galerkin) rc = var_build(s, l);
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess && rc == MGX_OK) rc = s->fail(MGX_ERR_HIP, "sampling the nodal coefficient failed");
    (void)hipFree(dev);
    if (s->galerkin && rc == MGX_OK) { s->lv[Lf].nine = false; galerkin_invalidate(s); }
    return rc;
}

int mgx_get_stencil(mgx_handle s, int level, int which, void* dst, size_t count)
{
    if (!s || !dst) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->var) return s->fail(MGX_ERR_STATE, "handle was created with op = MGX_OPERATOR_POISSON");
    if (!level_ok(s, level) || which < 0 || which > 9) return s->fail(MGX_ERR_INVALID, "level or array selector out of range");
    Level& l = s->lv[level];
    if (l.nine) return s->fail(MGX_ERR_STATE, "nine-point operator (a coarse level, or a nine-point finest level, of a GALERKIN handle): use mgx_get_stencil9");
    if (!l.stencil_set) return s->fail(MGX_ERR_STATE, "operator of this level not set");
    if (s->galerkin && which >= 5 && !s->gal_built) return s->fail(MGX_ERR_STATE, "Galerkin hierarchy not built (mgx_build_galerkin)");
    return copy_out(s, l, which < 5 ? l.A[which] : l.J[which - 5], dst, count);
}

int mgx_build_galerkin(mgx_handle s)
{
    if (!s) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->galerkin) return s->fail(MGX_ERR_STATE, "handle was not created with op = MGX_OPERATOR_GALERKIN");
    if (!s->lv[s->cfg.finest_level].stencil_set)
        return s->fail(MGX_ERR_STATE, "finest operator not set (mgx_set_stencil / mgx_set_coefficient / mgx_set_stencil9 / mgx_set_tensor)");
    return s->work_f64 ? galerkin_build_t<double>(s, MGX_TRANSFER_BILINEAR) : galerkin_build_t<float>(s, MGX_TRANSFER_BILINEAR);
}

int mgx_build_galerkin_transfer(mgx_handle s, int transfer)
{
    if (!s) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->galerkin) return s->fail(MGX_ERR_STATE, "handle was not created with op = MGX_OPERATOR_GALERKIN");
    if (transfer != MGX_TRANSFER_BILINEAR && transfer != MGX_TRANSFER_OPERATOR)
        return s->fail(MGX_ERR_INVALID, "transfer must be MGX_TRANSFER_BILINEAR or MGX_TRANSFER_OPERATOR");
    if (!s->lv[s->cfg.finest_level].stencil_set)
        return s->fail(MGX_ERR_STATE, "finest operator not set (mgx_set_stencil / mgx_set_coefficient / mgx_set_stencil9 / mgx_set_tensor)");
    return s->work_f64 ? galerkin_build_t<double>(s, transfer) : galerkin_build_t<float>(s, transfer);
}

int mgx_get_transfer(mgx_handle s, int* transfer)
{
    if (!s || !transfer) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->galerkin) return s->fail(MGX_ERR_STATE, "handle was not created with op = MGX_OPERATOR_GALERKIN");
    if (!s->gal_built) return s->fail(MGX_ERR_STATE, "Galerkin hierarchy not built (mgx_build_galerkin)");
    *transfer = s->transfer;
    return MGX_OK;
}

int mgx_get_lambda_max(mgx_handle s, int level, double* out)
{
    if (!s || !out) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->var) return s->fail(MGX_ERR_STATE, "handle was created with op = MGX_OPERATOR_POISSON (g = 2 for the constant stencil)");
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    if (s->galerkin && !s->gal_built) return s->fail(MGX_ERR_STATE, "Galerkin hierarchy not built (mgx_build_galerkin)");
    if (!s->lv[level].stencil_set) return s->fail(MGX_ERR_STATE, "operator of this level not set");
    *out = s->lv[level].lambda_g;
    return MGX_OK;
}

int mgx_get_line_factor(mgx_handle s, int level, int dir, int which, void* dst, size_t count)
{
    if (!s || !dst) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->line_dirs) return s->fail(MGX_ERR_STATE, "handle was not created with a line smoother (MGX_SMOOTHER_LINE_X / LINE_Y / LINE_ALT)");
    if (!level_ok(s, level) || dir < 0 || dir > 1 || which < 0 || which > 1) return s->fail(MGX_ERR_INVALID, "level, direction or array selector out of range");
    if (!(s->line_dirs & (1 << dir))) return s->fail(MGX_ERR_STATE, dir == 0 ? "the handle's smoother has no x-lines (MGX_SMOOTHER_LINE_Y)" : "the handle's smoother has no y-lines (MGX_SMOOTHER_LINE_X)");
    if (s->galerkin && !s->gal_built) return s->fail(MGX_ERR_STATE, "Galerkin hierarchy not built (mgx_build_galerkin)");
    if (!s->lv[level].stencil_set) return s->fail(MGX_ERR_STATE, "operator of this level not set");
    Level& l = s->lv[level];
    return copy_out(s, l, which == 0 ? l.line_m[dir] : l.line_g[dir], dst, count);
}

int mgx_get_line_chunks(mgx_handle s, int level, int* rows, int* chunks)
{
    if (!s || !rows || !chunks) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!(s->line_dirs & 2)) return s->fail(MGX_ERR_STATE, "the handle's smoother has no y-lines (MGX_SMOOTHER_LINE_Y / LINE_ALT)");
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    *rows = s->lv[level].line_R;
    *chunks = line_chunks(s->lv[level].N, s->lv[level].line_R);
    return MGX_OK;
}

int mgx_get_prolongation(mgx_handle s, int level, int which, void* dst, size_t count)
{
    if (!s || !dst) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->galerkin) return s->fail(MGX_ERR_STATE, "handle was not created with op = MGX_OPERATOR_GALERKIN");
    if (level <= s->cfg.coarsest_level || level > s->cfg.finest_level || which < 0 || which > 7)
        return s->fail(MGX_ERR_INVALID, "level or array selector out of range");
    if (!s->gal_built) return s->fail(MGX_ERR_STATE, "Galerkin hierarchy not built (mgx_build_galerkin)");
    if (s->transfer != MGX_TRANSFER_OPERATOR)
        return s->fail(MGX_ERR_STATE, "the hierarchy was built with MGX_TRANSFER_BILINEAR: its weights are 1/2 and 1/4 and are not stored");
    Level& c = s->lv[level - 1];
    return copy_out(s, c, c.wt[which], dst, count);
}

int mgx_get_stencil9(mgx_handle s, int level, int which, void* dst, size_t count)
{
    if (!s || !dst) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (!s->galerkin) return s->fail(MGX_ERR_STATE, "handle was not created with op = MGX_OPERATOR_GALERKIN");
    if (!level_ok(s, level) || which < 0 || which > 17) return s->fail(MGX_ERR_INVALID, "level or array selector out of range");
    if (!s->gal_built) return s->fail(MGX_ERR_STATE, "Galerkin hierarchy not built (mgx_build_galerkin)");
    Level& l = s->lv[level];
    // 0..8: c, n, s, w, e, nw, ne, sw, se;  9: D_inv;  10..17: R_n, R_s, R_w, R_e, R_nw, R_ne, R_sw, R_se
    const void* src = which < 9 ? l.A[which] : l.J[which - 9];
    const int slot = which < 9 ? which : which - 9;
    if (!src || (!l.nine && slot >= 5)) {                     // corners of a five-point finest level (arrays of an earlier nine-point operator: not read)
        const size_t n = (size_t)l.N - 1;
        if (count != n * n) return s->fail(MGX_ERR_INVALID, "vector length must be n*n with n = 2^level - 1");
        std::memset(dst, 0, count * l.esize());
        return MGX_OK;
    }
    return copy_out(s, l, src, dst, count);
}

// ---- operators ------------------------------------------------------------------------
// On a MIXED handle the finest level exists twice: the double u, b the accessors address
// (mgx_set_level / mgx_get_level / mgx_set_rhs ...) and the float correction / residual scratch of
// the inner cycle, which is what the working hierarchy holds at that level.  An operator or
// schedule call there would silently act on the scratch pair: refuse it (only mgx_solve, and
// operators on the coarser float levels, are meaningful on a MIXED handle).
#define MIXED_GUARD(lvl)                                                                  \
    if (s->mixed && (lvl) == s->cfg.finest_level)                                         \
        return s->fail(MGX_ERR_STATE, "dtype MIXED: operators and schedules are not defined on the finest level " \
                                      "(double data, float inner cycle); use mgx_solve, or a F64 / F32 handle");

#define OP_PROLOGUE(lvl_min)                                                              \
    if (!s) return MGX_ERR_INVALID;                                                       \
    NO_DIST(s)                                                                            \
    if (level < (lvl_min) || level > s->cfg.finest_level)                                 \
        return s->fail(MGX_ERR_INVALID, "level out of range for this operator");          \
    MIXED_GUARD(level)                                                                    \
    if (int vr__ = var_ready(s, s->cfg.coarsest_level, level)) return vr__;

#define OP_EPILOGUE                                                                       \
    HIPCHK(s, hipGetLastError());                                                         \
    HIPCHK(s, hipStreamSynchronize(s->stream));                                           \
    return MGX_OK;

int mgx_smooth(mgx_handle s, int level, int mu)
{
    OP_PROLOGUE(s->cfg.coarsest_level)
    if (mu < 0) return s->fail(MGX_ERR_INVALID, "mu must be >= 0");
    smooth(s, level, mu);
    OP_EPILOGUE
}

int mgx_residual(mgx_handle s, int level)
{
    OP_PROLOGUE(s->cfg.coarsest_level)
    Level& l = s->lv[level];
    int rc = ensure_r(s, l);
    if (rc) return rc;
    residual_level<0>(s, l, l.u, l.b, l.r);
    OP_EPILOGUE
}

int mgx_restrict(mgx_handle s, int level)
{
    OP_PROLOGUE(s->cfg.coarsest_level + 1)
    restrict_level(s, level, true, true);
    OP_EPILOGUE
}

int mgx_restrict_rhs(mgx_handle s, int level)
{
    OP_PROLOGUE(s->cfg.coarsest_level + 1)
    restrict_level(s, level, false, false);
    OP_EPILOGUE
}

int mgx_prolong_add(mgx_handle s, int level)
{
    OP_PROLOGUE(s->cfg.coarsest_level + 1)
    prolong_level(s, level, true);
    OP_EPILOGUE
}

int mgx_prolong(mgx_handle s, int level)
{
    OP_PROLOGUE(s->cfg.coarsest_level + 1)
    prolong_level(s, level, false);
    OP_EPILOGUE
}

int mgx_bottom_solve(mgx_handle s)
{
    if (!s) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (s->cfg.bottom != MGX_BOTTOM_EXACT) return s->fail(MGX_ERR_STATE, "handle was created with bottom = SMOOTH");
    MIXED_GUARD(s->cfg.coarsest_level)
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.coarsest_level)) return vr;
    bottom_solve(s);
    OP_EPILOGUE
}

int mgx_residual_norm(mgx_handle s, int level, double* out)
{
    if (!s || !out) return MGX_ERR_INVALID;
    if (!level_ok(s, level)) return s->fail(MGX_ERR_INVALID, "level out of range");
    if (s->dist) {
        if (level != s->cfg.finest_level) return s->fail(MGX_ERR_STATE, "multi-GPU handles: residual norm of the finest level only");
        return dist_norm(s, s->dist, out);
    }
    if (int vr = var_ready(s, level, level)) return vr;
    void* gu = nullptr; void* gb = nullptr;
    Level* l = pick(s, level, MGX_VEC_U, &gu);
    (void)pick(s, level, MGX_VEC_B, &gb);
    return residual_norm_grid(s, *l, gu, gb, out, level == s->cfg.finest_level ? MGX_PROF_NORM_FINE : MGX_PROF_COARSE);
}

int mgx_vcycle(mgx_handle s, int level)
{
    if (s && s->dist) {
        if (level != s->cfg.finest_level) return s->fail(MGX_ERR_STATE, "multi-GPU handles: V-cycles from the finest level only");
        int rc = dist_vcycle(s, s->dist);
        return rc ? rc : dist_sync(s, s->dist);
    }
    OP_PROLOGUE(s->cfg.coarsest_level)
    vcycle(s, level);
    OP_EPILOGUE
}

int mgx_set_cycle(mgx_handle s, int cycle)
{
    if (!s) return MGX_ERR_INVALID;
    if (cycle != MGX_CYCLE_V && cycle != MGX_CYCLE_W && cycle != MGX_CYCLE_F)
        return s->fail(MGX_ERR_INVALID, "cycle must be MGX_CYCLE_V, MGX_CYCLE_W or MGX_CYCLE_F");
    if (s->dist) return s->fail(MGX_ERR_STATE, "mgx_set_cycle: multi-GPU handles run V-cycles only (the slab plan has no second coarse visit)");
    if (s->mixed) return s->fail(MGX_ERR_STATE, "mgx_set_cycle: dtype MIXED handles run V-cycles only; use a F64 or F32 handle");
    if (!s->var)
        return s->fail(MGX_ERR_STATE, "mgx_set_cycle: op = MGX_OPERATOR_POISSON handles run V-cycles only; W- and F-cycles are for "
                                      "MGX_OPERATOR_STENCIL5 and MGX_OPERATOR_GALERKIN");
    drop_graphs(s);                                           // a captured cycle is a cycle of the old kind: recapture
    s->cycle = cycle;
    if (s->shadow) { drop_graphs(s->shadow); s->shadow->cycle = cycle; }      // mgx_solve_refine's float cycle: the same kind
    return MGX_OK;
}

int mgx_get_cycle(mgx_handle s, int* cycle)
{
    if (!s) return MGX_ERR_INVALID;
    if (!cycle) return s->fail(MGX_ERR_INVALID, "null argument");
    *cycle = s->cycle;
    return MGX_OK;
}

int mgx_vcycle_zero(mgx_handle s)
{
    if (!s) return MGX_ERR_INVALID;
    NO_DIST(s)
    MIXED_GUARD(s->cfg.finest_level)
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    double unused = 0.0;
    int rc = cycle_body(s, false, true, &unused);
    if (rc) return rc;
    OP_EPILOGUE
}

int mgx_fmg(mgx_handle s)
{
    if (!s) return MGX_ERR_INVALID;
    if (s->dist) {
        int rc = dist_fmg(s, s->dist);
        return rc ? rc : dist_sync(s, s->dist);
    }
    MIXED_GUARD(s->cfg.finest_level)
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    int rc = fmg(s);
    if (rc) return rc;
    OP_EPILOGUE
}

// ---- solve ----------------------------------------------------------------------------
int mgx_solve(mgx_handle s, double tol, int max_cycles, mgx_stats* stats, double* history, int history_cap)
{
    if (!s || max_cycles < 0 || !(tol >= 0.0)) return MGX_ERR_INVALID;
    if (s->dist) return dist_solve(s, s->dist, tol, max_cycles, stats, history, history_cap);
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    const int L = s->cfg.finest_level;
    const bool do_fmg = (s->cfg.schedule == MGX_SCHEDULE_FMG);
    std::vector<double> hist;
    hist.reserve(max_cycles + 1);
    s->fine_updates = 0.0;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    const auto t0 = std::chrono::steady_clock::now();
    int rc = MGX_OK;
    double r = 0.0;
    int k = 0;

    if (!s->mixed) {
        Level& l = s->lv[L];
        if ((rc = residual_norm_grid(s, l, l.u, l.b, &r, MGX_PROF_NORM_FINE))) return rc;
        hist.push_back(r);
        for (k = 0; k < max_cycles; ++k) {
            if (hist[k] <= tol * hist[0]) break;
            s->norm_blocks_ready = 0;
            if (k == 0 && do_fmg) {
                if ((rc = fmg(s))) return rc;
                if ((rc = residual_norm_grid(s, l, l.u, l.b, &r, MGX_PROF_NORM_FINE))) return rc;
            } else if ((rc = cycle_body(s, true, false, &r))) {
                return rc;
            }
            hist.push_back(r);
        }
    } else {
        // BASELINE config 5: double residual and solution, float inner cycle on
        // the residual scaled by a power of two near its rms (exact scaling).
        Level& w = s->lv[L];            // float: u = e32, b = r32
        Level& d = s->fine64;           // double: u, b
        const double n = (double)(w.N - 1);
        const int rpc = s->rows_per_chunk;
        if ((rc = residual_norm_grid(s, d, d.u, d.b, &r, MGX_PROF_NORM_FINE))) return rc;
        hist.push_back(r);
        for (k = 0; k < max_cycles; ++k) {
            if (hist[k] <= tol * hist[0]) break;
            const Launch g = make_launch(d.N, 2, d.N - 1, rpc);
            double pending_scale = 0.0;
            if (k == 0 && do_fmg) {
                // ||b||: residual norm against a zero guess (FMG discards the guess, PS:630)
                HIPCHK(s, hipMemsetAsync(d.u, 0, d.bytes, s->stream));
                double bn = 0.0;
                if ((rc = residual_norm_grid(s, d, d.u, d.b, &bn, MGX_PROF_NORM_FINE))) return rc;
                const double scale = pow2_floor(bn / n);
                hipLaunchKernelGGL(k_scale_f64_to_f32, dim3(g.blocks), dim3(kBlock), 0, s->stream, (float*)w.b,
                                   (const double*)d.b, 1.0 / scale, d.N, d.pitch, w.pitch, 1, d.N, g.R, g.strips, g.chunks);
                if ((rc = fmg(s))) return rc;
                hipLaunchKernelGGL(k_axpy_f32_to_f64, dim3(g.blocks), dim3(kBlock), 0, s->stream, (double*)d.u,
                                   (const float*)w.u, scale, d.N, d.pitch, w.pitch, 1, d.N, g.R, g.strips, g.chunks, 1);
            } else {
                const double scale = pow2_floor(hist[k > 0 ? k - 1 : 0] / n);
                if (k == 0) {
                    // no scaled residual is pending yet: produce it now
                    Prof p(s, MGX_PROF_NORM_FINE, 2);
                    launch_residual<double, 2>((const double*)d.u, (const double*)d.b, w.b, w.pitch, s->partial,
                                               s->sum_dev, 1.0 / scale, d.N, d.pitch, 1, d.N, rpc, s->stream, s->partial_cap, d.rows);
                }
                double unused = 0.0;
                if ((rc = cycle_body(s, false, true, &unused))) return rc;   // e = M r from a PS:613-style zero guess
                pending_scale = scale;                        // u += scale * e still to be applied
                if (!(s->mixed_fuse && d.tmp)) {
                    hipLaunchKernelGGL(k_axpy_f32_to_f64, dim3(g.blocks), dim3(kBlock), 0, s->stream, (double*)d.u,
                                       (const float*)w.u, scale, d.N, d.pitch, w.pitch, 1, d.N, g.R, g.strips, g.chunks, 0);
                    pending_scale = 0.0;
                }
            }
            // residual of the new iterate: its norm is hist[k+1]; the same pass
            // writes the float residual the next cycle consumes, scaled by the
            // power of two derived from hist[k] (known now).
            {
                const double next_scale = pow2_floor(hist[k] / n);
                Prof p(s, MGX_PROF_NORM_FINE, 2);
                if (pending_scale != 0.0) {
                    // the correction and the residual in one out-of-place pass (32 instead of 40 B per point)
                    // rows per wave of this pass (MGX_MIXED_ROWS; 0: the marching default of make_launch)
                    static const int mixed_rows = env_int("MGX_MIXED_ROWS", 0);
                    Launch gr = make_launch(d.N, 2, d.N - 1, mixed_rows > 0 ? mixed_rows : rpc);
                    if (gr.blocks > s->partial_cap) {
                        const int R = (int)(((long)gr.strips * (d.N - 1) / kWavesPerBlock + s->partial_cap - 9) / (s->partial_cap - 8)) + 1;
                        gr = make_launch(d.N, 2, d.N - 1, R);
                    }
                    hipLaunchKernelGGL(k_update_residual, dim3(gr.blocks), dim3(kBlock), 0, s->stream, (const double*)d.u,
                                       (const float*)w.u, (const double*)d.b, (double*)d.tmp, (float*)w.b, pending_scale,
                                       1.0 / next_scale, s->partial, d.N, d.pitch, w.pitch, 1, d.N, gr.R, gr.strips, gr.chunks);
                    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, s->stream, s->partial, gr.blocks, s->sum_dev);
                    std::swap(d.u, d.tmp);
                } else {
                    launch_residual<double, 2>((const double*)d.u, (const double*)d.b, w.b, w.pitch, s->partial,
                                               s->sum_dev, 1.0 / next_scale, d.N, d.pitch, 1, d.N, rpc, s->stream, s->partial_cap, d.rows);
                }
            }
            HIPCHK(s, hipMemcpyAsync(s->sum_host, s->sum_dev, sizeof(double), hipMemcpyDeviceToHost, s->stream));
            HIPCHK(s, hipStreamSynchronize(s->stream));
            hist.push_back(std::sqrt(*s->sum_host));
        }
    }
    HIPCHK(s, hipGetLastError());
    HIPCHK(s, hipStreamSynchronize(s->stream));
    finish_solve(stats, history, history_cap, hist, k, hist.back() <= tol * hist.front(), t0, s->fine_updates);
    return MGX_OK;
}

int mgx_solve_pcg(mgx_handle s, double tol, int max_iters, mgx_stats* stats, double* history, int history_cap)
{
    return krylov_solve(s, "mgx_solve_pcg", krylov_guard, nullptr, nullptr, tol, max_iters, stats, history, history_cap,
                        [](auto t) { return PcgMethod<decltype(t)>{}; });
}

int mgx_solve_gcr(mgx_handle s, double tol, int max_iters, int restart, mgx_stats* stats, double* history, int history_cap)
{
    static_assert(kGcrMaxRestart == MGX_GCR_MAX_RESTART, "mgx_krylov.hpp and mgx.h disagree");
    const char* bad_restart = (restart < 1 || restart > MGX_GCR_MAX_RESTART) ? "1 <= restart <= MGX_GCR_MAX_RESTART required" : nullptr;
    return krylov_solve(s, "mgx_solve_gcr", krylov_guard, bad_restart, nullptr, tol, max_iters, stats, history, history_cap,
                        [restart](auto t) { return GcrMethod<decltype(t)>{restart}; });
}

int mgx_time_gcr_pass(mgx_handle s, int pass, int j, int repeats, double* ms)
{
    if (!s || !ms || repeats < 1 || pass < MGX_GCR_PASS_UPDATE || pass > MGX_GCR_PASS_DIRECTION || j < 0 || j >= MGX_GCR_MAX_RESTART ||
        (pass == MGX_GCR_PASS_DOTS && j == 0))
        return s ? s->fail(MGX_ERR_INVALID, "mgx_time_gcr_pass: pass, 0 <= j < MGX_GCR_MAX_RESTART (dots: j >= 1) and repeats >= 1 required")
                 : MGX_ERR_INVALID;
    NO_DIST(s)
    if (s->mixed) return s->fail(MGX_ERR_STATE, "mgx_time_gcr_pass: dtype MIXED is not supported");
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    for (int i = 0; i <= j; ++i)
        if (!s->kry.Z[i] || !s->kry.Q[i] || !s->kry.x || !s->kry.sc)
            return s->fail(MGX_ERR_STATE, "mgx_time_gcr_pass: call mgx_solve_gcr with restart > j first (it allocates the basis)");
    return s->work_f64 ? gcr_time_pass<double>(s, pass, j, repeats, ms) : gcr_time_pass<float>(s, pass, j, repeats, ms);
}

int mgx_solve_refine(mgx_handle s, double tol, int max_cycles, mgx_stats* stats, double* history, int history_cap)
{
    if (!s) return MGX_ERR_INVALID;
    if (int rc = refine_guard(s, "mgx_solve_refine")) return rc;
    if (max_cycles < 0 || !(tol >= 0.0)) return s->fail(MGX_ERR_INVALID, "mgx_solve_refine: tol >= 0 and max_cycles >= 0 required");
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    if (int rc = refine_shadow(s)) return rc;
    mgx_solver* f = s->shadow;
    Level& d = s->lv[s->cfg.finest_level];
    const double n = (double)(d.N - 1);
    std::vector<double> hist;
    hist.reserve(max_cycles + 1);
    s->fine_updates = 0.0;
    f->fine_updates = 0.0;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    const auto t0 = std::chrono::steady_clock::now();
    double r = 0.0;
    if (int rc = residual_norm_grid(s, d, d.u, d.b, &r, MGX_PROF_NORM_FINE)) return rc;
    hist.push_back(r);
    int k = 0;
    for (k = 0; k < max_cycles; ++k) {
        if (hist[k] <= tol * hist[0]) break;
        // s_k: a power of two near the rms of the residual the float cycle is given (exact scaling, the rule of dtype MIXED)
        const double scale = pow2_floor(hist[k > 0 ? k - 1 : 0] / n);
        if (k == 0) {
            // no scaled residual is pending yet: produce it now
            Prof p(s, MGX_PROF_NORM_FINE, 2);
            refine_pass(s, false, 0.0, 1.0 / scale);
        }
        double unused = 0.0;
        if (int rc = cycle_body(f, false, true, &unused)) return s->fail(rc, "mgx_solve_refine: float cycle: " + f->err);    // e = M32 r32 from zero
        {
            // u += s_k e, the residual of the new iterate (its norm is hist[k + 1]) and the float residual the next cycle
            // consumes, scaled by the power of two derived from hist[k] (known now): one out-of-place pass
            Prof p(s, MGX_PROF_NORM_FINE, 2);
            refine_pass(s, true, scale, 1.0 / pow2_floor(hist[k] / n));
            std::swap(d.u, d.tmp);
        }
        HIPCHK(s, hipMemcpyAsync(s->sum_host, s->sum_dev, sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(s, hipStreamSynchronize(s->stream));
        hist.push_back(std::sqrt(*s->sum_host));
    }
    s->norm_blocks_ready = 0;                                 // partial[] holds this pass's sums, not a smoothing block's
    HIPCHK(s, hipGetLastError());
    HIPCHK(s, hipStreamSynchronize(s->stream));
    finish_solve(stats, history, history_cap, hist, k, hist.back() <= tol * hist.front(), t0, f->fine_updates);
    return MGX_OK;
}

int mgx_time_refine_pass(mgx_handle s, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || repeats < 1) return s->fail(MGX_ERR_INVALID, "mgx_time_refine_pass: repeats >= 1 required");
    if (int rc = refine_guard(s, "mgx_time_refine_pass")) return rc;
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    if (!s->shadow) return s->fail(MGX_ERR_STATE, "mgx_time_refine_pass: call mgx_solve_refine first (it creates the float copy of the hierarchy)");
    // scale 0, and the updated iterate stays in tmp (no swap): U and B are unchanged; the shadow's right-hand side is
    // rewritten (it has no meaning between two mgx_solve_refine calls)
    const int rc = time_on_stream(s, ms, [&] { for (int i = 0; i < repeats; ++i) refine_pass(s, true, 0.0, 1.0); });
    s->norm_blocks_ready = 0;
    if (rc == MGX_OK) *ms /= repeats;
    return rc;
}

int mgx_solve_refine_gcr(mgx_handle s, double tol, int max_iters, int restart, mgx_stats* stats, double* history, int history_cap)
{
    const char* bad_restart = (restart < 1 || restart > MGX_GCR_MAX_RESTART) ? "1 <= restart <= MGX_GCR_MAX_RESTART required" : nullptr;
    // (refine_guard admits F64 handles only: the method is the same for either tag)
    return krylov_solve(s, "mgx_solve_refine_gcr", refine_guard, bad_restart, refine_cycle_of, tol, max_iters, stats, history, history_cap,
                        [restart](auto) { return RefineGcrMethod{restart}; });
}

int mgx_time_refine_gcr_pass(mgx_handle s, int pass, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || repeats < 1 || pass < MGX_REFINE_GCR_PASS_UPDATE || pass > MGX_REFINE_GCR_PASS_DIRECTION)
        return s->fail(MGX_ERR_INVALID, "mgx_time_refine_gcr_pass: pass 0 or 1 and repeats >= 1 required");
    if (int rc = refine_guard(s, "mgx_time_refine_gcr_pass")) return rc;
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    if (!s->shadow || !s->kry.Z[0] || !s->kry.Q[0] || !s->kry.x || !s->kry.sc)
        return s->fail(MGX_ERR_STATE, "mgx_time_refine_gcr_pass: call mgx_solve_refine_gcr first (it creates the float copy of the hierarchy and the basis)");
    const Level& l = s->lv[s->cfg.finest_level];
    const Launch g = make_launch(l.N, 2, l.N - 1, s->rows_per_chunk);
    // the scalars zeroed, as in gcr_time_pass: alpha = 0, so the update leaves x and lv.b (the caller's b here) as they are; it
    // rewrites the shadow's right-hand side, the direction pass basis slot 0 (neither has a meaning between two solves)
    const KrylovView v = krylov_view(s);
    HIPCHK(s, hipMemsetAsync(v.sc, 0, kGcrScalars * sizeof(double), s->stream));
    const int rc = time_on_stream(s, ms, [&] {
        for (int i = 0; i < repeats; ++i) {
            if (pass == MGX_REFINE_GCR_PASS_UPDATE) refine_gcr_update(s, v, g, 0, 1.0);
            else refine_gcr_direction(s, v, g, 0, 1.0);
        }
    });
    if (rc == MGX_OK) *ms /= repeats;
    return rc;
}

// ---- measurement ------------------------------------------------------------------------
int mgx_profile_reset(mgx_handle s)
{
    if (!s) return MGX_ERR_INVALID;
    if (s->dist) {
        int rc = dist_prof_collect(s, s->dist);
        if (rc) return rc;
        for (int i = 0; i < MGX_PROF_COUNT; ++i) { s->dist->prof_ms[i] = 0.0; s->dist->prof_launches[i] = 0; s->dist->prof_sweeps[i] = 0; }
        return MGX_OK;
    }
    int rc = prof_collect(s);
    if (rc) return rc;
    for (int i = 0; i < MGX_PROF_COUNT; ++i) { s->prof_ms[i] = 0.0; s->prof_launches[i] = 0; s->prof_sweeps[i] = 0; }
    return MGX_OK;
}

int mgx_profile_get(mgx_handle s, mgx_profile* out)
{
    if (!s || !out) return MGX_ERR_INVALID;
    if (s->dist) {
        int rc = dist_prof_collect(s, s->dist);
        if (rc) return rc;
        for (int i = 0; i < MGX_PROF_COUNT; ++i) {
            out->ms[i] = s->dist->prof_ms[i]; out->launches[i] = s->dist->prof_launches[i]; out->sweeps[i] = s->dist->prof_sweeps[i];
        }
        return MGX_OK;
    }
    int rc = prof_collect(s);
    if (rc) return rc;
    for (int i = 0; i < MGX_PROF_COUNT; ++i) {
        out->ms[i] = s->prof_ms[i];
        out->launches[i] = s->prof_launches[i];
        out->sweeps[i] = s->prof_sweeps[i];
    }
    return MGX_OK;
}

int mgx_time_smoother(mgx_handle s, int sweeps, double* ms)
{
    if (!s || !ms || sweeps < 1) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (int vr = var_ready(s, s->cfg.finest_level, s->cfg.finest_level)) return vr;
    Level& l = s->lv[s->cfg.finest_level];
    return time_on_stream(s, ms, [&] {
        if (s->var) smooth_var(s, s->cfg.finest_level, kOwnSet, sweeps);
        else smooth_t(s, l, sweeps);
    });
}

// ---- mgx_solve_multi: up to MGX_MAX_RHS right-hand sides per operator read ---------------------------------------
int mgx_solve_multi(mgx_handle s, int nrhs, const void* b, void* u, double tol, int max_cycles, mgx_stats* stats, double* history,
                    int history_cap)
{
    static_assert(kMultiMax == MGX_MAX_RHS, "mgx_var.hpp and mgx.h disagree");
    if (!s) return MGX_ERR_INVALID;
    if (nrhs < 1 || nrhs > MGX_MAX_RHS) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi: 1 <= nrhs <= MGX_MAX_RHS required");
    if (!b || !u) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi: b and u must not be NULL");
    if (!(tol >= 0.0) || max_cycles < 0) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi: tol >= 0 and max_cycles >= 0 required");
    if (int rc = multi_guard(s, "mgx_solve_multi")) return rc;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return s->work_f64 ? multi_solve_t<double>(s, nrhs, b, u, tol, max_cycles, stats, history, history_cap)
                       : multi_solve_t<float>(s, nrhs, b, u, tol, max_cycles, stats, history, history_cap);
}

int mgx_time_multi_smoother(mgx_handle s, int nrhs, int sweeps, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || sweeps < 1 || nrhs < 1 || nrhs > MGX_MAX_RHS)
        return s->fail(MGX_ERR_INVALID, "mgx_time_multi_smoother: 1 <= nrhs <= MGX_MAX_RHS, sweeps >= 1 and ms required");
    if (int rc = multi_guard(s, "mgx_time_multi_smoother")) return rc;
    if (s->multi.cols < nrhs)
        return s->fail(MGX_ERR_STATE, "mgx_time_multi_smoother: call mgx_solve_multi with at least this nrhs first (it allocates the columns)");
    const MultiSet a = multi_all(nrhs);
    return time_on_stream(s, ms, [&] {
        smooth_var(s, s->cfg.finest_level, a, sweeps);
    });
}

// ---- mgx_solve_multi_gcr: restarted GCR on up to MGX_MAX_RHS right-hand sides per operator read ------------------------
int mgx_solve_multi_gcr(mgx_handle s, int nrhs, const void* b, void* u, double tol, int max_iters, int restart, mgx_stats* stats,
                        double* history, int history_cap)
{
    if (!s) return MGX_ERR_INVALID;
    if (nrhs < 1 || nrhs > MGX_MAX_RHS) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi_gcr: 1 <= nrhs <= MGX_MAX_RHS required");
    if (!b || !u) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi_gcr: b and u must not be NULL");
    if (!(tol >= 0.0) || max_iters < 0) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi_gcr: tol >= 0 and max_iters >= 0 required");
    if (restart < 1 || restart > MGX_GCR_MAX_RESTART)
        return s->fail(MGX_ERR_INVALID, "mgx_solve_multi_gcr: 1 <= restart <= MGX_GCR_MAX_RESTART required");
    if (int rc = multi_guard(s, "mgx_solve_multi_gcr")) return rc;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return s->work_f64 ? multi_gcr_solve_t<double>(s, nrhs, b, u, tol, max_iters, restart, stats, history, history_cap)
                       : multi_gcr_solve_t<float>(s, nrhs, b, u, tol, max_iters, restart, stats, history, history_cap);
}

int mgx_time_multi_gcr_direction(mgx_handle s, int nrhs, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || repeats < 1 || nrhs < 1 || nrhs > MGX_MAX_RHS)
        return s->fail(MGX_ERR_INVALID, "mgx_time_multi_gcr_direction: 1 <= nrhs <= MGX_MAX_RHS, repeats >= 1 and ms required");
    if (int rc = multi_guard(s, "mgx_time_multi_gcr_direction")) return rc;
    bool ready = s->multi.cols >= nrhs && s->multi.gsc;
    for (int c = 0; ready && c < nrhs; ++c) ready = s->multi.gpart[c] && s->multi.Z[c][0] && s->multi.Q[c][0];
    if (!ready)
        return s->fail(MGX_ERR_STATE, "mgx_time_multi_gcr_direction: call mgx_solve_multi_gcr with at least this nrhs first (it allocates basis slot 0 "
                                      "of the columns)");
    return s->work_f64 ? multi_gcr_time_direction<double>(s, nrhs, repeats, ms) : multi_gcr_time_direction<float>(s, nrhs, repeats, ms);
}

// ---- mgx_eigs: the smallest eigenpairs of the finest operator by LOBPCG around the block cycle (mgx_eig.hpp) -------------
int mgx_eigs(mgx_handle s, int nev, void* x, double* lambda, double tol, int max_iters, mgx_stats* stats, double* history, int history_cap)
{
    if (!s) return MGX_ERR_INVALID;
    if (nev < 1 || nev > MGX_MAX_RHS) return s->fail(MGX_ERR_INVALID, "mgx_eigs: 1 <= nev <= MGX_MAX_RHS required");
    if (!x || !lambda) return s->fail(MGX_ERR_INVALID, "mgx_eigs: x and lambda must not be NULL");
    if (!(tol >= 0.0)) return s->fail(MGX_ERR_INVALID, "mgx_eigs: tol >= 0 required");
    if (max_iters < 0) return s->fail(MGX_ERR_INVALID, "mgx_eigs: max_iters >= 0 required");
    if (int rc = multi_guard(s, "mgx_eigs")) return rc;
    return s->work_f64 ? eigs_t<double>(s, nev, x, lambda, tol, max_iters, stats, history, history_cap)
                       : eigs_t<float>(s, nev, x, lambda, tol, max_iters, stats, history, history_cap);
}

// ---- mgx_eigs_many: up to MGX_EIGS_MAX pairs, blocks of mgx_eigs' iteration deflated by the pairs found (mgx_eig_many.hpp) ----
int mgx_eigs_many(mgx_handle s, int nev, void* x, double* lambda, double tol, int max_iters, mgx_stats* stats, double* history, int history_cap)
{
    if (!s) return MGX_ERR_INVALID;
    if (nev < 1 || nev > MGX_EIGS_MAX) return s->fail(MGX_ERR_INVALID, "mgx_eigs_many: 1 <= nev <= MGX_EIGS_MAX required");
    if (!x || !lambda) return s->fail(MGX_ERR_INVALID, "mgx_eigs_many: x and lambda must not be NULL");
    if (!(tol >= 0.0)) return s->fail(MGX_ERR_INVALID, "mgx_eigs_many: tol >= 0 required");
    if (max_iters < 0) return s->fail(MGX_ERR_INVALID, "mgx_eigs_many: max_iters >= 0 required");
    if (int rc = multi_guard(s, "mgx_eigs_many")) return rc;
    return s->work_f64 ? eigs_many_t<double>(s, nev, x, lambda, tol, max_iters, stats, history, history_cap)
                       : eigs_many_t<float>(s, nev, x, lambda, tol, max_iters, stats, history, history_cap);
}

int mgx_time_eig_project(mgx_handle s, int pass, int m, int k, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (pass < MGX_EIG_PROJECT_DOTS || pass > MGX_EIG_PROJECT_SUB || repeats < 1 || m < 1 || m > MGX_EIGS_MAX - 1 || k < 1 || k > MGX_MAX_RHS || !ms)
        return s->fail(MGX_ERR_INVALID, "mgx_time_eig_project: a pass of MGX_EIG_PROJECT_*, repeats >= 1, 1 <= m <= MGX_EIGS_MAX - 1, 1 <= k <= MGX_MAX_RHS "
                                        "and ms required");
    if (int rc = multi_guard(s, "mgx_time_eig_project")) return rc;
    if (s->eigm.slots < m + k || s->multi.cols < k)
        return s->fail(MGX_ERR_STATE, "mgx_time_eig_project: call mgx_eigs_many with nev >= m + k first (it allocates the locked vectors and the columns)");
    return s->work_f64 ? eig_time_project<double>(s, pass, m, k, repeats, ms) : eig_time_project<float>(s, pass, m, k, repeats, ms);
}

int mgx_time_eig_pass(mgx_handle s, int pass, int nev, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (pass < MGX_EIG_PASS_GRAM || pass > MGX_EIG_PASS_APPLY || nev < 1 || nev > MGX_MAX_RHS || repeats < 1 || !ms)
        return s->fail(MGX_ERR_INVALID, "mgx_time_eig_pass: a pass of MGX_EIG_PASS_*, 1 <= nev <= MGX_MAX_RHS, repeats >= 1 and ms required");
    if (int rc = multi_guard(s, "mgx_time_eig_pass")) return rc;
    if (s->multi.cols < nev || s->eig.cols < nev)
        return s->fail(MGX_ERR_STATE, "mgx_time_eig_pass: call mgx_eigs with at least this nev first (it allocates the columns)");
    return s->work_f64 ? eig_time_pass<double>(s, pass, nev, repeats, ms) : eig_time_pass<float>(s, pass, nev, repeats, ms);
}

// ---- mgx_solve_multi_refine_gcr: fp64 restarted GCR around the float block cycle, up to MGX_MAX_RHS right-hand sides ------
int mgx_solve_multi_refine_gcr(mgx_handle s, int nrhs, const void* b, void* u, double tol, int max_iters, int restart, mgx_stats* stats,
                               double* history, int history_cap)
{
    if (!s) return MGX_ERR_INVALID;
    if (nrhs < 1 || nrhs > MGX_MAX_RHS) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi_refine_gcr: 1 <= nrhs <= MGX_MAX_RHS required");
    if (!b || !u) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi_refine_gcr: b and u must not be NULL");
    if (!(tol >= 0.0) || max_iters < 0) return s->fail(MGX_ERR_INVALID, "mgx_solve_multi_refine_gcr: tol >= 0 and max_iters >= 0 required");
    if (restart < 1 || restart > MGX_GCR_MAX_RESTART)
        return s->fail(MGX_ERR_INVALID, "mgx_solve_multi_refine_gcr: 1 <= restart <= MGX_GCR_MAX_RESTART required");
    if (int rc = multi_refine_guard(s, "mgx_solve_multi_refine_gcr")) return rc;
    if (int rc = refine_shadow(s)) return rc;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    return multi_refine_gcr_solve(s, nrhs, b, u, tol, max_iters, restart, stats, history, history_cap);
}

int mgx_time_multi_refine_direction(mgx_handle s, int nrhs, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || repeats < 1 || nrhs < 1 || nrhs > MGX_MAX_RHS)
        return s->fail(MGX_ERR_INVALID, "mgx_time_multi_refine_direction: 1 <= nrhs <= MGX_MAX_RHS, repeats >= 1 and ms required");
    if (int rc = multi_refine_guard(s, "mgx_time_multi_refine_direction")) return rc;
    bool ready = s->shadow && s->shadow->multi.cols >= nrhs && s->multi.cols >= nrhs && s->multi.gsc;
    for (int c = 0; ready && c < nrhs; ++c) ready = s->multi.gpart[c] && s->multi.Z[c][0] && s->multi.Q[c][0];
    if (!ready)
        return s->fail(MGX_ERR_STATE, "mgx_time_multi_refine_direction: call mgx_solve_multi_refine_gcr with at least this nrhs first (it allocates "
                                      "the float columns and basis slot 0 of the columns)");
    return multi_refine_time_direction(s, nrhs, repeats, ms);
}

// ---- the zero-order term and implicit time stepping (mgx_theta_host.hpp) ---------------------------------------------
int mgx_set_reaction(mgx_handle s, const void* d, size_t count)
{
    if (!s) return MGX_ERR_INVALID;
    if (int rc = reaction_guard(s, "mgx_set_reaction")) return rc;
    return set_reaction(s, d, count);
}

int mgx_get_reaction(mgx_handle s, void* dst, size_t count)
{
    if (!s || !dst) return MGX_ERR_INVALID;
    if (int rc = reaction_guard(s, "mgx_get_reaction")) return rc;
    if (!s->rx.set) return s->fail(MGX_ERR_STATE, "mgx_get_reaction: no zero-order term is set (mgx_set_reaction)");
    return copy_out(s, s->lv[s->cfg.finest_level], s->rx.d, dst, count);
}

int mgx_theta_steps(mgx_handle s, double theta, int nsteps, const void* g, int solver, double tol, int max_iters, int restart, int* steps_done,
                    mgx_stats* stats, double* history, int history_cap)
{
    if (!s) return MGX_ERR_INVALID;
    if (steps_done) *steps_done = 0;
    if (!(theta > 0.0 && theta <= 1.0)) return s->fail(MGX_ERR_INVALID, "mgx_theta_steps: 0 < theta <= 1 required");
    if (nsteps < 0) return s->fail(MGX_ERR_INVALID, "mgx_theta_steps: nsteps >= 0 required");
    if (solver < MGX_STEP_SOLVE || solver > MGX_STEP_REFINE_GCR)
        return s->fail(MGX_ERR_INVALID, "mgx_theta_steps: solver must be MGX_STEP_SOLVE, MGX_STEP_GCR or MGX_STEP_REFINE_GCR");
    if (!(tol >= 0.0) || max_iters < 0) return s->fail(MGX_ERR_INVALID, "mgx_theta_steps: tol >= 0 and max_iters >= 0 required");
    if (solver != MGX_STEP_SOLVE && (restart < 1 || restart > MGX_GCR_MAX_RESTART))
        return s->fail(MGX_ERR_INVALID, "mgx_theta_steps: 1 <= restart <= MGX_GCR_MAX_RESTART required");
    if (int rc = reaction_guard(s, "mgx_theta_steps")) return rc;
    if (!s->rx.set) return s->fail(MGX_ERR_STATE, "mgx_theta_steps: no zero-order term is set: there is no mass term to step with (mgx_set_reaction)");
    if (solver == MGX_STEP_REFINE_GCR)
        if (int rc = refine_guard(s, "mgx_theta_steps: MGX_STEP_REFINE_GCR")) return rc;
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    return theta_steps(s, theta, nsteps, g, solver, tol, max_iters, restart, steps_done, stats, history, history_cap);
}

int mgx_time_theta_rhs(mgx_handle s, double theta, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || repeats < 1 || !(theta > 0.0 && theta <= 1.0))
        return s->fail(MGX_ERR_INVALID, "mgx_time_theta_rhs: 0 < theta <= 1, repeats >= 1 and ms required");
    if (int rc = reaction_guard(s, "mgx_time_theta_rhs")) return rc;
    if (!s->rx.set) return s->fail(MGX_ERR_STATE, "mgx_time_theta_rhs: no zero-order term is set (mgx_set_reaction)");
    Level& l = s->lv[s->cfg.finest_level];
    if (int rc = ensure_r(s, l)) return rc;
    // with a source, so that the pass reads what a step with a source reads (zeros until a mgx_theta_steps call gave one)
    if (int rc = reaction_grid(s, &s->rx.g, "mgx_time_theta_rhs", "the source term")) return rc;
    const int rc = time_on_stream(s, ms, [&] { for (int i = 0; i < repeats; ++i) theta_rhs(s, theta, l.u, s->rx.g, l.r); });
    if (rc == MGX_OK) *ms /= repeats;
    return rc;
}

// ---- Newton-multigrid for -div(a grad u) + kappa phi(u) = f (mgx_newton_host.hpp) ----------------------------------------
int mgx_newton(mgx_handle s, const mgx_newton_opts* o, const void* kappa, size_t count, mgx_newton_stats* nstats, mgx_stats* lin_stats,
               double* step_lengths, double* history, int history_cap)
{
    if (!s || !o) return MGX_ERR_INVALID;
    if (int rc = newton_opts_check(s, o, "mgx_newton")) return rc;
    if (!kappa) return s->fail(MGX_ERR_INVALID, "mgx_newton: kappa required");
    const size_t n = ((size_t)1 << s->cfg.finest_level) - 1;
    if (count != n * n) return s->fail(MGX_ERR_INVALID, "mgx_newton: vector length must be n*n with n = 2^finest_level - 1");
    if (int rc = newton_guard(s, "mgx_newton")) return rc;
    if (o->solver == MGX_STEP_REFINE_GCR)
        if (int rc = refine_guard(s, "mgx_newton: MGX_STEP_REFINE_GCR")) return rc;
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    return newton(s, *o, kappa, count, nstats, lin_stats, step_lengths, history, history_cap);
}

int mgx_time_newton_pass(mgx_handle s, int step, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || repeats < 1 || step < 0 || step > 1) return s->fail(MGX_ERR_INVALID, "mgx_time_newton_pass: step 0 or 1, repeats >= 1 and ms required");
    if (int rc = reaction_guard(s, "mgx_time_newton_pass")) return rc;
    if (!s->nwt.un) return s->fail(MGX_ERR_STATE, "mgx_time_newton_pass: call mgx_newton first (it allocates the workspace)");
    Level& l = s->lv[s->cfg.finest_level];
    if (int rc = ensure_r(s, l)) return rc;
    const int rc = time_on_stream(s, ms, [&] { for (int i = 0; i < repeats; ++i) (void)newton_pass(s, step != 0, 1.0, nullptr, l.r, nullptr); });
    if (rc == MGX_OK) *ms /= repeats;
    return rc;
}

// ---- implicit time stepping of rho u_t = div(a grad u) - kappa phi(u) + f (mgx_newton_steps_host.hpp) ------------------
int mgx_newton_steps(mgx_handle s, const mgx_newton_opts* o, double theta, int nsteps, const void* mass, const void* kappa, const void* g,
                     size_t count, int* steps_done, mgx_newton_stats* step_stats, double* history, int history_cap)
{
    if (!s || !o) return MGX_ERR_INVALID;
    if (steps_done) *steps_done = 0;
    if (int rc = newton_opts_check(s, o, "mgx_newton_steps")) return rc;
    if (!(theta > 0.0 && theta <= 1.0)) return s->fail(MGX_ERR_INVALID, "mgx_newton_steps: 0 < theta <= 1 required");
    if (nsteps < 0) return s->fail(MGX_ERR_INVALID, "mgx_newton_steps: nsteps >= 0 required");
    if (!mass) return s->fail(MGX_ERR_INVALID, "mgx_newton_steps: mass required");
    if (!kappa) return s->fail(MGX_ERR_INVALID, "mgx_newton_steps: kappa required");
    const size_t n = ((size_t)1 << s->cfg.finest_level) - 1;
    if (count != n * n) return s->fail(MGX_ERR_INVALID, "mgx_newton_steps: vector length must be n*n with n = 2^finest_level - 1");
    if (int rc = newton_guard(s, "mgx_newton_steps")) return rc;
    if (o->solver == MGX_STEP_REFINE_GCR)
        if (int rc = refine_guard(s, "mgx_newton_steps: MGX_STEP_REFINE_GCR")) return rc;
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    if (nsteps == 0) return MGX_OK;                           // nothing is touched, the workspace included
    return newton_steps(s, *o, theta, nsteps, mass, kappa, g, count, steps_done, step_stats, history, history_cap);
}

int mgx_time_newton_step_pass(mgx_handle s, int pass, double theta, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || repeats < 1 || pass < 0 || pass > 2 || !(theta > 0.0 && theta <= 1.0))
        return s->fail(MGX_ERR_INVALID, "mgx_time_newton_step_pass: pass 0, 1 or 2, 0 < theta <= 1, repeats >= 1 and ms required");
    if (int rc = reaction_guard(s, "mgx_time_newton_step_pass")) return rc;
    if (!s->nwt.dm) return s->fail(MGX_ERR_STATE, "mgx_time_newton_step_pass: call mgx_newton_steps first (it allocates the workspace)");
    Level& l = s->lv[s->cfg.finest_level];
    if (int rc = ensure_r(s, l)) return rc;
    // with a source, so that pass 0 reads what a step with a source reads (zeros until a mgx_newton_steps call gave one)
    if (int rc = reaction_grid(s, &s->nwt.g, "mgx_time_newton_step_pass", "the source term")) return rc;
    const int rc = time_on_stream(s, ms, [&] {
        for (int i = 0; i < repeats; ++i) {
            if (pass == 0) newton_step_rhs(s, theta, s->nwt.un, s->nwt.g, l.r);
            else (void)newton_pass(s, pass == 2, 1.0, s->nwt.dm, l.r, nullptr);
        }
    });
    if (rc == MGX_OK) *ms /= repeats;
    return rc;
}

// =====================================================================================
// slab-level operators on caller-owned device memory
// =====================================================================================
// ---- Picard and Newton multigrid for -div(a k(u) grad u) = f (mgx_quasi_host.hpp) --------------------------------------
int mgx_quasi(mgx_handle s, const mgx_quasi_opts* o, const double* a_nodes, size_t count, mgx_newton_stats* nstats, mgx_stats* lin_stats,
              double* step_lengths, double* history, int history_cap)
{
    if (!s || !o) return MGX_ERR_INVALID;
    if (int rc = quasi_opts_check(s, o, "mgx_quasi")) return rc;
    if (!a_nodes) return s->fail(MGX_ERR_INVALID, "mgx_quasi: a_nodes required");
    const size_t nodes = ((size_t)1 << s->cfg.finest_level) + 1;
    if (count != nodes * nodes) return s->fail(MGX_ERR_INVALID, "mgx_quasi: coefficient must hold (N + 1)^2 nodal values, N = 2^finest_level");
    if (int rc = quasi_guard(s, "mgx_quasi")) return rc;
    if (o->solver == MGX_STEP_REFINE_GCR)
        if (int rc = refine_guard(s, "mgx_quasi: MGX_STEP_REFINE_GCR")) return rc;
    return quasi(s, *o, a_nodes, nstats, lin_stats, step_lengths, history, history_cap);
}

int mgx_time_quasi_pass(mgx_handle s, int step, int method, int repeats, double* ms)
{
    if (!s) return MGX_ERR_INVALID;
    if (!ms || repeats < 1 || step < 0 || step > 1 || (method != MGX_QUASI_PICARD && method != MGX_QUASI_NEWTON))
        return s->fail(MGX_ERR_INVALID, "mgx_time_quasi_pass: step 0 or 1, method MGX_QUASI_PICARD or MGX_QUASI_NEWTON, repeats >= 1 and ms required");
    if (int rc = quasi_guard(s, "mgx_time_quasi_pass")) return rc;
    if (!s->qsi.an) return s->fail(MGX_ERR_STATE, "mgx_time_quasi_pass: call mgx_quasi first (it allocates the workspace)");
    Level& l = s->lv[s->cfg.finest_level];
    if (int rc = ensure_r(s, l)) return rc;
    const int rc = time_on_stream(s, ms, [&] { for (int i = 0; i < repeats; ++i) (void)quasi_pass(s, step != 0, method == MGX_QUASI_NEWTON, 1.0, l.r, nullptr); });
    if (rc == MGX_OK) *ms /= repeats;
    return rc;
}

static int slab_check(const mgx_slab* s)
{
    if (!s || s->level < 2 || s->level > 15 || s->rows < 1) return MGX_ERR_INVALID;
    if (s->dtype != MGX_DTYPE_F32 && s->dtype != MGX_DTYPE_F64) return MGX_ERR_INVALID;
    if (s->arith != MGX_ARITH_SEPARATE && s->arith != MGX_ARITH_FMA) return MGX_ERR_INVALID;
    // the slab must lie inside the grid: rows row0 .. row0 + rows - 1 of rows 0 .. N
    if (s->row0 < 0 || s->row0 + s->rows > (1 << s->level) + 1) return MGX_ERR_INVALID;
    return MGX_OK;
}

long mgx_slab_scratch_doubles(const mgx_slab* s)
{
    if (slab_check(s)) return -1;
    const int N = 1 << s->level;
    const int rpc = env_int("MGX_ROWS", 0);
    long cap = 0;
    for (int r : {rpc, 1}) {
        cap = std::max(cap, sumsq_blocks<double>(N, s->rows, r));
        cap = std::max(cap, sumsq_blocks<float>(N, s->rows, r));
    }
    return cap + 8;
}

// the plan request of a block on slab s (mgx_slab_jacobi / _rbgs / _cycle): knobs read per call
static BlockReq slab_req(const mgx_slab& s, int smoother, int row_lo, int row_hi, int mu, bool pre = false, int post = 0,
                         bool zero_in = false)
{
    BlockReq q{smoother, s.dtype == MGX_DTYPE_F64, 1 << s.level, s.row0, s.rows, row_lo, row_hi, mu, pre, post, zero_in};
    q.rpc = env_int("MGX_ROWS", 0);
    return q;
}

static int slab_smooth(int smoother, const mgx_slab* s, void* u, const void* b, void* tmp, int row_lo, int row_hi,
                       int mu, double omega, int shrink, int* result_in_tmp, void* stream)
{
    if (slab_check(s) || !u || !b || !tmp || mu < 0) return MGX_ERR_INVALID;
    FuseCfg fc = fuse_cfg();
    fc.arith = s->arith;
    BlockReq q = slab_req(*s, smoother, row_lo, row_hi, mu);
    q.widen = shrink != 0;
    q.strict = true;
    const long pitch = level_pitch(s->level, s->dtype);
    int flips = 0;
    const int rc = with_kernel_set(q.f64, smoother, s->arith, [&](auto k) {
        using K = decltype(k);
        using T = typename K::T;
        return fold_block<T, K::SM, K::AR>(fc, q, (T*)u, (const T*)b, (T*)tmp, pitch, omega, nullptr, nullptr, nullptr, nullptr,
                                           0, 0, 0, nullptr, (hipStream_t)stream, &flips);
    });
    if (rc < 0) return MGX_ERR_INVALID;
    if (result_in_tmp) *result_in_tmp = flips & 1;
    return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

int mgx_slab_jacobi(const mgx_slab* s, void* u, const void* b, void* tmp, int row_lo, int row_hi, int mu,
                    double omega, int shrink, int* result_in_tmp, void* stream)
{
    return slab_smooth(MGX_SMOOTHER_JACOBI, s, u, b, tmp, row_lo, row_hi, mu, omega, shrink, result_in_tmp, stream);
}

int mgx_slab_rbgs(const mgx_slab* s, void* u, const void* b, void* tmp, int row_lo, int row_hi, int mu,
                  int shrink, int* result_in_tmp, void* stream)
{
    return slab_smooth(MGX_SMOOTHER_RBGS, s, u, b, tmp, row_lo, row_hi, mu, 1.0, shrink, result_in_tmp, stream);
}

int mgx_slab_cycle(const mgx_slab* f, void* u, const void* b, void* tmp, int row_lo, int row_hi, int mu, double omega,
                   int smoother, const mgx_slab* c, const void* coarse_e, void* coarse_b, int crow_lo, int crow_hi,
                   int restrict_mode, int zero_in, double* scratch, double* sum_dev, int* result_in_tmp, void* stream)
{
    if (zero_in && coarse_e) return MGX_ERR_INVALID;
    // the slab kernels implement Jacobi / red-black GS and the two weights of full weighting (include/mgx.h)
    if (smoother != MGX_SMOOTHER_JACOBI && smoother != MGX_SMOOTHER_RBGS) return MGX_ERR_INVALID;
    if (restrict_mode != MGX_RESTRICT_CONSISTENT && restrict_mode != MGX_RESTRICT_FW16) return MGX_ERR_INVALID;
    // the folded restriction wants its range to start on an odd global row (include/mgx.h) - whichever kernel serves the call
    if (coarse_b && !((std::max(row_lo + f->row0, 1)) & 1)) return MGX_ERR_INVALID;
    if (slab_check(f) || !u || !b || !tmp || mu < 1 || mu > 64 || row_hi <= row_lo) return MGX_ERR_INVALID;
    if ((coarse_e || coarse_b) && (slab_check(c) || c->level != f->level - 1 || c->dtype != f->dtype)) return MGX_ERR_INVALID;
    if (coarse_b && sum_dev) return MGX_ERR_INVALID;
    if (sum_dev && !scratch) return MGX_ERR_INVALID;
    if (coarse_b && (crow_lo < 0 || crow_hi > c->rows || crow_hi < crow_lo)) return MGX_ERR_INVALID;
    const int N = 1 << f->level;
    if (row_lo < 0 || row_hi > f->rows || row_lo + f->row0 < 1 || row_hi + f->row0 > N) return MGX_ERR_INVALID;
    FuseCfg fc = fuse_cfg();
    fc.arith = f->arith;
    const int post = coarse_b ? 1 : (sum_dev ? 2 : 0);
    BlockReq q = slab_req(*f, smoother, row_lo, row_hi, mu, coarse_e != nullptr, post, zero_in != 0);
    q.tile_points = env_int("MGX_SLAB_TILE_POINTS", 1 << 20);      // (read per call: the parity tests switch it)
    const long pitch = level_pitch(f->level, f->dtype);
    hipStream_t st = (hipStream_t)stream;
    int flips = 0;
    const int nb = with_kernel_set(q.f64, smoother, f->arith, [&](auto k) {
        using K = decltype(k);
        using T = typename K::T;
        return fold_block<T, K::SM, K::AR>(fc, q, (T*)u, (const T*)b, (T*)tmp, pitch, omega, c, (const T*)coarse_e,
                                           (T*)coarse_b, nullptr, crow_lo, crow_hi, restrict_mode, scratch, st, &flips);
    });
    if (nb < 0) return MGX_ERR_INVALID;
    if (post == 2) hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, st, scratch, nb, sum_dev);
    if (result_in_tmp) *result_in_tmp = flips & 1;
    return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

int mgx_slab_restrict(const mgx_slab* f, const void* u, const void* b, const mgx_slab* c, void* cb, void* zero_u,
                      int crow_lo, int crow_hi, int restrict_mode, int fused, void* stream)
{
    if (slab_check(f) || slab_check(c) || !b || !cb || (fused && !u)) return MGX_ERR_INVALID;
    if (restrict_mode != MGX_RESTRICT_CONSISTENT && restrict_mode != MGX_RESTRICT_FW16) return MGX_ERR_INVALID;
    if (c->level != f->level - 1 || c->dtype != f->dtype) return MGX_ERR_INVALID;
    const int N = 1 << f->level;
    const long pitch = level_pitch(f->level, f->dtype), cpitch = level_pitch(c->level, c->dtype);
    const int off = 2 * c->row0 - f->row0;
    // coarse rows must be unknown rows; fine rows 2I+off-2 .. 2I+off+2 must exist (fused), +-1 otherwise
    const int halo = fused ? 2 : 1;
    if (crow_lo < 0 || crow_hi > c->rows || crow_lo + c->row0 < 1 || crow_hi + c->row0 > N / 2) return MGX_ERR_INVALID;
    if (crow_hi > crow_lo && (2 * crow_lo + off - halo < 0 || 2 * (crow_hi - 1) + off + halo > f->rows - 1)) return MGX_ERR_INVALID;
    const int rpc = env_int("MGX_ROWS", 0);
    if (f->dtype == MGX_DTYPE_F64)
        launch_restrict<double>((const double*)u, (const double*)b, (double*)cb, (double*)zero_u, N, pitch, cpitch,
                                crow_lo, crow_hi, off, restrict_mode, fused != 0, rpc, (hipStream_t)stream);
    else
        launch_restrict<float>((const float*)u, (const float*)b, (float*)cb, (float*)zero_u, N, pitch, cpitch,
                               crow_lo, crow_hi, off, restrict_mode, fused != 0, rpc, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

int mgx_slab_prolong(const mgx_slab* f, void* u, const mgx_slab* c, const void* e, int row_lo, int row_hi, int add,
                     void* stream)
{
    if (slab_check(f) || slab_check(c) || !u || !e) return MGX_ERR_INVALID;
    if (c->level != f->level - 1 || c->dtype != f->dtype) return MGX_ERR_INVALID;
    const int N = 1 << f->level;
    const long pitch = level_pitch(f->level, f->dtype), cpitch = level_pitch(c->level, c->dtype);
    const int off = 2 * c->row0 - f->row0;
    if (row_lo < 0 || row_hi > f->rows || row_lo + f->row0 < 1 || row_hi + f->row0 > N) return MGX_ERR_INVALID;
    if (row_hi > row_lo) {
        const int ylo = row_lo - off, yhi = row_hi - 1 - off;
        if (ylo < 0 || (yhi >> 1) + (yhi & 1) > c->rows - 1) return MGX_ERR_INVALID;
    }
    const int rpc = env_int("MGX_ROWS", 0);
    if (f->dtype == MGX_DTYPE_F64)
        launch_prolong<double>((double*)u, (const double*)e, N, pitch, cpitch, row_lo, row_hi, off, add != 0, rpc, (hipStream_t)stream);
    else
        launch_prolong<float>((float*)u, (const float*)e, N, pitch, cpitch, row_lo, row_hi, off, add != 0, rpc, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

int mgx_slab_residual_sumsq(const mgx_slab* s, const void* u, const void* b, int row_lo, int row_hi,
                            double* scratch, double* sum_dev, void* stream)
{
    if (slab_check(s) || !u || !b || !scratch || !sum_dev) return MGX_ERR_INVALID;
    const int N = 1 << s->level;
    const long pitch = level_pitch(s->level, s->dtype);
    if (row_lo < 1 || row_hi > s->rows - 1 || row_lo + s->row0 < 1 || row_hi + s->row0 > N || row_hi <= row_lo) return MGX_ERR_INVALID;
    const int rpc = env_int("MGX_ROWS", 0);
    if (s->dtype == MGX_DTYPE_F64)
        launch_residual<double, 1>((const double*)u, (const double*)b, nullptr, 0, scratch, sum_dev, 1.0, N, pitch, row_lo, row_hi, rpc, (hipStream_t)stream, -1, s->rows);
    else
        launch_residual<float, 1>((const float*)u, (const float*)b, nullptr, 0, scratch, sum_dev, 1.0, N, pitch, row_lo, row_hi, rpc, (hipStream_t)stream, -1, s->rows);
    return hipGetLastError() == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

// ---- multi-GPU: ranks, plans, helpers ----------------------------------------------------------------
int mgx_create_rank(const mgx_config* cfg, int rank, int world, const void* rccl_id, const mgx_transport* transport,
                    mgx_handle* out)
{
    if (!cfg || !out) { g_create_error = "null argument"; return MGX_ERR_INVALID; }
    *out = nullptr;
    if (cfg->smoother == MGX_SMOOTHER_CHEBYSHEV) {
        g_create_error = "MGX_SMOOTHER_CHEBYSHEV: single-GPU handles of op = MGX_OPERATOR_STENCIL5 / MGX_OPERATOR_GALERKIN only";
        return MGX_ERR_INVALID;
    }
    if (cfg->smoother == MGX_SMOOTHER_COLOR_GS || cfg->smoother == MGX_SMOOTHER_COLOR_SGS) {
        g_create_error = "MGX_SMOOTHER_COLOR_GS / COLOR_SGS: single-GPU handles of op = MGX_OPERATOR_STENCIL5 / MGX_OPERATOR_GALERKIN only";
        return MGX_ERR_INVALID;
    }
    if (cfg->smoother >= MGX_SMOOTHER_LINE_X && cfg->smoother <= MGX_SMOOTHER_LINE_ALT) {
        g_create_error = "MGX_SMOOTHER_LINE_X / LINE_Y / LINE_ALT: single-GPU handles of op = MGX_OPERATOR_STENCIL5 / MGX_OPERATOR_GALERKIN only";
        return MGX_ERR_INVALID;
    }
    if (cfg->coarsest_level < 2 || cfg->finest_level < cfg->coarsest_level || cfg->finest_level > 15 ||
        cfg->mu1 < 0 || cfg->mu2 < 0 || !(cfg->omega > 0.0 && cfg->omega < 2.0) || cfg->smoother < 0 || cfg->smoother > 1 ||
        cfg->dtype < 0 || cfg->dtype > 2 || cfg->restrict_mode < 0 || cfg->restrict_mode > 1 || cfg->bottom < 0 || cfg->bottom > 1 || cfg->arith < 0 || cfg->arith > 1 ||
        (rank >= 0 && (world < 1 || rank >= world)) || (rank < 0 && cfg->n_gpus < 2)) {
        g_create_error = "invalid configuration";
        return MGX_ERR_INVALID;
    }
    // the slab plan runs the constant stencil only: a general operator must not silently become Poisson
    if (cfg->op != MGX_OPERATOR_POISSON) {
        g_create_error = "multi-GPU handles: op = MGX_OPERATOR_POISSON only (MGX_OPERATOR_STENCIL5 / MGX_OPERATOR_GALERKIN: one GPU)";
        return MGX_ERR_INVALID;
    }
    log_runtime_libs("mgx_create_rank");
    mgx_solver* s = new (std::nothrow) mgx_solver();
    if (!s) { g_create_error = "out of host memory"; return MGX_ERR_ALLOC; }
    s->cfg = *cfg;
    const int rc = dist_create(s, &s->cfg, rank, world, rccl_id, transport);
    if (rc != MGX_OK) { g_create_error = s->err; mgx_destroy(s); return rc; }
    *out = s;
    return MGX_OK;
}

// Which ROCm runtime libraries this process has mapped (/proc/self/maps): libmgx is built against /opt/rocm
// (RUNPATH), and a host application that loaded another copy of libamdhip64 / libhsa-runtime64 / librccl
// first (the torch wheel bundles its own, with the same SONAMEs) would run this library's code objects on
// THAT stack.  One path per line; returns the number of bytes written (without the terminator), < 0 on error.
int mgx_runtime_libs(char* buf, size_t cap)
{
    if (!buf || cap == 0) return -1;
    buf[0] = 0;
    FILE* fh = std::fopen("/proc/self/maps", "r");
    if (!fh) return -1;
    std::vector<std::string> seen;
    char line[4096];
    while (std::fgets(line, sizeof line, fh)) {
        const char* path = std::strchr(line, '/');
        if (!path) continue;
        std::string p(path);
        while (!p.empty() && (p.back() == '\n' || p.back() == ' ')) p.pop_back();
        const char* names[] = {"libamdhip64", "libhsa-runtime64", "librccl", "libmgx", "libhiprtc", "libamd_comgr"};
        bool want = false;
        for (const char* n : names) want = want || p.find(n) != std::string::npos;
        if (!want || std::find(seen.begin(), seen.end(), p) != seen.end()) continue;
        seen.push_back(p);
    }
    std::fclose(fh);
    std::string out;
    for (const auto& p : seen) { out += p; out += '\n'; }
    if (out.size() + 1 > cap) out.resize(cap - 1);
    std::memcpy(buf, out.c_str(), out.size() + 1);
    return (int)out.size();
}

int mgx_rccl_unique_id(void* out128)
{
    if (!out128) return MGX_ERR_INVALID;
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return MGX_ERR_HIP;
    std::memset(out128, 0, 128);
    std::memcpy(out128, &id, sizeof(id) < 128 ? sizeof(id) : 128);
    return MGX_OK;
}

#ifdef MGX_WAVE_TRACE
// debug build only: the wave trace of the last k_jacobi_cycle launch; returns the number of waves
__attribute__((visibility("default"))) int mgx_debug_wave_trace(void* out, int cap)
{
    int n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(mgx::g_wave_trace_n), sizeof(int)) != hipSuccess) return -1;
    n = std::min(std::min(n, cap), 1 << 16);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mgx::g_wave_trace), (size_t)n * sizeof(mgx::WaveTrace)) != hipSuccess) return -1;
    return n;
}
// debug build only: the phase records of k_dst_pair / k_tile_wide (mgx_phase_trace.hpp), oldest first; returns their number
__attribute__((visibility("default"))) int mgx_debug_phase_trace(void* out, int cap)
{
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(mgx::g_phase_trace_n), sizeof(n)) != hipSuccess) return -1;
    std::vector<mgx::PhaseTrace> ring(mgx::kPhaseCap);
    if (hipMemcpyFromSymbol(ring.data(), HIP_SYMBOL(mgx::g_phase_trace), ring.size() * sizeof(mgx::PhaseTrace)) != hipSuccess) return -1;
    const unsigned have = std::min<unsigned>(n, mgx::kPhaseCap), take = std::min<unsigned>(have, (unsigned)std::max(cap, 0));
    for (unsigned q = 0; q < take; ++q)
        static_cast<mgx::PhaseTrace*>(out)[q] = ring[(n - take + q) & (mgx::kPhaseCap - 1)];
    return (int)take;
}
#endif

long mgx_dist_exchanges(mgx_handle s) { return (s && s->dist) ? s->dist->exchanges : -1; }
long mgx_dist_overlapped(mgx_handle s) { return (s && s->dist) ? s->dist->overlapped : -1; }

int mgx_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream)
{
    if (hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return MGX_ERR_HIP;
    return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

int mgx_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream)
{
    if (hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) return MGX_ERR_HIP;
    return hipStreamSynchronize((hipStream_t)stream) == hipSuccess ? MGX_OK : MGX_ERR_HIP;
}

struct mgx_dist_planner { mgx::DistPlanner p; };

int mgx_plan_create(const mgx_config* cfg, int n_slabs, int g, int fold, int deep, mgx_plan_handle* out)
{
    if (!cfg || !out) { g_plan_error = "null argument"; return MGX_ERR_INVALID; }
    *out = nullptr;
    if (cfg->smoother == MGX_SMOOTHER_CHEBYSHEV) {
        g_plan_error = "MGX_SMOOTHER_CHEBYSHEV: the slab plan runs the constant stencil (Jacobi or red-black GS) only";
        return MGX_ERR_INVALID;
    }
    if (cfg->smoother == MGX_SMOOTHER_COLOR_GS || cfg->smoother == MGX_SMOOTHER_COLOR_SGS) {
        g_plan_error = "MGX_SMOOTHER_COLOR_GS / COLOR_SGS: the slab plan runs the constant stencil (Jacobi or red-black GS) only";
        return MGX_ERR_INVALID;
    }
    if (cfg->smoother >= MGX_SMOOTHER_LINE_X && cfg->smoother <= MGX_SMOOTHER_LINE_ALT) {
        g_plan_error = "MGX_SMOOTHER_LINE_X / LINE_Y / LINE_ALT: the slab plan runs the constant stencil (Jacobi or red-black GS) only";
        return MGX_ERR_INVALID;
    }
    const int cut = dist_cut_level(*cfg, n_slabs);
    mgx_dist_planner* h = new (std::nothrow) mgx_dist_planner();
    if (!h) return MGX_ERR_ALLOC;
    if (h->p.init(plan_cfg_of(*cfg, n_slabs, g, cut, fold != 0, deep != 0)) != MGX_OK) {
        g_plan_error = h->p.err;
        delete h;
        return MGX_ERR_INVALID;
    }
    *out = h;
    return MGX_OK;
}

int mgx_plan_destroy(mgx_plan_handle p) { delete p; return MGX_OK; }
const char* mgx_plan_last_error(void) { return g_plan_error.c_str(); }
int mgx_plan_cut_level(mgx_plan_handle p) { return p ? p->p.c.cut : -1; }

int mgx_plan_level(mgx_plan_handle p, int level, mgx_dist_level* out)
{
    if (!p || !out || level <= p->p.c.cut || level > p->p.c.finest) return MGX_ERR_INVALID;
    *out = p->p.L(level);
    return MGX_OK;
}

int mgx_plan_cut_share(mgx_plan_handle p, int* row0, int* rows)
{
    if (!p || !row0 || !rows) return MGX_ERR_INVALID;
    *row0 = p->p.c_row0; *rows = p->p.c_rows;
    return MGX_OK;
}

int mgx_plan_guess_set(mgx_plan_handle p, int all_rows)
{
    if (!p) return MGX_ERR_INVALID;
    if (all_rows) p->p.guess_set(); else p->p.guess_changed();
    return MGX_OK;
}

static int plan_emit(mgx_plan_handle p, mgx_dist_op* ops, int cap, bool norm)
{
    if (!p || (!ops && cap > 0)) return MGX_ERR_INVALID;
    std::vector<mgx_dist_op> v;
    // emit on a copy first: a too-small buffer must not advance the planner's halo state
    mgx::DistPlanner trial = p->p;
    if (norm) trial.emit_norm(v); else trial.emit_vcycle(v);
    if ((int)v.size() > cap) return -(int)v.size();
    p->p = trial;
    for (size_t i = 0; i < v.size(); ++i) ops[i] = v[i];
    return (int)v.size();
}
int mgx_plan_vcycle(mgx_plan_handle p, mgx_dist_op* ops, int cap) { return plan_emit(p, ops, cap, false); }
int mgx_plan_norm(mgx_plan_handle p, mgx_dist_op* ops, int cap) { return plan_emit(p, ops, cap, true); }
int mgx_plan_fmg(mgx_plan_handle p, mgx_dist_op* ops, int cap)
{
    if (!p || (!ops && cap > 0)) return MGX_ERR_INVALID;
    std::vector<mgx_dist_op> v;
    mgx::DistPlanner trial = p->p;
    trial.emit_fmg(v);
    if ((int)v.size() > cap) return -(int)v.size();
    p->p = trial;
    for (size_t i = 0; i < v.size(); ++i) ops[i] = v[i];
    return (int)v.size();
}

} // extern "C"
