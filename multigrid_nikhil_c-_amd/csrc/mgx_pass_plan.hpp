// mgx_pass_plan.hpp - the pass planner: how a block of mu smoother sweeps is split into launches (single sweeps, fused
// passes, passes with the cycle's transfers folded in, register tiles), the chunk height each launch gets and the tuning
// knobs behind both.  Plain C++ without HIP: the executor (fold_block, mgx.hip) runs what fold_plan returns, and
// tests/pass_plan_check.cpp compiles this header on the CPU.
#pragma once

#include "../../include/mgx.h"
#include "mgx_geom.hpp"

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace mgx {

inline int env_int(const char* name, int dflt)
{
    const char* s = getenv(name);
    return (s && *s) ? atoi(s) : dflt;
}

// temporal fusion knobs: levels per pass, chunk height (0 = by grid size), smallest
// fused grid, levels per pass for the folded kernels
struct FuseCfg {
    int kmax; int rows; int min_n; int fold_kmax; int fold_kmax_big; int tile_max_n; int tile_k; int fold_kmax_nopost;
    int tile_wide; int tile_short_n;    // register tiles: k_tile_wide for fp64 (1) / all levels (2), else k_tile_smooth; 8-row bands up to tile_short_n
    // explicit pass plans (sweeps per pass) for the pre- / post-smoothing block of grids with
    // N >= plan_min_n: tuning knobs MGX_PLAN_PRE / MGX_PLAN_POST ("8,2"), MGX_PLAN_MIN_N.  They apply to the
    // folded blocks of whole levels and of slabs alike (fold_plan)
    int plan_pre[8] = {0}; int n_pre = 0; int plan_post[8] = {0}; int n_post = 0; int plan_min_n = 8192;
    // mgx_config.arith (MGX_ARITH_*): not a tuning knob - it selects which of the two arithmetic modes of the
    // Jacobi update every smoother kernel uses (jac_pt in mgx_kernels.hpp); set by the handle / the slab, never from the environment
    int arith = 0;
};

// chunk height of a fused pass: a chunk recomputes 2K halo rows, so the deeper the pass the
// taller the chunk, against the parallelism short chunks give (all measured, bench.py sweeps
// of MGX_FUSE_ROWS): K <= 2: 8 rows (flat from 8 to 24); K = 3, 4: 16-24 rows (8192^2 RB-GS
// V(2,2) 1.52 -> 1.32 ms, Jacobi V(4,3) 1.45 -> 1.27 ms against 8 rows; 4-7 % at 4096^2 and
// 2048^2); K >= 5: N/128 clamped to [8, 64] in double (flat between 48 and 96 at 8192^2), to
// [8, 32] in float (a float wave covers twice the columns, so a grid has half the strips:
// 8192^2 fp32 V(10,10) finest level 0.96 -> 0.90 ms at 32 rows)
// deep double passes (K >= 8: two workgroups of four waves per CU = 2048 waves per round): whole
// rounds.  One wave per (chunk, strip of 52-54 vectors): with cpr = 2048 / strips chunk rows per round,
// `rows` rows in m rounds take R = rows / (m cpr); m = the fewest rounds with R <= 200.  Measured (one
// pass, us): 4096^2 whole 183 at 36 rows, 154 at 84 (m = 1, 490 workgroups), 167-190 at 48-72 and
// 90-108; 16384^2 whole 1947 at 72, 1807 at 200; 8192^2 whole 487-498 at 72 and 484-492 at 168 (flat; on
// a box that clocks down under the f64 load, 540 against 492).  Fewer, taller chunks also recompute
// fewer halo rows (2K + 3 per chunk).
inline int fuse_rows_deep(int N, int rows)
{
    const int strips = (N / 2 + 51) / 52;
    const int cpr = std::max(1, 2048 / strips);
    for (int m = 1; m <= 64; ++m) {
        const int R = (rows + m * cpr - 1) / (m * cpr);
        if (R <= 200) return std::max(R, 16);
    }
    return 64;
}

// deep double passes on big grids, height not given by MGX_FUSE_ROWS: launch_cycle_k sizes the chunks itself
// (edge tiles shorter than interior ones) - it is handed -fuse_rows(...)
// (float: the 10-level passes, whose rhs window is in LDS like the deep double ones - until round 3 they ran 32-row
// chunks, 52 row steps for 32 rows)
inline bool fuse_rows_auto(const FuseCfg& fc, int N, int K, bool f64)
{
    return fc.rows <= 0 && K >= (f64 ? 8 : 10) && N >= 2048;
}

inline int shallow_big_n() { static const int n = env_int("MGX_SHALLOW_BIG_N", 8192); return n; }
// (4096^2: 48 rows - config 2's V(2,1) cycle 0.416-0.418 -> 0.389-0.395 ms, the 4096^2 level of config 3 -4 %; 96 there: 0.402)
inline int shallow_mid_rows() { static const int r = env_int("MGX_SHALLOW_ROWS_MID", 48); return r; }

inline int fuse_rows(const FuseCfg& fc, int N, int K, bool f64 = true, int rows = 0)
{
    if (fc.rows > 0) return fc.rows;
    if (K <= 2) {
        // (8192^2 and up: 96 rows like the K <= 4 passes below - together −2..−3.5 % on the finest-level part of a V(2,1) cycle)
        static const int big2 = env_int("MGX_SHALLOW2_ROWS_BIG", 96);
        return N >= shallow_big_n() ? big2 : (N >= 4096 ? shallow_mid_rows() : 8);
    }
    if (K <= 4) {
        // (8192^2 and up: 96 rows - finest-level part of the red-black V(2,1) cycle 0.828-0.833 -> 0.789 ms, Jacobi V(2,1)
        // 0.811-0.817 -> 0.786-0.794; round 1's 24 rows paid (24 + 2K) / 24 in recomputed rows)
        static const int big = env_int("MGX_SHALLOW_ROWS_BIG", 96);
        return N >= shallow_big_n() ? big : (N >= 4096 ? shallow_mid_rows() : 16);
    }
    if (f64 && K >= 8 && N >= 2048) return fuse_rows_deep(N, rows > 0 ? rows : N - 1);
    int R = N / 128;
    if (R < 8) R = 8;
    if (R > (f64 ? 64 : 32)) R = f64 ? 64 : 32;
    return R;
}

inline FuseCfg fuse_cfg()
{
    FuseCfg f;
    f.kmax = env_int("MGX_FUSE", 10);          // levels per pass; 1 disables temporal fusion
    if (f.kmax < 1) f.kmax = 1;
    if (f.kmax > 10) f.kmax = 10;
    f.rows = env_int("MGX_FUSE_ROWS", 0);      // 0: chosen from the grid size
    if (f.rows < 0) f.rows = 0;
    // smallest grid (N = 2^L) on which fused / folded passes replace single sweeps
    f.min_n = std::max(64, env_int("MGX_FUSE_MIN_N", 256));
    // Levels per pass for the folded kernels.  They carry one more level window and the
    // transfer state, so their sweet spot is shallower than the plain fused kernel's and
    // flat: measured in one process on one MI355X, V(10,10) at 8192^2 fp64 takes 2.63 ms as
    // [5,5] and 2.62 as [10] (244-256 VGPRs, 2 waves/SIMD); [5,5] is better on smaller grids.
    f.fold_kmax = std::max(1, std::min(f.kmax, env_int("MGX_FOLD_KMAX", 10)));
    // The same for grids with N >= 8192 (separate knob): there the deep variant [10] is
    // device-dependent - 1.55 vs 1.62 ms for the finest level on one MI355X, 1.87 vs 1.50 ms on
    // another (VALU-bound passes follow the clock the chip holds; the HBM-bound [5,5] does not).
    f.fold_kmax_big = std::max(1, std::min(f.kmax, env_int("MGX_FOLD_KMAX_BIG", 10)));
    // Whole levels up to this N (= 2^L) are smoothed by the LDS tile kernel, all sweeps of a
    // block (up to tile_k levels) per launch; 0 disables it.  MGX_TILE_WIDE selects the kernel: k_tile_wide for fp64
    // levels (1, the default), for fp32 levels too (2), or k_tile_smooth everywhere (0).  In fp32 k_tile_wide measured
    // slower (bench --dtype f32: 0.918 against 0.902-0.910 ms), so fp32 levels keep k_tile_smooth by default.  At 2048^2 the tiles lose to the marching passes (k_tile_wide 64 + 64 us per V(10,10)
    // against 47 + 44: 580 workgroups of one per CU are three rounds), so the default stays 1024.  MGX_TILE_SHORT_N:
    // levels up to this N run k_tile_wide with 8-row bands (tile_wide_rw, mgx_geom.hpp).
    f.tile_wide = std::max(0, std::min(2, env_int("MGX_TILE_WIDE", 1)));
    f.tile_short_n = env_int("MGX_TILE_SHORT_N", 512);
    f.tile_max_n = std::max(0, env_int("MGX_TILE_MAX_N", 1024));
    f.tile_k = std::max(2, std::min(10, env_int("MGX_TILE_K", 10)));
    // levels per folded pass for blocks that end WITHOUT a residual stage (post-smoothing below
    // the finest level): those passes keep c1 * b in their window and are cheaper per level
    f.fold_kmax_nopost = std::max(1, std::min(f.kmax, env_int("MGX_FOLD_KMAX_NOPOST", 10)));
    auto parse = [](const char* name, int* out) {
        const char* v = std::getenv(name);
        int n = 0;
        while (v && *v && n < 8) {
            char* end = nullptr;
            const long k = std::strtol(v, &end, 10);
            if (end == v || k < 1 || k > 10) return 0;
            out[n++] = (int)k;
            v = (*end == ',') ? end + 1 : end;
            if (*end && *end != ',') return 0;
        }
        return n;
    };
    f.n_pre = parse("MGX_PLAN_PRE", f.plan_pre);
    f.n_post = parse("MGX_PLAN_POST", f.plan_post);
    f.plan_min_n = env_int("MGX_PLAN_MIN_N", 8192);
    return f;
}

// levels per pass the folded kernels (k_jacobi_cycle) are instantiated for
inline bool cycle_k_supported(int K, bool rbgs, bool f64, int post, bool pre, int arith)
{
    if (K == 10) return !(pre && post == 1) && !(rbgs && post == 1) && !(!f64 && pre && post == 2) && !(!f64 && post == 1 && arith == 0);
    if (K == 8 && !f64 && !pre && post != 0) return false;
    return rbgs ? (K == 2 || K == 4 || K == 6 || K == 8) : (K >= 1 && K <= 8 && K != 7);
}

// levels per pass the plain fused kernel (k_jacobi_fused) is instantiated for
inline bool fused_k_supported(int K, bool rbgs)
{
    return K == 2 || K == 4 || K == 6 || K == 8 || K == 10 || (!rbgs && (K == 3 || K == 5));
}

// band height of k_tile_wide for a level of N (= 2^L), 0: k_tile_smooth
inline int tile_band(const FuseCfg& fc, int N, bool f64)
{
    return (fc.tile_wide >= (f64 ? 1 : 2)) ? tile_wide_rw(N, fc.tile_short_n) : 0;
}

// ---- cost model of blocks without a folded stage --------------------------------------------------
// Per-sweep throughput of a fused launch relative to one stand-alone sweep,
// measured on MI355X at 8192^2 (tools/microbench, profiles/r01_fused_microbench.md).
// Index = sweeps per launch; 0 = not instantiated.  Jacobi: K = 5 is poor in
// float because it needs a second halo lane per side for one extra column.
// Re-measured after the fused Jacobi passes started keeping c1 * b in their rhs window
// (K - 1 fewer multiplications per point: fp64 K=8 1138 -> 1349 G upd/s, fp32 K=6 1457 -> 1852,
// fp32 K=10 1371 -> 2019).
constexpr double kFuseRate64[11] = {0, 1.00, 1.80, 2.45, 3.16, 3.81, 4.80, 0, 5.60, 0, 5.63};
// float again after the row operators were written on pairs (all arithmetic packed:
// v_pk_add_f32 / v_pk_mul_f32): K=5 1508 -> 1743, K=8 1731 -> 2301 G upd/s.
constexpr double kFuseRate32[11] = {0, 1.00, 1.67, 2.38, 3.10, 3.77, 4.26, 0, 4.98, 0, 4.67};
// red-black Gauss-Seidel: s sweeps = 2 s levels, s <= 5
constexpr double kFuseRateGS64[11] = {0, 1.00, 1.81, 2.50, 3.19, 3.12, 0, 0, 0, 0, 0};
constexpr double kFuseRateGS32[11] = {0, 1.00, 1.79, 2.20, 2.87, 2.69, 0, 0, 0, 0, 0};

// ---- cost model of blocks with a folded stage ----------------------------------------------------
// Pass costs relative to a pass of up to 5 levels (HBM-bound: ~385 us at 8192^2 in double whatever
// its depth), from bench.py runs with explicit plans (MGX_PLAN_PRE / MGX_PLAN_POST) against each other
// inside one GPU call.  Round 2, double, after the deep passes got their rhs window in LDS and
// branch-free interior bodies (rows really in flight): 6 levels 1.05, 8 levels 1.12, 10 levels 1.46
// (0.56 ms) - a 10-level pass now costs less than two 5-level ones, so V(10,10) is planned as ONE
// pass per block ([10]: 1.93 ms per cycle against 2.35 as [5,5], 2.28 as [8,2], 2.35 as [6,4]).
// float (no LDS variants, packed arithmetic): 6: 1.34, 8: 1.53; red-black Gauss-Seidel (levels =
// 2 x sweeps) 6: 1.1, 8: 1.3, 10: 2.4.  MGX_FOLD_KMAX / _BIG / _NOPOST / _GS still cap the depth.
inline double fold_pass_cost(int K, bool rbgs, int post, bool f64, int arith)
{
    if (!cycle_k_supported(K, rbgs, f64, post, false, arith)) return -1.0;
    if (rbgs) return K <= 4 ? 1.0 : (K == 6 ? 1.1 : (K == 8 ? 1.3 : 2.4));
    if (K <= 5) return 1.0;
    if (!f64) return K == 6 ? 1.34 : (K == 8 ? 1.53 : 1.75);      // (10 levels: rhs window in LDS since round 3)
    if (K == 6) return 1.05;
    if (K == 8) return 1.12;
    return 1.46;
}

// sweeps per pass of mu sweeps minimising sum(cost(k, m) + launch) over passes of at most smax sweeps (cost < 0: no such
// pass; a split must be cheaper by more than eps to replace another), in the order the DP picks them
template <typename Cost>
std::vector<int> split_sweeps(int mu, int smax, double launch, double eps, Cost cost)
{
    std::vector<double> best(mu + 1, 1e300);
    std::vector<int> pick(mu + 1, 1);
    best[0] = 0.0;
    for (int m = 1; m <= mu; ++m)
        for (int k = 1; k <= std::min(m, smax); ++k) {
            const double c = cost(k, m);
            if (c < 0.0) continue;
            const double t = best[m - k] + c + launch;
            if (t < best[m] - eps) { best[m] = t; pick[m] = k; }
        }
    std::vector<int> parts;
    for (int m = mu; m > 0; m -= pick[m]) parts.push_back(pick[m]);
    return parts;
}

// ---- the plan of a smoothing block -------------------------------------------------------------
enum PassKind {
    PASS_JACOBI,    // one Jacobi sweep (launch_jacobi: k_jacobi_rows, or k_jacobi with R rows per chunk)
    PASS_RBGS,      // one red-black sweep (k_rbgs)
    PASS_FUSED,     // K levels, no folded stage (k_jacobi_fused)
    PASS_FOLDED,    // K levels with the correction (pre) and / or the residual stage (post) folded in (k_jacobi_cycle)
    PASS_TILE,      // K levels on register tiles (k_tile_wide with bands of R rows, k_tile_smooth when R = 0)
};

struct Pass {
    int kind;
    int K;              // levels (sweeps, twice that for red-black Gauss-Seidel)
    bool pre; int post; // folded stages, as in BlockReq
    bool zero_in;       // the pass takes its input iterate as all zero and does not read it
    int lo, hi;         // GLOBAL rows [lo, hi) it updates; hi <= lo: nothing is launched, the buffers still swap
    int R;              // chunk height handed to the launcher: rows per chunk of a single sweep (0: one wave per row),
                        // fuse_rows for fused / folded passes (negative: the folded launcher sizes the chunks itself),
                        // the band height for tiles
};

struct BlockReq {
    int smoother = MGX_SMOOTHER_JACOBI; bool f64 = true;
    int N = 0, row0 = 0, rows = 0;     // grid of N (= 2^L) and the window of rows row0 .. row0 + rows - 1 the arrays hold
    int row_lo = 0, row_hi = 0;        // rows to smooth, LOCAL numbers (row 0 = row0)
    int mu = 0;
    bool pre = false;                  // the first pass adds the prolonged correction while loading
    int post = 0;                      // the last pass restricts the residual (1) or sums its squares (2)
    bool zero_in = false;              // the input iterate is all zero: the first pass must not read it
    bool widen = true;                 // each pass widens its range by the rows the later passes still consume
    bool strict = false;               // a pass that would read rows outside the window is refused (not clipped)
    long tile_points = 0;              // register tiles for ranges of at most this many rows x N points (0: never)
    int rpc = 0;                       // rows per chunk of single sweeps (0: one wave per row)
};

// The passes of a block of q.mu sweeps, or false when the kernels cannot run it as asked (before anything is launched):
//  - register tiles for ranges of at most tile_points points: up to tile_k levels per launch in equal parts, all on the
//    same range (so a block deeper than one launch only on a range that needs no rows beyond it, a whole grid);
//  - no folded stage: the DP over the fused rates (+ 0.02 per launch) when fusion pays (kmax > levels per sweep,
//    N >= min_n, at least 64 rows, mu <= 64), otherwise single sweeps;
//  - a stage: an explicit plan (MGX_PLAN_PRE / _POST) when it fits, otherwise the DP over fold_pass_cost, deepest pass
//    first (the last pass carries the residual stage, which gets expensive with depth; a leading single sweep could not
//    synthesise a zero input).
// A pass covers [row_lo, row_hi) widened (q.widen) by the rows the later passes still consume, and the one / two rows a
// residual stage recomputes beyond its range; never beyond the unknown rows nor the window's first or last row.
inline bool fold_plan(const FuseCfg& fc, const BlockReq& q, std::vector<Pass>* plan)
{
    plan->clear();
    const bool rbgs = (q.smoother == MGX_SMOOTHER_RBGS);
    const int per = rbgs ? 2 : 1, N = q.N, mu = q.mu;
    const int first = 1 - q.row0, last = N - q.row0;          // local unknown rows [first, last)
    {
        const int lo = std::max(std::max(q.row_lo, first), 1), hi = std::min(std::min(q.row_hi, last), q.rows - 1);
        const bool whole = q.row_lo <= first && q.row_hi >= last;
        if (fc.tile_max_n > 0 && hi > lo && (long)(hi - lo) * N <= q.tile_points && (per * mu <= fc.tile_k || whole)) {
            // halo of at most tile_k + 2 <= 12 rows: every tile geometry keeps its output tile (mgx_kernels.hpp, mgx_geom.hpp)
            const int smax = std::max(1, fc.tile_k / per), np = (mu + smax - 1) / smax;
            for (int p = 0; p < np; ++p) {
                const int sw = mu / np + (p < mu % np ? 1 : 0);
                plan->push_back({PASS_TILE, per * sw, q.pre && p == 0, p == np - 1 ? q.post : 0, q.zero_in && p == 0,
                                 lo + q.row0, hi + q.row0, tile_band(fc, N, q.f64)});
            }
            return true;
        }
    }
    const bool staged = q.pre || q.post != 0;
    const bool fuse = fc.kmax > per && N >= fc.min_n && (q.row_hi - q.row_lo) >= 64 && mu <= 64;
    std::vector<int> parts;
    if (!staged) {
        const double* rate = rbgs ? (q.f64 ? kFuseRateGS64 : kFuseRateGS32) : (q.f64 ? kFuseRate64 : kFuseRate32);
        if (fuse)
            parts = split_sweeps(mu, std::max(1, std::min(fc.kmax, 10) / per), 0.02, 0.0,
                                 [&](int k, int) { return rate[k] > 0.0 ? (double)k / rate[k] : -1.0; });
        else
            parts.assign(std::max(mu, 0), 1);
    } else {
        const int* forced = nullptr;
        int nf = 0;
        if (!q.pre && q.post == 1) { forced = fc.plan_pre; nf = fc.n_pre; }
        else if (q.pre) { forced = fc.plan_post; nf = fc.n_post; }
        if (nf > 0 && N >= fc.plan_min_n) {
            int sum = 0;
            bool ok = true;
            for (int i = 0; i < nf; ++i) {
                sum += forced[i];
                const int K = per * forced[i];
                const bool folded = (i == 0 && q.pre) || (i == nf - 1 && q.post != 0);
                const int Q = (i == nf - 1) ? q.post : 0;
                ok = ok && K <= 10 && (folded ? cycle_k_supported(K, rbgs, q.f64, Q, q.pre && i == 0, fc.arith) : (K != 7 && K != 9 && (!rbgs || K % 2 == 0)));
            }
            if (ok && sum == mu) parts.assign(forced, forced + nf);
        }
        if (parts.empty()) {
            int kcap = N >= 8192 ? fc.fold_kmax_big : fc.fold_kmax;
            if (q.post == 0) kcap = std::min(kcap, fc.fold_kmax_nopost);
            if (rbgs) kcap = std::min(kcap, env_int("MGX_FOLD_KMAX_GS", 10));
            if (q.pre && q.post == 1) kcap = std::min(kcap, 8);         // correction and restriction may meet in one pass: at most 8 levels
            parts = split_sweeps(mu, std::max(1, kcap / per), 1e-3, 1e-12, [&](int k, int m) {
                // a block done in ONE pass carries the correction AND the residual stage: some depths exist for either only
                if (k == mu && m == mu && !cycle_k_supported(per * k, rbgs, q.f64, q.post, q.pre, fc.arith)) return -1.0;
                return fold_pass_cost(per * k, rbgs, q.post, q.f64, fc.arith);
            });
            std::sort(parts.begin(), parts.end(), [](int a, int b) { return a > b; });
        }
    }
    const int np = (int)parts.size();
    const int stage_rows = q.post == 2 ? 1 : (q.post == 1 ? 2 : 0);
    int done = 0;
    for (int p = 0; p < np; ++p) {
        const int sw = parts[p], K = per * sw;
        const bool P = q.pre && p == 0, zin = q.zero_in && p == 0;
        const int Q = (p == np - 1) ? q.post : 0;
        const int ext = q.widen ? per * (mu - (done + sw)) + (p != np - 1 ? stage_rows : 0) : 0;
        int lo = std::max(q.row_lo - ext, first), hi = std::min(q.row_hi + ext, last);
        // rows read: [lo - K, hi + K) clipped to the global boundary rows
        if (q.strict && hi > lo && (std::max(lo - K, first - 1) < 0 || std::min(hi + K - 1, last) > q.rows - 1)) return false;
        lo = std::max(lo, 1);
        hi = std::min(hi, q.rows - 1);
        const int kind = (P || Q) ? PASS_FOLDED : (!rbgs && K == 1) ? PASS_JACOBI : (rbgs && !staged && !fuse) ? PASS_RBGS : PASS_FUSED;
        int R = q.rpc;
        if (kind == PASS_FUSED || kind == PASS_FOLDED) R = fuse_rows(fc, N, K, q.f64, hi - lo);
        if (hi > lo) {
            if (kind == PASS_FOLDED) {
                if (!cycle_k_supported(K, rbgs, q.f64, Q, P, fc.arith)) return false;
                if (Q == 1 && !((lo + q.row0) & 1)) return false;        // the restriction's chunks start on odd rows
                if (fuse_rows_auto(fc, N, K, q.f64)) R = -R;
            }
            if (kind == PASS_FUSED && !fused_k_supported(K, rbgs)) return false;
            if (zin && (kind == PASS_JACOBI || kind == PASS_RBGS)) return false;     // a stand-alone single sweep reads its input
        }
        plan->push_back({kind, K, P, Q, zin, lo + q.row0, hi + q.row0, R});
        done += sw;
    }
    return true;
}

} // namespace mgx
