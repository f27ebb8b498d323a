// mgx_launch.hpp - host side of the kernels of mgx_kernels.hpp: launch geometry and the typed launch
// wrappers.  Which launches make up a smoothing block is decided by the pass planner (mgx_pass_plan.hpp).
// No solver state here: the single-GPU handle (mgx.hip) and the slab operators of the multi-GPU
// driver use the same functions.
#pragma once

#include "../../include/mgx.h"
#include "mgx_kernels.hpp"
#include "mgx_pass_plan.hpp"

#include <algorithm>

namespace mgx {

inline long level_pitch(int level, int dtype)
{
    const long N = 1L << level;
    const long align = (dtype == MGX_DTYPE_F64) ? 32 : 64;   // 256 bytes
    return (N + 1 + align - 1) / align * align;
}

// PS:127, 138-140: the Jacobi scalars c0 = 1 - omega, c1 = omega / 4.  The float path evaluates them in double
// from the float omega and narrows them: the float bits depend on this exact expression.
template <typename T> struct JacobiCoef { T c0, c1; };
template <typename T>
JacobiCoef<T> jacobi_coef(double omega)
{
    const T om = (T)omega;
    return {(T)(1.0 - (double)om), (T)((double)om / 4.0)};
}

// The smoother kernels come in three sets per element type: Jacobi separately rounded, Jacobi FMA, red-black GS.
// f(KernelSet<T, SM, AR>{}) for the set of (f64, smoother, arith).
template <typename T_, int SM_, int AR_> struct KernelSet { using T = T_; static constexpr int SM = SM_, AR = AR_; };
template <typename F>
decltype(auto) with_kernel_set(bool f64, int smoother, int arith, F&& f)
{
    const bool rbgs = (smoother == MGX_SMOOTHER_RBGS);
    if (f64) return rbgs ? f(KernelSet<double, 1, 0>{}) : (arith ? f(KernelSet<double, 0, 1>{}) : f(KernelSet<double, 0, 0>{}));
    return rbgs ? f(KernelSet<float, 1, 0>{}) : (arith ? f(KernelSet<float, 0, 1>{}) : f(KernelSet<float, 0, 0>{}));
}

// ---- typed operator launches ----------------------------------------------------
// rows_alloc: rows the arrays hold.  A sweep of rows [row_lo,row_hi) reads rows row_lo-1 .. row_hi:
// ranges that would read outside the allocation are refused here, in one place for every caller
// (and the kernels predicate their row loads on rows_alloc as well).
template <typename T>
int launch_jacobi(const T* vin, const T* b, T* vout, int N, long pitch, int row_lo, int row_hi,
                  double omega, int rpc, hipStream_t st, int rows_alloc, int arith = 0)
{
    if (row_hi <= row_lo) return MGX_OK;
    if (row_lo < 1 || row_hi > rows_alloc - 1) return MGX_ERR_INVALID;
    const auto [c0, c1] = jacobi_coef<T>(omega);
    if (rpc <= 0) {
        // default: one wave per row and strip (see k_jacobi_rows)
        const Launch g = make_launch(N, VecOf<T>::W, row_hi - row_lo, 1);
        if (arith) hipLaunchKernelGGL((k_jacobi_rows<T, 1>), dim3(g.blocks), dim3(kBlock), 0, st, vin, b, vout, N, pitch,
                                      row_lo, row_hi, g.strips, c0, c1, rows_alloc);
        else hipLaunchKernelGGL((k_jacobi_rows<T, 0>), dim3(g.blocks), dim3(kBlock), 0, st, vin, b, vout, N, pitch,
                                row_lo, row_hi, g.strips, c0, c1, rows_alloc);
        return MGX_OK;
    }
    const Launch g = make_launch(N, VecOf<T>::W, row_hi - row_lo, rpc);
    if (arith) hipLaunchKernelGGL((k_jacobi<T, 1>), dim3(g.blocks), dim3(kBlock), 0, st, vin, b, vout, N, pitch,
                                  row_lo, row_hi, g.R, g.strips, g.chunks, c0, c1, rows_alloc);
    else hipLaunchKernelGGL((k_jacobi<T, 0>), dim3(g.blocks), dim3(kBlock), 0, st, vin, b, vout, N, pitch,
                            row_lo, row_hi, g.R, g.strips, g.chunks, c0, c1, rows_alloc);
    return MGX_OK;
}

template <typename T>
void launch_rbgs(const T* vin, const T* b, T* vout, int N, long pitch, int row_lo, int row_hi,
                 int row_parity, int bnd_lo, int bnd_hi, int rpc, hipStream_t st)
{
    if (row_hi <= row_lo) return;
    const Launch g = make_launch(N, VecOf<T>::W, row_hi - row_lo, rpc);
    hipLaunchKernelGGL((k_rbgs<T>), dim3(g.blocks), dim3(kBlock), 0, st, vin, b, vout, N, pitch,
                       row_lo, row_hi, g.R, g.strips, g.chunks, row_parity, bnd_lo, bnd_hi);
}

// K levels in one pass (k_jacobi_fused<T,K,SM>): K Jacobi sweeps (SM = 0) or K/2
// red-black Gauss-Seidel sweeps (SM = 1)
template <typename T, int K, int SM, int AR>
void launch_fused_k(const T* vin, const T* b, T* vout, int N, long pitch, int row_lo, int row_hi,
                    T c0, T c1, int bnd_lo, int bnd_hi, int row_parity, int R, hipStream_t st, int rows_alloc, int zero_in)
{
    constexpr int OUT = fused_out_lanes<K, VecOf<T>::W>();
    R = trip_rows(R, 2 * K, trip_steps<T>(), 1);       // whole loop trips in the interior body
    Launch g = make_launch(N, VecOf<T>::W, row_hi - row_lo, R);
    g.strips = (N / VecOf<T>::W + OUT - 1) / OUT;
    const long waves = (long)g.strips * g.chunks;
    g.blocks = (int)(((waves + kWavesPerBlock - 1) / kWavesPerBlock + 7) / 8 * 8);
    hipLaunchKernelGGL((k_jacobi_fused<T, K, SM, AR>), dim3(g.blocks), dim3(kBlock), 0, st, vin, b, vout, N, pitch,
                       row_lo, row_hi, g.R, g.strips, g.chunks, c0, c1, bnd_lo, bnd_hi, row_parity, rows_alloc, zero_in);
}

// rows_alloc: number of rows the arrays hold (every load is bounded by it)
template <typename T, int SM, int AR>
bool launch_fused(int K, const T* vin, const T* b, T* vout, int N, long pitch, int row_lo, int row_hi,
                  T c0, T c1, int bnd_lo, int bnd_hi, int row_parity, int R, hipStream_t st, int rows_alloc, int zero_in)
{
    switch (K) {
        case 2: launch_fused_k<T, 2, SM, AR>(vin, b, vout, N, pitch, row_lo, row_hi, c0, c1, bnd_lo, bnd_hi, row_parity, R, st, rows_alloc, zero_in); return true;
        case 4: launch_fused_k<T, 4, SM, AR>(vin, b, vout, N, pitch, row_lo, row_hi, c0, c1, bnd_lo, bnd_hi, row_parity, R, st, rows_alloc, zero_in); return true;
        case 6: launch_fused_k<T, 6, SM, AR>(vin, b, vout, N, pitch, row_lo, row_hi, c0, c1, bnd_lo, bnd_hi, row_parity, R, st, rows_alloc, zero_in); return true;
        case 8: launch_fused_k<T, 8, SM, AR>(vin, b, vout, N, pitch, row_lo, row_hi, c0, c1, bnd_lo, bnd_hi, row_parity, R, st, rows_alloc, zero_in); return true;
        case 10: launch_fused_k<T, 10, SM, AR>(vin, b, vout, N, pitch, row_lo, row_hi, c0, c1, bnd_lo, bnd_hi, row_parity, R, st, rows_alloc, zero_in); return true;
        default: break;
    }
    if constexpr (SM == 0) {
        switch (K) {
            case 3: launch_fused_k<T, 3, 0, AR>(vin, b, vout, N, pitch, row_lo, row_hi, c0, c1, bnd_lo, bnd_hi, row_parity, R, st, rows_alloc, zero_in); return true;
            case 5: launch_fused_k<T, 5, 0, AR>(vin, b, vout, N, pitch, row_lo, row_hi, c0, c1, bnd_lo, bnd_hi, row_parity, R, st, rows_alloc, zero_in); return true;
            default: break;
        }
    }
    return false;
}

// ---- smoother passes with the cycle's transfers folded in (k_jacobi_cycle) ----------
struct FoldArgs {
    const void* coarse_e = nullptr;   // PRE: correction to add while loading
    void* coarse_b = nullptr;         // POST 1: restricted residual
    void* coarse_zero = nullptr;      // POST 1: coarse guess to zero
    int restrict_mode = 0;
    double* partial = nullptr;        // POST 2: per-block sums of r^2
    long cpitch = 0;
    int zero_in = 0;                  // the input iterate is all zero: the pass does not read it
    // rows to update, GLOBAL numbers (base pointers moved back by the window's first row), and the window of rows that exist
    int row_lo = 0, row_hi = 0;
    CycleWin win{0, 0, 0, 0, 0, 0};
};

// chunk geometry of a k_jacobi_cycle launch: mgx_geom.hpp (cycle_geom_pick / cycle_tile_at); the knobs from the environment
// (read at every launch of a deep pass: the parity tests switch them inside one process)
inline GeomKnobs geom_knobs()
{
    GeomKnobs k;
    k.edge_short = env_int("MGX_EDGE_SHORT", 1) != 0;
    k.edge_pct = env_int("MGX_EDGE_PCT", 23);
    k.last_pct = env_int("MGX_LAST_PCT", 38);
    k.min_chunk = std::max(8, env_int("MGX_MIN_CHUNK", 16));
    k.min_rounds = std::max(1, env_int("MGX_MIN_ROUNDS", 1));
    k.min_rounds_rows = env_int("MGX_MIN_ROUNDS_ROWS", 1024);
    k.pair = env_int("MGX_PAIR", 1) != 0;
    k.pair_ratio = std::max(100, env_int("MGX_PAIR_RATIO", 130));
    k.pair_max_rows = env_int("MGX_PAIR_MAX_ROWS", 640);
    k.pair_min_rows = env_int("MGX_PAIR_MIN_ROWS", 150);
    return k;
}
// R < 0: choose the chunk height here (deep double passes: whole rounds of 2048 waves, see fuse_rows_deep;
// -R is the height the uniform rule gave)
template <typename T, int K, int PRE, int POST, int SM, int AR>
int launch_cycle_k(const T* vin, const T* b, T* vout, const FoldArgs& fa, int N, long pitch, T c0, T c1, int R,
                   hipStream_t st)
{
    constexpr int OUT = cycle_out_lanes<K, POST, VecOf<T>::W>();
    constexpr bool BL = cycle_b_in_lds<T, K, POST, SM>();
    constexpr int E = (POST == 1 ? 3 : (POST == 2 ? 2 : 0)) + (cycle_skew<T, K, PRE, POST, SM, AR>() > 0 ? 1 : 0);   // row steps of a chunk beyond R + 2K
    constexpr int kTripSteps = BL ? kBRing : trip_steps<T>();
    const int row_lo = fa.row_lo, row_hi = fa.row_hi;
    const CycleWin& win = fa.win;
    if (POST == 1 && !(row_lo & 1)) return -1;         // chunks must start on odd rows (POST = 1)
    const int strips = (N / VecOf<T>::W + OUT - 1) / OUT;
    const bool auto_rows = R < 0;
    if (auto_rows) R = -R;
    // the bodies run whole trips (kBRing steps for the deep variants, kTrip otherwise): a chunk is R + 2K + (stage rows)
    // steps long; cycle_geom_pick takes even heights that make it a multiple of the trip (or one short of it).
    // Deep passes (rhs ring in LDS): shorter edge-class tiles; auto_rows: the fewest rounds of resident workgroups with
    // chunks of at most ~200 rows, or ONE round with paired heights (mgx_geom.hpp)
    // an end of the range whose cone (K + 1 rows above, K + 1..2 below: the kernel's `interior`) leaves the unknown rows
    // that exist runs the edge body and gets shorter chunks; the ends of a middle slab, whose halo rows hold the cone, do not
    constexpr int ETOP = POST ? 1 : 0, EBOT = POST == 1 ? 2 : (POST == 2 ? 1 : 0);
    const bool top_edge = (row_lo - K - ETOP) < std::max(win.row_first, 1) || (PRE && ((row_lo - K - ETOP) >> 1) < win.crow_first);
    const bool bot_edge = (row_hi + K + EBOT - 1) > std::min(win.row_last, N - 1) || (PRE && ((row_hi + K + EBOT) >> 1) > win.crow_last);
    GeomKnobs kn = BL ? geom_knobs() : GeomKnobs();
    // (float passes: a wave covers twice the columns, a grid has half the strips and twice the chunks per strip - the paired
    // form pays from shorter chunks: mixed V(10,10) at 8192^2, float finest-level passes 0.403 -> 0.393-0.395 ms at 100 rows)
    if (sizeof(T) == 4 && BL) kn.pair_min_rows = std::min(kn.pair_min_rows, env_int("MGX_PAIR_MIN_ROWS_F32", 100));
    const CycleGeom g = cycle_geom_pick(row_lo, row_hi, strips, 2 * K + E, kTripSteps, R, auto_rows, BL, kn, top_edge, bot_edge);
    const int blocks = g.blocks;
    const T w = (fa.restrict_mode == MGX_RESTRICT_FW16) ? (T)0.0625 : (T)0.25;
    hipLaunchKernelGGL((k_jacobi_cycle<T, K, PRE, POST, SM, AR>), dim3(blocks), dim3(kBlock), 0, st, vin, b, vout,
                       (const T*)fa.coarse_e, (T*)fa.coarse_b, (T*)fa.coarse_zero, w, fa.partial, N, pitch, fa.cpitch,
                       row_lo, row_hi, g.R, strips, g.chunks, g.Re, g.chunks_e, g.row_last0, g.Rl, g.RB, g.n_tall, g.n_short, g.Rf, c0, c1, fa.zero_in, win);
    return blocks;
}

template <typename T, int PRE, int POST, int SM, int AR>
int launch_cycle(int K, const T* vin, const T* b, T* vout, const FoldArgs& fa, int N, long pitch, T c0, T c1, int R,
                 hipStream_t st)
{
    switch (K) {
        case 2: return launch_cycle_k<T, 2, PRE, POST, SM, AR>(vin, b, vout, fa, N, pitch, c0, c1, R, st);
        case 4: return launch_cycle_k<T, 4, PRE, POST, SM, AR>(vin, b, vout, fa, N, pitch, c0, c1, R, st);
        case 6: return launch_cycle_k<T, 6, PRE, POST, SM, AR>(vin, b, vout, fa, N, pitch, c0, c1, R, st);
        default: break;
    }
    // 8 levels: not for float passes that start from the input and end with a residual stage (with the
    // branch-free interior bodies their predicated body extracts an odd-indexed pair of a float4
    // through a stack slot: scratch)
    if constexpr (sizeof(T) == 8 || PRE == 1 || POST == 0) {
        if (K == 8) return launch_cycle_k<T, 8, PRE, POST, SM, AR>(vin, b, vout, fa, N, pitch, c0, c1, R, st);
    }
    // 10 levels with folded stages: not the most register-hungry combinations (correction AND restriction in
    // one pass; red-black GS with the restriction; in float - packed arithmetic wants aligned register pairs -
    // the correction with the norm): with the rhs window in LDS every instantiated variant fits 256
    // registers = two waves per SIMD, float ones included since round 3 (cycle_b_in_lds)
    // (and the float pre-smoothing pass with the restriction only in FMA mode: the separately rounded one spills 3 dwords)
    if constexpr (!(PRE == 1 && POST == 1) && !(SM == 1 && POST == 1) && !(sizeof(T) == 4 && PRE == 1 && POST == 2) &&
                  !(sizeof(T) == 4 && POST == 1 && AR == 0)) {
        if (K == 10) return launch_cycle_k<T, 10, PRE, POST, SM, AR>(vin, b, vout, fa, N, pitch, c0, c1, R, st);
    }
    if constexpr (SM == 0) {
        switch (K) {
            case 1: return launch_cycle_k<T, 1, PRE, POST, 0, AR>(vin, b, vout, fa, N, pitch, c0, c1, R, st);
            case 3: return launch_cycle_k<T, 3, PRE, POST, 0, AR>(vin, b, vout, fa, N, pitch, c0, c1, R, st);
            case 5: return launch_cycle_k<T, 5, PRE, POST, 0, AR>(vin, b, vout, fa, N, pitch, c0, c1, R, st);
            default: break;
        }
    }
    return -1;
}

// runtime (pre, post) -> the folded stages of k_jacobi_cycle / k_tile_smooth: f(Stages<PRE, POST>{}), all six pairs
template <int PRE_, int POST_> struct Stages { static constexpr int PRE = PRE_, POST = POST_; };
template <typename F>
int with_stages(bool pre, int post, F&& f)
{
    if (pre) return post == 2 ? f(Stages<1, 2>{}) : (post == 1 ? f(Stages<1, 1>{}) : f(Stages<1, 0>{}));
    return post == 2 ? f(Stages<0, 2>{}) : (post == 1 ? f(Stages<0, 1>{}) : f(Stages<0, 0>{}));
}

// ---- small levels: every sweep of a block in one launch on register tiles (k_tile_smooth / k_tile_wide) ----
template <typename T, int SM, int PRE, int POST, int AR>
int launch_tile(const T* vin, const T* b, T* vout, const FoldArgs& fa, int N, long pitch, T c0, T c1, int levels,
                hipStream_t st)
{
    const int He = levels + tile_extra<POST>();
    const int TH = kTileSY - 2 * He, TW = kTileSX - 2 * He;
    if (TH < 8 || TW < 8) return -1;
    const int row_lo = fa.row_lo, row_hi = fa.row_hi;
    const CycleWin& win = fa.win;
    const int tiles_y = (row_hi - row_lo + TH - 1) / TH, tiles_x = (N - 1 + TW - 1) / TW;
    if (tiles_y < 1) return 0;
    const T w = (fa.restrict_mode == MGX_RESTRICT_FW16) ? (T)0.0625 : (T)0.25;
    hipLaunchKernelGGL((k_tile_smooth<T, SM, PRE, POST, AR>), dim3(tiles_y * tiles_x), dim3(kBlock), 0, st, vin, b, vout,
                       (const T*)fa.coarse_e, (T*)fa.coarse_b, (T*)fa.coarse_zero, w, fa.partial, N, pitch, fa.cpitch,
                       levels, c0, c1, tiles_x, fa.zero_in, row_lo, row_hi, win);
    return tiles_y * tiles_x;
}

// the same block on k_tile_wide with bands of rw (8 or 10) rows; geometry: tile_wide_geom (mgx_geom.hpp)
template <typename T, int SM, int PRE, int POST, int AR>
int launch_tile_wide(const T* vin, const T* b, T* vout, const FoldArgs& fa, int N, long pitch, T c0, T c1, int levels,
                     int rw, hipStream_t st)
{
    // fp32: four columns per lane, 256-column arrays; 12-row bands would not fit the registers
    if (VecOf<T>::W == 4) rw = 8;
    const int row_lo = fa.row_lo, row_hi = fa.row_hi;
    const CycleWin& win = fa.win;
    const TileWideGeom g = tile_wide_geom(N, row_lo, row_hi, levels + tile_extra<POST>(), VecOf<T>::W, rw);
    if (g.TH < 8 || g.TW < 8) return -1;
    if (g.tiles_y < 1) return 0;
    const T w = (fa.restrict_mode == MGX_RESTRICT_FW16) ? (T)0.0625 : (T)0.25;
    const dim3 grid(g.tiles_y * g.tiles_x), block(kTileWideWaves * kWave);
    if (rw == 8)
        hipLaunchKernelGGL((k_tile_wide<T, SM, PRE, POST, AR, 8>), grid, block, 0, st, vin, b, vout, (const T*)fa.coarse_e,
                           (T*)fa.coarse_b, (T*)fa.coarse_zero, w, fa.partial, N, pitch, fa.cpitch, levels, c0, c1, g.tiles_x,
                           fa.zero_in, row_lo, row_hi, win);
    else if constexpr (VecOf<T>::W == 2) {
        if (rw != 10) return -1;
        hipLaunchKernelGGL((k_tile_wide<T, SM, PRE, POST, AR, 10>), grid, block, 0, st, vin, b, vout, (const T*)fa.coarse_e,
                           (T*)fa.coarse_b, (T*)fa.coarse_zero, w, fa.partial, N, pitch, fa.cpitch, levels, c0, c1, g.tiles_x,
                           fa.zero_in, row_lo, row_hi, win);
    } else {
        return -1;
    }
    return g.tiles_y * g.tiles_x;
}

// one register-tile launch of `levels` levels with the stages (pre, post): k_tile_wide with bands of `band` rows
// (tile_band), k_tile_smooth when band = 0.  Returns the number of tiles, < 0 when the geometry does not fit.
template <typename T, int SM, int AR>
int launch_tile_pass(const T* vin, const T* b, T* vout, const FoldArgs& fa, int N, long pitch, T c0, T c1, int levels,
                     int band, bool pre, int post, hipStream_t st)
{
    return with_stages(pre, post, [&](auto s) {
        using S = decltype(s);
        return band ? launch_tile_wide<T, SM, S::PRE, S::POST, AR>(vin, b, vout, fa, N, pitch, c0, c1, levels, band, st)
                    : launch_tile<T, SM, S::PRE, S::POST, AR>(vin, b, vout, fa, N, pitch, c0, c1, levels, st);
    });
}

template <typename T>
void launch_restrict(const T* v, const T* b, T* cb, T* czero, int N, long pitch, long cpitch,
                     int crow_lo, int crow_hi, int fine_row_off, int mode, bool fused, int rpc, hipStream_t st)
{
    if (crow_hi <= crow_lo) return;
    Launch g = make_launch(N, VecOf<T>::W, crow_hi - crow_lo, rpc > 0 ? (rpc + 1) / 2 : 0);
    const T w = (mode == MGX_RESTRICT_FW16) ? (T)0.0625 : (T)0.25;
    if (fused)
        hipLaunchKernelGGL((k_restrict<T, true>), dim3(g.blocks), dim3(kBlock), 0, st, v, b, cb, czero, N, pitch,
                           cpitch, crow_lo, crow_hi, fine_row_off, g.R, g.strips, g.chunks, w);
    else
        hipLaunchKernelGGL((k_restrict<T, false>), dim3(g.blocks), dim3(kBlock), 0, st, v, b, cb, czero, N, pitch,
                           cpitch, crow_lo, crow_hi, fine_row_off, g.R, g.strips, g.chunks, w);
}

template <typename T>
void launch_prolong(T* v, const T* e, int N, long pitch, long cpitch, int row_lo, int row_hi,
                    int fine_row_off, bool add, int rpc, hipStream_t st)
{
    if (row_hi <= row_lo) return;
    const Launch g = make_launch(N, VecOf<T>::W, row_hi - row_lo, rpc);
    if (add)
        hipLaunchKernelGGL((k_prolong<T, true>), dim3(g.blocks), dim3(kBlock), 0, st, v, e, N, pitch, cpitch,
                           row_lo, row_hi, fine_row_off, g.R, g.strips, g.chunks);
    else
        hipLaunchKernelGGL((k_prolong<T, false>), dim3(g.blocks), dim3(kBlock), 0, st, v, e, N, pitch, cpitch,
                           row_lo, row_hi, fine_row_off, g.R, g.strips, g.chunks);
}

// blocks needed by the sum-of-squares kernel for a given geometry
template <typename T> long sumsq_blocks(int N, int rows, int rpc)
{
    return make_launch(N, VecOf<T>::W, rows, rpc).blocks;
}

// sum (b - A u)^2 over rows -> sum_dev[0]; MODE 2 also writes scaled float residual
// rows_alloc: rows the arrays hold (rows row_lo-1 .. row_hi are read; the kernel predicates on it)
template <typename T, int MODE>
void launch_residual(const T* v, const T* b, void* out, long pitch_out, double* partial, double* sum_dev,
                     double inv_scale, int N, long pitch, int row_lo, int row_hi, int rpc, hipStream_t st,
                     long partial_cap, int rows_alloc)
{
    Launch g = make_launch(N, VecOf<T>::W, row_hi - row_lo, rpc);
    if (MODE != 0 && partial_cap >= 0 && g.blocks > partial_cap) {
        // never write past the partial-sum buffer: fall back to taller chunks
        const int R = (int)(((long)g.strips * (row_hi - row_lo) / kWavesPerBlock + partial_cap - 9) / (partial_cap - 8)) + 1;
        g = make_launch(N, VecOf<T>::W, row_hi - row_lo, R);
    }
    hipLaunchKernelGGL((k_residual<T, MODE>), dim3(g.blocks), dim3(kBlock), 0, st, v, b, out, pitch_out, partial,
                       inv_scale, N, pitch, row_lo, row_hi, g.R, g.strips, g.chunks, rows_alloc);
    if (MODE != 0)
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, st, partial, g.blocks, sum_dev);
}


// ---- one translation unit per group of kernels --------------------------------------------------------
// The smoother kernels are instantiated for every (type, depth, folded stages, smoother, arithmetic mode):
// a few hundred device functions, three minutes of compile time in one translation unit.  mgx.hip therefore
// only DECLARES the launch wrappers' instantiations; mgx_inst.hip, compiled once per group (Makefile:
// -DMGX_INST_KIND / _T / _SMAR / _PP), defines them.  (SM, AR) pairs: Jacobi separate / Jacobi FMA / red-black GS.
#define MGX_FOR_SMAR(X, T) X(T, 0, 0) X(T, 0, 1) X(T, 1, 0)
#define MGX_DECL_CYCLE_PP(T, PRE, POST, SM, AR) \
    extern template int launch_cycle<T, PRE, POST, SM, AR>(int, const T*, const T*, T*, const FoldArgs&, int, long, T, T, int, hipStream_t);
#define MGX_DECL_CYCLE(T, SM, AR) MGX_DECL_CYCLE_PP(T, 1, 2, SM, AR) MGX_DECL_CYCLE_PP(T, 1, 0, SM, AR) MGX_DECL_CYCLE_PP(T, 0, 1, SM, AR) \
    MGX_DECL_CYCLE_PP(T, 0, 2, SM, AR) MGX_DECL_CYCLE_PP(T, 1, 1, SM, AR)
#define MGX_DECL_FUSED(T, SM, AR) \
    extern template bool launch_fused<T, SM, AR>(int, const T*, const T*, T*, int, long, int, int, T, T, int, int, int, int, hipStream_t, int, int);
#define MGX_DECL_TILE(T, SM, AR) \
    extern template int launch_tile_pass<T, SM, AR>(const T*, const T*, T*, const FoldArgs&, int, long, T, T, int, int, bool, int, hipStream_t);
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
MGX_FOR_SMAR(MGX_DECL_CYCLE, double) MGX_FOR_SMAR(MGX_DECL_CYCLE, float)
MGX_FOR_SMAR(MGX_DECL_FUSED, double) MGX_FOR_SMAR(MGX_DECL_FUSED, float)
MGX_FOR_SMAR(MGX_DECL_TILE, double) MGX_FOR_SMAR(MGX_DECL_TILE, float)
#endif

} // namespace mgx
