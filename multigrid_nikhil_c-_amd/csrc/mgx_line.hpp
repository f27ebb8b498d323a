// mgx_line.hpp - zebra line Gauss-Seidel smoothing for the general-operator hierarchies (cfg.smoother =
// MGX_SMOOTHER_LINE_X / LINE_Y / LINE_ALT with op = MGX_OPERATOR_STENCIL5 / MGX_OPERATOR_GALERKIN): the answer to
// anisotropy, which no point smoother, transfer or cycle index repairs.  tests/line_ref.py states everything below in
// numpy, operation by operation.
//
// THE SWEEP.  An x-line sweep solves the tridiagonal system T x = rhs of every grid row exactly, T = tridiag(w, c, e),
// rhs = b minus the off-line terms: first the odd grid rows (colour 1: the rows that are not coarse rows), then the even
// ones, which read the rows just written.  A row couples to rows i +- 1 only, on nine-point levels too, so two colours
// suffice and the rows of a colour are independent.  Off-line terms are subtracted one by one in the order NW, N, NE,
// SW, S, SE (five-point levels: N, S); coefficients that point at the Dirichlet ring are never read.  A y-line sweep is
// the same with rows and columns exchanged (T = tridiag(n, c, s), odd grid columns first, off-line order NW, W, SW, NE,
// E, SE); an alternating sweep is an x-sweep followed by a y-sweep.  No damping: cfg.omega is not used.
//
// THE FACTORS depend on the operator only and are built with it (k_line_factor, one lane per line, sequential), in the
// level's type:   m_0 = 1 / c_0,   g_{j-1} = e_{j-1} m_{j-1},   m_j = 1 / (c_j - w_j g_{j-1}),   g_last = 0.
// A sweep is then  y_j = (rhs_j - w_j y_{j-1}) m_j,  x_j = y_j - g_j x_{j+1}.  A zero or non-finite pivot raises a
// device flag (an ordinary atomic OR) that the host reads after the build: MGX_ERR_INVALID.
//
// BOTH RECURRENCES ARE AFFINE in the value carried along the line, y_j = (-w_j m_j) y_{j-1} + rhs_j m_j, so a line can be
// cut into segments that run at the same time from a zero carry and are then joined, in segment order:
//   k_line_x  one wave per row, marching in tiles of 64 lanes x one 16-byte vector.  A lane folds its W points into a
//             map (alpha, beta), a 6-step wave scan composes the maps, the tile's carry comes from lane 63 of the
//             previous tile, and every lane then runs the recurrence itself from its true carry-in.  y goes out to the
//             row (which belongs to this wave; nobody else reads it in this launch) and the backward recurrence runs
//             the same way from the last tile to the first, reading y back.
//   k_line_y  one lane per column (every access of a wave is one row segment), the column cut into chunks of R rows,
//             one wave per chunk, all chunks of a 64-column strip in one workgroup.  Pass 1: y' from a zero carry;
//             the true carry-in of chunk k follows from the chunk ends in LDS, combined in chunk order by every wave
//             for itself: c_{k+1} = y'_end(k) + hf_end(k) c_k.  Pass 2, backwards: y = y' + hf c and x' from a zero
//             carry; x carries likewise; pass 3: x = x' + hb c.  hf_r = prod_{chunk start..r} (-n_j m_j) and
//             hb_r = prod_{r..chunk end} (-g_j) depend on the operator and R only: built beside m and g.  With one
//             chunk (small levels) passes 1 and 2 are the plain recurrences and hf / hb are not read.
// NOT BUILT: carries of more chunks than one workgroup holds, through a small global array and a second launch.  A colour
// launch of k_line_y is therefore ceil(N / 128) workgroups (32 at N = 4096), and the kernel is far from the HBM rate on
// large levels (profiles/line_kernel_trace_summary.md: 0.10-0.17 of k_jacobi_var's bytes/s at 4096^2 - the open item).
// Lane l of k_line_y takes column 2 l + 1 (or 2 l + 2): the coefficient loads use every other element of a cache line;
// the iterate's lines are used in full (the columns in between are the off-line neighbours).
// Every combination order is fixed and there is no floating-point atomic: two runs give the same bits.  Against the
// sequential recurrence of the reference the carries are rounded differently (agreement to rounding, not bit for bit);
// the factors are bit for bit.
//
// ALGORITHMIC BYTES per updated point, in sizeof(T) (what tools/galerkin_bench.py divides by): forward b, the two
// neighbouring lines of v, the off-line coefficients (2 / 6), the sub-diagonal and m in, y out; backward y and g in, x
// out:  11 on five-point levels, 15 on nine-point levels.  k_line_y with more than one chunk adds hf, x', hb in and x out:
// 15 / 19.  A colour launch updates half the level.
#pragma once

#include "mgx_var.hpp"

namespace mgx {

constexpr int kLineMaxChunks = 16;          // waves of a k_line_y workgroup

// rows per chunk of k_line_y on a level of N intervals: at least 64 and at most kLineMaxChunks chunks; `want` > 0
// (MGX_LINE_CHUNK) overrides the 64
inline int line_chunk_rows(int N, int want)
{
    const int least = (N - 1 + kLineMaxChunks - 1) / kLineMaxChunks;
    return std::max(want > 0 ? want : 64, std::max(least, 1));
}
inline int line_chunks(int N, int R) { return (N - 1 + R - 1) / R; }

// ---- set-up ---------------------------------------------------------------------------------------------------
// DIR 0: the lines are grid rows (sub-diagonal w, super-diagonal e); DIR 1: grid columns (n, s).  hf / hb (DIR 1 only,
// may be null): the homogeneous factors of chunks of R rows
template <typename T, int DIR>
__global__ void k_line_factor(Op9<T> a, T* __restrict__ m, T* __restrict__ g, T* __restrict__ hf, T* __restrict__ hb, int N, long pitch,
                              int R, int* __restrict__ flag)
{
    const int line = 1 + blockIdx.x * blockDim.x + threadIdx.x;
    if (line >= N) return;
    const T* __restrict__ sub = a.a[DIR == 0 ? 3 : 1];
    const T* __restrict__ sup = a.a[DIR == 0 ? 4 : 2];
    const T* __restrict__ dia = a.a[0];
    const long step = DIR == 0 ? 1 : pitch;
    const long base = DIR == 0 ? (long)line * pitch : (long)line;
    T gprev = (T)0, h = (T)0;
    bool bad = false;
    for (int j = 1; j < N; ++j) {
        const long at = base + (long)j * step;
        T p = dia[at];
        const T sb = j > 1 ? sub[at] : (T)0;
        if (j > 1) p = p - sb * gprev;
        bad = bad || !(p != (T)0 && isfinite(p));
        const T mj = (T)1 / p;
        const T gj = j < N - 1 ? sup[at] * mj : (T)0;
        m[at] = mj;
        g[at] = gj;
        if (hf) {
            const T f = -(sb * mj);
            h = (j - 1) < R ? (T)0 : ((j - 1) % R == 0 ? f : f * h);      // the first chunk has no carry-in
            hf[at] = h;
        }
        gprev = gj;
    }
    if (hb)
        for (int j = N - 1; j >= 1; --j) {
            const long at = base + (long)j * step;
            const T f = -g[at];
            h = (j == N - 1 || (j - 1) % R == R - 1) ? f : f * h;
            hb[at] = h;
        }
    if (bad) atomicOr(flag, 1 << DIR);
}

// ---- x-lines ---------------------------------------------------------------------------------------------------
template <typename T> struct Affine { T a, b; };            // y_out = a y_in + b

// the maps of lanes 0 .. l composed (UP) or of lanes l .. 63 (!UP), in lane order: 6 steps
template <bool UP, typename T>
__device__ __forceinline__ Affine<T> wave_scan(Affine<T> f, int lane)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T pa = UP ? __shfl_up(f.a, d, kWave) : __shfl_down(f.a, d, kWave);
        const T pb = UP ? __shfl_up(f.b, d, kWave) : __shfl_down(f.b, d, kWave);
        const bool has = UP ? lane >= d : lane + d < kWave;
        if (has) { f.b = f.a * pb + f.b; f.a = f.a * pa; }
    }
    return f;
}
// the carry into this lane: the scanned map of the lane before it applied to the tile's carry
template <bool UP, typename T>
__device__ __forceinline__ T lane_carry(const Affine<T>& scanned, T tile_carry, int lane)
{
    const T pa = UP ? __shfl_up(scanned.a, 1, kWave) : __shfl_down(scanned.a, 1, kWave);
    const T pb = UP ? __shfl_up(scanned.b, 1, kWave) : __shfl_down(scanned.b, 1, kWave);
    const bool edge = UP ? lane == 0 : lane == kWave - 1;
    return edge ? tile_carry : pa * tile_carry + pb;
}

// one colour of an x-line sweep, in place: wave q of the launch takes grid row row0 + 2 q (lines of them)
template <typename T, int NQ>
__global__ void __launch_bounds__(kBlock)
k_line_x(T* __restrict__ v, const T* __restrict__ rhs, Op9<T> a, const T* __restrict__ mf, const T* __restrict__ gf, int N, long pitch,
         int row0, int lines)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    constexpr int TW = kWave * W;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= lines) return;
    const int row = row0 + 2 * q;
    const bool up_in = row > 1, dn_in = row < N - 1;          // else the coefficients point at the ring: not read
    const int tiles = (N + TW - 1) / TW;
    T* __restrict__ vr = v + (long)row * pitch;
    const long ro = (long)row * pitch;

    T carry = (T)0;
    for (int t = 0; t < tiles; ++t) {
        const int col = t * TW + lane * W;
        const bool in = col < N;
        const Lanes<T> b = load_lanes(rhs + ro + col, in);
        const Lanes<T> up = load_lanes(vr - pitch + col, in), dn = load_lanes(vr + pitch + col, in);
        const Lanes<T> w = load_lanes(a.a[3] + ro + col, in), m = load_lanes(mf + ro + col, in);
        const Lanes<T> cn = load_lanes(a.a[1] + ro + col, in && up_in), cs = load_lanes(a.a[2] + ro + col, in && dn_in);
        Lanes<T> cnw, cne, csw, cse;
        T ul = (T)0, ur = (T)0, dl = (T)0, dr = (T)0;
        if constexpr (NQ == 9) {
            cnw = load_lanes(a.a[5] + ro + col, in && up_in); cne = load_lanes(a.a[6] + ro + col, in && up_in);
            csw = load_lanes(a.a[7] + ro + col, in && dn_in); cse = load_lanes(a.a[8] + ro + col, in && dn_in);
            if (in && col > 0) { ul = vr[-pitch + col - 1]; dl = vr[pitch + col - 1]; }
            if (in) { ur = vr[-pitch + col + W]; dr = vr[pitch + col + W]; }          // col + W <= N: inside the row
        }
        Lanes<T> r, ww, mm;
        Affine<T> f{(T)1, (T)0};
#pragma unroll
        for (int x = 0; x < W; ++x) {
            const int c = col + x;
            const bool valid = c >= 1 && c < N;
            const int xl = x == 0 ? 0 : x - 1, xr = x == W - 1 ? x : x + 1;
            T acc = b.a[x];
            if constexpr (NQ == 9) acc = acc - (c > 1 ? cnw.a[x] : (T)0) * (x == 0 ? ul : up.a[xl]);
            acc = acc - cn.a[x] * up.a[x];
            if constexpr (NQ == 9) acc = acc - (c < N - 1 ? cne.a[x] : (T)0) * (x == W - 1 ? ur : up.a[xr]);
            if constexpr (NQ == 9) acc = acc - (c > 1 ? csw.a[x] : (T)0) * (x == 0 ? dl : dn.a[xl]);
            acc = acc - cs.a[x] * dn.a[x];
            if constexpr (NQ == 9) acc = acc - (c < N - 1 ? cse.a[x] : (T)0) * (x == W - 1 ? dr : dn.a[xr]);
            r.a[x] = valid ? acc : (T)0;
            ww.a[x] = (valid && c > 1) ? w.a[x] : (T)0;
            mm.a[x] = valid ? m.a[x] : (T)0;
            f.b = (r.a[x] - ww.a[x] * f.b) * mm.a[x];
            f.a = (-(ww.a[x] * mm.a[x])) * f.a;
        }
        T y = lane_carry<true>(wave_scan<true>(f, lane), carry, lane);
        Lanes<T> o;
#pragma unroll
        for (int x = 0; x < W; ++x) { y = (r.a[x] - ww.a[x] * y) * mm.a[x]; o.a[x] = y; }
        carry = __shfl(y, kWave - 1, kWave);
        vstore<V>(vr + col, from_lanes(o), in);
    }

    carry = (T)0;
    for (int t = tiles - 1; t >= 0; --t) {
        const int col = t * TW + lane * W;
        const bool in = col < N;
        const Lanes<T> y = load_lanes(vr + col, in), g = load_lanes(gf + ro + col, in);
        Lanes<T> gg;
        Affine<T> f{(T)1, (T)0};
#pragma unroll
        for (int x = W - 1; x >= 0; --x) {
            const int c = col + x;
            gg.a[x] = (c >= 1 && c < N) ? g.a[x] : (T)0;               // y is zero there already
            f.b = y.a[x] - gg.a[x] * f.b;
            f.a = (-gg.a[x]) * f.a;
        }
        T xv = lane_carry<false>(wave_scan<false>(f, lane), carry, lane);
        Lanes<T> o;
#pragma unroll
        for (int x = W - 1; x >= 0; --x) { xv = y.a[x] - gg.a[x] * xv; o.a[x] = xv; }
        carry = __shfl(xv, 0, kWave);
        V ov = from_lanes(o);
        mask_cols(ov, (long)col, N);
        vstore<V>(vr + col, ov, in);
    }
}

// ---- y-lines ---------------------------------------------------------------------------------------------------
// one colour of a y-line sweep, in place: lane l of workgroup g takes grid column col0 + 2 (64 g + l) (lines of them),
// wave k the rows [1 + k R, 1 + (k + 1) R) of it; blockDim.x = 64 * chunks
template <typename T, int NQ>
__global__ void __launch_bounds__(kWave * kLineMaxChunks)
k_line_y(T* __restrict__ v, const T* __restrict__ rhs, Op9<T> a, const T* __restrict__ mf, const T* __restrict__ gf,
         const T* __restrict__ hf, const T* __restrict__ hb, int N, long pitch, int col0, int lines, int R)
{
    __shared__ T ends[2][kLineMaxChunks][kWave];
    const int lane = threadIdx.x & 63;
    const int k = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int chunks = blockDim.x >> 6;
    const int l = blockIdx.x * kWave + lane;
    const bool active = l < lines;
    const int col = col0 + 2 * (active ? l : 0);
    const int r0 = 1 + k * R, r1 = min(r0 + R, N);
    const bool w_in = col > 1, e_in = col < N - 1;            // else the coefficients point at the ring: not read

    // pass 1: y' down the chunk from a zero carry
    T y = (T)0;
    if (active)
        for (int r = r0; r < r1; ++r) {
            const long at = (long)r * pitch + col;
            const bool up_in = r > 1, dn_in = r < N - 1;
            T acc = rhs[at];
            if constexpr (NQ == 9) acc = acc - ((w_in && up_in) ? a.a[5][at] : (T)0) * v[at - pitch - 1];
            acc = acc - (w_in ? a.a[3][at] : (T)0) * v[at - 1];
            if constexpr (NQ == 9) acc = acc - ((w_in && dn_in) ? a.a[7][at] : (T)0) * v[at + pitch - 1];
            if constexpr (NQ == 9) acc = acc - ((e_in && up_in) ? a.a[6][at] : (T)0) * v[at - pitch + 1];
            acc = acc - (e_in ? a.a[4][at] : (T)0) * v[at + 1];
            if constexpr (NQ == 9) acc = acc - ((e_in && dn_in) ? a.a[8][at] : (T)0) * v[at + pitch + 1];
            const T sb = r > r0 ? a.a[1][at] : (T)0;
            y = (acc - sb * y) * mf[at];
            v[at] = y;
        }
    T cin = (T)0;
    if (chunks > 1) {
        ends[0][k][lane] = y;
        __syncthreads();
        if (active)
            for (int j = 0; j < k; ++j) {
                const int last = min(1 + (j + 1) * R, N) - 1;
                cin = ends[0][j][lane] + hf[(long)last * pitch + col] * cin;
            }
    }
    // pass 2, up the chunk: the true y, and x' from a zero carry
    T x = (T)0;
    if (active)
        for (int r = r1 - 1; r >= r0; --r) {
            const long at = (long)r * pitch + col;
            T yv = v[at];
            if (k > 0) yv = yv + hf[at] * cin;
            const T gg = r < r1 - 1 ? gf[at] : (T)0;
            x = yv - gg * x;
            v[at] = x;
        }
    if (chunks > 1) {
        ends[1][k][lane] = x;
        __syncthreads();
        T xin = (T)0;
        if (active && k < chunks - 1) {
            for (int j = chunks - 1; j > k; --j) xin = ends[1][j][lane] + hb[(long)(1 + j * R) * pitch + col] * xin;
            // pass 3: the carry from the chunks below
            for (int r = r0; r < r1; ++r) {
                const long at = (long)r * pitch + col;
                v[at] = v[at] + hb[at] * xin;
            }
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------
// what a launch needs of a level: the operator and the factors of the directions the handle smooths in (null otherwise)
template <typename T> struct LineLevel {
    Op9<T> a;
    bool nine;
    int N;
    long pitch;
    T *mx, *gx, *my, *gy, *hf, *hb;
    int R;                                  // rows per chunk of k_line_y
};

// the factors of one direction of the operator in l.a; flag: device int, bit `dir` raised on a breakdown
template <typename T>
void launch_line_factor(const LineLevel<T>& l, int dir, int* flag, hipStream_t st)
{
    const dim3 grd((l.N - 1 + 63) / 64), blk(64);
    const bool chunked = line_chunks(l.N, l.R) > 1;
    if (dir == 0) hipLaunchKernelGGL((k_line_factor<T, 0>), grd, blk, 0, st, l.a, l.mx, l.gx, (T*)nullptr, (T*)nullptr, l.N, l.pitch, l.R, flag);
    else hipLaunchKernelGGL((k_line_factor<T, 1>), grd, blk, 0, st, l.a, l.my, l.gy, chunked ? l.hf : nullptr, chunked ? l.hb : nullptr, l.N,
                            l.pitch, l.R, flag);
}

// one sweep of v in place: dirs bit 0: x-lines, bit 1: y-lines (both: x first).  Returns the launches made
template <typename T>
int launch_line_sweep(const LineLevel<T>& l, T* v, const T* b, int dirs, hipStream_t st)
{
    int launches = 0;
    with_point_count(l.nine, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        for (int colour = 0; colour < 2 && (dirs & 1); ++colour) {
            const int lines = colour == 0 ? l.N / 2 : l.N / 2 - 1;
            if (lines <= 0) continue;
            hipLaunchKernelGGL((k_line_x<T, NQ>), dim3((lines + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, st, v, b, l.a,
                               (const T*)l.mx, (const T*)l.gx, l.N, l.pitch, 1 + colour, lines);
            ++launches;
        }
        for (int colour = 0; colour < 2 && (dirs & 2); ++colour) {
            const int lines = colour == 0 ? l.N / 2 : l.N / 2 - 1;
            if (lines <= 0) continue;
            const int chunks = line_chunks(l.N, l.R);
            hipLaunchKernelGGL((k_line_y<T, NQ>), dim3((lines + kWave - 1) / kWave), dim3(kWave * chunks), 0, st, v, b, l.a, (const T*)l.my,
                               (const T*)l.gy, (const T*)l.hf, (const T*)l.hb, l.N, l.pitch, 1 + colour, lines, l.R);
            ++launches;
        }
    });
    return launches;
}

// mgx.hip declares these instantiations; mgx_inst.hip (-DMGX_INST_KIND=6) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
extern template void launch_line_factor<double>(const LineLevel<double>&, int, int*, hipStream_t);
extern template void launch_line_factor<float>(const LineLevel<float>&, int, int*, hipStream_t);
extern template int launch_line_sweep<double>(const LineLevel<double>&, double*, const double*, int, hipStream_t);
extern template int launch_line_sweep<float>(const LineLevel<float>&, float*, const float*, int, hipStream_t);
#endif

} // namespace mgx
