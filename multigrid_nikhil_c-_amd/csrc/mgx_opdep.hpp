// mgx_opdep.hpp - the operator-dependent ("black box", Alcouffe / Dendy) transfers of the Galerkin hierarchy
// (mgx_build_galerkin_transfer(h, MGX_TRANSFER_OPERATOR)): the weights of P_l are read off the stencil of A_l, the
// restriction is R_l = c P_l^T (c = 1: CONSISTENT, 1/4: FW16) and the coarse operator is A_{l-1} = R_l A_l P_l, again
// nine-point.  tests/opdep_ref.py states every kernel here in numpy, operation by operation (-ffp-contract=off).
//
// Storage: eight weight grids per coarse level in that level's layout, in the order n, s, w, e, nw, ne, sw, se:
// grid x at coarse (I, J) is the weight with which that coarse point contributes to the fine point 2 (I, J) + x.  The
// coincident weight is 1 and is not stored; the ring rows and columns of the grids are zero.  Both transfers are
// gathers: the restriction reads the eight weights of its own coarse point, the prolongation of a fine point one
// weight of each coarse point around it.  No atomics.
//
// Geometry of all four kernels: that of k_galerkin_rap - one wave per coarse row and strip, a lane owns W coarse
// points (one 16-byte vector per coarse grid) and the 2 W fine columns under them (two 16-byte vectors per fine grid),
// the fine column to the left and the coarse columns to either side from the adjacent lanes by DPP.
//
// k_opdep_weights - with the stencil (c, n, s, w, e, nw, ne, sw, se) of the FINE point the weight belongs to:
//     n:  fine (2I-1, 2J)    -(((sw + s) + se) / ((w + c) + e))        s:  fine (2I+1, 2J)    -(((nw + n) + ne) / ((w + c) + e))
//     w:  fine (2I, 2J-1)    -(((ne + e) + se) / ((n + c) + s))        e:  fine (2I, 2J+1)    -(((nw + w) + sw) / ((n + c) + s))
//     nw: fine (2I-1, 2J-1)  -(((se + s W_w) + e W_n) / c)             ne: fine (2I-1, 2J+1)  -(((sw + s W_e) + w W_n) / c)
//     sw: fine (2I+1, 2J-1)  -(((ne + n W_w) + e W_s) / c)             se: fine (2I+1, 2J+1)  -(((nw + n W_e) + w W_s) / c)
//   An edge point collapses its stencil across the grid line it lies on; a cell centre solves its row of A for the
//   centre value with its edge neighbours replaced by their own formula - and the weight with which the edge point
//   between the centre and the coarse point's row / column interpolates from this coarse point is this coarse point's
//   own edge weight (W_x above), so one kernel computes all eight.  A denominator that is zero or not finite gives the
//   bilinear weight (1/2, 1/4).  No coefficient that points at the Dirichlet ring enters any formula.
//
// k_galerkin_rap_opdep - k_galerkin_rap with general weights.  SUMMATION ORDER: that of k_galerkin_rap (accumulator
//   from +0; i row-major over the 3 x 3 patch around 2I; d row-major; D row-major; structurally zero P(i+d, I+D)
//   skipped); each term is ((c P(i, I)) A_f(i, i+d)) P(i+d, I+D), the products formed left to right, a coincident
//   weight being the constant 1 (its multiplication is exact and left out).  Every weight formula is homogeneous of
//   degree 0 in A, so CONSISTENT and FW16 still give operators that differ by an exact factor 4 per level.
//
// k_restrict_opdep - B_c = c P^T f, f the residual B - A U formed in registers (MODE 1: five-point A, the finest
//   level; MODE 2: nine-point A; the sums of k_residual_var, stencil_sum<5 | 9>) or B itself (MODE 0: mgx_restrict_rhs,
//   FMG).  Sum over the 3 x 3 fine patch row-major (NW, N, NE, W, C, E, SW, S, SE; the centre is added unmultiplied),
//   then one multiplication by c.  Optionally zeroes the coarse guess.
//   Bytes per fine point: MODE 0: f in, B_c out, weights: (1 + 1/4 + 2) sizeof(T);  MODE 1: U, B, five A grids:
//   (7 + 1/4 + 2) sizeof(T);  MODE 2: (11 + 1/4 + 2) sizeof(T).
//
// k_prolong_opdep - U (+)= P e.  Coarse row I produces the fine rows 2I and 2I + 1.  A fine point on a coarse row:
//   west coarse point first, then east; on a coarse column: north, then south; a cell centre: ((NW + NE) + SW) + SE.
//   Ring coarse points carry e = 0 and the weight 0.  Bytes per fine point: U in and out (ADD) or out, e (1/4, each
//   row read by two waves: 1/2), weights 2: (2 + 1/2 + 2) sizeof(T).
#pragma once

#include "mgx_galerkin.hpp"

namespace mgx {

template <typename T> struct Wt8 { const T* w[8]; };      // n, s, w, e, nw, ne, sw, se
template <typename T> struct Wt8Out { T* w[8]; };

// storage slot of the weight towards the fine point at offset (dy, dx) != (0, 0)
__host__ __device__ constexpr int wt_slot(int dy, int dx)
{
    return dy < 0 ? (dx < 0 ? 4 : dx == 0 ? 0 : 5) : dy == 0 ? (dx < 0 ? 2 : 3) : (dx < 0 ? 6 : dx == 0 ? 1 : 7);
}

// out[1 + m]: the element at fine column fcol + m of the row at p, m = -1 .. 2W - 1 (two vectors and the last element
// of the left neighbour's second vector)
template <typename T>
__device__ __forceinline__ void load_fine(const T* p, bool ld0, bool ld1, T* out)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    const V v0 = vload<V>(p, ld0);
    const V v1 = vload<V>(p + W, ld1);
    const Lanes<T> l0 = to_lanes(v0), l1 = to_lanes(v1);
    out[0] = from_left(last(v1));
#pragma unroll
    for (int k = 0; k < W; ++k) { out[1 + k] = l0.a[k]; out[1 + W + k] = l1.a[k]; }
}

// out[1 + m]: the element at coarse column col + m, m = -1 .. W
template <typename T>
__device__ __forceinline__ void load_coarse(const T* p, bool ld, T* out)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    const V v = vload<V>(p, ld);
    const Lanes<T> l = to_lanes(v);
    out[0] = from_left(last(v));
    out[W + 1] = from_right(first(v));
#pragma unroll
    for (int k = 0; k < W; ++k) out[1 + k] = l.a[k];
}

template <typename T> __device__ __forceinline__ T opdep_weight(T num, T den, T fallback)
{
    const T w = -(num / den);
    return (isfinite(den) && den != (T)0) ? w : fallback;
}

template <typename T, bool CORNERS>
__global__ void __launch_bounds__(kBlock)
k_opdep_weights(Op9<T> f, Wt8Out<T> w, int NC, long fpitch, long cpitch, int strips)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    constexpr int NQ = CORNERS ? 9 : 5;
    const Tile t = wave_tile(strips, NC - 1);
    if (!t.active) return;
    const Cols cc = lane_cols<W>(t.strip, NC, cpitch);
    const int I = 1 + t.chunk;
    const long fcol = 2 * cc.col;
    const bool ld0 = cc.ld && fcol + W <= fpitch, ld1 = cc.ld && fcol + 2 * W <= fpitch;
    // fv[q][1 + m]: coefficient q of the current fine row at fine column 2 col + m (corners of a five-point level: 0)
    T fv[9][2 * W + 1];
    auto load_row = [&](int iy) {
        const long at = (long)(2 * I + iy) * fpitch + fcol;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            if (q < NQ) load_fine<T>(f.a[q] + at, ld0, ld1, fv[q]);
            else {
#pragma unroll
                for (int m = 0; m < 2 * W + 1; ++m) fv[q][m] = (T)0;
            }
        }
    };
    const T half = (T)0.5, quarter = (T)0.25;
    Lanes<T> o[8];
    load_row(0);
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int m = 1 + 2 * k;
        o[2].a[k] = opdep_weight((fv[6][m - 1] + fv[4][m - 1]) + fv[8][m - 1], (fv[1][m - 1] + fv[0][m - 1]) + fv[2][m - 1], half);
        o[3].a[k] = opdep_weight((fv[5][m + 1] + fv[3][m + 1]) + fv[7][m + 1], (fv[1][m + 1] + fv[0][m + 1]) + fv[2][m + 1], half);
    }
    load_row(-1);
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int m = 1 + 2 * k;
        const T wn = opdep_weight((fv[7][m] + fv[2][m]) + fv[8][m], (fv[3][m] + fv[0][m]) + fv[4][m], half);
        o[0].a[k] = wn;
        o[4].a[k] = opdep_weight((fv[8][m - 1] + fv[2][m - 1] * o[2].a[k]) + fv[4][m - 1] * wn, fv[0][m - 1], quarter);
        o[5].a[k] = opdep_weight((fv[7][m + 1] + fv[2][m + 1] * o[3].a[k]) + fv[3][m + 1] * wn, fv[0][m + 1], quarter);
    }
    load_row(1);
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int m = 1 + 2 * k;
        const T ws = opdep_weight((fv[5][m] + fv[1][m]) + fv[6][m], (fv[3][m] + fv[0][m]) + fv[4][m], half);
        o[1].a[k] = ws;
        o[6].a[k] = opdep_weight((fv[6][m - 1] + fv[1][m - 1] * o[2].a[k]) + fv[4][m - 1] * ws, fv[0][m - 1], quarter);
        o[7].a[k] = opdep_weight((fv[5][m + 1] + fv[1][m + 1] * o[3].a[k]) + fv[3][m + 1] * ws, fv[0][m + 1], quarter);
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        V ov = from_lanes(o[x]);
        mask_cols(ov, cc.col, NC);
        vstore<V>(w.w[x] + (long)I * cpitch + cc.col, ov, cc.st);
    }
}

template <typename T, bool CORNERS>
__global__ void __launch_bounds__(kBlock)
k_galerkin_rap_opdep(Op9<T> f, Wt8<T> w, Op9Out<T> c, int NC, long fpitch, long cpitch, int strips, T rscale)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    constexpr int NQ = CORNERS ? 9 : 5;
    const Tile t = wave_tile(strips, NC - 1);
    if (!t.active) return;
    const Cols cc = lane_cols<W>(t.strip, NC, cpitch);
    const int I = 1 + t.chunk;
    const long fcol = 2 * cc.col;
    const bool ld0 = cc.ld && fcol + W <= fpitch, ld1 = cc.ld && fcol + 2 * W <= fpitch;
    // wt[x][1 + Dy][1 + m]: weight x of the coarse point (I + Dy, col + m), m = -1 .. W (rows 0 and NC hold zeros)
    T wt[8][3][W + 2];
#pragma unroll
    for (int x = 0; x < 8; ++x)
#pragma unroll
        for (int Dy = -1; Dy <= 1; ++Dy) load_coarse<T>(w.w[x] + (long)(I + Dy) * cpitch + cc.col, cc.ld, wt[x][1 + Dy]);
    T acc[9][W];
#pragma unroll
    for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[q][k] = (T)0;
#pragma unroll
    for (int iy = -1; iy <= 1; ++iy) {
        T fv[NQ][2 * W + 1];
        const long at = (long)(2 * I + iy) * fpitch + fcol;
#pragma unroll
        for (int q = 0; q < NQ; ++q) load_fine<T>(f.a[q] + at, ld0, ld1, fv[q]);
#pragma unroll
        for (int ix = -1; ix <= 1; ++ix) {
            T ri[W];                                                                       // c P(i, I)
#pragma unroll
            for (int k = 0; k < W; ++k) ri[k] = rscale * ((iy == 0 && ix == 0) ? (T)1 : wt[wt_slot(iy, ix)][1][1 + k]);
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int q = op9_slot(dy, dx);
                if (q >= NQ) continue;
                T ra[W];
#pragma unroll
                for (int k = 0; k < W; ++k) ra[k] = ri[k] * fv[q][1 + 2 * k + ix];
#pragma unroll
                for (int Dy = -1; Dy <= 1; ++Dy)
#pragma unroll
                for (int Dx = -1; Dx <= 1; ++Dx) {
                    const int oy = iy + dy - 2 * Dy, ox = ix + dx - 2 * Dx;                // i + d relative to 2 (I + D)
                    if (iabs(oy) > 1 || iabs(ox) > 1) continue;
                    const int o = op9_slot(Dy, Dx);
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        if (oy == 0 && ox == 0) acc[o][k] = acc[o][k] + ra[k];
                        else acc[o][k] = acc[o][k] + ra[k] * wt[wt_slot(oy, ox)][1 + Dy][1 + k + Dx];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int Dy = -1; Dy <= 1; ++Dy)
#pragma unroll
    for (int Dx = -1; Dx <= 1; ++Dx) {
        const int o = op9_slot(Dy, Dx);
        Lanes<T> out;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const long J = cc.col + k;
            const bool ring = (Dy < 0 && I == 1) || (Dy > 0 && I == NC - 1) || (Dx < 0 && J == 1) || (Dx > 0 && J == NC - 1);
            out.a[k] = ring ? (T)0 : acc[o][k];
        }
        V ov = from_lanes(out);
        mask_cols(ov, cc.col, NC);
        vstore<V>(c.a[o] + (long)I * cpitch + cc.col, ov, cc.st);
    }
}

// c P^T f at one coarse point: r0 / r1 / r2 the three fine values (west, centre, east) of the rows 2I - 1, 2I, 2I + 1, w the
// eight weights of the coarse point in slot order (k_restrict_opdep and the one-workgroup visit of mgx_small.hpp)
template <typename T>
__device__ __forceinline__ T opdep_restrict_value(const T (&w)[8], const T (&r0)[3], const T (&r1)[3], const T (&r2)[3], T rscale)
{
    T acc = w[4] * r0[0];
    acc = acc + w[0] * r0[1];
    acc = acc + w[5] * r0[2];
    acc = acc + w[2] * r1[0];
    acc = acc + r1[1];
    acc = acc + w[3] * r1[2];
    acc = acc + w[6] * r2[0];
    acc = acc + w[1] * r2[1];
    acc = acc + w[7] * r2[2];
    return rscale * acc;
}
// P e between two coarse points (west then east, north then south) and at a cell centre ((NW + NE) + SW) + SE; every
// argument pair: the weight of a coarse point towards the fine point, and that point's e
template <typename T> __device__ __forceinline__ T opdep_prolong_edge(T wa, T ea, T wb, T eb) { return wa * ea + wb * eb; }
template <typename T>
__device__ __forceinline__ T opdep_prolong_centre(T w0, T e0, T w1, T e1, T w2, T e2, T w3, T e3)   // the coarse points NW, NE, SW, SE of the centre
{
    T acc = w0 * e0 + w1 * e1;
    acc = acc + w2 * e2;
    return acc + w3 * e3;
}

// MODE 0: f = b;  1: f = b - A u, five-point A (slots 0..4 of a);  2: nine-point A
template <typename T, int MODE>
__global__ void __launch_bounds__(kBlock)
k_restrict_opdep(const T* __restrict__ u, const T* __restrict__ b, Op9<T> a, Wt8<T> w, T* __restrict__ cb, T* __restrict__ czero,
                 int NC, long fpitch, long cpitch, int strips, T rscale)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    constexpr int NQ = MODE == 2 ? 9 : 5;
    const Tile t = wave_tile(strips, NC - 1);
    if (!t.active) return;
    const Cols cc = lane_cols<W>(t.strip, NC, cpitch);
    const int I = 1 + t.chunk;
    const long fcol = 2 * cc.col;
    const bool ld0 = cc.ld && fcol + W <= fpitch, ld1 = cc.ld && fcol + 2 * W <= fpitch;
    // r[1 + iy][1 + m]: the field at fine (2I + iy, 2 col + m), m = -1 .. 2W - 1
    T r[3][2 * W + 1];
    if constexpr (MODE == 0) {
#pragma unroll
        for (int iy = -1; iy <= 1; ++iy) load_fine<T>(b + (long)(2 * I + iy) * fpitch + fcol, ld0, ld1, r[1 + iy]);
    } else {
        // u rows 2I - 2 .. 2I + 2 (all inside the grid: 1 <= I <= NC - 1), two vectors each
        V u0[5], u1[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const long at = (long)(2 * I - 2 + j) * fpitch + fcol;
            u0[j] = vload<V>(u + at, ld0);
            u1[j] = vload<V>(u + at + W, ld1);
        }
#pragma unroll
        for (int iy = -1; iy <= 1; ++iy) {
            const long at = (long)(2 * I + iy) * fpitch + fcol;
            const int j = 2 + iy;
            Lanes<T> k0[9], k1[9];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                k0[q] = to_lanes(vload<V>(a.a[q] + at, ld0));
                k1[q] = to_lanes(vload<V>(a.a[q] + at + W, ld1));
            }
            const Lanes<T> b0 = to_lanes(vload<V>(b + at, ld0)), b1 = to_lanes(vload<V>(b + at + W, ld1));
            // neighbours across the vector seams: vector 0's left is the left lane's vector 1, vector 1's right the
            // right lane's vector 0
            const Rows3<T> w0{to_lanes(u0[j - 1]), to_lanes(u0[j]), to_lanes(u0[j + 1]),
                              from_left(last(u1[j - 1])), first(u1[j - 1]), from_left(last(u1[j])), first(u1[j]),
                              from_left(last(u1[j + 1])), first(u1[j + 1])};
            const Rows3<T> w1{to_lanes(u1[j - 1]), to_lanes(u1[j]), to_lanes(u1[j + 1]),
                              last(u0[j - 1]), from_right(first(u0[j - 1])), last(u0[j]), from_right(first(u0[j])),
                              last(u0[j + 1]), from_right(first(u0[j + 1]))};
            const Lanes<T> av0 = stencil_sum<NQ>(w0, k0, [&](int k) { return k0[0].a[k]; });
            const Lanes<T> av1 = stencil_sum<NQ>(w1, k1, [&](int k) { return k1[0].a[k]; });
            Lanes<T> r1;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                r[1 + iy][1 + k] = b0.a[k] - av0.a[k];
                r1.a[k] = b1.a[k] - av1.a[k];
                r[1 + iy][1 + W + k] = r1.a[k];
            }
            r[1 + iy][0] = from_left(r1.a[W - 1]);
        }
    }
    Lanes<T> wv[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) wv[x] = to_lanes(vload<V>(w.w[x] + (long)I * cpitch + cc.col, cc.ld));
    Lanes<T> o;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int m = 1 + 2 * k;
        const T wk[8] = {wv[0].a[k], wv[1].a[k], wv[2].a[k], wv[3].a[k], wv[4].a[k], wv[5].a[k], wv[6].a[k], wv[7].a[k]};
        const T r0[3] = {r[0][m - 1], r[0][m], r[0][m + 1]}, r1[3] = {r[1][m - 1], r[1][m], r[1][m + 1]}, r2[3] = {r[2][m - 1], r[2][m], r[2][m + 1]};
        o.a[k] = opdep_restrict_value(wk, r0, r1, r2, rscale);
    }
    V ov = from_lanes(o);
    mask_cols(ov, cc.col, NC);
    vstore<V>(cb + (long)I * cpitch + cc.col, ov, cc.st);
    if (czero) vstore<V>(czero + (long)I * cpitch + cc.col, vzero((V*)nullptr), cc.st);
}

// on K columns (mgx_var.hpp, COLUMNS): the weights read once; a column's loads of v (ADD) follow the stores of the columns
// before it, which no column's e or weights alias
template <typename T, bool ADD, int K>
__global__ void __launch_bounds__(kBlock)
k_prolong_opdep(MultiOut<T, K> v, MultiIn<T, K> e, Wt8<T> w, int NC, long fpitch, long cpitch, int strips)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    const Tile t = wave_tile(strips, NC);
    if (!t.active) return;
    const Cols cc = lane_cols<W>(t.strip, NC, cpitch);
    const int I = t.chunk;                                    // 0 .. NC - 1: fine rows 2I (not the ring row 0) and 2I + 1
    const long fcol = 2 * cc.col;
    const bool st0 = cc.st && fcol + W <= fpitch, st1 = cc.st && fcol + 2 * W <= fpitch;
    const int NF = 2 * NC;
    const long c0 = (long)I * cpitch + cc.col, c1 = c0 + cpitch;
    // x[1 + m]: coarse column col + m
    T e0[K][W + 2], e1[K][W + 2];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        load_coarse<T>(e.p[j] + c0, cc.ld, e0[j]);
        load_coarse<T>(e.p[j] + c1, cc.ld, e1[j]);
    }
    T we[W + 2], ww[W + 2], ws[W + 2], wse[W + 2], wsw[W + 2], wn[W + 2], wne[W + 2], wnw[W + 2];
    load_coarse<T>(w.w[3] + c0, cc.ld, we);
    load_coarse<T>(w.w[2] + c0, cc.ld, ww);
    load_coarse<T>(w.w[1] + c0, cc.ld, ws);
    load_coarse<T>(w.w[7] + c0, cc.ld, wse);
    load_coarse<T>(w.w[6] + c0, cc.ld, wsw);
    load_coarse<T>(w.w[0] + c1, cc.ld, wn);
    load_coarse<T>(w.w[5] + c1, cc.ld, wne);
    load_coarse<T>(w.w[4] + c1, cc.ld, wnw);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        T f[2 * W], g[2 * W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int m = 1 + k;
            f[2 * k] = e0[j][m];
            f[2 * k + 1] = opdep_prolong_edge(we[m], e0[j][m], ww[m + 1], e0[j][m + 1]);
            g[2 * k] = opdep_prolong_edge(ws[m], e0[j][m], wn[m], e1[j][m]);
            // the cell centre south-east of coarse (I, col + k): its NW / NE / SW / SE coarse points
            g[2 * k + 1] = opdep_prolong_centre(wse[m], e0[j][m], wsw[m + 1], e0[j][m + 1], wne[m], e1[j][m], wnw[m + 1], e1[j][m + 1]);
        }
        auto put = [&](const T* x, int row) {
            Lanes<T> a0, a1;
#pragma unroll
            for (int k = 0; k < W; ++k) { a0.a[k] = x[k]; a1.a[k] = x[W + k]; }
            V v0 = from_lanes(a0), v1 = from_lanes(a1);
            mask_cols(v0, fcol, NF);
            mask_cols(v1, fcol + W, NF);
            T* p = v.p[j] + (long)row * fpitch + fcol;
            if (ADD) {
                const Lanes<T> o0 = to_lanes(vload<V>(p, st0)), o1 = to_lanes(vload<V>(p + W, st1));
                const Lanes<T> n0 = to_lanes(v0), n1 = to_lanes(v1);
                Lanes<T> s0, s1;
#pragma unroll
                for (int k = 0; k < W; ++k) { s0.a[k] = o0.a[k] + n0.a[k]; s1.a[k] = o1.a[k] + n1.a[k]; }
                v0 = from_lanes(s0); v1 = from_lanes(s1);
            }
            vstore<V>(p, v0, st0);
            vstore<V>(p + W, v1, st1);
        };
        if (I > 0) put(f, 2 * I);
        put(g, 2 * I + 1);
    }
}

// v_j += P e_j (add) or v_j = P e_j on m = 1 .. kMultiMax columns (host arrays of m pointers), NC the coarse level's N.
// (Only mgx_solve's FMG launches !add, on one column; the K > 1 forms of it are what a multi-column FMG would launch)
template <typename T>
void launch_prolong_opdep(int m, bool add, T* const* v, const T* const* e, const Wt8<T>& w, int NC, long fpitch, long cpitch, hipStream_t st)
{
    const Launch g = make_launch(NC, VecOf<T>::W, NC, 1);
    with_count<kMultiMax>(m, [&](auto kc) {
        constexpr int K = decltype(kc)::value;
        if (add) hipLaunchKernelGGL((k_prolong_opdep<T, true, K>), dim3(g.blocks), dim3(kBlock), 0, st, columns_out<K>(v), columns_in<K>(e), w, NC,
                                    fpitch, cpitch, g.strips);
        else hipLaunchKernelGGL((k_prolong_opdep<T, false, K>), dim3(g.blocks), dim3(kBlock), 0, st, columns_out<K>(v), columns_in<K>(e), w, NC,
                                fpitch, cpitch, g.strips);
    });
}

} // namespace mgx
