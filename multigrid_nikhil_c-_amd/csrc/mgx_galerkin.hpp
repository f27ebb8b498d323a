// mgx_galerkin.hpp - the variational hierarchy of a general five-point operator (cfg.op = MGX_OPERATOR_GALERKIN):
// A_{l-1} = R A_l P with P the bilinear prolongation (k_prolong) and R the handle's own full weighting
// (CONSISTENT: R = P^T, weights 1, 1/2, 1/4; FW16: R = P^T / 4).  R A P of a five-point operator is a NINE-point
// operator, so every level below the finest carries nine coefficient grids and the nine-point forms of the
// kernels of mgx_var.hpp.  Storage order of an operator's grids: c, n, s, w, e, nw, ne, sw, se (slots 0..8).
//
// k_galerkin_rap - for the coarse node I and the offset D in {-1,0,1}^2
//     A_c(I, I+D) = sum_i sum_d R(I, i) A_f(i, i+d) P(i+d, I+D),     i in 2I + {-1,0,1}^2,  d in {-1,0,1}^2,
//     P(j, J) = (1 - |j_y - 2J_y|/2)(1 - |j_x - 2J_x|/2) where both factors are positive, else 0;  R(I, i) = r P(i, I).
//   SUMMATION ORDER (tests/galerkin_ref.py follows it term by term): the accumulator starts at +0; outer loop: the
//   fine point i row-major over the 3 x 3 patch (i_y - 2I_y = -1, 0, 1; inside it i_x - 2I_x = -1, 0, 1); inner loop: d
//   row-major (NW, N, NE, W, C, E, SW, S, SE); pairs whose P(i+d, I+D) is structurally zero (an offset of i + d - 2(I+D)
//   outside {-1,0,1}) are skipped; each term is  w * A_f(i, i+d)  with the exact power of two w = r P(i, I) P(i+d, I+D),
//   added as its own IEEE operation (-ffp-contract=off).  An offset D that points at the eliminated Dirichlet ring
//   (I + D on row / column 0 or NC) gets the coefficient 0: such coefficients are ignored anyway (as for STENCIL5) and
//   a zero keeps the nine-point sums free of whatever the caller's finest operator holds there.
//   All weights are powers of two, so CONSISTENT and FW16 give operators that differ by an exact factor 4 per level.
//
// k_jacobi_var9 / k_residual_var9 - MF's sweep v' = R_omega v + omega (D_inv b) and r = b - A v for nine-point
//   operators, in the geometry of k_jacobi_var / k_residual_var (one wave per row and strip, 16-byte lanes, the
//   neighbours of all three rows from the adjacent lanes by DPP).  Sums in the CSR column order of a row-major
//   nine-point operator: NW, N, NE, W, C, E, SW, S, SE.
//   Roofline: v, b, D_inv and eight R grids in, v' out: 12 sizeof(T) per point and sweep; v, b and nine A grids in,
//   r out: 12 sizeof(T) per point for the residual.  HBM-bound single passes like their five-point forms.
#pragma once

#include "mgx_var.hpp"

namespace mgx {

template <typename T> struct Op9 { const T* a[9]; };     // c, n, s, w, e, nw, ne, sw, se (corners may be null)
template <typename T> struct Op9Out { T* a[9]; };

// storage slot of the coefficient that points at (dy, dx)
__host__ __device__ constexpr int op9_slot(int dy, int dx)
{
    return dy < 0 ? (dx < 0 ? 5 : dx == 0 ? 1 : 6) : dy == 0 ? (dx < 0 ? 3 : dx == 0 ? 0 : 4) : (dx < 0 ? 7 : dx == 0 ? 2 : 8);
}
__host__ __device__ constexpr int iabs(int x) { return x < 0 ? -x : x; }

// one coarse row per wave and strip; each lane owns W coarse points and reads the 2W + 1 fine columns under them as
// two 16-byte vectors plus the last element of its left neighbour's second vector.  CORNERS: the fine operator has
// corner grids (false on the finest level: slots 5..8 are not read)
template <typename T, bool CORNERS>
__global__ void __launch_bounds__(kBlock)
k_galerkin_rap(Op9<T> f, Op9Out<T> c, int NC, long fpitch, long cpitch, int strips, T rscale)
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
    T acc[9][W];
#pragma unroll
    for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[q][k] = (T)0;
#pragma unroll
    for (int iy = -1; iy <= 1; ++iy) {
        // fv[q][1 + m]: coefficient q of the fine row 2I + iy at fine column 2 col + m, m = -1 .. 2W - 1
        T fv[NQ][2 * W + 1];
        const long at = (long)(2 * I + iy) * fpitch + fcol;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const V v0 = vload<V>(f.a[q] + at, ld0);
            const V v1 = vload<V>(f.a[q] + at + W, ld1);
            const Lanes<T> l0 = to_lanes(v0), l1 = to_lanes(v1);
            fv[q][0] = from_left(last(v1));
#pragma unroll
            for (int k = 0; k < W; ++k) { fv[q][1 + k] = l0.a[k]; fv[q][1 + W + k] = l1.a[k]; }
        }
#pragma unroll
        for (int ix = -1; ix <= 1; ++ix) {
            const float wr = (1.f - 0.5f * iabs(iy)) * (1.f - 0.5f * iabs(ix));          // P(i, I)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int q = op9_slot(dy, dx);
                if (q >= NQ) continue;
#pragma unroll
                for (int Dy = -1; Dy <= 1; ++Dy)
#pragma unroll
                for (int Dx = -1; Dx <= 1; ++Dx) {
                    const int oy = iy + dy - 2 * Dy, ox = ix + dx - 2 * Dx;                // i + d relative to 2 (I + D)
                    if (iabs(oy) > 1 || iabs(ox) > 1) continue;
                    const float wp = (1.f - 0.5f * iabs(oy)) * (1.f - 0.5f * iabs(ox));   // P(i + d, I + D)
                    const T w = rscale * (T)(wr * wp);
                    const int o = op9_slot(Dy, Dx);
#pragma unroll
                    for (int k = 0; k < W; ++k) acc[o][k] = acc[o][k] + w * fv[q][1 + 2 * k + ix];
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

// sum_k coef_k * neighbour_k in CSR column order NW, N, NE, W, C, E, SW, S, SE.  xl / xr: the element left of the
// lane's first / right of its last column in row x (u = up, c = current, d = down)
template <typename T, typename CF>
__device__ __forceinline__ Lanes<T> stencil9(const Lanes<T>& up, const Lanes<T>& cur, const Lanes<T>& dn, T ul, T ur, T cl, T cr, T dl, T dr,
                                             const Lanes<T>& cnw, const Lanes<T>& cn, const Lanes<T>& cne, const Lanes<T>& cw, CF centre,
                                             const Lanes<T>& ce, const Lanes<T>& csw, const Lanes<T>& cs, const Lanes<T>& cse)
{
    constexpr int W = VecOf<T>::W;
    Lanes<T> o;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const bool first_k = (k == 0), last_k = (k == W - 1);
        T acc = cnw.a[k] * (first_k ? ul : up.a[first_k ? 0 : k - 1]);
        acc = acc + cn.a[k] * up.a[k];
        acc = acc + cne.a[k] * (last_k ? ur : up.a[last_k ? k : k + 1]);
        acc = acc + cw.a[k] * (first_k ? cl : cur.a[first_k ? 0 : k - 1]);
        acc = acc + centre(k) * cur.a[k];
        acc = acc + ce.a[k] * (last_k ? cr : cur.a[last_k ? k : k + 1]);
        acc = acc + csw.a[k] * (first_k ? dl : dn.a[first_k ? 0 : k - 1]);
        acc = acc + cs.a[k] * dn.a[k];
        acc = acc + cse.a[k] * (last_k ? dr : dn.a[last_k ? k : k + 1]);
        o.a[k] = acc;
    }
    return o;
}

// one sweep of v' = R_omega v + omega (D_inv b), out of place; rows [row_lo, row_hi).  r: the eight off-diagonals of
// R_omega in slots 1..8 (slot 0 unused: its diagonal is the scalar rc = 1 - omega)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_jacobi_var9(const T* __restrict__ vin, const T* __restrict__ rhs, T* __restrict__ vout, const T* __restrict__ dinv, Op9<T> r,
              int N, long pitch, int row_lo, int row_hi, int strips, T rc, T omega, int rows_alloc)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    const Tile t = wave_tile(strips, row_hi - row_lo);
    if (!t.active) return;
    const Cols c = lane_cols<W>(t.strip, N, pitch);
    const int row = row_lo + t.chunk;
    const long at = c.col + (long)row * pitch;
    const bool in = c.ld && row >= 0 && row < rows_alloc;
    const V up = vload<V>(vin + at - pitch, c.ld && row >= 1 && row <= rows_alloc);
    const V cur = vload<V>(vin + at, in);
    const V dn = vload<V>(vin + at + pitch, c.ld && row >= -1 && row + 1 < rows_alloc);
    const V bb = vload<V>(rhs + at, in);
    const V dv = vload<V>(dinv + at, in);
    Lanes<T> k9[9];
#pragma unroll
    for (int q = 1; q < 9; ++q) k9[q] = to_lanes(vload<V>(r.a[q] + at, in));
    const T ul = from_left(last(up)), ur = from_right(first(up));
    const T cl = from_left(last(cur)), cr = from_right(first(cur));
    const T dl = from_left(last(dn)), dr = from_right(first(dn));
    const Lanes<T> p1 = stencil9<T>(to_lanes(up), to_lanes(cur), to_lanes(dn), ul, ur, cl, cr, dl, dr, k9[5], k9[1], k9[6], k9[3],
                                    [&](int) { return rc; }, k9[4], k9[7], k9[2], k9[8]);
    const Lanes<T> b = to_lanes(bb), d = to_lanes(dv);
    Lanes<T> o;
#pragma unroll
    for (int k = 0; k < W; ++k) o.a[k] = p1.a[k] + omega * (d.a[k] * b.a[k]);
    V ov = from_lanes(o);
    mask_cols(ov, c.col, N);
    vstore<V>(vout + at, ov, c.st && in);
}

// r = b - A v for a nine-point A.  MODE 0: store r;  MODE 1: per-block sums of r^2
template <typename T, int MODE>
__global__ void __launch_bounds__(kBlock)
k_residual_var9(const T* __restrict__ vin, const T* __restrict__ rhs, T* __restrict__ out, double* __restrict__ partial, Op9<T> a,
                int N, long pitch, int row_lo, int row_hi, int strips, int rows_alloc)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[kWavesPerBlock];
    const Tile t = wave_tile(strips, row_hi - row_lo);
    double acc = 0.0;
    if (t.active) {
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int row = row_lo + t.chunk;
        const long at = c.col + (long)row * pitch;
        const bool in = c.ld && row >= 0 && row < rows_alloc;
        const V up = vload<V>(vin + at - pitch, c.ld && row >= 1 && row <= rows_alloc);
        const V cur = vload<V>(vin + at, in);
        const V dn = vload<V>(vin + at + pitch, c.ld && row >= -1 && row + 1 < rows_alloc);
        const Lanes<T> b = to_lanes(vload<V>(rhs + at, in));
        Lanes<T> k9[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) k9[q] = to_lanes(vload<V>(a.a[q] + at, in));
        const T ul = from_left(last(up)), ur = from_right(first(up));
        const T cl = from_left(last(cur)), cr = from_right(first(cur));
        const T dl = from_left(last(dn)), dr = from_right(first(dn));
        const Lanes<T> av = stencil9<T>(to_lanes(up), to_lanes(cur), to_lanes(dn), ul, ur, cl, cr, dl, dr, k9[5], k9[1], k9[6], k9[3],
                                        [&](int k) { return k9[0].a[k]; }, k9[4], k9[7], k9[2], k9[8]);
        Lanes<T> o;
#pragma unroll
        for (int k = 0; k < W; ++k) o.a[k] = b.a[k] - av.a[k];
        V ov = from_lanes(o);
        mask_cols(ov, c.col, N);
        if (MODE == 0) {
            vstore<V>(out + at, ov, c.st && in);
        } else if (c.st && in) {
            const Lanes<T> q = to_lanes(ov);
            if constexpr (W == 2) acc = (double)q.a[0] * (double)q.a[0] + (double)q.a[1] * (double)q.a[1];
            else acc = ((double)q.a[0] * (double)q.a[0] + (double)q.a[1] * (double)q.a[1]) +
                       ((double)q.a[2] * (double)q.a[2] + (double)q.a[3] * (double)q.a[3]);
        }
    }
    if (MODE != 0) {
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double sum = 0.0;
            for (int w2 = 0; w2 < kWavesPerBlock; ++w2) sum += wsum[w2];
            partial[blockIdx.x] = sum;
        }
    }
}

// the Jacobi splitting of a nine-point operator: D_inv = 1 / c, R_x = -(omega (D_inv a_x)) for the eight
// off-diagonals (slots 1..8 of r); the diagonal of R_omega is 1 - omega exactly and is not stored
template <typename T>
__global__ void k_var_build_jacobi9(Op9<T> a, T* __restrict__ dinv, Op9Out<T> r, int N, long pitch, T omega)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = blockIdx.y;
    if (c < 1 || c >= N || row < 1 || row >= N) return;
    const long at = (long)row * pitch + c;
    const T d = (T)1 / a.a[0][at];
    dinv[at] = d;
#pragma unroll
    for (int q = 1; q < 9; ++q) r.a[q][at] = -(omega * (d * a.a[q][at]));
}

// the coarsest nine-point operator as a dense matrix (and the identity next to it) for k_gj_prow / k_gj_elim
template <typename T>
__global__ void k_var_dense_fill9(double* __restrict__ M, double* __restrict__ Inv, Op9<T> a, int n, long pitch)
{
    const int NN = n * n;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;      // column
    const int k = blockIdx.y;                                  // row = unknown (ri, rj)
    if (j >= NN) return;
    const int ri = k / n, rj = k - ri * n;
    const int ci = j / n, cj = j - ci * n;
    const int dy = ci - ri, dx = cj - rj;
    double v = 0.0;
    if (dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) v = (double)a.a[op9_slot(dy, dx)][(long)(ri + 1) * pitch + (rj + 1)];
    M[(long)k * NN + j] = v;
    Inv[(long)k * NN + j] = (j == k) ? 1.0 : 0.0;
}

} // namespace mgx
