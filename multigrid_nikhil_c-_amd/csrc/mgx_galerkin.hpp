// mgx_galerkin.hpp - the variational hierarchy of a general five- or nine-point operator (cfg.op = MGX_OPERATOR_GALERKIN):
// A_{l-1} = R A_l P with P the bilinear prolongation (k_prolong) and R the handle's own full weighting
// (CONSISTENT: R = P^T, weights 1, 1/2, 1/4; FW16: R = P^T / 4).  R A P of a five-point operator is a NINE-point
// operator, so every level below the finest carries nine coefficient grids and runs the NQ = 9 instances of the
// kernels of mgx_var.hpp (k_jacobi_var<T, 9>, k_residual_var<T, 9, MODE>, ...; slot and summation order: there).
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
#pragma once

#include "mgx_var.hpp"

namespace mgx {

__host__ __device__ constexpr int iabs(int x) { return x < 0 ? -x : x; }

// one coarse row per wave and strip; each lane owns W coarse points and reads the 2W + 1 fine columns under them as
// two 16-byte vectors plus the last element of its left neighbour's second vector.  CORNERS: the fine operator has
// corner grids (false on a five-point finest level: slots 5..8 are not read)
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

} // namespace mgx
