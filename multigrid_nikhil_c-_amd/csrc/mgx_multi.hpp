// mgx_multi.hpp - the two passes of the block solves that keep a K-column kernel of their own, K = 2, 3 or 4, next to a
// single-column one with another body.  Every other pass of mgx_solve_multi's cycle that reads an operator is the
// K-column kernel of its own header (mgx_var.hpp: k_jacobi_var, k_residual_var, k_var_dense_solve; mgx_opdep.hpp:
// k_prolong_opdep; mgx_refine_gcr.hpp: k_refine_direction), whose K = 1 instance is the pass of mgx_solve; mgx_var.hpp
// (COLUMNS) has the traffic count, MultiIn / MultiOut and the load-before-store discipline that stands in for
// __restrict__.
//
//   k_restrict_opdep_multi   next to k_restrict_opdep (mgx_opdep.hpp), which loads five u rows once and keeps three
//                            residual rows live; this one walks the fine rows one at a time so that K = 3, 4 do not spill
//   k_gcr_direction_multi    next to k_pcg_direction (mgx_krylov.hpp), which also forms the partials of p.q
//
// Per column the arithmetic and its order are those of the single-column kernel - the same helpers (stencil_sum, the
// row-major nine-term sum of opdep_restrict_value), the same launch geometry - so a column's iterate has the bits
// mgx_solve gives it, however the columns are grouped into launches.
#pragma once

#include "mgx_opdep.hpp"

namespace mgx {

// k_restrict_opdep on K columns: cb_j = c P^T f_j, f_j = b_j (MODE 0) or b_j - A u_j formed in registers (MODE 1: five-
// point A, MODE 2: nine-point A); czero.p[j] (all null or none) is zeroed.  The eight weights of the coarse point are
// read once, and each fine row's coefficients once for the K columns.  The sum of opdep_restrict_value is taken row by
// row - the same nine terms in the same order (NW, N, NE, W, C, E, SW, S, SE, the first starting the accumulator, the
// centre unmultiplied), then one multiplication by c - so that only one fine row of residuals is live per column.
// (mgx_solve_multi instantiates MODE 1 and 2 only: it has no FMG.  MODE 0 is the form a multi-column FMG would launch)
template <typename T, int MODE, int K>
__global__ void __launch_bounds__(kBlock)
k_restrict_opdep_multi(MultiIn<T, K> u, MultiIn<T, K> b, Op9<T> a, Wt8<T> w, MultiOut<T, K> cb, MultiOut<T, K> czero,
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
    auto weight = [&](int x) { return to_lanes(vload<V>(w.w[x] + (long)I * cpitch + cc.col, cc.ld)); };
    T acc[K][W];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[j][k] = (T)0;         // (the first term of the first row replaces it)
    // not unrolled: one fine row's loads and residuals are live at a time (unrolled, the three rows' loads are hoisted
    // together and the K = 3, 4 instances spill).  The branches on iy are uniform; every array index in them is a constant
#pragma unroll 1
    for (int iy = -1; iy <= 1; ++iy) {
        const long at = (long)(2 * I + iy) * fpitch + fcol;
        // the weights towards the fine row's west, centre and east points (the coincident weight is 1: not stored)
        Lanes<T> ww, wm, we;
        if (iy < 0) { ww = weight(4); wm = weight(0); we = weight(5); }
        else if (iy == 0) { ww = weight(2); we = weight(3); wm = ww; }
        else { ww = weight(6); wm = weight(1); we = weight(7); }
        // r[j][1 + m]: the field of column j at fine (2I + iy, 2 col + m), m = -1 .. 2W - 1
        T r[K][2 * W + 1];
        if constexpr (MODE == 0) {
#pragma unroll
            for (int j = 0; j < K; ++j) load_fine<T>(b.p[j] + at, ld0, ld1, r[j]);
        } else {
            // u rows 2I + iy - 1 .. 2I + iy + 1 (all inside the grid: 1 <= I <= NC - 1), two vectors each
            V u0[K][3], u1[K][3];
            Lanes<T> b0[K], b1[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    u0[j][d] = vload<V>(u.p[j] + at + (long)(d - 1) * fpitch, ld0);
                    u1[j][d] = vload<V>(u.p[j] + at + (long)(d - 1) * fpitch + W, ld1);
                }
                b0[j] = to_lanes(vload<V>(b.p[j] + at, ld0));
                b1[j] = to_lanes(vload<V>(b.p[j] + at + W, ld1));
            }
            Lanes<T> k0[9], k1[9];
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                k0[q] = to_lanes(vload<V>(a.a[q] + at, ld0));
                k1[q] = to_lanes(vload<V>(a.a[q] + at + W, ld1));
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                // neighbours across the vector seams: vector 0's left is the left lane's vector 1, vector 1's right
                // the right lane's vector 0
                const Rows3<T> w0{to_lanes(u0[j][0]), to_lanes(u0[j][1]), to_lanes(u0[j][2]),
                                  from_left(last(u1[j][0])), first(u1[j][0]), from_left(last(u1[j][1])), first(u1[j][1]),
                                  from_left(last(u1[j][2])), first(u1[j][2])};
                const Rows3<T> w1{to_lanes(u1[j][0]), to_lanes(u1[j][1]), to_lanes(u1[j][2]),
                                  last(u0[j][0]), from_right(first(u0[j][0])), last(u0[j][1]), from_right(first(u0[j][1])),
                                  last(u0[j][2]), from_right(first(u0[j][2]))};
                const Lanes<T> av0 = stencil_sum<NQ>(w0, k0, [&](int k) { return k0[0].a[k]; });
                const Lanes<T> av1 = stencil_sum<NQ>(w1, k1, [&](int k) { return k1[0].a[k]; });
                Lanes<T> r1;
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    r[j][1 + k] = b0[j].a[k] - av0.a[k];
                    r1.a[k] = b1[j].a[k] - av1.a[k];
                    r[j][1 + W + k] = r1.a[k];
                }
                r[j][0] = from_left(r1.a[W - 1]);
            }
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int m = 1 + 2 * k;
                const T west = ww.a[k] * r[j][m - 1];
                T s = iy < 0 ? west : acc[j][k] + west;
                s = s + (iy == 0 ? r[j][m] : wm.a[k] * r[j][m]);
                acc[j][k] = s + we.a[k] * r[j][m + 1];
            }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        Lanes<T> o;
#pragma unroll
        for (int k = 0; k < W; ++k) o.a[k] = rscale * acc[j][k];
        V ov = from_lanes(o);
        mask_cols(ov, cc.col, NC);
        vstore<V>(cb.p[j] + (long)I * cpitch + cc.col, ov, cc.st);
        if (czero.p[j]) vstore<V>(czero.p[j] + (long)I * cpitch + cc.col, vzero((V*)nullptr), cc.st);
    }
}

// ---- mgx_solve_multi_gcr ------------------------------------------------------------------------------------------
// The direction pass of GCR on K columns: Z_j = z_j, Q_j = A z_j - the first_it = 1 form of k_pcg_direction<T, 1 | 2>
// (mgx_krylov.hpp) with the level's NQ coefficient grids loaded once per row for the K columns: (NQ + 3K) sizeof(T) per
// point against K (NQ + 3).  The same march down R rows per wave, the same prow masking, the same edge hand-up for
// NQ = 9, stencil_sum<NQ> with the same centre-coefficient lambda and mask_cols before the stores: per column the
// arithmetic and its order are the single-column kernel's, whatever R is.  No partial sums: GCR never reads
// k_pcg_direction's p'.q.  A wave without a tile returns at once (nothing below synchronises the workgroup).
template <typename T, int NQ, int K>
__global__ void __launch_bounds__(kBlock)
k_gcr_direction_multi(MultiIn<T, K> z, MultiOut<T, K> zo, MultiOut<T, K> q, Op9<T> a, int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    const Tile t = wave_tile(strips, chunks);
    if (!t.active) return;
    const Cols c = lane_cols<VecOf<T>::W>(t.strip, N, pitch);
    const int r0 = 1 + t.chunk * R;
    const int r1 = min(r0 + R, N);
    // rows 0 and N are the Dirichlet ring: z = 0 there without a load
    auto prow = [&](const T* zp, int y) -> V {
        const bool in = c.ld && y >= 1 && y < N;
        V v = vload<V>(zp + c.col + (long)y * pitch, in);
        mask_cols(v, c.col, N);
        return v;
    };
    V up[K], cur[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { up[j] = prow(z.p[j], r0 - 1); cur[j] = prow(z.p[j], r0); }
    // the edge values of the rows above and at y from the adjacent lanes: NQ = 9 hands those of row y + 1 up as the march
    // goes down (two moves per new row and column), NQ = 5 needs those of row y only
    T ul[K], ur[K], cl[K], cr[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        ul[j] = ur[j] = (T)0;
        if constexpr (NQ == 9) { ul[j] = from_left(last(up[j])); ur[j] = from_right(first(up[j])); }
        cl[j] = from_left(last(cur[j])); cr[j] = from_right(first(cur[j]));
    }
    for (int y = r0; y < r1; ++y) {
        const long at = c.col + (long)y * pitch;
        V dn[K];
#pragma unroll
        for (int j = 0; j < K; ++j) dn[j] = prow(z.p[j], y + 1);
        Lanes<T> k[9];
        load_coefs<NQ, 0>(a, at, c.ld, k);
        V o[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const T dl = from_left(last(dn[j])), dr = from_right(first(dn[j]));
            const Rows3<T> u{to_lanes(up[j]), to_lanes(cur[j]), to_lanes(dn[j]), ul[j], ur[j], cl[j], cr[j], dl, dr};
            o[j] = from_lanes(stencil_sum<NQ>(u, k, [&](int x) { return k[0].a[x]; }));
            mask_cols(o[j], c.col, N);
            ul[j] = cl[j]; ur[j] = cr[j]; cl[j] = dl; cr[j] = dr;
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            vstore<V>(zo.p[j] + at, cur[j], c.st);
            vstore<V>(q.p[j] + at, o[j], c.st);
            up[j] = cur[j]; cur[j] = dn[j];
        }
    }
}

// one launch of k_gcr_direction_multi on m = 2 .. 4 columns (host arrays of m pointers) of a five- or nine-point level
template <typename T>
void launch_gcr_direction_multi(int m, bool nine, const T* const* z, T* const* zo, T* const* q, const Op9<T>& a, int N, long pitch,
                                const Launch& g, hipStream_t st)
{
    with_point_count(nine, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        with_count<kMultiMax, 2>(m, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            hipLaunchKernelGGL((k_gcr_direction_multi<T, NQ, K>), dim3(g.blocks), dim3(kBlock), 0, st, columns_in<K>(z), columns_out<K>(zo),
                               columns_out<K>(q), a, N, pitch, g.R, g.strips, g.chunks);
        });
    });
}

// mgx.hip uses these instantiations; mgx_inst.hip (-DMGX_INST_KIND=9) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
extern template void launch_gcr_direction_multi<double>(int, bool, const double* const*, double* const*, double* const*, const Op9<double>&, int,
                                                        long, const Launch&, hipStream_t);
extern template void launch_gcr_direction_multi<float>(int, bool, const float* const*, float* const*, float* const*, const Op9<float>&, int, long,
                                                       const Launch&, hipStream_t);
#endif

} // namespace mgx
