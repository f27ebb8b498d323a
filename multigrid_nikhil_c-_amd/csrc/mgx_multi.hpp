// mgx_multi.hpp - the kernels of mgx_solve_multi: the passes of a general-operator cycle (mgx_var.hpp, mgx_opdep.hpp) on
// K = 2, 3 or 4 vectors at once.  Every pass of that cycle is bound by HBM traffic that is mostly coefficients: a Jacobi
// sweep moves (NQ + 3) sizeof(T) per point, of which 3 belong to the vector.  These kernels load an operator's
// coefficients (D_inv and R_omega, A, the eight transfer weights, the dense coarsest inverse) ONCE into registers and
// apply them to K columns, so a sweep moves (NQ + 3K) sizeof(T) per point instead of K (NQ + 3):
//     five-point, K = 4: 17 words against 32 (0.53);  nine-point, K = 4: 21 against 48 (0.44).
//
// K is a compile-time parameter; the column pointers arrive by value (MultiIn / MultiOut) and are indexed by unrolled
// constants only (a run-time index would put the arrays into scratch).  One active column runs the single-column kernel.
//
// Per column the arithmetic and its order are those of the single-column kernel - the same helpers (load_rows, rows_of,
// load_coefs, stencil_sum, jacobi_value, store_row, opdep_prolong_*), the same launch geometry
// (make_launch(N, W, N - 1, 1)), the same block of k_residual_var<T, NQ, 1> summing the same points in the same order -
// so a column's iterate and norm have the bits mgx_solve gives it, however the columns are grouped into launches.
//
// Load order: all K columns' row loads (3 K vectors), their right-hand sides and then the coefficients are issued before
// the first stencil_sum; nothing is stored before every load of the wave has been issued (the column pointers carry no
// __restrict__, so a store between two columns' loads would order them).
#pragma once

#include "mgx_opdep.hpp"

namespace mgx {

constexpr int kMultiMax = 4;                              // MGX_MAX_RHS

template <typename T, int K> struct MultiIn { const T* p[K]; };
template <typename T, int K> struct MultiOut { T* p[K]; };

// k_jacobi_var on K columns: v_j' = R_omega v_j + omega D^-1 b_j
template <typename T, int NQ, int K>
__global__ void __launch_bounds__(kBlock)
k_jacobi_var_multi(MultiIn<T, K> vin, MultiIn<T, K> rhs, MultiOut<T, K> vout, const T* __restrict__ dinv, Op9<T> r,
                   int N, long pitch, int row_lo, int row_hi, int strips, T rc, T omega, int rows_alloc)
{
    constexpr int W = VecOf<T>::W;
    RowTile<T> t[K];
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = load_rows<T>(vin.p[j], N, pitch, row_lo, row_hi, strips, rows_alloc);
    if (!t[0].active) return;
    Lanes<T> b[K];
#pragma unroll
    for (int j = 0; j < K; ++j) b[j] = load_lanes(rhs.p[j] + t[0].at, t[0].in);
    const Lanes<T> d = load_lanes(dinv + t[0].at, t[0].in);
    Lanes<T> k[9];
    load_coefs<NQ, 1>(r, t[0].at, t[0].in, k);
    Lanes<T> o[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const Lanes<T> p1 = stencil_sum<NQ>(rows_of<NQ>(t[j]), k, [&](int) { return rc; });
#pragma unroll
        for (int x = 0; x < W; ++x) o[j].a[x] = jacobi_value(p1.a[x], omega, d.a[x], b[j].a[x]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) store_row(vout.p[j], o[j], t[j], N);
}

// k_residual_var on K columns.  MODE 0: out.p[j] = b_j - A v_j;  MODE 1: partial.p[j][block] = the block's sum of r_j^2,
// block i of column j summing what block i of k_residual_var<T, NQ, 1> sums
template <typename T, int NQ, int MODE, int K>
__global__ void __launch_bounds__(kBlock)
k_residual_var_multi(MultiIn<T, K> vin, MultiIn<T, K> rhs, MultiOut<T, K> out, MultiOut<double, K> partial, Op9<T> a,
                     int N, long pitch, int row_lo, int row_hi, int strips, int rows_alloc)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[K][kWavesPerBlock];
    RowTile<T> t[K];
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = load_rows<T>(vin.p[j], N, pitch, row_lo, row_hi, strips, rows_alloc);
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    if (t[0].active) {
        Lanes<T> b[K];
#pragma unroll
        for (int j = 0; j < K; ++j) b[j] = load_lanes(rhs.p[j] + t[0].at, t[0].in);
        Lanes<T> k[9];
        load_coefs<NQ, 0>(a, t[0].at, t[0].in, k);
        V ov[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const Lanes<T> av = stencil_sum<NQ>(rows_of<NQ>(t[j]), k, [&](int x) { return k[0].a[x]; });
            Lanes<T> o;
#pragma unroll
            for (int x = 0; x < W; ++x) o.a[x] = b[j].a[x] - av.a[x];
            ov[j] = masked_row(o, t[j], N);
        }
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (MODE == 0) {
                vstore<V>(out.p[j] + t[j].at, ov[j], t[j].st);
            } else if (t[j].st) {
                const Lanes<T> q = to_lanes(ov[j]);
                if constexpr (W == 2) acc[j] = (double)q.a[0] * (double)q.a[0] + (double)q.a[1] * (double)q.a[1];
                else acc[j] = ((double)q.a[0] * (double)q.a[0] + (double)q.a[1] * (double)q.a[1]) +
                              ((double)q.a[2] * (double)q.a[2] + (double)q.a[3] * (double)q.a[3]);
            }
        }
    }
    if (MODE != 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) block_reduce<kWavesPerBlock>(acc[j], wsum[j], partial.p[j] + blockIdx.x, ReduceSum{});
    }
}

// k_restrict_opdep on K columns: cb_j = c P^T f_j, f_j = b_j (MODE 0) or b_j - A u_j formed in registers (MODE 1: five-
// point A, MODE 2: nine-point A); czero.p[j] (all null or none) is zeroed.  The eight weights of the coarse point are
// read once, and each fine row's coefficients once for the K columns.  The sum of opdep_restrict_value is taken row by
// row - the same nine terms in the same order (NW, N, NE, W, C, E, SW, S, SE, the first starting the accumulator, the
// centre unmultiplied), then one multiplication by c - so that only one fine row of residuals is live per column.
// (mgx_solve_multi instantiates MODE 1 and 2, and k_prolong_opdep_multi with ADD only: it has no FMG.  MODE 0 and !ADD are
// the forms a multi-column FMG would launch; no test runs them yet)
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

// k_prolong_opdep on K columns: v_j (+)= P e_j, the weights read once
template <typename T, bool ADD, int K>
__global__ void __launch_bounds__(kBlock)
k_prolong_opdep_multi(MultiOut<T, K> v, MultiIn<T, K> e, Wt8<T> w, int NC, long fpitch, long cpitch, int strips)
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

// k_var_dense_solve on K columns: x_j = Inv b_j, every element of Inv read once, each column's row sum in order
template <typename T, int K>
__global__ void k_var_dense_solve_multi(const double* __restrict__ Inv, MultiIn<T, K> b, MultiOut<T, K> x, int n, long pitch)
{
    const int NN = n * n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NN) return;
    const double* row = Inv + (long)i * NN;
    double acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = 0.0;
    for (int q = 0; q < NN; ++q) {
        const int bi = q / n, bj = q - bi * n;
        const double m = row[q];
        const long at = (long)(bi + 1) * pitch + (bj + 1);
#pragma unroll
        for (int j = 0; j < K; ++j) acc[j] += m * (double)b.p[j][at];
    }
    const int ri = i / n, rj = i - ri * n;
#pragma unroll
    for (int j = 0; j < K; ++j) x.p[j][(long)(ri + 1) * pitch + (rj + 1)] = (T)acc[j];
}

// f(tag) with decltype(tag)::value == 2, 3 or 4: the column count of a launch as a compile-time constant
template <typename F> void with_column_count(int k, F&& f)
{
    if (k == 2) f(std::integral_constant<int, 2>{});
    else if (k == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 4>{});
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
        with_column_count(m, [&](auto kc) {
            constexpr int K = decltype(kc)::value;
            MultiIn<T, K> zi;
            MultiOut<T, K> zz, qq;
            for (int j = 0; j < K; ++j) { zi.p[j] = z[j]; zz.p[j] = zo[j]; qq.p[j] = q[j]; }
            hipLaunchKernelGGL((k_gcr_direction_multi<T, NQ, K>), dim3(g.blocks), dim3(kBlock), 0, st, zi, zz, qq, a, N, pitch, g.R, g.strips,
                               g.chunks);
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
