// mgx_theta.hpp - the zero-order term of a finest GALERKIN operator and the right-hand side of a theta step (absent in
// the reference).  Two kernels on the finest level, both on top of mgx_var.hpp:
//
//   k_reaction_shift<T>            c = c0 + d on the interior points: slot 0 of S = A0 + diag(d), one rounding in T.
//                                  Set-up time only (mgx_set_reaction), one thread per point.
//   k_theta_rhs<T, NQ, EULER>      the right-hand side of one theta step of  M u_t + A0 u = f  on S = A0 + diag(d),
//                                  d = M / (theta dt):
//                                      S u+ = (1 / theta) d.u - ((1 - theta) / theta) S u + g.
//                                  Per point p, every product and sum rounded on its own in T (no contraction):
//                                      m = d_p * u_p
//                                      EULER (theta = 1):  b_p = m                          [+ g_p when g is given]
//                                      otherwise:          q = (S u)_p;  b_p = c1 * m - c0 * q   [+ g_p]
//                                  with c1 = (T)(1 / theta), c0 = (T)((1 - theta) / theta) formed in double by the host, and
//                                  q the sum stencil_sum forms for k_residual_var: CSR order, centre included, the
//                                  coefficients that point at the ring times the zero ring.
//
// Geometry: k_residual_var's - one wave per row and strip, 16-byte lanes, the x-neighbours from the adjacent lanes by
// DPP (load_rows, load_coefs, rows_of, stencil_sum, store_row).  The EULER instance reads no neighbour and no
// coefficient grid: the lane's own vector of u, d (and g) only, on the lanes that store.  Words per point: NQ + 3 in
// (u, d, g and the NQ grids of S) and 1 out - one more than k_residual_var<T, NQ, 0, 1> (u, b, NQ grids in, r out), the
// yardstick of tools/theta_bench.py; EULER 3 in and 1 out.  No atomics, no reductions, no LDS, no scratch.
// Ring and padding of the output are not touched: rows 1 .. N - 1 are written, columns 0 and >= N with zeros.
#pragma once

#include "mgx_var.hpp"

namespace mgx {

template <typename T>
__global__ void k_reaction_shift(const T* __restrict__ c0, const T* __restrict__ d, T* __restrict__ c, int N, long pitch)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (x < 1 || x >= N || r < 1 || r >= N) return;
    const long at = (long)r * pitch + x;
    c[at] = c0[at] + d[at];
}

template <typename T, int NQ, bool EULER>
__global__ void __launch_bounds__(kBlock)
k_theta_rhs(const T* __restrict__ u, const T* __restrict__ d, const T* __restrict__ g, T* __restrict__ out, Op9<T> a, int N, long pitch,
            int row_lo, int row_hi, int strips, int rows_alloc, T c1, T c0)
{
    constexpr int W = VecOf<T>::W;
    const bool has_g = g != nullptr;                          // (uniform; m + 0 is not m for m = -0)
    if constexpr (EULER) {
        using V = typename VecOf<T>::type;
        const Tile t = wave_tile(strips, row_hi - row_lo);
        if (!t.active) return;
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int row = row_lo + t.chunk;
        const long at = c.col + (long)row * pitch;
        const bool st = c.ld && c.st && row >= 0 && row < rows_alloc;
        const Lanes<T> uu = load_lanes(u + at, st), dd = load_lanes(d + at, st);
        Lanes<T> gg{};
        if (has_g) gg = load_lanes(g + at, st);
        Lanes<T> o;
#pragma unroll
        for (int x = 0; x < W; ++x) {
            o.a[x] = dd.a[x] * uu.a[x];
            if (has_g) o.a[x] = o.a[x] + gg.a[x];
        }
        V ov = from_lanes(o);
        mask_cols(ov, c.col, N);
        vstore<V>(out + at, ov, st);
    } else {
        const RowTile<T> t = load_rows<T>(u, N, pitch, row_lo, row_hi, strips, rows_alloc);
        if (!t.active) return;
        const Lanes<T> dd = load_lanes(d + t.at, t.in);
        Lanes<T> gg{};
        if (has_g) gg = load_lanes(g + t.at, t.in);
        Lanes<T> k[9];
        load_coefs<NQ, 0>(a, t.at, t.in, k);
        const Lanes<T> q = stencil_sum<NQ>(rows_of<NQ>(t), k, [&](int x) { return k[0].a[x]; });
        const Lanes<T> uu = to_lanes(t.cur);
        Lanes<T> o;
#pragma unroll
        for (int x = 0; x < W; ++x) {
            const T m = dd.a[x] * uu.a[x];
            o.a[x] = c1 * m - c0 * q.a[x];
            if (has_g) o.a[x] = o.a[x] + gg.a[x];
        }
        store_row(out, o, t, N);
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------
// c = c0 + d on the interior of a level
template <typename T>
void launch_reaction_shift(const T* c0, const T* d, T* c, int N, long pitch, hipStream_t st)
{
    hipLaunchKernelGGL(k_reaction_shift<T>, dim3((N + 1 + 255) / 256, N + 1), dim3(256), 0, st, c0, d, c, N, pitch);
}

// out = the right-hand side of one theta step from u, d, g (null: none) and the level's operator; theta = 1 is the EULER
// instance, which ignores v.a, c1 and c0
template <typename T>
void launch_theta_rhs(const VarLevel<T>& v, const T* u, const T* d, const T* g, T* out, double theta, hipStream_t st)
{
    const Launch gm = make_launch(v.N, VecOf<T>::W, v.N - 1, 1);
    const T c1 = (T)(1.0 / theta), c0 = (T)((1.0 - theta) / theta);
    const dim3 grd(gm.blocks), blk(kBlock);
    if (theta == 1.0) {
        hipLaunchKernelGGL((k_theta_rhs<T, 5, true>), grd, blk, 0, st, u, d, g, out, v.a, v.N, v.pitch, 1, v.N, gm.strips, v.rows, c1, c0);
        return;
    }
    with_point_count(v.nine, [&](auto nq) {
        hipLaunchKernelGGL((k_theta_rhs<T, decltype(nq)::value, false>), grd, blk, 0, st, u, d, g, out, v.a, v.N, v.pitch, 1, v.N, gm.strips,
                           v.rows, c1, c0);
    });
}

// mgx.hip uses these instantiations; mgx_inst.hip (-DMGX_INST_KIND=13) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
#define MGX_THETA_EXTERN(T)                                                                                          \
    extern template void launch_reaction_shift<T>(const T*, const T*, T*, int, long, hipStream_t);                   \
    extern template void launch_theta_rhs<T>(const VarLevel<T>&, const T*, const T*, const T*, T*, double, hipStream_t);
MGX_THETA_EXTERN(double)
MGX_THETA_EXTERN(float)
#undef MGX_THETA_EXTERN
#endif

} // namespace mgx
