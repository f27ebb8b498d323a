// mgx_newton.hpp - the fused pass of mgx_newton (absent in the reference): one sweep over the finest
// level of a GALERKIN handle forms, for  F(u) = A0 u + kap phi(u) - f,  phi(u) = p1 u + p2 u^2 + p3 u^3:
//
//   k_newton_pass<T, NQ, STEP>     v   = u                       (STEP = false: the first evaluation)
//                                  v   = u + lam * de            (STEP = true: a trial of the line search; ut <- v)
//                                  q   = (A0 v)_p                stencil_sum's CSR-order sum, the centre from c0, the
//                                                                coefficients that point at the ring times the zero ring
//                                  ph  = ((p3 * v + p2) * v + p1) * v
//                                  dp  = (q3 * v + q2) * v + p1          q2 = (T)(2 p2), q3 = (T)(3 p3) by the host
//                                  b_p = f_p - (q + kap_p * ph)          the right-hand side -F(v) of the Newton step
//                                  d_p = kap_p * dp                      the zero-order term of the Jacobian A0 + diag(d)
//                                  partial[block] = the block's sum of b_p^2
//                                  every product and sum rounded on its own in T (no contraction).
//
// Geometry: k_theta_rhs's non-Euler branch - one wave per row and strip, 16-byte lanes, the x-neighbours from the
// adjacent lanes by DPP (load_rows, load_coefs, rows_of, stencil_sum, store_row).  The off-diagonals come from the
// level's A (slots 1 .. NQ - 1), the centre from c0: A's own slot 0 carries the term of the previous step.  STEP loads
// the three rows of u and of de and forms v for all three in registers (the ring rows and columns of both are zero, so
// v is zero there); rows_of is fed from the computed vectors; only the current row of ut is stored.  The squares are
// k_residual_var<T, NQ, 1, 1>'s: lane_squares of the masked row, block_reduce per workgroup of the same launch, then
// k_reduce_partials - the sum is bit for bit the one mgx_residual_norm forms from (U = 0, B = b).
// Every load of the wave comes before its first store (mgx_var.hpp, ALIASING).
// Words per point: NQ + 3 in (u, f, kap, c0, NQ - 1 grids of A) and 2 out (b, d) for STEP = false; NQ + 4 in (de) and 3
// out (ut) for STEP = true.  No LDS beyond the reduction's, no atomics, no scratch.
// Ring and padding of the outputs are not touched: rows 1 .. N - 1 are written, columns 0 and >= N with zeros.
#pragma once

#include "mgx_var.hpp"

namespace mgx {

// the scalars of a pass, in T: the polynomial, its derivative's coefficients and the step length
template <typename T> struct NewtonPoly { T p1, p2, p3, q2, q3, lam; };

template <typename T> NewtonPoly<T> newton_poly(double p1, double p2, double p3, T lam)
{
    return NewtonPoly<T>{(T)p1, (T)p2, (T)p3, (T)(2.0 * p2), (T)(3.0 * p3), lam};
}

template <typename T, int NQ, bool STEP>
__global__ void __launch_bounds__(kBlock)
k_newton_pass(const T* __restrict__ u, const T* __restrict__ de, const T* __restrict__ f, const T* __restrict__ kap, const T* __restrict__ c0,
              Op9<T> a, T* __restrict__ ut, T* __restrict__ b, T* __restrict__ d, double* __restrict__ partial, NewtonPoly<T> p, int N,
              long pitch, int row_lo, int row_hi, int strips, int rows_alloc)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[kWavesPerBlock];
    RowTile<T> t = load_rows<T>(u, N, pitch, row_lo, row_hi, strips, rows_alloc);
    double acc = 0.0;
    if (t.active) {
        if constexpr (STEP) {
            const RowTile<T> e = load_rows<T>(de, N, pitch, row_lo, row_hi, strips, rows_alloc);
            auto trial = [&](const V& uv, const V& ev) {
                const Lanes<T> ul = to_lanes(uv), el = to_lanes(ev);
                Lanes<T> o;
#pragma unroll
                for (int x = 0; x < W; ++x) o.a[x] = ul.a[x] + p.lam * el.a[x];
                return from_lanes(o);
            };
            t.up = trial(t.up, e.up);
            t.cur = trial(t.cur, e.cur);
            t.dn = trial(t.dn, e.dn);
        }
        const Lanes<T> ff = load_lanes(f + t.at, t.in), kk = load_lanes(kap + t.at, t.in), cc = load_lanes(c0 + t.at, t.in);
        Lanes<T> k[9];
        load_coefs<NQ, 1>(a, t.at, t.in, k);
        const Lanes<T> q = stencil_sum<NQ>(rows_of<NQ>(t), k, [&](int x) { return cc.a[x]; });
        const Lanes<T> v = to_lanes(t.cur);
        Lanes<T> ob, od;
#pragma unroll
        for (int x = 0; x < W; ++x) {
            const T ph = ((p.p3 * v.a[x] + p.p2) * v.a[x] + p.p1) * v.a[x];
            const T dp = (p.q3 * v.a[x] + p.q2) * v.a[x] + p.p1;
            ob.a[x] = ff.a[x] - (q.a[x] + kk.a[x] * ph);
            od.a[x] = kk.a[x] * dp;
        }
        const V bv = masked_row(ob, t, N);
        if (t.st) acc = lane_squares(to_lanes(bv));
        if constexpr (STEP) store_row(ut, v, t, N);
        vstore<V>(b + t.at, bv, t.st);
        store_row(d, od, t, N);
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

// one pass on a level: b, d (and ut when step) from u (and de), then sum[0] = the sum of b^2 through partial (one double
// per workgroup, k_residual_var's geometry).  c0: the centre of A0; v.a's slot 0 is not read
template <typename T>
void launch_newton_pass(const VarLevel<T>& v, bool step, const T* u, const T* de, const T* f, const T* kap, const T* c0, T* ut, T* b, T* d,
                        const NewtonPoly<T>& p, double* partial, double* sum, hipStream_t st)
{
    const Launch g = make_launch(v.N, VecOf<T>::W, v.N - 1, 1);
    const dim3 grd(g.blocks), blk(kBlock);
    with_point_count(v.nine, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if (step)
            hipLaunchKernelGGL((k_newton_pass<T, NQ, true>), grd, blk, 0, st, u, de, f, kap, c0, v.a, ut, b, d, partial, p, v.N, v.pitch, 1, v.N,
                               g.strips, v.rows);
        else
            hipLaunchKernelGGL((k_newton_pass<T, NQ, false>), grd, blk, 0, st, u, de, f, kap, c0, v.a, ut, b, d, partial, p, v.N, v.pitch, 1, v.N,
                               g.strips, v.rows);
    });
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, st, partial, g.blocks, sum);
}

// mgx.hip uses these instantiations; mgx_inst.hip (-DMGX_INST_KIND=14) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
#define MGX_NEWTON_EXTERN(T)                                                                                                              \
    extern template void launch_newton_pass<T>(const VarLevel<T>&, bool, const T*, const T*, const T*, const T*, const T*, T*, T*, T*, \
                                               const NewtonPoly<T>&, double*, double*, hipStream_t);
MGX_NEWTON_EXTERN(double)
MGX_NEWTON_EXTERN(float)
#undef MGX_NEWTON_EXTERN
#endif

} // namespace mgx
