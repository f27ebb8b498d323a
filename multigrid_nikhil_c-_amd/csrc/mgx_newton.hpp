// mgx_newton.hpp - the fused pass of mgx_newton (absent in the reference): one sweep over the finest
// level of a GALERKIN handle forms, for  F(u) = A0 u + kap phi(u) - f,  phi(u) = p1 u + p2 u^2 + p3 u^3:
//
//   k_newton_pass<T, NQ, STEP, false>  v   = u                   (STEP = false: the first evaluation)
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
//
// The time stepper mgx_newton_steps runs the same family with a mass term, and one more kernel.  One
// theta step from the time level u solves  G(v) = A0 v + dm v + kap phi(v) - r = 0,  dm = rho h^2 / (theta dt):
//
//   k_newton_pass<T, NQ, STEP, true>   MASS: one more grid in, dm; v, q, ph, dp, the trial, the squares and the
//                                  reduction as above, r arrives as f, and
//                                  b_p = r_p - ((q + dm_p * v) + kap_p * ph)
//                                  d_p = dm_p + kap_p * dp
//                                  One word per point more than the MASS = false instance, which does not read dm.
//   k_newton_step_rhs<T, NQ, EULER>    the step's explicit part r, in k_theta_rhs's geometry (no reduction, no LDS):
//                                  m = dm_p * u_p
//                                  EULER (theta = 1):  r_p = m                               [+ g_p when g is given]
//                                  otherwise:          q = (A0 u)_p and ph as above;
//                                                      r_p = m - c0 * (q + kap_p * ph)       [+ g_p]
//                                  c0 = (T)((1 - theta) / theta) formed in double by the host.  The EULER instance reads
//                                  no neighbour and no coefficient grid: the lane's own vector of u, dm (and g) only, on
//                                  the lanes that store.  Words per point: NQ + 4 in (u, dm, kap, g, the centre, NQ - 1
//                                  grids of A) and 1 out; EULER 3 in and 1 out.
#pragma once

#include "mgx_var.hpp"

namespace mgx {

// the scalars of a pass, in T: the polynomial, its derivative's coefficients and the step length
template <typename T> struct NewtonPoly { T p1, p2, p3, q2, q3, lam; };

template <typename T> NewtonPoly<T> newton_poly(double p1, double p2, double p3, T lam)
{
    return NewtonPoly<T>{(T)p1, (T)p2, (T)p3, (T)(2.0 * p2), (T)(3.0 * p3), lam};
}

template <typename T, int NQ, bool STEP, bool MASS>
__global__ void __launch_bounds__(kBlock)
k_newton_pass(const T* __restrict__ u, const T* __restrict__ de, const T* __restrict__ f, const T* __restrict__ kap, const T* __restrict__ c0,
              Op9<T> a, T* __restrict__ ut, T* __restrict__ b, T* __restrict__ d, double* __restrict__ partial, NewtonPoly<T> p, int N,
              long pitch, int row_lo, int row_hi, int strips, int rows_alloc, const T* __restrict__ dm)
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
        Lanes<T> mm{};
        if constexpr (MASS) mm = load_lanes(dm + t.at, t.in);
        Lanes<T> k[9];
        load_coefs<NQ, 1>(a, t.at, t.in, k);
        const Lanes<T> q = stencil_sum<NQ>(rows_of<NQ>(t), k, [&](int x) { return cc.a[x]; });
        const Lanes<T> v = to_lanes(t.cur);
        Lanes<T> ob, od;
#pragma unroll
        for (int x = 0; x < W; ++x) {
            const T ph = ((p.p3 * v.a[x] + p.p2) * v.a[x] + p.p1) * v.a[x];
            const T dp = (p.q3 * v.a[x] + p.q2) * v.a[x] + p.p1;
            if constexpr (MASS) {
                ob.a[x] = ff.a[x] - ((q.a[x] + mm.a[x] * v.a[x]) + kk.a[x] * ph);
                od.a[x] = mm.a[x] + kk.a[x] * dp;
            } else {
                ob.a[x] = ff.a[x] - (q.a[x] + kk.a[x] * ph);
                od.a[x] = kk.a[x] * dp;
            }
        }
        const V bv = masked_row(ob, t, N);
        if (t.st) acc = lane_squares(to_lanes(bv));
        if constexpr (STEP) store_row(ut, v, t, N);
        vstore<V>(b + t.at, bv, t.st);
        store_row(d, od, t, N);
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

// the explicit part of a time step (mgx_newton_steps).  cen: the centre of A0; a's slot 0 is not read
template <typename T, int NQ, bool EULER>
__global__ void __launch_bounds__(kBlock)
k_newton_step_rhs(const T* __restrict__ u, const T* __restrict__ dm, const T* __restrict__ kap, const T* __restrict__ g, const T* __restrict__ cen,
                  Op9<T> a, T* __restrict__ out, NewtonPoly<T> p, T c0, int N, long pitch, int row_lo, int row_hi, int strips, int rows_alloc)
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
        const Lanes<T> uu = load_lanes(u + at, st), mm = load_lanes(dm + at, st);
        Lanes<T> gg{};
        if (has_g) gg = load_lanes(g + at, st);
        Lanes<T> o;
#pragma unroll
        for (int x = 0; x < W; ++x) {
            o.a[x] = mm.a[x] * uu.a[x];
            if (has_g) o.a[x] = o.a[x] + gg.a[x];
        }
        V ov = from_lanes(o);
        mask_cols(ov, c.col, N);
        vstore<V>(out + at, ov, st);
    } else {
        const RowTile<T> t = load_rows<T>(u, N, pitch, row_lo, row_hi, strips, rows_alloc);
        if (!t.active) return;
        const Lanes<T> mm = load_lanes(dm + t.at, t.in), kk = load_lanes(kap + t.at, t.in), cc = load_lanes(cen + t.at, t.in);
        Lanes<T> gg{};
        if (has_g) gg = load_lanes(g + t.at, t.in);
        Lanes<T> k[9];
        load_coefs<NQ, 1>(a, t.at, t.in, k);
        const Lanes<T> q = stencil_sum<NQ>(rows_of<NQ>(t), k, [&](int x) { return cc.a[x]; });
        const Lanes<T> uu = to_lanes(t.cur);
        Lanes<T> o;
#pragma unroll
        for (int x = 0; x < W; ++x) {
            const T m = mm.a[x] * uu.a[x];
            const T ph = ((p.p3 * uu.a[x] + p.p2) * uu.a[x] + p.p1) * uu.a[x];
            o.a[x] = m - c0 * (q.a[x] + kk.a[x] * ph);
            if (has_g) o.a[x] = o.a[x] + gg.a[x];
        }
        store_row(out, o, t, N);
    }
}

// one pass on a level: b, d (and ut when step) from u (and de), then sum[0] = the sum of b^2 through partial (one double
// per workgroup, k_residual_var's geometry).  c0: the centre of A0; v.a's slot 0 is not read.  dm: the mass term of a
// time step (the MASS instances; f is then the step's r), null for mgx_newton's F
template <typename T>
void launch_newton_pass(const VarLevel<T>& v, bool step, const T* u, const T* de, const T* f, const T* kap, const T* c0, const T* dm, T* ut, T* b,
                        T* d, const NewtonPoly<T>& p, double* partial, double* sum, hipStream_t st)
{
    const Launch g = make_launch(v.N, VecOf<T>::W, v.N - 1, 1);
    const dim3 grd(g.blocks), blk(kBlock);
    with_point_count(v.nine, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grd, blk, 0, st, u, de, f, kap, c0, v.a, ut, b, d, partial, p, v.N, v.pitch, 1, v.N, g.strips, v.rows, dm);
        };
        if (dm) {
            if (step) go(k_newton_pass<T, NQ, true, true>);
            else go(k_newton_pass<T, NQ, false, true>);
        } else {
            if (step) go(k_newton_pass<T, NQ, true, false>);
            else go(k_newton_pass<T, NQ, false, false>);
        }
    });
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, st, partial, g.blocks, sum);
}

// out = the explicit part of one theta step from u, dm, kap, g (null: none) and A0 (cen, v.a's slots 1 ..); theta = 1 is
// the EULER instance, which ignores kap, cen, v.a, p and c0
template <typename T>
void launch_newton_step_rhs(const VarLevel<T>& v, const T* u, const T* dm, const T* kap, const T* g, const T* cen, T* out, const NewtonPoly<T>& p,
                            double theta, hipStream_t st)
{
    const Launch gm = make_launch(v.N, VecOf<T>::W, v.N - 1, 1);
    const T c0 = (T)((1.0 - theta) / theta);
    const dim3 grd(gm.blocks), blk(kBlock);
    if (theta == 1.0) {
        hipLaunchKernelGGL((k_newton_step_rhs<T, 5, true>), grd, blk, 0, st, u, dm, kap, g, cen, v.a, out, p, c0, v.N, v.pitch, 1, v.N, gm.strips,
                           v.rows);
        return;
    }
    with_point_count(v.nine, [&](auto nq) {
        hipLaunchKernelGGL((k_newton_step_rhs<T, decltype(nq)::value, false>), grd, blk, 0, st, u, dm, kap, g, cen, v.a, out, p, c0, v.N, v.pitch,
                           1, v.N, gm.strips, v.rows);
    });
}

// mgx.hip uses these instantiations; mgx_inst.hip (-DMGX_INST_KIND=14) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
#define MGX_NEWTON_EXTERN(T)                                                                                                                      \
    extern template void launch_newton_pass<T>(const VarLevel<T>&, bool, const T*, const T*, const T*, const T*, const T*, const T*, T*, T*, T*, \
                                               const NewtonPoly<T>&, double*, double*, hipStream_t);                                            \
    extern template void launch_newton_step_rhs<T>(const VarLevel<T>&, const T*, const T*, const T*, const T*, const T*, T*,                    \
                                                   const NewtonPoly<T>&, double, hipStream_t);
MGX_NEWTON_EXTERN(double)
MGX_NEWTON_EXTERN(float)
#undef MGX_NEWTON_EXTERN
#endif

} // namespace mgx
