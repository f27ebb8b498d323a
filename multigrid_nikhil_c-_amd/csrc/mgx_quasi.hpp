// mgx_quasi.hpp - the fused pass of mgx_quasi (absent in the reference): one sweep over the finest level
// of a GALERKIN handle turns the iterate into the operator of the next linear solve and its right-hand side, for
//   F(u) = A(u) u - f,   A(u) the five-point discretisation of -div(a(x) k(u) grad u),  k(u) = k0 + k1 u + k2 u^2:
//
//   k_quasi_pass<T, STEP, NEWTON>  v      = u                 (STEP = false: the first evaluation)
//                                  v      = u + lam * de      (STEP = true: a trial of the line search; ut <- v), in T
//                                  at the point p and its four neighbours x, in double whatever T is:
//                                  vd_x   = (double)v_x
//                                  kap_x  = a_x * ((k2 * vd_x + k1) * vd_x + k0)
//                                  fn     = 0.5 * (kap_p + kap_N), fs, fw, fe alike        (k_var_from_nodes' faces)
//                                  cP     = (T)(((fn + fw) + fe) + fs);  nP = (T)(-fn), sP, wP, eP alike
//                                  q      = stencil_sum<5> of v with (cP, nP, sP, wP, eP), in T: mgx_residual's sum
//                                  b_p    = f_p - q;   partial[block] = the block's sum of b_p^2
//                                  NEWTON = false: the five output grids take (cP, nP, sP, wP, eP)
//                                  NEWTON = true:  dk_x = a_x * (kk2 * vd_x + k1),  kk2 = 2.0 * k2 by the host
//                                                  gN = vd_p - vd_N, gS, gW, gE alike;  sg = ((gN + gW) + gE) + gS
//                                                  cJ = (T)((((fn + fw) + fe) + fs) + (0.5 * dk_p) * sg)
//                                                  nJ = (T)((0.5 * dk_N) * gN - fn), sJ, wJ, eJ alike
//                                  the Jacobian of F: five-point, not symmetric.  The residual uses the Picard
//                                  coefficients either way; every product and sum is rounded on its own (no contraction),
//                                  one rounding to T per coefficient.
//
// a is the nodal coefficient in a double grid of the level's rows and pitch (elements), boundary nodes included, padding
// zero: a lane's W points are 8 W bytes of it, 32 in float.  The ring of u and de is zero, so v is zero there and a ring
// node's kap is a * k0; coefficients that point at the ring are stored as computed.
// Geometry: k_newton_pass's - one wave per row and strip, 16-byte lanes, load_rows / rows_of / stencil_sum<5> / masked_row,
// lane_squares and block_reduce, then k_reduce_partials: the sum is bit for bit the one mgx_residual_norm forms from
// (U = 0, B = b).  kap (and dk) of the w / e neighbours come from the adjacent lanes by DPP, which computed them from the
// same inputs.  Every load of the wave comes before its first store (mgx_var.hpp, ALIASING).  Rows 1 .. N - 1 are
// written, columns 0 and >= N with zeros; no LDS beyond the reduction's, no atomics, no scratch.
// Words of T per point: u, f and a in (a counts two in float), five coefficients and b out; STEP: de in and ut out too.
#pragma once

#include "mgx_var.hpp"

namespace mgx {

// the scalars of a pass: the polynomial in double, kk2 = 2 k2, and the step length in T
template <typename T> struct QuasiPoly { double k0, k1, k2, kk2; T lam; };

template <typename T> QuasiPoly<T> quasi_poly(double k0, double k1, double k2, T lam) { return QuasiPoly<T>{k0, k1, k2, 2.0 * k2, lam}; }

// the five output grids c, n, s, w, e (indexed by constants only)
template <typename T> struct Quasi5Out { T* a[5]; };

template <typename T> struct LanesD { double a[VecOf<T>::W]; };

// a lane's W nodal values: W / 2 loads of 16 bytes
template <typename T> __device__ __forceinline__ LanesD<T> load_nodes(const double* __restrict__ a, long at, bool pred)
{
    constexpr int W = VecOf<T>::W;
    LanesD<T> o;
#pragma unroll
    for (int x = 0; x < W; x += 2) {
        const double2 v = vload<double2>(a + at + x, pred);
        o.a[x] = v.x;
        o.a[x + 1] = v.y;
    }
    return o;
}

// rows [row_lo, row_hi) must lie in [1, rows_alloc - 1): the rows above and below a tile's are then inside the allocation
template <typename T, bool STEP, bool NEWTON>
__global__ void __launch_bounds__(kBlock)
k_quasi_pass(const T* __restrict__ u, const T* __restrict__ de, const T* __restrict__ f, const double* __restrict__ an, Quasi5Out<T> out,
             T* __restrict__ ut, T* __restrict__ b, double* __restrict__ partial, QuasiPoly<T> p, int N, long pitch, int row_lo, int row_hi,
             int strips, int rows_alloc)
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
        const Lanes<T> ff = load_lanes(f + t.at, t.in);
        const LanesD<T> au = load_nodes<T>(an, t.at - pitch, t.in), ac = load_nodes<T>(an, t.at, t.in), ad = load_nodes<T>(an, t.at + pitch, t.in);
        const Rows3<T> r = rows_of<5>(t);
        auto kappa = [&](double a, double vd) { return a * ((p.k2 * vd + p.k1) * vd + p.k0); };
        auto dkappa = [&](double a, double vd) { return a * (p.kk2 * vd + p.k1); };
        double vu[W], vc[W], vn[W], ku[W], kc[W], kn[W];
#pragma unroll
        for (int x = 0; x < W; ++x) {
            vu[x] = (double)r.up.a[x]; vc[x] = (double)r.cur.a[x]; vn[x] = (double)r.dn.a[x];
            ku[x] = kappa(au.a[x], vu[x]); kc[x] = kappa(ac.a[x], vc[x]); kn[x] = kappa(ad.a[x], vn[x]);
        }
        const double kl = from_left(kc[W - 1]), kr = from_right(kc[0]);
        const double vl = (double)r.cl, vr = (double)r.cr;
        double du[W], dc[W], dn[W], dl = 0.0, dr = 0.0;
        if constexpr (NEWTON) {
#pragma unroll
            for (int x = 0; x < W; ++x) { du[x] = dkappa(au.a[x], vu[x]); dc[x] = dkappa(ac.a[x], vc[x]); dn[x] = dkappa(ad.a[x], vn[x]); }
            dl = from_left(dc[W - 1]);
            dr = from_right(dc[0]);
        }
        Lanes<T> k[9], o[5];
        double fnn[W], fss[W], fww[W], fee[W], ctr[W];
#pragma unroll
        for (int x = 0; x < W; ++x) {
            const double kw = x == 0 ? kl : kc[x == 0 ? 0 : x - 1], ke = x == W - 1 ? kr : kc[x == W - 1 ? x : x + 1];
            fnn[x] = 0.5 * (kc[x] + ku[x]); fss[x] = 0.5 * (kc[x] + kn[x]);
            fww[x] = 0.5 * (kc[x] + kw); fee[x] = 0.5 * (kc[x] + ke);
            ctr[x] = ((fnn[x] + fww[x]) + fee[x]) + fss[x];
            k[0].a[x] = (T)ctr[x];
            k[1].a[x] = (T)(-fnn[x]); k[2].a[x] = (T)(-fss[x]); k[3].a[x] = (T)(-fww[x]); k[4].a[x] = (T)(-fee[x]);
        }
        const Lanes<T> q = stencil_sum<5>(r, k, [&](int x) { return k[0].a[x]; });
        Lanes<T> ob;
#pragma unroll
        for (int x = 0; x < W; ++x) ob.a[x] = ff.a[x] - q.a[x];
        if constexpr (NEWTON) {
#pragma unroll
            for (int x = 0; x < W; ++x) {
                const double vw = x == 0 ? vl : vc[x == 0 ? 0 : x - 1], ve = x == W - 1 ? vr : vc[x == W - 1 ? x : x + 1];
                const double dw = x == 0 ? dl : dc[x == 0 ? 0 : x - 1], dee = x == W - 1 ? dr : dc[x == W - 1 ? x : x + 1];
                const double gN = vc[x] - vu[x], gS = vc[x] - vn[x], gW = vc[x] - vw, gE = vc[x] - ve;
                const double sg = ((gN + gW) + gE) + gS;
                o[0].a[x] = (T)(ctr[x] + (0.5 * dc[x]) * sg);
                o[1].a[x] = (T)((0.5 * du[x]) * gN - fnn[x]);
                o[2].a[x] = (T)((0.5 * dn[x]) * gS - fss[x]);
                o[3].a[x] = (T)((0.5 * dw) * gW - fww[x]);
                o[4].a[x] = (T)((0.5 * dee) * gE - fee[x]);
            }
        } else {
#pragma unroll
            for (int q5 = 0; q5 < 5; ++q5) o[q5] = k[q5];
        }
        const V bv = masked_row(ob, t, N);
        if (t.st) acc = lane_squares(to_lanes(bv));
        if constexpr (STEP) store_row(ut, to_lanes(t.cur), t, N);
        vstore<V>(b + t.at, bv, t.st);
#pragma unroll
        for (int q5 = 0; q5 < 5; ++q5) store_row(out.a[q5], o[q5], t, N);
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

// one pass on a level of N intervals (rows allocated, pitch in elements): out, b (and ut when step) from u (and de), f and
// the nodal a, then sum[0] = the sum of b^2 through partial (one double per workgroup, k_residual_var's geometry)
template <typename T>
void launch_quasi_pass(int N, int rows, long pitch, bool step, bool newton, const T* u, const T* de, const T* f, const double* an,
                       const Quasi5Out<T>& out, T* ut, T* b, const QuasiPoly<T>& p, double* partial, double* sum, hipStream_t st)
{
    const Launch g = make_launch(N, VecOf<T>::W, N - 1, 1);
    const dim3 grd(g.blocks), blk(kBlock);
    auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grd, blk, 0, st, u, de, f, an, out, ut, b, partial, p, N, pitch, 1, N, g.strips, rows); };
    if (newton) {
        if (step) go(k_quasi_pass<T, true, true>);
        else go(k_quasi_pass<T, false, true>);
    } else {
        if (step) go(k_quasi_pass<T, true, false>);
        else go(k_quasi_pass<T, false, false>);
    }
    hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, st, partial, g.blocks, sum);
}

// mgx.hip uses these instantiations; mgx_inst.hip (-DMGX_INST_KIND=15) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
#define MGX_QUASI_EXTERN(T)                                                                                                                   \
    extern template void launch_quasi_pass<T>(int, int, long, bool, bool, const T*, const T*, const T*, const double*, const Quasi5Out<T>&, \
                                              T*, T*, const QuasiPoly<T>&, double*, double*, hipStream_t);
MGX_QUASI_EXTERN(double)
MGX_QUASI_EXTERN(float)
#undef MGX_QUASI_EXTERN
#endif

} // namespace mgx
