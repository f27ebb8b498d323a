// mgx_cheby.hpp - Chebyshev polynomial smoothing for the general-operator hierarchies (cfg.smoother =
// MGX_SMOOTHER_CHEBYSHEV with op = MGX_OPERATOR_STENCIL5 / MGX_OPERATOR_GALERKIN) and the eigenvalue bound it needs.
//
// THE ITERATION (tests/cheby_ref.py states it in numpy, operation by operation).  J(v) = R_omega v + omega (D_inv b) is
// the sweep of k_jacobi_var (mgx_var.hpp: stencil_sum, jacobi_value), computed exactly as there; z = J(v) - v = omega D^-1 (b - A v).  With
//     lmax = omega g_l,  lmin = lmax / 4,  theta = (lmax + lmin) / 2,  delta = (lmax - lmin) / 2,  sigma = theta / delta
// a block of degree mu is, from d undefined,
//     step 0:       d = c_0 z                      c_0 = 1 / theta,                       rho_0 = 1 / sigma
//     step k >= 1:  d = (a_k d) + (c_k z)          rho_k = 1 / (2 sigma - rho_{k-1}),  a_k = rho_k rho_{k-1},  c_k = (2 rho_k) / delta
//     every step:   v' = v + d
// The scalars are formed on the host in double (cheby_scalars) and rounded to T once.  In the kernel z = J - v is one
// rounding, the new d is one multiplication, one multiplication and one addition in that order (no contraction), and
// v' = v + d is one more.  v goes out of place (u <-> tmp like the Jacobi sweep); d is updated in place: a lane reads
// and writes its own columns of d only.  FIRST = 1 (step 0) does not read d.  Columns 0 and >= N of v' and d are
// written as zero; ring rows are never written.
//
// Roofline: the Jacobi sweep's traffic plus d in and d out: 10 sizeof(T) per point on five-point levels (9 on a first
// step), 14 on nine-point levels (13 on a first step).  HBM-bound single passes in the geometry of k_jacobi_var.
//
// THE BOUND  g_l = max over the interior points of  1 + sum_x |D_inv a_x|,  x = n, s, w, e (five-point levels) or
// n, s, w, e, nw, ne, sw, se (nine-point levels): the Gershgorin row sum of D^-1 A, an upper bound of its spectrum.
// Per point: acc = 1.0; acc = acc + |(double)D_inv * (double)a_x| in that order, in double whatever T is.  A coefficient
// that points at the Dirichlet ring is not counted (the library never reads it).  A maximum does not depend on the
// order it is taken in: k_lambda_partials leaves one maximum per block, k_reduce_max (one workgroup, the pattern of
// k_reduce_partials) the level's.
#pragma once

#include "mgx_var.hpp"

#include <vector>

namespace mgx {

// the two scalars (a_k, c_k) of every step of a degree-mu block, in double
struct ChebyStep { double a, c; };
inline std::vector<ChebyStep> cheby_scalars(double omega, double g, int mu)
{
    const double lmax = omega * g, lmin = lmax / 4.0;
    const double theta = (lmax + lmin) / 2.0, delta = (lmax - lmin) / 2.0, sigma = theta / delta;
    std::vector<ChebyStep> st;
    double rho = 1.0 / sigma;
    for (int k = 0; k < mu; ++k) {
        if (k == 0) { st.push_back({0.0, 1.0 / theta}); continue; }
        const double rho_k = 1.0 / (2.0 * sigma - rho);
        st.push_back({rho_k * rho, (2.0 * rho_k) / delta});
        rho = rho_k;
    }
    return st;
}

// z = J - v, the new d and v' = v + d of one lane; dv: the lane's d (unused when FIRST)
template <typename T, int FIRST>
__device__ __forceinline__ void cheby_update(const Lanes<T>& p1, const Lanes<T>& cur, const Lanes<T>& b, const Lanes<T>& dinv,
                                             const Lanes<T>& dv, T omega, T ca, T cc, Lanes<T>& dnew, Lanes<T>& vnew)
{
    constexpr int W = VecOf<T>::W;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const T z = jacobi_value(p1.a[k], omega, dinv.a[k], b.a[k]) - cur.a[k];
        T d;
        if (FIRST) d = cc * z;
        else {
            const T t1 = ca * dv.a[k];
            const T t2 = cc * z;
            d = t1 + t2;
        }
        dnew.a[k] = d;
        vnew.a[k] = cur.a[k] + d;
    }
}

// one Chebyshev step on a level; rows [row_lo, row_hi).  r: the off-diagonals of R_omega in slots 1 .. NQ - 1
template <typename T, int NQ, int FIRST>
__global__ void __launch_bounds__(kBlock)
k_cheby_var(const T* __restrict__ vin, const T* __restrict__ rhs, T* __restrict__ vout, T* __restrict__ dir, const T* __restrict__ dinv,
            Op9<T> r, int N, long pitch, int row_lo, int row_hi, int strips, T rc, T omega, T ca, T cc, int rows_alloc)
{
    const RowTile<T> t = load_rows<T>(vin, N, pitch, row_lo, row_hi, strips, rows_alloc);
    if (!t.active) return;
    const Lanes<T> b = load_lanes(rhs + t.at, t.in), d = load_lanes(dinv + t.at, t.in);
    Lanes<T> k[9];
    load_coefs<NQ, 1>(r, t.at, t.in, k);
    Lanes<T> dold = to_lanes(t.cur);
    if (!FIRST) dold = load_lanes(dir + t.at, t.in);
    const Lanes<T> p1 = stencil_sum<NQ>(rows_of<NQ>(t), k, [&](int) { return rc; });
    Lanes<T> dnew, vnew;
    cheby_update<T, FIRST>(p1, to_lanes(t.cur), b, d, dold, omega, ca, cc, dnew, vnew);
    store_row(dir, dnew, t, N);
    store_row(vout, vnew, t, N);
}

// per-block maxima of the Gershgorin row sums of D^-1 A: block b takes the interior rows 1 + b, 1 + b + gridDim.x, ...
// a: the operator (slots 1 .. NQ - 1), dinv: its D_inv.  partial[b] >= 1 for every block (rows <= N - 1 blocks)
template <typename T, int NQ>
__global__ void __launch_bounds__(kBlock)
k_lambda_partials(Op9<T> a, const T* __restrict__ dinv, int N, long pitch, double* __restrict__ partial)
{
    __shared__ double wmax[kWavesPerBlock];
    double m = 0.0;
    for (int row = 1 + blockIdx.x; row < N; row += gridDim.x)
        for (int col = 1 + threadIdx.x; col < N; col += blockDim.x) {
            const long at = (long)row * pitch + col;
            const double d = (double)dinv[at];
            const bool rn = row > 1, rs = row < N - 1, cw = col > 1, ce = col < N - 1;
            double acc = 1.0;
            if (rn) acc = acc + fabs(d * (double)a.a[1][at]);
            if (rs) acc = acc + fabs(d * (double)a.a[2][at]);
            if (cw) acc = acc + fabs(d * (double)a.a[3][at]);
            if (ce) acc = acc + fabs(d * (double)a.a[4][at]);
            if (NQ == 9) {
                if (rn && cw) acc = acc + fabs(d * (double)a.a[5][at]);
                if (rn && ce) acc = acc + fabs(d * (double)a.a[6][at]);
                if (rs && cw) acc = acc + fabs(d * (double)a.a[7][at]);
                if (rs && ce) acc = acc + fabs(d * (double)a.a[8][at]);
            }
            m = acc > m ? acc : m;
        }
    block_reduce<kWavesPerBlock>(m, wmax, partial + blockIdx.x, ReduceMax{});
}

// out[0] = max of n partials: one workgroup, the pattern of k_reduce_partials with max in place of sum
static __global__ void __launch_bounds__(kReduceThreads) k_reduce_max(const double* __restrict__ partial, int n, double* __restrict__ out)
{
    __shared__ double wmax[kReduceThreads / kWave];
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += kReduceThreads) m = partial[i] > m ? partial[i] : m;
    block_reduce<kReduceThreads / kWave>(m, wmax, out, ReduceMax{});
}

// ---- host side (the level view VarLevel and the dispatchers: mgx_var.hpp) ---------------------------------------
// one step over the whole level: v' into vout, d in place
template <typename T>
void launch_cheby(const VarLevel<T>& l, const T* vin, const T* b, T* vout, T* dir, bool first, T rc, T omega, T ca, T cc, hipStream_t st)
{
    const Launch g = make_launch(l.N, VecOf<T>::W, l.N - 1, 1);
    const dim3 grd(g.blocks), blk(kBlock);
    with_point_count(l.nine, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        if (first) hipLaunchKernelGGL((k_cheby_var<T, NQ, 1>), grd, blk, 0, st, vin, b, vout, dir, l.dinv, l.r, l.N, l.pitch, 1, l.N, g.strips, rc, omega, ca, cc, l.rows);
        else hipLaunchKernelGGL((k_cheby_var<T, NQ, 0>), grd, blk, 0, st, vin, b, vout, dir, l.dinv, l.r, l.N, l.pitch, 1, l.N, g.strips, rc, omega, ca, cc, l.rows);
    });
}

// g_l into out[0] (device); partial holds at least partial_cap doubles
template <typename T>
void launch_lambda_max(const VarLevel<T>& l, double* partial, long partial_cap, double* out, hipStream_t st)
{
    const int blocks = (int)std::max(1L, std::min<long>(std::min<long>(l.N - 1, partial_cap), 1024));
    with_point_count(l.nine, [&](auto nq) {
        hipLaunchKernelGGL((k_lambda_partials<T, decltype(nq)::value>), dim3(blocks), dim3(kBlock), 0, st, l.a, l.dinv, l.N, l.pitch, partial);
    });
    hipLaunchKernelGGL(k_reduce_max, dim3(1), dim3(kReduceThreads), 0, st, partial, blocks, out);
}

// mgx.hip declares these instantiations; mgx_inst.hip (-DMGX_INST_KIND=4) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
extern template void launch_cheby<double>(const VarLevel<double>&, const double*, const double*, double*, double*, bool, double, double, double, double, hipStream_t);
extern template void launch_cheby<float>(const VarLevel<float>&, const float*, const float*, float*, float*, bool, float, float, float, float, hipStream_t);
extern template void launch_lambda_max<double>(const VarLevel<double>&, double*, long, double*, hipStream_t);
extern template void launch_lambda_max<float>(const VarLevel<float>&, double*, long, double*, hipStream_t);
#endif

} // namespace mgx
