// mgx_cheby.hpp - Chebyshev polynomial smoothing for the general-operator hierarchies (cfg.smoother =
// MGX_SMOOTHER_CHEBYSHEV with op = MGX_OPERATOR_STENCIL5 / MGX_OPERATOR_GALERKIN) and the eigenvalue bound it needs.
//
// THE ITERATION (tests/cheby_ref.py states it in numpy, operation by operation).  J(v) = R_omega v + omega (D_inv b) is
// the sweep of k_jacobi_var / k_jacobi_var9, computed exactly as there; z = J(v) - v = omega D^-1 (b - A v).  With
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

#include "mgx_galerkin.hpp"

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
        const T j = p1.a[k] + omega * (dinv.a[k] * b.a[k]);
        const T z = j - cur.a[k];
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

// one Chebyshev step on a five-point level; rows [row_lo, row_hi).  r: the off-diagonals of R_omega in slots 1..4
template <typename T, int FIRST>
__global__ void __launch_bounds__(kBlock)
k_cheby_var(const T* __restrict__ vin, const T* __restrict__ rhs, T* __restrict__ vout, T* __restrict__ dir, const T* __restrict__ dinv,
            Op9<T> r, int N, long pitch, int row_lo, int row_hi, int strips, T rc, T omega, T ca, T cc, int rows_alloc)
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
    const Lanes<T> n = to_lanes(vload<V>(r.a[1] + at, in)), s = to_lanes(vload<V>(r.a[2] + at, in));
    const Lanes<T> w = to_lanes(vload<V>(r.a[3] + at, in)), e = to_lanes(vload<V>(r.a[4] + at, in));
    Lanes<T> dold = to_lanes(cur);
    if (!FIRST) dold = to_lanes(vload<V>(dir + at, in));
    const T left = from_left(last(cur)), right = from_right(first(cur));
    const Lanes<T> p1 = stencil5<T>(to_lanes(up), to_lanes(cur), to_lanes(dn), left, right, n, w, [&](int) { return rc; }, e, s);
    Lanes<T> dnew, vnew;
    cheby_update<T, FIRST>(p1, to_lanes(cur), to_lanes(bb), to_lanes(dv), dold, omega, ca, cc, dnew, vnew);
    V od = from_lanes(dnew), ov = from_lanes(vnew);
    mask_cols(od, c.col, N);
    mask_cols(ov, c.col, N);
    vstore<V>(dir + at, od, c.st && in);
    vstore<V>(vout + at, ov, c.st && in);
}

// one Chebyshev step on a nine-point level.  r: the eight off-diagonals of R_omega in slots 1..8
template <typename T, int FIRST>
__global__ void __launch_bounds__(kBlock)
k_cheby_var9(const T* __restrict__ vin, const T* __restrict__ rhs, T* __restrict__ vout, T* __restrict__ dir, const T* __restrict__ dinv,
             Op9<T> r, int N, long pitch, int row_lo, int row_hi, int strips, T rc, T omega, T ca, T cc, int rows_alloc)
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
    Lanes<T> dold = to_lanes(cur);
    if (!FIRST) dold = to_lanes(vload<V>(dir + at, in));
    const T ul = from_left(last(up)), ur = from_right(first(up));
    const T cl = from_left(last(cur)), cr = from_right(first(cur));
    const T dl = from_left(last(dn)), dr = from_right(first(dn));
    const Lanes<T> p1 = stencil9<T>(to_lanes(up), to_lanes(cur), to_lanes(dn), ul, ur, cl, cr, dl, dr, k9[5], k9[1], k9[6], k9[3],
                                    [&](int) { return rc; }, k9[4], k9[7], k9[2], k9[8]);
    Lanes<T> dnew, vnew;
    cheby_update<T, FIRST>(p1, to_lanes(cur), to_lanes(bb), to_lanes(dv), dold, omega, ca, cc, dnew, vnew);
    V od = from_lanes(dnew), ov = from_lanes(vnew);
    mask_cols(od, c.col, N);
    mask_cols(ov, c.col, N);
    vstore<V>(dir + at, od, c.st && in);
    vstore<V>(vout + at, ov, c.st && in);
}

// per-block maxima of the Gershgorin row sums of D^-1 A: block b takes the interior rows 1 + b, 1 + b + gridDim.x, ...
// a: the operator (slots 1..4, and 5..8 when NINE), dinv: its D_inv.  partial[b] >= 1 for every block (rows <= N - 1 blocks)
template <typename T, bool NINE>
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
            if (NINE) {
                if (rn && cw) acc = acc + fabs(d * (double)a.a[5][at]);
                if (rn && ce) acc = acc + fabs(d * (double)a.a[6][at]);
                if (rs && cw) acc = acc + fabs(d * (double)a.a[7][at]);
                if (rs && ce) acc = acc + fabs(d * (double)a.a[8][at]);
            }
            m = acc > m ? acc : m;
        }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(m, off, kWave);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int w = 0; w < kWavesPerBlock; ++w) r = wmax[w] > r ? wmax[w] : r;
        partial[blockIdx.x] = r;
    }
}

// out[0] = max of n partials: one workgroup, the pattern of k_reduce_partials with max in place of sum
static __global__ void __launch_bounds__(kReduceThreads) k_reduce_max(const double* __restrict__ partial, int n, double* __restrict__ out)
{
    __shared__ double wmax[kReduceThreads / kWave];
    double m = 0.0;
    for (int i = threadIdx.x; i < n; i += kReduceThreads) m = partial[i] > m ? partial[i] : m;
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(m, off, kWave);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int w = 0; w < kReduceThreads / kWave; ++w) r = wmax[w] > r ? wmax[w] : r;
        out[0] = r;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------
// what the launches below need of a level: the operator a (slots 0..8, corners null on five-point levels), its D_inv
// and the off-diagonals r of R_omega (slots 1..8)
template <typename T> struct ChebyLevel {
    Op9<T> a, r;
    const T* dinv;
    bool nine;
    int N, rows;
    long pitch;
};

// one step over the whole level: v' into vout, d in place
template <typename T>
void launch_cheby(const ChebyLevel<T>& l, const T* vin, const T* b, T* vout, T* dir, bool first, T rc, T omega, T ca, T cc, hipStream_t st)
{
    const Launch g = make_launch(l.N, VecOf<T>::W, l.N - 1, 1);
    const dim3 grd(g.blocks), blk(kBlock);
    if (l.nine) {
        if (first) hipLaunchKernelGGL((k_cheby_var9<T, 1>), grd, blk, 0, st, vin, b, vout, dir, l.dinv, l.r, l.N, l.pitch, 1, l.N, g.strips, rc, omega, ca, cc, l.rows);
        else hipLaunchKernelGGL((k_cheby_var9<T, 0>), grd, blk, 0, st, vin, b, vout, dir, l.dinv, l.r, l.N, l.pitch, 1, l.N, g.strips, rc, omega, ca, cc, l.rows);
    } else {
        if (first) hipLaunchKernelGGL((k_cheby_var<T, 1>), grd, blk, 0, st, vin, b, vout, dir, l.dinv, l.r, l.N, l.pitch, 1, l.N, g.strips, rc, omega, ca, cc, l.rows);
        else hipLaunchKernelGGL((k_cheby_var<T, 0>), grd, blk, 0, st, vin, b, vout, dir, l.dinv, l.r, l.N, l.pitch, 1, l.N, g.strips, rc, omega, ca, cc, l.rows);
    }
}

// g_l into out[0] (device); partial holds at least partial_cap doubles
template <typename T>
void launch_lambda_max(const ChebyLevel<T>& l, double* partial, long partial_cap, double* out, hipStream_t st)
{
    const int blocks = (int)std::max(1L, std::min<long>(std::min<long>(l.N - 1, partial_cap), 1024));
    if (l.nine) hipLaunchKernelGGL((k_lambda_partials<T, true>), dim3(blocks), dim3(kBlock), 0, st, l.a, l.dinv, l.N, l.pitch, partial);
    else hipLaunchKernelGGL((k_lambda_partials<T, false>), dim3(blocks), dim3(kBlock), 0, st, l.a, l.dinv, l.N, l.pitch, partial);
    hipLaunchKernelGGL(k_reduce_max, dim3(1), dim3(kReduceThreads), 0, st, partial, blocks, out);
}

// mgx.hip declares these instantiations; mgx_inst.hip (-DMGX_INST_KIND=4) defines them
#if !defined(MGX_INST_KIND) && !defined(MGX_SINGLE_TU)
extern template void launch_cheby<double>(const ChebyLevel<double>&, const double*, const double*, double*, double*, bool, double, double, double, double, hipStream_t);
extern template void launch_cheby<float>(const ChebyLevel<float>&, const float*, const float*, float*, float*, bool, float, float, float, float, hipStream_t);
extern template void launch_lambda_max<double>(const ChebyLevel<double>&, double*, long, double*, hipStream_t);
extern template void launch_lambda_max<float>(const ChebyLevel<float>&, double*, long, double*, hipStream_t);
#endif

} // namespace mgx
