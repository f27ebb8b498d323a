// mgx_krylov.hpp - the Krylov passes of mgx_solve_pcg: conjugate gradients on the finest level, preconditioned
// by one V-cycle from zero (absent in the reference).
//
// Flexible PCG with the Polak-Ribiere beta; per iteration, after the V-cycle z = M r:
//   k_pcg_dots       rho_new = r.z and gamma = z.q                         reads r, z, q           3 sizeof(T)
//   k_pcg_direction  p' = z + beta p, q = A p', delta = p'.q               reads z, p; writes p', q 4 sizeof(T)
//                    (STENCIL5: + the five coefficient grids)              (+ 5 sizeof(T))
//   k_pcg_update     x += alpha p, r -= alpha q, ||r||^2                   reads x, p, r, q;
//                                                                          writes x, r             6 sizeof(T)
//   k_pcg_reduce     the per-block partials of one pass summed in a fixed order by one workgroup, and the scalar
//                    that depends on them (alpha after delta; beta and rho after the dots): no host round trip
// 13 sizeof(T) per fine point and iteration: 104 B in double, 52 B in float.
//
// Every pass covers rows 1 .. N-1 in the geometry of k_residual (row chunks marching down a column strip,
// W-wide vectors, halo lanes 0 and 63 never store) and masks columns 0 and >= N, so the Dirichlet ring and the
// padding of p, q and x stay zero: A reads them as neighbours.  p is written out of place (p' into a second
// buffer): a wave's halo rows and halo lanes are another wave's output.  Dots are accumulated in double whatever
// T is, per lane, then per wave (shuffles), per workgroup (LDS) and over the workgroups (k_pcg_reduce): the same
// order on every call - no atomics.  alpha and beta are doubles on the device, rounded to T once where applied.
#pragma once

#include "mgx_kernels.hpp"
#include "mgx_var.hpp"

namespace mgx {

// the device-side scalars of one solve (mgx_solver::pcg_sc)
enum { kPcgRho = 0, kPcgDelta, kPcgAlpha, kPcgBeta, kPcgGamma, kPcgRR, kPcgBreak, kPcgScalars = 8 };
enum { kPcgInit = 0, kPcgAlphaMode = 1, kPcgRRMode = 2, kPcgBetaMode = 3 };

// sum of a lane's products in double: a.x b.x + a.y b.y (+ a.z b.z + a.w b.w), pairwise like k_residual's sums
__device__ __forceinline__ double vdot(const double2& a, const double2& b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ double vdot(const float4& a, const float4& b)
{
    return ((double)a.x * (double)b.x + (double)a.y * (double)b.y) + ((double)a.z * (double)b.z + (double)a.w * (double)b.w);
}
__device__ __forceinline__ double2 vaxpy(const double2& x, double a, const double2& y) { return make_double2(x.x + a * y.x, x.y + a * y.y); }
__device__ __forceinline__ float4 vaxpy(const float4& x, float a, const float4& y)
{
    return make_float4(x.x + a * y.x, x.y + a * y.y, x.z + a * y.z, x.w + a * y.w);
}
__device__ __forceinline__ double2 vaxmy(const double2& x, double a, const double2& y) { return make_double2(x.x - a * y.x, x.y - a * y.y); }
__device__ __forceinline__ float4 vaxmy(const float4& x, float a, const float4& y)
{
    return make_float4(x.x - a * y.x, x.y - a * y.y, x.z - a * y.z, x.w - a * y.w);
}

// A u of the constant stencil, the operator of residual_vec: -(((N + W) + E) + S) + 4 u
__device__ __forceinline__ double2 poisson_vec(const double2& up, const double2& cur, const double2& dn)
{
    const double l = from_left(cur.y), r = from_right(cur.x);
    return make_double2(-nbr(up.x, l, cur.y, dn.x) + 4.0 * cur.x, -nbr(up.y, cur.x, r, dn.y) + 4.0 * cur.y);
}
__device__ __forceinline__ float4 poisson_vec(const float4& up, const float4& cur, const float4& dn)
{
    const NbrPairs t = nbr_pairs(up, cur, dn);
    const f32x2 p0 = {cur.x, cur.y}, p1 = {cur.z, cur.w};
    const f32x2 o0 = -t.t0 + 4.f * p0, o1 = -t.t1 + 4.f * p1;
    return make_float4(o0.x, o0.y, o1.x, o1.y);
}

// rho_new = r.z -> partial[b],  gamma = z.q -> partial[nb + b]   (nb = gridDim.x)
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_pcg_dots(const T* __restrict__ r, const T* __restrict__ z, const T* __restrict__ q, double* __restrict__ partial,
           int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[2][kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double rz = 0.0, zq = 0.0;
    if (t.active) {
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        if (c.st) {
            for (int y = r0; y < r1; ++y) {
                const long at = c.col + (long)y * pitch;
                const V rr = vload<V>(r + at, true), zz = vload<V>(z + at, true), qq = vload<V>(q + at, true);
                rz += vdot(rr, zz);
                zq += vdot(zz, qq);
            }
        }
    }
    block_reduce<kWavesPerBlock>(rz, wsum[0], partial + blockIdx.x, ReduceSum{});
    block_reduce<kWavesPerBlock>(zq, wsum[1], partial + (long)gridDim.x + blockIdx.x, ReduceSum{});
}

// p' = z + beta p (first_it: p' = z, p not read), q = A p', delta partials p'.q.  A lane forms p' of its row
// neighbours from z and p as it marches down (rows r0-1 .. r1), its column neighbours come from the adjacent lanes.
// OP 0: the constant five-point stencil in the order of residual_vec (A u = -(((N + W) + E) + S) + 4 u);
// OP 1: the level's five coefficient grids a, in the order of stencil_sum<5>().
template <typename T, int OP>
__global__ void __launch_bounds__(kBlock)
k_pcg_direction(const T* __restrict__ z, const T* __restrict__ p, T* __restrict__ pn, T* __restrict__ q,
                const double* __restrict__ sc, int first_it, double* __restrict__ partial, Op9<T> a,
                int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double acc = 0.0;
    if (t.active) {
        const T beta = first_it ? (T)0 : (T)sc[kPcgBeta];
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        // rows 0 and N are the Dirichlet ring: p' = 0 there without a load
        auto prow = [&](int y) -> V {
            const bool in = c.ld && y >= 1 && y < N;
            const long at = c.col + (long)y * pitch;
            V v = vload<V>(z + at, in);
            if (!first_it) v = vaxpy(v, beta, vload<V>(p + at, in));
            mask_cols(v, c.col, N);
            return v;
        };
        V up = prow(r0 - 1);
        V cur = prow(r0);
        for (int y = r0; y < r1; ++y) {
            const V dn = prow(y + 1);
            const long at = c.col + (long)y * pitch;
            V o;
            if constexpr (OP == 0) {
                o = poisson_vec(up, cur, dn);
            } else {
                Lanes<T> k[9];
                load_coefs<5, 0>(a, at, c.ld, k);
                Rows3<T> u{to_lanes(up), to_lanes(cur), to_lanes(dn)};
                u.cl = from_left(last(cur)); u.cr = from_right(first(cur));
                o = from_lanes(stencil_sum<5>(u, k, [&](int x) { return k[0].a[x]; }));
            }
            mask_cols(o, c.col, N);
            vstore<V>(pn + at, cur, c.st);
            vstore<V>(q + at, o, c.st);
            if (c.st) acc += vdot(cur, o);
            up = cur; cur = dn;
        }
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

// x += alpha p, r -= alpha q, partials of ||r||^2.  After a breakdown (sc[kPcgBreak] != 0) nothing is updated.
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_pcg_update(T* __restrict__ x, const T* __restrict__ p, T* __restrict__ r, const T* __restrict__ q,
             const double* __restrict__ sc, double* __restrict__ partial, int N, long pitch, int R, int strips, int chunks)
{
    using V = typename VecOf<T>::type;
    constexpr int W = VecOf<T>::W;
    __shared__ double wsum[kWavesPerBlock];
    const Tile t = wave_tile(strips, chunks);
    double acc = 0.0;
    if (t.active && sc[kPcgBreak] == 0.0) {
        const T alpha = (T)sc[kPcgAlpha];
        const Cols c = lane_cols<W>(t.strip, N, pitch);
        const int r0 = 1 + t.chunk * R;
        const int r1 = min(r0 + R, N);
        if (c.st) {
            for (int y = r0; y < r1; ++y) {
                const long at = c.col + (long)y * pitch;
                const V xx = vaxpy(vload<V>(x + at, true), alpha, vload<V>(p + at, true));
                const V rr = vaxmy(vload<V>(r + at, true), alpha, vload<V>(q + at, true));
                vstore<V>(x + at, xx, true);
                vstore<V>(r + at, rr, true);
                acc += vdot(rr, rr);
            }
        }
    }
    block_reduce<kWavesPerBlock>(acc, wsum, partial + blockIdx.x, ReduceSum{});
}

// fixed-order sum of n partials (the order of k_reduce_partials)
__device__ __forceinline__ double pcg_reduce_sum(const double* __restrict__ part, int n, double* wsum)
{
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int i = threadIdx.x;
    for (; i + 3 * kReduceThreads < n; i += 4 * kReduceThreads) {
        a0 += part[i];
        a1 += part[i + kReduceThreads];
        a2 += part[i + 2 * kReduceThreads];
        a3 += part[i + 3 * kReduceThreads];
    }
    for (; i < n; i += kReduceThreads) a0 += part[i];
    double acc = (a0 + a1) + (a2 + a3);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, kWave);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < kReduceThreads / kWave; ++w) s += wsum[w];
    return s;                                   // the same value in every thread
}

// one workgroup: the partials of the pass just run and the scalars that follow from them
//   kPcgInit:       rho = r.z, beta = 0, no breakdown
//   kPcgAlphaMode:  delta = p.q; alpha = rho / delta, or a breakdown (delta not > 0 or not finite: alpha = 0)
//   kPcgRRMode:     ||r||^2
//   kPcgBetaMode:   rho_new = r.z, gamma = z.q; beta = -alpha gamma / rho; rho = rho_new
__global__ void __launch_bounds__(kReduceThreads) k_pcg_reduce(const double* __restrict__ part, int n, int mode, double* __restrict__ sc)
{
    __shared__ double wsum[kReduceThreads / kWave];
    const double s0 = pcg_reduce_sum(part, n, wsum);
    const double s1 = (mode == kPcgBetaMode) ? pcg_reduce_sum(part + n, n, wsum) : 0.0;
    if (threadIdx.x != 0) return;
    if (mode == kPcgInit) {
        sc[kPcgRho] = s0; sc[kPcgBeta] = 0.0; sc[kPcgBreak] = 0.0;
    } else if (mode == kPcgAlphaMode) {
        sc[kPcgDelta] = s0;
        const bool ok = (s0 > 0.0) && isfinite(s0);
        sc[kPcgAlpha] = ok ? sc[kPcgRho] / s0 : 0.0;
        sc[kPcgBreak] = ok ? 0.0 : 1.0;
    } else if (mode == kPcgRRMode) {
        sc[kPcgRR] = s0;
    } else {
        sc[kPcgGamma] = s1;
        sc[kPcgBeta] = -sc[kPcgAlpha] * s1 / sc[kPcgRho];
        sc[kPcgRho] = s0;
    }
}

} // namespace mgx
