// mgx_bottom.hpp — exact coarsest-level solve on the GPU.
//
// Replaces MF:63-72 direct_solver (Eigen SparseLU on the host) called from
// MF:137-139 and MF:178-181; the first draft's PS:581-587 "solve" (mu1+mu2
// Jacobi sweeps) is kept only as MGX_BOTTOM_SMOOTH.
//
// The 5-point Dirichlet Laplacian on an n x n grid is diagonalised by the
// type-I discrete sine transform: with S_jk = sqrt(2/(n+1)) sin(pi j k/(n+1))
// (symmetric, S S = I) and lambda_ij = 4 sin^2(pi i/2(n+1)) + 4 sin^2(pi j/2(n+1)),
//     U = S ( (S B S) ./ lambda ) S .
// n <= 255, so the four n^3 products are ~8 MFLOP: two small launches of two products each, always
// in double whatever the level's storage type.  This is a direct solver (no
// iteration, no tolerance); the oracle uses banded Cholesky, an independent
// exact method, so agreement between the two checks both.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>
#include <type_traits>
#include <vector>

#include "mgx_phase_trace.hpp"

#ifndef MGX_DST_DEEP
#define MGX_DST_DEEP 32
#endif

namespace mgx {

// ---- the pieces of k_dst_pair ----------------------------------------------------------------------------------
// One column of a row-major array through a raw buffer descriptor: the lane's column offset in a VGPR (the out-of-range
// offset for a lane without a column: it reads 0 and touches no memory), the row offset in an SGPR - one vector
// instruction per load, where a pointer sum per load cost some twenty (1090 vector instructions per wave for 254
// multiply-add pairs).  The scalar offset takes no part in the range check: callers pass rows that exist.
constexpr unsigned kDstOob = 0xFFFFFF00u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dst_rsrc(const void* p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
template <typename E> __device__ __forceinline__ double dst_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff)
{
    if constexpr (sizeof(E) == 8) {
        const auto t = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0);
        return __hiloint2double(t[1], t[0]);
    } else {
        return (double)__int_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
    }
}
// rows k0 .. k0 + D - 1 of the lane's column; beyond the last row the last row again (loaded, never used)
template <typename E, int D>
__device__ __forceinline__ void dst_batch(double (&x)[D], __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned rowbytes, int k0, int n)
{
    const unsigned last = (unsigned)(n - 1) * rowbytes;
    unsigned off = (unsigned)k0 * rowbytes;
#pragma unroll
    for (int q = 0; q < D; ++q, off += rowbytes) x[q] = dst_load<E>(r, voff, min(off, last));
}
// acc += m[k] * x[k] over the first CNT rows of a batch, in k order: the product is rounded, then added (-ffp-contract=off)
template <int CNT, int D> __device__ __forceinline__ void dst_chain(double& acc, const double* m, const double (&x)[D])
{
#pragma unroll
    for (int q = 0; q < CNT; ++q) acc += m[q] * x[q];
}
// the last batch, rem <= D rows.  Levels have n = 2^L - 1: from L = 5 on the last batch is one row short of a whole one
// and runs as straight-line code; any other length takes a uniform branch per row (each waits for its own LDS read).
template <int D> __device__ __forceinline__ void dst_chain_last(double& acc, const double* m, const double (&x)[D], int rem)
{
    if (rem == D - 1) {
        dst_chain<D - 1>(acc, m, x);
    } else {
#pragma unroll
        for (int q = 0; q < D; ++q)
            if (q < rem) acc += m[q] * x[q];
    }
}
// sum_k m[k] x_k over k = 0 .. n-1, one accumulator, with the column x_k arriving D rows at a time through `load`.
// Software-pipelined over two register batches: the loads of batch t + 1 are in flight while the add chain of batch t
// runs (before, a wave issued D loads, waited for all of them, and then ran D dependent adds with nothing in flight).
// xa holds batch 0 on entry; `before_last` runs in front of the last batch's chain, when this sum has nothing left to
// load: the caller issues the NEXT sum's first batch there.
template <int D, typename Load, typename Before, typename Stamp>
__device__ __forceinline__ double dst_dot(const double* m, int n, double (&xa)[D], Load load, Before before_last, Stamp landed)
{
    double xb[D];
    double acc = 0.0;
    int k = 0;
    for (;;) {
        if (k + D >= n) { before_last(); landed(xa[D - 1]); dst_chain_last<D>(acc, m + k, xa, n - k); break; }
        load(xb, k + D);
        landed(xa[D - 1]);
        dst_chain<D, D>(acc, m + k, xa);
        k += D;
        if (k + D >= n) { before_last(); landed(xb[D - 1]); dst_chain_last<D>(acc, m + k, xb, n - k); break; }
        load(xa, k + D);
        landed(xb[D - 1]);
        dst_chain<D, D>(acc, m + k, xb);
        k += D;
    }
    return acc;
}

// Two of the four products per launch.  U = S ((S B S) ./ lambda) S is two row-local pairs - row i of (S B) S needs
// only row i of S B, row i of (S T) S only row i of S T - so one workgroup owns output row i: its threads j first form
// P[i][j] = sum_k S[i][k] X[k][j] (X the level's grid b, or the scaled transform T of the first launch), park the row
// in LDS, and then form sum_k P[i][k] S[k][j].  Every sum runs in k order with one accumulator, exactly the four
// products of the oracle's ORC_BOTTOM_DST (same bits as the four-launch form of rounds 1-2: 4 x 9 us -> 2 launches).
// The workgroup is n rounded up to whole waves (a wave without a column has nothing to do); row i of S is fetched
// once, one element per thread, and read from LDS like P's row in the second sum; the second sum's first batch of S
// is issued in front of the first sum's last chain (it does not depend on it).
//  FIRST: X is the padded grid of type T (element (k, j) at (k + 1, j + 1)); the result is divided by
//         s[i] + s[j] and written to the n x n double array `out`
//  else : X is the n x n double array; the result is written to the padded grid of type T
template <typename T, bool FIRST>
__global__ void __launch_bounds__(256)
k_dst_pair(const double* __restrict__ S, const void* __restrict__ Xv, void* __restrict__ Ov, const double* __restrict__ s,
           int n, long gpitch)
{
    using E = std::conditional_t<FIRST, T, double>;         // X's element type
    __shared__ double srow[256], prow[256];
    MGX_PHASE_BEGIN();
    const int j = threadIdx.x;
    const int i = blockIdx.x;
    const bool live = j < n;
    // the loads of a sum are independent of its accumulator: they are issued kDeep at a time (a 127-term dot
    // product is nothing but L2 latency otherwise; 64 deep measured slower: 98 against 86 us for the coarse part of the reference hierarchy)
    constexpr int kDeep = MGX_DST_DEEP;
    const unsigned srb = (unsigned)n * 8u, xrb = FIRST ? (unsigned)gpitch * (unsigned)sizeof(T) : srb;
    const char* xp = static_cast<const char*>(Xv) + (FIRST ? (gpitch + 1) * (long)sizeof(T) : 0L);
    const __amdgpu_buffer_rsrc_t rs = dst_rsrc(S, (unsigned)n * srb);
    const __amdgpu_buffer_rsrc_t rx = dst_rsrc(xp, (unsigned)(n - 1) * xrb + (unsigned)n * (unsigned)sizeof(E));
    const unsigned vs = live ? (unsigned)j * 8u : kDstOob, vx = live ? (unsigned)j * (unsigned)sizeof(E) : kDstOob;
    auto landed = [&](const double& v) { MGX_PHASE_AFTER(v); (void)v; };

    const double si = dst_load<double>(rs, vs, (unsigned)i * srb);      // S[i][j]
    double ei = 0.0, ej = 0.0;                                           // eigenvalue halves s[i], s[j]: fetched now, used last
    if constexpr (FIRST) {
        const __amdgpu_buffer_rsrc_t re = dst_rsrc(s, srb);
        ei = dst_load<double>(re, live ? 0u : kDstOob, (unsigned)i * 8u);
        ej = dst_load<double>(re, vs, 0u);
    }
    double xa[kDeep], s2[kDeep];
    dst_batch<E, kDeep>(xa, rx, vx, xrb, 0, n);
    srow[j] = si;
    __syncthreads();
    const double acc = dst_dot<kDeep>(srow, n, xa, [&](double (&x)[kDeep], int k0) { dst_batch<E, kDeep>(x, rx, vx, xrb, k0, n); },
                                      [&]() { dst_batch<double, kDeep>(s2, rs, vs, srb, 0, n); }, landed);
    MGX_PHASE_AFTER(acc);
    prow[j] = acc;
    __syncthreads();
    MGX_PHASE();
    const double out = dst_dot<kDeep>(prow, n, s2, [&](double (&x)[kDeep], int k0) { dst_batch<double, kDeep>(x, rs, vs, srb, k0, n); },
                                      []() {}, landed);
    MGX_PHASE_AFTER(out);
    if (live) {
        if constexpr (FIRST) reinterpret_cast<double*>(Ov)[(long)i * n + j] = out / (ei + ej);
        else reinterpret_cast<T*>(Ov)[(long)(i + 1) * gpitch + (j + 1)] = (T)out;
    }
    MGX_PHASE_END(kPhaseDst, n | (FIRST ? 1 << 16 : 0));
}

struct BottomDST {
    int n = 0;
    double* S = nullptr;      // n x n sine matrix
    double* s = nullptr;      // n eigenvalue halves: 4 sin^2(pi (i+1) / (2 (n+1)))
    double* w1 = nullptr;     // n x n: (S B S) ./ lambda between the two launches

    hipError_t init(int n_)
    {
        n = n_;
        const size_t nn = (size_t)n * n;
        std::vector<double> hS(nn), hs(n);
        const long double pi = 3.14159265358979323846264338327950288L;
        const long double norm = sqrtl(2.0L / (long double)(n + 1));
        for (int i = 0; i < n; ++i) {
            const long double a = sinl(pi * (long double)(i + 1) / (2.0L * (long double)(n + 1)));
            hs[i] = (double)(4.0L * a * a);
            for (int k = 0; k < n; ++k) {
                // reduce the argument exactly before calling sin
                const long m = ((long)(i + 1) * (long)(k + 1)) % (2L * (n + 1));
                hS[(size_t)i * n + k] = (double)(norm * sinl(pi * (long double)m / (long double)(n + 1)));
            }
        }
        hipError_t e;
        if ((e = hipMalloc(&S, nn * sizeof(double))) != hipSuccess) return e;
        if ((e = hipMalloc(&s, n * sizeof(double))) != hipSuccess) return e;
        if ((e = hipMalloc(&w1, nn * sizeof(double))) != hipSuccess) return e;
        if ((e = hipMemcpy(S, hS.data(), nn * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(s, hs.data(), n * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return e;
        return hipSuccess;
    }

    void destroy()
    {
        if (S) (void)hipFree(S);
        if (s) (void)hipFree(s);
        if (w1) (void)hipFree(w1);
        S = s = w1 = nullptr;
    }

    // u_grid = A^-1 b_grid on the padded coarsest-level grids (2 launches; w1 holds (S B S) ./ lambda in between)
    template <typename T>
    void solve(const T* b_grid, T* u_grid, long gpitch, hipStream_t st) const
    {
        const int block = (n + 63) / 64 * 64;       // n <= 255
        hipLaunchKernelGGL((k_dst_pair<T, true>), dim3(n), dim3(block), 0, st, S, (const void*)b_grid, (void*)w1, s, n, gpitch);
        hipLaunchKernelGGL((k_dst_pair<T, false>), dim3(n), dim3(block), 0, st, S, (const void*)w1, (void*)u_grid, s, n, gpitch);
    }
};

} // namespace mgx
