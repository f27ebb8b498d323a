// mgx_phase_trace.hpp — debug build only (make trace, -DMGX_WAVE_TRACE): where the time goes INSIDE the latency-bound
// kernels of the V-cycle's tail (k_dst_pair, k_tile_wide).  Wave 0 of every workgroup stamps the 100 MHz wall clock at
// its phase boundaries into LDS and appends one record per workgroup when it ends; tools/phase_trace.py reads the
// records back (mgx_debug_phase_trace) and prints the per-phase medians.  Without MGX_WAVE_TRACE every macro is empty:
// the production kernels do not change by one instruction.
#pragma once

#include <hip/hip_runtime.h>

#ifdef MGX_WAVE_TRACE
namespace mgx {

constexpr int kPhaseMax = 24;               // stamps per workgroup
constexpr int kPhaseCap = 1 << 14;          // records kept (a ring: the newest overwrite the oldest)
constexpr int kPhaseDst = 0, kPhaseTile = 1;
struct PhaseTrace { int kind, tag, block, n; long long t[kPhaseMax]; };
__device__ PhaseTrace g_phase_trace[kPhaseCap];
__device__ unsigned g_phase_trace_n;

__device__ __forceinline__ void phase_mark(long long* t, int& n)
{
    if (threadIdx.x < 64) {                 // wave 0
        const long long c = wall_clock64();
        if (threadIdx.x == 0 && n < kPhaseMax) t[n] = c;
    }
    ++n;
}
// the stamp follows the instruction that produces v (a load: after it has landed; a sum: after its last add)
template <typename X> __device__ __forceinline__ void phase_mark_after(long long* t, int& n, const X& v)
{
    asm volatile("" ::"v"(v) : "memory");
    phase_mark(t, n);
}
__device__ __forceinline__ void phase_flush(const long long* t, int n, int kind, int tag)
{
    if (threadIdx.x == 0) {
        PhaseTrace& r = g_phase_trace[atomicAdd(&g_phase_trace_n, 1u) & (kPhaseCap - 1)];
        r.kind = kind; r.tag = tag; r.block = (int)blockIdx.x; r.n = n < kPhaseMax ? n : kPhaseMax;
        for (int q = 0; q < r.n; ++q) r.t[q] = t[q];
    }
}

} // namespace mgx
#define MGX_PHASE_BEGIN() __shared__ long long ph_t[mgx::kPhaseMax]; int ph_n = 0; mgx::phase_mark(ph_t, ph_n)
#define MGX_PHASE() mgx::phase_mark(ph_t, ph_n)
#define MGX_PHASE_AFTER(v) mgx::phase_mark_after(ph_t, ph_n, (v))
#define MGX_PHASE_END(kind, tag) (mgx::phase_mark(ph_t, ph_n), mgx::phase_flush(ph_t, ph_n, (kind), (tag)))
#else
#define MGX_PHASE_BEGIN() ((void)0)
#define MGX_PHASE() ((void)0)
#define MGX_PHASE_AFTER(v) ((void)0)
#define MGX_PHASE_END(kind, tag) ((void)0)
#endif
