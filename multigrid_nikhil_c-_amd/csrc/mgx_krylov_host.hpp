// mgx_krylov_host.hpp - the host side of mgx_solve_pcg and mgx_solve_gcr (absent in the reference; the passes and
// their arithmetic are mgx_krylov.hpp's).  Included by mgx.hip after the single-GPU solver:
// it uses cycle_body, residual_norm_grid, residual_level, finish_solve and time_on_stream of its anonymous namespace.
//
// One workspace (mgx_solver::kry), one driver (krylov_run) and one entry-point body (krylov_solve) serve both methods.
// A method is a struct with T, name, quantity, prepare and enqueue: what it allocates beyond the shared pieces and
// sets before the solve, and the passes of iteration k after the cycle z = M r, up to and including the reduction
// of ||r||^2.
#pragma once

// ---- the workspace ----------------------------------------------------------------------------------------------------
// fine-level vectors, each allocated once and zeroed
int mgx_solver::KrylovWs::vecs(mgx_solver* s, std::initializer_list<void**> vs, size_t bytes)
{
    for (void** v : vs) {
        if (*v) continue;
        if (hipMalloc(v, bytes) != hipSuccess) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for the Krylov vectors");
        HIPCHK(s, hipMemsetAsync(*v, 0, bytes, s->stream));            // the ring and the padding stay zero from here on
    }
    return MGX_OK;
}

// what every solve needs: x, the caller's b, the partial sums of a launch of `blocks` workgroups and the scalars
int mgx_solver::KrylovWs::shared(mgx_solver* s, size_t bytes, int blocks)
{
    if (int rc = vecs(s, {&x, &b}, bytes)) return rc;
    const long widest = (long)(mgx::kGcrMaxRestart - 1) * blocks;      // k_gcr_dots<T, 7> writes seven partials per workgroup
    if (!part) {
        part_cap = widest + 8;
        if (hipMalloc(&part, part_cap * sizeof(double)) != hipSuccess) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for the Krylov partial sums");
    }
    if (!sc && hipMalloc(&sc, mgx::kGcrScalars * sizeof(double)) != hipSuccess) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for the Krylov scalars");
    if (!sc_host && hipHostMalloc(&sc_host, mgx::kGcrScalars * sizeof(double)) != hipSuccess)
        return s->fail(MGX_ERR_ALLOC, "hipHostMalloc failed for the Krylov scalars");
    if (widest > part_cap) return s->fail(MGX_ERR_STATE, "Krylov partial-sum buffer smaller than its launch");
    return MGX_OK;
}

void mgx_solver::KrylovWs::free()
{
    for (void* v : {x, b, p[0], p[1], q, (void*)part, (void*)sc}) if (v) (void)hipFree(v);
    for (int i = 0; i < mgx::kGcrMaxRestart; ++i)
        for (void* v : {Z[i], Q[i]}) if (v) (void)hipFree(v);
    if (sc_host) (void)hipHostFree(sc_host);
    *this = KrylovWs{};
}

namespace {

// ---- the passes both methods launch ------------------------------------------------------------------------------------
inline void krylov_reduce(mgx_solver* s, int n, int mode)
{
    hipLaunchKernelGGL(k_pcg_reduce, dim3(1), dim3(kReduceThreads), 0, s->stream, s->kry.part, n, mode, s->kry.sc);
}

// pn = z + beta p (first: pn = z, p is not read), q = A pn on the handle's finest operator, the partials of pn.q
template <typename T>
void krylov_direction(mgx_solver* s, const Level& l, const Launch& g, const T* z, const T* p, T* pn, T* q, bool first)
{
    if (s->var && l.nine)
        hipLaunchKernelGGL((k_pcg_direction<T, 2>), dim3(g.blocks), dim3(kBlock), 0, s->stream, z, p, pn, q, s->kry.sc, first ? 1 : 0, s->kry.part,
                           op9_of<T>(l), l.N, l.pitch, g.R, g.strips, g.chunks);
    else if (s->var)
        hipLaunchKernelGGL((k_pcg_direction<T, 1>), dim3(g.blocks), dim3(kBlock), 0, s->stream, z, p, pn, q, s->kry.sc, first ? 1 : 0, s->kry.part,
                           op9_of<T>(l), l.N, l.pitch, g.R, g.strips, g.chunks);
    else
        hipLaunchKernelGGL((k_pcg_direction<T, 0>), dim3(g.blocks), dim3(kBlock), 0, s->stream, z, p, pn, q, s->kry.sc, first ? 1 : 0, s->kry.part,
                           Op9<T>{}, l.N, l.pitch, g.R, g.strips, g.chunks);
}

// x += alpha p, r -= alpha q (r in lv.b), the partials of ||r||^2
template <typename T>
void krylov_update(mgx_solver* s, const Level& l, const Launch& g, const T* p, const T* q)
{
    hipLaunchKernelGGL((k_pcg_update<T>), dim3(g.blocks), dim3(kBlock), 0, s->stream, (T*)s->kry.x, p, (T*)l.b, q, s->kry.sc, s->kry.part, l.N,
                       l.pitch, g.R, g.strips, g.chunks);
}

// ---- the methods -------------------------------------------------------------------------------------------------------
// flexible conjugate gradients (mgx_krylov.hpp's header)
template <typename T_>
struct PcgMethod {
    using T = T_;
    static constexpr const char* name = "PCG";
    static constexpr const char* quantity = "p.Ap";
    int pp = 0;                                                        // p = kry.p[pp], p' = kry.p[pp ^ 1]

    // (the scalars need nothing: the kPcgInit reduction writes rho, beta and the flag)
    int prepare(mgx_solver* s, size_t bytes) { return s->kry.vecs(s, {&s->kry.p[0], &s->kry.p[1], &s->kry.q}, bytes); }
    void enqueue(mgx_solver* s, const Level& l, const Launch& g, int k)
    {
        mgx_solver::KrylovWs& w = s->kry;
        // rho_new = r.z, gamma = z.q (r = B, z = U of the finest level); k = 0: rho = r.z alone (p' = z below)
        hipLaunchKernelGGL((k_pcg_dots<T>), dim3(g.blocks), dim3(kBlock), 0, s->stream, (const T*)l.b, (const T*)l.u, (const T*)w.q, w.part, l.N,
                           l.pitch, g.R, g.strips, g.chunks);
        krylov_reduce(s, g.blocks, k == 0 ? kPcgInit : kPcgBetaMode);  // beta = -alpha z.q / rho, rho = r.z
        // p' = z + beta p, q = A p', alpha = rho / p'.q; then x += alpha p', r -= alpha q and ||r||^2
        T* pn = (T*)w.p[pp ^ 1];
        krylov_direction<T>(s, l, g, (const T*)l.u, (const T*)w.p[pp], pn, (T*)w.q, k == 0);
        krylov_reduce(s, g.blocks, kPcgAlphaMode);
        pp ^= 1;
        krylov_update<T>(s, l, g, (const T*)pn, (const T*)w.q);
        krylov_reduce(s, g.blocks, kPcgRRMode);
    }
};

// the earlier pairs of an iteration, by value (slots that are not allocated are never read: J < restart)
template <typename T> GcrBasis<T> gcr_basis(const mgx_solver* s)
{
    GcrBasis<T> bs{};
    for (int i = 0; i < kGcrMaxRestart - 1; ++i) { bs.Q[i] = (const T*)s->kry.Q[i]; bs.Z[i] = (const T*)s->kry.Z[i]; }
    return bs;
}

// restarted GCR (mgx_krylov.hpp's header)
template <typename T_>
struct GcrMethod {
    using T = T_;
    static constexpr const char* name = "GCR";
    static constexpr const char* quantity = "q'.q'";
    int restart;

    int prepare(mgx_solver* s, size_t bytes)
    {
        for (int i = 0; i < restart; ++i)
            if (int rc = s->kry.vecs(s, {&s->kry.Z[i], &s->kry.Q[i]}, bytes)) return rc;
        HIPCHK(s, hipMemsetAsync(s->kry.sc, 0, kGcrScalars * sizeof(double), s->stream));
        return MGX_OK;
    }
    void enqueue(mgx_solver* s, const Level& l, const Launch& g, int k)
    {
        const int j = k % restart;
        T *zj = (T*)s->kry.Z[j], *qj = (T*)s->kry.Q[j];
        // Z_j = z (out of lv.u), Q_j = A z: k_pcg_direction's first iteration (its own partials z.q are not used)
        krylov_direction<T>(s, l, g, (const T*)l.u, (const T*)l.u, zj, qj, true);
        launch_gcr_orth<T>(j, qj, zj, (const T*)l.b, gcr_basis<T>(s), s->kry.sc, s->kry.part, l.N, l.pitch, g, kGcrAllPasses, s->stream);
        krylov_update<T>(s, l, g, (const T*)zj, (const T*)qj);
        krylov_reduce(s, g.blocks, kPcgRRMode);
    }
};

// ---- the driver --------------------------------------------------------------------------------------------------------
// The iteration proper.  r lives in lv[L].b for the whole solve: it is the cycle's right-hand side, and the cached
// cycle graphs hold that pointer (they are keyed on the u / tmp pointers only).  x is in kry.x, the caller's b waits
// in kry.b.
template <typename Method>
int krylov_run(mgx_solver* s, double tol, int max_iters, Method m, std::vector<double>& hist, int* iters, int* breakdown)
{
    using T = typename Method::T;
    mgx_solver::KrylovWs& w = s->kry;
    Level& l = s->lv[s->cfg.finest_level];
    const Launch g = make_launch(l.N, VecOf<T>::W, l.N - 1, s->rows_per_chunk);
    int rc = w.shared(s, l.bytes, g.blocks);
    if (!rc) rc = m.prepare(s, l.bytes);
    if (rc) return rc;
    HIPCHK(s, hipMemcpyAsync(w.x, l.u, l.bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(s, hipMemcpyAsync(w.b, l.b, l.bytes, hipMemcpyDeviceToDevice, s->stream));
    s->norm_blocks_ready = 0;
    double h0 = 0.0;
    if ((rc = residual_norm_grid(s, l, w.x, w.b, &h0, MGX_PROF_NORM_FINE))) return rc;
    hist.push_back(h0);
    if (h0 <= tol * h0 || max_iters == 0) return MGX_OK;               // (b = 0, u = 0: converged, nothing divided)
    residual_level<0>(s, l, w.x, w.b, l.b);                            // r = b - A x, into lv[L].b
    for (int k = 0; k < max_iters; ++k) {
        double unused = 0.0;
        if ((rc = cycle_body(s, false, true, &unused))) return rc;     // z = M r: one cycle from zero, into lv[L].u
        m.enqueue(s, l, g, k);
        HIPCHK(s, hipGetLastError());
        HIPCHK(s, hipMemcpyAsync(w.sc_host, w.sc, kPcgScalars * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(s, hipStreamSynchronize(s->stream));                    // the one host synchronisation per iteration
        if (w.sc_host[kPcgBreak] != 0.0) {
            *breakdown = 1;
            char msg[160];
            std::snprintf(msg, sizeof msg, "%s breakdown at iteration %d: %s = %.17g is not a positive finite number", Method::name, k + 1,
                          Method::quantity, w.sc_host[kPcgDelta]);
            s->err = msg;
            return MGX_OK;
        }
        *iters = k + 1;
        const double rn = std::sqrt(w.sc_host[kPcgRR]);
        hist.push_back(rn);
        if (rn <= tol * h0 || k + 1 == max_iters) break;
    }
    return MGX_OK;
}

// ---- the entry-point body ----------------------------------------------------------------------------------------------
// mgx_solve_pcg and mgx_solve_gcr behind their argument lists.  fn: the entry point's name for the messages; bad_args:
// what is wrong with the arguments only this entry point has (nullptr: nothing); make(T{}): the method for the
// handle's working type T.
template <typename Make>
int krylov_solve(mgx_solver* s, const char* fn, const char* bad_args, double tol, int max_iters, mgx_stats* stats, double* history,
                 int history_cap, Make make)
{
    if (!s) return MGX_ERR_INVALID;
    NO_DIST(s)
    if (s->mixed) return s->fail(MGX_ERR_STATE, std::string(fn) + ": dtype MIXED is not supported (F64 or F32 handles)");
    if (max_iters < 0 || !(tol >= 0.0)) return s->fail(MGX_ERR_INVALID, std::string(fn) + ": tol >= 0 and max_iters >= 0 required");
    if (bad_args) return s->fail(MGX_ERR_INVALID, std::string(fn) + ": " + bad_args);
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    Level& l = s->lv[s->cfg.finest_level];
    std::vector<double> hist;
    hist.reserve(max_iters + 1);
    s->fine_updates = 0.0;
    HIPCHK(s, hipStreamSynchronize(s->stream));
    const auto t0 = std::chrono::steady_clock::now();
    int iters = 0, breakdown = 0;
    const int rc = s->work_f64 ? krylov_run(s, tol, max_iters, make(double{}), hist, &iters, &breakdown)
                               : krylov_run(s, tol, max_iters, make(float{}), hist, &iters, &breakdown);
    // U = x, B = the caller's b again (also after a failure part way, where they were saved)
    if (s->kry.x && s->kry.b && !hist.empty()) {
        (void)hipMemcpyAsync(l.u, s->kry.x, l.bytes, hipMemcpyDeviceToDevice, s->stream);
        (void)hipMemcpyAsync(l.b, s->kry.b, l.bytes, hipMemcpyDeviceToDevice, s->stream);
    }
    s->norm_blocks_ready = 0;
    if (rc) return rc;
    HIPCHK(s, hipGetLastError());
    HIPCHK(s, hipStreamSynchronize(s->stream));
    finish_solve(stats, history, history_cap, hist, iters, !breakdown && hist.back() <= tol * hist.front(), t0, s->fine_updates);
    return MGX_OK;
}

// ---- mgx_time_gcr_pass -------------------------------------------------------------------------------------------------
// `repeats` launches of one pass between two events.  The scalar block is zeroed first (and stays zeroed), so every
// h_i and alpha is 0 and the update and orthogonalisation leave x, r and slot j as they are (finite values:
// v - 0 w = v); the direction pass rewrites slot j from lv.u, which no later solve reads before writing it
template <typename T>
int gcr_time_pass(mgx_solver* s, int pass, int j, int repeats, double* ms)
{
    mgx_solver::KrylovWs& w = s->kry;
    Level& l = s->lv[s->cfg.finest_level];
    const Launch g = make_launch(l.N, VecOf<T>::W, l.N - 1, s->rows_per_chunk);
    const GcrBasis<T> bs = gcr_basis<T>(s);
    T *zj = (T*)w.Z[j], *qj = (T*)w.Q[j];
    HIPCHK(s, hipMemsetAsync(w.sc, 0, kGcrScalars * sizeof(double), s->stream));
    const int rc = time_on_stream(s, ms, [&] {
        for (int i = 0; i < repeats; ++i) {
            if (pass == MGX_GCR_PASS_UPDATE) krylov_update<T>(s, l, g, (const T*)zj, (const T*)qj);
            else if (pass == MGX_GCR_PASS_DIRECTION) krylov_direction<T>(s, l, g, (const T*)l.u, (const T*)l.u, zj, qj, true);
            else launch_gcr_orth<T>(j, qj, zj, (const T*)l.b, bs, w.sc, w.part, l.N, l.pitch, g,
                                    pass == MGX_GCR_PASS_DOTS ? kGcrDotsPass : kGcrOrthPass, s->stream);
        }
    });
    if (!rc) *ms /= repeats;
    return rc;
}

} // namespace
