// mgx_krylov_host.hpp - the host side of mgx_solve_pcg and mgx_solve_gcr (absent in the reference; the passes and
// their arithmetic are mgx_krylov.hpp's).  Included by mgx.hip after the single-GPU solver:
// it uses cycle_body, residual_norm_grid, residual_level, finish_solve and time_on_stream of its anonymous namespace.
//
// One workspace (mgx_solver::kry), one driver (krylov_run) and one entry-point body (krylov_solve) serve these two and
// mgx_solve_refine_gcr (mgx_refine_host.hpp).  A method is a struct with T, name, quantity, prepare, precondition and
// enqueue: what it allocates beyond the shared pieces and sets before the solve, z = M r of iteration k, and the
// passes after it, up to and including the reduction of ||r||^2.
//
// The passes run on a KrylovView: where the Krylov state of one right-hand side lives.  The handle's own workspace and
// every column of mgx_solve_multi_gcr (mgx_multi_host.hpp) go through the same launches.
#pragma once

// *p = `bytes` of device memory, zeroed on the handle's stream (the ring and the padding of a grid stay zero from there
// on).  On any failure *p is freed and null and the sticky error is cleared: whatever existed before is as it was
static bool alloc_zeroed(mgx_solver* s, void** p, size_t bytes)
{
    if (hipMalloc(p, bytes) != hipSuccess) { *p = nullptr; (void)hipGetLastError(); return false; }
    if (hipMemsetAsync(*p, 0, bytes, s->stream) == hipSuccess) return true;
    (void)hipGetLastError();
    (void)hipStreamSynchronize(s->stream);
    (void)hipFree(*p);
    *p = nullptr;
    return false;
}

// ---- the workspace ----------------------------------------------------------------------------------------------------
// fine-level vectors, each allocated once and zeroed
int mgx_solver::KrylovWs::vecs(mgx_solver* s, std::initializer_list<void**> vs, size_t bytes)
{
    for (void** v : vs)
        if (!*v && !alloc_zeroed(s, v, bytes)) return s->fail(MGX_ERR_ALLOC, "hipMalloc failed for the Krylov vectors");
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

// ---- where the Krylov state of one right-hand side lives ----------------------------------------------------------------
struct KrylovView {
    void *x, *r;                    // the iterate; the residual, which is the cycle's right-hand side of the finest level
    void *const *Z, *const *Q;      // the kGcrMaxRestart basis slots
    double *sc, *part;              // the scalar block; the per-block partials of one pass
};

// the handle's own workspace: r lives in lv[finest].b
inline KrylovView krylov_view(mgx_solver* s)
{
    return {s->kry.x, s->lv[s->cfg.finest_level].b, s->kry.Z, s->kry.Q, s->kry.sc, s->kry.part};
}

// column c of s->multi: r lives in the column's finest b, its scalars are block c of gsc
inline KrylovView krylov_view(mgx_solver* s, int c)
{
    auto& w = s->multi;
    return {w.x[c], w.lv[s->cfg.finest_level].b[c], w.Z[c], w.Q[c], w.gsc + (size_t)c * kGcrScalars, w.gpart[c]};
}

// ---- the passes every method launches ----------------------------------------------------------------------------------
inline void krylov_reduce(mgx_solver* s, const KrylovView& v, int n, int mode)
{
    hipLaunchKernelGGL(k_pcg_reduce, dim3(1), dim3(kReduceThreads), 0, s->stream, v.part, n, mode, v.sc);
}

// pn = z + beta p (first: pn = z, p is not read), q = A pn on the handle's finest operator, the partials of pn.q
template <typename T>
void krylov_direction(mgx_solver* s, const KrylovView& v, const Level& l, const Launch& g, const T* z, const T* p, T* pn, T* q, bool first)
{
    if (s->var && l.nine)
        hipLaunchKernelGGL((k_pcg_direction<T, 2>), dim3(g.blocks), dim3(kBlock), 0, s->stream, z, p, pn, q, v.sc, first ? 1 : 0, v.part,
                           op9_of<T>(l), l.N, l.pitch, g.R, g.strips, g.chunks);
    else if (s->var)
        hipLaunchKernelGGL((k_pcg_direction<T, 1>), dim3(g.blocks), dim3(kBlock), 0, s->stream, z, p, pn, q, v.sc, first ? 1 : 0, v.part,
                           op9_of<T>(l), l.N, l.pitch, g.R, g.strips, g.chunks);
    else
        hipLaunchKernelGGL((k_pcg_direction<T, 0>), dim3(g.blocks), dim3(kBlock), 0, s->stream, z, p, pn, q, v.sc, first ? 1 : 0, v.part,
                           Op9<T>{}, l.N, l.pitch, g.R, g.strips, g.chunks);
}

// x += alpha p, r -= alpha q, the partials of ||r||^2
template <typename T>
void krylov_update(mgx_solver* s, const KrylovView& v, const Level& l, const Launch& g, const T* p, const T* q)
{
    hipLaunchKernelGGL((k_pcg_update<T>), dim3(g.blocks), dim3(kBlock), 0, s->stream, (T*)v.x, p, (T*)v.r, q, v.sc, v.part, l.N, l.pitch, g.R,
                       g.strips, g.chunks);
}

// ---- the GCR iteration after z = M r, on any view ------------------------------------------------------------------------
// the earlier pairs of an iteration, by value (slots that are not allocated are never read: J < restart)
template <typename T> GcrBasis<T> gcr_basis(const KrylovView& v)
{
    GcrBasis<T> bs{};
    for (int i = 0; i < kGcrMaxRestart - 1; ++i) { bs.Q[i] = (const T*)v.Q[i]; bs.Z[i] = (const T*)v.Z[i]; }
    return bs;
}

// the pair of slot j against the earlier pairs, alpha and the breakdown flag (mgx_krylov.hpp)
template <typename T>
void gcr_orth(mgx_solver* s, const KrylovView& v, const Level& l, const Launch& g, int j)
{
    launch_gcr_orth<T>(j, (T*)v.Q[j], (T*)v.Z[j], (const T*)v.r, gcr_basis<T>(v), v.sc, v.part, l.N, l.pitch, g, kGcrAllPasses, s->stream);
}

// x += alpha Z_j, r -= alpha Q_j and ||r||^2
template <typename T>
void gcr_update(mgx_solver* s, const KrylovView& v, const Level& l, const Launch& g, int j)
{
    krylov_update<T>(s, v, l, g, (const T*)v.Z[j], (const T*)v.Q[j]);
    krylov_reduce(s, v, g.blocks, kPcgRRMode);
}

// ---- what the host reads of an iteration -----------------------------------------------------------------------------------
// the scalar block h after the iteration's last reduction: broke down (value: the quantity that is not positive and
// finite), or ||r||
struct KrylovStep { bool broke; double value; };
inline KrylovStep krylov_step(const double* h)
{
    return h[kPcgBreak] != 0.0 ? KrylovStep{true, h[kPcgDelta]} : KrylovStep{false, std::sqrt(h[kPcgRR])};
}

// who: what broke down, with the entry point and the column where the caller's message names them ("GCR")
inline std::string breakdown_message(const std::string& who, int iteration, const char* quantity, double value)
{
    char msg[256];
    std::snprintf(msg, sizeof msg, "%s breakdown at iteration %d: %s = %.17g is not a positive finite number", who.c_str(), iteration, quantity,
                  value);
    return msg;
}

// z = M r: one cycle of the handle from zero, into lv[finest].u
inline int krylov_cycle(mgx_solver* s)
{
    double unused = 0.0;
    return cycle_body(s, false, true, &unused);
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
    int precondition(mgx_solver* s, const Level&, int, const std::vector<double>&) { return krylov_cycle(s); }
    void enqueue(mgx_solver* s, const Level& l, const Launch& g, int k, const std::vector<double>&)
    {
        mgx_solver::KrylovWs& w = s->kry;
        const KrylovView v = krylov_view(s);
        // rho_new = r.z, gamma = z.q (r = B, z = U of the finest level); k = 0: rho = r.z alone (p' = z below)
        hipLaunchKernelGGL((k_pcg_dots<T>), dim3(g.blocks), dim3(kBlock), 0, s->stream, (const T*)l.b, (const T*)l.u, (const T*)w.q, w.part, l.N,
                           l.pitch, g.R, g.strips, g.chunks);
        krylov_reduce(s, v, g.blocks, k == 0 ? kPcgInit : kPcgBetaMode);  // beta = -alpha z.q / rho, rho = r.z
        // p' = z + beta p, q = A p', alpha = rho / p'.q; then x += alpha p', r -= alpha q and ||r||^2
        T* pn = (T*)w.p[pp ^ 1];
        krylov_direction<T>(s, v, l, g, (const T*)l.u, (const T*)w.p[pp], pn, (T*)w.q, k == 0);
        krylov_reduce(s, v, g.blocks, kPcgAlphaMode);
        pp ^= 1;
        krylov_update<T>(s, v, l, g, (const T*)pn, (const T*)w.q);
        krylov_reduce(s, v, g.blocks, kPcgRRMode);
    }
};

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
    int precondition(mgx_solver* s, const Level&, int, const std::vector<double>&) { return krylov_cycle(s); }
    void enqueue(mgx_solver* s, const Level& l, const Launch& g, int k, const std::vector<double>&)
    {
        const KrylovView v = krylov_view(s);
        const int j = k % restart;
        // Z_j = z (out of lv.u), Q_j = A z: k_pcg_direction's first iteration (its own partials z.q are not used)
        krylov_direction<T>(s, v, l, g, (const T*)l.u, (const T*)l.u, (T*)v.Z[j], (T*)v.Q[j], true);
        gcr_orth<T>(s, v, l, g, j);
        gcr_update<T>(s, v, l, g, j);
    }
};

// ---- the driver --------------------------------------------------------------------------------------------------------
// The iteration proper.  r lives in lv[L].b for the whole solve: it is the cycle's right-hand side, and the cached
// cycle graphs hold that pointer (they are keyed on the u / tmp pointers only).  x is in kry.x, the caller's b waits
// in kry.b.  The method sees the history so far: hist[0 .. k] when iteration k is preconditioned and enqueued.
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
        if ((rc = m.precondition(s, l, k, hist))) return rc;           // z = M r
        m.enqueue(s, l, g, k, hist);
        HIPCHK(s, hipGetLastError());
        HIPCHK(s, hipMemcpyAsync(w.sc_host, w.sc, kPcgScalars * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(s, hipStreamSynchronize(s->stream));                    // the one host synchronisation per iteration
        const KrylovStep st = krylov_step(w.sc_host);
        if (st.broke) {
            *breakdown = 1;
            s->err = breakdown_message(Method::name, k + 1, Method::quantity, st.value);
            return MGX_OK;
        }
        *iters = k + 1;
        hist.push_back(st.value);
        if (st.value <= tol * h0 || k + 1 == max_iters) break;
    }
    return MGX_OK;
}

// ---- the entry-point body ----------------------------------------------------------------------------------------------
// which handles mgx_solve_pcg and mgx_solve_gcr serve
inline int krylov_guard(mgx_solver* s, const char* fn)
{
    NO_DIST(s)
    if (s->mixed) return s->fail(MGX_ERR_STATE, std::string(fn) + ": dtype MIXED is not supported (F64 or F32 handles)");
    return MGX_OK;
}

// The Krylov entry points behind their argument lists.  fn: the entry point's name for the messages; guard(s, fn): which
// handles it serves; bad_args: what is wrong with the arguments only this entry point has (nullptr: nothing);
// cycle_of(s, &f) (nullptr: the handle itself): once the arguments and the operators have passed, makes the solver f
// ready whose cycle the method runs - its fine_updates go into the stats; make(T{}): the method for the handle's
// working type T.
template <typename Make>
int krylov_solve(mgx_solver* s, const char* fn, int (*guard)(mgx_solver*, const char*), const char* bad_args,
                 int (*cycle_of)(mgx_solver*, mgx_solver**), double tol, int max_iters, mgx_stats* stats, double* history, int history_cap,
                 Make make)
{
    if (!s) return MGX_ERR_INVALID;
    if (int rc = guard(s, fn)) return rc;
    if (max_iters < 0 || !(tol >= 0.0)) return s->fail(MGX_ERR_INVALID, std::string(fn) + ": tol >= 0 and max_iters >= 0 required");
    if (bad_args) return s->fail(MGX_ERR_INVALID, std::string(fn) + ": " + bad_args);
    if (int vr = var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level)) return vr;
    mgx_solver* f = s;
    if (cycle_of)
        if (int rc = cycle_of(s, &f)) return rc;
    Level& l = s->lv[s->cfg.finest_level];
    std::vector<double> hist;
    hist.reserve(max_iters + 1);
    s->fine_updates = 0.0;
    f->fine_updates = 0.0;
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
    finish_solve(stats, history, history_cap, hist, iters, !breakdown && hist.back() <= tol * hist.front(), t0, f->fine_updates);
    return MGX_OK;
}

// ---- mgx_time_gcr_pass -------------------------------------------------------------------------------------------------
// `repeats` launches of one pass between two events.  The scalar block is zeroed first (and stays zeroed), so every
// h_i and alpha is 0 and the update and orthogonalisation leave x, r and slot j as they are (finite values:
// v - 0 w = v); the direction pass rewrites slot j from lv.u, which no later solve reads before writing it
template <typename T>
int gcr_time_pass(mgx_solver* s, int pass, int j, int repeats, double* ms)
{
    Level& l = s->lv[s->cfg.finest_level];
    const Launch g = make_launch(l.N, VecOf<T>::W, l.N - 1, s->rows_per_chunk);
    const KrylovView v = krylov_view(s);
    const GcrBasis<T> bs = gcr_basis<T>(v);
    T *zj = (T*)v.Z[j], *qj = (T*)v.Q[j];
    HIPCHK(s, hipMemsetAsync(v.sc, 0, kGcrScalars * sizeof(double), s->stream));
    const int rc = time_on_stream(s, ms, [&] {
        for (int i = 0; i < repeats; ++i) {
            if (pass == MGX_GCR_PASS_UPDATE) krylov_update<T>(s, v, l, g, (const T*)zj, (const T*)qj);
            else if (pass == MGX_GCR_PASS_DIRECTION) krylov_direction<T>(s, v, l, g, (const T*)l.u, (const T*)l.u, zj, qj, true);
            else launch_gcr_orth<T>(j, qj, zj, (const T*)v.r, bs, v.sc, v.part, l.N, l.pitch, g,
                                    pass == MGX_GCR_PASS_DOTS ? kGcrDotsPass : kGcrOrthPass, s->stream);
        }
    });
    if (!rc) *ms /= repeats;
    return rc;
}

} // namespace
