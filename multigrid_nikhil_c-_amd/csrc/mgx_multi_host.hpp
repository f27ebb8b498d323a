// mgx_multi_host.hpp - the host side of mgx_solve_multi and mgx_solve_multi_gcr (absent in the reference; the K-column
// kernels are mgx_multi.hpp's).  Included by mgx.hip after mgx_krylov_host.hpp.
// Here: the workspace of the columns (multi_ensure, multi_free*), their norms (multi_norms), which handles solve blocks
// (multi_guard), the frame of a block solve (MultiFrame) and the block GCR.  The cycle is mgx.hip's one walk (vcycle)
// on a MultiSet of these columns: wherever a coefficient is read the set runs one launch of the pass's K-column kernel,
// K = m - the kernel, launch helper and geometry of mgx_solve's own pass, which is its m = 1 call (mgx_var.hpp, COLUMNS) -
// and where none is (the bilinear transfers, the injection) the single-column kernel once per column.
#pragma once

namespace {

void multi_free_column(mgx_solver::MultiWs& w, int c)
{
    auto drop = [](std::initializer_list<void**> ps) {
        for (void** p : ps) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
    };
    for (auto& g : w.lv) drop({&g.u[c], &g.tmp[c], &g.b[c], &g.r[c]});
    drop({(void**)&w.part[c], &w.x[c], (void**)&w.gpart[c]});
    for (int i = 0; i < kGcrMaxRestart; ++i) drop({&w.Z[c][i], &w.Q[c][i]});
}

void multi_free(mgx_solver::MultiWs& w)
{
    for (int c = 0; c < MGX_MAX_RHS; ++c) multi_free_column(w, c);
    if (w.sums) (void)hipFree(w.sums);
    if (w.sums_host) (void)hipHostFree(w.sums_host);
    w.sums = w.sums_host = nullptr;
    if (w.gsc) (void)hipFree(w.gsc);
    if (w.gsc_host) (void)hipHostFree(w.gsc_host);
    w.gsc = w.gsc_host = nullptr;
    w.cols = 0;
}

// columns [0, nrhs) of the workspace exist afterwards.  A failure frees the column it was allocating and leaves the
// columns that existed: the handle and the smaller workspace stay usable
int multi_ensure(mgx_solver* s, int nrhs)
{
    auto& w = s->multi;
    const int lo = s->cfg.coarsest_level, hi = s->cfg.finest_level;
    if (w.lv.empty()) w.lv.resize(s->lv.size());
    if (!w.sums && hipMalloc((void**)&w.sums, MGX_MAX_RHS * sizeof(double)) != hipSuccess) {
        w.sums = nullptr;
        return s->fail(MGX_ERR_ALLOC, "mgx_solve_multi: hipMalloc failed for the column sums");
    }
    if (!w.sums_host && hipHostMalloc((void**)&w.sums_host, MGX_MAX_RHS * sizeof(double)) != hipSuccess) {
        w.sums_host = nullptr;
        return s->fail(MGX_ERR_ALLOC, "mgx_solve_multi: hipHostMalloc failed for the column sums");
    }
    const Level& f = s->lv[hi];
    const size_t blocks = (size_t)make_launch(f.N, f.f64 ? 2 : 4, f.N - 1, 1).blocks;
    for (int c = w.cols; c < nrhs; ++c) {
        bool ok = hipMalloc((void**)&w.part[c], blocks * sizeof(double)) == hipSuccess;
        if (!ok) w.part[c] = nullptr;
        for (int l = lo; ok && l <= hi; ++l)
            for (void** p : {&w.lv[l].u[c], &w.lv[l].tmp[c], &w.lv[l].b[c], &w.lv[l].r[c]})
                if (!(ok = alloc_zeroed(s, p, s->lv[l].bytes))) break;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(s->stream);
            multi_free_column(w, c);
            return s->fail(MGX_ERR_ALLOC, "mgx_solve_multi: hipMalloc failed for the arrays of column " + std::to_string(c));
        }
        w.cols = c + 1;
    }
    return MGX_OK;
}

// ||b_j - A u_j|| of the set's columns on the finest level into r[column]: one copy, one host synchronisation
template <typename T>
int multi_norms(mgx_solver* s, const MultiSet& a, double* r)
{
    residual_set<T, 1>(s, s->cfg.finest_level, a);
    HIPCHK(s, hipMemcpyAsync(s->multi.sums_host, s->multi.sums, MGX_MAX_RHS * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    for (int j = 0; j < a.m; ++j) r[a.act[j]] = std::sqrt(s->multi.sums_host[a.act[j]]);
    return MGX_OK;
}

// which handles solve blocks of right-hand sides (the message names the reason); then the operators must be set / built
int multi_guard(mgx_solver* s, const char* fn)
{
    const std::string f(fn);
    if (s->dist) return s->fail(MGX_ERR_STATE, f + ": not available on a multi-GPU handle (see mgx.h, Multi-GPU)");
    if (!s->var)
        return s->fail(MGX_ERR_STATE, f + ": op = MGX_OPERATOR_POISSON kernels read no coefficient grids, there is nothing for the columns to "
                                          "share; this entry point is for MGX_OPERATOR_STENCIL5 and MGX_OPERATOR_GALERKIN");
    if (s->mixed) return s->fail(MGX_ERR_STATE, f + ": dtype MIXED is not supported (F64 or F32)");
    if (s->cfg.smoother != MGX_SMOOTHER_JACOBI)
        return s->fail(MGX_ERR_STATE, f + ": smoother MGX_SMOOTHER_JACOBI only (multi-column Chebyshev, line and colour smoothers are a follow-up)");
    return var_ready(s, s->cfg.coarsest_level, s->cfg.finest_level);
}

// ---- the frame of a block solve: what mgx_solve_multi, mgx_solve_multi_gcr and mgx_solve_multi_refine_gcr
// (mgx_multi_refine_host.hpp) do around their loops -----------------------------------------------------------------------
template <typename T>
struct MultiFrame {
    mgx_solver* s;
    int nrhs;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<double> hist[MGX_MAX_RHS];
    double fu[MGX_MAX_RHS] = {};
    int iters[MGX_MAX_RHS] = {}, broke[MGX_MAX_RHS] = {};

    Level& fine() const { return s->lv[s->cfg.finest_level]; }
    size_t nn() const { return (size_t)(fine().N - 1) * (size_t)(fine().N - 1); }
    // the caller's b and u into the finest b and u of the columns (which exist); hist[j][0] = ||b_j - A u_j||
    int begin(const void* b, const void* u, int max_iters)
    {
        auto& w = s->multi.lv[s->cfg.finest_level];
        for (int j = 0; j < nrhs; ++j) {
            if (int rc = copy_in(s, fine(), w.b[j], (const T*)b + (size_t)j * nn(), nn())) return rc;
            if (int rc = copy_in(s, fine(), w.u[j], (const T*)u + (size_t)j * nn(), nn())) return rc;
        }
        double r[MGX_MAX_RHS] = {};
        if (int rc = multi_norms<T>(s, multi_all(nrhs), r)) return rc;
        for (int j = 0; j < nrhs; ++j) {
            hist[j].reserve(max_iters + 1);
            hist[j].push_back(r[j]);
        }
        return MGX_OK;
    }

    // the columns of `a` that go on: a column leaves the set for good as soon as it breaks down or its history meets the
    // tolerance, and nothing reads or writes it again
    MultiSet active(const MultiSet& a, double tol) const
    {
        MultiSet next{};
        for (int i = 0; i < a.m; ++i) {
            const int j = a.act[i];
            if (!broke[j] && !(hist[j].back() <= tol * hist[j][0])) next.act[next.m++] = j;
        }
        return next;
    }

    // what the host reads of GCR iteration k of the set (each column's passes up to the reduction of ||r||^2 are
    // enqueued): the scalar blocks of all columns in one copy and one host synchronisation, then per column a breakdown
    // (fn and the column go into first_break, which keeps the first) or the next history entry
    int gcr_step(const MultiSet& a, int k, const char* fn, const char* quantity, std::string& first_break)
    {
        auto& ws = s->multi;
        HIPCHK(s, hipGetLastError());
        HIPCHK(s, hipMemcpyAsync(ws.gsc_host, ws.gsc, (size_t)nrhs * kGcrScalars * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(s, hipStreamSynchronize(s->stream));                        // the one host synchronisation per iteration
        for (int i = 0; i < a.m; ++i) {
            const int c = a.act[i];
            const KrylovStep st = krylov_step(ws.gsc_host + (size_t)c * kGcrScalars);
            if (st.broke) {
                broke[c] = 1;
                if (first_break.empty())
                    first_break = breakdown_message(std::string(fn) + ": column " + std::to_string(c) + ": GCR", k + 1, quantity, st.value);
                continue;
            }
            iters[c] = k + 1;
            hist[c].push_back(st.value);
        }
        return MGX_OK;
    }

    // the iterates out of src[column] into the caller's u, the statistics and histories, one `seconds` for all columns
    int finish(void* const* src, void* u, double tol, mgx_stats* stats, double* history, int history_cap)
    {
        HIPCHK(s, hipGetLastError());
        HIPCHK(s, hipStreamSynchronize(s->stream));
        for (int j = 0; j < nrhs; ++j)
            if (int rc = copy_out(s, fine(), src[j], (T*)u + (size_t)j * nn(), nn())) return rc;
        for (int j = 0; j < nrhs; ++j)
            finish_solve(stats ? stats + j : nullptr, history ? history + (size_t)j * (size_t)history_cap : nullptr, history_cap, hist[j], iters[j],
                         !broke[j] && hist[j].back() <= tol * hist[j].front(), t0, fu[j]);
        if (stats) {
            const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            for (int j = 0; j < nrhs; ++j) stats[j].seconds = seconds;
        }
        return MGX_OK;
    }
};

template <typename T>
int multi_solve_t(mgx_solver* s, int nrhs, const void* b, void* u, double tol, int max_cycles, mgx_stats* stats, double* history, int history_cap)
{
    MultiFrame<T> fr{s, nrhs};
    if (int rc = multi_ensure(s, nrhs)) return rc;
    if (int rc = fr.begin(b, u, max_cycles)) return rc;
    const int L = s->cfg.finest_level;
    MultiSet a = multi_all(nrhs);
    for (int k = 0; k < max_cycles; ++k) {
        a = fr.active(a, tol);
        if (a.m == 0) break;
        vcycle(s, L, false, 0, s->cycle, a, fr.fu);
        double r[MGX_MAX_RHS] = {};
        if (int rc = multi_norms<T>(s, a, r)) return rc;
        for (int i = 0; i < a.m; ++i) { fr.hist[a.act[i]].push_back(r[a.act[i]]); fr.iters[a.act[i]] = k + 1; }
    }
    return fr.finish(s->multi.lv[L].u, u, tol, stats, history, history_cap);
}

// ---- mgx_solve_multi_gcr: GcrMethod's passes (mgx_krylov_host.hpp) on the view of every active column, around the block cycle ----
// the geometry of every Krylov pass, krylov_run's: the per-block partial sums set the summation order
template <typename T> Launch multi_gcr_launch(const mgx_solver* s)
{
    const Level& l = s->lv[s->cfg.finest_level];
    return make_launch(l.N, VecOf<T>::W, l.N - 1, s->rows_per_chunk);
}

// the Krylov pieces of columns [0, nrhs) with `restart` basis pairs each exist afterwards (multi_ensure has made the
// columns).  Every piece is allocated once, by the first call that needs it; a failure leaves what existed
int multi_gcr_ensure(mgx_solver* s, int nrhs, int restart, int blocks)
{
    auto& w = s->multi;
    const Level& l = s->lv[s->cfg.finest_level];
    if (!w.gsc && hipMalloc((void**)&w.gsc, MGX_MAX_RHS * kGcrScalars * sizeof(double)) != hipSuccess) {
        w.gsc = nullptr;
        (void)hipGetLastError();
        return s->fail(MGX_ERR_ALLOC, "mgx_solve_multi_gcr: hipMalloc failed for the column scalars");
    }
    if (!w.gsc_host && hipHostMalloc((void**)&w.gsc_host, MGX_MAX_RHS * kGcrScalars * sizeof(double)) != hipSuccess) {
        w.gsc_host = nullptr;
        (void)hipGetLastError();
        return s->fail(MGX_ERR_ALLOC, "mgx_solve_multi_gcr: hipHostMalloc failed for the column scalars");
    }
    for (int c = 0; c < nrhs; ++c) {
        // k_gcr_dots<T, 7> writes seven partials per workgroup (KrylovWs::shared)
        if (!w.gpart[c] && hipMalloc((void**)&w.gpart[c], ((size_t)(kGcrMaxRestart - 1) * blocks + 8) * sizeof(double)) != hipSuccess) {
            w.gpart[c] = nullptr;
            (void)hipGetLastError();
            return s->fail(MGX_ERR_ALLOC, "mgx_solve_multi_gcr: hipMalloc failed for the partial sums of column " + std::to_string(c));
        }
        auto vec = [&](void** p) { return *p || alloc_zeroed(s, p, l.bytes); };
        bool ok = vec(&w.x[c]);
        for (int i = 0; ok && i < restart; ++i) ok = vec(&w.Z[c][i]) && vec(&w.Q[c][i]);
        if (!ok) return s->fail(MGX_ERR_ALLOC, "mgx_solve_multi_gcr: hipMalloc failed for the Krylov vectors of column " + std::to_string(c));
    }
    return MGX_OK;
}

// Z_c[j] = z_c (the finest u of the column), Q_c[j] = A z_c for the columns of the set: one launch, the operator read once
template <typename T>
void multi_gcr_direction(mgx_solver* s, const MultiSet& a, int j, const Launch& g)
{
    const Level& l = s->lv[s->cfg.finest_level];
    auto& ws = s->multi;
    auto& w = ws.lv[s->cfg.finest_level];
    if (a.m == 1) {
        // k_pcg_direction's first iteration, as mgx_solve_gcr launches it (its partials z.q go where nothing reads them);
        // that kernel also forms those partials, so it is not the K = 1 form of k_gcr_direction_multi
        const KrylovView v = krylov_view(s, a.act[0]);
        krylov_direction<T>(s, v, l, g, (const T*)w.u[a.act[0]], (const T*)w.u[a.act[0]], (T*)v.Z[j], (T*)v.Q[j], true);
        return;
    }
    const T* z[MGX_MAX_RHS];
    T *zo[MGX_MAX_RHS], *q[MGX_MAX_RHS];
    for (int i = 0; i < a.m; ++i) {
        const int c = a.act[i];
        z[i] = (const T*)w.u[c]; zo[i] = (T*)ws.Z[c][j]; q[i] = (T*)ws.Q[c][j];
    }
    launch_gcr_direction_multi<T>(a.m, l.nine, z, zo, q, op9_of<T>(l), l.N, l.pitch, g, s->stream);
}

template <typename T>
int multi_gcr_solve_t(mgx_solver* s, int nrhs, const void* b, void* u, double tol, int max_iters, int restart, mgx_stats* stats,
                      double* history, int history_cap)
{
    MultiFrame<T> fr{s, nrhs};
    const Launch g = multi_gcr_launch<T>(s);
    if (int rc = multi_ensure(s, nrhs)) return rc;
    if (int rc = multi_gcr_ensure(s, nrhs, restart, g.blocks)) return rc;
    if (int rc = fr.begin(b, u, max_iters)) return rc;
    const int L = s->cfg.finest_level;
    Level& l = s->lv[L];
    auto& ws = s->multi;
    auto& w = ws.lv[L];
    // x_j: the guess, which a column that never iterates returns (b = 0, u = 0: converged, nothing divided)
    for (int j = 0; j < nrhs; ++j) HIPCHK(s, hipMemcpyAsync(ws.x[j], w.u[j], l.bytes, hipMemcpyDeviceToDevice, s->stream));
    MultiSet a = max_iters > 0 ? fr.active(multi_all(nrhs), tol) : MultiSet{};
    if (a.m > 0) {
        // r_j = b_j - A x_j becomes the cycle's right-hand side of the finest level for the whole solve (the caller's b is
        // on the host: nothing to restore); the scalar blocks start from zero, as GcrMethod::prepare leaves them
        residual_set<T, 0>(s, L, a);
        for (int i = 0; i < a.m; ++i) std::swap(w.b[a.act[i]], w.r[a.act[i]]);
        HIPCHK(s, hipMemsetAsync(ws.gsc, 0, MGX_MAX_RHS * kGcrScalars * sizeof(double), s->stream));
    }
    // zero_start_u: a one-level hierarchy starts its cycle from what the finest u holds (the guess, then the last z)
    const bool zero_start = L > s->cfg.coarsest_level;
    std::string first_break;
    for (int k = 0; k < max_iters && a.m > 0; ++k) {
        const int j = k % restart;
        if (int rc = zero_start ? zero_u(s, L, a) : MGX_OK) return rc;
        vcycle(s, L, false, 0, s->cycle, a, fr.fu);                        // z_c = M r_c, into the finest u of the column
        multi_gcr_direction<T>(s, a, j, g);
        for (int i = 0; i < a.m; ++i) {
            const KrylovView v = krylov_view(s, a.act[i]);
            gcr_orth<T>(s, v, l, g, j);
            gcr_update<T>(s, v, l, g, j);
        }
        if (int rc = fr.gcr_step(a, k, "mgx_solve_multi_gcr", GcrMethod<T>::quantity, first_break)) return rc;
        a = fr.active(a, tol);
    }
    if (int rc = fr.finish(ws.x, u, tol, stats, history, history_cap)) return rc;
    if (!first_break.empty()) s->err = first_break;
    return MGX_OK;
}

// mgx_time_multi_gcr_direction: `repeats` launches of the direction pass on the first nrhs columns, from the finest u of
// each into its basis slot 0 (which has no meaning between two solves)
template <typename T>
int multi_gcr_time_direction(mgx_solver* s, int nrhs, int repeats, double* ms)
{
    const Launch g = multi_gcr_launch<T>(s);
    const MultiSet a = multi_all(nrhs);
    const int rc = time_on_stream(s, ms, [&] {
        for (int i = 0; i < repeats; ++i) multi_gcr_direction<T>(s, a, 0, g);
    });
    if (!rc) *ms /= repeats;
    return rc;
}

} // namespace
