// mgx_eig_many_host.hpp - the host side of mgx_eigs_many and mgx_time_eig_project (absent in the reference): mgx_eigs'
// block iteration (eig_block, mgx_eig_host.hpp) on blocks of at most MGX_MAX_RHS columns, each constrained to the
// complement of the pairs locked so far.  The iteration and the projection are stated in mgx_eig_many.hpp, whose kernels
// this file launches; the partition, the order and the scatter of the results are mgx_eig_many_plan.hpp's (plain C++).
// Included by mgx.hip after mgx_eig_host.hpp.
#pragma once

#include "mgx_eig_many_plan.hpp"

namespace {

static_assert(mgx::kEigManyMax == MGX_EIGS_MAX && mgx_eig_many::kBlockMax == mgx::kMultiMax, "one cap, one block width");

constexpr int kEigProjectSums = mgx::kEigChunk * MGX_MAX_RHS;         // sums of one chunk of k_eig_project_dots

void eig_many_free(mgx_solver::EigManyWs& w)
{
    for (int i = 0; i < MGX_EIGS_MAX; ++i) {
        if (w.Y[i]) (void)hipFree(w.Y[i]);
        w.Y[i] = nullptr;
    }
    if (w.ytab) (void)hipFree(w.ytab);
    if (w.coef) (void)hipFree(w.coef);
    if (w.part) (void)hipFree(w.part);
    w.ytab = nullptr;
    w.coef = w.part = nullptr;
    w.slots = 0;
}

// the locked slots [0, nev), the pointer table, the coefficients and their partial sums exist afterwards.  A failure
// frees the slot it was allocating and leaves what existed (the table names the slots that exist)
int eig_many_ensure(mgx_solver* s, int nev, int blocks)
{
    auto& w = s->eigm;
    const Level& l = s->lv[s->cfg.finest_level];
    auto bad = [&](const std::string& what) {
        (void)hipGetLastError();
        return s->fail(MGX_ERR_ALLOC, "mgx_eigs_many: allocation failed for " + what);
    };
    if (!w.part && hipMalloc((void**)&w.part, (size_t)kEigProjectSums * blocks * sizeof(double)) != hipSuccess) { w.part = nullptr; return bad("the partial sums of the projection"); }
    if (!w.coef && hipMalloc((void**)&w.coef, MGX_EIGS_MAX * MGX_MAX_RHS * sizeof(double)) != hipSuccess) { w.coef = nullptr; return bad("the coefficients of the projection"); }
    if (!w.ytab && hipMalloc((void**)&w.ytab, MGX_EIGS_MAX * sizeof(void*)) != hipSuccess) { w.ytab = nullptr; return bad("the table of the locked vectors"); }
    const int had = w.slots;
    int rc = MGX_OK;
    for (int i = w.slots; i < nev; ++i) {
        if (!alloc_zeroed(s, &w.Y[i], l.bytes)) { rc = bad("locked vector " + std::to_string(i)); break; }
        w.slots = i + 1;
    }
    if (w.slots > had) {
        HIPCHK(s, hipStreamSynchronize(s->stream));
        HIPCHK(s, hipMemcpy(w.ytab, w.Y, MGX_EIGS_MAX * sizeof(void*), hipMemcpyHostToDevice));
    }
    return rc;
}

// V <- V - Y (Y^T V) on k device columns against the first m locked slots (mgx_eig_many.hpp, THE PROJECTION); no host
// synchronisation
template <typename T>
void eig_project(mgx_solver* s, const EigGeom& e, int m, int k, void* const* cols, bool dots = true, bool sub = true)
{
    auto& w = s->eigm;
    const T* y[MGX_EIGS_MAX];
    const T* ci[MGX_MAX_RHS];
    T* co[MGX_MAX_RHS];
    for (int i = 0; i < m; ++i) y[i] = (const T*)w.Y[i];
    for (int j = 0; j < k; ++j) { ci[j] = (const T*)cols[j]; co[j] = (T*)cols[j]; }
    if (dots) launch_eig_project_dots<T>(m, k, y, ci, w.part, w.coef, e, s->stream);
    if (sub) launch_eig_project_sub<T>(m, k, (const T* const*)w.ytab, co, w.coef, e, s->stream);
}

template <typename T>
int eigs_many_t(mgx_solver* s, int nev, void* x, double* lambda, double tol, int max_iters, mgx_stats* stats, double* history, int history_cap)
{
    namespace em = mgx_eig_many;
    const auto t0 = std::chrono::steady_clock::now();
    const EigGeom e = eig_geom<T>(s);
    int size[em::kMax];
    const int nb = em::partition(nev, size);
    if (int rc = multi_ensure(s, size[0])) return rc;
    if (int rc = eig_ensure(s, size[0], e.g.blocks)) return rc;
    if (int rc = eig_many_ensure(s, nev, e.g.blocks)) return rc;
    Level& l = s->lv[s->cfg.finest_level];
    const size_t nn = (size_t)(l.N - 1) * (size_t)(l.N - 1);

    EigBlockResult res[em::kMax / em::kBlockMax];
    em::Pair pair[em::kMax];
    const void* src[em::kMax];                       // where the vector of a computed pair lives on the device
    int done = 0;                                    // pairs computed; the first `locked` of them are in Y
    std::string reason;
    for (int b = 0; b < nb; ++b) {
        const int kb = size[b], m = done;
        const std::string who = "mgx_eigs_many: block " + std::to_string(b);
        EigRun<T> run{s, kb, e};
        auto project = [&](int k, void* const* cols) {
            if (m > 0) eig_project<T>(s, e, m, k, cols);
        };
        if (int rc = eig_block<T>(run, (const T*)x + (size_t)done * nn, tol, max_iters, who, project, res[b])) {
            if (rc == MGX_ERR_INVALID && m > 0) s->err += " (after the projection against the " + std::to_string(m) + " pairs of the blocks before it)";
            return rc;
        }
        bool all = true;
        for (int j = 0; j < kb; ++j) {
            em::Pair& p = pair[done + j];
            p.lambda = res[b].theta[j];
            p.hist = &res[b].hist[j];
            p.cycles = res[b].cycles[j];
            p.converged = res[b].converged(j, tol);
            p.fine_updates = res[b].fu[j];
            all = all && p.converged;
            src[done + j] = s->eig.X[j];
        }
        done += kb;
        if (!all) {
            reason = !res[b].reason.empty() ? res[b].reason
                                            : who + " did not converge within max_iters = " + std::to_string(max_iters) + " iterations";
            if (done < nev) reason += "; the pairs " + std::to_string(done) + " .. " + std::to_string(nev - 1) + " of the later blocks were not computed";
            break;
        }
        if (done < nev) {
            // Y <- [Y, X]: the next block overwrites the workspace's X
            for (int j = 0; j < kb; ++j) {
                HIPCHK(s, hipMemcpyAsync(s->eigm.Y[m + j], s->eig.X[j], l.bytes, hipMemcpyDeviceToDevice, s->stream));
                src[m + j] = s->eigm.Y[m + j];
            }
        }
    }
    HIPCHK(s, hipStreamSynchronize(s->stream));
    const double seconds_so_far = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (int rc = em::scatter(nev, done, pair, seconds_so_far, lambda, stats, history, history_cap, [&](int p, int slot) {
            return copy_out(s, l, src[p], (T*)x + (size_t)slot * nn, nn);
        }))
        return rc;
    if (stats) {
        // the whole call, the copies of the vectors to the host included (as mgx_eigs counts it)
        const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int j = 0; j < done; ++j) stats[j].seconds = seconds;
    }
    if (!reason.empty()) s->err = reason;
    return MGX_OK;
}

// mgx_time_eig_project: `repeats` launches of one pass of the projection of the first k workspace columns (their finest
// u, where the cycle leaves W) against the first m locked slots, between two events.  DOTS: every chunk of
// k_eig_project_dots with its reduction; SUB: k_eig_project_sub with the coefficients zeroed, so W keeps its bits
template <typename T>
int eig_time_project(mgx_solver* s, int pass, int m, int k, int repeats, double* ms)
{
    const EigGeom e = eig_geom<T>(s);
    auto& w = s->multi.lv[s->cfg.finest_level];
    HIPCHK(s, hipMemsetAsync(s->eigm.coef, 0, MGX_EIGS_MAX * MGX_MAX_RHS * sizeof(double), s->stream));
    const int rc = time_on_stream(s, ms, [&] {
        for (int i = 0; i < repeats; ++i) eig_project<T>(s, e, m, k, w.u, pass == MGX_EIG_PROJECT_DOTS, pass == MGX_EIG_PROJECT_SUB);
    });
    if (!rc) *ms /= repeats;
    return rc;
}

} // namespace
