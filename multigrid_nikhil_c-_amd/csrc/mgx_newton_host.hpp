// mgx_newton_host.hpp - the host side of mgx_newton and mgx_time_newton_pass (absent in the reference; the pass and its
// arithmetic are mgx_newton.hpp's).  Included by mgx.hip after mgx_theta_host.hpp, whose zero-order term
// (reaction_base, reaction_shift) carries the Jacobian's diagonal.  In two parts: the workspace with the entry copies
// (newton), and the iteration on the loaded grids (newton_iterate), which mgx_newton_steps runs once per time step with
// a mass grid (mgx_newton_steps_host.hpp).
#pragma once

namespace {

void newton_free(mgx_solver::NewtonWs& w)
{
    for (void** p : {&w.un, &w.ut, &w.f, &w.kap, &w.dn, &w.dm, &w.g}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

// which handles run Newton steps: those that carry a zero-order term (reaction_guard), with the hierarchy built - the
// transfer it was built with is the one every step rebuilds it with
int newton_guard(mgx_solver* s, const char* fn)
{
    if (int rc = reaction_guard(s, fn)) return rc;
    if (!s->gal_built) return s->fail(MGX_ERR_STATE, std::string(fn) + ": Galerkin hierarchy not built (mgx_build_galerkin[_transfer]): the steps rebuild it with the transfer of that build");
    return MGX_OK;
}

// the checks on the options, in the documented order
int newton_opts_check(mgx_solver* s, const mgx_newton_opts* o, const char* fn)
{
    const std::string pre = std::string(fn) + ": ";
    if (!std::isfinite(o->p1) || !std::isfinite(o->p2) || !std::isfinite(o->p3)) return s->fail(MGX_ERR_INVALID, pre + "p1, p2, p3 must be finite");
    if (o->solver < MGX_STEP_SOLVE || o->solver > MGX_STEP_REFINE_GCR)
        return s->fail(MGX_ERR_INVALID, pre + "solver must be MGX_STEP_SOLVE, MGX_STEP_GCR or MGX_STEP_REFINE_GCR");
    if (!(o->lin_tol >= 0.0)) return s->fail(MGX_ERR_INVALID, pre + "lin_tol >= 0 required");
    if (o->lin_max_iters < 0) return s->fail(MGX_ERR_INVALID, pre + "lin_max_iters >= 0 required");
    if (o->solver != MGX_STEP_SOLVE && (o->restart < 1 || o->restart > MGX_GCR_MAX_RESTART))
        return s->fail(MGX_ERR_INVALID, pre + "1 <= restart <= MGX_GCR_MAX_RESTART required");
    if (!(o->tol >= 0.0)) return s->fail(MGX_ERR_INVALID, pre + "tol >= 0 required");
    if (o->max_newton < 0) return s->fail(MGX_ERR_INVALID, pre + "max_newton >= 0 required");
    if (o->max_backtracks < 0 || o->max_backtracks > 30) return s->fail(MGX_ERR_INVALID, pre + "0 <= max_backtracks <= 30 required");
    return MGX_OK;
}

// the grids of mgx_newton, and mgx_set_reaction's two, before anything is touched: a failure leaves the operator and the
// hierarchy as they were
int newton_workspace(mgx_solver* s, const char* fn)
{
    auto& w = s->nwt;
    const struct { void** p; const char* what; } grids[] = {{&w.un, "the iterate"}, {&w.ut, "the trial iterate"}, {&w.f, "the right-hand side"},
                                                            {&w.kap, "kappa"}, {&w.dn, "the Jacobian's diagonal term"},
                                                            {&s->rx.c0, "the base centre"}, {&s->rx.d, "the zero-order term"}};
    for (const auto& g : grids)
        if (int rc = reaction_grid(s, g.p, fn, g.what)) return rc;
    return MGX_OK;
}

// one launch of k_newton_pass on the finest level and the reduction of its sums: b, dn (and ut when step) from un (and the
// linear solve's result in U), *r = ||b||_2; dm: the mass term of a time step, or null.  One D2H of one double and one
// host synchronisation
int newton_pass(mgx_solver* s, bool step, double lam, const void* dm, void* b, double* r)
{
    const Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->nwt;
    const void* centre = s->rx.set ? s->rx.c0 : l.A[0];       // A0's: slot 0 carries the term once one is set
    with_float_type(l.f64, [&](auto tag) {
        using T = decltype(tag);
        launch_newton_pass<T>(var_level<T>(l), step, (const T*)w.un, (const T*)l.u, (const T*)w.f, (const T*)w.kap, (const T*)centre, (const T*)dm,
                              (T*)w.ut, (T*)b, (T*)w.dn, newton_poly<T>(w.p1, w.p2, w.p3, (T)lam), s->partial, s->sum_dev, s->stream);
    });
    s->norm_blocks_ready = 0;                                 // partial[] holds this pass's sums
    HIPCHK(s, hipGetLastError());
    if (!r) return MGX_OK;
    HIPCHK(s, hipMemcpyAsync(s->sum_host, s->sum_dev, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIPCHK(s, hipStreamSynchronize(s->stream));
    *r = std::sqrt(*s->sum_host);
    return MGX_OK;
}

// what an iteration leaves: the norms, the counts and what mgx_last_error says after the call
struct NewtonRun {
    std::vector<double> hist;
    int backtracks = 0, lin_iters = 0;
    std::string msg;
};

// the iteration on the loaded grids: un the guess, f the right-hand side, kap, p1 .. p3, and dm the mass term (null: none).
// It leaves the last accepted iterate in un; B holds the right-hand side of the last pass.  pre: what precedes the step's
// number in a message
int newton_iterate(mgx_solver* s, const mgx_newton_opts& o, const std::string& pre, const void* dm, mgx_stats* lin_stats, double* step_lengths,
                   NewtonRun& run)
{
    const int L = s->cfg.finest_level;
    Level& l = s->lv[L];
    auto& w = s->nwt;
    std::vector<double>& hist = run.hist;
    std::string& msg = run.msg;
    hist.assign(1, 0.0);
    int rc = MGX_OK;
    if ((rc = newton_pass(s, false, 0.0, dm, l.b, &hist[0])) != MGX_OK) msg = s->err;
    for (int k = 0; rc == MGX_OK && k < o.max_newton && !(hist[k] <= o.tol * hist[0]); ++k) {
        // the Jacobian A0 + diag(d) of the iterate: what mgx_set_reaction(d) + mgx_build_galerkin_transfer leave
        if ((rc = reaction_base(s)) != MGX_OK) { msg = s->err; break; }
        std::swap(s->rx.d, w.dn);
        if ((rc = reaction_shift(s)) == MGX_OK) rc = s->work_f64 ? galerkin_build_t<double>(s, s->transfer) : galerkin_build_t<float>(s, s->transfer);
        if (rc == MGX_OK) rc = zero_u(s, L);                 // (B holds b: the pass wrote it there)
        if (rc == MGX_OK) {
            s->norm_blocks_ready = 0;
            s->err.clear();
            mgx_stats st{};
            if (o.solver == MGX_STEP_SOLVE) rc = mgx_solve(s, o.lin_tol, o.lin_max_iters, &st, nullptr, 0);
            else if (o.solver == MGX_STEP_GCR) rc = mgx_solve_gcr(s, o.lin_tol, o.lin_max_iters, o.restart, &st, nullptr, 0);
            else rc = mgx_solve_refine_gcr(s, o.lin_tol, o.lin_max_iters, o.restart, &st, nullptr, 0);
            if (rc == MGX_OK) {
                if (lin_stats) lin_stats[k] = st;
                run.lin_iters += st.cycles;
            }
        }
        if (rc != MGX_OK) { msg = pre + std::to_string(k) + ": " + s->err; break; }
        // backtracking on ||F||: the trial un + lam de with lam = 1, 1/2, ... (the solvers swap u and tmp: l.u afresh)
        double lam = 1.0, r = 0.0;
        bool accepted = false;
        for (int j = 0;;) {
            if ((rc = newton_pass(s, true, lam, dm, l.b, &r)) != MGX_OK) { msg = pre + std::to_string(k) + ": " + s->err; break; }
            if (r <= (1.0 - 1e-4 * lam) * hist[k]) { accepted = true; break; }       // (NaN rejects)
            ++run.backtracks;
            if (++j > o.max_backtracks) break;
            lam *= 0.5;
        }
        if (rc != MGX_OK) break;
        if (!accepted) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "%d: line search failed: smallest lam tried %.17g gave ||F|| = %.17g against %.17g of the iterate", k, lam, r,
                          hist[k]);
            msg = pre + buf;
            break;
        }
        std::swap(w.un, w.ut);
        hist.push_back(r);
        if (step_lengths) step_lengths[k] = lam;
    }
    return rc;
}

// U = the last accepted iterate and B = the workspace's f, on every path of a call; then the status of the call
int newton_leave(mgx_solver* s, int rc, const std::string& msg, const char* fn)
{
    Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->nwt;
    const hipError_t e1 = hipMemcpyAsync(l.u, w.un, l.bytes, hipMemcpyDeviceToDevice, s->stream);
    const hipError_t e2 = hipMemcpyAsync(l.b, w.f, l.bytes, hipMemcpyDeviceToDevice, s->stream);
    const hipError_t e3 = hipStreamSynchronize(s->stream);
    s->norm_blocks_ready = 0;
    s->err = msg;
    if (rc != MGX_OK) return rc;
    for (hipError_t e : {e1, e2, e3})
        if (e != hipSuccess) return s->fail(MGX_ERR_HIP, std::string(fn) + ": restoring U and B: " + hipGetErrorString(e));
    return MGX_OK;
}

void newton_report(const NewtonRun& run, double tol, double seconds, mgx_newton_stats* nstats, double* history, int history_cap)
{
    const std::vector<double>& hist = run.hist;
    if (nstats) {
        nstats->iterations = (int)hist.size() - 1;
        nstats->converged = hist.back() <= tol * hist[0] ? 1 : 0;
        nstats->initial_residual = hist.front();
        nstats->final_residual = hist.back();
        nstats->seconds = seconds;
        nstats->linear_iterations = run.lin_iters;
        nstats->backtracks = run.backtracks;
        nstats->history_len = (int)hist.size();
    }
    if (history)
        for (int i = 0; i < (int)hist.size() && i < history_cap; ++i) history[i] = hist[i];
}

int newton(mgx_solver* s, const mgx_newton_opts& o, const void* kappa, size_t count, mgx_newton_stats* nstats, mgx_stats* lin_stats,
           double* step_lengths, double* history, int history_cap)
{
    const auto t0 = std::chrono::steady_clock::now();
    Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->nwt;
    if (int rc = newton_workspace(s, "mgx_newton")) return rc;
    w.p1 = o.p1; w.p2 = o.p2; w.p3 = o.p3;
    if (int rc = copy_in(s, l, w.kap, kappa, count)) return rc;
    HIPCHK(s, hipMemcpyAsync(w.un, l.u, l.bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(s, hipMemcpyAsync(w.f, l.b, l.bytes, hipMemcpyDeviceToDevice, s->stream));

    NewtonRun run;
    int rc = newton_iterate(s, o, "mgx_newton: step ", nullptr, lin_stats, step_lengths, run);
    // U = the last accepted iterate, B = the caller's f, on every path
    if ((rc = newton_leave(s, rc, run.msg, "mgx_newton")) != MGX_OK) return rc;
    newton_report(run, o.tol, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), nstats, history, history_cap);
    return MGX_OK;
}

} // namespace
