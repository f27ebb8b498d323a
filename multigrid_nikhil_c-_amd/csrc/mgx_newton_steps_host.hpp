// mgx_newton_steps_host.hpp - the host side of mgx_newton_steps and mgx_time_newton_step_pass (absent in the reference;
// the kernels and their arithmetic are mgx_newton.hpp's).  Included by mgx.hip after mgx_newton_host.hpp,
// whose workspace and iteration (newton_workspace, newton_iterate, newton_leave) every time step runs with a mass grid.
#pragma once

namespace {

// one launch of k_newton_step_rhs on the finest level: out <- the explicit part of a theta step from the time level u
void newton_step_rhs(mgx_solver* s, double theta, const void* u, const void* g, void* out)
{
    const Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->nwt;
    const void* centre = s->rx.set ? s->rx.c0 : l.A[0];       // A0's, as in newton_pass
    with_float_type(l.f64, [&](auto tag) {
        using T = decltype(tag);
        launch_newton_step_rhs<T>(var_level<T>(l), (const T*)u, (const T*)w.dm, (const T*)w.kap, (const T*)g, (const T*)centre, (T*)out,
                                  newton_poly<T>(w.p1, w.p2, w.p3, (T)0), theta, s->stream);
    });
}

int newton_steps(mgx_solver* s, const mgx_newton_opts& o, double theta, int nsteps, const void* mass, const void* kappa, const void* g, size_t count,
                 int* steps_done, mgx_newton_stats* step_stats, double* history, int history_cap)
{
    Level& l = s->lv[s->cfg.finest_level];
    auto& w = s->nwt;
    // the whole workspace before anything is touched
    if (int rc = newton_workspace(s, "mgx_newton_steps")) return rc;
    if (int rc = reaction_grid(s, &w.dm, "mgx_newton_steps", "the mass term")) return rc;
    if (g)
        if (int rc = reaction_grid(s, &w.g, "mgx_newton_steps", "the source term")) return rc;
    w.p1 = o.p1; w.p2 = o.p2; w.p3 = o.p3;
    if (int rc = copy_in(s, l, w.kap, kappa, count)) return rc;
    if (int rc = copy_in(s, l, w.dm, mass, count)) return rc;
    if (g)
        if (int rc = copy_in(s, l, w.g, g, count)) return rc;
    HIPCHK(s, hipMemcpyAsync(w.un, l.u, l.bytes, hipMemcpyDeviceToDevice, s->stream));
    HIPCHK(s, hipMemcpyAsync(w.f, l.b, l.bytes, hipMemcpyDeviceToDevice, s->stream));      // (what B keeps if the first pass fails)

    int rc = MGX_OK;
    std::string msg;
    for (int k = 0; k < nsteps; ++k) {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string step = "mgx_newton_steps: step " + std::to_string(k);
        // r of this step from the time level un, into the iteration's right-hand side; then Newton from un as the guess
        newton_step_rhs(s, theta, w.un, g ? w.g : nullptr, w.f);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) {
            rc = MGX_ERR_HIP;
            msg = step + ": the right-hand-side pass: " + hipGetErrorString(e);
            break;
        }
        NewtonRun run;
        if ((rc = newton_iterate(s, o, step + ": Newton step ", w.dm, nullptr, nullptr, run)) != MGX_OK) {
            msg = run.msg.rfind(step, 0) == 0 ? run.msg : step + ": " + run.msg;
            break;
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        newton_report(run, o.tol, sec, step_stats ? step_stats + k : nullptr, history ? history + (size_t)k * (size_t)history_cap : nullptr, history_cap);
        if (steps_done) *steps_done = k + 1;
        if (!(run.hist.back() <= o.tol * run.hist[0])) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "||G|| is %.3e of the initial one after %d of max_newton = %d Newton steps", run.hist.back() / run.hist[0],
                          (int)run.hist.size() - 1, o.max_newton);
            msg = step + " did not converge: " + (run.msg.empty() ? std::string(buf) : run.msg) + "; the later steps were not taken";
            break;
        }
    }
    // U = the last time level (the last accepted iterate), B = the last step's r, on every path
    return newton_leave(s, rc, msg, "mgx_newton_steps");
}

} // namespace
