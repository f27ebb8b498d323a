// mgx_multi_refine_host.hpp - the host side of mgx_solve_multi_refine_gcr (absent in the reference): the
// iteration of mgx_solve_refine_gcr on up to four right-hand sides, each column bit for bit what that call returns for it.
// Included by mgx.hip after mgx_refine_host.hpp and mgx_multi_host.hpp, whose pieces it puts together:
//   the frame (copy in, fp64 norms, active set, copy out, statistics)    MultiFrame<double>
//   the preconditioner: the float block cycle on the shadow's columns    vcycle(s->shadow, .., a, fu)
//   the orthogonalisation, the mixed update, the reductions              gcr_orth, refine_gcr_update, krylov_reduce on
//                                                                        krylov_view(s, c), r32 = the shadow column's b
//   the host's reading of an iteration                                   MultiFrame::gcr_step
// The direction pass runs on the set (k_refine_direction<NQ, K>, mgx_refine_gcr.hpp).
// Workspaces: the shadow (refine_shadow, shared with mgx_solve_refine*), the shadow's MultiWs float columns on every
// level, the parent's MultiWs with its Krylov pieces (shared with mgx_solve_multi_gcr; its coarse fp64 columns are
// allocated and not used here).  The handle's own vectors, kry workspace and graphs and the shadow's are not touched.
#pragma once

namespace {

// the handles that refine (refine_guard) and solve blocks (multi_guard): one GPU, F64, STENCIL5 or GALERKIN, Jacobi
int multi_refine_guard(mgx_solver* s, const char* fn)
{
    if (int rc = refine_guard(s, fn)) return rc;
    return multi_guard(s, fn);
}

// Z_c[j] = z_c = scale[c] * (double) z32_c (the shadow column's finest u), Q_c[j] = A z_c for the columns of the set: one
// launch of k_refine_direction, the operator read once
void multi_refine_direction(mgx_solver* s, const MultiSet& a, int j, const Launch& g, const double* scale)
{
    const int L = s->cfg.finest_level;
    const Level& l = s->lv[L];
    const Level& fl = s->shadow->lv[L];
    auto& ws = s->multi;
    auto& fw = s->shadow->multi.lv[L];
    const float* z32[MGX_MAX_RHS];
    double *z[MGX_MAX_RHS], *q[MGX_MAX_RHS], sc[MGX_MAX_RHS];
    for (int i = 0; i < a.m; ++i) {
        const int c = a.act[i];
        z32[i] = (const float*)fw.u[c]; z[i] = (double*)ws.Z[c][j]; q[i] = (double*)ws.Q[c][j]; sc[i] = scale[c];
    }
    launch_refine_direction(a.m, l.nine, z32, z, q, sc, op9_of<double>(l), l.N, l.pitch, fl.pitch, g, s->stream);
}

// the three workspaces for nrhs columns and `restart` basis pairs; a failure leaves what existed
int multi_refine_ensure(mgx_solver* s, int nrhs, int restart, int blocks)
{
    mgx_solver* f = s->shadow;
    if (int rc = multi_ensure(f, nrhs)) return s->fail(rc, "mgx_solve_multi_refine_gcr: float columns: " + f->err);
    if (int rc = multi_ensure(s, nrhs)) return rc;
    return multi_gcr_ensure(s, nrhs, restart, blocks);
}

int multi_refine_gcr_solve(mgx_solver* s, int nrhs, const void* b, void* u, double tol, int max_iters, int restart, mgx_stats* stats,
                           double* history, int history_cap)
{
    mgx_solver* f = s->shadow;
    MultiFrame<double> fr{s, nrhs};
    const Launch g = multi_gcr_launch<double>(s);
    if (int rc = multi_refine_ensure(s, nrhs, restart, g.blocks)) return rc;
    if (int rc = fr.begin(b, u, max_iters)) return rc;
    const int L = s->cfg.finest_level;
    Level& l = s->lv[L];
    const Level& fl = f->lv[L];
    auto& ws = s->multi;
    auto& w = ws.lv[L];
    auto& fw = f->multi.lv[L];
    // s_k of a column: RefineGcrMethod's rule on the column's own history
    auto scale = [&](int c, int k) { return RefineGcrMethod::scale(l, fr.hist[c], k); };
    for (int j = 0; j < nrhs; ++j) HIPCHK(s, hipMemcpyAsync(ws.x[j], w.u[j], l.bytes, hipMemcpyDeviceToDevice, s->stream));
    MultiSet a = max_iters > 0 ? fr.active(multi_all(nrhs), tol) : MultiSet{};
    if (a.m > 0) {
        // r_c = b_c - A x_c becomes the column's finest b (mgx_solve_multi_gcr's step); before the swap, the first float
        // right-hand side of every column by the launch mgx_solve_refine_gcr makes at k = 0 - once per solve and column
        residual_set<double, 0>(s, L, a);
        const long cap = (long)(kGcrMaxRestart - 1) * g.blocks + 8;     // of gpart (multi_gcr_ensure)
        for (int i = 0; i < a.m; ++i) {
            const int c = a.act[i];
            refine_gcr_first_residual(s, ws.x[c], w.b[c], (const float*)fw.u[c], (float*)fw.b[c], 1.0 / scale(c, 0), ws.gpart[c], cap);
            std::swap(w.b[c], w.r[c]);
        }
        HIPCHK(s, hipMemsetAsync(ws.gsc, 0, MGX_MAX_RHS * kGcrScalars * sizeof(double), s->stream));
    }
    // every float cycle starts from zero.  On a one-level hierarchy with the exact bottom the dense solve overwrites u;
    // with bottom = SMOOTH mgx_solve_refine_gcr starts from what the shadow's U held, this call from zero (mgx.h)
    const bool zero_start = L > s->cfg.coarsest_level || s->cfg.bottom != MGX_BOTTOM_EXACT;
    std::string first_break;
    for (int k = 0; k < max_iters && a.m > 0; ++k) {
        const int j = k % restart;
        if (int rc = zero_start ? zero_u(f, L, a) : MGX_OK) return s->fail(rc, f->err);
        vcycle(f, L, false, 0, f->cycle, a, fr.fu);                        // z32_c = M32 r32_c, into the shadow column's finest u
        double sk[MGX_MAX_RHS] = {};
        for (int i = 0; i < a.m; ++i) sk[a.act[i]] = scale(a.act[i], k > 0 ? k - 1 : 0);
        multi_refine_direction(s, a, j, g, sk);
        for (int i = 0; i < a.m; ++i) {
            const int c = a.act[i];
            const KrylovView v = krylov_view(s, c);
            gcr_orth<double>(s, v, l, g, j);
            refine_gcr_update(s, v, g, j, 1.0 / scale(c, k), (float*)fw.b[c], fl.pitch);
            krylov_reduce(s, v, g.blocks, kPcgRRMode);
        }
        if (int rc = fr.gcr_step(a, k, "mgx_solve_multi_refine_gcr", RefineGcrMethod::quantity, first_break)) return rc;
        a = fr.active(a, tol);
    }
    if (int rc = fr.finish(ws.x, u, tol, stats, history, history_cap)) return rc;
    if (!first_break.empty()) s->err = first_break;
    return MGX_OK;
}

// mgx_time_multi_refine_direction: `repeats` launches of the direction pass with scale 1 on the first nrhs columns, from
// the shadow column's finest u into basis slot 0 of the parent's column (which has no meaning between two solves)
int multi_refine_time_direction(mgx_solver* s, int nrhs, int repeats, double* ms)
{
    const Launch g = multi_gcr_launch<double>(s);
    const MultiSet a = multi_all(nrhs);
    const double one[MGX_MAX_RHS] = {1.0, 1.0, 1.0, 1.0};
    const int rc = time_on_stream(s, ms, [&] {
        for (int i = 0; i < repeats; ++i) multi_refine_direction(s, a, 0, g, one);
    });
    if (!rc) *ms /= repeats;
    return rc;
}

} // namespace
