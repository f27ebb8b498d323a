// mgx_refine_host.hpp - the host side of mgx_solve_refine and mgx_solve_refine_gcr (absent in the reference; the mixed
// passes are mgx_refine.hpp's and mgx_refine_gcr.hpp's).  Included by mgx.hip after
// mgx_krylov_host.hpp.
#pragma once

// ---- mgx_solve_refine: fp64 defect correction around the cycle of a float copy of the hierarchy ---------------
// which handles refine (the message names the reason); then the operators must be set / built
static int refine_guard(mgx_solver* s, const char* fn)
{
    NO_DIST(s)
    if (!s->var)
        return s->fail(MGX_ERR_STATE, std::string(fn) + ": op = MGX_OPERATOR_POISSON handles refine with dtype MIXED (use dtype MIXED and mgx_solve); "
                                                        "this entry point is for MGX_OPERATOR_STENCIL5 and MGX_OPERATOR_GALERKIN");
    if (s->mixed || !s->work_f64)
        return s->fail(MGX_ERR_STATE, std::string(fn) + ": dtype F64 handles only (the float cycle runs in a copy of the hierarchy inside the handle)");
    return MGX_OK;
}

// the whole grids of slots 0 .. nq - 1 of the operator of level lv, rounded to float into the shadow's
static int refine_round_level(mgx_solver* s, int lv, int nq)
{
    const Level& d = s->lv[lv];
    const Level& w = s->shadow->lv[lv];
    const dim3 blk(256), grd((unsigned)((d.pitch + 255) / 256), d.rows);
    for (int q = 0; q < nq; ++q)
        hipLaunchKernelGGL(k_grid_f64_to_f32, grd, blk, 0, s->stream, (const double*)d.A[q], (float*)w.A[q], d.pitch, w.pitch);
    HIPCHK(s, hipGetLastError());
    return MGX_OK;
}

// The shadow exists and holds the float32 of the handle's current operator: what a public F32 handle of the same cfg
// holds after mgx_set_stencil on every level (STENCIL5), or after mgx_set_stencil / mgx_set_stencil9 on the finest level
// and mgx_build_galerkin_transfer with the parent's transfer (GALERKIN) - its splittings, lambda bounds, line factors
// and dense bottom inverse come from those build paths in float.  A failure (allocation; a breakdown of the float
// line factors) is returned with the F32 build's message and leaves the fp64 handle as it was; the next call tries again
static int refine_shadow(mgx_solver* s)
{
    if (!s->shadow) {
        mgx_config c = s->cfg;
        c.dtype = MGX_DTYPE_F32;
        c.profile = 0;                                        // (the float cycle is not timed span by span: one graph replay)
        mgx_handle sh = nullptr;
        if (int rc = create_solver(&c, s, &sh)) return s->fail(rc, "mgx_solve_refine: float copy of the hierarchy: " + g_create_error);
        sh->cycle = s->cycle;
        s->shadow = sh;
        s->shadow_gen = -1;
    }
    if (s->shadow_gen == s->op_gen) return MGX_OK;
    mgx_solver* f = s->shadow;
    const int lo = s->cfg.coarsest_level, hi = s->cfg.finest_level;
    auto failed = [&](int rc) { return s->fail(rc, "mgx_solve_refine: float copy of the hierarchy: " + f->err); };
    s->shadow_gen = -1;
    if (s->galerkin) {
        const bool nine = s->lv[hi].nine;
        if (nine)
            if (int rc = finest_corners(f, f->lv[hi])) return failed(rc);
        if (int rc = refine_round_level(s, hi, nine ? 9 : 5)) return rc;
        f->lv[hi].nine = nine;
        galerkin_invalidate(f);
        if (int rc = galerkin_build_t<float>(f, s->transfer)) return failed(rc);
    } else {
        for (int lv = lo; lv <= hi; ++lv) {
            if (int rc = refine_round_level(s, lv, 5)) return rc;
            if (int rc = var_build(f, f->lv[lv])) return failed(rc);
        }
    }
    s->shadow_gen = s->op_gen;
    return MGX_OK;
}

// one launch of k_refine_pass on the finest level, u -> tmp (has_e) with r32 into the shadow's right-hand side, and
// the sum of its partials into sum_dev; the caller swaps u and tmp
static void refine_pass(mgx_solver* s, bool has_e, double scale, double inv_scale)
{
    const Level& d = s->lv[s->cfg.finest_level];
    const Level& w = s->shadow->lv[s->cfg.finest_level];
    with_point_count(d.nine, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        const auto launch = has_e ? launch_refine_pass<NQ, true> : launch_refine_pass<NQ, false>;
        const int nb = launch((const double*)d.u, (const float*)w.u, (const double*)d.b, op9_of<double>(d), (double*)d.tmp, (float*)w.b, scale,
                              inv_scale, s->partial, s->partial_cap, d.N, d.pitch, w.pitch, s->rows_per_chunk, s->stream);
        hipLaunchKernelGGL(k_reduce_partials, dim3(1), dim3(kReduceThreads), 0, s->stream, s->partial, nb, s->sum_dev);
    });
}

// ---- mgx_solve_refine_gcr: fp64 restarted GCR (mgx_krylov.hpp) around the float cycle of the shadow ---------------
// x += alpha Z_j, r -= alpha Q_j, the partials of ||r||^2 and r32 = (float)(r * inv_scale_next), the right-hand side of
// the next float cycle
static void refine_gcr_update(mgx_solver* s, const KrylovView& v, const Launch& g, int j, double inv_scale_next, float* r32, long epitch)
{
    const Level& d = s->lv[s->cfg.finest_level];
    hipLaunchKernelGGL(k_refine_update, dim3(g.blocks), dim3(kBlock), 0, s->stream, (double*)v.x, (const double*)v.Z[j], (double*)v.r,
                       (const double*)v.Q[j], r32, inv_scale_next, (const double*)v.sc, v.part, d.N, d.pitch, epitch, g.R, g.strips, g.chunks);
}

// the two on the handle's own workspace: z32 is the shadow's U (with the shadow's pitch), r32 the shadow's right-hand side.
// Z_j = z = scale * (double) z32, Q_j = A z on the handle's finest operator: the one-column launch of k_refine_direction
static void refine_gcr_direction(mgx_solver* s, const KrylovView& v, const Launch& g, int j, double scale)
{
    const Level& d = s->lv[s->cfg.finest_level];
    const Level& w = s->shadow->lv[s->cfg.finest_level];
    const float* const z32 = (const float*)w.u;
    double* const z = (double*)v.Z[j];
    double* const q = (double*)v.Q[j];
    launch_refine_direction(1, d.nine, &z32, &z, &q, &scale, op9_of<double>(d), d.N, d.pitch, w.pitch, g, s->stream);
}
static void refine_gcr_update(mgx_solver* s, const KrylovView& v, const Launch& g, int j, double inv_scale_next)
{
    const Level& w = s->shadow->lv[s->cfg.finest_level];
    refine_gcr_update(s, v, g, j, inv_scale_next, (float*)w.b, w.pitch);
}

// no scaled residual is pending before the first float cycle of a solve: r32 = (float)((b - A x) * inv_scale), the bits
// of r = b - A x, by k_refine_pass without a correction (e is not read; its sums of squares go into `partial`, unread)
static void refine_gcr_first_residual(mgx_solver* s, const void* x, const void* b, const float* e, float* r32, double inv_scale, double* partial,
                                      long partial_cap)
{
    const Level& l = s->lv[s->cfg.finest_level];
    const Level& fl = s->shadow->lv[s->cfg.finest_level];
    with_point_count(l.nine, [&](auto nq) {
        launch_refine_pass<decltype(nq)::value, false>((const double*)x, e, (const double*)b, op9_of<double>(l), (double*)l.tmp, r32, 0.0, inv_scale,
                                                       partial, partial_cap, l.N, l.pitch, fl.pitch, s->rows_per_chunk, s->stream);
    });
}

// The shadow is the solver whose cycle preconditions mgx_solve_refine_gcr
static int refine_cycle_of(mgx_solver* s, mgx_solver** f)
{
    if (int rc = refine_shadow(s)) return rc;
    *f = s->shadow;
    return MGX_OK;
}

// mgx_solve_gcr's method (krylov_run, over the same workspace) with the cycle replaced by the scaled float cycle of the
// shadow: r32 is the shadow's lv[L].b and z32 its lv[L].u, the pointers its cached cycle graphs hold.  The
// orthogonalisation and the reductions are GcrMethod's; the direction and the update are the mixed passes above
struct RefineGcrMethod {
    using T = double;
    static constexpr const char* name = "mgx_solve_refine_gcr: GCR";
    static constexpr const char* quantity = GcrMethod<double>::quantity;
    int restart;

    // s_k: mgx_solve_refine's rule, a power of two near the rms of the residual the float cycle of iteration k is given
    static double scale(const Level& l, const std::vector<double>& hist, int k) { return pow2_floor(hist[k] / (double)(l.N - 1)); }

    int prepare(mgx_solver* s, size_t bytes) { return GcrMethod<double>{restart}.prepare(s, bytes); }
    int precondition(mgx_solver* s, const Level& l, int k, const std::vector<double>& hist)
    {
        mgx_solver* f = s->shadow;
        if (k == 0) {
            // r32 = (float)((b - A x) / s_0), the bits of r in lv[L].b
            const Level& fl = f->lv[s->cfg.finest_level];
            Prof p(s, MGX_PROF_NORM_FINE, 1);
            refine_gcr_first_residual(s, s->kry.x, s->kry.b, (const float*)fl.u, (float*)fl.b, 1.0 / scale(l, hist, 0), s->partial, s->partial_cap);
        }
        if (int rc = krylov_cycle(f)) return s->fail(rc, "mgx_solve_refine_gcr: float cycle: " + f->err);   // z32 = M32 r32 from zero
        return MGX_OK;
    }
    void enqueue(mgx_solver* s, const Level& l, const Launch& g, int k, const std::vector<double>& hist)
    {
        const KrylovView v = krylov_view(s);
        const int j = k % restart;
        Prof p(s, MGX_PROF_NORM_FINE, j ? 7 : 5);                      // direction, (dots, reduce,) orth, reduce, update, reduce
        refine_gcr_direction(s, v, g, j, scale(l, hist, k > 0 ? k - 1 : 0));
        gcr_orth<double>(s, v, l, g, j);
        refine_gcr_update(s, v, g, j, 1.0 / scale(l, hist, k));
        krylov_reduce(s, v, g.blocks, kPcgRRMode);
    }
};
