// mgx_inst.hip - explicit instantiations of the smoother launch wrappers (and through them of the
// k_jacobi_cycle / k_jacobi_fused / k_tile_smooth kernels), one group per compilation so that the library
// builds in parallel (see the end of mgx_launch.hpp and the Makefile):
//   -DMGX_INST_KIND=1  launch_cycle<T, PRE, POST, SM, AR> for the (PRE, POST) pair number MGX_INST_PP
//   -DMGX_INST_KIND=2  launch_fused<T, SM, AR>
//   -DMGX_INST_KIND=3  launch_tile_pass<T, SM, AR>  (all six (PRE, POST) pairs of k_tile_smooth and k_tile_wide)
//   -DMGX_INST_KIND=4  launch_cheby<T>, launch_lambda_max<T>  (mgx_cheby.hpp: k_cheby_var, k_lambda_partials)
//   -DMGX_INST_KIND=5  launch_small_visit<T>, small_visit_prepare<T>  (mgx_small.hpp: k_small_visit)
//   -DMGX_INST_KIND=6  launch_line_factor<T>, launch_line_sweep<T>  (mgx_line.hpp: k_line_factor, k_line_x, k_line_y)
//   -DMGX_INST_KIND=7  launch_gcr_orth<T>  (mgx_krylov.hpp: k_gcr_dots<T, 1..7>, k_gcr_orth<T, 0..7>, k_gcr_reduce)
//   -DMGX_INST_KIND=8  launch_gs_colours<T>, launch_gs_rb<T>  (mgx_colour.hpp: k_gs_colour<T, 5 | 9>, k_gs_rb)
//   -DMGX_INST_KIND=9  launch_gcr_direction_multi<T>  (mgx_multi.hpp: k_gcr_direction_multi<T, 5 | 9, 2..4>)
//   -DMGX_INST_KIND=10 launch_refine_direction  (mgx_refine_gcr.hpp: k_refine_direction<5 | 9, 1..4>; T = double)
//   -DMGX_INST_KIND=11 launch_eig_gram<T>, launch_eig_combine<T>, launch_eig_residual<T>, launch_eig_apply<T>  (mgx_eig.hpp)
//   -DMGX_INST_KIND=12 launch_eig_project_dots<T>, launch_eig_project_sub<T>  (mgx_eig_many.hpp: k_eig_project_dots<T, 1..8, 1..4>,
//                      k_eig_project_sub<T, 1..4>)
//   -DMGX_INST_KIND=13 launch_reaction_shift<T>, launch_theta_rhs<T>  (mgx_theta.hpp: k_reaction_shift, k_theta_rhs<T, 5 | 9, false>,
//                      k_theta_rhs<T, 5, true>)
//   -DMGX_INST_KIND=14 launch_newton_pass<T>, launch_newton_step_rhs<T>  (mgx_newton.hpp: k_newton_pass<T, 5 | 9, STEP, MASS> with both
//                      flags false | true, k_newton_step_rhs<T, 5 | 9, false>, k_newton_step_rhs<T, 5, true>)
//   -DMGX_INST_KIND=15 launch_quasi_pass<T>  (mgx_quasi.hpp: k_quasi_pass<T, STEP, NEWTON> with both flags false | true)
//   -DMGX_INST_T=double|float   -DMGX_INST_SM=0|1   -DMGX_INST_AR=0|1
#include "mgx_launch.hpp"
#if MGX_INST_KIND == 4
#include "mgx_cheby.hpp"
#elif MGX_INST_KIND == 5
#include "mgx_small.hpp"
#elif MGX_INST_KIND == 6
#include "mgx_line.hpp"
#elif MGX_INST_KIND == 7
#include "mgx_krylov.hpp"
#elif MGX_INST_KIND == 8
#include "mgx_colour.hpp"
#elif MGX_INST_KIND == 9
#include "mgx_multi.hpp"
#elif MGX_INST_KIND == 10
#include "mgx_refine_gcr.hpp"
#elif MGX_INST_KIND == 11
#include "mgx_eig.hpp"
#elif MGX_INST_KIND == 12
#include "mgx_eig_many.hpp"
#elif MGX_INST_KIND == 13
#include "mgx_theta.hpp"
#elif MGX_INST_KIND == 14
#include "mgx_newton.hpp"
#elif MGX_INST_KIND == 15
#include "mgx_quasi.hpp"
#endif

namespace mgx {
using T_ = MGX_INST_T;
#if MGX_INST_KIND == 1
#if MGX_INST_PP == 0
#define PP_ 1, 2
#elif MGX_INST_PP == 1
#define PP_ 1, 0
#elif MGX_INST_PP == 2
#define PP_ 0, 1
#elif MGX_INST_PP == 3
#define PP_ 0, 2
#else
#define PP_ 1, 1
#endif
template int launch_cycle<T_, PP_, MGX_INST_SM, MGX_INST_AR>(int, const T_*, const T_*, T_*, const FoldArgs&, int, long, T_, T_, int, hipStream_t);
#elif MGX_INST_KIND == 2
template bool launch_fused<T_, MGX_INST_SM, MGX_INST_AR>(int, const T_*, const T_*, T_*, int, long, int, int, T_, T_, int, int, int, int, hipStream_t, int, int);
#elif MGX_INST_KIND == 3
template int launch_tile_pass<T_, MGX_INST_SM, MGX_INST_AR>(const T_*, const T_*, T_*, const FoldArgs&, int, long, T_, T_, int, int, bool, int, hipStream_t);
#elif MGX_INST_KIND == 4
template void launch_cheby<T_>(const VarLevel<T_>&, const T_*, const T_*, T_*, T_*, bool, T_, T_, T_, T_, hipStream_t);
template void launch_lambda_max<T_>(const VarLevel<T_>&, double*, long, double*, hipStream_t);
#elif MGX_INST_KIND == 5
template hipError_t small_visit_prepare<T_>();
template void launch_small_visit<T_>(const SmallVisit<T_>&, hipStream_t);
#elif MGX_INST_KIND == 6
template void launch_line_factor<T_>(const LineLevel<T_>&, int, int*, hipStream_t);
template int launch_line_sweep<T_>(const LineLevel<T_>&, T_*, const T_*, int, hipStream_t);
#elif MGX_INST_KIND == 7
template void launch_gcr_orth<T_>(int, T_*, T_*, const T_*, const GcrBasis<T_>&, double*, double*, int, long, const Launch&, int, hipStream_t);
#elif MGX_INST_KIND == 8
template int launch_gs_colours<T_>(const ColourLevel<T_>&, T_*, const T_*, bool, hipStream_t);
template void launch_gs_rb<T_>(const ColourLevel<T_>&, const T_*, const T_*, T_*, bool, hipStream_t);
#elif MGX_INST_KIND == 9
template void launch_gcr_direction_multi<T_>(int, bool, const T_* const*, T_* const*, T_* const*, const Op9<T_>&, int, long, const Launch&, hipStream_t);
#elif MGX_INST_KIND == 10
// (not a template: mgx_refine_gcr.hpp defines launch_refine_direction in this compilation)
#elif MGX_INST_KIND == 11
template void launch_eig_gram<T_>(int, int, bool, const T_* const*, const T_* const*, double*, double*, const EigGeom&, hipStream_t);
template void launch_eig_combine<T_>(int, int, const T_* const*, T_* const*, const double*, const EigGeom&, hipStream_t);
template void launch_eig_residual<T_>(int, const T_* const*, const T_* const*, T_* const*, double* const*, double* const*, const double*, const EigGeom&,
                                      hipStream_t);
template void launch_eig_apply<T_>(int, bool, const T_* const*, T_* const*, const Op9<T_>&, const EigGeom&, hipStream_t);
#elif MGX_INST_KIND == 12
template void launch_eig_project_dots<T_>(int, int, const T_* const*, const T_* const*, double*, double*, const EigGeom&, hipStream_t);
template void launch_eig_project_sub<T_>(int, int, const T_* const*, T_* const*, const double*, const EigGeom&, hipStream_t);
#elif MGX_INST_KIND == 13
template void launch_reaction_shift<T_>(const T_*, const T_*, T_*, int, long, hipStream_t);
template void launch_theta_rhs<T_>(const VarLevel<T_>&, const T_*, const T_*, const T_*, T_*, double, hipStream_t);
#elif MGX_INST_KIND == 14
template void launch_newton_pass<T_>(const VarLevel<T_>&, bool, const T_*, const T_*, const T_*, const T_*, const T_*, const T_*, T_*, T_*, T_*,
                                     const NewtonPoly<T_>&, double*, double*, hipStream_t);
template void launch_newton_step_rhs<T_>(const VarLevel<T_>&, const T_*, const T_*, const T_*, const T_*, const T_*, T_*, const NewtonPoly<T_>&,
                                         double, hipStream_t);
#elif MGX_INST_KIND == 15
template void launch_quasi_pass<T_>(int, int, long, bool, bool, const T_*, const T_*, const T_*, const double*, const Quasi5Out<T_>&, T_*, T_*,
                                    const QuasiPoly<T_>&, double*, double*, hipStream_t);
#else
#error "MGX_INST_KIND must be 1 .. 15"
#endif
} // namespace mgx
