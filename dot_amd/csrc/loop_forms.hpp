// loop_forms.hpp -- which template instantiation three kernels of the L-BFGS iteration launch, stated once (host only, no HIP):
//   vertex gather      vertex_gather_kernel<true, 512, 2>         beyond two trips of the 256-thread form (4 dofs per lane and trip)
//   early merge        merge_tiles_early_kernel<512, .>           beyond two trips of the 256-thread form (a dof per lane and trip)
//   direction kernel   spmv_zp_wide_kernel (1024 threads)         beyond one trip of the 256-thread form (32 lane groups x 3 rows)
// Every reducing kernel runs LOOP_NB_RED workgroups, so a "trip" is a fixed number of dofs / rows whatever the mesh.  The launchers of
// k_loopvec.hip call these functions and nothing else; dotmi_loop_forms (what a handle launches) and dotmi_plan_loop_forms (host only:
// tests/test_loop_forms.py) evaluate the same three on their own counts, so neither can drift from the launchers.
// The counts are what the launch visits: scalar dofs (3 x vertices) for the gather and the merge, block rows (vertices) for the
// direction kernel; under the owner exchange the held vertices only.
// force (DOTMI_WIDE_FORMS, Tuning::wideForms): -1 = by size; any other value is a bit mask over the three kernels -- a set bit
// forces the wide form, a clear bit the narrow one.
#pragma once

namespace dotmi {

constexpr int LOOP_NB_RED = 256;     // = NB_RED (dotmi_internal.hpp), asserted in k_loopvec.hip like the two below
constexpr int LOOP_GATHER_R = 4;     // = GATHER_R: dofs per lane and trip of the 256-thread gather
constexpr int LOOP_SPMV_R = 3;       // = SPMV_R (k_dirbody.hpp): block rows per lane group and trip of the 256-thread direction kernel

constexpr int FORM_WIDE_GATHER = 1, FORM_WIDE_MERGE = 2, FORM_WIDE_SPMV = 4;   // the mask's bits (also dotmi_loop_forms' low bits)
constexpr int FORM_WIDE_ALL = FORM_WIDE_GATHER | FORM_WIDE_MERGE | FORM_WIDE_SPMV;

inline bool form_forced(int force, int bit, bool by_size) { return force < 0 ? by_size : (force & bit) != 0; }

// (the 512-thread gather exists in the device loop's instantiation only: the launcher asks for a launch with a controller)
inline bool gather_is_wide(long long ndof, int force)
{
    return form_forced(force, FORM_WIDE_GATHER, ndof > 2ll * LOOP_GATHER_R * LOOP_NB_RED * 256);
}
inline bool merge_early_is_wide(long long ndof, int force) { return form_forced(force, FORM_WIDE_MERGE, ndof > 2ll * LOOP_NB_RED * 256); }
inline bool spmv_zp_is_wide(long long nrows, int force)
{
    return form_forced(force, FORM_WIDE_SPMV, nrows > (long long)LOOP_NB_RED * 32 * LOOP_SPMV_R);
}

// the three as one mask
inline int loop_forms_mask(long long ndof_gather, long long ndof_merge, long long nrows_spmv, int force)
{
    return (gather_is_wide(ndof_gather, force) ? FORM_WIDE_GATHER : 0) | (merge_early_is_wide(ndof_merge, force) ? FORM_WIDE_MERGE : 0) |
           (spmv_zp_is_wide(nrows_spmv, force) ? FORM_WIDE_SPMV : 0);
}

// dotmi_loop_forms' further bits: the split merge, and which twolevel_backward_kernel<CW> the two-level back-solve launches
// (launch_gemv: CW column pairs across a workgroup, by the widest panel's columns) as 1 / 2 / 3 = 32 / 64 / 128 in bits 16-17
constexpr int FORM_SPLIT_MERGE = 8, FORM_TWOLEVEL_CW_SHIFT = 16;
inline int twolevel_backward_cw(int max_panel_cols) { return max_panel_cols / 2 <= 32 ? 32 : max_panel_cols / 2 <= 64 ? 64 : 128; }
inline int twolevel_backward_code(int max_panel_cols) { return twolevel_backward_cw(max_panel_cols) == 32 ? 1 : twolevel_backward_cw(max_panel_cols) == 64 ? 2 : 3; }

}  // namespace dotmi
