// bs_forms.hpp -- the forms of the subdomain back-solve kernels (k_backsolve.hip), stated once (host readable: no HIP).
// A single-pass tile is held in registers by a FAMILY of lanes -- one wavefront of a pack, the 256-thread workgroup, the 512-thread
// workgroup.  Each family has a table of forms, ascending: a lane holds `chunks` column pairs of every row (columns c0 + 2 lane +
// 2 lanes m, m < chunks) and `sub` rows per pass, so the longest row a form takes is 2 x lanes x chunks -- computed, never written;
// rlds: the right-hand side and the accumulators live in LDS.  bs_select_form maps (family, longest row of a tile) to the form: the
// device dispatch (backsolve_block, backsolve_pack) instantiates the tile body per entry through it, the 256 / 512 choice of
// launch_gemv_part and the host-only entry dotmi_plan_backsolve_forms (tests/backsolve_cases.py) use it as bs_form_index -- a form added
// to a table is compiled, reached, reported and tested without a further edit.  BS_WAVE / BS_NARROW / BS_LONG (dotmi_internal.hpp),
// by which the job table (bs_tiles.hpp) sorts the tiles, are the capacities of the three families.
#pragma once
#include <type_traits>
#include <utility>

namespace dotmi {

struct BsForm {
    int chunks, sub;
    bool rlds;
};
constexpr int BSF_PACK = 0, BSF_NARROW = 1, BSF_WIDE = 2;
constexpr int BSF_LANES[3] = {64, 256, 512};
constexpr BsForm BSF_PACK_FORMS[] = {{1, 32, false}, {2, 16, false}};
constexpr BsForm BSF_NARROW_FORMS[] = {{1, 32, false}, {2, 16, false}, {3, 8, false}, {5, 8, false}, {6, 8, true}};
constexpr BsForm BSF_WIDE_FORMS[] = {{1, 32, false}, {2, 16, false}, {4, 8, false}, {5, 8, false}};

constexpr int bs_form_count(int fam)
{
    return fam == BSF_PACK ? std::extent<decltype(BSF_PACK_FORMS)>::value
                           : fam == BSF_NARROW ? std::extent<decltype(BSF_NARROW_FORMS)>::value : std::extent<decltype(BSF_WIDE_FORMS)>::value;
}
constexpr BsForm bs_form(int fam, int i) { return fam == BSF_PACK ? BSF_PACK_FORMS[i] : fam == BSF_NARROW ? BSF_NARROW_FORMS[i] : BSF_WIDE_FORMS[i]; }
// longest row (columns, first column of the tile to the diagonal) form i of the family holds, and the family's last form
constexpr int bs_form_capacity(int fam, int i) { return 2 * BSF_LANES[fam] * bs_form(fam, i).chunks; }
constexpr int bs_family_capacity(int fam) { return bs_form_capacity(fam, bs_form_count(fam) - 1); }
constexpr bool bs_forms_ascend(int fam, int i = 1)
{
    return i >= bs_form_count(fam) || (bs_form_capacity(fam, i - 1) < bs_form_capacity(fam, i) && bs_forms_ascend(fam, i + 1));
}
static_assert(bs_forms_ascend(BSF_PACK) && bs_forms_ascend(BSF_NARROW) && bs_forms_ascend(BSF_WIDE), "the first form that holds a row is the smallest");
// The form that takes a tile whose longest row has len columns -- the first whose capacity holds it: calls f(integral constant I) with
// its index.  The table is walked at compile time, so a caller that instantiates a kernel body per I (bs_form(FAM, I) is a constant
// expression there) gets one comparison and one instantiation per entry; the last form takes whatever is left, as the last `else` of
// a chain written out would (the job table gives a launch no tile beyond its family's capacity).
// (Capacities as integral constants in one flat expression: evaluated by a call, or with an index formed first and compared again, the
// kernels came out with other scalar registers and spills.)
template <int FAM, class F, int... I>
__attribute__((always_inline)) constexpr void bs_select_form(int len, F &&f, std::integer_sequence<int, I...>)
{
    (void)(((I + 1 == sizeof...(I) || len <= std::integral_constant<int, bs_form_capacity(FAM, I)>::value) &&
            (f(std::integral_constant<int, I>()), true)) || ...);
}
template <int FAM, class F>
__attribute__((always_inline)) constexpr void bs_select_form(int len, F &&f)
{
    bs_select_form<FAM>(len, f, std::make_integer_sequence<int, bs_form_count(FAM)>());
}
// the same as a number, for a family chosen at run time; bs_form_count(fam) if the family holds no row that long
constexpr int bs_form_index(int fam, int len)
{
    int idx = bs_form_count(fam);
    auto set = [&idx](auto I) { idx = I; };
    if (len > bs_family_capacity(fam)) return idx;
    if (fam == BSF_PACK) bs_select_form<BSF_PACK>(len, set);
    else if (fam == BSF_NARROW) bs_select_form<BSF_NARROW>(len, set);
    else bs_select_form<BSF_WIDE>(len, set);
    return idx;
}
static_assert(bs_form_index(BSF_NARROW, 1) == 0 && bs_form_index(BSF_NARROW, bs_form_capacity(BSF_NARROW, 1) + 1) == 2 &&
                  bs_form_index(BSF_WIDE, bs_family_capacity(BSF_WIDE) + 1) == bs_form_count(BSF_WIDE),
              "the first form that holds the row");

// Rows beyond the wide family's capacity: the two-phase kernel (backsolve_long_kernel), BSL_THREADS lanes x BSL_CH chunks, BSL_SUB rows
// per pass, on column chunks of BS_LONG_CHUNK per workgroup.  The job table (bs_long_chunks, bs_tiles.hpp) counts its work items in
// this same number, NOT in the wide family's capacity: they were one number until the register tile grew from 4096 to 5120 columns, and a
// tile of more than 8192 columns then lost its last work item (bunny5K as one subdomain, 14 976 columns: |H M r - r| / |r| = 2)
constexpr int BSL_THREADS = 512, BSL_CH = 4, BSL_SUB = 8;
constexpr int BS_LONG_CHUNK = 2 * BSL_THREADS * BSL_CH;   // 4096 columns

}  // namespace dotmi
