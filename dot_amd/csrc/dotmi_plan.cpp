// dotmi_plan.cpp -- the host-only planning entries of include/dotmi.h (dotmi_plan_*, dotmi_partition): the planners of block_plan.hpp,
// patches.hpp / vpatches.hpp, partition.hpp, ic_plan.hpp, coarse_plan.hpp and pd_plan.hpp on the caller's arrays.  Plain C++ for the
// host compiler: no handle, no device, no call into the HIP runtime -- the object links into a program without it (plan_check.cpp
// does, under the address and undefined-behaviour sanitizers).  Built once and linked into both libraries.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/dotmi.h"
#include "block_plan.hpp"
#include "coarse_plan.hpp"
#include "ic_plan.hpp"
#include "loop_forms.hpp"
#include "partition.hpp"
#include "pd_plan.hpp"
#include "time_integration.hpp"
#include "tuning.hpp"
#include "vpatches.hpp"

using namespace dotmi;

namespace {

// The planners take the addresses of the factor and the work buffer; the entries below have no buffers and return offsets, so they
// plan on this base.  It is never dereferenced: only differences to it leave a function.
double *offset_base() { return reinterpret_cast<double *>(1ull << 40); }

// The row-block table of n_blocks blocks of nt tile rows, one block's storage behind the other's: tile row j keeps the columns
// [64 c0[j], 64 (j + 1)) if live[j], else nothing (off = -1).  live, c0 == NULL: every row from column 0.  Returns the doubles per block.
long long row_block_table(int n_blocks, int nt, const uint8_t *live, const int32_t *c0, RowTileArrays &rt)
{
    const size_t rows = (size_t)n_blocks * nt;
    rt = RowTileArrays{std::vector<long long>(rows, -1), std::vector<int>(rows, 0), std::vector<int>(rows, 0)};
    long long at = 0;
    for (int b = 0; b < n_blocks; ++b)
        for (int j = 0; j < nt; ++j) {
            if (live && !live[j]) continue;
            const size_t r = (size_t)b * nt + j;
            rt.c0[r] = c0 ? 64 * c0[j] : 0;
            rt.ld[r] = 64 * (j + 1) - rt.c0[r];
            rt.off[r] = at;
            at += 64ll * rt.ld[r];
        }
    return at / n_blocks;
}

// ONE block planned on offset_base(), its scratch tiles behind its storage, the tasks sorted by level (stable: the planner's order inside
// a level).  leaf_tile != NULL: the two-level form -- a separator row j keeps the leaf tile columns [c0m[j], c0m[j] + ntm[j]) in rtM.
struct BlockTasks {
    RowTileArrays rt, rtM;
    long long storage = 0;   // doubles of both tables
    std::vector<TileTaskL> tasks;
};
BlockTasks plan_one_block(int nt, const uint8_t *live, const uint8_t *pattern, const int32_t *c0, int eager_min, int eager_chunk,
                          const uint8_t *leaf_tile, const int32_t *c0m, const int32_t *ntm)
{
    BlockTasks B;
    B.storage = row_block_table(1, nt, live, c0, B.rt);
    B.rtM = RowTileArrays{std::vector<long long>(nt, -1), std::vector<int>(nt, 0), std::vector<int>(nt, 0)};   // (none stored)
    if (leaf_tile)
        for (int j = 0; j < nt; ++j) {
            if (!live[j] || leaf_tile[j] || ntm[j] <= 0) continue;
            B.rtM.c0[j] = 64 * c0m[j];
            B.rtM.ld[j] = 64 * ntm[j] + 16;
            B.rtM.off[j] = B.storage;
            B.storage += 64ll * B.rtM.ld[j];
        }
    double *const W = offset_base();
    const std::vector<uint8_t> lv(live, live + nt), pat(pattern, pattern + (size_t)nt * nt);
    TileSchedule S;   // (the clear tiles and the counters are not exported)
    size_t sn = 0;
    plan_subdomain_tiles(0, nt, W, B.rt.off.data(), B.rt.ld.data(), B.rt.c0.data(), lv, pat, W + B.storage, sn, B.tasks, S.clearTiles,
                         S.clearLd, S.flops, S.qTiles, std::max(1, eager_min), std::max(1, eager_chunk), 0, true, -1,
                         leaf_tile ? B.rtM.off.data() : nullptr, leaf_tile ? B.rtM.ld.data() : nullptr,
                         leaf_tile ? B.rtM.c0.data() : nullptr, leaf_tile);
    std::stable_sort(B.tasks.begin(), B.tasks.end(), [](const TileTaskL &a, const TileTaskL &b) { return a.level < b.level; });
    return B;
}

// n_blocks blocks of nt x nt tiles in one layout (rt: every row block from tile column 0; the work buffer behind the factor buffer):
// every block planned (hfill: for tiles built from entry lists) and the grouped level table over them.  Returns the doubles per block.
long long plan_blocks(int n_blocks, int nt, const uint8_t *live, const uint8_t *pattern, int eager_min, int eager_chunk, int groups,
                      bool hfill, RowTileArrays &rt, TileSchedule &S)
{
    const long long tot = row_block_table(n_blocks, nt, nullptr, nullptr, rt);
    double *const W = offset_base(), *const W2 = W + (long long)n_blocks * tot;
    std::vector<SubdomainTiles> subs(n_blocks);
    size_t sn = 0;
    for (int b = 0; b < n_blocks; ++b) {
        std::vector<uint8_t> lv(live + (size_t)b * nt, live + (size_t)(b + 1) * nt);
        std::vector<uint8_t> pat(pattern + (size_t)b * nt * nt, pattern + (size_t)(b + 1) * nt * nt);
        plan_subdomain_tiles(b, nt, W, &rt.off[(size_t)b * nt], &rt.ld[(size_t)b * nt], &rt.c0[(size_t)b * nt], lv, pat, W2, sn,
                             subs[b].tasks, subs[b].clearTiles, subs[b].clearLd, S.flops, S.qTiles, std::max(1, eager_min),
                             std::max(1, eager_chunk), 0, true, -1, nullptr, nullptr, nullptr, nullptr, hfill);
    }
    finish_grouped_schedule(subs, groups, S);
    return tot;
}

void out(int32_t *dst, const std::vector<int> &src)
{
    if (dst) std::copy(src.begin(), src.end(), dst);
}

// hdr[5] of the two vertex-patch entries
void vpatch_header(const HostVPatches &H, int32_t *hdr)
{
    const int32_t h[5] = {H.nPatches, H.PE, H.PV, H.PO, H.RUN};
    std::copy(h, h + 5, hdr);
}

}  // namespace

extern "C" {

// host-only: no device is touched
int dotmi_plan_shards(int32_t nParts, const int32_t *part_scalar_size, int32_t world, int32_t *first_part)
{
    if (nParts < 0 || world < 1 || !first_part || (nParts > 0 && !part_scalar_size)) return DOTMI_E_INVALID;
    std::vector<double> cost(nParts + 1, 0.0);
    for (int p = 0; p < nParts; ++p) cost[p + 1] = cost[p] + (double)part_scalar_size[p] * part_scalar_size[p];
    first_part[0] = 0;
    first_part[world] = nParts;
    for (int r = 1; r < world; ++r) {
        const double target = cost[nParts] * r / world;
        int c = (int)(std::lower_bound(cost.begin(), cost.end(), target) - cost.begin());
        if (c > 0 && target - cost[c - 1] < cost[c] - target) --c;
        c = std::min(std::max(c, first_part[r - 1]), nParts);
        first_part[r] = c;
    }
    return 0;
}

// host-only: which of the loop's three kernels take their wide form on launches of these sizes (loop_forms.hpp: the functions the
// launchers of k_loopvec.hip and dotmi_loop_forms call), as the mask 1 gather | 2 early merge | 4 direction kernel
int dotmi_plan_loop_forms(int64_t ndof_gather, int64_t ndof_merge, int64_t nrows_spmv, int32_t force, int32_t *out)
{
    if (ndof_gather < 0 || ndof_merge < 0 || nrows_spmv < 0 || !out) return DOTMI_E_INVALID;
    *out = loop_forms_mask(ndof_gather, ndof_merge, nrows_spmv, force);
    return 0;
}

// host-only: the time integration rule of one step (time_integration.hpp: what dotmi_step and the entries of dotmi_reconfig.hip plan with)
int dotmi_plan_time_integration(int32_t kind, double dt, double dt_prev, int32_t levels, double *c0, double *c1, double *gamma,
                                double *dt_eff)
{
    if (kind != DOTMI_TIT_BE && kind != DOTMI_TIT_BDF2) return DOTMI_E_INVALID;
    if (!(dt > 0) || !std::isfinite(dt) || levels < 0 || levels > 1) return DOTMI_E_INVALID;
    if (kind == DOTMI_TIT_BDF2 && levels == 1 && (!(dt_prev > 0) || !std::isfinite(dt_prev))) return DOTMI_E_INVALID;
    const TitPlan p = tit_plan(kind, dt, dt_prev, levels);
    if (c0) *c0 = p.c0;
    if (c1) *c1 = p.c1;
    if (gamma) *gamma = p.gamma;
    if (dt_eff) *dt_eff = p.dt_eff;
    return 0;
}

// host-only: the back-solve's form tables (bs_forms.hpp: what k_backsolve.hip instantiates and dispatches on), family after family
int dotmi_plan_backsolve_forms(int32_t cap, int32_t *forms, int32_t *counts)
{
    if (!counts || cap < 0 || (cap > 0 && !forms)) return DOTMI_E_INVALID;
    int n = 0;
    for (int fam : {BSF_PACK, BSF_NARROW, BSF_WIDE})
        for (int i = 0; i < bs_form_count(fam); ++i, ++n) {
            if (!forms) continue;
            if (n >= cap) return DOTMI_E_INVALID;
            const BsForm f = bs_form(fam, i);
            const int32_t row[6] = {fam, BSF_LANES[fam], f.chunks, f.sub, f.rlds, bs_form_capacity(fam, i)};
            // (the table's own map puts a row of that length on this form, and one column more on the next)
            if (bs_form_index(fam, row[5]) != i || bs_form_index(fam, row[5] + 1) != i + 1) return DOTMI_E_INVALID;
            std::copy(row, row + 6, forms + 6 * (size_t)n);
        }
    const int32_t c[4] = {n, BSL_THREADS, BSL_SUB, BS_LONG_CHUNK};
    std::copy(c, c + 4, counts);
    return 0;
}

// host-only: the element patches of patches.hpp for all elements of a mesh.  First call with elem == NULL for the sizes
// (n_patches, pv, n_slots), then with arrays of nPatches*PE (elem), 4*nPatches*PE (tl, epos: uint16), nPatches*PV (pv_gid,
// pv_slot), nPatches (pv_cnt), nPatches*(PV+1) (c_ptr: uint16) and 2*nV (pp_rng).  tests/test_patches.py checks the
// invariants the element pass relies on and replays the two-stage gradient sum in numpy.
int dotmi_plan_patches(int32_t nV, int32_t nT, const int32_t *T, const double *X, int32_t PE, int32_t *n_patches, int32_t *pv,
                       int32_t *n_slots, int32_t *elem, uint16_t *tl, uint16_t *epos, int32_t *pv_gid, int32_t *pv_slot,
                       int32_t *pv_cnt, uint16_t *c_ptr, int32_t *pp_rng)
{
    if (nV < 1 || nT < 1 || !T || !X || (PE != 256 && PE != 512) || !n_patches || !pv || !n_slots) return DOTMI_E_INVALID;
    std::vector<int> all(nT);
    for (int e = 0; e < nT; ++e) all[e] = e;
    const HostPatches H = build_patches(nV, T, X, all, PE);
    *n_patches = H.nPatches;
    *pv = H.PV;
    *n_slots = H.nSlots;
    if (!elem) return 0;
    std::copy(H.elem.begin(), H.elem.end(), elem);
    std::copy(H.tl.begin(), H.tl.end(), tl);
    std::copy(H.epos.begin(), H.epos.end(), epos);
    std::copy(H.pv_gid.begin(), H.pv_gid.end(), pv_gid);
    std::copy(H.pv_slot.begin(), H.pv_slot.end(), pv_slot);
    std::copy(H.pv_cnt.begin(), H.pv_cnt.end(), pv_cnt);
    std::copy(H.c_ptr.begin(), H.c_ptr.end(), c_ptr);
    std::copy(H.pp_rng.begin(), H.pp_rng.end(), pp_rng);
    return 0;
}

// host-only: the vertex patches of vpatches.hpp (see include/dotmi.h)
int dotmi_plan_vpatches(int32_t nV, int32_t nT, const int32_t *T, const double *X, int32_t PE, int32_t max_own, int32_t *hdr,
                        int32_t *owner, int32_t *elem, int32_t *eown, int32_t *runlen)
{
    if (nV < 1 || nT < 1 || !T || !X || PE < 1 || max_own < 1 || !hdr) return DOTMI_E_INVALID;
    const HostVPatches H = build_vpatches(nV, nT, T, X, PE, max_own);
    vpatch_header(H, hdr);
    if (!owner || H.nPatches == 0) return 0;
    for (int p = 0; p < H.nPatches; ++p) {
        const uint16_t *cp = &H.c_ptr[(size_t)p * (H.PO + 1)];
        for (int lv = 0; lv < H.po_cnt[p]; ++lv) {
            const int v = H.pv_gid[(size_t)p * H.PV + lv];
            owner[v] = p;
            if (runlen) runlen[v] = cp[lv + 1] - cp[lv];
        }
    }
    if (elem) std::copy(H.elem.begin(), H.elem.end(), elem);
    if (eown)
        for (size_t s = 0; s < H.eown.size(); ++s) eown[s] = H.eown[s];
    return 0;
}

// host-only: the owned vertices' static operands in patch order (vpatches.hpp: build_vpatch_records, what dotmi_create uploads as
// DevVPatches::orec) from the caller's flat arrays; see include/dotmi.h
int dotmi_plan_vpatch_records(int32_t nV, int32_t nT, const int32_t *T, const double *X, int32_t PE, int32_t max_own, const double *mass,
                              const uint8_t *fixed, const int32_t *vp_ptr, const int32_t *vp_off, const uint8_t *fixed2, int32_t *hdr,
                              int32_t *pv_gid, int32_t *po_cnt, double *rec_mass, int32_t *rec_fixed, int32_t *rec_cnt, int32_t *rec_off)
{
    if (nV < 1 || nT < 1 || !T || !X || PE < 1 || max_own < 1 || !mass || !fixed || !vp_ptr || !vp_off || !hdr) return DOTMI_E_INVALID;
    const HostVPatches H = build_vpatches(nV, nT, T, X, PE, max_own);
    vpatch_header(H, hdr);
    if (!pv_gid || H.nPatches == 0) return 0;
    if (!po_cnt || !rec_mass || !rec_fixed || !rec_cnt || !rec_off) return DOTMI_E_INVALID;
    std::vector<VpOwnRec> R = build_vpatch_records(H, mass, fixed, vp_ptr, vp_off);
    if (fixed2) refix_vpatch_records(vpatch_own_gid(H), fixed2, R);   // (what dotmi_refix does to the handle's copy)
    std::copy(H.pv_gid.begin(), H.pv_gid.end(), pv_gid);
    std::copy(H.po_cnt.begin(), H.po_cnt.end(), po_cnt);
    for (size_t i = 0; i < R.size(); ++i) {
        rec_mass[i] = R[i].mass;
        rec_fixed[i] = R[i].fixed;
        rec_cnt[i] = R[i].cnt;
        for (int c = 0; c < 4; ++c) rec_off[4 * i + c] = R[i].off[c];
    }
    return 0;
}

// host-only: the level schedule of tile_factor.hpp for ONE block of nt x nt tiles with the given upper tile pattern, in the
// compact row-block layout (c0[j] = first tile column stored for tile row j, c0[j] <= every pattern entry of column j).
// Offsets are in doubles into one array: the factor storage first, the scratch tiles after it (*scratch_base).
//   tasks: 11 int64 per task  {level, form, init, post, nprod, first product, c offset, q offset (-1), ldc, ldq, offset of the tile written}
//   prods:  4 int64 per product {a offset, b offset, lda, ldb}
// With tasks == NULL only the counts are returned.  The tests execute the schedule in numpy, level after level, and
// compare with a dense inverse Cholesky factor (tests/test_tile_schedule.py).
static int plan_tile_schedule_impl(int32_t nt, const uint8_t *live, const uint8_t *pattern, const int32_t *c0, int32_t eager_min,
                                   int32_t eager_chunk, int64_t *tasks, int64_t *prods, int64_t *n_tasks, int64_t *n_prods,
                                   int64_t *n_levels, int64_t *storage, int64_t *scratch_base, int64_t *row_off, int32_t *row_ld,
                                   const uint8_t *leaf_tile, const int32_t *c0m, const int32_t *ntm, int64_t *row_off_m,
                                   int32_t *row_ld_m)
{
    if (nt < 1 || !live || !pattern || !c0 || !n_tasks || !n_prods) return DOTMI_E_INVALID;
    const BlockTasks B = plan_one_block(nt, live, pattern, c0, eager_min, eager_chunk, leaf_tile, c0m, ntm);
    const std::vector<TileTaskL> &all = B.tasks;
    size_t np = 0;
    for (auto &t : all) np += t.prods.size();
    *n_tasks = (int64_t)all.size();
    *n_prods = (int64_t)np;
    if (n_levels) *n_levels = all.empty() ? 0 : all.back().level;
    if (storage) *storage = B.storage;
    if (scratch_base) *scratch_base = B.storage;
    if (row_off) std::copy(B.rt.off.begin(), B.rt.off.end(), row_off);
    if (row_ld) std::copy(B.rt.ld.begin(), B.rt.ld.end(), row_ld);
    if (row_off_m) std::copy(B.rtM.off.begin(), B.rtM.off.end(), row_off_m);
    if (row_ld_m) std::copy(B.rtM.ld.begin(), B.rtM.ld.end(), row_ld_m);
    if (!tasks || !prods) return 0;
    const double *const W = offset_base();
    size_t pi = 0;
    for (size_t k = 0; k < all.size(); ++k) {
        const TileTask &t = all[k].t;
        const int64_t row[11] = {all[k].level, t.form, t.init, t.post, (int64_t)all[k].prods.size(), (int64_t)pi, t.c - W,
                                 t.q ? t.q - W : -1, t.ldc, t.ldq, t.o - W};
        std::copy(row, row + 11, tasks + 11 * k);
        for (auto &pr : all[k].prods) {
            const int64_t q[4] = {pr.a - W, pr.b - W, pr.lda, pr.ldb};
            std::copy(q, q + 4, prods + 4 * pi++);
        }
    }
    return 0;
}

int dotmi_plan_tile_schedule(int32_t nt, const uint8_t *live, const uint8_t *pattern, const int32_t *c0, int32_t eager_min,
                             int32_t eager_chunk, int64_t *tasks, int64_t *prods, int64_t *n_tasks, int64_t *n_prods,
                             int64_t *n_levels, int64_t *storage, int64_t *scratch_base, int64_t *row_off, int32_t *row_ld)
{
    return plan_tile_schedule_impl(nt, live, pattern, c0, eager_min, eager_chunk, tasks, prods, n_tasks, n_prods, n_levels, storage,
                                   scratch_base, row_off, row_ld, nullptr, nullptr, nullptr, nullptr, nullptr);
}
// host-only: the same schedule in the TWO-LEVEL form (tile_factor.hpp, twoLevel; a leaves-first block): leaf_tile[t] = tile row t
// belongs to a leaf; a separator's row block j stores the leaf tile columns [c0m[j], c0m[j] + ntm[j]) of its sub-tree in a second
// range (row_off_m / row_ld_m) and its main range starts at its sub-tree's first separator column c0[j]
int dotmi_plan_tile_schedule_two_level(int32_t nt, const uint8_t *live, const uint8_t *pattern, const int32_t *c0,
                                       const uint8_t *leaf_tile, const int32_t *c0m, const int32_t *ntm, int32_t eager_min,
                                       int32_t eager_chunk, int64_t *tasks, int64_t *prods, int64_t *n_tasks, int64_t *n_prods,
                                       int64_t *n_levels, int64_t *storage, int64_t *row_off, int32_t *row_ld, int64_t *row_off_m,
                                       int32_t *row_ld_m)
{
    if (!leaf_tile || !c0m || !ntm) return DOTMI_E_INVALID;
    return plan_tile_schedule_impl(nt, live, pattern, c0, eager_min, eager_chunk, tasks, prods, n_tasks, n_prods, n_levels, storage,
                                   nullptr, row_off, row_ld, leaf_tile, c0m, ntm, row_off_m, row_ld_m);
}

// host-only: the subdomain groups of the level launches (tile_factor.hpp, plan_tile_groups): group_of[i] for n_parts weights;
// returns the number of groups used (groups clamped to [1, n_parts]), or an error
int dotmi_plan_tile_groups(int32_t n_parts, const int64_t *weight, int32_t groups, int32_t *group_of)
{
    if (n_parts < 1 || !weight || !group_of) return DOTMI_E_INVALID;
    std::vector<long long> w(weight, weight + n_parts);
    std::vector<int> g(n_parts, 0);
    const int G = plan_tile_groups(n_parts, w.data(), groups, g.data());
    std::copy(g.begin(), g.end(), group_of);
    return G;
}

// host-only: the grouped level table plan_factor_schedule builds, for n_blocks blocks of nt x nt tiles (live / pattern per block,
// every row block stored from tile column 0, block b's storage behind block b - 1's).
//   tasks: 6 int64 per task, in the order of the task array {group, level inside the group (from 1), block, offset of the tile
//          written, post, products};  clear: 2 int64 per cleared tile {group, offset};  group_level[g + 1] - group_level[g] =
//          levels of group g;  fill_perm / fill_start: the n_fill entries of a list whose entry e belongs to block fill_sub[e],
//          group by group (partition_by_group).
// With tasks == NULL only the counts are returned.  Returns the number of groups used.  tests/test_tile_groups.py
int dotmi_plan_grouped_tile_schedule(int32_t n_blocks, int32_t nt, const uint8_t *live, const uint8_t *pattern, int32_t eager_min,
                                     int32_t eager_chunk, int32_t groups, int64_t *tasks, int64_t *n_tasks, int32_t *group_of,
                                     int32_t *group_level, int64_t *clear, int64_t *n_clear, int32_t n_fill, const int32_t *fill_sub,
                                     int32_t *fill_perm, int32_t *fill_start)
{
    if (n_blocks < 1 || nt < 1 || !live || !pattern || !n_tasks || !n_clear || n_fill < 0 || (n_fill > 0 && !fill_sub))
        return DOTMI_E_INVALID;
    for (int e = 0; e < n_fill; ++e)
        if (fill_sub[e] < 0 || fill_sub[e] >= n_blocks) return DOTMI_E_INVALID;
    RowTileArrays rt;
    TileSchedule S;
    plan_blocks(n_blocks, nt, live, pattern, eager_min, eager_chunk, groups, false, rt, S);
    const double *const W = offset_base();
    const int G = (int)S.groupLevel.size() - 1;
    *n_tasks = (int64_t)S.tasks.size();
    *n_clear = (int64_t)S.clearTiles.size();
    if (!tasks) return G;
    if (!group_of || !group_level || !clear || !fill_perm || !fill_start) return DOTMI_E_INVALID;
    std::copy(S.groupOf.begin(), S.groupOf.end(), group_of);
    std::copy(S.groupLevel.begin(), S.groupLevel.end(), group_level);
    for (int g = 0; g < G; ++g) {
        for (int l = S.groupLevel[g]; l < S.groupLevel[g + 1]; ++l)
            for (int k = S.levelStart[l]; k < S.levelStart[l + 1]; ++k) {
                const TileTask &t = S.tasks[k];
                const int64_t row[6] = {g, l - S.groupLevel[g] + 1, t.sub, t.o - W, t.post, t.nprod};
                std::copy(row, row + 6, tasks + 6 * (size_t)k);
            }
        for (int k = S.clearStart[g]; k < S.clearStart[g + 1]; ++k) {
            clear[2 * (size_t)k] = g;
            clear[2 * (size_t)k + 1] = S.clearTiles[k] - W;
        }
    }
    std::vector<int> perm, start;
    partition_by_group(fill_sub, (size_t)n_fill, S.groupOf, G, perm, start);
    std::copy(perm.begin(), perm.end(), fill_perm);
    std::copy(start.begin(), start.end(), fill_start);
    return G;
}

// host-only: what the two entries below return of a schedule planned with hfill and its entry lists (build_tile_fill).
//   counts[8] = {tasks, clear tiles, entries, fill blocks, padding scalars, groups, doubles of one buffer, 0}
//   tasks: 10 int64 each, in the order of the task array {group, level inside the group (from 1), block, offset of the c tile and
//          of the tile written (each in its own buffer: the work buffer, or the factor buffer for the inversion's tiles and the tile
//          a diagonal task writes), init, post, first entry, entries, form};
//   clear: 5 int64 per clear tile {group, offset in the work buffer, leading dimension, first entry, entries};
//   entry_pos / entry_src: per entry its place in the 64 x 65 LDS tile and its scalar of Hval (-1: the padding's 1.0).
static void export_tile_fill(const TileSchedule &S, const double *W, const double *W2, int64_t *tasks, int64_t *clear,
                             int32_t *entry_pos, int32_t *entry_src)
{
    const int G = (int)S.groupLevel.size() - 1;
    for (int g = 0; g < G; ++g) {
        for (int l = S.groupLevel[g]; l < S.groupLevel[g + 1]; ++l)
            for (int k = S.levelStart[l]; k < S.levelStart[l + 1]; ++k) {
                const TileTask &t = S.tasks[k];
                const bool inv = t.form == TF_INV;   // (its tiles lie in the factor buffer, like the tile a diagonal task writes)
                const int64_t row[10] = {g, l - S.groupLevel[g] + 1, t.sub, t.c - (inv ? W : W2),
                                         t.o - (inv || t.post == TP_DIAG ? W : W2), t.init, t.post, t.fillFirst, t.fillCount, t.form};
                std::copy(row, row + 10, tasks + 10 * (size_t)k);
            }
        for (int k = S.clearStart[g]; k < S.clearStart[g + 1]; ++k) {
            const int64_t row[5] = {g, S.clearTiles[k] - W2, S.clearLd[k], S.fillPtr[k], S.fillPtr[k + 1] - S.fillPtr[k]};
            std::copy(row, row + 5, clear + 5 * (size_t)k);
        }
    }
    for (size_t e = 0; e < S.fill.size(); ++e) {
        entry_pos[e] = S.fill[e].pos;
        entry_src[e] = S.fill[e].src;
    }
}

// host-only: the H tiles' entry lists (DOTMI_TILE_HFILL; build_tile_fill, block_plan.hpp) for n_blocks blocks of nt x nt tiles in the
// layout of dotmi_plan_grouped_tile_schedule, from the CALLER's fill lists: fill_dst[9 n_fill] (offsets in the work buffer, -1: not
// stored), fill_src[n_fill] (blocks of Hval), pad_dst[n_pad].  tasks == NULL: counts only.  Returns the groups used or an error
// (DOTMI_E_INVALID also when an address lies in no H-pattern tile).  tests/test_tile_fill.py
int dotmi_plan_tile_fill(int32_t n_blocks, int32_t nt, const uint8_t *live, const uint8_t *pattern, int32_t eager_min,
                         int32_t eager_chunk, int32_t groups, int64_t n_fill, const int64_t *fill_dst, const int32_t *fill_src,
                         int64_t n_pad, const int64_t *pad_dst, int64_t *counts, int64_t *tasks, int64_t *clear, int32_t *entry_pos,
                         int32_t *entry_src)
{
    if (n_blocks < 1 || nt < 1 || !live || !pattern || !counts || n_fill < 0 || n_pad < 0 || (n_fill > 0 && (!fill_dst || !fill_src)) ||
        (n_pad > 0 && !pad_dst))
        return DOTMI_E_INVALID;
    RowTileArrays rt, rtM;
    TileSchedule S;
    const long long tot = plan_blocks(n_blocks, nt, live, pattern, eager_min, eager_chunk, groups, true, rt, S);
    const double *const W = offset_base(), *const W2 = W + (long long)n_blocks * tot;
    FillLists fill;
    fill.fill_dst.assign(fill_dst, fill_dst + 9 * n_fill);
    fill.fill_src.assign(fill_src, fill_src + n_fill);
    fill.pad_dst.assign(pad_dst, pad_dst + n_pad);
    for (long long d : fill.fill_dst)
        if (d >= (long long)n_blocks * tot) return DOTMI_E_INVALID;
    for (long long d : fill.pad_dst)
        if (d < 0 || d >= (long long)n_blocks * tot) return DOTMI_E_INVALID;
    if (!build_tile_fill(S, W2, fill, rt, rtM).empty()) return DOTMI_E_INVALID;
    const int G = (int)S.groupLevel.size() - 1;
    const int64_t c[8] = {(int64_t)S.tasks.size(), (int64_t)S.clearTiles.size(), (int64_t)S.fill.size(), n_fill, n_pad, G,
                          (int64_t)n_blocks * tot, 0};
    std::copy(c, c + 8, counts);
    if (!tasks) return G;
    if (!clear || !entry_pos || !entry_src) return DOTMI_E_INVALID;
    export_tile_fill(S, W, W2, tasks, clear, entry_pos, entry_src);
    return G;
}

// host-only: the same for ALL parts of the caller's mesh, through the stages dotmi_create runs (block_plan.hpp: layout -- two_level:
// the leaves-first form with its second row-block table --, rows, storage, fill lists, level schedule with `groups` chains, entry
// lists); additionally returns the fill lists the entry lists were derived from: fill_dst[9 * counts[3]], fill_src[counts[3]],
// pad_dst[counts[4]].  tasks == NULL: counts only.
int dotmi_plan_tile_fill_mesh(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, const int32_t *epart, int32_t nParts,
                              int32_t groups, int32_t two_level, int64_t *counts, int64_t *tasks, int64_t *clear, int32_t *entry_pos,
                              int32_t *entry_src, int64_t *fill_dst, int32_t *fill_src, int64_t *pad_dst)
{
    if (nV < 1 || nT < 1 || !T || !Xrest || !epart || nParts < 1 || !counts || !mesh_is_valid(nV, nT, T, epart, nParts))
        return DOTMI_E_INVALID;
    const MeshGraph G = mesh_graph(nV, nT, T, Xrest);
    const std::vector<std::vector<int>> sets = part_vertex_sets(nT, T, epart, nParts);
    LayoutRules LR;
    LR.twoLevel = two_level ? 1 : 0;
    BlockLayout L;
    choose_block_layout(G, sets, 0, nParts, LR, L);
    RowPlacement rows;
    place_rows(L, sets, 0, nParts, rows);
    FactorStorage F;
    plan_factor_storage(L, rows.dofmap, nParts, F);
    const RowTileArrays rt = row_tile_arrays(F.rtab), rtM = row_tile_arrays(F.rtabM);
    FillLists fill;
    build_fill_lists(G, sets, 0, nParts, rows, L.nmax, F, fill);
    double *const W = offset_base();
    double *const W2 = W + (long long)F.wTotal;
    FactorSchedule FS;
    ScheduleRules SR;
    {   // the eager rules dotmi_create reads from the environment (DOTMI_TILE_EAGER_MIN, DOTMI_TILE_EAGER_MIN_RMUL)
        const Tuning tune = Tuning::from_env();
        SR.eagerMin = tune.tileEagerMin;
        SR.eagerMinRmul = tune.tileEagerMinRmul;
        SR.eagerMinRmulByUser = tune.tileEagerMinRmulByUser;
    }
    SR.tileFlow = 0;
    SR.groups = groups;
    SR.hfill = true;
    plan_factor_schedule(nParts, L.nmax, rows.dofmap, fill.fillBlk, rt, rtM, L.twoLevel ? F.leafTile.data() : nullptr, W, W2, SR, FS);
    if (!build_tile_fill(FS.S, W2, fill, rt, rtM).empty()) return DOTMI_E_INVALID;
    const TileSchedule &S = FS.S;
    const int Gn = (int)S.groupLevel.size() - 1;
    const int64_t c[8] = {(int64_t)S.tasks.size(), (int64_t)S.clearTiles.size(), (int64_t)S.fill.size(), (int64_t)fill.fill_src.size(),
                          (int64_t)fill.pad_dst.size(), Gn, (int64_t)F.wTotal, L.twoLevel ? 1 : 0};
    std::copy(c, c + 8, counts);
    if (!tasks) return Gn;
    if (!clear || !entry_pos || !entry_src || !fill_dst || !fill_src || !pad_dst) return DOTMI_E_INVALID;
    export_tile_fill(S, W, W2, tasks, clear, entry_pos, entry_src);
    std::copy(fill.fill_dst.begin(), fill.fill_dst.end(), fill_dst);
    std::copy(fill.fill_src.begin(), fill.fill_src.end(), fill_src);
    std::copy(fill.pad_dst.begin(), fill.pad_dst.end(), pad_dst);
    return Gn;
}

// host-only: the dependencies the dataflow kernel (tile_flow_kernel) waits on, for the task list dotmi_plan_tile_schedule
// returns (same arguments, same task order): task v may run once the tasks dep_idx[dep_ptr[v] .. dep_ptr[v+1]) have finished.
// With dep_idx == NULL only *n_deps is returned.  tests/test_tile_schedule.py executes the tasks in random orders that
// respect exactly these edges.
int dotmi_plan_tile_deps(int32_t nt, const uint8_t *live, const uint8_t *pattern, const int32_t *c0, int32_t eager_min,
                         int32_t eager_chunk, int64_t *dep_ptr, int64_t *dep_idx, int64_t *n_deps)
{
    if (nt < 1 || !live || !pattern || !c0 || !n_deps) return DOTMI_E_INVALID;
    const BlockTasks B = plan_one_block(nt, live, pattern, c0, eager_min, eager_chunk, nullptr, nullptr, nullptr);
    TileSchedule S;
    for (auto &t : B.tasks) {
        TileTask k = t.t;
        k.first = (int)S.prods.size();
        k.nprod = (int)t.prods.size();
        for (auto &p : t.prods) S.prods.push_back(p);
        S.tasks.push_back(k);
    }
    std::vector<int> depPtr, depIdx;
    build_tile_deps(S.tasks, S.prods, depPtr, depIdx);
    *n_deps = (int64_t)depIdx.size();
    if (!dep_ptr || !dep_idx) return 0;
    for (size_t k = 0; k < depPtr.size(); ++k) dep_ptr[k] = depPtr[k];
    for (size_t k = 0; k < depIdx.size(); ++k) dep_idx[k] = depIdx[k];
    return 0;
}

// host-only: the nested-dissection layout build_device_mesh() would use for parts [p0,p1)
int dotmi_plan_layout(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, const int32_t *epart,
                      int32_t nParts, int32_t p0, int32_t p1, int32_t levels, int32_t min_split, int32_t node_cap,
                      int32_t *nodes, int32_t *n_nodes, int32_t *nmax, int32_t *pos)
{
    if (nV < 1 || nT < 1 || !T || !Xrest || !epart || nParts < 1 || p0 < 0 || p1 > nParts || p0 > p1 || !n_nodes || !nmax ||
        !mesh_is_valid(nV, nT, T, epart, nParts))
        return DOTMI_E_INVALID;
    const MeshGraph G = mesh_graph(nV, nT, T, Xrest);
    const std::vector<std::vector<int>> allSets = part_vertex_sets(nT, T, epart, nParts);
    // dotmi_create's rule where the caller leaves them open: depth (and, with it, the split threshold) from ALL subdomains of the mesh
    // (the leaves-first layout of the two-level back-solve when the environment forces that form: DOTMI_TWO_LEVEL=1, on the tree the
    // caller asks for; the automatic choice of dotmi_create -- where the one-pass form would stream 240 MB or more, on at least four
    // levels -- is the caller's to mirror)
    LayoutRules R;
    R.ndLevels = levels;
    R.ndMin = min_split < 128 ? ND_MIN_SPLIT : min_split;
    R.ndMinByUser = min_split >= 128;
    R.twoLevel = Tuning::from_env().twoLevel > 0;
    R.keepDepth = true;
    BlockLayout L;
    choose_block_layout(G, allSets, p0, p1, R, L);
    const std::vector<NdNode> &tree = L.nd;
    *nmax = L.nmax;
    *n_nodes = (int32_t)tree.size();
    if (nodes) {
        if ((int)tree.size() > node_cap) return DOTMI_E_INVALID;
        for (size_t i = 0; i < tree.size(); ++i) {
            const NdNode &N = tree[i];
            const int32_t row[6] = {N.off, N.size, N.a, N.c, N.offS, N.sizeS};
            std::copy(row, row + 6, nodes + 6 * i);
        }
    }
    if (pos) {
        RowPlacement rows;
        place_rows(L, allSets, p0, p1, rows);
        for (const auto &pp : rows.partPos) pos = std::copy(pp.begin(), pp.end(), pos);
    }
    return 0;
}

// host-only: the job table of the back-solve launches dotmi_create builds for parts [p0, p1) of this mesh (bs_tiles.hpp) -- the
// product's own planners (nd_choose_depth / nd_plan, plan_backsolve_tiles) on the caller's mesh, no device touched.
// tiles: up to `cap` rows of 6 int32 {part (local), first row, rows, first column, tile index in the part, job}: job = index of
// the launch's workgroup that runs the tile -- 0 .. n_wide-1 in the 512-thread launch, then 0 .. n_narrow-1 one-tile jobs of the
// 256-thread launch, then n_narrow + k for the four tiles of pack k; tiles of the two-phase kernel (rows beyond 5120 columns)
// have job = -1.  counts: {tiles, n_wide, n_narrow, n_packs, n_long, nmax, shallow launch (0 / 1), few-subdomains rule (0 / 1)}.
int dotmi_plan_backsolve_tiles(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, const int32_t *epart, int32_t nParts,
                               int32_t p0, int32_t p1, int32_t cap, int32_t *tiles, int32_t *counts)
{
    if (nV < 1 || nT < 1 || !T || !Xrest || !epart || nParts < 1 || p0 < 0 || p1 > nParts || p0 > p1 || !counts ||
        !mesh_is_valid(nV, nT, T, epart, nParts))
        return DOTMI_E_INVALID;
    const MeshGraph G = mesh_graph(nV, nT, T, Xrest);
    const Tuning tune = Tuning::from_env();
    BlockLayout L;   // (the one-pass form's layout)
    choose_block_layout(G, part_vertex_sets(nT, T, epart, nParts), p0, p1, LayoutRules{tune.ndLevels, tune.ndMin, tune.ndMinByUser, 0}, L);
    const int nmax = L.nmax;
    BsTilePlan TP;
    plan_backsolve_tiles(L.nd, [&](int k, int ls) { return 3 * (int)L.region[k][ls].size(); }, p1 - p0, nmax,
                         BsTileRules{tune.tileRows, tune.tileRowsLong, tune.tilePasses, tune.wavePacks}, TP);
    const int nN = TP.ntiles - TP.ntilesWide;
    int n = 0;
    auto put = [&](const int4 &t, int job) {
        if (tiles && n < cap) {
            int32_t *o = tiles + 6 * (size_t)n;
            o[0] = t.x; o[1] = t.y; o[2] = t.z >> 16; o[3] = t.w; o[4] = t.z & 0xffff; o[5] = job;
        }
        ++n;
    };
    for (int j = 0; j < TP.ntiles; ++j) put(TP.tiles[j], j < TP.ntilesWide ? j : j - TP.ntilesWide);
    for (int k = 0; k < 4 * TP.nquad; ++k)
        if ((TP.tiles[TP.ntiles + k].z >> 16) > 0) put(TP.tiles[TP.ntiles + k], nN + k / 4);
    for (const int4 &t : TP.ltiles) put(t, -1);
    counts[0] = n; counts[1] = TP.ntilesWide; counts[2] = nN; counts[3] = TP.nquad; counts[4] = (int)TP.ltiles.size();
    counts[5] = nmax; counts[6] = TP.shallow ? 1 : 0; counts[7] = TP.fewTiles ? 1 : 0;
    return (tiles && n > cap) ? DOTMI_E_INVALID : 0;
}

// host-only: what one rank owns under dotmi_create's plan
int dotmi_plan_rank(int32_t nV, int32_t nT, const int32_t *T, const int32_t *epart, int32_t nParts, int32_t rank,
                    int32_t world, int32_t *p0, int32_t *p1, int32_t *elems, int32_t *n_elems, int32_t *v0, int32_t *v1,
                    int32_t *part_size)
{
    if (nV < 1 || nT < 1 || !T || !epart || nParts < 1 || world < 1 || rank < 0 || rank >= world) return DOTMI_E_INVALID;
    if (!mesh_is_valid(nV, nT, T, nullptr, nParts)) return DOTMI_E_INVALID;
    const std::vector<std::vector<int>> sets = part_vertex_sets(nT, T, epart, nParts);
    std::vector<int32_t> ps(nParts), first(world + 1);
    for (int pI = 0; pI < nParts; ++pI) ps[pI] = 3 * (int32_t)sets[pI].size();
    dotmi_plan_shards(nParts, ps.data(), world, first.data());
    if (p0) *p0 = first[rank];
    if (p1) *p1 = first[rank + 1];
    int ne = 0;
    for (int e = 0; e < nT; ++e)
        if (epart[e] >= first[rank] && epart[e] < first[rank + 1]) {
            if (elems) elems[ne] = e;
            ++ne;
        }
    if (n_elems) *n_elems = ne;
    if (v0) *v0 = (int32_t)((long long)nV * rank / world);
    if (v1) *v1 = (int32_t)((long long)nV * (rank + 1) / world);
    if (part_size) std::copy(ps.begin(), ps.end(), part_size);
    return 0;
}

// host-only: the built-in element partitioner (partition.hpp)
int dotmi_partition(int32_t nV, int32_t nT, const int32_t *T, const double *X, int32_t nParts, int32_t *epart)
{
    if (nV < 1 || nT < 1 || !T || !X || nParts < 1 || !epart || !mesh_is_valid(nV, nT, T, nullptr, nParts)) return DOTMI_E_INVALID;
    partition_elements(nV, nT, T, X, nParts, epart);
    return 0;
}

// host-only: the form of the block solve dotmi_create chooses for this mesh and partition when DOTMI_TWO_LEVEL is unset (0 = explicit
// inverse in one pass, 1 = two-level), and the bytes per application of the one-pass form on its own layout, counted over all
// subdomains, that decide it (>= 240 MB and a tree with separators: two-level)
int dotmi_plan_backsolve_form(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, const int32_t *epart, int32_t nParts,
                              int32_t *form, int64_t *one_pass_bytes)
{
    if (nV < 1 || nT < 1 || !T || !Xrest || !epart || nParts < 1 || !form || !mesh_is_valid(nV, nT, T, epart, nParts)) return DOTMI_E_INVALID;
    BlockLayout L;
    choose_block_layout(mesh_graph(nV, nT, T, Xrest), part_vertex_sets(nT, T, epart, nParts), 0, nParts, LayoutRules(), L);
    *form = L.twoLevel ? 1 : 0;
    if (one_pass_bytes) *one_pass_bytes = L.onePassBytes;
    return 0;
}

// host-only: the multicolour ordering and the lists of the block IC(0).  sizes[3] = {colours, lower blocks, products} always; the
// arrays (any may be NULL) as in ic_plan.hpp
int dotmi_plan_ic(int32_t nV, int32_t nT, const int32_t *T, int32_t *sizes, int32_t *colour, int32_t *pos, int32_t *lptr,
                  int32_t *lidx, int32_t *lsrc, int32_t *dsrc, int32_t *pptr, int32_t *pa, int32_t *pb)
{
    if (nV < 1 || nT < 1 || !T || !sizes || !mesh_is_valid(nV, nT, T, nullptr, 0)) return DOTMI_E_INVALID;
    const MeshGraph G = mesh_graph(nV, nT, T, nullptr);
    IcPlan P;
    ic_plan(nV, G.adj_ptr, G.adj_idx, P);
    const int32_t n[3] = {P.nColours, (int32_t)P.lidx.size(), (int32_t)P.pa.size()};
    std::copy(n, n + 3, sizes);
    out(colour, P.colour);
    out(pos, P.pos);
    out(lptr, P.lptr);
    out(lidx, P.lidx);
    out(lsrc, P.lsrc);
    out(dsrc, P.dsrc);
    out(pptr, P.pptr);
    out(pa, P.pa);
    out(pb, P.pb);
    return 0;
}

// host-only: the lists of the coarse assembly and of the per-iteration kernels.  sizes[3] = {pairs, entries, (vertex, subdomain)
// incidences} always; the arrays (any may be NULL) as in coarse_plan.hpp
int dotmi_plan_coarse(int32_t nV, int32_t nT, const int32_t *T, const int32_t *epart, int32_t nParts, int32_t *sizes, int32_t *pairS,
                      int32_t *pairT, int32_t *pairPtr, int32_t *pairBlk, int32_t *vsPtr, int32_t *vsIdx, int32_t *svPtr, int32_t *svIdx)
{
    if (nV < 1 || nT < 1 || !T || !epart || !sizes || nParts < 1 || nParts > COARSE_MAX_PARTS || !mesh_is_valid(nV, nT, T, epart, nParts))
        return DOTMI_E_INVALID;
    const MeshGraph G = mesh_graph(nV, nT, T, nullptr);
    CoarsePlan P;
    coarse_plan(nV, nT, T, epart, nParts, G.adj_ptr, G.adj_idx, P);
    const int32_t n[3] = {(int32_t)P.pairS.size(), (int32_t)P.pairBlk.size(), (int32_t)P.vsIdx.size()};
    std::copy(n, n + 3, sizes);
    out(pairS, P.pairS);
    out(pairT, P.pairT);
    out(pairPtr, P.pairPtr);
    out(pairBlk, P.pairBlk);
    out(vsPtr, P.vsPtr);
    out(vsIdx, P.vsIdx);
    out(svPtr, P.svPtr);
    out(svIdx, P.svIdx);
    return 0;
}

// host-only: the lists of W = H Z for the balanced coarse term (dotmi_set_dot_coarse_mode, mode 2).  sizes[2] = {(vertex, subdomain) entries,
// H blocks over all entries} always; the arrays (any may be NULL) as in coarse_plan.hpp (CoarseHzPlan)
int dotmi_plan_coarse_hz(int32_t nV, int32_t nT, const int32_t *T, const int32_t *epart, int32_t nParts, int32_t *sizes, int32_t *hzPtr,
                         int32_t *hzSub, int32_t *hzVert, int32_t *hzBlkPtr, int32_t *hzBlk, int32_t *hzTPtr, int32_t *hzTEnt)
{
    if (nV < 1 || nT < 1 || !T || !epart || !sizes || nParts < 1 || nParts > COARSE_MAX_PARTS || !mesh_is_valid(nV, nT, T, epart, nParts))
        return DOTMI_E_INVALID;
    const MeshGraph G = mesh_graph(nV, nT, T, nullptr);
    CoarsePlan P;
    coarse_plan(nV, nT, T, epart, nParts, G.adj_ptr, G.adj_idx, P);
    CoarseHzPlan Z;
    coarse_hz_plan(nV, nParts, P.vsPtr, P.vsIdx, G.adj_ptr, G.adj_idx, Z);
    const int32_t n[2] = {(int32_t)Z.hzSub.size(), (int32_t)Z.hzBlk.size()};
    std::copy(n, n + 2, sizes);
    out(hzPtr, Z.hzPtr);
    out(hzSub, Z.hzSub);
    out(hzVert, Z.hzVert);
    out(hzBlkPtr, Z.hzBlkPtr);
    out(hzBlk, Z.hzBlk);
    out(hzTPtr, Z.hzTPtr);
    out(hzTEnt, Z.hzTEnt);
    return 0;
}

// host-only: the scalar layout's padded size and the bytes one application of L^-1 reads from the factor
int dotmi_plan_pd(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, int32_t *padded, int64_t *apply_bytes)
{
    if (nV < 1 || nT < 1 || !T || !Xrest || !mesh_is_valid(nV, nT, T, nullptr, 0)) return DOTMI_E_INVALID;
    const MeshGraph G = mesh_graph(nV, nT, T, Xrest);
    PdPlan P;
    pd_plan(nV, G.adj_ptr, G.adj_idx, Xrest, P);
    if (padded) *padded = P.nmax;
    if (apply_bytes) *apply_bytes = 8 * P.readElems;
    return 0;
}

}  // extern "C"
