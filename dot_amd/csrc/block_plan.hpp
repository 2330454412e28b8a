// block_plan.hpp -- the planning of the subdomain block solve as a sequence of stages (host only): vertex sets -> dissection layout and
// form -> padded rows -> factor storage -> fill / reduce / merge lists -> tile schedule of the factorisation -> two-level panels.
// Plain data in, plain data out: no device call and no handle.  dotmi_create (build_device_mesh) runs the stages with the uploads of
// each stage's arrays in between; the host-only entries dotmi_plan_layout / _backsolve_tiles / _backsolve_form / _rank (dotmi_plan.cpp) run the
// first ones on the caller's mesh, so that what tests/test_host_logic.py pins is the code dotmi_create runs.
//
// Role in the reference: the ADMMDDTimeStepper constructor (ADMMDDTimeStepper.cpp:88-262: subdomain vertex sets, local maps); the
// layout, storage and schedules below are what CHOLMOD's analysis does behind CHOLMODSolver::analyze_pattern.
#pragma once
#include <cstdio>
#include <string>
#include <unordered_map>

#include "bs_tiles.hpp"

namespace dotmi {

inline bool mesh_is_valid(int nV, int nT, const int *T, const int *epart /* or null: the vertex indices only */, int nParts)
{
    for (int e = 0; e < nT; ++e) {
        if (epart && (epart[e] < 0 || epart[e] >= nParts)) return false;
        for (int k = 0; k < 4; ++k)
            if (T[4 * e + k] < 0 || T[4 * e + k] >= nV) return false;
    }
    return true;
}

// vertices of every part's elements, ascending and unique (an element whose part is out of range belongs to none)
inline std::vector<std::vector<int>> part_vertex_sets(int nT, const int *T, const int *epart, int nParts)
{
    std::vector<std::vector<int>> sets(nParts);
    for (int e = 0; e < nT; ++e)
        if (epart[e] >= 0 && epart[e] < nParts)
            for (int k = 0; k < 4; ++k) sets[epart[e]].push_back(T[4 * e + k]);
    for (auto &v : sets) {
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
    }
    return sets;
}

struct MeshGraph {   // the mesh as the stages read it: vertex adjacency incl. self (the block pattern of the global Hessian), rest positions
    int nV = 0;
    std::vector<int> adj_ptr, adj_idx;
    const double *Xrest = nullptr;
};
inline MeshGraph mesh_graph(int nV, int nT, const int *T, const double *Xrest)
{
    MeshGraph G{nV, {}, {}, Xrest};
    build_adjacency(nV, nT, T, G.adj_ptr, G.adj_idx);
    return G;
}

// ---- nested-dissection layout of the owned subdomains and the form of the block solve ------------------------------
struct LayoutRules {
    int ndLevels = -1;          // DOTMI_ND_LEVELS (Tuning)
    int ndMin = ND_MIN_SPLIT;   // DOTMI_ND_MIN
    bool ndMinByUser = false;
    int twoLevel = -1;          // DOTMI_TWO_LEVEL: 1 / 0 the form, -1 by the bytes of the one-pass form
    bool eligible = true;       // (not GSDD, which solves one subdomain at a time)
    bool keepDepth = false;     // the two-level form does not choose the depth (dotmi_plan_layout: the tree its caller asks for)
    bool log = false;           // DOTMI_FUSE_LOG
};
struct BlockLayout {
    std::vector<NdNode> nd;                               // the tree shared by the owned parts (root = 0)
    std::vector<std::vector<std::vector<int>>> region;    // [node][owned part] -> vertices of the leaf / separator
    bool twoLevel = false;
    int nmax = 0;                                         // padded size of every owned block
    long long onePassBytes = 0;                           // of the one-pass form over ALL parts (counted when the bytes decide)
};

// structural non-zeros of the one-pass form (explicit inverse) on a planned layout: every row of a region from the region's first
// column to its diagonal, live columns only -- x 8 = the bytes one application streams (dotmi_step_stats.precond_bytes)
inline long long one_pass_nnz(const std::vector<NdNode> &nd, const std::vector<std::vector<std::vector<int>>> &reg, int nParts)
{
    long long nnz = 0;
    const int nmax0 = nd[0].size;
    std::vector<int> usedBefore(nmax0 + 1);   // number of live columns before a padded position
    for (int ls = 0; ls < nParts; ++ls) {
        std::vector<uint8_t> live(nmax0, 0);
        for (size_t k = 0; k < nd.size(); ++k) {
            const int used = 3 * (int)reg[k][ls].size(), ro = nd_region_first_row(nd[k], used);
            std::fill(live.begin() + ro, live.begin() + ro + used, 1);
        }
        usedBefore[0] = 0;
        for (int c = 0; c < nmax0; ++c) usedBefore[c + 1] = usedBefore[c] + live[c];
        for (size_t k = 0; k < nd.size(); ++k) {
            const NdNode &N = nd[k];
            const int used = 3 * (int)reg[k][ls].size(), ro = nd_region_first_row(N, used);
            const int cb = N.a < 0 ? (ro & ~15) : N.off;
            for (int r = ro; r < ro + used; ++r) nnz += usedBefore[r + 1] - usedBefore[cb];
        }
    }
    return nnz;
}
constexpr long long TWO_LEVEL_FROM_BYTES = 240000000ll;   // one-pass bytes per application from which the two-level form is the default

// allSets: the vertex sets of ALL parts of the mesh; [p0, p1) the owned ones, which the layout is for
inline void choose_block_layout(const MeshGraph &G, const std::vector<std::vector<int>> &allSets, int p0, int p1,
                                const LayoutRules &R, BlockLayout &L)
{
    const std::vector<std::vector<int>> sets(allSets.begin() + p0, allSets.begin() + p1);
    // two-level form of the back-solve (DevTwoLevel): the block solve as a whole (not GSDD's subdomain at
    // a time); per subdomain, so sharded subdomains take it as well.  By default where the one-pass form would stream at least 240 MB per application on its own
    // layout: the three launches around the tile kernels and the split merge cost 25-40 us per iteration, the form saves bytes
    // and a third of the factorisation -- measured (profiles/r06_two_level.txt H): bar17K (197 MB) +21 % per step, monkey
    // (124 MB) +42 %, horse7K / 8 (107 MB) +8 %; kingkong18K / 18 (245 MB) -10 %, horse7K@r1:64 (681 MB) -12 %, 1 M tets
    // (3.8 GB) -16 %.  The form wants a tree of at least four levels with regions split down to ~200 scalars (the horse at
    // three levels / 384: +4 % instead of -12 %).
    const bool userDepth = R.ndLevels >= 0 || R.ndMinByUser || R.keepDepth;
    bool wantTwoLevel = R.eligible && R.twoLevel > 0;
    int lv = 0, mn = 0;
    auto plan = [&](bool twoLevelDepth) {
        lv = R.ndLevels;
        mn = R.ndMin;
        if (twoLevelDepth && !userDepth) {
            // sixteen leaves per subdomain where its size allows: four levels, regions split down to a fifteenth of the biggest
            // subdomain (between 128 and 256 scalars) -- 1 M tets / 256 (3.2 k dofs): 213, the same tree as with 256; 4.2 M tets /
            // 1024 (2.9 k dofs): 192, 16 leaves instead of 8: 13.8 -> 9.8 GB per application, the step -7 %; 192 k tets / 64:
            // 433 -> 325 MB, -7.5 % (profiles/r06_two_level.txt J)
            lv = std::max(4, nd_default_levels(allSets));
            int nsmax = 0;
            for (auto &v : allSets) nsmax = std::max(nsmax, 3 * (int)v.size());
            mn = std::min(256, std::max(128, nsmax / 15));
        } else if (lv < 0 && !R.ndMinByUser) {
            // depth and split threshold from ALL subdomains of the mesh: the same tree on every rank (nd_layout.hpp)
            nd_choose_depth(allSets, G.nV, G.adj_ptr, G.adj_idx, G.Xrest, BS_NARROW, mn, lv, mn);
        } else if (lv < 0) {
            lv = nd_default_levels(allSets);
        }
        if (R.log) fprintf(stderr, "dotmi: dissection: %d levels, regions split down to %d scalars\n", lv, mn);
        nd_plan(sets, G.nV, G.adj_ptr, G.adj_idx, G.Xrest, lv, mn, L.nd, L.region);
    };
    plan(wantTwoLevel);
    L.onePassBytes = 0;
    if (!wantTwoLevel && R.eligible && R.twoLevel < 0 && !L.nd.empty()) {
        // counted over ALL subdomains of the mesh, so that every rank of a sharded run -- and the single-GPU run it is
        // compared with -- takes the same form (a rank's own factors are private, but the forms differ in rounding)
        if (sets.size() == allSets.size()) {
            L.onePassBytes = 8 * one_pass_nnz(L.nd, L.region, (int)sets.size());
        } else if (L.nd[0].a >= 0) {
            std::vector<NdNode> treeAll;
            std::vector<std::vector<std::vector<int>>> regionAll;
            nd_plan(allSets, G.nV, G.adj_ptr, G.adj_idx, G.Xrest, lv, mn, treeAll, regionAll);
            if (!treeAll.empty()) L.onePassBytes = 8 * one_pass_nnz(treeAll, regionAll, (int)allSets.size());
        }
        if (L.nd[0].a >= 0 && L.onePassBytes >= TWO_LEVEL_FROM_BYTES) {   // (a tree that has separators at all)
            wantTwoLevel = true;
            if (!userDepth) plan(true);
        }
    }
    L.twoLevel = wantTwoLevel && !L.nd.empty() && L.nd[0].a >= 0;
    if (L.twoLevel) nd_relayout_leaves_first(L.nd);
    L.nmax = L.nd[0].size;
}

// ---- per owned part: padded position of every local vertex, structural non-zeros -------------------------------------
struct RowPlacement {
    std::vector<int> dofmap;                  // owned * nmax: padded local position -> global scalar dof, -1 = padding
    std::vector<std::vector<int>> partPos;    // owned parts: padded scalar position of the part's i-th vertex
    long long nnzX = 0;                       // every structural non-zero of the inverse factors is streamed once per back-solve
};
inline void place_rows(const BlockLayout &L, const std::vector<std::vector<int>> &allSets, int p0, int p1, RowPlacement &out)
{
    const int nParts = p1 - p0;
    out.partPos.assign(nParts, {});
    out.dofmap.assign((size_t)nParts * L.nmax, -1);
    for (int ls = 0; ls < nParts; ++ls) {
        const auto &pv = allSets[p0 + ls];
        std::unordered_map<int, int> posOf;
        posOf.reserve(pv.size() * 2);
        for (size_t nd = 0; nd < L.nd.size(); ++nd) {
            const auto &rv = L.region[nd][ls];
            const int ro = nd_region_first_row(L.nd[nd], 3 * (int)rv.size());
            for (size_t k = 0; k < rv.size(); ++k) {
                posOf[rv[k]] = ro + 3 * (int)k;
                for (int d = 0; d < 3; ++d) out.dofmap[(size_t)ls * L.nmax + ro + 3 * k + d] = 3 * rv[k] + d;
            }
        }
        out.partPos[ls].resize(pv.size());
        for (size_t i = 0; i < pv.size(); ++i) out.partPos[ls][i] = posOf.at(pv[i]);
    }
    out.nnzX = one_pass_nnz(L.nd, L.region, nParts);
}

// ---- factor storage: 64-row blocks (RowTile) ---------------------------------------------------------------
struct FactorStorage {
    int ntl = 0;                         // row blocks per subdomain
    std::vector<RowTile> rtab, rtabM;    // per (owned subdomain, row block): its range; two-level form: a separator's second range
    std::vector<uint8_t> leafTile;       // two-level form: the row block belongs to a leaf
    size_t wOnePass = 0, wTotal = 0;     // doubles: the first ranges; with the second ranges
    // offset in W of (memory row r, column c) of owned subdomain ls, or -1 when that place is not stored
    long long addr(int ls, int r, int c) const
    {
        const size_t at = (size_t)ls * ntl + (r >> 6);
        const RowTile &R = rtab[at], &M = rtabM[at];
        if (R.off < 0) return -1;
        if (c < R.c0) {
            if (M.off < 0 || c < M.c0 || c >= M.c0 + M.ld) return -1;
            return M.off + (long long)(r & 63) * M.ld + (c - M.c0);
        }
        if (c >= R.c0 + R.ld) return -1;
        return R.off + (long long)(r & 63) * R.ld + (c - R.c0);
    }
};
// a RowTile table as the parallel arrays plan_subdomain_tiles and dotmi_part_matrix read
struct RowTileArrays {
    std::vector<long long> off;
    std::vector<int> ld, c0;
};
inline RowTileArrays row_tile_arrays(const std::vector<RowTile> &t)
{
    RowTileArrays A;
    for (const RowTile &R : t) {
        A.off.push_back(R.off);
        A.ld.push_back(R.ld);
        A.c0.push_back(R.c0);
    }
    return A;
}
inline void plan_factor_storage(const BlockLayout &L, const std::vector<int> &dofmap, int nParts, FactorStorage &F)
{
    const int ntl = F.ntl = L.nmax / 64;
    F.rtab.assign((size_t)std::max(nParts, 1) * ntl, RowTile{-1, 0, 0});
    F.rtabM = F.rtab;
    F.leafTile.assign(ntl, 0);
    F.wTotal = 0;
    // first column a row of the layout can have non-zero: that of its tree node
    std::vector<int> nodeC0(L.nmax, 0), nodeOfRow(L.nmax, -1);
    for (size_t k = 0; k < L.nd.size(); ++k) {
        const NdNode &N = L.nd[k];
        const bool leaf = N.a < 0;
        for (int r = leaf ? N.off : N.offS; r < (leaf ? N.off + N.size : N.offS + N.sizeS); ++r) {
            nodeC0[r] = N.off;
            if (leaf) F.leafTile[r / 64] = L.twoLevel;
            else nodeOfRow[r] = (int)k;
        }
    }
    for (int ls = 0; ls < nParts; ++ls)
        for (int J = 0; J < ntl; ++J) {
            bool live = false;
            for (int r = 64 * J; r < 64 * J + 64 && !live; ++r) live = dofmap[(size_t)ls * L.nmax + r] >= 0;
            if (!live) continue;   // identity padding only: nothing stored, nothing read
            const int c0 = nodeC0[64 * J];
            F.rtab[(size_t)ls * ntl + J] = RowTile{(long long)F.wTotal, 64 * (J + 1) - c0, c0};
            F.wTotal += (size_t)64 * (64 * (J + 1) - c0);
        }
    F.wOnePass = F.wTotal;
    if (!L.twoLevel) return;
    // two-level form: a separator's row blocks store the LEAF columns of their sub-tree in a second range (their main range starts
    // at the sub-tree's first separator column)
    for (int ls = 0; ls < nParts; ++ls)
        for (int J = 0; J < ntl; ++J) {
            const size_t at = (size_t)ls * ntl + J;
            if (F.rtab[at].off < 0 || nodeOfRow[64 * J] < 0) continue;
            const NdNode &N = L.nd[nodeOfRow[64 * J]];
            // (+ 16: a leaf range is a multiple of 64 columns, often a power of two -- consecutive rows of a panel would then
            // start on the same HBM channels)
            F.rtabM[at] = RowTile{(long long)F.wTotal, N.endL - N.offL + 16, N.offL};
            F.wTotal += (size_t)64 * F.rtabM[at].ld;
        }
}

// ---- dense fill list: per scalar of every 3x3 block of the principal sub-matrix -------------------------------------
struct FillLists {
    std::vector<long long> fill_dst, pad_dst;
    std::vector<int> fill_src;
    std::vector<int4> fillBlk;   // (owned subdomain, memory row, memory column) of the blocks' corners, for the tile pattern
};
inline void build_fill_lists(const MeshGraph &G, const std::vector<std::vector<int>> &allSets, int p0, int p1, const RowPlacement &rows,
                             int nmax, const FactorStorage &F, FillLists &out)
{
    std::vector<int> g2p(G.nV, -1);
    for (int ls = 0; ls < p1 - p0; ++ls) {
        const auto &pv = allSets[p0 + ls];
        for (int i = 0; i < (int)pv.size(); ++i) g2p[pv[i]] = rows.partPos[ls][i];
        for (int i = 0; i < (int)pv.size(); ++i) {
            const int v = pv[i];
            for (int k = G.adj_ptr[v]; k < G.adj_ptr[v + 1]; ++k) {
                const int j = g2p[G.adj_idx[k]];
                if (j < 0) continue;
                const int r0 = rows.partPos[ls][i];
                for (int rc = 0; rc < 9; ++rc) out.fill_dst.push_back(F.addr(ls, r0 + rc / 3, j + rc % 3));
                out.fill_src.push_back(k);
                out.fillBlk.push_back(make_int4(ls, r0, j, 0));
            }
        }
        for (int r = 0; r < nmax; ++r)
            if (rows.dofmap[(size_t)ls * nmax + r] < 0) {
                const long long a = F.addr(ls, r, r);
                if (a >= 0) out.pad_dst.push_back(a);
            }
        for (int v : pv) g2p[v] = -1;
    }
}

// reduce_partial_p: the tiles of a part that hold a group of 16 columns, ascending (a tile's range starts on a multiple of 16)
inline void build_reduce_lists(const std::vector<std::vector<int2>> &ranges, int nParts, int nmax, std::vector<int> &rptr,
                               std::vector<int> &ridx)
{
    const int ng = nmax / 16;
    rptr.assign((size_t)std::max(nParts, 1) * (ng + 1), 0);
    for (int ls = 0; ls < nParts; ++ls) {
        std::vector<std::vector<int>> lists(ng);
        for (size_t b = 0; b < ranges[ls].size(); ++b)
            for (int g = ranges[ls][b].x / 16; g <= (ranges[ls][b].y - 1) / 16 && g < ng; ++g)
                lists[g].push_back((int)b | (std::min(16, ranges[ls][b].y - 16 * g) << 24));   // tile | columns of the group it holds
        for (int g = 0; g < ng; ++g) {
            rptr[(size_t)ls * (ng + 1) + g] = (int)ridx.size();
            ridx.insert(ridx.end(), lists[g].begin(), lists[g].end());
        }
        rptr[(size_t)ls * (ng + 1) + ng] = (int)ridx.size();
    }
    if (ridx.empty()) ridx.push_back(0);
}

// ---- merge lists (owned parts only) ------------------------------------------------------------------------------------
struct MergeLists {
    std::vector<int> vp_ptr, vp_off;   // per vertex: owned subdomain * nmax + padded position of its copies
    std::vector<int> mp, ment;         // per scalar dof: the tile partials that make up its value (DevParts::mt_ptr / mt_ent)
    std::vector<int2> mw;              // the lists once more, interleaved by wavefront (DevParts::mt_wave / mt_il); empty: not used
    std::vector<int> il;
    long long count = 0;               // tile partials one merge reads (either form)
    bool splitMerge = false;
    bool walk = false;                 // the one-launch merge walks mp / ment
};
inline void build_merge_lists(int nV, const std::vector<std::vector<int>> &allSets, int p0, int p1, const RowPlacement &rows, int nmax,
                              int nbmax, const std::vector<std::vector<int2>> &ranges, int splitMergeRule /* DOTMI_SPLIT_MERGE */,
                              bool twoLevel, bool gsdd, MergeLists &M)
{
    const int nParts = p1 - p0;
    M.vp_ptr.assign(nV + 1, 0);
    for (int ls = 0; ls < nParts; ++ls)
        for (int v : allSets[p0 + ls]) M.vp_ptr[v + 1]++;
    for (int v = 0; v < nV; ++v) M.vp_ptr[v + 1] += M.vp_ptr[v];
    M.vp_off.resize(M.vp_ptr[nV]);
    {
        std::vector<int> cur(M.vp_ptr.begin(), M.vp_ptr.end() - 1);
        for (int ls = 0; ls < nParts; ++ls) {
            const auto &pv = allSets[p0 + ls];
            for (int i = 0; i < (int)pv.size(); ++i) M.vp_off[cur[pv[i]]++] = ls * nmax + rows.partPos[ls][i];
        }
    }
    if (gsdd) return;   // (one subdomain at a time: neither form of the merge)
    // merge straight from the tile partials (merge_tiles_kernel): per global scalar dof the ppart entries that make
    // up its value -- subdomain after subdomain (vp order), inside a subdomain the tiles that hold the column in
    // tile order; the first entry of a subdomain is stored complemented.  Same sums, same order as
    // reduce_partial_p + merge.
    const long long ppartN = (long long)nParts * nbmax * nmax;
    // Big meshes: the walk over a dof's ~20 tile partials is a walk over scattered 8-byte words and 4-byte list entries
    // (1 M tets: 75 us per iteration at 0.26 of the HBM peak); the two-launch form reads the partials coalesced in the
    // subdomains' own order and gathers one 24-byte triple per (vertex, subdomain).  Small meshes keep the one launch.
    M.splitMerge = splitMergeRule >= 0 ? (splitMergeRule != 0) : (3ll * nV >= 400000 || ppartN >= (1ll << 31));
    if (twoLevel) M.splitMerge = true;   // (the leaves' results are finished on the per-subdomain sums psub)
    const bool lists = !M.splitMerge && ppartN < (1ll << 31);
    std::vector<int> &mp = M.mp, &ment = M.ment;
    mp.assign(lists ? (size_t)3 * nV + 1 : 0, 0);
    for (int v = 0; v < nV; ++v)
        for (int d = 0; d < 3; ++d) {
            for (int k = M.vp_ptr[v]; k < M.vp_ptr[v + 1]; ++k) {
                const int ls = M.vp_off[k] / nmax, col = M.vp_off[k] % nmax + d;
                bool first = true;
                for (size_t b = 0; b < ranges[ls].size(); ++b)
                    if (col >= ranges[ls][b].x && col < ranges[ls][b].y) {
                        ++M.count;
                        if (lists) {
                            const int off = (int)(((long long)ls * nbmax + (long long)b) * nmax + col);
                            ment.push_back(first ? ~off : off);
                        }
                        first = false;
                    }
            }
            if (lists) mp[(size_t)3 * v + d + 1] = (int)ment.size();
        }
    // Few subdomains with long rows in short tiles (bunny5K: 8-16 rows per tile): a column is covered by dozens of tiles,
    // ~30 scattered partials per dof against ~10 on bar17K -- there too the coalesced within-subdomain sum first is the
    // shorter way (bunny5K 1.395 -> 1.367 ms per step; the stiff monkey, 8 per dof, loses 3 % with it)
    const bool longLists = splitMergeRule < 0 && M.count >= 24ll * 3 * nV;
    if (lists && longLists) M.splitMerge = true;
    M.walk = lists && !longLists;
    if (!M.walk) return;
    // the lists once more, interleaved by wavefront (DevParts::mt_il): what the merge kernels walk when they visit
    // every dof (the owner exchange's vertex lists keep the CSR walk)
    const int n3 = 3 * nV, nw = (n3 + 63) / 64;
    std::vector<int2> &mw = M.mw;
    std::vector<int> &il = M.il;
    mw.resize(nw);
    for (int w = 0; w < nw; ++w) {
        int L = 0;
        for (int l = 0; l < 64 && 64 * w + l < n3; ++l) L = std::max(L, mp[64 * w + l + 1] - mp[64 * w + l]);
        mw[w] = make_int2((int)il.size(), L);
        il.resize(il.size() + (size_t)64 * L, MT_PAD);
        for (int l = 0; l < 64 && 64 * w + l < n3; ++l)
            for (int q = 0, e = mp[64 * w + l]; e < mp[64 * w + l + 1]; ++q, ++e) il[(size_t)mw[w].x + 64 * q + l] = ment[e];
    }
    if (il.empty()) il.push_back(MT_PAD);
    if (il.size() >= (size_t)1 << 31) {   // (beyond 32-bit offsets: the CSR walk only)
        mw.clear();
        il.clear();
    }
}

// ---- tile schedule of the factorisation (tile_factor.hpp) ------------------------------------------------
struct ScheduleRules {
    int eagerMin = 0;              // DOTMI_TILE_EAGER_MIN (0: by the number of subdomains)
    int eagerMinRmul = -1;         // DOTMI_TILE_EAGER_MIN_RMUL
    bool eagerMinRmulByUser = false;
    int tileFlow = -1;             // DOTMI_TILE_FLOW
    int groups = 1;                // subdomain groups of the level launches (tile_factor.hpp; the dataflow launch has one)
    bool hfill = false;            // DOTMI_TILE_HFILL: H tiles built inside their first task from entry lists (build_tile_fill)
};
struct FactorSchedule {
    TileSchedule S;                    // with its per-group level ranges and clear tiles (S.groupLevel, S.clearStart)
    std::vector<int> fillPerm, fillStart;   // the dense fill's entries group by group (partition_by_group)
    bool flow = false;                 // the dataflow launch (tile_flow_kernel) instead of one launch per level
    std::vector<int> depPtr, depIdx;   // its dependencies
};
// The fill of the work buffer as per-tile entry lists (TileSchedule::fillPtr / fill, tile_factor.hpp): every stored scalar the dense
// fill writes (fill_dst >= 0; source hval_idx(fill_src, rc)) and every 1.0 of the identity padding (pad_dst; source -1) goes to the
// list of the clear tile that holds its address -- through the row blocks' main table and, in the two-level form, the second one --
// and every task planned with init == 2 receives its tile's range.  Inside a list the entries ascend by source, so neighbouring
// lanes gather neighbouring scalars of Hval.  Returns the error text, empty when every address has found its tile.
inline std::string build_tile_fill(TileSchedule &S, const double *W2, const FillLists &fill, const RowTileArrays &rt,
                                   const RowTileArrays &rtM)
{
    struct Blk {
        long long off;
        int ld, c0;
    };
    std::vector<Blk> blks;
    for (const RowTileArrays *A : {&rt, &rtM})
        for (size_t k = 0; k < A->off.size(); ++k)
            if (A->off[k] >= 0 && A->ld[k] > 0) blks.push_back({A->off[k], A->ld[k], A->c0[k]});
    std::sort(blks.begin(), blks.end(), [](const Blk &a, const Blk &b) { return a.off < b.off; });
    std::unordered_map<long long, int> tileAt;   // offset of a clear tile's origin in the work buffer -> its index
    tileAt.reserve(S.clearTiles.size() * 2);
    for (size_t k = 0; k < S.clearTiles.size(); ++k) tileAt[S.clearTiles[k] - W2] = (int)k;
    std::vector<std::vector<TileFillEntry>> lists(S.clearTiles.size());
    auto put = [&](long long d, long long src) -> bool {
        auto it = std::upper_bound(blks.begin(), blks.end(), d, [](long long v, const Blk &b) { return v < b.off; });
        if (it == blks.begin()) return false;
        const Blk &B = *(it - 1);
        const long long local = d - B.off;
        if (local >= 64ll * B.ld) return false;
        const int j = (int)(local / B.ld), col = (int)(local % B.ld) + B.c0, i = col / TILE, k = col % TILE;
        auto at = tileAt.find(B.off + (long long)TILE * i - B.c0);
        if (at == tileAt.end() || S.clearLd[at->second] != B.ld || src >= (1ll << 31)) return false;
        lists[at->second].push_back(TileFillEntry{(int)src, (unsigned short)(k * TILE_LDS_LD + j), 0});
        return true;
    };
    for (size_t e = 0; e < fill.fill_dst.size(); ++e)
        if (fill.fill_dst[e] >= 0 && !put(fill.fill_dst[e], (long long)hval_idx(fill.fill_src[e / 9], (int)(e % 9))))
            return "tile fill: a scalar of H has no tile of the work buffer";
    for (long long d : fill.pad_dst)
        if (!put(d, -1)) return "tile fill: a padding scalar has no tile of the work buffer";
    S.fillPtr.assign(1, 0);
    S.fill.clear();
    for (auto &l : lists) {
        std::stable_sort(l.begin(), l.end(), [](const TileFillEntry &a, const TileFillEntry &b) { return a.src < b.src; });
        S.fill.insert(S.fill.end(), l.begin(), l.end());
        if (S.fill.size() >= (size_t)1 << 31) return "tile fill: more than 2^31 entries";
        S.fillPtr.push_back((int)S.fill.size());
    }
    for (TileTask &t : S.tasks) {
        if (t.init != 2) continue;
        auto at = tileAt.find(t.c - W2);
        if (at == tileAt.end()) return "tile fill: a task starts from a tile without an entry list";
        t.fillFirst = S.fillPtr[at->second];
        t.fillCount = S.fillPtr[at->second + 1] - t.fillFirst;
    }
    return std::string();
}

// rt / rtM: row_tile_arrays of the storage's two tables; W, W2: the device addresses of the factor and the work buffer, which the
// tasks carry
inline void plan_factor_schedule(int nParts, int nmax, const std::vector<int> &dofmap, const std::vector<int4> &fillBlk,
                                 const RowTileArrays &rt, const RowTileArrays &rtM, const uint8_t *leafTile /* two-level form, or null */,
                                 double *W, double *W2, const ScheduleRules &R, FactorSchedule &out)
{
    const int nt = nmax / TILE;
    std::vector<std::vector<uint8_t>> live(nParts, std::vector<uint8_t>(nt, 0)), pat(nParts);
    for (int ls = 0; ls < nParts; ++ls) {
        for (int r = 0; r < nmax; ++r)
            if (dofmap[(size_t)ls * nmax + r] >= 0) live[ls][r / TILE] = 1;
        pat[ls].assign((size_t)nt * nt, 0);
    }
    for (const int4 &fb : fillBlk) {
        const int ls = fb.x, r0 = fb.y, c0 = fb.z;   // memory row / column of the 3x3 block's corner
        for (int a = 0; a < 3; a += 2)
            for (int b = 0; b < 3; b += 2) {
                const int I = (c0 + b) / TILE, J = (r0 + a) / TILE;   // column-major element (c0+b, r0+a)
                if (I <= J) pat[ls][(size_t)I * nt + J] = 1;
            }
    }
    // eager partial updates shorten the launches of a latency-bound factorisation (few subdomains) and cost tile
    // traffic in a throughput-bound one (measured: profiles/r03_factor_tiles.txt)
    // (round 4: with very few tile columns in total -- bunny5K: 8 x 32 -- the chain of dependent tasks is all there is, and
    // the dataflow launch runs finer eager tasks at no barrier cost: 2 / 2 there, factor 0.43 -> 0.39 ms; horse7K, 8 x 47,
    // keeps 4 / 4)
    const bool tiny = (long long)nParts * nt <= 320;
    const int eagerMin = R.eagerMin > 0 ? R.eagerMin : (tiny ? 2 : nParts <= 64 ? 4 : 8);
    const int eagerChunk = tiny ? 2 : nParts <= 64 ? 4 : 8;   // early products per eager task
    // the last task of a Q tile (sum, then the multiplication with -Q_jj): up to 64 subdomains it keeps ONE early product and
    // hands the others to a task that runs beside DIAG(j) -- the launch between two diagonal launches is then as short as
    // before round 5 (bar17K 1.125 -> 1.077 ms); above, where every launch is several rounds of workgroups, it keeps them
    // like any other task and saves the partial sum's round trip (1 M tets 15.5 -> 14.5 ms)
    const int eagerMinRmul = R.eagerMinRmul >= -1 && R.eagerMinRmulByUser ? R.eagerMinRmul : (nParts <= 64 ? 1 : -1);
    TileSchedule &S = out.S;
    std::vector<SubdomainTiles> subs(nParts);
    size_t nTasks = 0;
    int maxLevel = 0;
    {
        size_t sn = 0;
        for (int ls = 0; ls < nParts; ++ls) {
            const size_t at = (size_t)ls * nt;
            plan_subdomain_tiles(ls, nt, W, &rt.off[at], &rt.ld[at], &rt.c0[at], live[ls], pat[ls], W2, sn, subs[ls].tasks,
                                 subs[ls].clearTiles, subs[ls].clearLd, S.flops, S.qTiles, eagerMin, eagerChunk, 0, true, eagerMinRmul,
                                 leafTile ? &rtM.off[at] : nullptr, leafTile ? &rtM.ld[at] : nullptr,
                                 leafTile ? &rtM.c0[at] : nullptr, leafTile, R.hfill);
            nTasks += subs[ls].tasks.size();
            for (auto &t : subs[ls].tasks) maxLevel = std::max(maxLevel, t.level);
        }
    }
    // Dataflow or levels (profiles/r04_factor_flow.txt): per task the dataflow launch pays a ticket, a look at its
    // dependencies' flags and write-through stores, and it runs the level kernel's 77 KB workgroups -- it wins where the
    // levels are launches of less than one round of workgroups, i.e. the chain of dependent tasks paces the phase
    // (bunny5K / 8 subdomains: 217 tasks per level, 0.57 -> 0.41 ms), and loses where the levels are several rounds
    // (bar17K / 32: 1000 per level, 1.11 -> 1.21 ms; 1 M tets: 15 -> 23 ms).
    const size_t nLevels = (size_t)std::max(maxLevel, 1);
    out.flow = nTasks > 0 && (R.tileFlow > 0 || (R.tileFlow < 0 && nTasks / nLevels <= 512));
    finish_grouped_schedule(subs, out.flow ? 1 : R.groups, S);
    {
        std::vector<int> subOf(fillBlk.size());
        for (size_t e = 0; e < fillBlk.size(); ++e) subOf[e] = fillBlk[e].x;
        partition_by_group(subOf.data(), subOf.size(), S.groupOf, (int)S.groupLevel.size() - 1, out.fillPerm, out.fillStart);
    }
    if (out.flow) {
        build_tile_deps(S.tasks, S.prods, out.depPtr, out.depIdx);
        if (out.depIdx.empty()) out.depIdx.push_back(0);
    }
}

// ---- two-level form: the panels ------------------------------------------------------------------------------------
struct TwoLevelPanels {
    std::vector<int4> panel;   // DevTwoLevel::panel
    std::vector<long long> rowBase, rowDst;
    std::vector<int> rowPos, gPtr, gIdx;
    std::vector<int2> items;
    long long packedN = 0, panelBytes = 0;
    int maxRows = 0, maxCols = 0;
};
// panels: per (subdomain, leaf) the separator vertices next to the leaf (a mesh edge into it; no fill path leaves a leaf),
// rows ascending in the layout.  Returns the error text, empty when the form can run.
inline std::string plan_two_level_panels(const MeshGraph &G, const BlockLayout &L, const std::vector<std::vector<int>> &allSets, int p0,
                                         int p1, const FactorStorage &F, TwoLevelPanels &T)
{
    const int nParts = p1 - p0, nmax = L.nmax;
    std::vector<std::vector<int>> sub((size_t)nParts * nmax);
    std::vector<int> sepPos(G.nV, -1);
    for (int ls = 0; ls < nParts; ++ls) {
        for (size_t k = 0; k < L.nd.size(); ++k) {
            const auto &rv = L.region[k][ls];
            const int ro = nd_region_first_row(L.nd[k], 3 * (int)rv.size());
            if (L.nd[k].a >= 0)
                for (size_t q = 0; q < rv.size(); ++q) sepPos[rv[q]] = ro + 3 * (int)q;
        }
        for (size_t k = 0; k < L.nd.size(); ++k) {
            const NdNode &N = L.nd[k];
            if (N.a >= 0 || L.region[k][ls].empty()) continue;
            const auto &rv = L.region[k][ls];
            std::vector<int> rows;   // padded positions of the coupled separator vertices
            for (int v : rv)
                for (int e = G.adj_ptr[v]; e < G.adj_ptr[v + 1]; ++e)
                    if (sepPos[G.adj_idx[e]] >= 0) rows.push_back(sepPos[G.adj_idx[e]]);
            std::sort(rows.begin(), rows.end());
            rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
            if (rows.empty()) continue;
            // (the kernels take two columns per lane: the panel starts on an even column -- one column of the leaf's identity
            // padding in front when its first live column is odd: zeros in M and in the right-hand side -- and ends at the
            // leaf's end, a multiple of 64)
            const int c0 = nd_region_first_row(N, 3 * (int)rv.size()) & ~1, used = N.off + N.size - c0;
            T.panel.push_back(make_int4((int)T.rowBase.size(), 3 * (int)rows.size(), ls * nmax + c0, used));
            T.maxRows = std::max(T.maxRows, 3 * (int)rows.size());
            T.maxCols = std::max(T.maxCols, used);
            T.panelBytes += 8ll * 3 * (long long)rows.size() * used;
            for (int rp : rows)
                for (int d = 0; d < 3; ++d) {
                    const long long a = F.addr(ls, rp + d, c0);
                    if (a < 0) return "two-level layout: a panel row has no storage";
                    sub[(size_t)ls * nmax + rp + d].push_back((int)T.rowBase.size());
                    T.rowBase.push_back(a);
                    T.rowDst.push_back(T.packedN);
                    T.packedN += used;
                    T.rowPos.push_back(ls * nmax + rp + d);
                }
        }
        for (int v : allSets[p0 + ls]) sepPos[v] = -1;
    }
    T.gPtr.assign((size_t)nParts * nmax + 1, 0);
    for (size_t i = 0; i < sub.size(); ++i) {
        T.gPtr[i] = (int)T.gIdx.size();
        T.gIdx.insert(T.gIdx.end(), sub[i].begin(), sub[i].end());
    }
    T.gPtr[sub.size()] = (int)T.gIdx.size();
    if (T.gIdx.empty()) T.gIdx.push_back(0);
    if (T.panel.empty()) T.panel.push_back(make_int4(0, 0, 0, 0));
    if (T.rowBase.empty()) {
        T.rowBase.push_back(0);
        T.rowDst.push_back(0);
        T.rowPos.push_back(0);
    }
    if (T.maxRows > 7000)   // (twolevel_backward_kernel keeps a panel's p_G entries in LDS)
        return "two-level form: a leaf couples to " + std::to_string(T.maxRows) + " separator rows (limit 7000): split the regions "
               "further (DOTMI_ND_LEVELS / DOTMI_ND_MIN) or use DOTMI_TWO_LEVEL=0";
    for (size_t q = 0; q < T.panel.size(); ++q)
        for (int k0 = 0; k0 < T.panel[q].y; k0 += 8) T.items.push_back(make_int2((int)q, k0));
    if (T.items.empty()) T.items.push_back(make_int2(0, 0));
    return std::string();
}

}  // namespace dotmi
