// coarse_plan.hpp -- host-only plan of Newton-PCG's rigid-mode coarse space (dotmi_set_pcg_coarse; dotmi_coarse.hip / k_coarse.hip;
// DESIGN.md section 9): the coarse matrix A0 = Z^T H Z has one 6 x 6 block per pair of subdomains (s, t) that an H block couples,
//     A0_st = sum over the H blocks (i, j) with i in s and j in t of Z_si^T H_ij Z_tj,
// and A0_ts = A0_st^T, so every unordered pair is listed once (s <= t, diagonals included) with the H blocks of ITS order: the blocks
// (i, j) with i in s and j in t -- for s == t both (i, j) and (j, i).  One entry per (H block, s containing i, t containing j, s <= t);
// the lists ascend in the block's index in the global block-CSR, which fixes the summation order of the assembly.  Beside them the
// two vertex lists the per-iteration kernels walk: the subdomains of a vertex and the vertices of a subdomain, both ascending.
// No device call here (exported as dotmi_plan_coarse; tests/test_coarse_host.py).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

namespace dotmi {

struct CoarsePlan {
    int nV = 0, nParts = 0;
    std::vector<int> vsPtr, vsIdx;       // per vertex: its subdomains, ascending (CSR over nV)
    std::vector<int> svPtr, svIdx;       // per subdomain: its vertices, ascending (CSR over nParts)
    std::vector<int> pairS, pairT;       // the coupled pairs, s <= t, ordered by (s, t)
    std::vector<int> pairPtr, pairBlk;   // per pair: the H blocks of its sum (indices into adj_idx), ascending
};

// adjacency incl. self, ascending (build_adjacency); block k of the global block-CSR is entry k of adj_idx
inline void coarse_plan(int nV, int nT, const int *T, const int *epart, int nParts, const std::vector<int> &adj_ptr,
                        const std::vector<int> &adj_idx, CoarsePlan &P)
{
    P.nV = nV;
    P.nParts = nParts;
    // (vertex, subdomain) incidences: a subdomain holds the vertices of its elements (DOTTimeStepper.cpp:47-56)
    std::vector<std::vector<int>> vs(nV);
    for (int e = 0; e < nT; ++e)
        for (int a = 0; a < 4; ++a) vs[T[4 * e + a]].push_back(epart[e]);
    P.vsPtr.assign(nV + 1, 0);
    P.vsIdx.clear();
    std::vector<int> cnt(nParts, 0);
    for (int v = 0; v < nV; ++v) {
        std::sort(vs[v].begin(), vs[v].end());
        vs[v].erase(std::unique(vs[v].begin(), vs[v].end()), vs[v].end());
        for (int s : vs[v]) {
            P.vsIdx.push_back(s);
            ++cnt[s];
        }
        P.vsPtr[v + 1] = (int)P.vsIdx.size();
    }
    P.svPtr.assign(nParts + 1, 0);
    for (int s = 0; s < nParts; ++s) P.svPtr[s + 1] = P.svPtr[s] + cnt[s];
    P.svIdx.assign(P.svPtr[nParts], 0);
    {
        std::vector<int> cur(P.svPtr.begin(), P.svPtr.end() - 1);
        for (int v = 0; v < nV; ++v)
            for (int s : vs[v]) P.svIdx[cur[s]++] = v;
    }
    // entries per pair: first the counts over a dense pair table, then the fill in ascending block order
    std::vector<int> count((size_t)nParts * nParts, 0);
    for (int i = 0; i < nV; ++i)
        for (int k = adj_ptr[i]; k < adj_ptr[i + 1]; ++k)
            for (int s : vs[i])
                for (int t : vs[adj_idx[k]])
                    if (s <= t) ++count[(size_t)s * nParts + t];
    P.pairS.clear();
    P.pairT.clear();
    P.pairPtr.assign(1, 0);
    std::vector<int> at((size_t)nParts * nParts, -1);
    for (int s = 0; s < nParts; ++s)
        for (int t = s; t < nParts; ++t) {
            const int c = count[(size_t)s * nParts + t];
            if (c == 0 && s != t) continue;   // (a diagonal pair exists even for a subdomain without elements)
            at[(size_t)s * nParts + t] = P.pairPtr.back();
            P.pairS.push_back(s);
            P.pairT.push_back(t);
            P.pairPtr.push_back(P.pairPtr.back() + c);
        }
    P.pairBlk.assign(P.pairPtr.back(), 0);
    for (int i = 0; i < nV; ++i)
        for (int k = adj_ptr[i]; k < adj_ptr[i + 1]; ++k)
            for (int s : vs[i])
                for (int t : vs[adj_idx[k]])
                    if (s <= t) P.pairBlk[at[(size_t)s * nParts + t]++] = k;
}

// The lists of W = H Z for the balanced form of DOT's coarse term (dotmi_set_dot_coarse_mode, mode 2): W has a 3 x 6 block W[i, t] for every
// vertex i and subdomain t that an H block (i, j) with j in t couples,
//     W[i, t] = sum over the H blocks (i, j), j in t, of H_ij Z_tj.
// Per vertex the subdomains of its entries ascending, per entry its H blocks ascending (indices into adj_idx: the summation order
// of coarse_hz_kernel), and the transposed index: per subdomain its entries in ascending vertex, which c = W^T u walks.
// No device call here (exported as dotmi_plan_coarse_hz; tests/test_dot_coarse_balanced_host.py).
struct CoarseHzPlan {
    std::vector<int> hzPtr, hzSub;      // per vertex: the subdomains t of its entries (i, t), ascending (CSR over nV)
    std::vector<int> hzVert;            // per entry: its vertex i
    std::vector<int> hzBlkPtr, hzBlk;   // per entry: the H blocks (i, j), j in t, ascending (CSR over the entries)
    std::vector<int> hzTPtr, hzTEnt;    // per subdomain: its entries, ascending in the vertex (CSR over nParts)
};

// vsPtr / vsIdx: the subdomains of a vertex, ascending (CoarsePlan)
inline void coarse_hz_plan(int nV, int nParts, const std::vector<int> &vsPtr, const std::vector<int> &vsIdx, const std::vector<int> &adj_ptr,
                           const std::vector<int> &adj_idx, CoarseHzPlan &P)
{
    P.hzPtr.assign(nV + 1, 0);
    P.hzSub.clear();
    P.hzVert.clear();
    P.hzBlkPtr.assign(1, 0);
    P.hzBlk.clear();
    std::vector<std::pair<int, int>> tk;   // (subdomain, block) of one vertex
    for (int i = 0; i < nV; ++i) {
        tk.clear();
        for (int k = adj_ptr[i]; k < adj_ptr[i + 1]; ++k)
            for (int a = vsPtr[adj_idx[k]]; a < vsPtr[adj_idx[k] + 1]; ++a) tk.emplace_back(vsIdx[a], k);
        std::sort(tk.begin(), tk.end());
        for (size_t e = 0; e < tk.size(); ++e) {
            if (e == 0 || tk[e].first != tk[e - 1].first) {
                if (e != 0) P.hzBlkPtr.push_back((int)P.hzBlk.size());
                P.hzSub.push_back(tk[e].first);
                P.hzVert.push_back(i);
            }
            P.hzBlk.push_back(tk[e].second);
        }
        if (!tk.empty()) P.hzBlkPtr.push_back((int)P.hzBlk.size());
        P.hzPtr[i + 1] = (int)P.hzSub.size();
    }
    // the transposed index: a counting sort by subdomain keeps the entries' ascending vertex order
    P.hzTPtr.assign(nParts + 1, 0);
    for (int t : P.hzSub) ++P.hzTPtr[t + 1];
    for (int t = 0; t < nParts; ++t) P.hzTPtr[t + 1] += P.hzTPtr[t];
    P.hzTEnt.assign(P.hzSub.size(), 0);
    std::vector<int> cur(P.hzTPtr.begin(), P.hzTPtr.end() - 1);
    for (int e = 0; e < (int)P.hzSub.size(); ++e) P.hzTEnt[cur[P.hzSub[e]]++] = e;
}

}  // namespace dotmi
