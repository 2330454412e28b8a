// pd_plan.hpp -- the host-only plan of LBFGS-PD's scalar Laplacian solve (dotmi_pd.hip): the nested dissection of the whole vertex
// graph with one unknown per vertex, the row-block storage of its inverse factor and the work items of the apply.  Plain data in,
// plain data out: build_pd uploads it, dotmi_plan_pd (dotmi_plan.cpp) reports its sizes.
#pragma once
#include <algorithm>
#include <vector>

#include "dotmi_internal.hpp"

namespace dotmi {

struct PdPlan {
    std::vector<NdNode> nd;
    int nmax = 0;
    std::vector<int> pos, cvert;       // vertex -> padded position; padded position -> vertex (-1: padding)
    std::vector<RowTile> rt;           // per 64-row block
    size_t wTotal = 0;
    std::vector<PdItem> items;         // one-pass items, then the chunks of the two-pass blocks
    int nOne = 0, nLong = 0;
    long long ppartN = 0;
    long long readElems = 0;           // structural entries of X one application uses (each streamed once ...)
    long long rereadElems = 0;         // ... except in the two-pass blocks, whose rows are read a second time
};

// depth of the scalar dissection: split until the leaves hold ~1000 vertices (at least two levels)
inline int pd_levels(int nV)
{
    int levels = 2;
    for (int sz = nV; sz > 2000 && levels < 8; sz /= 2) ++levels;
    return levels;
}

inline void pd_plan(int nV, const std::vector<int> &adj_ptr, const std::vector<int> &adj_idx, const double *X, PdPlan &P)
{
    std::vector<std::vector<int>> sets(1);
    sets[0].resize(nV);
    for (int v = 0; v < nV; ++v) sets[0][v] = v;
    std::vector<std::vector<std::vector<int>>> region;
    P.nmax = nd_plan(sets, nV, adj_ptr, adj_idx, X, pd_levels(nV), ND_MIN_SPLIT, P.nd, region, 1);
    const int nmax = P.nmax, ntl = nmax / 64;
    P.pos.assign(nV, -1);
    P.cvert.assign(nmax, -1);
    std::vector<int> nodeC0(nmax, 0), rowStart(nmax, 0);   // first column of a row's tree node / of what the apply reads
    for (size_t k = 0; k < P.nd.size(); ++k) {
        const NdNode &N = P.nd[k];
        const auto &rv = region[k][0];
        const int ro = nd_region_first_row(N, (int)rv.size());
        for (size_t i = 0; i < rv.size(); ++i) {
            P.pos[rv[i]] = ro + (int)i;
            P.cvert[ro + i] = rv[i];
        }
        if (N.a < 0) {
            for (int r = N.off; r < N.off + N.size; ++r) {
                nodeC0[r] = N.off;
                rowStart[r] = std::max(N.off, ro & ~15);   // (a leaf is right-aligned: its padding columns are in front)
            }
        } else {
            for (int r = N.offS; r < N.offS + N.sizeS; ++r) nodeC0[r] = rowStart[r] = N.off;
        }
    }
    P.rt.assign(ntl, RowTile{-1, 0, 0});
    P.wTotal = 0;
    constexpr int CW = 256 * PD_KC;
    std::vector<PdItem> lng;
    for (int J = 0; J < ntl; ++J) {
        int lastLive = -1;
        for (int r = 64 * J; r < 64 * J + 64; ++r)
            if (P.cvert[r] >= 0) lastLive = r;
        if (lastLive < 0) continue;   // identity padding only: nothing stored, nothing read
        const int c0 = nodeC0[64 * J];
        P.rt[J] = RowTile{(long long)P.wTotal, 64 * (J + 1) - c0, c0};
        P.wTotal += (size_t)64 * P.rt[J].ld;
        const int cs = rowStart[64 * J], ce = lastLive + 1, L = ce - cs;
        const bool two = L > CW;
        for (int r = 64 * J; r <= lastLive; ++r)
            if (P.cvert[r] >= 0) {
                P.readElems += r - cs + 1;
                if (two) P.rereadElems += r - cs + 1;
            }
        if (!two) {
            P.items.push_back(PdItem{J, cs, ce, 1, 0, 0});
        } else {
            const int nch = (L + CW - 1) / CW, first = (int)lng.size();
            for (int ch = 0; ch < nch; ++ch) lng.push_back(PdItem{J, cs + ch * CW, std::min(ce, cs + (ch + 1) * CW), nch, first, 0});
        }
    }
    P.nOne = (int)P.items.size();
    P.nLong = (int)lng.size();
    P.items.insert(P.items.end(), lng.begin(), lng.end());
    P.ppartN = 0;
    for (PdItem &it : P.items) {
        it.pbase = P.ppartN;
        P.ppartN += 3ll * (it.ce - it.cs);
    }
}

}  // namespace dotmi
