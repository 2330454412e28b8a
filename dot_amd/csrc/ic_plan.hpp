// ic_plan.hpp -- host-only plan of LBFGS-HI's block incomplete Cholesky (DOTMI_FLAG_LBFGS_HI; dotmi_ic.hip / k_ic.hip): a
// multicolour ordering of the vertex graph and, in that ordering, the fixed lists the colour launches walk.  The factor has the
// block pattern of H itself (IC(0)): one 3 x 3 block L_ij per edge (i, j) with j earlier in the order, one lower-triangular L_ii
// per vertex.  Vertices of one colour share no edge, so a colour's rows depend on earlier colours only and one launch per colour
// is the only synchronisation.  Every list is in ascending order position, which fixes every summation order: the factor and
// its application are bit-identical run to run.  No device call here (exported as dotmi_plan_ic; tests/test_ic_host.py).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

namespace dotmi {

struct IcPlan {
    int nV = 0, nColours = 0;
    std::vector<int> colour, pos;   // per vertex: its colour, its position in the (colour, vertex id) order
    std::vector<int> vert;          // per position: the vertex
    std::vector<int> cstart;        // nColours + 1: the positions [cstart[c], cstart[c + 1]) of colour c
    // lower blocks, CSR over positions: block s of row p couples position p to the EARLIER position lidx[s] (ascending per row)
    std::vector<int> lptr, lidx;
    std::vector<int> lsrc, dsrc;    // the block of the global block-CSR behind lower block s / behind the diagonal of position p
    // per lower block s = (i, j): the products L_ik L_jk^T over the common lower neighbours k of i and j (k before j by
    // construction), ascending position of k: pa = the block (i, k) of row i, pb = the block (j, k) of row j
    std::vector<int> pptr, pa, pb;
    // per position p: the blocks L_kp of LATER rows k (the backward sweep gathers L_kp^T x_k), ascending position of k
    std::vector<int> uptr, ublk, uvert;   // ublk: the lower block; uvert: the VERTEX of row k
};

// adjacency incl. self, ascending (build_adjacency); block k of the global block-CSR is entry k of adj_idx
inline void ic_plan(int nV, const std::vector<int> &adj_ptr, const std::vector<int> &adj_idx, IcPlan &P)
{
    P.nV = nV;
    // greedy colouring in ascending vertex id: the smallest colour no neighbour holds (deterministic, seedless)
    P.colour.assign(nV, -1);
    P.nColours = 0;
    std::vector<int> seen;   // seen[c] == v: a neighbour of v holds colour c
    for (int v = 0; v < nV; ++v) {
        for (int k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) {
            const int c = P.colour[adj_idx[k]];
            if (c >= 0 && adj_idx[k] != v) seen[c] = v;
        }
        int c = 0;
        while (c < P.nColours && seen[c] == v) ++c;
        if (c == P.nColours) {
            ++P.nColours;
            seen.push_back(-1);
        }
        P.colour[v] = c;
    }
    // order by (colour, vertex id)
    P.cstart.assign(P.nColours + 1, 0);
    for (int v = 0; v < nV; ++v) P.cstart[P.colour[v] + 1]++;
    for (int c = 0; c < P.nColours; ++c) P.cstart[c + 1] += P.cstart[c];
    P.pos.assign(nV, 0);
    P.vert.assign(nV, 0);
    {
        std::vector<int> cur(P.cstart.begin(), P.cstart.end() - 1);
        for (int v = 0; v < nV; ++v) {
            P.pos[v] = cur[P.colour[v]]++;
            P.vert[P.pos[v]] = v;
        }
    }
    // lower neighbours per position, ascending position
    P.lptr.assign(nV + 1, 0);
    P.lidx.clear();
    P.lsrc.clear();
    P.dsrc.assign(nV, -1);
    std::vector<std::pair<int, int>> row;
    for (int p = 0; p < nV; ++p) {
        const int v = P.vert[p];
        row.clear();
        for (int k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) {
            const int u = adj_idx[k];
            if (u == v) P.dsrc[p] = k;
            else if (P.pos[u] < p) row.push_back({P.pos[u], k});
        }
        std::sort(row.begin(), row.end());
        for (const auto &e : row) {
            P.lidx.push_back(e.first);
            P.lsrc.push_back(e.second);
        }
        P.lptr[p + 1] = (int)P.lidx.size();
    }
    const int nL = (int)P.lidx.size();
    // products: both rows ascend, so one merge per block; row i only up to the block itself (k before j)
    P.pptr.assign(nL + 1, 0);
    P.pa.clear();
    P.pb.clear();
    for (int i = 0; i < nV; ++i)
        for (int s = P.lptr[i]; s < P.lptr[i + 1]; ++s) {
            const int j = P.lidx[s];
            int a = P.lptr[i], b = P.lptr[j];
            while (a < s && b < P.lptr[j + 1]) {
                if (P.lidx[a] < P.lidx[b]) ++a;
                else if (P.lidx[a] > P.lidx[b]) ++b;
                else {
                    P.pa.push_back(a++);
                    P.pb.push_back(b++);
                }
            }
            P.pptr[s + 1] = (int)P.pa.size();
        }
    // upper entries: rows visited in ascending position, so every list ascends
    P.uptr.assign(nV + 1, 0);
    for (int s = 0; s < nL; ++s) P.uptr[P.lidx[s] + 1]++;
    for (int p = 0; p < nV; ++p) P.uptr[p + 1] += P.uptr[p];
    P.ublk.assign(nL, 0);
    P.uvert.assign(nL, 0);
    {
        std::vector<int> cur(P.uptr.begin(), P.uptr.end() - 1);
        for (int i = 0; i < nV; ++i)
            for (int s = P.lptr[i]; s < P.lptr[i + 1]; ++s) {
                const int at = cur[P.lidx[s]]++;
                P.ublk[at] = s;
                P.uvert[at] = P.vert[i];
            }
    }
}

}  // namespace dotmi
