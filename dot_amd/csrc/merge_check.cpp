// merge_check.cpp -- the three storage forms of the merges' sum (merge_sum.hpp: the CSR walk, the wave-interleaved walk, the gather
// from the subdomains' own sums) against the plain two-stage statement, bit for bit, on the CPU under the address / UB sanitizers
// (make merge_check; links nothing of HIP).  The plain statement:
//   1. psub[s][col] = the tiles of subdomain s that hold the column, added in tile order from 0.0
//   2. value of dof 3 v + d = the subdomains of v in vp order, psub[s][position of v in s + d] added from 0.0
// The lists come from build_merge_lists (block_plan.hpp), the function dotmi_create runs, on synthetic subdomains: five overlapping
// vertex ranges over 150 vertices plus a few vertices spread over three and four of them, every subdomain's vertices at shuffled padded
// positions, tiles with random column ranges behind a first one that holds every column.  Subdomain 0 has exactly MT_CH tiles that all hold
// every column, so a vertex it shares has the next subdomain's first -- complemented -- entry as the first entry of the second batch;
// subdomain 4 has one tile, so the vertices only it holds have one-entry lists.  main() asserts that each of these is there.  The lists
// are built twice per trial: with the rule forced to the walk (all three forms) and forced to split (no lists: the gather alone).
#include "block_plan.hpp"
#include "merge_sum.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace dotmi;

namespace {

constexpr int NV = 150, NPARTS = 5, NBMAX = 30, TRIALS = 20;

struct Input {
    std::vector<std::vector<int>> sets;
    RowPlacement rows;
    std::vector<std::vector<int2>> ranges;
    int nmax = 0;
    std::vector<double> ppart;
};

Input make_input(std::mt19937_64 &rng)
{
    Input in;
    in.sets.assign(NPARTS, {});
    for (int s = 0; s < NPARTS; ++s)
        for (int v = 25 * s; v < (s == NPARTS - 1 ? NV : 25 * s + 40); ++v) in.sets[s].push_back(v);
    // vertices in three and four subdomains (ranges 1 and 2 hold 60 and 61 already, ranges 0 and 1 hold 30)
    for (int s : {0, 4}) in.sets[s].push_back(60);
    in.sets[3].push_back(61);
    in.sets[2].push_back(30);
    size_t most = 0;
    for (auto &pv : in.sets) {
        std::sort(pv.begin(), pv.end());
        most = std::max(most, pv.size());
    }
    in.nmax = 64 * (int)((3 * most + 63) / 64);
    in.rows.partPos.assign(NPARTS, {});
    in.ranges.assign(NPARTS, {});
    for (int s = 0; s < NPARTS; ++s) {
        std::vector<int> slot(in.nmax / 3);
        for (size_t i = 0; i < slot.size(); ++i) slot[i] = 3 * (int)i;
        std::shuffle(slot.begin(), slot.end(), rng);
        in.rows.partPos[s].assign(slot.begin(), slot.begin() + in.sets[s].size());
        const int nb = s == 0 ? MT_CH : s == 4 ? 1 : 2 + (int)(rng() % (NBMAX - 1));
        in.ranges[s].push_back(make_int2(0, in.nmax));
        for (int b = 1; b < nb; ++b) {
            const int x = s == 0 ? 0 : (int)(rng() % in.nmax), y = s == 0 ? in.nmax : x + 1 + (int)(rng() % (in.nmax - x));
            in.ranges[s].push_back(make_int2(x, y));
        }
    }
    // mixed sign and magnitude: +-[0.1, 1) x 10^[-8, 8]
    std::uniform_real_distribution<double> mant(0.1, 1.0), expo(-8.0, 8.0);
    in.ppart.resize((size_t)NPARTS * NBMAX * in.nmax);
    for (double &p : in.ppart) p = ((rng() & 1) ? -1.0 : 1.0) * mant(rng) * std::pow(10.0, expo(rng));
    return in;
}

bool same_bits(double a, double b) { return !memcmp(&a, &b, sizeof(double)); }

}  // namespace

int main()
{
    static_assert(3 * NV % 64 != 0, "the last wave of the interleaved lists is a partial one");
    static_assert(NBMAX > MT_CH, "a subdomain of MT_CH tiles and longer lists beside it");
    std::mt19937_64 rng(20240611);
    long long sums = 0;
    for (int trial = 0; trial < TRIALS; ++trial) {
        const Input in = make_input(rng);
        const int nmax = in.nmax, n3 = 3 * NV;
        MergeLists W, S;   // the walk's lists; the rule forced to split
        build_merge_lists(NV, in.sets, 0, NPARTS, in.rows, nmax, NBMAX, in.ranges, 0, false, false, W);
        build_merge_lists(NV, in.sets, 0, NPARTS, in.rows, nmax, NBMAX, in.ranges, 1, false, false, S);
        if (!W.walk || W.mw.empty() || S.walk || !S.mp.empty() || !S.mw.empty() || S.vp_off != W.vp_off || S.vp_ptr != W.vp_ptr) {
            fprintf(stderr, "merge_check: build_merge_lists did not make the forms asked for\n");
            return 1;
        }
        // ---- the plain statement ----
        std::vector<double> psub((size_t)NPARTS * nmax, 0.0), ref(n3);
        for (int s = 0; s < NPARTS; ++s)
            for (int col = 0; col < nmax; ++col) {
                double a = 0.0;
                for (size_t b = 0; b < in.ranges[s].size(); ++b)
                    if (col >= in.ranges[s][b].x && col < in.ranges[s][b].y) a += in.ppart[((size_t)s * NBMAX + b) * nmax + col];
                psub[(size_t)s * nmax + col] = a;
            }
        for (int v = 0; v < NV; ++v)
            for (int d = 0; d < 3; ++d) {
                double z = 0.0;
                for (int k = W.vp_ptr[v]; k < W.vp_ptr[v + 1]; ++k) z += psub[W.vp_off[k] + d];
                ref[3 * v + d] = z;
            }
        // ---- what the inputs must contain ----
        bool three = false, boundary = false, one = false, ragged = false;
        for (int v = 0; v < NV; ++v) three |= W.vp_ptr[v + 1] - W.vp_ptr[v] >= 3;
        for (int k = 0; k < n3; ++k) {
            const int len = W.mp[k + 1] - W.mp[k];
            one |= len == 1;
            ragged |= len < W.mw[k >> 6].y;
            for (int q = MT_CH; q < len; q += MT_CH) boundary |= W.ment[W.mp[k] + q] < 0;
        }
        if (!three || !boundary || !one || !ragged) {
            fprintf(stderr, "merge_check: trial %d lacks a case: vertex in three subdomains %d, subdomain boundary on a batch's first entry %d, "
                            "one-entry list %d, wave of unequal lists %d\n", trial, three, boundary, one, ragged);
            return 1;
        }
        // ---- the three forms ----
        for (int k = 0; k < n3; ++k) {
            const int v = k / 3, d = k - 3 * v;
            const double csr = merge_sum_csr(W.mp[k], W.mp[k + 1], W.ment.data(), in.ppart.data(), 0.0);
            const double il = merge_sum_interleaved(k, W.mw.data(), W.il.data(), in.ppart.data(), 0.0);
            double g1[1] = {0.0};
            merge_sum_psub(S.vp_ptr[v], S.vp_ptr[v + 1], S.vp_off.data(), psub.data() + d, g1);
            double g3[3] = {0.0, 0.0, 0.0};
            merge_sum_psub(S.vp_ptr[v], S.vp_ptr[v + 1], S.vp_off.data(), psub.data(), g3);
            if (!same_bits(csr, ref[k]) || !same_bits(il, ref[k]) || !same_bits(g1[0], ref[k]) || !same_bits(g3[d], ref[k])) {
                fprintf(stderr, "merge_check: trial %d, dof %d: plain %.17g, CSR walk %.17g, interleaved walk %.17g, gather %.17g / %.17g\n",
                        trial, k, ref[k], csr, il, g1[0], g3[d]);
                return 1;
            }
            sums += 4;
        }
    }
    printf("merge_check: %lld sums over %d sets of lists, every one equal to the plain two-stage statement\n", sums, TRIALS);
    return 0;
}
