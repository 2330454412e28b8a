// history_check.cpp -- the shared L-BFGS bookkeeping (lbfgs_history.hpp: guarded loops of constant trip count, the form the device
// controller needs) against its plain statement with run-time indices, bit for bit, on the CPU under the address / UB sanitizers
// (make history_check; links nothing of HIP).  The plain statement below is what the host loop ran before the two were one.
// For every history length 1 .. HIST_MAX: 200 random sequences of 40 accepted trials, about one in five with y.s <= 0, so that the
// oldest pair is dropped many times at every length.  After every update m, order / ys / b / sy over [0, m), xi and the free slot
// are compared (entries at or beyond m are never read by either loop and may differ).  `order` in both extents the library uses:
// HIST_MAX + 1 (the handle) and HIST_MAX (the controller's register copy).
#include "lbfgs_history.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

using namespace dotmi;

namespace {

template <int NO>
struct History {
    int m = 0;
    int order[NO] = {0};
    double ys[HIST_MAX] = {0}, b[HIST_MAX] = {0}, sy[HIST_MAX][HIST_MAX] = {{0}};
};

// ---- the plain statement --------------------------------------------------------------------------------------------
void plain_push_pair(History<HIST_MAX + 1> &h, int hist, int slot, const double *R)
{
    const double ys_new = R[1], sg_new = R[2];
    const double *siy = R + 3, *snyj = R + 3 + HIST_MAX, *sig = R + 3 + 2 * HIST_MAX;
    if (ys_new <= 0.0) {
        for (int i = 0; i < h.m; ++i) h.b[i] = sig[i];
        return;
    }
    int m = h.m;
    int off = 0;
    if (m == hist) {  // drop the oldest pair
        off = 1;
        for (int i = 0; i + 1 < m; ++i) {
            h.order[i] = h.order[i + 1];
            h.ys[i] = h.ys[i + 1];
            for (int j = 0; j + 1 < m; ++j) h.sy[i][j] = h.sy[i + 1][j + 1];
        }
        m -= 1;
    }
    for (int i = 0; i < m; ++i) {
        h.sy[i][m] = siy[i + off];
        h.sy[m][i] = snyj[i + off];
        h.b[i] = sig[i + off];
    }
    h.order[m] = slot;
    h.ys[m] = ys_new;
    h.sy[m][m] = ys_new;
    h.b[m] = sg_new;
    h.m = m + 1;
}

void plain_two_loop_xi(int m, const double *b, const double (*sy)[HIST_MAX], const double *ys, double *xi)
{
    for (int i = 0; i < HIST_MAX; ++i) xi[i] = 0.0;
    for (int i = m - 1; i >= 0; --i) {
        double sq = -b[i];
        for (int j = m - 1; j > i; --j) sq -= xi[j] * sy[i][j];
        xi[i] = sq / ys[i];
    }
}

int plain_free_slot(const History<HIST_MAX + 1> &h, int hist)
{
    for (int s = 0; s <= hist; ++s) {
        bool used = false;
        for (int i = 0; i < h.m; ++i) used |= (h.order[i] == s);
        if (!used) return s;
    }
    return 0;
}

// ---- comparison ---------------------------------------------------------------------------------------------------------
long long g_updates = 0;

template <int NO>
bool same(const History<HIST_MAX + 1> &ref, const History<NO> &got, int hist, const char *what)
{
    const int m = ref.m;
    bool ok = got.m == m && !memcmp(got.order, ref.order, sizeof(int) * m) && !memcmp(got.ys, ref.ys, sizeof(double) * m) &&
              !memcmp(got.b, ref.b, sizeof(double) * m);
    for (int i = 0; ok && i < m; ++i) ok = !memcmp(got.sy[i], ref.sy[i], sizeof(double) * m);
    double xr[HIST_MAX], xg[HIST_MAX];
    plain_two_loop_xi(m, ref.b, ref.sy, ref.ys, xr);
    lbfgs_two_loop_xi(got.m, got.b, got.sy, got.ys, xg);
    ok = ok && !memcmp(xg, xr, sizeof(xr));
    ok = ok && lbfgs_free_slot(hist, got.m, got.order) == plain_free_slot(ref, hist);
    if (!ok) fprintf(stderr, "history_check: %s differs from the plain statement: hist %d, update %lld, m %d / %d\n", what, hist,
                     g_updates, got.m, m);
    return ok;
}

}  // namespace

int main()
{
    constexpr int RED_K = 3 * HIST_MAX + 3;   // |g|^2, y.s, s.g and the three rows (dotmi_internal.hpp)
    std::mt19937_64 rng(20240607);
    std::uniform_real_distribution<double> val(-1.0, 1.0);
    for (int hist = 1; hist <= HIST_MAX; ++hist)
        for (int seq = 0; seq < 200; ++seq) {
            History<HIST_MAX + 1> ref, wide;   // wide: the handle's extent of `order`
            History<HIST_MAX> narrow;          // the controller's
            for (int trial = 0; trial < 40; ++trial) {
                double R[RED_K];
                for (double &r : R) r = val(rng);
                R[1] = (rng() % 5 == 0) ? -std::abs(R[1]) : std::abs(R[1]) + 1e-3;   // y.s
                const int slot = plain_free_slot(ref, hist);
                plain_push_pair(ref, hist, slot, R);
                lbfgs_push_pair(hist, slot, R[1], R[2], R + 3, R + 3 + HIST_MAX, R + 3 + 2 * HIST_MAX, wide.m, wide.order, wide.ys,
                                wide.b, wide.sy);
                lbfgs_push_pair(hist, slot, R[1], R[2], R + 3, R + 3 + HIST_MAX, R + 3 + 2 * HIST_MAX, narrow.m, narrow.order,
                                narrow.ys, narrow.b, narrow.sy);
                ++g_updates;
                if (!same(ref, wide, hist, "order[HIST_MAX + 1]") || !same(ref, narrow, hist, "order[HIST_MAX]")) return 1;
            }
        }
    printf("history_check: %lld updates, every one equal to the plain statement\n", g_updates);
    return 0;
}
