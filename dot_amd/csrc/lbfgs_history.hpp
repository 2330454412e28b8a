// lbfgs_history.hpp -- the L-BFGS bookkeeping of a time step on its m x m scalars, stated once for the host-driven loop
// (run_host_loop, dotmi_probe_direction) and for thread 0 of the device controller (k_loopctl.hpp): the history update after an
// accepted trial (DOTTimeStepper.cpp:474-494), the first half of the two-loop recursion (DOTTimeStepper.cpp:386-404), the free slot.
// Needs neither the HIP runtime nor the handle: history_check.cpp compiles it with the host compiler and compares the three
// functions bit for bit with plain indexed restatements.
// The form is the device's: every loop has a constant trip count and a guard, no array is indexed with a run-time value, so that
// after inlining everything the controller holds stays in registers (a run-time index sends the arrays to scratch, or through LDS
// in the dependent chain).  The host pays a few dozen predicated moves per iteration for it.
#pragma once

#if defined(__HIPCC__)
#define LBFGS_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define LBFGS_HD inline
#endif

namespace dotmi {

constexpr int HIST_MAX = 6;     // L-BFGS pairs kept (reference uses 5, DOTTimeStepper.cpp:45)

// History update of an accepted trial whose pair went to `newslot`.  ys_new = y.s and sg_new = s.g of the new pair; the three rows of
// HIST_MAX statistics against the stored pairs i (chronological): siy[i] = s_i.y_new, snyj[i] = s_new.y_i, sig[i] = s_i.g.
// In place: m, order, ys, b, sy over [0, m); entries at or beyond m are never read.  y.s <= 0: no pair is stored, b is refreshed.
// NO: the extent of `order` -- HIST_MAX + 1 in the handle and in DevLoop, HIST_MAX in the controller's registers.
template <int NO>
LBFGS_HD void lbfgs_push_pair(int hist, int newslot, double ys_new, double sg_new, const double *siy_in, const double *snyj_in,
                              const double *sig_in, int &m, int (&order)[NO], double (&ys)[HIST_MAX], double (&b)[HIST_MAX],
                              double (&sy)[HIST_MAX][HIST_MAX])
{
    constexpr int H = HIST_MAX;
    static_assert(NO >= H, "order holds every stored pair");
    double siy[H], snyj[H], sig[H];
#pragma unroll
    for (int i = 0; i < H; ++i) {
        siy[i] = siy_in[i];
        snyj[i] = snyj_in[i];
        sig[i] = sig_in[i];
    }
    if (ys_new > 0.0) {
        if (m == hist) {  // drop the oldest pair: everything moves down by one, the statistic rows too (they are read at [i] below)
#pragma unroll
            for (int i = 0; i + 1 < H; ++i) {
                order[i] = order[i + 1];
                ys[i] = ys[i + 1];
                siy[i] = siy[i + 1];
                snyj[i] = snyj[i + 1];
                sig[i] = sig[i + 1];
#pragma unroll
                for (int j = 0; j + 1 < H; ++j) sy[i][j] = sy[i + 1][j + 1];
            }
            m -= 1;
        }
#pragma unroll
        for (int i = 0; i < H; ++i)
            if (i < m) {
                // (a loop for each of the two stores: with both in one loop the compiler for gfx950 leaves sy in scratch memory)
#pragma unroll
                for (int j = 0; j < H; ++j)
                    if (j == m) sy[i][j] = siy[i];    // sy[i][m]
#pragma unroll
                for (int j = 0; j < H; ++j)
                    if (j == m) sy[j][i] = snyj[i];   // sy[m][i]
                b[i] = sig[i];
            }
#pragma unroll
        for (int i = 0; i < H; ++i)
            if (i == m) {
                order[i] = newslot;
                ys[i] = ys_new;
                sy[i][i] = ys_new;
                b[i] = sg_new;
            }
        m += 1;
    } else {
#pragma unroll
        for (int i = 0; i < H; ++i)
            if (i < m) b[i] = sig[i];
    }
}

// First half of the two-loop recursion: xi[i] = (-b[i] - sum_{j > i} xi[j] sy[i][j]) / ys[i] for i = m - 1 .. 0, zero from m on
LBFGS_HD void lbfgs_two_loop_xi(int m, const double (&b)[HIST_MAX], const double (&sy)[HIST_MAX][HIST_MAX],
                                const double (&ys)[HIST_MAX], double (&xi)[HIST_MAX])
{
    constexpr int H = HIST_MAX;
#pragma unroll
    for (int i = 0; i < H; ++i) xi[i] = 0.0;
#pragma unroll
    for (int i = H - 1; i >= 0; --i)
        if (i < m) {
            double sq = -b[i];
#pragma unroll
            for (int j = H - 1; j > i; --j)
                if (j < m) sq -= xi[j] * sy[i][j];
            xi[i] = sq / ys[i];
        }
}

// The smallest slot in [0, hist] that none of order[0 .. m) holds (hist + 1 slots, at most hist pairs: there is one; else 0)
template <int NO>
LBFGS_HD int lbfgs_free_slot(int hist, int m, const int (&order)[NO])
{
    static_assert(NO >= HIST_MAX && HIST_MAX < 31, "one bit per slot");
    unsigned used = 0;
#pragma unroll
    for (int i = 0; i < HIST_MAX; ++i)
        if (i < m) used |= 1u << order[i];
    const unsigned avail = ~used & ((2u << hist) - 1u);
    return avail ? __builtin_ctz(avail) : 0;
}

}  // namespace dotmi
