// loop_verdict.hpp -- the line search's policy and the loop controller's decision, stated once in a form the host compiler reads too
// (LBFGS_HD, lbfgs_history.hpp; of HIP only the types dotmi_internal.hpp needs):
//   * ls_first_step      alpha_0 of a new direction (Optimizer.cpp:1085): step_forward_kernel, the two element kernels, the controller
//   * ls_rejects         the back-tracking test (Optimizer.cpp:806-833; c1 = 0, lower bound 0): the controller and backtrack()
//   * ctl_chunk_sum      a chunk of chunked_sum() as the controller's threads add it
//   * loop_verdict<CTL>  what one thread of the controller (k_loopctl.hpp) does with the summed columns of a slot: judge the trial,
//                        halve or accept, update the history, stop at the tolerance, the cap or a collapsed step, publish the verdict
//                        for the back-solve beside it, learn the hold forecast and the pairing rule
//   * loop_stopped_launches  the back-solves a finished step's controller told to stop, from the harvested counters: fill_step_stats
// loopctl_check.cpp drives loop_verdict slot by slot on the CPU, in all five forms, against a sequential restatement of the
// reference's loop, bit for bit, under the address / UB sanitizers (make loopctl_check; links nothing of HIP).
#pragma once
#include "dotmi_internal.hpp"
#include <math.h>

namespace dotmi {

LBFGS_HD double ls_first_step(double pg, double pHp, double alphaMin) { return fmax(alphaMin, fmin(1.0, -pg / pHp)); }

LBFGS_HD bool ls_rejects(double E, double E_cur, double alpha) { return E > E_cur && alpha > 0.0; }

// a saturating counter (0 .. 3) one step up or down
LBFGS_HD void ctr_learn(int &ctr, bool up) { ctr = up ? (ctr < 3 ? ctr + 1 : 3) : (ctr > 0 ? ctr - 1 : 0); }

// Chunk ch of chunked_sum() (dotmi_internal.hpp) over n rows of a column, row k at p[STRIDE k]: eight loads in flight, then their
// eight additions in row order -- the order of the host's sum, which is what makes host and device agree
template <int STRIDE>
LBFGS_HD double ctl_chunk_sum(const double *__restrict__ p, int n, int ch)
{
    const int LE = (n + SUM_CHUNKS - 1) / SUM_CHUNKS;
    const int k1 = n < (ch + 1) * LE ? n : (ch + 1) * LE;
    double s = 0.0;
    int k = ch * LE;
    for (; k + 8 <= k1; k += 8) {
        double v8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v8[u] = p[(size_t)(k + u) * STRIDE];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v8[u];
    }
    for (; k < k1; ++k) s += p[(size_t)k * STRIDE];
    return s;
}

// The controller's decision on one slot.  C: the loop state (the device's copy in LDS); R: the slot's summed columns -- RED_K statistics
// (|g|^2, y.s, s.g, the three rows of lbfgs_push_pair), then the elastic and the inertia energy.  init: the evaluation at the start of
// the step, nothing to decide.  alpha_in: the step the slot evaluated.  alpha_full > 0 (PAIR): a paired slot -- alpha_in is the half
// step, ea / ei the energy columns of the full step alpha_full.  a0spec (SPEC): alpha_0 of the direction the slot computed beside its
// unit step.  publish(stop, slots, holdVerdict): the two values a back-solve that runs beside the controller, or waits for it, reads
// (DevLoop::abortEpoch when stop, DevLoop::holdVerdict) -- the device stores them to memory at once, long before C is written back.
template <int CTL, class Publish>
LBFGS_HD void loop_verdict(DevLoop &C, const double *R, int init, double alpha_in, double alpha_full, double ea, double ei,
                           double a0spec, Publish publish)
{
    constexpr bool PAIR = CTL == CTL_PAIR || CTL == CTL_PAIR_VP, SPEC = CTL == CTL_SPEC;
    if (init) {
        // evaluation at the start of the step (DOTTimeStepper.cpp:299): nothing to decide yet
        const double E = C.dtSq * R[RED_K] + R[RED_K + 1];
        C.evals++;
        C.E_cur = C.E0 = E;
        C.g2_cur = C.g2_0 = R[0];
        return;
    }
    // The verdict on this slot's trial for the back-solve that may be running beside this workgroup, or waiting for it
    // (backsolve_ctl_kernel): holdVerdict = 2 slot + stop lets a held one start or leave; stop -- the trial is rejected, the slot
    // is redone, or the loop ends with this iterate -- also tells one that streams speculatively to stop (abortEpoch)
    auto publish_verdict = [&](bool stop) {
        if (stop) C.abortEpoch = C.slots;
        C.holdVerdict = 2 * C.slots + (stop ? 1 : 0);
        publish(stop, C.slots, C.holdVerdict);
    };
    // the forecast learns the outcome of a trial of its kind: the counter of the kind's current pattern, then the pattern
    auto forecast_update = [&](int kind, bool rejected) {
        ctr_learn(C.predCtr[kind][C.predHist[kind] & 3], rejected);
        C.predHist[kind] = ((C.predHist[kind] << 1) | (rejected ? 1 : 0)) & 3;
    };
    // the slot in the step's records; a0: the step estimate of its direction, counted when the slot is the direction's first
    // (the gate of the next step's speculation: how often the estimate is the unit step).  Returns the kind of its trial:
    // 0 first trial of an iteration (a redone slot is one), 1 retry after a halving
    auto account_slot = [&](double a0) {
        if (C.slots < C.kindCap) C.slot_kind[C.slots] = C.phase == 0 ? 1 : 2;
        C.slots++;
        if (C.phase == 0) {
            C.firstTrials++;
            C.unitFirst += a0 == 1.0 ? 1 : 0;
        }
        return (C.phase == 0 || ((PAIR || SPEC) && C.redo)) ? 0 : 1;
    };
    double alpha = alpha_in;
    const double E = C.dtSq * R[RED_K] + R[RED_K + 1];
    int kind = 0;
    bool decided = false;
    if constexpr (PAIR) {
        // what a first trial with alpha_0 < 1 teaches the pairing rule (a redone trial has taught it already)
        const double a0 = alpha_full > 0.0 ? alpha_full : alpha_in;
        const bool learns = C.phase == 0 && a0 < 1.0;
        kind = account_slot(a0);
        C.redo = 0;
        if (alpha_full > 0.0) {
            // Paired slot: the energy of the FULL step first, as the reference's line search would see it
            const double EA = C.dtSq * ea + ei;
            C.pairSlots++;
            ctr_learn(C.pairCtr[pair_band(alpha_full)], EA > C.E_cur);
            if (!(EA > C.E_cur)) {
                // the full step is acceptable: the slot's gradient belongs to the half step and is of no use.  The next slot
                // evaluates the full step as a plain trial (its energy is counted there); nothing else has happened
                C.pairRedo++;
                publish_verdict(true);
                C.phase = 1;
                C.alpha = alpha_full;
                C.redo = 1;
                decided = true;
            } else {
                // rejected: one halving; the trial in front of the controller is the retry with the half step
                C.evals++;
                C.halvings++;
                forecast_update(kind, true);
                kind = 1;
            }
        }
        if (!decided) C.evals++;
        C.heldSlots += (C.holdNext || alpha_full > 0.0) ? 1 : 0;
        if (learns && alpha_full == 0.0) ctr_learn(C.pairCtr[pair_band(a0)], ls_rejects(E, C.E_cur, alpha));
    } else if constexpr (SPEC) {
        kind = account_slot(a0spec);
        C.redo = 0;
        if (C.phase == 0) {
            // the slot computed a new direction and evaluated x + 1 p beside it
            C.specSlots++;
            if (a0spec != 1.0) {
                // the estimate lies inside (alphaMin, 1): the unit step is not the line search's first trial.  Nothing has
                // happened yet: the slot's back-solve stops, the next slot evaluates x + alpha_0 p (its energy is counted there)
                C.specRedo++;
                publish_verdict(true);
                C.phase = 1;
                C.alpha = a0spec;
                C.redo = 1;
                decided = true;
            }
        }
        if (!decided) C.evals++;
        C.heldSlots += C.holdNext;
    } else {
        C.evals++;
        kind = account_slot(alpha_in);
        C.heldSlots += C.holdNext;
    }
    if (decided) {
    } else if (ls_rejects(E, C.E_cur, alpha)) {
        // back-tracking
        publish_verdict(true);
        forecast_update(kind, true);
        C.heldRejected += (C.holdNext || alpha_full > 0.0) ? 1 : 0;
        alpha /= 2.0;
        C.halvings++;
        if (alpha == 0.0) {
            // the step length underflowed: the reference stops at the last trial point (Optimizer.cpp:819-861)
            C.status = 3;
            double *tmp = C.x_cur;
            C.x_cur = C.x_trial;
            C.x_trial = tmp;
            C.E_cur = E;
        } else {
            C.phase = 1;
            C.alpha = alpha;
        }
    } else {
        double *tmp = C.x_cur;
        C.x_cur = C.x_trial;
        C.x_trial = tmp;
        tmp = C.g_cur;
        C.g_cur = C.g_trial;
        C.g_trial = tmp;
        C.E_cur = E;
        const double g2 = R[0];
        C.g2_cur = g2;
        // when the loop ends with this iterate the back-solve for the next direction may stop -- said before the history
        // update below; else a held one may start now
        publish_verdict(C.iter + 1 >= C.iterCap || !(g2 > C.tol));
        forecast_update(kind, false);
        // The history in registers: lbfgs_history.hpp indexes nothing dynamically, so no LDS round trip sits in the
        // dependent chain of the update and the two-loop
        constexpr int H = HIST_MAX;
        double ys[H], b[H], sy[H][H], xi[H];
        int order[H];
#pragma unroll
        for (int i = 0; i < H; ++i) {
            ys[i] = C.L.ys[i];
            b[i] = C.b[i];
            order[i] = C.order[i];
            xi[i] = 0.0;
#pragma unroll
            for (int jj = 0; jj < H; ++jj) sy[i][jj] = C.L.sy[i][jj];
        }
        int m = C.L.m;
        const int hist = C.hist;
        C.pairNew = R[1] > 0.0 ? 1 : 0;
        lbfgs_push_pair(hist, C.slot, R[1], R[2], R + 3, R + 3 + H, R + 3 + 2 * H, m, order, ys, b, sy);
        if (C.iter < C.logCap) {
            C.log_alpha[C.iter] = alpha;
            C.log_E[C.iter] = E;
            C.log_g2[C.iter] = g2;
        }
        C.iter++;
        int fs = C.slot;
        if (C.iter >= C.iterCap) C.status = 2;
        else if (!(g2 > C.tol)) C.status = 1;
        if (C.status == 0) {
            // next direction: first half of the two-loop, free slot
            lbfgs_two_loop_xi(m, b, sy, ys, xi);
            fs = lbfgs_free_slot(hist, m, order);
            C.phase = 0;
        }
        // back to the shared copy (stores only; the operand views take their pointers from the slot table)
        C.L.m = m;
        C.slot = fs;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            C.L.ys[i] = ys[i];
            C.b[i] = b[i];
            C.order[i] = order[i];
            C.X.xi[i] = xi[i];
#pragma unroll
            for (int jj = 0; jj < H; ++jj) C.L.sy[i][jj] = sy[i][jj];
            if (i < m) {
                C.L.s[i] = C.S[order[i]];
                C.L.y[i] = C.Y[order[i]];
            }
        }
        devloop_resolve(C);   // (S[slot], MY[order[i]], HS[order[i]]: the kernels of the next slot read them resolved)
    }
    // forecast for the slot that follows: hold its back-solve if its kind's counter for the current pattern says "rejected"
    const int nk = C.phase == 0 ? 0 : 1;
    C.holdNext = (C.holdEnable && C.status == 0 && !((PAIR || SPEC) && C.redo) && C.predCtr[nk][C.predHist[nk] & 3] >= 2) ? 1 : 0;
}

// The back-solve launches a finished step's controller told to stop (dotmi_step_stats::backsolve_stopped), from the counters it
// leaves: every halving stops one and so does the accept that ends the loop; a paired slot whose full step was rejected takes a
// halving without a stopped launch (pairSlots - pairRedo of them), a redone slot -- paired or speculative -- stops one without a
// halving.  Equal to the stop verdicts loop_verdict published, except in a step whose line search collapsed (status 3): there the
// halving that underflows is also the step's end -- one verdict, counted twice here.  (loopctl_check.cpp asserts both.)
inline int loop_stopped_launches(long long halvings, int pairSlots, int pairRedo, int specRedo)
{
    return (int)(halvings + 1) + 2 * pairRedo - pairSlots + specRedo;
}

}  // namespace dotmi
