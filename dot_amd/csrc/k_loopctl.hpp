// k_loopctl.hpp -- the loop controller: what the host loop of dotmi_step does between a trial and the next launch
// (line search Optimizer.cpp:806-833, history update DOTTimeStepper.cpp:474-494, stopping test Optimizer.cpp:317-330), on the
// device.  Included by k_backsolve.hip only, whose kernels run it: as a launch of its own (loop_control_kernel) or as workgroup 0
// of the back-solve launch (backsolve_ctl_kernel) -- 256 threads either way.  The partial sums are added in block order, the same
// order the host path uses, and the history update is the host's own statement (lbfgs_history.hpp), so both paths produce the
// same bits.
//
// The forms (CTL_*, dotmi_internal.hpp) are a template parameter: the plain instantiation compiles the other forms' branches away.
// CTL_PAIR: the controller of a step with paired line-search trials (it understands paired slots: the full step's energy partials
// in partE2, alpha_dev[1] > 0 marks a paired slot).  CTL_SPEC: the controller of a step whose new-direction slots take the unit
// step speculatively (k_dirstep.hip): it sums the SpMV partials itself -- the element pass's prologue, the same additions -- and
// when alpha_0 = clamp(-p.g / p.Hp, alphaMin, 1) is not 1 the slot did not evaluate the reference's first trial: its back-solve is
// stopped and the next slot evaluates x + alpha_0 p as the first trial it is (phase 1, redo: nothing counted twice).
// CTL_VP: the controller of a step on vertex patches (k_elemvert.hip): the statistics come in one row per PATCH (nbE rows, like the
// energy partials) instead of NB_RED rows; summed in chunked_sum's order over that many rows.
// CTL_PAIR_VP: both -- a step with paired trials on vertex patches.
#pragma once
#include "k_device.hpp"

namespace dotmi {

// Chunk ch of chunked_sum() (dotmi_internal.hpp) over n rows of a column, row k at p[STRIDE k]: eight loads in flight, then their
// eight additions in row order -- the order of the host's sum, which is what makes host and device agree
template <int STRIDE>
__device__ __forceinline__ double ctl_chunk_sum(const double *__restrict__ p, int n, int ch)
{
    const int LE = (n + SUM_CHUNKS - 1) / SUM_CHUNKS;
    const int k1 = min(n, (ch + 1) * LE);
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

template <int CTL>
__device__ __forceinline__ void loop_control_body(DevLoop *__restrict__ ctl, const double *__restrict__ partE, int nbE,
                                  const double *__restrict__ partR, const double *__restrict__ alpha_dev,
                                  int *__restrict__ flags_host, int init, const double *__restrict__ partE2 = nullptr)
{
    constexpr bool PAIR = CTL == CTL_PAIR || CTL == CTL_PAIR_VP, SPEC = CTL == CTL_SPEC;
    constexpr bool VPROWS = CTL == CTL_VP || CTL == CTL_PAIR_VP;   // one row of statistics per patch (nbE rows)
    static_assert(sizeof(DevLoop) % 8 == 0, "DevLoop is copied as 8-byte words");
    static_assert(RED_K <= 32, "two passes of 16 columns");
    __shared__ double chunk[RED_K + 2][SUM_CHUNKS];
    __shared__ double R[RED_K + 2];
    __shared__ DevLoop C;  // the state is worked on in LDS: one wide load, one wide store
    const int t = threadIdx.x;
    constexpr int NW8 = (int)(sizeof(DevLoop) / 8);
    {
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(ctl);
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(&C);
        for (int i = t; i < NW8; i += 256) dst[i] = src[i];
    }
    const double alpha_in = *alpha_dev;
    // SPEC: the partials of p.g and p.Hp, requested with everything else (wave 0; summed below as elem_patch_body's prologue does)
    double pgv[NB_RED / 64], pHpv[NB_RED / 64];
    if constexpr (SPEC) {
        if (t < 64 && !init) {
            const double *__restrict__ sp = ctl->specPartials;
#pragma unroll
            for (int u = 0; u < NB_RED / 64; ++u) {
                pgv[u] = sp[(size_t)(t + 64 * u) * RED_K];
                pHpv[u] = sp[(size_t)(t + 64 * u) * RED_K + 1];
            }
        }
    }
    const double alpha_full = (PAIR && partE2 && !init) ? alpha_dev[1] : 0.0;   // > 0: a paired slot (elem_patch_kernel)
    __shared__ double chunk2[PAIR ? 2 : 1][SUM_CHUNKS];
    // chunked_sum() order (dotmi_internal.hpp), one thread per (column, chunk): every load of the kernel is in flight at
    // once and the dependent add chains are 16 long instead of NB_RED long.  The column index runs fastest over the
    // lanes, so a load instruction touches a few 168-byte partial rows instead of 64 different ones.
    {
        constexpr int LR = (NB_RED + SUM_CHUNKS - 1) / SUM_CHUNKS;
        static_assert(LR * SUM_CHUNKS == NB_RED, "chunks of equal length");
        constexpr int NPAIR = RED_K * SUM_CHUNKS;            // (statistic column, chunk) pairs
        static_assert(NPAIR + 2 * SUM_CHUNKS <= 512, "two passes of 256 threads");
        const int qa = t, qb = t + 256;
        const int colA = qa % RED_K, chA = qa / RED_K;
        const int colB = qb % RED_K, chB = qb / RED_K;
        const bool hasA = qa < NPAIR, hasB = qb < NPAIR;
        double va[LR], vb[LR];
        if constexpr (!VPROWS) {
            if (hasA) {
#pragma unroll
                for (int k = 0; k < LR; ++k) va[k] = partR[(size_t)(chA * LR + k) * RED_K + colA];
            }
            if (hasB) {
#pragma unroll
                for (int k = 0; k < LR; ++k) vb[k] = partR[(size_t)(chB * LR + k) * RED_K + colB];
            }
        }
        const int te = qb - NPAIR;  // the next 2 * SUM_CHUNKS slots: the two energy columns
        if (te >= 0 && te < 2 * SUM_CHUNKS) {
            const int c = te / SUM_CHUNKS, ch = te % SUM_CHUNKS;
            chunk[RED_K + c][ch] = ctl_chunk_sum<2>(partE + c, nbE, ch);
            // a paired slot: the same chunks of the full step's partials (same order: the same bits as a plain slot)
            if (PAIR && alpha_full > 0.0) chunk2[PAIR ? c : 0][ch] = ctl_chunk_sum<2>(partE2 + c, nbE, ch);
        }
        if constexpr (VPROWS) {   // nbE rows of statistics
            if (hasA) chunk[colA][chA] = ctl_chunk_sum<RED_K>(partR + colA, nbE, chA);
            if (hasB) chunk[colB][chB] = ctl_chunk_sum<RED_K>(partR + colB, nbE, chB);
        } else {
            if (hasA) {
                double a = 0.0;
#pragma unroll
                for (int k = 0; k < LR; ++k) a += va[k];
                chunk[colA][chA] = a;
            }
            if (hasB) {
                double b = 0.0;
#pragma unroll
                for (int k = 0; k < LR; ++k) b += vb[k];
                chunk[colB][chB] = b;
            }
        }
    }
    double a0spec = 1.0;   // SPEC: alpha_0 of the direction the slot computed (valid in thread 0)
    if constexpr (SPEC) {
        if (t < 64 && !init) {
            double pg = 0.0, pHp = 0.0;
#pragma unroll
            for (int u = 0; u < NB_RED / 64; ++u) {
                pg += pgv[u];
                pHp += pHpv[u];
            }
            pg = wave_sum(pg);
            pHp = wave_sum(pHp);
            a0spec = fmax(ctl->alphaMin, fmin(1.0, -pg / pHp));  // Optimizer.cpp:1085
        }
    }
    __syncthreads();
    if (C.status != 0) return;
    if (t < RED_K + 2) {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < SUM_CHUNKS; ++c) acc += chunk[t][c];
        R[t] = acc;
    }
    __syncthreads();
    if (t == 0 && init) {
        // evaluation at the start of the step (DOTTimeStepper.cpp:299): nothing to decide yet
        const double E = C.dtSq * R[RED_K] + R[RED_K + 1];
        C.evals++;
        C.E_cur = C.E0 = E;
        C.g2_cur = C.g2_0 = R[0];
    } else if (t == 0) {
        // The verdict on this slot's trial for the back-solve that may be running beside this workgroup, or waiting for it
        // (backsolve_ctl_kernel): holdVerdict = 2 slot + stop lets a held one start or leave; stop -- the trial is rejected, the slot
        // is redone, or the loop ends with this iterate -- also tells one that streams speculatively to stop (abortEpoch)
        auto publish_verdict = [&](bool stop) {
            if (stop) {
                C.abortEpoch = C.slots;
                __hip_atomic_store(&ctl->abortEpoch, C.slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            C.holdVerdict = 2 * C.slots + (stop ? 1 : 0);
            __hip_atomic_store(&ctl->holdVerdict, C.holdVerdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        // the forecast learns the outcome of a trial of its kind: the counter of the kind's current pattern, then the pattern
        auto forecast_update = [&](int kind, bool rejected) {
            int &ctr = C.predCtr[kind][C.predHist[kind] & 3];
            ctr = rejected ? min(3, ctr + 1) : max(0, ctr - 1);
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
                double ea = 0.0, ei = 0.0;
#pragma unroll
                for (int c = 0; c < SUM_CHUNKS; ++c) {
                    ea += chunk2[0][c];
                    ei += chunk2[PAIR ? 1 : 0][c];
                }
                const double EA = C.dtSq * ea + ei;
                C.pairSlots++;
                {
                    int &pc = C.pairCtr[pair_band(alpha_full)];
                    pc = (EA > C.E_cur) ? min(3, pc + 1) : max(0, pc - 1);
                }
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
            if (learns && alpha_full == 0.0) {
                int &pc = C.pairCtr[pair_band(a0)];
                pc = (E > C.E_cur && alpha > 0.0) ? min(3, pc + 1) : max(0, pc - 1);
            }
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
        } else if (E > C.E_cur && alpha > 0.0) {
            // back-tracking (c1 = 0, lower bound 0)
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
    }
    // forecast for the slot that follows: hold its back-solve if its kind's counter for the current pattern says "rejected"
    if (t == 0 && !init) {
        const int nk = C.phase == 0 ? 0 : 1;
        C.holdNext = (C.holdEnable && C.status == 0 && !((PAIR || SPEC) && C.redo) && C.predCtr[nk][C.predHist[nk] & 3] >= 2) ? 1 : 0;
    }
    __syncthreads();
    {
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(ctl);
        const unsigned long long *src = reinterpret_cast<const unsigned long long *>(&C);
        for (int i = t; i < NW8; i += 256) dst[i] = src[i];
    }
    // a store to host memory holds the kernel's end back by several microseconds: only near the expected
    // end of the loop, where the host needs the progress to stop enqueueing
    if (t == 0 && !init && (C.status != 0 || C.slots >= C.notifyFrom)) {
        __threadfence_system();
        flags_host[1] = C.slots;
        flags_host[0] = C.status;
    }
}

}  // namespace dotmi
