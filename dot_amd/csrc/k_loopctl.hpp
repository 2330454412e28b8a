// k_loopctl.hpp -- the loop controller: what the host loop of dotmi_step does between a trial and the next launch
// (line search Optimizer.cpp:806-833, history update DOTTimeStepper.cpp:474-494, stopping test Optimizer.cpp:317-330), on the
// device.  Included by k_backsolve.hip only, whose kernels run it: as a launch of its own (loop_control_kernel) or as workgroup 0
// of the back-solve launch (backsolve_ctl_kernel) -- 256 threads either way.  The partial sums are added in block order, the same
// order the host path uses, and the history update is the host's own statement (lbfgs_history.hpp), so both paths produce the
// same bits.
// The decision itself -- everything thread 0 does between the column sums and the write-back -- is loop_verdict<CTL> in
// loop_verdict.hpp, which the host compiler reads too (loopctl_check.cpp runs it on the CPU against a sequential line search).  What
// is here is the device's: the wide load and store of DevLoop through LDS, the (column, chunk) thread mapping of the sums, the SPEC
// partial loads, the two atomic stores of a verdict, the host notification.
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
#include "loop_verdict.hpp"

namespace dotmi {

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
            a0spec = ls_first_step(pg, pHp, ctl->alphaMin);
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
    if (t == 0) {
        double ea = 0.0, ei = 0.0;   // a paired slot: the full step's energy columns
        if constexpr (PAIR) {
            if (alpha_full > 0.0) {
#pragma unroll
                for (int c = 0; c < SUM_CHUNKS; ++c) {
                    ea += chunk2[0][c];
                    ei += chunk2[PAIR ? 1 : 0][c];
                }
            }
        }
        // the decision (loop_verdict.hpp); its verdict goes to memory at once, for the back-solve beside this workgroup
        loop_verdict<CTL>(C, R, init, alpha_in, alpha_full, ea, ei, a0spec, [&](bool stop, int slots, int verdict) {
            if (stop) __hip_atomic_store(&ctl->abortEpoch, slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ctl->holdVerdict, verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        });
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
