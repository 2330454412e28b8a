// dotmi_pcg.hip -- Newton-PCG: a linear solve with the global projected Hessian, H u = b, by conjugate gradients preconditioned with
// the symmetric scaling of DOT's block solve (kernels and recurrences: k_pcg.hip).  It costs the subdomain factorisation the handle
// already has plus one streaming block-solve application per iteration, so it scales like a DOT step where the reference's Newton
// (one subdomain, a factor of the whole mesh per iteration) does not.  dotmi_solve_hessian exposes the solve on every handle that
// has both H and the block solve; DOTMI_FLAG_NEWTON_PCG puts it into run_newton_loop (dotmi_loop.hip) in place of the single
// application, DOTMI_FLAG_NEWTON_PCG_DIST does so on sharded subdomains (pcg_iteration below has the collectives; DESIGN.md sections
// 6 and 9).  The reference has no counterpart (its Newton is Optimizer::solve_oneStep on CHOLMOD, Optimizer.cpp:703-749).
#include "dotmi_handle.hpp"

namespace dotmi {

// isd[v] = 1 / sqrt(dup[v]), at create: the partition fixes dup (dotmi_refix changes the fixed set, not the subdomains)
int pcg_build_scaling(dotmi_handle *h)
{
    std::vector<double> isd((size_t)h->nV);
    for (int v = 0; v < h->nV; ++v) isd[v] = 1.0 / std::sqrt((double)std::max(h->dup[v], 1));
    return upload(h, &h->pcg.isd, isd);
}

// the records, the partial arrays and the five vectors, at the first solve; kept
static int pcg_alloc(dotmi_handle *h)
{
    DevPcg &C = h->pcg;
    if (C.rec) return 0;
    double *blk = nullptr;
    if (int rc = dalloc(h, &blk, (size_t)PCG_READBACK)) return rc;
    double **parts[] = {&C.partAT, &C.partA, &C.partB};
    const size_t cnt[] = {(size_t)2 * NB_RED, (size_t)NB_RED * RED_K, (size_t)NB_RED * RED_K};
    for (int i = 0; i < 3; ++i)
        if (int rc = dalloc(h, parts[i], cnt[i])) return rc;
    double **vecs[] = {&C.r, &C.d, &C.Hd, &C.w, &C.s};
    for (double **pp : vecs)
        if (int rc = dalloc(h, pp, (size_t)h->n)) return rc;
    if (h->shardHess) {   // the packet [s | gamma | delta] of the sharded rows' second collective
        if (int rc = dalloc(h, &C.pkt, (size_t)h->n + 2)) return rc;
        HIPCHECK(h, hipMemsetAsync(C.pkt, 0, sizeof(double) * ((size_t)h->n + 2), h->st));
    }
    HIPCHECK(h, hipHostMalloc((void **)&h->h_pcg, sizeof(double) * PCG_READBACK));
    HIPCHECK(h, hipMemsetAsync(blk, 0, sizeof(double) * PCG_READBACK, h->st));
    C.partBT = blk + 2 * (sizeof(PcgRec) / sizeof(double));
    C.rec = (PcgRec *)blk;
    return 0;
}

// CG iteration k.  One rank: four launches.  Sharded subdomains (h->dist): the block solves and the merge run over the rank's own
// subdomains and leave its share of zsum = S q in h->z; one all-reduce of n doubles makes zsum whole, and with a replicated Hessian
// the two kernels then run unchanged and redundantly on replicated vectors.  With sharded Hessian rows a rank multiplies its rows
// [v0, v1) only: pcg_spmv_rows_kernel leaves s on them (zeros elsewhere) in the packet [s (n) | gamma | delta], reduce_rows_kernel
// puts the rank's two scalars into its tail (as reduce_step_dots does), a second all-reduce of n + 2 doubles sums it and
// pcg_update_kernel<true> reads s and the scalars from it.  gamma, delta, |r|^2, the verdict and u are functions of all-reduced data
// only: bit-identical on every rank.  The collectives are issued whatever the record says -- a gated kernel returns at once and the
// payload is scratch -- so every rank issues the same sequence (the rule of the DOT slots, dotmi_devloop.hip).
static int pcg_iteration(dotmi_handle *h, bool coarse, int k, double rel_tol)
{
    const DevPcg &C = h->pcg;
    const Bracket br = backsolve_bracket(h);
    if (coarse) coarse_restrict_solve(h, C.r);                          // y = A0^-1 Z^T r (needs nothing of the block solve)
    launch_gemv(h->P, h->q, h->st, nullptr, br.ev0, br.ev1);           // the block solves of q = r (.) isd
    launch_merge(h->M, h->P, NO_HISTORY, {.z = h->z}, h->st);           // zsum = S q: no division, no dots
    if (coarse) coarse_prolong(h, h->z);                                // zsum += (Z y) / isd: w = M_sym r + Z y
    if (h->dist)
        if (int rc = allreduce_sum(h, h->z, (size_t)h->n)) return rc;
    if (!h->shardHess) {
        launch_pcg_spmv(h->M, C, h->Hval, h->z, k, h->st);
        launch_pcg_update(C, h->n, h->p, h->q, k, rel_tol, h->st);
        return 0;
    }
    launch_pcg_spmv_rows(h->M, C, h->Hval, h->z, h->v0, h->v1, k, h->st);
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(64), 0, h->st, C.partA, NB_RED, RED_K, 2, 0.0, 0.0, 0, C.pkt + h->n);
    if (int rc = allreduce_sum(h, C.pkt, (size_t)h->n + 2)) return rc;
    launch_pcg_update_packet(C, h->n, h->p, h->q, k, rel_tol, h->st);
    return 0;
}

// world > 1, after a batch: every rank takes the record's (state, iter, rr, bb) and the batch's last |r|^2 from rank 0 and the ranks
// check that they had the same state and iteration count -- one collective of 9 doubles: rank 0's five values (zeros from the
// others: a broadcast), every rank's (state, iter) and their squares.  The ranks agree exactly when the variance
// vanishes, world * sum(v^2) == (sum v)^2 (small integers, exact in FP64): the test of enqueue_batches (dotmi_devloop.hip), taken on
// reduced data only, so ranks that disagree fail together instead of one of them waiting in the next all-reduce.
static int pcg_agree(dotmi_handle *h, int *state, int *iter, double *rr, double *bb, double *rrLast)
{
    if (h->world <= 1) return 0;
    const double mine[2] = {(double)*state, (double)*iter};
    double red[9] = {0.0, 0.0, 0.0, 0.0, 0.0, mine[0], mine[1], mine[0] * mine[0], mine[1] * mine[1]};
    if (h->rank == 0) {
        red[0] = mine[0];
        red[1] = mine[1];
        red[2] = *rr;
        red[3] = *bb;
        red[4] = *rrLast;
    }
    HIPCHECK(h, hipMemcpyAsync(h->ctrlDev, red, sizeof(red), hipMemcpyHostToDevice, h->st));
    if (int rc = allreduce_sum(h, h->ctrlDev, 9)) return rc;
    HIPCHECK(h, hipMemcpyAsync(red, h->ctrlDev, sizeof(red), hipMemcpyDeviceToHost, h->st));
    HIPCHECK(h, hipStreamSynchronize(h->st));
    const double w = (double)h->world;
    if (w * red[7] != red[5] * red[5] || w * red[8] != red[6] * red[6]) {
        h->err = "the ranks left a batch of PCG iterations in different states (this rank: state " + std::to_string(*state) + " after " +
                 std::to_string(*iter) + " iterations; sum over " + std::to_string(h->world) + " ranks: " +
                 std::to_string((long long)red[5]) + " / " + std::to_string((long long)red[6]) + ")";
        h->poisoned = true;
        return DOTMI_E_DEVICE;
    }
    *state = (int)red[0];
    *iter = (int)red[1];
    *rr = red[2];
    *bb = red[3];
    *rrLast = red[4];
    return 0;
}

// H u = b from u = 0 with the handle's current Hval and subdomain factors; b on the device (not q, z or p); the iterate is left in
// h->p.  The host enqueues check_every iterations, then reads the two records and the |r|^2 partials once: the device has decided
// convergence and breakdown for every iteration but the batch's last, whose |r|^2 the host sums in the same order.  An iteration
// enqueued behind the deciding one finds the ended record and leaves u alone; its block solve and merge -- the existing launches,
// unchanged -- run on a right-hand side nobody reads.
// Sharded subdomains: b, like every vector of the recurrences, is replicated; pcg_iteration has the collectives of an iteration and
// pcg_agree what the ranks exchange after a batch.
// returns 0 converged, 2 cap or breakdown (u is the last iterate: every CG iterate from zero is a descent direction), < 0 error
int pcg_solve(dotmi_handle *h, const double *b, double rel_tol, int max_iter, int check_every, int *iters, double *rel_res)
{
    if (int rc = pcg_alloc(h)) return rc;
    if (int rc = coarse_refresh(h)) return rc;   // (dotmi_set_pcg_coarse; nothing unless the mode is on and H has been refreshed)
    const bool coarse = h->coarse.mode != 0 && h->coarse.active;
    const DevPcg &C = h->pcg;
    const int n = h->n;
    launch_pcg_init(C, n, b, h->p, h->q, h->st);
    int k = 0, state = PCG_RUNNING, done = 0;
    double rr = 0.0, bb = 0.0;
    while (state == PCG_RUNNING) {
        const int nb = std::min(check_every, max_iter - k);
        for (int j = 0; j < nb; ++j) {
            ++k;
            if (int rc = pcg_iteration(h, coarse, k, rel_tol)) return rc;
        }
        HIPCHECK(h, hipMemcpyAsync(h->h_pcg, C.rec, sizeof(double) * PCG_READBACK, hipMemcpyDeviceToHost, h->st));
        HIPCHECK(h, hipStreamSynchronize(h->st));
        PcgRec rec;
        memcpy(&rec, (const char *)h->h_pcg + sizeof(PcgRec) * (k & 1), sizeof(rec));
        state = rec.state;
        done = rec.iter;
        bb = rec.bb;
        // iteration k's |r|^2 is in the partials (if it ran, the device would decide on it in iteration k + 1's prologue)
        const double *col = h->h_pcg + 2 * (sizeof(PcgRec) / sizeof(double)) + (size_t)(k & 1) * NB_RED;
        double rrLast = chunked_sum(NB_RED, [&](int i) { return col[i]; });
        if (int rc = pcg_agree(h, &state, &done, &rec.rr, &bb, &rrLast)) return rc;   // (world > 1: rank 0's, or all fail together)
        if (state != PCG_RUNNING) {
            rr = rec.rr;
            break;
        }
        rr = rrLast;
        if (rr <= rel_tol * rel_tol * bb) state = PCG_CONVERGED;
        else if (k >= max_iter) break;
    }
    HIPCHECK(h, hipGetLastError());
    h->pcgSolves++;
    h->pcgItersTotal += done;
    h->pcgLastIters = done;
    h->pcgLastRes = bb > 0.0 ? std::sqrt(rr / bb) : 0.0;
    if (iters) *iters = done;
    if (rel_res) *rel_res = h->pcgLastRes;
    return state == PCG_CONVERGED ? 0 : 2;
}

const char *pcg_refusal(const dotmi_handle *h)
{
    return h->pd      ? "an LBFGS-PD handle has no Hessian block solve"
           : h->hi    ? "an LBFGS-HI handle has no Hessian block solve"
           : h->gsdd  ? "a GSDD handle solves one subdomain at a time"
           // (owner exchange: its vectors are not replicated, and its refresh leaves the slice [v0, v1) of the SpMV unassembled)
           : h->owner ? "not on a handle with DOTMI_FLAG_OWNER_EXCHANGE (its vectors are valid on a rank's own vertices only)"
                      : nullptr;
}

static bool pcg_settings_ok(double rel_tol, int max_iter) { return std::isfinite(rel_tol) && rel_tol > 0.0 && max_iter >= 1; }

}  // namespace dotmi

extern "C" {

int dotmi_solve_hessian(dotmi_handle *h, const double *b, double *u, double rel_tol, int32_t max_iter, int32_t *iters, double *rel_res)
{
    if (!h) return DOTMI_E_INVALID;
    if (!b || !u) {
        h->err = "dotmi_solve_hessian: b and u must be given";
        return DOTMI_E_INVALID;
    }
    if (!pcg_settings_ok(rel_tol, max_iter)) {
        h->err = "dotmi_solve_hessian: rel_tol must be finite and positive, max_iter at least 1";
        return DOTMI_E_INVALID;
    }
    if (const char *why = pcg_refusal(h)) {
        h->err = std::string("dotmi_solve_hessian: ") + why;
        return DOTMI_E_INVALID;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    if (int rc = enter_with_factors(h)) return rc;
    HIPCHECK(h, hipMemcpyAsync(h->tmpn, b, sizeof(double) * h->n, hipMemcpyHostToDevice, h->st));
    int it = 0;
    double res = 0.0;
    const int rc = pcg_solve(h, h->tmpn, rel_tol, max_iter, h->pcgEvery, &it, &res);
    if (rc < 0) return rc;
    HIPCHECK(h, hipMemcpyAsync(u, h->p, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->st));
    HIPCHECK(h, hipStreamSynchronize(h->st));
    if (iters) *iters = it;
    if (rel_res) *rel_res = res;
    return rc;
}

int dotmi_set_pcg(dotmi_handle *h, double rel_tol, int32_t max_iter, int32_t check_every)
{
    if (!h) return DOTMI_E_INVALID;
    if (!pcg_settings_ok(rel_tol, max_iter) || check_every < 1) {
        h->err = "dotmi_set_pcg: rel_tol must be finite and positive, max_iter and check_every at least 1";
        return DOTMI_E_INVALID;
    }
    h->pcgTol = rel_tol;
    h->pcgCap = max_iter;
    h->pcgEvery = check_every;
    return 0;
}

int dotmi_pcg_info(const dotmi_handle *h, int64_t *solves, int64_t *iters_total, int32_t *last_iters, double *last_rel_res)
{
    if (!h) return DOTMI_E_INVALID;
    if (solves) *solves = h->pcgSolves;
    if (iters_total) *iters_total = h->pcgItersTotal;
    if (last_iters) *last_iters = h->pcgLastIters;
    if (last_rel_res) *last_rel_res = h->pcgLastRes;
    return 0;
}

}  // extern "C"
