// dotmi_loop.hip -- one time step (DOTTimeStepper::fullyImplicit / solve_oneStep, DOTTimeStepper.cpp:273-504; Optimizer::lineSearch, Optimizer.cpp:752-881): dotmi_step, the pieces every loop driver shares, the host-driven L-BFGS-H loop and its GSDD and Newton siblings (the device-resident loop: dotmi_devloop.hip)
#include "dotmi_handle.hpp"
#include "loop_verdict.hpp"   // the back-tracking test, the stopped-launch count

namespace dotmi {

// DOTMI_FLAG_TIME_PHASES: a phase boundary on the stream; the interval that ends here is booked under `slot`
// (slot < 0: the boundary only starts an interval)
inline void phase_mark(dotmi_handle *h, int slot)
{
    if (!h->timePhases || h->evPn >= 8) return;
    hipEventRecord(h->evP[h->evPn], h->st);
    h->evPslot[h->evPn] = slot;
    h->evPn++;
}

// after a stream synchronisation: read the recorded brackets
inline void phase_collect(dotmi_handle *h)
{
    for (int k = 1; k < h->evPn; ++k) {
        float ms = 0;
        if (h->evPslot[k] >= 0 && hipEventElapsedTime(&ms, h->evP[k - 1], h->evP[k]) == hipSuccess)
            h->phaseMs[h->evPslot[k]] += ms;
    }
    h->evPn = 0;
}

// DOTMI_FLAG_TIME_BACKSOLVE: the event pair around the back-solve about to be launched, or nulls (an event record costs ~6 us
// of stream time: sample, do not bracket every launch)
Bracket backsolve_bracket(dotmi_handle *h)
{
    const bool timed = (h->flags & DOTMI_FLAG_TIME_BACKSOLVE) && h->evUsed + 2 <= (int)h->evPre.size() &&
                       (h->timeCount++ % h->timeStride) == 0;
    if (!timed) return Bracket{nullptr, nullptr, -1};
    h->evUsed += 2;
    return Bracket{h->evPre[h->evUsed - 2], h->evPre[h->evUsed - 1], h->evUsed - 2};
}

// this rank's rows of p.g and p.Hp -> two scalars -> summed over the ranks (row 0 of partG; rows >= 1 stay zero); *spart: the
// partials alpha_0 is formed from
int reduce_step_dots(dotmi_handle *h, const double **spart)
{
    *spart = h->partS;
    if (!h->shardElems) return 0;
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(64), 0, h->st, h->partS, NB_RED, RED_K, 2, 0.0, 0.0, 0, h->partG);
    *spart = h->partG;
    return allreduce_sum(h, h->partG, 2);
}

// E_local = dtSq * sum(elastic) + sum(inertia) of nb blocks of energy partials into *dst (packed behind a gradient that is
// about to be all-reduced)
void stage_energy(dotmi_handle *h, int nb, double *dst)
{
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(1), dim3(64), 0, h->st, h->partE, nb, 2, 2, h->dtSq, 1.0, 1, dst);
}

// ---- the operand records of the loop's launches, built from the handle once (dotmi_handle.hpp); the call sites set what differs ----
GatherArgs gather_args(const dotmi_handle *h) { return {.xt = h->xt, .iv0 = h->v0, .iv1 = h->v1, .wide = h->tune.wideForms}; }

// the early order's gather: the new pair and its statistics, H s_new = alpha H p beside s_new (the fused direction kernel's H p: the
// owner exchange has no other), -g_trial straight into the padded right-hand sides
GatherArgs early_gather_args(const dotmi_handle *h)
{
    return {.xt = h->xt, .p = h->p, .alpha_dev = h->alpha_dev, .make_pair = 1, .iv0 = h->v0, .iv1 = h->v1, .vp_ptr = h->P.vp_ptr,
            .vp_off = h->P.vp_off, .rpad = h->P.rpad, .hp = h->tune.fuseDir ? h->Hp : nullptr, .wide = h->tune.wideForms};
}

// the loop's direction kernel (build_p + spmv_dots in one launch, H p from the cached H s_j) in its three forms
SpmvZpArgs spmv_zp_args(const dotmi_handle *h, bool sharded)
{
    if (sharded && h->owner)   // the held rows with this rank's own elements' part of H; the y_i . z came with the packet
        return {.Hval = h->HvalOwn, .z = h->z, .c_partials = h->partGC, .p = h->p, .Hp = h->Hp, .partials = h->partS,
                .rowMask = h->heldMask, .ownMask = h->ownMask, .vl = h->held(), .wide = h->tune.wideForms};
    // one rank: the y_i . z partials from their column-major twin, which merge_early writes beside the rows; partST: the twin of
    // p.g / p.Hp that elem_vertex_kernel reads; a sharded element pass: this rank's rows
    const bool rows = sharded && h->shardElems;
    return {.Hval = h->Hval, .z = h->z, .c_partials = h->dist ? h->partC : h->partCT, .ctrans = !h->dist, .p = h->p, .Hp = h->Hp,
            .partials = h->partS, .partialsT = h->partST, .v0 = rows ? h->v0 : 0, .v1 = rows ? h->v1 : -1, .wide = h->tune.wideForms};
}

// x_trial = x + alpha p, alpha from the p.g / p.Hp partials when there are any; the step taken goes to alpha_dev
StepForwardArgs step_forward_args(const dotmi_handle *h, const double *spmv_partials, double alpha)
{
    return {.x0 = h->x, .p = h->p, .x = h->x_trial, .spmv_partials = spmv_partials, .alpha = alpha, .alpha_min = h->alphaMin,
            .alpha_out = h->alpha_dev};
}

StepElemPass step_elem_pass(const dotmi_handle *h, const double *x, int grad, bool sharded)
{
    const bool ow = sharded && h->owner;
    return {ow ? h->Mown : h->M, {.x = x, .xt = h->xt, .v0 = ow ? 0 : h->v0, .v1 = ow ? h->nV : h->v1, .grad = grad, .partials = h->partE}};
}

int eval_all_elements(dotmi_handle *h, const double *x, int grad)
{
    const int nb = launch_elem_pass(h->M, h->PTall, h->mat, h->dtSq, {.x = x, .xt = h->xt, .v1 = h->nV, .grad = grad, .partials = h->partE}, h->st);
    if (grad) launch_vertex_gather(h->M, h->PTall, {.x = x, .xt = h->xt, .g_new = h->g_trial, .iv1 = h->nV}, NO_HISTORY, h->partR, h->st);
    return nb;
}

double energy_of_partials(const dotmi_handle *h, int nb)
{
    const double se = chunked_sum(nb, [&](int b) { return h->h_partE[2 * b]; });
    const double si = chunked_sum(nb, [&](int b) { return h->h_partE[2 * b + 1]; });
    return h->dtSq * se + si;
}

int gradient_over_ranks(dotmi_handle *h, int nb, const GatherArgs &pair)
{
    const int n = h->n;
    GatherArgs ag = pair;   // the gather only stages this rank's part: no pair, no right-hand sides, no H s_new
    ag.make_pair = 0;
    ag.stage = 1;
    ag.g_new = h->gstage;
    ag.hp = nullptr;
    ag.vp_ptr = ag.vp_off = nullptr;
    ag.rpad = nullptr;
    launch_vertex_gather(h->M, h->PT, ag, NO_HISTORY, h->partR, h->st, h->ctl);
    stage_energy(h, nb, h->gstage + n + 1);   // [g (n) ; 0 ; E_local]
    if (int rc = allreduce_sum(h, h->gstage, (size_t)n + 2)) return rc;
    // (pair_stats copies the summed gradient to the trial gradient, whose address only the controller knows)
    launch_pair_stats(n, pair, NO_HISTORY, h->partR, h->st, h->gstage, h->ctl);
    return 0;
}

// p = D^-1 sum_s R_s^T W_s R_s q   (DOTTimeStepper.cpp:406-450); leaves y_i.z partials in partC
// dotmi_set_dot_coarse with an active term: + Z A0^-1 Z^T q -- the restriction from the padded right-hand sides (where launch_gemv has
// put q, or build_qpad before it) and the coarse solve behind the back-solve, the prolongation inside the merge (sharded subdomains,
// DOTMI_FLAG_DOT_COARSE: the restriction in the tail of z's packet, the solve behind the collective, the prolongation in zfinish)
// Mode 2 with an active term, the balanced form M'' = C + (I - C H) M (I - H C): q (a global vector: the gather into the padded
// right-hand sides is launch_gemv's) is deflated in front of the block solve, the merge leaves its division to the finishing kernel
// behind the second coarse solve, which adds Z (y1 - y2) and forms the y_i . z on the corrected vector (dot_coarse_deflate / _balance)
int apply_precond(dotmi_handle *h, const double *q, double *z, const LbfgsArgs &L)
{
    if (dot_coarse_balanced(h)) {
        const double *r1 = dot_coarse_deflate(h, q);
        const Bracket br = backsolve_bracket(h);
        launch_gemv(h->P, r1, h->st, nullptr, br.ev0, br.ev1);
        launch_merge(h->M, h->P, L, {.z = z}, h->st);   // the sum over the subdomains: no division, no coarse term, no dots
        dot_coarse_balance(h, z, L);
        return 0;
    }
    const Bracket br = backsolve_bracket(h);
    launch_gemv(h->P, q, h->st, nullptr, br.ev0, br.ev1);
    const CoarseMerge *co = dot_coarse(h);
    if (h->dist) {
        // DOTMI_FLAG_DOT_COARSE: c = Z^T q of this rank's subdomains in the tail of z, summed with z; the solve on every rank behind the
        // collective; the prolongation behind the division (z: one of the handle's vectors, which have room for the tail)
        if (co) dot_coarse_restrict(h, z + h->n);
        return merge_over_ranks(h, L, z, RANKSUM_ZFINISH, nullptr);
    }
    if (co) dot_coarse_restrict_solve(h);
    launch_merge(h->M, h->P, L, {.z = z, .partials = h->partC, .dots = true, .divide = true, .co = co}, h->st);
    return 0;
}

// energy + element gradients + vertex gather (+ pair) at `xeval`; results: *E, stats in h_partR
int trial(dotmi_handle *h, const double *xeval, double *gout, int make_pair, const LbfgsArgs &L, int slot,
          double *E, int evalSlot = DOTMI_T_LINESEARCH_EVAL, int gradSlot = DOTMI_T_UPDATE_HISTORY)
{
    // single-GPU: the reduction partials go straight to pinned host memory (zero-copy), so one stream
    // synchronisation is the only host<->device interaction of a line-search trial
    StepElemPass e = step_elem_pass(h, xeval, 1);
    if (!h->shardElems) e.a.partials = h->h_partE;
    double *partR = h->shardElems ? h->partR : h->h_partR;
    const int nb = launch_elem_pass(e.M, h->PT, h->mat, h->dtSq, e.a, h->st);
    h->nbE = nb;
    phase_mark(h, evalSlot);
    GatherArgs a = gather_args(h);
    a.x = xeval;
    a.g_old = h->g;
    a.p = h->p;
    a.alpha_dev = h->alpha_dev;
    a.g_new = gout;
    a.s_new = h->S[slot];
    a.y_new = h->Y[slot];
    if (!h->shardElems) {
        a.make_pair = make_pair;
        launch_vertex_gather(h->M, h->PT, a, L, partR, h->st);
    } else {
        a.make_pair = 0;
        launch_vertex_gather(h->M, h->PT, a, L, h->partR, h->st);
        // pack E_local behind the gradient and reduce both in one collective
        stage_energy(h, nb, gout + h->n);
        if (int rc = allreduce_sum(h, gout, (size_t)h->n + 1)) return rc;
        if (make_pair) launch_pair_stats(h->n, a, L, h->partR, h->st);
        else {
            // |g|^2 only
            const double *vecs[1] = {gout};
            launch_multidot(h->n, gout, vecs, 1, h->partR, h->st);
        }
        HIPCHECK(h, hipMemcpyAsync(h->h_partE, gout + h->n, sizeof(double), hipMemcpyDeviceToHost, h->st));
        HIPCHECK(h, hipMemcpyAsync(h->h_partR, h->partR, sizeof(double) * NB_RED * RED_K, hipMemcpyDeviceToHost,
                                   h->st));
    }
    phase_mark(h, gradSlot);
    HIPCHECK(h, hipStreamSynchronize(h->st));
    phase_collect(h);
    *E = h->shardElems ? h->h_partE[0] : energy_of_partials(h, nb);
    if (h->world > 1) {
        // one set of control scalars for all ranks: rank 0's (energy, step length, every column of the statistics)
        h->ctrl[0] = *E;
        h->ctrl[1] = h->h_alpha[0];
        for (int j = 0; j < RED_K; ++j)
            h->ctrl[2 + j] = chunked_sum(h->M_nbR(), [&](int b) { return h->h_partR[(size_t)b * RED_K + j]; });
        if (int rc = adopt_rank0(h, h->ctrl, RED_K + 2)) return rc;
        *E = h->ctrl[0];
        h->h_alpha[0] = h->ctrl[1];
    }
    h->energy_evals++;
    return 0;
}

void sum_stats(const dotmi_handle *h, int nvals, double *R)
{
    if (h->world > 1) {   // what trial() adopted from rank 0
        for (int j = 0; j < nvals; ++j) R[j] = h->ctrl[2 + j];
        return;
    }
    for (int j = 0; j < nvals; ++j) R[j] = chunked_sum(NB_RED, [&](int b) { return h->h_partR[(size_t)b * RED_K + j]; });
}

// the operands of the one-launch element pass + gather on vertex patches (k_elemvert.hip)
ElemVertArgs elem_vertex_args(const dotmi_handle *h)
{
    ElemVertArgs a;
    memset(&a, 0, sizeof(a));
    a.mass = h->M.mass;
    a.xt = h->xt;
    a.p = h->p;
    a.hp = h->Hp;
    a.spmv_partials = h->partST;
    a.fixed = h->M.fixed;
    a.vp_ptr = h->P.vp_ptr;
    a.vp_off = h->P.vp_off;
    a.rpad = h->P.rpad;
    a.partE = h->partE;
    a.partR = h->partR;
    a.alpha_out = h->alpha_dev;
    a.dtSq = h->dtSq;
    a.alpha_min = h->alphaMin;
    return a;
}

// the host-driven loops' step: alpha also to pinned memory, where the host reads it after the trial
static void host_step(dotmi_handle *h, const double *spmv_partials, double alpha)
{
    StepForwardArgs a = step_forward_args(h, spmv_partials, alpha);
    a.alpha_out_host = h->h_alpha;
    launch_step_forward(h->n, a, h->st);
}

// The back-tracking line search (Optimizer.cpp:806-833; c1 = 0, lower bound 0) from a first trial at *alpha with energy *E:
// halve while the energy increases; *failed when the step length runs out.  marks: the retry's step launch is a phase of its own
// (DOTMI_FLAG_TIME_PHASES, the L-BFGS loop only)
static int backtrack(dotmi_handle *h, const LbfgsArgs &L, int make_pair, int slot, double lastE, bool marks, double *alpha,
                     double *E, bool *failed)
{
    while (ls_rejects(*E, lastE, *alpha)) {
        *alpha /= 2.0;
        h->numLineSearch++;
        if (*alpha == 0.0) {
            *failed = true;
            break;
        }
        if (marks) phase_mark(h, -1);
        host_step(h, nullptr, *alpha);
        if (marks) phase_mark(h, DOTMI_T_LINESEARCH_OTHER);
        if (int rc = trial(h, h->x_trial, h->g_trial, make_pair, L, slot, E)) return rc;
    }
    return 0;
}

// The reference's Gauss-Seidel domain-decomposition iteration (`timeStepper GSDD`, DOTTimeStepper::solve_oneStep_GSDD,
// DOTTimeStepper.cpp:507-565, driven by fullyImplicit :299-337) on this path's factors and kernels: one sweep over the
// subdomains per iteration; for subdomain s  p_s = H_s^-1 (-g restricted to s)  (:521-527), the search direction is p_s
// on the subdomain's vertices and zero elsewhere (:529-532), the line search starts from step 1 (initStepSize,
// Optimizer.cpp:1076-1093: only TST_DOT estimates it) and halves while the energy increases, and the gradient is
// brought up to date before the next subdomain (:541-551).  Host-driven: every trial needs its energy on the host.
static int run_gsdd_loop(dotmi_handle *h, LoopOut &r)
{
    const int n = h->n;
    double R[RED_K];
    do {
        for (int ls = 0; ls < h->P.nParts && !r.failed; ++ls) {
            launch_build_q(n, h->g, NO_HISTORY, nullptr, h->q, h->st);                     // q = -g
            launch_gemv_part(h->P, ls, h->P.tileByPart + h->partTilePtr[ls], h->partTilePtr[ls + 1] - h->partTilePtr[ls],
                             h->P.lworkByPart + h->partLworkPtr[ls], h->partLworkPtr[ls + 1] - h->partLworkPtr[ls],
                             h->q, n, h->p, h->st);
            double alpha = 1.0, E = 0;
            host_step(h, nullptr, alpha);
            if (int rc = trial(h, h->x_trial, h->g_trial, 0, NO_HISTORY, 0, &E)) return rc;
            if (int rc = backtrack(h, NO_HISTORY, 0, 0, r.lastE, false, &alpha, &E, &r.failed)) return rc;
            std::swap(h->x, h->x_trial);   // also on failure: the reference stays at the last trial point
            std::swap(h->g, h->g_trial);   // the gradient of the accepted point came with its energy
            r.lastE = E;
            h->log_alpha.push_back(alpha);
            h->log_E.push_back(E);
            sum_stats(h, 1, R);
            h->log_g2.push_back(R[0]);
        }
        if (r.failed) break;
        sum_stats(h, 1, R);
        r.g2 = R[0];
        if (++r.it >= h->iterCap) break;
    } while (r.g2 > h->targetGRes);
    return 0;
}

// The reference's projected Newton (`timeStepper Newton`: the base Optimizer::fullyImplicit, Optimizer.cpp:654-700, with
// Optimizer::solve_oneStep :703-749 and needRefactorize set): per iteration the projected Hessian at the current iterate
// is assembled and factorised (:705-729), p = H^-1 (-g) (:735-737), the line search starts from step 1 (initStepSize
// :1088) and the gradient is refreshed (:745).  Uses the same refresh / back-solve kernels as the DOT path.
// DOTMI_FLAG_NEWTON_PCG: the same loop with H p = -g solved by conjugate gradients on the subdomain factors (dotmi_pcg.hip).
static int run_newton_loop(dotmi_handle *h, LoopOut &r, double *ms_hess, double *ms_fact)
{
    const int n = h->n;
    double R[RED_K];
    do {
        if (int rc = refactor(h, h->x, ms_hess, ms_fact)) return rc;
        if (h->newtonPcg) {
            // DOTMI_FLAG_NEWTON_PCG: p = PCG(H, -g) on any number of subdomains (dotmi_pcg.hip).  A solve that ends at its cap or in
            // breakdown hands over its iterate all the same -- every CG iterate from zero is a descent direction -- and the step goes on
            launch_build_q(n, h->g, NO_HISTORY, nullptr, h->tmpn, h->st);              // b = -g
            int cg = 0;
            if (int rc = pcg_solve(h, h->tmpn, h->pcgTol, h->pcgCap, h->pcgEvery, &cg, nullptr); rc < 0) return rc;
            r.applies += cg;
        } else {
            launch_build_q(n, h->g, NO_HISTORY, nullptr, h->q, h->st);                 // q = -g
            if (int rc = apply_precond(h, h->q, h->p, NO_HISTORY)) return rc;           // p = H^-1 q (one subdomain: no averaging)
        }
        double alpha = 1.0, E = 0;
        host_step(h, nullptr, alpha);
        if (int rc = trial(h, h->x_trial, h->g_trial, 0, NO_HISTORY, 0, &E)) return rc;
        if (int rc = backtrack(h, NO_HISTORY, 0, 0, r.lastE, false, &alpha, &E, &r.failed)) return rc;
        std::swap(h->x, h->x_trial);
        std::swap(h->g, h->g_trial);
        r.lastE = E;
        if (r.failed) break;
        sum_stats(h, 1, R);
        r.g2 = R[0];
        h->log_alpha.push_back(alpha);
        h->log_E.push_back(E);
        h->log_g2.push_back(r.g2);
        if (++r.it >= h->iterCap) break;
    } while (r.g2 > h->targetGRes);
    return 0;
}

// The host-driven L-BFGS-H loop (DOTMI_FLAG_HOST_LOOP, LBFGS-PD and LBFGS-HI): one stream synchronisation per line-search trial, the
// two-loop's scalars and the accept / halve / converged decisions on the host.  In the q-based order of the reference
static int run_host_loop(dotmi_handle *h, LoopOut &r)
{
    const int n = h->n;
    double R[RED_K];
    do {
        // ---- two-loop, first half (host scalars, lbfgs_history.hpp) + q -----------------------------
        double xi[HIST_MAX];
        lbfgs_two_loop_xi(h->m, h->b, h->sy, h->ys, xi);
        const LbfgsArgs L = lbfgs_args(h);
        phase_mark(h, -1);
        if (h->pd) {
            // LBFGS-PD (LBFGSTimeStepper::solve_oneStep, :338-449): q interleaved, z = L^-1 q per coordinate (dotmi_pd.hip)
            launch_build_q(n, h->g, L, xi, h->q, h->st);
            phase_mark(h, DOTMI_T_MODIFY_GRAD);
            if (int rc = pd_apply(h, h->q, h->z, L)) return rc;
        } else if (h->hi) {
            // LBFGS-HI (D0T_HI, LBFGSTimeStepper.cpp:376-378): q interleaved, z = (L L^T)^-1 q through the colour launches (dotmi_ic.hip)
            launch_build_q(n, h->g, L, xi, h->q, h->st);
            phase_mark(h, DOTMI_T_MODIFY_GRAD);
            if (int rc = ic_apply(h, h->q, h->z, L)) return rc;
        } else {
            // q, straight into the padded right-hand sides (the balanced coarse term deflates the global vector first)
            const bool balanced = dot_coarse_balanced(h) != nullptr;
            if (balanced) launch_build_q(n, h->g, L, xi, h->q, h->st);
            else launch_build_qpad(h->P, h->g, L, xi, h->st);
            phase_mark(h, DOTMI_T_MODIFY_GRAD);
            // ---- subdomain back-solve, merge, second half ------------------------------------------------
            if (int rc = apply_precond(h, balanced ? h->q : nullptr, h->z, L)) return rc;
        }
        phase_mark(h, DOTMI_T_BACKSOLVE);
        launch_build_p(n, h->z, L, h->partC, xi, h->p, h->st);
        phase_mark(h, DOTMI_T_MODIFY_SEARCHDIR);
        // ---- alpha_0 and the first trial ---------------------------------------------------------------
        if (h->pd || h->hi) {
            // only TST_DOT estimates alpha_0 (Optimizer::initStepSize, Optimizer.cpp:1076-1093): the unit step, no H p
            host_step(h, nullptr, 1.0);
        } else {
            launch_spmv_dots(h->M, h->Hval, h->p, h->g, nullptr, h->v0, h->v1, h->partS, h->st);
            const double *spart = nullptr;
            if (int rc = reduce_step_dots(h, &spart)) return rc;
            host_step(h, spart, 0.0);
        }
        phase_mark(h, DOTMI_T_LINESEARCH_OTHER);
        const int slot = lbfgs_free_slot(h->hist, h->m, h->order);
        double E = 0;
        if (int rc = trial(h, h->x_trial, h->g_trial, 1, L, slot, &E)) return rc;
        double alpha = h->h_alpha[0];
        if (int rc = backtrack(h, L, 1, slot, r.lastE, true, &alpha, &E, &r.failed)) return rc;
        // on failure the reference leaves result.V at the last trial point and lastEnergyVal at its energy
        // (Optimizer.cpp:819-861); the iteration is not counted (DOTTimeStepper.cpp:311-316)
        std::swap(h->x, h->x_trial);
        r.lastE = E;
        if (r.failed) break;
        std::swap(h->g, h->g_trial);
        sum_stats(h, RED_K, R);
        r.g2 = R[0];
        // history update (DOTTimeStepper.cpp:474-494) from the statistics of the accepted trial: y.s, s.g and the three rows
        lbfgs_push_pair(h->hist, slot, R[1], R[2], R + 3, R + 3 + HIST_MAX, R + 3 + 2 * HIST_MAX, h->m, h->order, h->ys, h->b, h->sy);
        h->log_alpha.push_back(alpha);
        h->log_E.push_back(r.lastE);
        h->log_g2.push_back(r.g2);
        if (++r.it >= h->iterCap) break;
    } while (r.g2 > h->targetGRes);
    return 0;
}

// the step's counters and timings for the caller (ms_total is the caller's to set)
static void fill_step_stats(dotmi_handle *h, dotmi_step_stats *st, const LoopOut &r, int status, long long halvings)
{
    st->iters = r.it;
    st->ls_halvings = (int)halvings;
    st->energy_evals = h->energy_evals;
    st->status = status;
    st->E0 = r.E0;
    st->g2_0 = r.g20;
    st->E = r.lastE;
    st->g2 = r.g2;
    std::vector<char> ran(h->evUsed / 2 + 1, h->devLoop ? 0 : 1);
    // device loop: slots enqueued past the end, and line-search retries, ran no back-solve
    for (size_t sl = 0; sl < h->slotTimed.size(); ++sl)
        if (h->slotTimed[sl] >= 0 && sl < h->slotKind.size() && h->slotKind[sl] == 1) ran[h->slotTimed[sl] / 2] = 1;
    for (int k = 0; k + 1 < h->evUsed; k += 2) {
        if (!ran[k / 2]) continue;
        float ms = 0;
        hipEventElapsedTime(&ms, h->evPre[k], h->evPre[k + 1]);
        st->ms_precond += ms;
        st->precond_launches++;
    }
    st->precond_bytes = h->precond_bytes;
    st->factor_flops = h->factorFlops;
    st->backsolve_launches = h->newtonPcg ? r.applies : r.it;   // (Newton-PCG: one block-solve application per CG iteration)
    // (only a step in the early order pairs or speculates: choose_step_forms)
    st->backsolve_stopped = (h->devLoop && h->earlyNow) ? loop_stopped_launches(halvings, h->pairNow ? h->pairSlots : 0,
                                                                                h->pairNow ? h->pairRedo : 0, h->specNow ? h->specRedo : 0)
                                                        : 0;
    st->spec_slots = (h->devLoop && h->specNow) ? h->specSlots : 0;
    st->spec_redone = (h->devLoop && h->specNow) ? h->specRedo : 0;
    st->backsolve_held = (h->devLoop && h->earlyNow) ? h->heldSlots : 0;
    st->backsolve_held_rejected = (h->devLoop && h->earlyNow) ? h->heldRejected : 0;
    st->paired_slots = (h->devLoop && h->pairNow) ? h->pairSlots : 0;
    st->paired_redone = (h->devLoop && h->pairNow) ? h->pairRedo : 0;
    for (int k = 0; k + 1 < h->evArUsed; k += 2) {
        float ms = 0;
        hipEventElapsedTime(&ms, h->evAr[k], h->evAr[k + 1]);
        st->ms_collective += ms;
        st->collective_timed++;
        st->collective_timed_bytes += (int64_t)h->arTimedBytes[k / 2];
    }
    st->collective_calls = h->arCallsStep;
    st->collective_bytes = (int64_t)h->arBytesStep;
    for (int k = 0; k < DOTMI_T_COUNT; ++k) st->ms_phase[k] = h->phaseMs[k];
}

}  // namespace dotmi

extern "C" {

int dotmi_step(dotmi_handle *h, dotmi_step_stats *st)
{
    if (!h) return DOTMI_E_INVALID;
    HIPCHECK(h, hipSetDevice(h->device));
    // a refresh still running from the last step is judged BEFORE anything of this step is enqueued: a step never runs on
    // factors whose factorisation failed (what the caller did between the two steps has already overlapped the refresh)
    if (int rc = enter_with_factors(h)) return rc;
    if (int rc = dot_coarse_refresh(h)) return rc;   // (nothing in a step that follows a refresh: dotmi_set_dot_coarse builds behind it)
    const double T0 = now_ms();
    h->m = 0;
    h->energy_evals = 0;
    h->evUsed = 0;
    h->evArUsed = 0;
    h->arTimedBytes.clear();
    h->arCallsStep = 0;
    h->arBytesStep = 0;
    h->log_alpha.clear();
    h->log_E.clear();
    h->log_g2.clear();
    h->logPending = 0;
    const long long ls0 = h->numLineSearch;
    double ms_hess = 0, ms_fact = 0;

    for (double &v : h->phaseMs) v = 0.0;
    h->evPn = 0;
    phase_mark(h, -1);
    // initX(2): x += dt v + dt^2 g on free vertices (Optimizer.cpp:442-582); BDF2: x = x~, which the last update formed from x^, v^
    const bool bdf2 = h->tit == TIT_BDF2;
    if (bdf2) launch_bdf2_init_x(h->nV, h->M.fixed, h->xt, h->x, h->st);
    else launch_init_x(h->nV, h->M.fixed, h->v, h->dt, h->gdtsq, h->x, h->st);
    LoopOut r;
    if (!h->devLoop) {
        double R[RED_K];
        if (int rc = trial(h, h->x, h->g, 0, lbfgs_args(h), 0, &r.lastE, DOTMI_T_FULLYIMPLICIT_ECOMP, DOTMI_T_FULLYIMPLICIT_ECOMP))
            return rc;
        sum_stats(h, 1, R);
        r.g2 = R[0];
        r.E0 = r.lastE;
        r.g20 = r.g2;
    }

    int status = 0;
    const double Tloop = now_ms();
    h->slotKind.clear();
    h->slotTimed.clear();
    if (int rc = h->newton    ? run_newton_loop(h, r, &ms_hess, &ms_fact)
                 : h->gsdd    ? run_gsdd_loop(h, r)
                 : h->devLoop ? run_device_loop(h, r)
                              : run_host_loop(h, r))
        return rc;
    if (h->owner) {
        // owner exchange: the loop kept the positions of the vertices this rank holds; every rank's positions are made whole
        // again here, once per step (the owners' entries, zeros elsewhere, summed) -- the refresh reads the halo elements'
        // vertices, dotmi_get_state everything
        launch_mask_owned(h->n, h->x, h->ownMask, h->st);
        if (int rc = allreduce_sum(h, h->x, (size_t)h->n)) return rc;
    }
    double Tloop1 = now_ms();
    ms_hess += h->carryHess;
    ms_fact += h->carryFact;
    h->carryHess = h->carryFact = 0.0;

    // BDF2: from here on the launches take the NEXT step's effective step -- the refresh below is issued at it.  It changes only at the
    // hand-over from the backward-Euler start step (dt) to the first BDF2 step (2/3 dt): there a failed step refreshes all the same,
    // LBFGS-PD factors its L once more below, LBFGS-HI and Newton read the new fields in their own refresh
    const double dtDone = h->dt;
    TitPlan next{};
    bool handOver = false;
    if (bdf2) {
        next = tit_plan(TIT_BDF2, h->dtUser, h->dtUser, 1);
        handOver = tit_apply(h, next);
        h->levels = 1;
        h->dtPrev = h->dtUser;
    }
    // (Newton refreshes at the START of every iteration instead; LBFGS-PD's preconditioner is constant: LBFGSTimeStepper::fullyImplicit
    // refactors only for H, HI and JH, :296-335)
    const bool refreshAtEnd = (!r.failed || handOver) && !h->newton && !h->pd;
    if (r.failed || r.it >= h->iterCap) status = 2;
    // (LBFGS-HI: its refresh takes one read-back per factorisation attempt, so it runs whole behind the BE update below)
    if (refreshAtEnd && !h->hi)
        if (int rc = refactor_issue(h, h->x)) return rc;
    // BE update (Optimizer.cpp:354-361); BDF2: v+ = (x - x^) / dt_e, the shift of the levels, the next step's x^ and x~
    phase_mark(h, -1);
    if (bdf2)
        launch_bdf2_update(h->nV, h->M.fixed, h->x, h->xhat, h->xn, h->v, h->xnm1, h->vnm1, h->xt, dtDone, next, h->gdtsq, h->st);
    else launch_be_update(h->nV, h->M.fixed, h->x, h->xn, h->v, h->xt, h->dt, h->gdtsq, h->st);
    phase_mark(h, DOTMI_T_SOLVE_EXTRACOMP);
    int rcFactor = 0;
    const bool asyncRefresh = refreshAtEnd && (h->flags & DOTMI_FLAG_ASYNC_REFRESH) && h->devLoop && !h->dist;
    if (asyncRefresh) {
        // the refresh and the BE update stay queued; whoever needs their result next waits for them (resolve_refresh)
        h->refreshPending = true;
    } else {
        HIPCHECK(h, hipStreamSynchronize(h->st));
        phase_collect(h);
        HIPCHECK(h, hipGetLastError());
        if (refreshAtEnd) rcFactor = h->hi ? ic_refresh(h, h->x, &ms_hess, &ms_fact) : refactor_finish(h, &ms_hess, &ms_fact);
        else if (handOver && h->pd) rcFactor = pd_factor(h);
        if (rcFactor == DOTMI_E_DEVICE) return rcFactor;
    }
    if (st) {
        memset(st, 0, sizeof(*st));
        st->ms_total = now_ms() - T0;
        st->ms_loop = Tloop1 - Tloop;
        st->ms_hessian = ms_hess;
        st->ms_factor = ms_fact;
        fill_step_stats(h, st, r, status, h->numLineSearch - ls0);
    }
    // a non-SPD subdomain: the step itself is complete (x, v advanced as the reference would have before it
    // exit(-1)s in the factorisation, Optimizer.cpp:301-313), the handle is poisoned until a refactor succeeds
    if (rcFactor) return rcFactor;
    return status;
}

}  // extern "C"
