// dotmi_devloop.hip -- the device-resident L-BFGS-H loop of one time step: the stages of a slot in the early and the q-based
// order, and run_device_loop's parts (forms of the step, DevLoop, start-of-step evaluation, the two enqueue policies, harvest)
#include "dotmi_handle.hpp"

namespace dotmi {

// what the stages of one early-order slot hand to each other
struct Slot {
    int nb = 0;                      // blocks of energy partials the controller sums
    const double *spart = nullptr;   // the p.g / p.Hp partials alpha_0 comes from
    const double *ctlE = nullptr;    // where the controller reads the energy partials
};

// stage 1, direction: p = z + sum delta_j s_j with H p and the p.g / p.Hp partials
static int slot_direction(dotmi_handle *h, Slot &s)
{
    if (h->specNow) {
        // the direction kernel and the first trial's element pass at the unit step in ONE launch (k_dirstep.hip); a retry slot:
        // the element pass alone, on the stored p with the controller's alpha
        const StepArgs sa{h->p, h->partS, h->alpha_dev, h->alphaMin};
        StepElemPass e = step_elem_pass(h, h->x_trial, 1);
        e.a.step = &sa;
        s.nb = launch_dirstep(e.M, h->PTspec, h->mat, h->dtSq, spmv_zp_args(h), e.a, h->st, h->ctl);
    } else if (h->owner || h->tune.fuseDir) {   // build_p + spmv_dots in one launch, H p from the cached H s_j
        launch_spmv_zp(h->M, spmv_zp_args(h), h->st, h->ctl);
    } else {
        launch_build_p(h->n, h->z, NO_HISTORY, h->partC, nullptr, h->p, h->st, h->ctl);
        launch_spmv_dots(h->M, h->Hval, h->p, h->g, nullptr, h->v0, h->v1, h->partS, h->st, h->ctl);
    }
    // (sharded element pass: the two sums cannot ride on the z all-reduce in front of them -- p.Hp is quadratic in the reduced
    // vector)
    return reduce_step_dots(h, &s.spart);
}

// stage 2, trial: the step x_trial = x_cur + alpha p and the element pass there
static void slot_trial(dotmi_handle *h, Slot &s)
{
    // (not on meshes whose workgroups walk several patches: the prefetched operands leave no registers for it)
    // (sharded element pass: the fused form writes the trial point only on this rank's vertex slice -- its inertia loop --,
    // so the step stays a launch of its own there)
    // (owner exchange: the inertia loop runs over every vertex with the owner's share of the mass, so the fused form writes the
    // whole trial point there too -- x + alpha 0 off the held vertices)
    if (h->specNow) {
    } else if (h->vpNow) {
        // vertex patches: the element pass, the step, the gather, the pair and its statistics, -g into the right-hand sides: one launch
        ElemVertArgs ea = elem_vertex_args(h);
        if (h->pairNow) ea.alpha_min = -h->alphaMin;   // (negative: a paired launch, as StepArgs::alpha_min)
        launch_elem_vertex(h->VP, h->mat, ea, h->st, h->ctl);
        s.nb = h->VP.nPatches;
    } else {
        StepElemPass e = step_elem_pass(h, h->x_trial, 1);
        const StepArgs sa{h->p, s.spart, h->alpha_dev, h->pairNow ? -h->alphaMin : h->alphaMin};   // (negative: a paired launch)
        if (h->tune.fuseStep && (!h->shardElems || h->owner)) {   // the step inside the element pass
            e.a.step = &sa;
            e.a.pair = h->pairNow;   // (a step with paired trials takes the PAIR instantiations)
        } else {
            StepForwardArgs f = step_forward_args(h, s.spart);
            f.vl = h->held();
            launch_step_forward(h->n, f, h->st, h->ctl);
        }
        s.nb = launch_elem_pass(e.M, h->PT, h->mat, h->dtSq, e.a, h->st, h->ctl);
    }
}

// stage 3, gradient: the trial gradient, the new pair and its statistics; -g_trial goes straight into the padded right-hand
// sides, whatever the controller will say about the trial
static int slot_gradient(dotmi_handle *h, Slot &s)
{
    const int n = h->n;
    const GatherArgs a = early_gather_args(h);
    s.ctlE = h->partE;
    if (h->vpNow) {
    } else if (!h->shardElems) {
        launch_vertex_gather(h->M, h->stepPT(), a, NO_HISTORY, h->partR, h->st, h->ctl);
    } else if (h->owner) {
        // Owner exchange, the statistics in the gradient's packet.  The gradient is complete on the vertices only this rank
        // holds: the gather forms the pair, the right-hand sides and the statistics there as on one GPU; on the shared vertices
        // it leaves this rank's part of the gradient in the staging buffer and its share of the sums -- those are linear in the
        // gradient -- in the partials, which ride in the packet's tail (summed by the pack's workgroup 0, like E).  After the
        // exchange only the shared vertices are left (|g|^2 over them: from the summed packet, in the unpack)
        GatherArgs ag = a;
        ag.ownMask = h->ownMask;
        ag.vlist = h->heldList;
        ag.nlist = h->nHeld;
        ag.kind = h->vkind;
        ag.pre = 1;
        ag.gshare = h->gstage;
        launch_vertex_gather(h->M, h->PT, ag, NO_HISTORY, h->partR, h->st, h->ctl);
        if (int rc = exchange_gradient_packed(h, n, s.nb, h->partR, RED_K)) return rc;
        ag.vlist = h->sharedList;
        ag.nlist = h->nShared;
        ag.pre = 0;
        if (h->nShared > 0) launch_pair_stats(n, ag, NO_HISTORY, nullptr, h->st, h->gstage, h->ctl);
        s.ctlE = h->gstage + n;   // the controller reads the energy as one block (0, E)
        s.nb = 1;
    } else {
        // this rank's partial gradient and energy to the staging buffer [g (n) ; 0 ; E_local], one all-reduce, then the pair,
        // its statistics, -g into the right-hand sides and H s_new from the SUM (pair_stats)
        if (int rc = gradient_over_ranks(h, s.nb, a)) return rc;
        s.ctlE = h->gstage + n;   // the controller reads the energy as one block (0, E)
        s.nb = 1;
    }
    return 0;
}

// stage 3b (dotmi_set_dot_coarse with an active term), coarse: c = Z^T (-g_trial) from the padded right-hand sides the gradient stage has
// just written, y = A0^-1 c.  Like the back-solve behind them the two kernels run whatever the controller will say about the trial --
// in a retry slot too, whose trial may be the accepted one --, and return at once past the end of the loop.  They write c and the
// parts of y only; a merge that is gated off never reads them, so held, stopped, paired and two-level slots need nothing else
// Sharded subdomains (DOTMI_FLAG_DOT_COARSE): only the restriction runs here, over the rank's own subdomains into the tail of the
// staging buffer slot_merge all-reduces; the solve follows that collective
static void slot_coarse(dotmi_handle *h)
{
    if (!dot_coarse(h)) return;
    if (h->dist) dot_coarse_restrict(h, h->zstage + h->n, h->ctl, 1);
    else dot_coarse_restrict_solve(h, h->ctl, 1);
}

// stage 4, back-solve on -g_trial with the controller as one workgroup of its launch
static void slot_backsolve(dotmi_handle *h, const Slot &s)
{
    const double *ctlR = h->owner ? h->partGR : h->partR;   // owner exchange: the statistics rode in the gradient's packet
    const Bracket br = backsolve_bracket(h);
    h->slotTimed.push_back(br.at);
    CtlLaunch ca{{h->ctl, s.ctlE, ctlR, h->alpha_dev, h->h_flags, s.nb, h->pairNow ? 2 : 0}, h->ctlForm};
    launch_gemv(h->P, nullptr, h->st, h->ctl, br.ev0, br.ev1, &ca, (int)h->slotTimed.size() /* the slot's epoch, 1-based */);
}

// stage 5, merge: z = u - sum_j xi_j (M y_j) from the tile partials and the cached M y_j (dotmi_set_dot_coarse: u with + Z y, so the
// cached vectors are M' y_j)
static int slot_merge(dotmi_handle *h)
{
    if (!h->dist) {
        launch_merge_early(h->M, h->P, {.z = h->z, .partials = h->partC, .partialsT = h->partCT, .co = dot_coarse(h), .wide = h->tune.wideForms}, h->st, h->ctl);
    } else if (!h->owner) {
        // sharded subdomains: this rank's part of the sum, the one collective of the iteration (issued in every slot,
        // whatever the controller decided: every rank enqueues the same sequence), then the division and the history terms
        // (the sum travels in a staging buffer: in a slot whose merge is gated off -- retry, past the end -- the collective
        // still runs, on stale scratch, and z is left alone)
        // DOTMI_FLAG_DOT_COARSE: the packet is [zsum (n) ; c (nc)] -- slot_coarse has left this rank's part of c = Z^T (-g_trial) in the
        // tail --, every rank solves A0 y = c on the summed tail behind the collective (gated like the merge that reads y: the
        // controller has spoken by now) and the zsum branch of the merge adds Z y behind the division
        return merge_over_ranks(h, NO_HISTORY, h->zstage, RANKSUM_EARLY, h->ctl, h->held());
    } else {
        // owner exchange: merge_early merges the tiles itself.
        // zstage: this rank's subdomains' sum, zero on the vertices it does not hold; only the shared vertices' entries
        // are summed over the ranks.  z is then whole on the held vertices and zero elsewhere -- and so is everything
        // the loop forms from it.  The five y_i . z travel inside the packet: merge_early merges this rank's tiles itself -- z,
        // u_old, M y_new and the y_i . z on the vertices only this rank holds, its part of the sum (to zstage) and its share
        // of the y_i . z on the shared ones --, then the exchange, then the shared vertices
        launch_merge_early(h->M, h->P, {.z = h->z, .partials = h->partC, .ownMask = h->ownMask, .vl = h->held(), .kind = h->vkind, .pre = 1,
                                        .zshare = h->zstage, .wide = h->tune.wideForms}, h->st, h->ctl);
        if (int rc = exchange_solve_packed(h)) return rc;
        if (h->nShared > 0)
            launch_merge_early(h->M, h->P, {.z = h->z, .zsum = h->zstage, .ownMask = h->ownMask, .vl = h->shared(), .wide = h->tune.wideForms}, h->st, h->ctl);
    }
    return 0;
}

// One slot of the device-resident loop in the early order (h->earlyNow): the preconditioner M is fixed during a step and
// linear, so the solve for the next direction does not have to wait for the controller's verdict and for q.  The slot starts at
// the direction; after the trial's gradient is gathered the back-solve runs on -g_trial with the CONTROLLER AS ONE WORKGROUP OF
// ITS LAUNCH, and merge_early forms z = u - sum_j xi_j (M y_j) from the cached M y_j (the newest: u_old - u).  The controller's
// ~7 us and its launch boundary leave the critical path of every iteration; a rejected trial (line-search halving) and the last
// iteration of a step stream the factors once for nothing.  z differs from the q-based value by rounding only
// (tests/test_gpu_round3.py: same iteration counts, positions to 1e-9).
static int enqueue_loop_slot_early(dotmi_handle *h)
{
    Slot s;
    if (int rc = slot_direction(h, s)) return rc;
    slot_trial(h, s);
    if (int rc = slot_gradient(h, s)) return rc;
    slot_coarse(h);
    slot_backsolve(h, s);
    return slot_merge(h);
}

// One slot in the q-based order (DOTMI_EARLY_BACKSOLVE=0; the order the host loop is bit-identical to): the nine kernels of an
// L-BFGS iteration (or, when the controller asked for a retry, only the three of a line-search trial -- the others return at
// once) and the controller.
static int enqueue_loop_slot(dotmi_handle *h)
{
    if (h->earlyNow) return enqueue_loop_slot_early(h);
    const int n = h->n;
    // dotmi_set_dot_coarse_mode, mode 2 (the balanced form, one rank): q as a global vector, y1 = A0^-1 Z^T q and r1 = q - W y1 between
    // build_q and the gather into the padded right-hand sides (launch_gemv's); behind the merge -- the sum over the subdomains only --
    // c1 - W^T u, the second coarse solve and the finishing kernel with the division, Z (y1 - y2) and the y_i . z.  All gated like
    // the back-solve of this order
    const CoarseMerge *bal = dot_coarse_balanced(h);
    const double *r1 = nullptr;
    if (bal) {
        launch_build_q(n, h->g, NO_HISTORY, nullptr, h->q, h->st, h->ctl);
        r1 = dot_coarse_deflate(h, h->q, h->ctl);
    } else {
        launch_build_qpad(h->P, h->g, NO_HISTORY, nullptr, h->st, h->ctl);   // q, straight into the padded right-hand sides
    }
    const CoarseMerge *co = dot_coarse(h);
    // dotmi_set_dot_coarse: y = A0^-1 Z^T q, gated like the back-solve (sharded subdomains: the restriction into the tail of z's
    // packet here, the solve behind the collective below)
    if (co && h->dist) dot_coarse_restrict(h, h->z + n, h->ctl, 0);
    else if (co) dot_coarse_restrict_solve(h, h->ctl, 0);
    const Bracket br = backsolve_bracket(h);
    h->slotTimed.push_back(br.at);
    launch_gemv(h->P, r1, h->st, h->ctl, br.ev0, br.ev1);
    if (bal) {
        launch_merge(h->M, h->P, NO_HISTORY, {.z = h->z}, h->st, h->ctl);
        dot_coarse_balance(h, h->z, NO_HISTORY, h->ctl);
    } else if (!h->dist) {
        launch_merge(h->M, h->P, NO_HISTORY, {.z = h->z, .partials = h->partC, .dots = true, .divide = true, .co = co}, h->st, h->ctl);
    } else {
        // sharded subdomains: the one collective of an iteration, enqueued like a kernel.  It runs in every slot (also
        // in retries and past the end, where the kernels around it return at once), so every rank issues the same
        // sequence of collectives whatever the controller decides
        if (int rc = merge_over_ranks(h, NO_HISTORY, h->z, RANKSUM_ZFINISH, h->ctl)) return rc;
    }
    launch_build_p(n, h->z, NO_HISTORY, h->partC, nullptr, h->p, h->st, h->ctl);
    launch_spmv_dots(h->M, h->Hval, h->p, h->g, nullptr, h->v0, h->v1, h->partS, h->st, h->ctl);
    const double *spart = nullptr;
    if (int rc = reduce_step_dots(h, &spart)) return rc;
    launch_step_forward(n, step_forward_args(h, spart), h->st, h->ctl);
    const StepElemPass e = step_elem_pass(h, h->x_trial, 1);
    const int nb = launch_elem_pass(e.M, h->PT, h->mat, h->dtSq, e.a, h->st, h->ctl);
    GatherArgs a = gather_args(h);
    a.p = h->p;
    a.alpha_dev = h->alpha_dev;
    a.make_pair = 1;
    if (!h->shardElems) {
        launch_vertex_gather(h->M, h->PT, a, NO_HISTORY, h->partR, h->st, h->ctl);
        launch_loop_control(h->ctl, h->partE, nb, h->partR, h->alpha_dev, h->h_flags, h->st);
        return 0;
    }
    // sharded element pass: the gradient and the energy summed over the ranks, the pair + statistics from the sum (no right-hand
    // sides, no H s_new in this order).  The controller reads the energy as one "block" (0, E): dtSq * 0 + E.
    if (int rc = gradient_over_ranks(h, nb, a)) return rc;
    launch_loop_control(h->ctl, h->gstage + n, 1, h->partR, h->alpha_dev, h->h_flags, h->st);
    return 0;
}

// which forms the slots of this step take
static void choose_step_forms(dotmi_handle *h)
{
    // The early order (back-solve issued on the trial gradient, beside the controller) in every step of a handle that has its
    // buffers: it takes the controller (~9 us with its launch boundary) off every iteration and starts a back-solve for
    // nothing per rejected trial and once at the end of the step, which the controller tells to stop (DevLoop::abortEpoch).
    // (Round 3's per-step rule from the previous step's counts, DOTMI_EARLY_BACKSOLVE=1, is gone: with the stop and the held
    // launches the early order is at least as fast on every workload, and the owner exchange has no other order -- ADVICE r04.)
    // (not in a step with the balanced coarse term active: the early order's merge forms z, M y_new and the y_i . z from u inside its
    // own launch, before the second coarse solution can exist -- such a step runs the q-based order)
    h->earlyNow = h->earlyBs && !dot_coarse_balanced(h);
    // paired trials: one rank, the fused step inside the element pass, the early order with held launches (the tiles of a paired
    // slot wait for the verdict); -1: only in steps that follow a step with halvings in at least a quarter of its iterations
    h->pairNow = h->earlyNow && !h->dist && h->tune.fuseStep && h->tune.fuseDir && h->tune.earlyHold &&
                 (h->tune.pairTrials > 0 || (h->tune.pairTrials < 0 && h->prevIters > 0 && 4 * h->prevHalv >= h->prevIters));
    // the unit step speculatively beside the direction kernel: one rank, the fused kernels, every patch a workgroup, no pairing
    // in this step (a step whose predecessor halved often); -1: only after a step whose first trials took the unit estimate at
    // least nine times in ten (a slot whose estimate is below 1 is redone: ~45 us lost against ~10 saved)
    // (not on a handle with dotmi_set_dot_coarse on: the coarse stage has not been run under the speculative slots)
    h->specNow = h->earlyNow && !h->dist && !h->pairNow && h->tune.fuseStep && h->tune.fuseDir &&
                 h->specFits && h->coarse.dotMode == 0 &&
                 (h->tune.specStep > 0 || (h->tune.specStep < 0 && h->prevFirst > 0 && 10 * h->prevUnit >= 9 * h->prevFirst));
    // the trial's element pass + gather as one launch on vertex patches (paired steps too: elem_vertex_kernel<MAT, true>); a step that
    // speculates keeps the element patches (one patch set per step: the start-of-step evaluation and the trials group their
    // energy partials alike)
    // A step that pairs its trials (its predecessor halved in a quarter of its iterations) keeps the element patches unless the
    // vertex patches are forced: a rejected trial costs the whole fused launch there (18 us against the element pass' 10), and the
    // second half of a paired launch is the element pass' energy only -- stiff monkey, ten steps, same box: 15.12 -> 14.17 ms per
    // step (111.8 -> 107.6 us per iteration)
    h->vpNow = h->vpFits && h->earlyNow && !h->dist && !h->specNow && !(h->pairNow && h->tune.vertexPatches < 0);
    // the controller that understands these slots
    h->ctlForm = h->pairNow ? (h->vpNow ? CTL_PAIR_VP : CTL_PAIR) : h->specNow ? CTL_SPEC : h->vpNow ? CTL_VP : CTL_PLAIN;
}

// the loop state of a fresh step, filled in pinned memory and uploaded; returns the slot from which the controller posts progress
static int init_devloop(dotmi_handle *h, int *notifyFrom)
{
    DevLoop &C = *h->h_ctl;
    memset(&C, 0, sizeof(C));
    C.specPartials = h->partS;
    C.alphaMin = h->alphaMin;
    C.iterCap = h->iterCap;
    C.hist = h->hist;
    C.tol = h->targetGRes;
    C.dtSq = h->dtSq;
    C.x_cur = h->x;
    C.x_trial = h->x_trial;
    C.g_cur = h->g;
    C.g_trial = h->g_trial;
    for (int s = 0; s <= h->hist; ++s) {
        C.S[s] = h->S[s];
        C.Y[s] = h->Y[s];
        C.MY[s] = h->MY[s];
        C.HS[s] = h->HS[s];
    }
    C.u_old = h->u_old;
    C.hrec = h->hrec;
    devloop_resolve(C);   // (slot 0, no pair yet)
    C.holdEnable = h->tune.earlyHold ? 1 : 0;
    // the forecast carries over from the last step (a function of the handle's own history)
    memcpy(C.predHist, h->predState, sizeof(int) * 2);
    memcpy(&C.predCtr[0][0], h->predState + 2, sizeof(int) * 8);
    memcpy(C.pairCtr, h->pairState, sizeof(int) * 3);
    C.log_alpha = h->dlog;
    C.log_E = h->dlog + h->logCap;
    C.log_g2 = h->dlog + 2 * (size_t)h->logCap;
    C.slot_kind = h->dkind;
    C.logCap = h->logCap;
    C.kindCap = h->kindCap;
    volatile int *flags = h->h_flags;
    flags[0] = 0;
    flags[1] = 0;
    // blind up to a little before last step's slot count, then two slots ahead of the posted progress
    C.notifyFrom = std::max(0, std::min(h->prevSlots - 3, h->prevSlots * 3 / 4));  // a shorter step wastes few slots
    if (h->dist) C.notifyFrom = 1 << 30;   // deterministic batches: nobody reads the progress (a host store costs ~18 us)
    *notifyFrom = C.notifyFrom;
    HIPCHECK(h, hipMemcpyAsync(h->ctl, h->h_ctl, sizeof(DevLoop), hipMemcpyHostToDevice, h->st));
    return 0;
}

// start of a step on the sharded element pass: the summed gradient and energy, |g|^2, the start-of-step controller and, in
// the early order, the first direction's solve
static int step_start_sharded(dotmi_handle *h, int nb)
{
    const int n = h->n;
    const double *ctlR = h->partR;
    if (!h->owner) {
        stage_energy(h, nb, h->gstage + n + 1);
        if (int rc = allreduce_sum(h, h->gstage, (size_t)n + 2)) return rc;
    } else {
        // |g|^2 over the owned vertices no other rank holds rides with the packet, the shared entries' squares are
        // added from the summed packet
        launch_masked_norm2(n, h->gstage, h->vkind, h->partR, h->st, 1);
        if (int rc = exchange_gradient_packed(h, n, nb, h->partR, 1)) return rc;
        ctlR = h->partGR;
    }
    HIPCHECK(h, hipMemcpyAsync(h->g, h->gstage, sizeof(double) * n, hipMemcpyDeviceToDevice, h->st));
    if (!h->owner) {
        const double *vecs[1] = {h->g};
        launch_multidot(n, h->g, vecs, 1, h->partR, h->st);   // |g|^2
    }
    if (!h->earlyNow) {
        launch_loop_control(h->ctl, h->gstage + n, 1, ctlR, h->alpha_dev, h->h_flags, h->st, 1);
        return 0;
    }
    // early order on the sharded element pass: -g_0 (the summed gradient) into this rank's right-hand sides, the
    // first direction's solve with the start-of-step controller inside its launch, the sum over the ranks, z = u
    launch_build_qpad(h->P, h->g, NO_HISTORY, nullptr, h->st, nullptr);
    const CoarseMerge *co = dot_coarse(h);   // (DOTMI_FLAG_DOT_COARSE, never with the owner exchange: as in slot_merge)
    if (co) dot_coarse_restrict(h, h->zstage + n);
    CtlLaunch ca{{h->ctl, h->gstage + n, ctlR, h->alpha_dev, h->h_flags, 1, 1}, CTL_PLAIN};
    launch_gemv(h->P, nullptr, h->st, h->ctl, nullptr, nullptr, &ca, 1 << 30);
    if (!h->owner) return merge_over_ranks(h, NO_HISTORY, h->zstage, RANKSUM_EARLY_FIRST, h->ctl, h->held());
    launch_merge(h->M, h->P, NO_HISTORY, {.z = h->zstage, .vl = h->held()}, h->st, h->ctl);
    if (int rc = exchange_iface(h, h->zstage, nullptr, 0)) return rc;
    // (no pair yet: no y_i . z to sum, no partials)
    launch_merge_early(h->M, h->P, {.z = h->z, .first = 1, .zsum = h->zstage, .ownMask = h->ownMask, .vl = h->held(), .wide = h->tune.wideForms}, h->st, h->ctl);
    HIPCHECK(h, hipMemsetAsync(h->partGC, 0, sizeof(double) * HIST_MAX, h->st));
    return 0;
}

// energy and gradient at the start of the step, reduced by the controller (no host round trip), and in the early order the
// first direction's solve
static int enqueue_step_start(dotmi_handle *h)
{
    int nb = h->VP.nPatches;
    if (h->vpNow) {
        // energy, gradient, |g|^2 and -g_0 in the padded right-hand sides from the one launch (no step, no pair: ctl == nullptr)
        ElemVertArgs ea = elem_vertex_args(h);
        ea.x0 = h->x;
        ea.g0 = h->g;
        launch_elem_vertex(h->VP, h->mat, ea, h->st, nullptr);
    } else {
        const StepElemPass e = step_elem_pass(h, h->x, 1);
        nb = launch_elem_pass(e.M, h->stepPT(), h->mat, h->dtSq, e.a, h->st);
    }
    GatherArgs a = gather_args(h);
    a.x = h->x;
    a.g_new = h->shardElems ? h->gstage : h->g;
    a.make_pair = 0;
    a.ownMask = h->owner ? h->ownMask : nullptr;
    a.vlist = h->owner ? h->heldList : nullptr;
    a.nlist = h->owner ? h->nHeld : 0;
    // owner exchange: the loop only touches the held vertices' entries; the trial buffer starts as a copy of the iterate
    // (the two swap roles on every accepted trial and must agree off the held set)
    if (h->owner) HIPCHECK(h, hipMemcpyAsync(h->x_trial, h->x, sizeof(double) * h->n, hipMemcpyDeviceToDevice, h->st));
    if (h->earlyNow && !h->shardElems) {   // -g_0 straight into the padded right-hand sides (their padding entries stay zero)
        a.vp_ptr = h->P.vp_ptr;
        a.vp_off = h->P.vp_off;
        a.rpad = h->P.rpad;
    }
    if (!h->vpNow) launch_vertex_gather(h->M, h->stepPT(), a, NO_HISTORY, h->partR, h->st);
    if (h->shardElems) return step_start_sharded(h, nb);
    if (!h->earlyNow) {
        launch_loop_control(h->ctl, h->partE, nb, h->partR, h->alpha_dev, h->h_flags, h->st, 1);
        return 0;
    }
    // the first direction's solve, u = -M g_0 and z = u, with the start-of-step controller inside its launch
    // (dotmi_set_dot_coarse: y = A0^-1 Z^T (-g_0) for the merge below; sharded subdomains: the restriction into the packet's tail)
    const CoarseMerge *co = dot_coarse(h);
    if (co && h->dist) dot_coarse_restrict(h, h->zstage + h->n);
    else if (co) dot_coarse_restrict_solve(h);
    // (no trial to judge yet: the plain controller, which only differs in how many rows of statistics there are)
    CtlLaunch ca{{h->ctl, h->partE, h->partR, h->alpha_dev, h->h_flags, nb, 1}, h->vpNow ? CTL_VP : CTL_PLAIN};
    launch_gemv(h->P, nullptr, h->st, h->ctl, nullptr, nullptr, &ca, 1 << 30);
    if (h->dist) return merge_over_ranks(h, NO_HISTORY, h->zstage, RANKSUM_EARLY_FIRST, h->ctl);
    launch_merge_early(h->M, h->P, {.z = h->z, .partials = h->partC, .partialsT = h->partCT, .first = 1, .co = co, .wide = h->tune.wideForms}, h->st, h->ctl);
    return 0;
}

// one rank: keep the queue AHEAD slots in front of the progress the controller posts to pinned memory (blind up to notifyFrom)
static int follow_progress(dotmi_handle *h, int notifyFrom, int *enq)
{
    const int AHEAD = 2;
    volatile int *flags = h->h_flags;
    const double tStart = now_ms();
    long spins = 0;
    while (flags[0] == 0) {
        if (*enq < std::max(notifyFrom, (int)flags[1]) + AHEAD) {
            if (int rc = enqueue_loop_slot(h)) return rc;
            ++*enq;
        } else if ((++spins & 0xfffff) == 0) {
            if (hipStreamQuery(h->st) != hipErrorNotReady && flags[0] == 0) {
                // the queue drained without the controller reporting progress: a kernel failed
                HIPCHECK(h, hipStreamSynchronize(h->st));
                HIPCHECK(h, hipGetLastError());
                if (flags[0] == 0 && *enq >= std::max(notifyFrom, (int)flags[1]) + AHEAD) {
                    h->err = "device loop made no progress";
                    return DOTMI_E_DEVICE;
                }
            }
            if (now_ms() - tStart > 600000.0) {
                h->err = "device loop timed out";
                return DOTMI_E_DEVICE;
            }
        }
    }
    return 0;
}

// Sharded subdomains: every slot carries a collective, so every rank must enqueue the SAME number of slots.
// Deterministic batches instead of following the posted progress: one slot more than the last step used, then
// (rarely) short batches; after a batch the ranks check against rank 0 that they stopped in the same state.
static int enqueue_batches(dotmi_handle *h, int *enq)
{
    const DevLoop &C = *h->h_ctl;
    const double tStart = now_ms();
    int target = std::max(h->prevSlots + 1, 4);
    for (;;) {
        while (*enq < target) {
            if (int rc = enqueue_loop_slot(h)) return rc;
            ++*enq;
        }
        HIPCHECK(h, hipMemcpyAsync(h->h_ctl, h->ctl, sizeof(DevLoop), hipMemcpyDeviceToHost, h->st));
        HIPCHECK(h, hipStreamSynchronize(h->st));
        HIPCHECK(h, hipGetLastError());
        // Every rank contributes v = (status, slots, iterations, halvings), its squares and a local error flag to ONE
        // sum all-reduce.  All ranks see the same sums, so the verdict is a function of reduced data only and they
        // fail together instead of one of them waiting in the next collective: the ranks agree exactly when the
        // variance vanishes, world * sum(v^2) == (sum v)^2 (small integers, exact in FP64) -- the earlier test
        // `sum == world * mine` could pass on one rank and fail on the others for world >= 3.
        double mine[4] = {(double)C.status, (double)C.slots, (double)C.iter, (double)C.halvings}, red[9];
#ifdef DOTMI_TEST_HOOKS
        mine[2] += (double)h->testIterDelta;   // this process reports a different iteration count
#endif
        for (int i = 0; i < 4; ++i) {
            red[i] = mine[i];
            red[4 + i] = mine[i] * mine[i];
        }
        red[8] = 0.0;   // local error flag (set by a rank that cannot go on; summed like the rest)
        if (h->world > 1) {
            HIPCHECK(h, hipMemcpyAsync(h->ctrlDev, red, sizeof(red), hipMemcpyHostToDevice, h->st));
            if (int rc = allreduce_sum(h, h->ctrlDev, 9)) return rc;
            HIPCHECK(h, hipMemcpyAsync(red, h->ctrlDev, sizeof(red), hipMemcpyDeviceToHost, h->st));
            HIPCHECK(h, hipStreamSynchronize(h->st));
        }
        const double w = h->world > 1 ? (double)h->world : 1.0;
        bool agree = red[8] == 0.0;
        for (int i = 0; i < 4; ++i) agree = agree && w * red[4 + i] == red[i] * red[i];
        if (!agree) {
            h->err = "the ranks left the L-BFGS loop in different states (this rank: status " + std::to_string(C.status) +
                     " after " + std::to_string(C.slots) + " slots, " + std::to_string(C.iter) + " iterations; sum over " +
                     std::to_string(h->world) + " ranks: " + std::to_string((long long)red[0]) + " / " +
                     std::to_string((long long)red[1]) + " / " + std::to_string((long long)red[2]) + ")";
            h->poisoned = true;
            return DOTMI_E_DEVICE;
        }
        if (C.status != 0) return 0;
        target = *enq + std::max(2, std::min(8, *enq / 4));
        if (now_ms() - tStart > 600000.0) {
            h->err = "device loop timed out";
            return DOTMI_E_DEVICE;
        }
    }
}

// the finished loop's state back into the handle and the step's result
static int harvest_devloop(dotmi_handle *h, int enq, LoopOut &r)
{
    const DevLoop &C = *h->h_ctl;
    HIPCHECK(h, hipMemcpyAsync(h->h_ctl, h->ctl, sizeof(DevLoop), hipMemcpyDeviceToHost, h->st));
    HIPCHECK(h, hipStreamSynchronize(h->st));
    r.it = C.iter;
    h->prevSlots = C.slots;
    h->prevIters = C.iter;
    h->prevHalv = C.halvings;
    memcpy(h->predState, C.predHist, sizeof(int) * 2);
    memcpy(h->predState + 2, &C.predCtr[0][0], sizeof(int) * 8);
    memcpy(h->pairState, C.pairCtr, sizeof(int) * 3);
    h->heldSlots = C.heldSlots;
    h->heldRejected = C.heldRejected;
    h->pairSlots = C.pairSlots;
    h->pairRedo = C.pairRedo;
    h->specSlots = C.specSlots;
    h->specRedo = C.specRedo;
    h->prevFirst = C.firstTrials;
    h->prevUnit = C.unitFirst;
    if (h->tune.fuseLog && C.pairSlots)
        fprintf(stderr, "dotmi: paired trials: %d slots, %d of them redone (the full step was acceptable)\n", C.pairSlots, C.pairRedo);
    r.failed = C.status == 3;
    r.lastE = C.E_cur;
    r.g2 = C.g2_cur;
    r.E0 = C.E0;
    r.g20 = C.g2_0;
    h->x = C.x_cur;
    h->x_trial = C.x_trial;
    h->g = C.g_cur;
    h->g_trial = C.g_trial;
    h->numLineSearch += C.halvings;
    h->energy_evals += C.evals;
    // the per-iteration log stays on the device until somebody asks for it (dotmi_last_iter_log)
    h->logPending = std::min(C.iter, h->logCap);
    // which of the enqueued slots really ran a back-solve (for DOTMI_FLAG_TIME_BACKSOLVE)
    h->slotKind.assign(enq, 0);
    const int nk = std::min(std::min(C.slots, enq), h->kindCap);
    if (nk > 0 && (h->flags & DOTMI_FLAG_TIME_BACKSOLVE))
        HIPCHECK(h, hipMemcpy(h->slotKind.data(), h->dkind, sizeof(int) * nk, hipMemcpyDeviceToHost));
    if (h->earlyNow && (h->flags & DOTMI_FLAG_TIME_BACKSOLVE)) {
        // early order: slot sl's back-solve ran to its end iff its trial was accepted and the loop went on, i.e. iff slot
        // sl + 1 computed a new direction (kind 1); the others were told to stop and do not count as timed launches
        for (int sl = 0; sl < nk; ++sl) h->slotKind[sl] = (sl + 1 < nk && h->slotKind[sl + 1] == 1) ? 1 : 0;
    }
    return 0;
}

// The L-BFGS loop of one time step with the control flow on the device (DevLoop).  The host only keeps
// the queue a few slots ahead of the controller's progress, which it reads from pinned memory.
int run_device_loop(dotmi_handle *h, LoopOut &r)
{
    choose_step_forms(h);
    int notifyFrom = 0, enq = 0;
    if (int rc = init_devloop(h, &notifyFrom)) return rc;
    if (int rc = enqueue_step_start(h)) return rc;
    if (int rc = h->dist ? enqueue_batches(h, &enq) : follow_progress(h, notifyFrom, &enq)) return rc;
    return harvest_devloop(h, enq, r);
}

}  // namespace dotmi
