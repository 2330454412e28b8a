// dotmi_coarse.hip -- the rigid-mode coarse space of Newton-PCG's preconditioner (dotmi_set_pcg_coarse; kernels k_coarse.hip, lists
// coarse_plan.hpp).  One-level additive Schwarz carries information across one subdomain per CG iteration; the
// additive coarse term  M = M_sym + Z A0^-1 Z^T,  A0 = Z^T H Z  with the subdomains' six rigid-body modes as Z's columns carries the
// smooth part across all of them at once.  Off by default and then absent: no list, no buffer, no launch.  With the mode on, every
// refresh of H (refactor_issue) marks A0 stale and the next solve rebuilds it from the handle's current iterate: centroids, the pairs'
// 6 x 6 blocks, the dense fill, and X = chol(A0)^-1 by the tile kernels of the block solve on a schedule of their own for this one
// dense block (as LBFGS-PD factors its Laplacian); the host reads back the pivot flag and nothing else.  A factorisation that meets a
// non-positive pivot (rank-deficient Z) switches the term off until the next successful build -- the solves run on M_sym alone and
// the handle is not poisoned.  The reference has no counterpart.
// dotmi_set_dot_coarse puts the same term into DOT's own preconditioner, M' = M + Z A0^-1 Z^T with M = D^-1 sum_s R_s^T H_s^-1 R_s: the
// same lists, Z, A0 and factor (one build serves both modes).  There the build is enqueued behind every refresh of H, at the positions
// the refresh was made at, and its pivot flag is read after the synchronisation the refresh ends in anyway -- no read-back of its own
// in a step.  The restriction reads the padded right-hand sides (coarse_restrict_pad_kernel), the prolongation is part of the merges.
// DOTMI_FLAG_DOT_COARSE puts that term on a sharded handle (world > 1, DOTMI_FLAG_FORCE_DIST).  The plan, Z, the
// weights, the dropped subdomains, the frozen x and the centroids are global and computed on every rank alike (x is replicated there);
// the restriction table covers the rank's own subdomains.  With a replicated Hessian every rank assembles every pair as one GPU does;
// with a sharded one a rank assembles the pairs (s, t), s <= t, whose s it owns -- the block rows of its subdomains' vertices are
// assembled whole, so every H block such a pair names is there --, writes zeros for the others, and one all-reduce of the 36 nPairs
// doubles per refresh makes pairA whole (disjoint contributions: the sum is exact).  Fill and factorisation of the one dense block run
// on every rank.  Per application c = Z^T r rides in the tail of the vector the iteration all-reduces anyway and the solve runs on
// every rank behind that collective (dot_coarse_restrict / dot_coarse_solve).
// Mode 2 (dotmi_set_dot_coarse_mode) is the balanced form  M'' = C + (I - C H) M (I - H C),  C = Z A0^-1 Z^T: the same Z, A0 and factor,
// and W = H Z as a sparse table of 3 x 6 blocks (coarse_hz_setup, coarse_hz_kernel behind the centroids of every build with the mode
// on).  Per application three launches in front of the block solve (dot_coarse_deflate) and two behind the merge, which then leaves its
// division, the prolongation and the y_i . z to the sharded merge's finishing kernel (dot_coarse_balance).  One rank, the q-based order.
#include "coarse_plan.hpp"
#include "dotmi_handle.hpp"

namespace dotmi {

// lists, buffers and the tile schedule, at the first switch-on; kept
static int coarse_setup(dotmi_handle *h)
{
    dotmi_handle::Coarse &K = h->coarse;
    if (K.planned) return 0;
    DevCoarse &D = K.D;
    const int nP = h->nPartsAll, nV = h->nV;
    std::vector<int> adj_ptr, adj_idx;
    build_adjacency(nV, h->nT, h->T.data(), adj_ptr, adj_idx);
    CoarsePlan P;
    coarse_plan(nV, h->nT, h->T.data(), h->epart.data(), nP, adj_ptr, adj_idx, P);
    for (int s = 0; s < nP; ++s)   // the plan's subdomains are the handle's (both from epart)
        if (!std::equal(P.svIdx.begin() + P.svPtr[s], P.svIdx.begin() + P.svPtr[s + 1], h->partVerts[s].begin(), h->partVerts[s].end())) {
            h->err = "dotmi_set_pcg_coarse: the coarse plan's subdomains differ from the handle's";
            return DOTMI_E_INVALID;
        }
    // the padded restriction (dotmi_set_dot_coarse) finds a subdomain's vertices in its padded range: every vertex of every subdomain
    // the handle owns has its three consecutive positions there (place_rows), the subdomains [p0, p1) in their order by local index
    // (one rank: all of them; a sharded handle restricts its own and the ranks' parts of c are summed, DOTMI_FLAG_DOT_COARSE)
    const int nOwn = h->p1 - h->p0;
    if (h->P.nParts != nOwn || (int)h->partPos.size() != nOwn || (!h->dist && nOwn != nP)) {
        h->err = "dotmi_set_pcg_coarse / dotmi_set_dot_coarse: the handle does not own every subdomain";
        return DOTMI_E_INVALID;
    }
    for (int ls = 0; ls < nOwn; ++ls) {
        bool ok = h->partPos[ls].size() == h->partVerts[h->p0 + ls].size();
        for (size_t i = 0; ok && i < h->partPos[ls].size(); ++i) ok = h->partPos[ls][i] >= 0 && h->partPos[ls][i] + 3 <= h->P.nmax;
        if (!ok) {
            h->err = "dotmi_set_dot_coarse: a vertex of subdomain " + std::to_string(h->p0 + ls) + " has no place in the padded right-hand sides";
            return DOTMI_E_INVALID;
        }
    }
    D.nmax = h->P.nmax;
    D.dofmap = h->P.dofmap;
    D.p0 = h->p0;
    D.nOwn = nOwn;
    // who assembles which pair: everything, unless the Hessian refresh is sharded -- then H is whole only on the block rows of the
    // rank's own subdomains' vertices, which is what the pairs (s, t), s <= t, with s its own read
    D.as0 = h->shardHess ? h->p0 : 0;
    D.as1 = h->shardHess ? h->p1 : nP;
    if (int rc = dalloc(h, &D.rtab, (size_t)nOwn * D.nmax)) return rc;
    D.nParts = nP;
    D.nc = 6 * nP;
    D.ncp = (D.nc + TILE - 1) / TILE * TILE;
    D.nPairs = (int)P.pairS.size();
    std::vector<int2> pair(D.nPairs);
    K.pairAt.assign((size_t)nP * nP, -1);
    for (int p = 0; p < D.nPairs; ++p) {
        pair[p] = make_int2(P.pairS[p], P.pairT[p]);
        K.pairAt[(size_t)P.pairS[p] * nP + P.pairT[p]] = p;
    }
    if (P.pairBlk.empty()) P.pairBlk.push_back(0);
    if (int rc = upload(h, &D.vsPtr, P.vsPtr)) return rc;
    if (int rc = upload(h, &D.vsIdx, P.vsIdx)) return rc;
    if (int rc = upload(h, &D.svPtr, P.svPtr)) return rc;
    if (int rc = upload(h, &D.svIdx, P.svIdx)) return rc;
    if (int rc = upload(h, &D.pair, pair)) return rc;
    if (int rc = upload(h, &D.pairPtr, P.pairPtr)) return rc;
    if (int rc = upload(h, &D.pairBlk, P.pairBlk)) return rc;
    if (int rc = upload(h, &D.pairAt, K.pairAt)) return rc;
    if (int rc = dalloc(h, &D.live, (size_t)nP)) return rc;
    if (int rc = dalloc(h, &D.wgt, (size_t)nV)) return rc;
    if (int rc = dalloc(h, &D.xf, (size_t)h->n)) return rc;
    if (int rc = dalloc(h, &D.cen, (size_t)3 * nP)) return rc;
    if (int rc = dalloc(h, &D.pairA, (size_t)36 * D.nPairs)) return rc;
    const size_t wn = (size_t)D.ncp * D.ncp;
    if (int rc = dalloc(h, &D.W, wn)) return rc;
    if (int rc = dalloc(h, &D.W2, wn)) return rc;
    if (int rc = dalloc(h, &D.c, (size_t)D.ncp)) return rc;
    if (int rc = dalloc(h, &D.y, (size_t)(D.ncp / TILE) * D.ncp)) return rc;
    if (int rc = dalloc(h, &D.info, 1)) return rc;
    HIPCHECK(h, hipMemset(D.W, 0, sizeof(double) * wn));   // (the factorisation writes the tiles of X and nothing else, ever)
    HIPCHECK(h, hipMemset(D.c, 0, sizeof(double) * D.ncp));
    HIPCHECK(h, hipMemset(D.y, 0, sizeof(double) * (size_t)(D.ncp / TILE) * D.ncp));
    // the tile schedule of one dense block of nt x nt tiles in plain row-major storage: row block J at 64 J ncp, all columns
    const int nt = D.ncp / TILE;
    std::vector<long long> rtOff(nt);
    std::vector<int> rtLd(nt, D.ncp), rtC0(nt, 0);
    for (int J = 0; J < nt; ++J) rtOff[J] = (long long)J * TILE * D.ncp;
    std::vector<uint8_t> live(nt, 1), pat((size_t)nt * nt, 0);
    for (int I = 0; I < nt; ++I)
        for (int J = I; J < nt; ++J) pat[(size_t)I * nt + J] = 1;
    TileSchedule S;
    {
        std::vector<TileTaskL> all;
        size_t sn = 0;
        plan_subdomain_tiles(0, nt, D.W, rtOff.data(), rtLd.data(), rtC0.data(), live, pat, D.W2, sn, all, S.clearTiles, S.clearLd, S.flops,
                             S.qTiles, 2, 2, 0, true, 1);
        finish_tile_schedule(all, S);
    }
    if (int rc = upload(h, &K.tasks, S.tasks)) return rc;
    if (S.prods.empty()) S.prods.push_back(TileProd{nullptr, nullptr, 0, 0});
    if (int rc = upload(h, &K.prods, S.prods)) return rc;
    K.levelStart = S.levelStart;
    HIPCHECK(h, hipHostMalloc((void **)&K.h_info, sizeof(int)));
    HIPCHECK(h, hipEventCreate(&K.ev0));
    HIPCHECK(h, hipEventCreate(&K.ev1));
    if (h->tune.fuseLog)
        fprintf(stderr, "dotmi: PCG coarse space: %d subdomains, dimension %d (padded %d), %d coupled pairs with %d entries, %zu tile tasks "
                "in %zu levels\n", nP, D.nc, D.ncp, D.nPairs, P.pairPtr.back(), S.tasks.size(), S.levelStart.size() - 1);
    K.cm = CoarseMerge{D.vsPtr, D.vsIdx, D.wgt, D.xf, D.cen, D.y, D.nc, D.ncp};
    K.planned = true;
    return 0;
}

// mode 2: the lists of W = H Z and its buffers, at the first switch to mode 2; kept
static int coarse_hz_setup(dotmi_handle *h)
{
    dotmi_handle::Coarse &K = h->coarse;
    if (K.hzPlanned) return 0;
    DevCoarse &D = K.D;
    const int nP = h->nPartsAll, nV = h->nV;
    std::vector<int> adj_ptr, adj_idx;
    build_adjacency(nV, h->nT, h->T.data(), adj_ptr, adj_idx);
    CoarsePlan P;
    coarse_plan(nV, h->nT, h->T.data(), h->epart.data(), nP, adj_ptr, adj_idx, P);
    CoarseHzPlan Z;
    coarse_hz_plan(nV, nP, P.vsPtr, P.vsIdx, adj_ptr, adj_idx, Z);
    D.nHz = (int)Z.hzSub.size();
    if (Z.hzSub.empty()) {   // (no vertex in any subdomain: the launches over the entries are skipped, the lists stay addressable)
        Z.hzSub.push_back(0);
        Z.hzVert.push_back(0);
        Z.hzTEnt.push_back(0);
    }
    if (Z.hzBlk.empty()) Z.hzBlk.push_back(0);
    if (int rc = upload(h, &D.hzPtr, Z.hzPtr)) return rc;
    if (int rc = upload(h, &D.hzSub, Z.hzSub)) return rc;
    if (int rc = upload(h, &D.hzVert, Z.hzVert)) return rc;
    if (int rc = upload(h, &D.hzBlkPtr, Z.hzBlkPtr)) return rc;
    if (int rc = upload(h, &D.hzBlk, Z.hzBlk)) return rc;
    if (int rc = upload(h, &D.hzTPtr, Z.hzTPtr)) return rc;
    if (int rc = upload(h, &D.hzTEnt, Z.hzTEnt)) return rc;
    if (int rc = dalloc(h, &D.hz, (size_t)18 * std::max(D.nHz, 1))) return rc;
    if (int rc = dalloc(h, &D.cd, (size_t)D.ncp)) return rc;
    if (int rc = dalloc(h, &D.r1, (size_t)h->n)) return rc;
    HIPCHECK(h, hipMemset(D.hz, 0, sizeof(double) * 18 * std::max(D.nHz, 1)));
    HIPCHECK(h, hipMemset(D.cd, 0, sizeof(double) * D.ncp));
    if (h->tune.fuseLog)
        fprintf(stderr, "dotmi: balanced coarse term: W = H Z in %d blocks of 3 x 6 over %zu H blocks\n", D.nHz, Z.hzBlk.size());
    K.hzPlanned = true;
    return 0;
}

int coarse_issue(dotmi_handle *h, const double *x)
{
    dotmi_handle::Coarse &K = h->coarse;
    if (int rc = coarse_setup(h)) return rc;
    if (K.dotMode == 2)
        if (int rc = coarse_hz_setup(h)) return rc;
    DevCoarse &D = K.D;
    // weights and dropped subdomains from the handle's current fixed set (dotmi_refix changes it); uploaded when they change
    std::vector<double> wgt(h->nV);
    std::vector<int> live(D.nParts, 0);
    for (int v = 0; v < h->nV; ++v) wgt[v] = h->fixed[v] ? 0.0 : 1.0 / (double)std::max(h->dup[v], 1);
    K.dropped = 0;
    for (int s = 0; s < D.nParts; ++s) {
        int nfree = 0;
        for (int v : h->partVerts[s]) nfree += h->fixed[v] ? 0 : 1;
        live[s] = nfree >= 3;
        K.dropped += nfree < 3;
    }
    if (!K.uploaded || wgt != K.wgt || live != K.live) {
        K.wgt.swap(wgt);
        K.live.swap(live);
        HIPCHECK(h, hipMemcpyAsync(D.wgt, K.wgt.data(), sizeof(double) * h->nV, hipMemcpyHostToDevice, h->st));
        HIPCHECK(h, hipMemcpyAsync(D.live, K.live.data(), sizeof(int) * D.nParts, hipMemcpyHostToDevice, h->st));
        K.uploaded = true;
    }
    HIPCHECK(h, hipEventRecord(K.ev0, h->st));
    HIPCHECK(h, hipMemcpyAsync(D.xf, x, sizeof(double) * h->n, hipMemcpyDeviceToDevice, h->st));   // frozen with this build
    launch_coarse_centroid(D, h->st);
    K.hzIssued = K.dotMode == 2;
    if (K.hzIssued) launch_coarse_hz(D, h->M, h->Hval, h->st);   // W = H Z of this H, Z and these centroids (mode 2 only)
    launch_coarse_rtab(D, h->st);
    launch_coarse_assemble(D, h->M, h->Hval, h->st);
    // sharded Hessian refresh: every pair's block was assembled by exactly one rank, the owner of s, and is zero elsewhere
    if (h->shardHess)
        if (int rc = allreduce_sum(h, D.pairA, (size_t)36 * D.nPairs)) return rc;
    // from here on every rank holds the same pairA, live flags and padding: the fill, the factorisation and with them the pivot flag
    // are functions of identical data, so a non-positive pivot leaves the term inactive on ALL ranks alike -- no agreement collective
    launch_coarse_fill(D, h->st);
    HIPCHECK(h, hipMemsetAsync(D.info, 0, sizeof(int), h->st));
    for (size_t l = 0; l + 1 < K.levelStart.size(); ++l)   // one launch per level of the block's own schedule
        launch_tile_level(K.tasks + K.levelStart[l], K.levelStart[l + 1] - K.levelStart[l], K.prods, D.info, h->st, h->fastDiag);
    HIPCHECK(h, hipEventRecord(K.ev1, h->st));
    HIPCHECK(h, hipMemcpyAsync(K.h_info, D.info, sizeof(int), hipMemcpyDeviceToHost, h->st));
    K.pending = true;
    return 0;
}

void coarse_finish(dotmi_handle *h)
{
    dotmi_handle::Coarse &K = h->coarse;
    if (!K.pending) return;
    K.pending = false;
    float ms = 0.f;
    hipEventElapsedTime(&ms, K.ev0, K.ev1);
    K.lastBuildMs = ms;
    K.stale = false;
    K.hzBuilt = K.hzIssued;
    K.builds++;
    K.active = K.h_info[0] == 0;   // a non-positive pivot: Z is rank deficient -- the applications go on without the coarse term
    if (h->tune.fuseLog)
        fprintf(stderr, "dotmi: coarse build %lld: %.3f ms, %d dropped, %s\n", K.builds, K.lastBuildMs, K.dropped,
                K.active ? "active" : "inactive (pivot)");
}

int coarse_refresh(dotmi_handle *h)
{
    dotmi_handle::Coarse &K = h->coarse;
    if ((K.mode == 0 && K.dotMode == 0) || !K.stale) return 0;
    if (int rc = coarse_issue(h, h->x)) return rc;
    HIPCHECK(h, hipStreamSynchronize(h->st));
    HIPCHECK(h, hipGetLastError());
    coarse_finish(h);
    return 0;
}

void dot_coarse_restrict(dotmi_handle *h, double *c, const DevLoop *ctl, int spec)
{
    launch_coarse_restrict_pad(h->coarse.D, h->P.rpad, h->st, ctl, spec, c);
}

void dot_coarse_solve(dotmi_handle *h, const double *c, const DevLoop *ctl, int spec)
{
    const DevCoarse &D = h->coarse.D;
    if (ctl) launch_coarse_solve_loop(D, h->st, ctl, spec, c);
    else launch_coarse_solve(D, h->st, c);
}

void dot_coarse_restrict_solve(dotmi_handle *h, const DevLoop *ctl, int spec)
{
    dot_coarse_restrict(h, nullptr, ctl, spec);
    dot_coarse_solve(h, nullptr, ctl, spec);
}

const double *dot_coarse_deflate(dotmi_handle *h, const double *q, const DevLoop *ctl)
{
    const DevCoarse &D = h->coarse.D;
    if (ctl) launch_coarse_restrict_loop(D, q, h->st, ctl);   // c1 = Z^T q
    else launch_coarse_restrict(D, q, h->st);
    dot_coarse_solve(h, nullptr, ctl, 0);                      // y1 = A0^-1 c1
    launch_coarse_deflate(D, h->n, q, D.r1, h->st, ctl);       // r1 = q - W y1
    return D.r1;
}

void dot_coarse_balance(dotmi_handle *h, double *z, const LbfgsArgs &L, const DevLoop *ctl)
{
    const DevCoarse &D = h->coarse.D;
    launch_coarse_restrict_hz(D, h->P.dup, z, h->st, ctl);     // cd = c1 - W^T u, u = z / dup
    dot_coarse_solve(h, D.cd, ctl, 0);                         // y1 - y2 = A0^-1 cd
    launch_zfinish(h->nV, h->P.dup, L, z, h->partC, h->st, ctl, &h->coarse.cm);   // z = u + Z (y1 - y2), the y_i . z
}

void coarse_restrict_solve(dotmi_handle *h, const double *r)
{
    launch_coarse_restrict(h->coarse.D, r, h->st);
    launch_coarse_solve(h->coarse.D, h->st);
}

void coarse_prolong(dotmi_handle *h, double *zsum) { launch_coarse_prolong(h->coarse.D, h->nV, h->pcg.isd, zsum, h->st); }

}  // namespace dotmi

extern "C" {

int dotmi_set_pcg_coarse(dotmi_handle *h, int32_t mode)
{
    if (!h) return DOTMI_E_INVALID;
    const char *why = pcg_refusal(h);
    if (!why && h->dist) why = "single-rank handles only (the subdomains of this one are sharded: its PCG has no coarse space)";
    if (!why && !h->vpart.empty()) why = "the subdomains of this handle are vertex sets (vpart), the coarse plan works on an element partition";
    if (why) {
        h->err = std::string("dotmi_set_pcg_coarse: ") + why;
        return DOTMI_E_INVALID;
    }
    if (mode != 0 && mode != 1) {
        h->err = "dotmi_set_pcg_coarse: mode must be 0 (off) or 1 (rigid modes)";
        return DOTMI_E_INVALID;
    }
    if (mode == 1 && h->nPartsAll > COARSE_MAX_PARTS) {
        h->err = "dotmi_set_pcg_coarse: at most " + std::to_string(COARSE_MAX_PARTS) + " subdomains (the coarse matrix is applied through a dense "
                 "inverse factor); this handle has " + std::to_string(h->nPartsAll);
        return DOTMI_E_INVALID;
    }
    if (mode == 1 && h->coarse.mode == 0 && h->coarse.dotMode == 0) h->coarse.stale = true;   // (whatever happened to H while the mode was off)
    h->coarse.mode = mode;
    return 0;
}

// the two setters of DOT's coarse term: dotmi_set_dot_coarse takes 0 and 1 as it always has (a caller that passes anything else is told
// so, as before); dotmi_set_dot_coarse_mode takes 0, 1 and 2 -- 2 the balanced form.  One handle state, one set of refusals, one stale /
// rebuild rule behind both
static int set_dot_coarse_mode(dotmi_handle *h, int32_t mode, bool balanced)
{
    const std::string entry = balanced ? "dotmi_set_dot_coarse_mode: " : "dotmi_set_dot_coarse: ";
    const char *why = (h->world > 1 || h->dist) ? "single-rank handles only (the subdomains of this one are sharded)"
                      : h->owner                ? "not with the owner exchange"
                      : h->gsdd                 ? "a GSDD handle solves one subdomain at a time"
                      : h->newtonPcg            ? "a Newton-PCG handle takes its coarse term through dotmi_set_pcg_coarse"
                      : h->newton               ? "a Newton handle factorises H as one subdomain"
                      : h->pd                   ? "an LBFGS-PD handle has no Hessian block solve"
                      : h->hi                   ? "an LBFGS-HI handle has no Hessian block solve"
                      : (h->flags & DOTMI_FLAG_ASYNC_REFRESH) ? "not with DOTMI_FLAG_ASYNC_REFRESH (the build is judged with the refresh)"
                      : !h->vpart.empty() ? "the subdomains of this handle are vertex sets (vpart), the coarse plan works on an element partition"
                                          : nullptr;
    if (why) {
        h->err = entry + why;
        return DOTMI_E_INVALID;
    }
    if (mode != 0 && mode != 1 && !(balanced && mode == 2)) {
        h->err = entry + (balanced ? "mode must be 0 (off), 1 (rigid modes, additive) or 2 (rigid modes, balanced)"
                                   : "mode must be 0 (off) or 1 (rigid modes)");
        return DOTMI_E_INVALID;
    }
    if (mode != 0 && h->nPartsAll > COARSE_MAX_PARTS) {
        h->err = entry + "at most " + std::to_string(COARSE_MAX_PARTS) + " subdomains (the coarse matrix is applied through a dense "
                 "inverse factor); this handle has " + std::to_string(h->nPartsAll);
        return DOTMI_E_INVALID;
    }
    const int prev = h->coarse.dotMode;
    if (mode == prev) return 0;
    h->coarse.dotMode = mode;
    if (mode == 0) return 0;
    // the refreshes of H that ran while the mode was off built nothing: build now, from the H and the positions of the last one
    // (mode 2 after a build that ran without it: that build left no W = H Z -- it is rebuilt with A0; 2 -> 1 keeps the build)
    if (mode == 2 && !h->coarse.hzBuilt) h->coarse.stale = true;
    HIPCHECK(h, hipSetDevice(h->device));
    if (int rc = enter_with_factors(h)) {
        h->coarse.dotMode = prev;
        return rc;
    }
    if (int rc = coarse_refresh(h)) {
        h->coarse.dotMode = prev;
        return rc;
    }
    return 0;
}

int dotmi_set_dot_coarse(dotmi_handle *h, int32_t mode) { return h ? set_dot_coarse_mode(h, mode, false) : DOTMI_E_INVALID; }

int dotmi_set_dot_coarse_mode(dotmi_handle *h, int32_t mode) { return h ? set_dot_coarse_mode(h, mode, true) : DOTMI_E_INVALID; }

int32_t dotmi_dot_coarse_mode(const dotmi_handle *h) { return h ? h->coarse.dotMode : 0; }

int dotmi_dot_coarse_info(const dotmi_handle *h, int32_t *dim, int32_t *dropped_subdomains, int32_t *active, int64_t *builds,
                          double *last_build_ms)
{
    if (!h) return DOTMI_E_INVALID;
    const dotmi_handle::Coarse &K = h->coarse;
    if (dim) *dim = K.dotMode ? 6 * h->nPartsAll : 0;
    if (dropped_subdomains) *dropped_subdomains = K.dotMode ? K.dropped : 0;
    if (active) *active = dot_coarse(h) != nullptr || dot_coarse_balanced(h) != nullptr;
    if (builds) *builds = K.builds;
    if (last_build_ms) *last_build_ms = K.lastBuildMs;
    return 0;
}

int dotmi_pcg_coarse_info(const dotmi_handle *h, int32_t *dim, int32_t *dropped_subdomains, int32_t *active, int64_t *builds)
{
    if (!h) return DOTMI_E_INVALID;
    const dotmi_handle::Coarse &K = h->coarse;
    if (dim) *dim = K.mode ? 6 * h->nPartsAll : 0;
    if (dropped_subdomains) *dropped_subdomains = K.dropped;
    if (active) *active = K.mode != 0 && K.active;
    if (builds) *builds = K.builds;
    return 0;
}

int dotmi_pcg_coarse_matrix(dotmi_handle *h, int32_t cap, double *A0)
{
    if (!h) return DOTMI_E_INVALID;
    dotmi_handle::Coarse &K = h->coarse;
    if (K.builds == 0) {
        h->err = "dotmi_pcg_coarse_matrix: no coarse matrix has been assembled on this handle";
        return DOTMI_E_INVALID;
    }
    const int nc = K.D.nc;
    if (!A0) return nc;
    if ((long long)cap < (long long)nc * nc) {
        h->err = "dotmi_pcg_coarse_matrix: room for " + std::to_string((long long)nc * nc) + " doubles is needed";
        return DOTMI_E_INVALID;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    std::vector<double> pairA((size_t)36 * K.D.nPairs);
    HIPCHECK(h, hipMemcpyAsync(pairA.data(), K.D.pairA, sizeof(double) * pairA.size(), hipMemcpyDeviceToHost, h->st));
    HIPCHECK(h, hipStreamSynchronize(h->st));
    coarse_dense_host(nc, K.D.nParts, K.pairAt.data(), K.live.data(), pairA.data(), A0);
    return nc;
}

int dotmi_pcg_apply_precond(dotmi_handle *h, const double *r, double *w)
{
    if (!h) return DOTMI_E_INVALID;
    if (!r || !w) {
        h->err = "dotmi_pcg_apply_precond: r and w must be given";
        return DOTMI_E_INVALID;
    }
    const char *why = pcg_refusal(h);
    if (!why && h->dist) why = "single-rank handles only (the subdomains of this one are sharded)";
    if (why) {
        h->err = std::string("dotmi_pcg_apply_precond: ") + why;
        return DOTMI_E_INVALID;
    }
    HIPCHECK(h, hipSetDevice(h->device));
    if (int rc = enter_with_factors(h)) return rc;
    if (int rc = coarse_refresh(h)) return rc;
    const bool coarse = h->coarse.mode != 0 && h->coarse.active;
    HIPCHECK(h, hipMemcpyAsync(h->tmpn, r, sizeof(double) * h->n, hipMemcpyHostToDevice, h->st));
    launch_coarse_scale(h->n, h->tmpn, h->pcg.isd, h->q, h->st);          // q = r (.) isd
    const Bracket br = backsolve_bracket(h);
    if (coarse) coarse_restrict_solve(h, h->tmpn);
    launch_gemv(h->P, h->q, h->st, nullptr, br.ev0, br.ev1);
    launch_merge(h->M, h->P, NO_HISTORY, {.z = h->z}, h->st);             // zsum = S q
    if (coarse) coarse_prolong(h, h->z);
    launch_coarse_scale(h->n, h->z, h->pcg.isd, h->tmpn, h->st);          // w = zsum (.) isd, as pcg_spmv_kernel forms it
    HIPCHECK(h, hipMemcpyAsync(w, h->tmpn, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->st));
    HIPCHECK(h, hipStreamSynchronize(h->st));
    HIPCHECK(h, hipGetLastError());
    return 0;
}

}  // extern "C"
