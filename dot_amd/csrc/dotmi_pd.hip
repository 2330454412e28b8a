// dotmi_pd.hip -- LBFGS-PD (DOTMI_FLAG_LBFGS_PD; `timeStepper LBFGS`, LBFGSTimeStepper with D0T_PD, src/main.cpp:918-919): L-BFGS
// whose initial inverse Hessian is the constant projective-dynamics Laplacian L = M + sum_e w_e D_e^T D_e, w_e = dt^2 vol_e (2 mu_e +
// lambda_e), fixed rows / columns replaced by the identity (LBFGSTimeStepper.cpp:113-194).  L is a scalar nV x nV matrix applied to
// the three coordinate columns separately (Optimizer::dimSeparatedSolve, Optimizer.cpp:884-957), so it gets a layout of its own:
// the nested dissection of the whole vertex graph with ONE unknown per vertex, its explicit inverse factor X (L^-1 = X^T X) from the
// tile kernels of the block solve (k_tilefactor.hip), built once per create / refix -- a PD step refreshes nothing.
#include "dotmi_handle.hpp"
#include "pd_plan.hpp"

namespace dotmi {

// the scalar layout, its factor storage, the fill list, the tile schedule and the apply's work items (once per create)
int build_pd(dotmi_handle *h, const std::vector<int> &adj_ptr, const std::vector<int> &adj_idx)
{
    const int nV = h->nV, nT = h->nT;
    DevPD &D = h->PD;
    PdPlan P;
    pd_plan(nV, adj_ptr, adj_idx, h->Xrest.data(), P);
    D.nmax = P.nmax;
    h->wTotal = P.wTotal;
    h->precond_bytes = 8 * P.readElems;
    {
        size_t freeB = 0, totalB = 0;
        HIPCHECK(h, hipMemGetInfo(&freeB, &totalB));
        if (8.0 * (double)P.wTotal * 2.1 > 0.9 * (double)freeB) {
            h->err = "LBFGS-PD: the scalar factor needs more than the free HBM";
            return DOTMI_E_INVALID;
        }
    }
    if (int rc = dalloc(h, &D.W, std::max<size_t>(P.wTotal, 64))) return rc;
    if (int rc = dalloc(h, &h->W2, std::max<size_t>(P.wTotal, 64))) return rc;
    HIPCHECK(h, hipMemset(D.W, 0, sizeof(double) * std::max<size_t>(P.wTotal, 64)));
    if (int rc = upload(h, &D.rt, P.rt)) return rc;
    if (int rc = upload(h, &D.cvert, P.cvert)) return rc;
    // incident (element, corner) lists, ascending element
    {
        std::vector<int> ip(nV + 1, 0), inc((size_t)4 * nT);
        for (int e = 0; e < nT; ++e)
            for (int a = 0; a < 4; ++a) ip[h->T[4 * e + a] + 1]++;
        for (int v = 0; v < nV; ++v) ip[v + 1] += ip[v];
        std::vector<int> cur(ip.begin(), ip.end() - 1);
        for (int e = 0; e < nT; ++e)
            for (int a = 0; a < 4; ++a) inc[cur[h->T[4 * e + a]]++] = 4 * e + a;
        if (int rc = upload(h, &D.inc_ptr, ip)) return rc;
        if (int rc = upload(h, &D.inc, inc)) return rc;
    }
    if (int rc = dalloc(h, &D.Lval, (size_t)adj_ptr[nV])) return rc;
    // fill list: CSR entry (v, u) -> memory row pos[v], column pos[u] (stored iff left of the row block's end)
    const int ntl = P.nmax / 64;
    auto waddr = [&](int r, int c) -> long long {
        const RowTile &R = P.rt[r >> 6];
        if (R.off < 0 || c < R.c0 || c >= R.c0 + R.ld) return -1;
        return R.off + (long long)(r & 63) * R.ld + (c - R.c0);
    };
    std::vector<long long> fill(adj_ptr[nV]), pad;
    for (int v = 0; v < nV; ++v)
        for (int k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) fill[k] = waddr(P.pos[v], P.pos[adj_idx[k]]);
    for (int r = 0; r < P.nmax; ++r)
        if (P.cvert[r] < 0 && waddr(r, r) >= 0) pad.push_back(waddr(r, r));
    D.npad = (int)pad.size();
    if (int rc = upload(h, &D.fill_dst, fill)) return rc;
    if (int rc = upload(h, &D.pad_dst, pad)) return rc;
    // apply: work items, partials, merge lists
    if (int rc = upload(h, &D.items, P.items)) return rc;
    D.nOne = P.nOne;
    D.nLong = P.nLong;
    if (int rc = dalloc(h, &D.ppart, (size_t)std::max<long long>(P.ppartN, 1))) return rc;
    if (int rc = dalloc(h, &D.tdots, (size_t)std::max(P.nLong, 1) * 64 * 3)) return rc;
    {
        std::vector<std::vector<long long>> lists(nV);
        for (int i = 0; i < (int)P.items.size(); ++i) {
            const PdItem &it = P.items[i];
            for (int c = it.cs; c < it.ce; ++c)
                if (P.cvert[c] >= 0) lists[P.cvert[c]].push_back(it.pbase + 3ll * (c - it.cs));
        }
        std::vector<int> mp(nV + 1, 0);
        std::vector<long long> me;
        for (int v = 0; v < nV; ++v) {
            me.insert(me.end(), lists[v].begin(), lists[v].end());
            mp[v + 1] = (int)me.size();
        }
        if (me.empty()) me.push_back(0);
        if (int rc = upload(h, &D.mptr, mp)) return rc;
        if (int rc = upload(h, &D.ment, me)) return rc;
    }
    // tile schedule of the factorisation (tile_factor.hpp), one "subdomain"
    const int nt = ntl;
    std::vector<uint8_t> live(nt, 0), pat((size_t)nt * nt, 0);
    for (int r = 0; r < P.nmax; ++r)
        if (P.cvert[r] >= 0) live[r / TILE] = 1;
    for (int v = 0; v < nV; ++v)
        for (int k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) {
            const int I = P.pos[adj_idx[k]] / TILE, J = P.pos[v] / TILE;   // column-major element (column pos[u], row pos[v])
            if (I <= J) pat[(size_t)I * nt + J] = 1;
        }
    std::vector<long long> rtOff(nt);
    std::vector<int> rtLd(nt), rtC0(nt);
    for (int J = 0; J < nt; ++J) {
        rtOff[J] = P.rt[J].off;
        rtLd[J] = P.rt[J].ld;
        rtC0[J] = P.rt[J].c0;
    }
    const bool tiny = nt <= 320;
    TileSchedule S;
    {
        std::vector<TileTaskL> all;
        size_t sn = 0;
        plan_subdomain_tiles(0, nt, D.W, rtOff.data(), rtLd.data(), rtC0.data(), live, pat, h->W2, sn, all, S.clearTiles, S.clearLd,
                             S.flops, S.qTiles, tiny ? 2 : 4, tiny ? 2 : 4, 0, true, 1);
        finish_tile_schedule(all, S);
    }
    if (int rc = upload(h, &h->ttasks, S.tasks)) return rc;
    if (int rc = upload(h, &h->tprods, S.prods)) return rc;
    h->tlevelStart = S.levelStart;
    h->tlevelDiag = S.levelDiag;
    h->tileSplit = false;
    h->nTtasks = (int)S.tasks.size();
    h->tileMode = true;
    const size_t nLevels = std::max<size_t>(S.levelStart.size() - 1, 1);
    h->tileFlow = !S.tasks.empty() && (h->tune.tileFlow > 0 || (h->tune.tileFlow < 0 && S.tasks.size() / nLevels <= 512));
    h->fastDiag = h->tune.fastDiag != 0;
    if (h->tileFlow) {
        std::vector<int> depPtr, depIdx;
        build_tile_deps(S.tasks, S.prods, depPtr, depIdx);
        if (depIdx.empty()) depIdx.push_back(0);
        if (int rc = upload(h, &h->tdepPtr, depPtr)) return rc;
        if (int rc = upload(h, &h->tdepIdx, depIdx)) return rc;
        if (int rc = dalloc(h, &h->tdone, S.tasks.size())) return rc;
        if (int rc = dalloc(h, &h->tnext, 2)) return rc;
        HIPCHECK(h, hipMemset(h->tdone, 0, sizeof(int) * S.tasks.size()));
        HIPCHECK(h, hipMemset(h->tnext, 0, sizeof(int) * 2));
        hipDeviceProp_t prop;
        HIPCHECK(h, hipGetDeviceProperties(&prop, h->device));
        h->tileFlowWg = 2 * prop.multiProcessorCount;
    }
    h->tileFlops = S.flops;
    if (h->tune.fuseLog)
        fprintf(stderr, "dotmi: LBFGS-PD: padded size %d, %.1f MB of factor storage, %.1f MB per application (%d one-pass items, %d "
                "two-pass chunks reading %.1f MB twice), %zu tile tasks in %zu levels\n", P.nmax, 8e-6 * P.wTotal, 8e-6 * P.readElems, P.nOne,
                P.nLong, 8e-6 * P.rereadElems,
                S.tasks.size(), nLevels);
    if (int rc = dalloc(h, &h->info_dev, 1)) return rc;
    HIPCHECK(h, hipHostMalloc((void **)&h->h_info, sizeof(int)));
    h->h_info[0] = 0;
    return 0;
}

// L for the handle's current fixed set -> work buffer -> X (create, refix).  The reference refactors only then
// (LBFGSTimeStepper::updatePrecondMtrAndFactorize, :266-270); a step never does.
int pd_factor(dotmi_handle *h)
{
    DevPD &D = h->PD;
    launch_pd_assemble(h->M, D, h->dtSq, h->st);
    HIPCHECK(h, hipMemsetAsync(h->W2, 0, sizeof(double) * std::max<size_t>(h->wTotal, 64), h->st));
    launch_pd_fill(D, h->M.nnzb, h->W2, h->st);
    HIPCHECK(h, hipMemsetAsync(h->info_dev, 0, sizeof(int), h->st));
    if (int rc = run_factor(h)) return rc;
    HIPCHECK(h, hipMemcpyAsync(h->h_info, h->info_dev, sizeof(int), hipMemcpyDeviceToHost, h->st));
    HIPCHECK(h, hipStreamSynchronize(h->st));
    HIPCHECK(h, hipGetLastError());
    if (h->h_info[0] != 0) {
        h->err = h->h_info[0] >= (1 << 30) ? "LBFGS-PD: the tile factorisation's dataflow scheduler timed out"
                                           : "LBFGS-PD: the Laplacian is not positive definite (pivot " + std::to_string(h->h_info[0]) + ")";
        h->poisoned = true;
        return h->h_info[0] >= (1 << 30) ? DOTMI_E_DEVICE : DOTMI_E_NOTSPD;
    }
    h->poisoned = false;
    return 0;
}

// z = L^-1 q per coordinate (q, z: nV x 3 interleaved); leaves the y_i . z partials of the stored pairs in partC
int pd_apply(dotmi_handle *h, const double *q, double *z, const LbfgsArgs &L)
{
    const bool timed = (h->flags & DOTMI_FLAG_TIME_BACKSOLVE) && h->evUsed + 2 <= (int)h->evPre.size() &&
                       (h->timeCount++ % h->timeStride) == 0;
    if (timed) HIPCHECK(h, hipEventRecord(h->evPre[h->evUsed], h->st));
    launch_pd_apply(h->PD, h->nV, q, z, h->st);
    if (timed) {
        HIPCHECK(h, hipEventRecord(h->evPre[h->evUsed + 1], h->st));
        h->evUsed += 2;
    }
    launch_multidot(h->n, z, L.y, L.m, h->partC, h->st);
    return 0;
}

}  // namespace dotmi
