// dotmi_create.hip -- dotmi_create and what it builds: mesh features, tolerance, the device side of every planning stage of block_plan.hpp (uploads and buffers), patches, loop state; dotmi_destroy and dotmi_last_error.  The host-only planning entries (dotmi_plan_*, dotmi_partition) are dotmi_plan.cpp
#include "dotmi_handle.hpp"
#include "block_plan.hpp"

namespace dotmi {
std::string g_create_error;
}

namespace dotmi {

// Mesh::computeFeatures (Mesh.cpp:589-700), computeMassMatrix tets (:552-585)
void host_features(dotmi_handle *h)
{
    const int nV = h->nV, nT = h->nT;
    h->A.assign((size_t)9 * nT, 0.0);
    h->vol.assign(nT, 0.0);
    h->mass.assign(nV, 0.0);
    for (int e = 0; e < nT; ++e) {
        const int *t = &h->T[4 * e];
        const double *p0 = &h->Xrest[3 * t[0]], *p1 = &h->Xrest[3 * t[1]], *p2 = &h->Xrest[3 * t[2]],
                     *p3 = &h->Xrest[3 * t[3]];
        Mat3 X0;
        for (int i = 0; i < 3; ++i) {
            X0.m[i][0] = p1[i] - p0[i];
            X0.m[i][1] = p2[i] - p0[i];
            X0.m[i][2] = p3[i] - p0[i];
        }
        const double d = det3(X0), id = 1.0 / d;
        const double(*m)[3] = X0.m;
        double *R = &h->A[(size_t)9 * e];
        R[0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) * id;
        R[1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * id;
        R[2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * id;
        R[3] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) * id;
        R[4] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * id;
        R[5] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * id;
        R[6] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) * id;
        R[7] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * id;
        R[8] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * id;
        h->vol[e] = d / 3.0 / 2.0;  // signed triArea, Mesh.cpp:639
        double a[3], b[3], c[3];
        for (int i = 0; i < 3; ++i) {
            a[i] = p0[i] - p3[i];
            b[i] = p1[i] - p3[i];
            c[i] = p2[i] - p3[i];
        }
        const double vv = std::fabs(a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) +
                                    a[2] * (b[0] * c[1] - b[1] * c[0])) / 6.0;
        for (int k = 0; k < 4; ++k) h->mass[t[k]] += vv / 4.0;
    }
    for (int v = 0; v < nV; ++v) h->mass[v] *= h->density;
}

// Optimizer::computeCharNormSq (Optimizer.cpp:613-651)
double host_target_gres(const dotmi_handle *h)
{
    Mat3 Aw;
    double Bw[3][4];
    const double S1[3] = {1, 1, 1};
#define TG_BLOCKS(MATV) spectral_blocks<MATV>(S1, h->mu[0], h->lam[0], 1.0, false, Aw, Bw)
    DM_DISPATCH_MAT(h->mat, TG_BLOCKS)
#undef TG_BLOCKS
    // with U = V = I the 9x9 matrix is exactly the 21 spectral entries (Energy.cpp:1183-1207)
    double sqH = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) sqH += Aw.m[i][j] * Aw.m[i][j];
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 4; ++k) sqH += Bw[c][k] * Bw[c][k];
    std::vector<double> ls(h->nV, 0.0);
    for (int e = 0; e < h->nT; ++e) {
        const int *t = &h->T[4 * e];
        for (int i = 0; i < 4; ++i) {
            const double *a = &h->Xrest[3 * t[(i + 1) % 4]], *b = &h->Xrest[3 * t[(i + 2) % 4]],
                         *c = &h->Xrest[3 * t[(i + 3) % 4]];
            const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
            const double w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
            const double cx = u[1] * w[2] - u[2] * w[1], cy = u[2] * w[0] - u[0] * w[2],
                         cz = u[0] * w[1] - u[1] * w[0];
            ls[t[i]] += 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
        }
    }
    double sql = 0;
    for (int v = 0; v < h->nV; ++v) sql += ls[v] * ls[v];
    // data0 carries exactly one fixed vertex (Mesh.cpp:592-598)
    const double cn = h->relTol * h->relTol * sqH * sql * (double)(h->nV - 1) / (double)h->nV;
    return cn * h->dtSq * h->dtSq;
}

// vertex patches (vpatches.hpp) -> device
int upload_vpatches(dotmi_handle *h, const HostVPatches &H, DevVPatches &D, dotmi_handle::SlotMap &SM)
{
    D.nPatches = H.nPatches;
    D.PE = H.PE;
    D.PV = H.PV;
    D.PO = H.PO;
    D.RUN = H.RUN;
    const size_t ns = (size_t)H.nPatches * H.PE;
    std::vector<ushort4> tl(ns), ep(ns);
    std::vector<double> A(9 * ns, 0.0), mu(ns, 1.0), lam(ns, 1.0), vol(ns, 0.0), volE(ns, 0.0);
    D.nSlotsUsed = 0;
    for (size_t s = 0; s < ns; ++s) {
        tl[s] = make_ushort4(H.tl[4 * s], H.tl[4 * s + 1], H.tl[4 * s + 2], H.tl[4 * s + 3]);
        ep[s] = make_ushort4(H.epos[4 * s], H.epos[4 * s + 1], H.epos[4 * s + 2], H.epos[4 * s + 3]);
        const int e = H.elem[s];
        if (e < 0) continue;
        D.nSlotsUsed++;
        for (int k = 0; k < 9; ++k) A[(size_t)k * ns + s] = h->A[(size_t)9 * e + k];
        mu[s] = h->mu[e];
        lam[s] = h->lam[e];
        vol[s] = h->vol[e];
        volE[s] = H.eown[s] ? h->vol[e] : 0.0;
    }
    if (int rc = upload(h, &D.tl, tl)) return rc;
    if (int rc = upload(h, &D.epos, ep)) return rc;
    if (int rc = upload(h, &D.A, A)) return rc;
    bool uniform = !h->mu.empty();
    for (size_t e = 1; e < h->mu.size() && uniform; ++e) uniform = h->mu[e] == h->mu[0] && h->lam[e] == h->lam[0];
    D.mu = D.lam = nullptr;
    if (uniform) {
        D.mu0 = h->mu[0];
        D.lam0 = h->lam[0];
    } else {
        if (int rc = upload(h, &D.mu, mu)) return rc;
        if (int rc = upload(h, &D.lam, lam)) return rc;
    }
    // the slot -> element table stays on the device: dotmi_set_lame fills the slot arrays through it (k_reconfig.hip)
    if (int rc = upload(h, &SM.elem, H.elem)) return rc;
    SM.nSlots = ns;
    SM.mu = D.mu;
    SM.lam = D.lam;
    if (int rc = upload(h, &D.vol, vol)) return rc;
    if (int rc = upload(h, &D.volE, volE)) return rc;
    if (int rc = upload(h, &D.pv_gid, H.pv_gid)) return rc;
    if (int rc = upload(h, &D.pv_cnt, H.pv_cnt)) return rc;
    if (int rc = upload(h, &D.po_cnt, H.po_cnt)) return rc;
    if (int rc = upload(h, &D.c_ptr, H.c_ptr)) return rc;
    return 0;
}

// patch lists + the element operands in patch order -> device
int upload_patches(dotmi_handle *h, const HostPatches &H, DevPatches &D, dotmi_handle::SlotMap &SM)
{
    D.nPatches = H.nPatches;
    D.PE = H.PE;
    D.PV = H.PV;
    D.nSlots = H.nSlots;
    const size_t ns = (size_t)H.nPatches * H.PE;
    std::vector<ushort4> tl(ns);
    std::vector<double> A(9 * ns, 0.0), mu(ns, 1.0), lam(ns, 1.0), vol(ns, 0.0);
    D.nElem = 0;
    for (size_t s = 0; s < ns; ++s) {
        tl[s] = make_ushort4(H.tl[4 * s], H.tl[4 * s + 1], H.tl[4 * s + 2], H.tl[4 * s + 3]);
        const int e = H.elem[s];
        if (e < 0) continue;
        D.nElem++;
        for (int k = 0; k < 9; ++k) A[(size_t)k * ns + s] = h->A[(size_t)9 * e + k];
        mu[s] = h->mu[e];
        lam[s] = h->lam[e];
        vol[s] = h->vol[e];
    }
    if (int rc = upload(h, &D.tl, tl)) return rc;
    if (int rc = upload(h, &D.A, A)) return rc;
    // one material (every input deck of the reference: Mesh.cpp:741-744 fills u / lambda from one Young's modulus and
    // Poisson ratio): the element pass takes the two numbers as kernel arguments instead of 16 bytes per tet
    bool uniform = !h->mu.empty();
    for (size_t e = 1; e < h->mu.size() && uniform; ++e) uniform = h->mu[e] == h->mu[0] && h->lam[e] == h->lam[0];
    D.mu = D.lam = nullptr;
    if (uniform) {
        D.mu0 = h->mu[0];
        D.lam0 = h->lam[0];
    } else {
        if (int rc = upload(h, &D.mu, mu)) return rc;
        if (int rc = upload(h, &D.lam, lam)) return rc;
    }
    // the slot -> element table stays on the device: dotmi_set_lame fills the slot arrays through it (k_reconfig.hip)
    if (int rc = upload(h, &SM.elem, H.elem)) return rc;
    SM.nSlots = ns;
    SM.mu = D.mu;
    SM.lam = D.lam;
    if (int rc = upload(h, &D.vol, vol)) return rc;
    if (int rc = upload(h, &D.pv_gid, H.pv_gid)) return rc;
    if (int rc = upload(h, &D.pv_slot, H.pv_slot)) return rc;
    if (int rc = upload(h, &D.pv_cnt, H.pv_cnt)) return rc;
    if (int rc = upload(h, &D.c_ptr, H.c_ptr)) return rc;
    {
        std::vector<ushort4> ep(ns);
        for (size_t s2 = 0; s2 < ns; ++s2) ep[s2] = make_ushort4(H.epos[4 * s2], H.epos[4 * s2 + 1], H.epos[4 * s2 + 2], H.epos[4 * s2 + 3]);
        if (int rc = upload(h, &D.epos, ep)) return rc;
    }
    {
        std::vector<int2> rng(H.pp_rng.size() / 2);
        for (size_t v = 0; v < rng.size(); ++v) rng[v] = make_int2(H.pp_rng[2 * v], H.pp_rng[2 * v + 1]);
        if (int rc = upload(h, &D.pp_rng, rng)) return rc;
    }
    if (int rc = dalloc(h, &D.gpart, (size_t)3 * std::max(H.nSlots, 1))) return rc;
    HIPCHECK(h, hipMemset(D.gpart, 0, sizeof(double) * 3 * (size_t)std::max(H.nSlots, 1)));
    return 0;
}

// what the element pass, the refresh's sharding and the owner exchange need beside the subdomains (the tail of build_device_mesh;
// an LBFGS-PD handle, which has no subdomains, builds this part only)
static int build_element_side(dotmi_handle *h, const std::vector<int> &adj_ptr, const std::vector<int> &blk_ptr,
                              const std::vector<int> &blk_ent)
{
    const int nV = h->nV, nT = h->nT;
    // element ownership + inertia vertex slice
    if (h->shardElems) {
        std::vector<int> el;
        for (int e = 0; e < nT; ++e)
            if (h->epart[e] >= h->p0 && h->epart[e] < h->p1) el.push_back(e);
        h->nOwnElem = (int)el.size();
        if (int rc = upload(h, &h->elist, el)) return rc;
        h->v0 = (int)((long long)nV * h->rank / h->world);
        h->v1 = (int)((long long)nV * (h->rank + 1) / h->world);
    } else {
        h->elist = nullptr;
        h->nOwnElem = nT;
        h->v0 = 0;
        h->v1 = nV;
    }
    // ---- sharded refresh lists ------------------------------------------------------------------------------------
    // The block rows this rank reads: the rows of its subdomains' vertices (dense fill of H_s = R_s H R_s^T) and its
    // slice [v0, v1) of the SpMV.  Their blocks are sums over the elements incident to the row vertex, so the elements
    // needed are the rank's own plus the halo that touches its interface vertices -- recomputed locally instead of
    // exchanging 1152 bytes per element (DOTTimeStepper.cpp:349-380, :574-616 run on every rank's share).
    h->shardHess = h->shardElems && (h->owner || (h->tune.shardHess >= 0 ? h->tune.shardHess != 0 : true));
    h->nHessElems = nT;
    if (h->shardHess) {
        std::vector<uint8_t> needV(nV, 0);
        for (int pI = h->p0; pI < h->p1; ++pI)
            for (int v : h->partVerts[pI]) needV[v] = 1;
        if (!h->owner)
            for (int v = h->v0; v < h->v1; ++v) needV[v] = 1;
        std::vector<int> el, e2c(nT, -1);
        for (int e = 0; e < nT; ++e)
            if (needV[h->T[4 * e]] || needV[h->T[4 * e + 1]] || needV[h->T[4 * e + 2]] || needV[h->T[4 * e + 3]]) {
                e2c[e] = (int)el.size();
                el.push_back(e);
            }
        std::vector<int> bl, bptr(1, 0), bent, optr(1, 0), oent;
        for (int v = 0; v < nV; ++v) {
            if (!needV[v]) continue;
            for (int k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) {
                bl.push_back(k);
                for (int i = blk_ptr[k]; i < blk_ptr[k + 1]; ++i) {
                    const int e = blk_ent[i] >> 4;
                    bent.push_back((e2c[e] << 4) | (blk_ent[i] & 15));   // every contributor touches v: listed
                    if (h->owner && h->epart[e] >= h->p0 && h->epart[e] < h->p1) oent.push_back(bent.back());
                }
                bptr.push_back((int)bent.size());
                optr.push_back((int)oent.size());
            }
        }
        if (h->owner) {
            if (oent.empty()) oent.push_back(-1);
            if (int rc = upload(h, &h->ownBlkPtr, optr)) return rc;
            if (int rc = upload(h, &h->ownBlkEnt, oent)) return rc;
        }
        h->nHessElems = (int)el.size();
        h->nHessBlk = (int)bl.size();
        if (int rc = upload(h, &h->hessElems, el)) return rc;
        if (int rc = upload(h, &h->hessBlk, bl)) return rc;
        if (int rc = upload(h, &h->hessBlkPtr, bptr)) return rc;
        if (int rc = upload(h, &h->hessBlkEnt, bent)) return rc;
    }
    // element patches (patches.hpp): PTall covers every element (the kernel-level entry points evaluate the whole mesh on
    // every rank), PT this rank's own elements -- the same object unless the element pass is sharded
    {
        int PE = h->tune.patchElems > 0 ? (h->tune.patchElems <= 256 ? 256 : 512) : 256;
        std::vector<int> all(nT);
        for (int e = 0; e < nT; ++e) all[e] = e;
        if (int rc = upload_patches(h, build_patches(nV, h->T.data(), h->Xrest.data(), all, PE), h->PTall, h->smAll)) return rc;
        if (h->shardElems) {
            std::vector<int> own;
            for (int e = 0; e < nT; ++e)
                if (h->epart[e] >= h->p0 && h->epart[e] < h->p1) own.push_back(e);
            if (int rc = upload_patches(h, build_patches(nV, h->T.data(), h->Xrest.data(), own, PE), h->PT, h->smOwn)) return rc;
        } else {
            h->PT = h->PTall;
        }
        // the patches of a speculating step (one rank): the set that keeps direction rows + patches + trial-point workgroups
        // resident at once -- the default set where it does, 512-element patches where only those do, none otherwise
        h->specFits = false;
        if (!h->dist && h->world == 1 && h->tune.specStep != 0) {
            const int nbv = (nV + 255) / 256, room = 512 - NB_RED - nbv;
            if (std::max(h->PT.nPatches, nbv) <= room) {
                h->PTspec = h->PT;
                h->specFits = true;
            } else if (h->tune.patchElems == 0 && PE == 256) {
                const HostPatches H2 = build_patches(nV, h->T.data(), h->Xrest.data(), all, 512);
                if (std::max(H2.nPatches, nbv) <= room) {
                    if (int rc = upload_patches(h, H2, h->PTspec, h->smSpec)) return rc;
                    h->specFits = true;
                }
            }
        }
    }
    if (h->owner) {
        // who holds / owns a vertex: a rank HOLDS the vertices of its subdomains (= of its elements); the lowest rank that
        // holds a vertex OWNS it (its inertia term, its share of every dot product).  Vertices held by two or more ranks
        // are the only ones whose entries travel inside the loop.
        std::vector<int> holders(nV, 0), last(nV, -1), ownerR(nV, -1);
        for (int r = 0; r < h->world; ++r)
            for (int pI = h->firstPart[r]; pI < h->firstPart[r + 1]; ++pI)
                for (int v : h->partVerts[pI])
                    if (last[v] != r) {
                        last[v] = r;
                        holders[v]++;
                        if (ownerR[v] < 0) ownerR[v] = r;
                    }
        std::vector<uint8_t> own(nV, 0), held(nV, 0);
        std::vector<int> iface;
        std::vector<double> mo(nV, 0.0);
        for (int pI = h->p0; pI < h->p1; ++pI)
            for (int v : h->partVerts[pI]) held[v] = 1;
        for (int v = 0; v < nV; ++v) {
            own[v] = ownerR[v] == h->rank || (ownerR[v] < 0 && h->rank == 0);
            if (own[v]) mo[v] = h->mass[v];
            if (holders[v] >= 2) iface.push_back(v);
        }
        h->nIface = (int)iface.size();
        if (iface.empty()) iface.push_back(0);
        std::vector<int> hl;
        for (int v = 0; v < nV; ++v)
            if (held[v]) hl.push_back(v);
        h->nHeld = (int)hl.size();
        if (hl.empty()) hl.push_back(0);
        if (int rc = upload(h, &h->heldList, hl)) return rc;
        if (int rc = upload(h, &h->ownMask, own)) return rc;
        if (int rc = upload(h, &h->heldMask, held)) return rc;
        {
            std::vector<uint8_t> kind(nV);
            for (int v = 0; v < nV; ++v) kind[v] = (uint8_t)((own[v] ? 1 : 0) | (holders[v] >= 2 ? 2 : 0));
            if (int rc = upload(h, &h->vkind, kind)) return rc;
            std::vector<int> sh;
            for (int v = 0; v < nV; ++v)
                if (held[v] && holders[v] >= 2) sh.push_back(v);
            h->nShared = (int)sh.size();
            if (sh.empty()) sh.push_back(0);
            if (int rc = upload(h, &h->sharedList, sh)) return rc;
        }
        if (int rc = upload(h, &h->ifaceIdx, iface)) return rc;
        if (int rc = upload(h, &h->massOwn, mo)) return rc;
        if (int rc = dalloc(h, &h->xpack, (size_t)3 * h->nIface + 8 + RED_K)) return rc;
        // the element pass' inertia term 1/2 m |x - x~|^2 by ownership too: the same kernel over every vertex with the
        // owner's share of the mass (positions outside the held vertices stay where the warm start put them)
        h->Mown = h->M;
        h->Mown.mass = h->massOwn;
        if (h->tune.fuseLog)
            fprintf(stderr, "dotmi: owner exchange: rank %d holds %d of %d vertices, %d are held by more than one rank\n", h->rank,
                    (int)std::count(held.begin(), held.end(), 1), nV, h->nIface);
    }
    return 0;
}

// element arrays, block-CSR adjacency incl. self and the per-block contribution lists -> device
static int build_mesh_graph(dotmi_handle *h, MeshGraph &G, std::vector<int> &blk_ptr, std::vector<int> &blk_ent)
{
    const int nV = h->nV, nT = h->nT;
    DevMesh &M = h->M;
    M.nV = nV;
    M.nT = nT;
    M.nTp = (nT + 63) / 64 * 64;
    // elements
    {
        std::vector<int4> T4(nT);
        for (int e = 0; e < nT; ++e) T4[e] = make_int4(h->T[4 * e], h->T[4 * e + 1], h->T[4 * e + 2], h->T[4 * e + 3]);
        if (int rc = upload(h, &M.T, T4)) return rc;
        std::vector<double> Asoa((size_t)9 * M.nTp, 0.0);
        for (int e = 0; e < nT; ++e)
            for (int k = 0; k < 9; ++k) Asoa[(size_t)k * M.nTp + e] = h->A[(size_t)9 * e + k];
        if (int rc = upload(h, &M.A, Asoa)) return rc;
        if (int rc = upload(h, &M.mu, h->mu)) return rc;
        if (int rc = upload(h, &M.lam, h->lam)) return rc;
        if (int rc = upload(h, &M.vol, h->vol)) return rc;
        if (int rc = upload(h, &M.mass, h->mass)) return rc;
        if (int rc = upload(h, &M.fixed, h->fixed)) return rc;
    }
    // adjacency incl. self
    G = mesh_graph(nV, nT, h->T.data(), h->Xrest.data());
    const std::vector<int> &adj_ptr = G.adj_ptr, &adj_idx = G.adj_idx;
    M.nnzb = adj_ptr[nV];
    std::vector<int> blk_row(M.nnzb);
    for (int v = 0; v < nV; ++v)
        for (int k = adj_ptr[v]; k < adj_ptr[v + 1]; ++k) blk_row[k] = v;
    auto find_block = [&](int v, int u) {
        const int *b = &adj_idx[adj_ptr[v]], *e = &adj_idx[adj_ptr[v + 1]];
        return (int)(std::lower_bound(b, e, u) - adj_idx.data());
    };
    // per-block contributions, ascending element
    std::vector<int> eblk((size_t)16 * nT);
    blk_ptr.assign(M.nnzb + 1, 0);
    blk_ent.resize((size_t)16 * nT);
    for (int e = 0; e < nT; ++e)
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const int k = find_block(h->T[4 * e + a], h->T[4 * e + b]);
                eblk[(size_t)16 * e + 4 * a + b] = k;
                blk_ptr[k + 1]++;
            }
    for (int k = 0; k < M.nnzb; ++k) blk_ptr[k + 1] += blk_ptr[k];
    {
        std::vector<int> cur(blk_ptr.begin(), blk_ptr.end() - 1);
        for (int e = 0; e < nT; ++e)
            for (int ab = 0; ab < 16; ++ab) blk_ent[cur[eblk[(size_t)16 * e + ab]]++] = 16 * e + ab;
    }
    if (int rc = upload(h, &M.adj_ptr, adj_ptr)) return rc;
    if (int rc = upload(h, &M.adj_idx, adj_idx)) return rc;
    if (int rc = upload(h, &M.blk_ptr, blk_ptr)) return rc;
    if (int rc = upload(h, &M.blk_ent, blk_ent)) return rc;
    if (int rc = upload(h, &M.blk_row, blk_row)) return rc;
    return 0;
}

// subdomains (ADMMDDTimeStepper.cpp:88-262): the vertex sets of all parts, how many hold a vertex, the parts this rank owns
static void choose_subdomains(dotmi_handle *h)
{
    const int nP = h->nPartsAll;
    if (!h->vpart.empty()) {   // vertex partition given: disjoint vertex sets (block-Jacobi, LBFGS-JH)
        h->partVerts.assign(nP, {});
        for (int v = 0; v < h->nV; ++v) h->partVerts[h->vpart[v]].push_back(v);
    } else {
        h->partVerts = part_vertex_sets(h->nT, h->T.data(), h->epart.data(), nP);
    }
    h->dup.assign(h->nV, 0);
    // ownership: contiguous groups of parts balanced by sum n_s^2 (the back-solve cost)
    std::vector<int32_t> ps(nP);
    for (int pI = 0; pI < nP; ++pI) {
        for (int v : h->partVerts[pI]) h->dup[v]++;
        ps[pI] = 3 * (int32_t)h->partVerts[pI].size();
    }
    h->firstPart.assign(h->world + 1, 0);
    dotmi_plan_shards(nP, ps.data(), h->world, h->firstPart.data());
    h->p0 = h->firstPart[h->rank];
    h->p1 = h->firstPart[h->rank + 1];
}

// the factors are the one allocation that grows with the square of the subdomain size: refuse what cannot fit
// instead of failing somewhere inside hipMalloc
static int check_factors_fit(dotmi_handle *h, const FactorStorage &F)
{
    size_t freeB = 0, totalB = 0;
    HIPCHECK(h, hipMemGetInfo(&freeB, &totalB));
    const double need = 8.0 * (double)F.wOnePass * 2.1;   // + the work buffer of the factorisation
    if (need > 0.9 * (double)freeB) {
        h->err = "the subdomain factors need " + std::to_string((long long)(need / 1e9)) + " GB (" + std::to_string(h->P.nParts) +
                 " subdomains, padded size " + std::to_string(h->P.nmax) + "), more than the free HBM: use more subdomains";
        return DOTMI_E_INVALID;
    }
    if (8.0 * (double)F.wTotal * 2.1 > 0.9 * (double)freeB) {
        h->err = "the two-level factors do not fit the free HBM";
        return DOTMI_E_INVALID;
    }
    return 0;
}

// the padded layout and the job table of the back-solve launches (bs_tiles.hpp) -> device
static int upload_backsolve_tables(dotmi_handle *h, const std::vector<int> &dofmap, const BsTilePlan &TP)
{
    DevParts &P = h->P;
    P.nbmax = 1;
    for (auto &r : TP.ranges) P.nbmax = std::max(P.nbmax, (int)r.size());
    std::vector<int2> trange((size_t)std::max(P.nParts, 1) * P.nbmax, make_int2(0, 0));
    for (int ls = 0; ls < P.nParts; ++ls) std::copy(TP.ranges[ls].begin(), TP.ranges[ls].end(), trange.begin() + (size_t)ls * P.nbmax);
    h->partTilePtr = TP.partTilePtr;
    h->partLworkPtr = TP.partLworkPtr;
    P.maxTileLen = TP.maxTileLen;
    P.maxChunks = TP.maxChunks;
    P.ntiles = TP.ntiles;
    P.ntilesWide = TP.ntilesWide;
    P.nquad = TP.nquad;
    P.nltiles = (int)TP.ltiles.size();
    P.nlwork = (int)TP.lwork.size();
    if (int rc = upload(h, &P.dofmap, dofmap)) return rc;
    if (int rc = upload(h, &P.tile, TP.tiles)) return rc;
    if (int rc = upload(h, &P.tileByPart, TP.tilesByPart)) return rc;
    if (int rc = upload(h, &P.ltileByPart, TP.ltilesByPart)) return rc;
    if (int rc = upload(h, &P.lworkByPart, TP.lworkByPart)) return rc;
    if (int rc = upload(h, &P.ltile, TP.ltiles)) return rc;
    if (int rc = upload(h, &P.lwork, TP.lwork)) return rc;
    if (int rc = dalloc(h, &P.tdots, (size_t)std::max(P.nltiles, 1) * P.maxChunks * 64)) return rc;
    HIPCHECK(h, hipMemset(P.tdots, 0, sizeof(double) * (size_t)std::max(P.nltiles, 1) * P.maxChunks * 64));
    return upload(h, &P.trange, trange);
}

static int upload_merge_lists(dotmi_handle *h, const MergeLists &M)
{
    DevParts &P = h->P;
    if (int rc = upload(h, &P.vp_ptr, M.vp_ptr)) return rc;
    if (int rc = upload(h, &P.vp_off, M.vp_off)) return rc;
    P.mt_ptr = nullptr;
    P.mt_ent = nullptr;
    P.mt_wave = nullptr;
    P.mt_il = nullptr;
    P.splitMerge = M.splitMerge;
    if (h->flags & DOTMI_FLAG_GSDD) return 0;
    if (M.walk) {
        if (int rc = upload(h, &P.mt_ptr, M.mp)) return rc;
        if (int rc = upload(h, &P.mt_ent, M.ment)) return rc;
        if (!M.il.empty()) {
            if (int rc = upload(h, &P.mt_wave, M.mw)) return rc;
            if (int rc = upload(h, &P.mt_il, M.il)) return rc;
        }
    }
    if (h->tune.fuseLog) {
        int lmax = 0;
        long long over24 = 0;
        for (size_t k = 0; k + 1 < M.mp.size(); ++k) {
            lmax = std::max(lmax, M.mp[k + 1] - M.mp[k]);
            over24 += M.mp[k + 1] - M.mp[k] > 24;
        }
        fprintf(stderr, "dotmi: merge: %.1f tile partials per dof (longest list %d, %lld lists beyond 24) -> %s\n",
                (double)M.count / std::max(1, 3 * h->nV), lmax, over24,
                P.splitMerge ? "sum per subdomain, then gather (split)" : "one walk over the list");
    }
    h->mergeEntries = M.count;   // tile partials one merge reads (either form)
    return 0;
}

// the tile schedule of the factorisation -> device, and what its launch form needs (flags and counters of the dataflow launch,
// the side stream and events of the split levels)
static bool tile_split_levels(const Tuning &tune, int nParts) { return tune.tileSplit >= 0 ? tune.tileSplit != 0 : nParts > 64; }

// Subdomain groups of the level launches (DOTMI_TILE_GROUPS; profiles/r07_factor_groups.txt).  Two by default wherever the
// levels run as one launch each: bar17K / 32 subdomains 0.979 -> 0.893 ms per factorisation, kingkong18K / 18 1.155 -> 1.046,
// the stiff monkey / 64 0.549 -> 0.507; three groups are level with two on the latter two and behind on bar17K, four lose again
// (every chain's diagonal-paced levels then hold slots the others' bulk levels want).  The split levels keep their one chain
// (their diagonal tasks already run beside the rest), and beside st there are at most three streams -- a process has four
// hardware queues.
static int choose_tile_groups(const Tuning &tune, int nParts)
{
    if (tile_split_levels(tune, nParts)) return 1;
    const int G = tune.tileGroups >= 0 ? tune.tileGroups : 2;
    return std::max(1, std::min(G, 4));
}

static int upload_factor_schedule(dotmi_handle *h, const FactorSchedule &FS)
{
    const TileSchedule &S = FS.S;
    if (int rc = upload(h, &h->ttasks, S.tasks)) return rc;
    if (int rc = upload(h, &h->tprods, S.prods)) return rc;
    if (int rc = upload(h, &h->tclear, S.clearTiles)) return rc;
    if (int rc = upload(h, &h->tclearLd, S.clearLd)) return rc;
    h->nTclear = (int)S.clearTiles.size();
    h->tileHfill = !S.fillPtr.empty();
    if (h->tileHfill) {
        std::vector<TileFillEntry> fl = S.fill;
        if (fl.empty()) fl.push_back(TileFillEntry{-1, 0, 0});
        if (int rc = upload(h, &h->tfill, fl)) return rc;
        if (h->tune.fuseLog)
            fprintf(stderr, "dotmi: tile fill: %zu entries in %zu tiles (%.1f MB of lists)\n", S.fill.size(), S.clearTiles.size(),
                    8e-6 * S.fill.size());
    }
    h->tlevelStart = S.levelStart;
    h->tlevelDiag = S.levelDiag;
    h->tgroupLevel = S.groupLevel;
    h->tileSplit = tile_split_levels(h->tune, h->P.nParts);
    h->nTtasks = (int)S.tasks.size();
    h->tileFlow = FS.flow;
    // the diagonal tasks' per-lane bottom steps (k_tilefactor.hip, block_chol_inv<N, FAST>): every layout (DOTMI_FAST_DIAG=0: the
    // one-row-per-lane base of round 3); the 256-thread level kernel keeps the old base, and then so does the dataflow launch
    h->fastDiag = h->tune.fastDiag != 0;
    if (h->tileFlow) {
        if (int rc = upload(h, &h->tdepPtr, FS.depPtr)) return rc;
        if (int rc = upload(h, &h->tdepIdx, FS.depIdx)) return rc;
        if (int rc = dalloc(h, &h->tdone, S.tasks.size())) return rc;
        if (int rc = dalloc(h, &h->tnext, 2)) return rc;
        HIPCHECK(h, hipMemset(h->tdone, 0, sizeof(int) * S.tasks.size()));
        HIPCHECK(h, hipMemset(h->tnext, 0, sizeof(int) * 2));
        hipDeviceProp_t prop;
        HIPCHECK(h, hipGetDeviceProperties(&prop, h->device));
        h->tileFlowWg = 2 * prop.multiProcessorCount;
        h->tileSplit = false;
        if (h->tune.fuseLog)
            fprintf(stderr, "dotmi: tile dataflow: %zu tasks, %zu dependencies, %d workgroups\n", S.tasks.size(), FS.depIdx.size(),
                    h->tileFlowWg);
    }
    if (h->tgroupLevel.size() > 2) {   // one stream per group beside st, one fork event, one join event per stream
        h->stGroup.assign(h->tgroupLevel.size() - 2, nullptr);
        h->evGroupJoin.assign(h->stGroup.size(), nullptr);
        for (auto &s : h->stGroup) HIPCHECK(h, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIPCHECK(h, hipEventCreateWithFlags(&h->evGroupFork, hipEventDisableTiming));
        for (auto &e : h->evGroupJoin) HIPCHECK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (h->tune.fuseLog)
            for (size_t g = 0; g + 1 < h->tgroupLevel.size(); ++g)
                fprintf(stderr, "dotmi: tile group %zu: %d levels, %d tasks\n", g, h->tgroupLevel[g + 1] - h->tgroupLevel[g],
                        h->tlevelStart[h->tgroupLevel[g + 1]] - h->tlevelStart[h->tgroupLevel[g]]);
    }
    if (h->tileSplit) {
        HIPCHECK(h, hipStreamCreateWithFlags(&h->stDiag, hipStreamNonBlocking));
        h->tFork.resize(S.levelDiag.size());
        h->tJoin.resize(S.levelDiag.size());
        for (auto &e : h->tFork) HIPCHECK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        for (auto &e : h->tJoin) HIPCHECK(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    h->tileFlops = S.flops;
    if (h->tune.fuseLog)
        fprintf(stderr, "dotmi: tile schedule: %zu tasks, %zu products, %zu levels, %lld Q tiles, %.1f GF\n", S.tasks.size(),
                S.prods.size(), S.levelStart.size() - 1, S.qTiles, S.flops / 1e9);
    return 0;
}

// the panels of the two-level form (DevTwoLevel) -> device
static int upload_two_level(dotmi_handle *h, const TwoLevelPanels &T)
{
    DevParts &P = h->P;
    int2 *dItem = nullptr;
    if (int rc = upload(h, &dItem, T.items)) return rc;
    P.tl.item = dItem;
    P.tl.nItems = T.maxRows > 0 ? (int)T.items.size() : 0;
    int4 *dPanel = nullptr;
    long long *dBase = nullptr, *dDst = nullptr;
    if (int rc = upload(h, &dDst, T.rowDst)) return rc;
    if (int rc = dalloc(h, &P.tl.packed, (size_t)std::max<long long>(T.packedN, 2))) return rc;
    int *dPos = nullptr, *dPtr = nullptr, *dIdx = nullptr;
    P.tl.nPanels = T.maxRows > 0 ? (int)T.panel.size() : 0;
    if (int rc = upload(h, &dPanel, T.panel)) return rc;
    if (int rc = upload(h, &dBase, T.rowBase)) return rc;
    if (int rc = upload(h, &dPos, T.rowPos)) return rc;
    if (int rc = upload(h, &dPtr, T.gPtr)) return rc;
    if (int rc = upload(h, &dIdx, T.gIdx)) return rc;
    if (int rc = dalloc(h, &P.tl.cbuf, T.rowBase.size())) return rc;
    if (int rc = dalloc(h, &P.tl.rpad2, (size_t)P.nParts * P.nmax + 8)) return rc;
    HIPCHECK(h, hipMemset(P.tl.rpad2, 0, sizeof(double) * ((size_t)P.nParts * P.nmax + 8)));
    P.tl.panel = dPanel;
    P.tl.rowSrc = dBase;
    P.tl.rowBase = dDst;
    P.tl.rowPos = dPos;
    P.tl.gPtr = dPtr;
    P.tl.gIdx = dIdx;
    P.tl.maxRows = T.maxRows;
    P.tl.maxCols = T.maxCols;
    P.tl.on = 1;
    h->precond_bytes += 2 * T.panelBytes;   // (the panels are streamed twice per application)
    if (h->tune.fuseLog)
        fprintf(stderr, "dotmi: two-level back-solve: %d panels (at most %d rows x %d columns), %.1f MB of panels (x 2), %.1f MB in all\n",
                P.tl.nPanels, T.maxRows, T.maxCols, T.panelBytes / 1e6, h->precond_bytes / 1e6);
    return 0;
}

// the subdomain side of the handle: every stage of block_plan.hpp, the uploads of its arrays, the next stage
int build_device_mesh(dotmi_handle *h)
{
    MeshGraph G;
    std::vector<int> blk_ptr, blk_ent;
    if (int rc = build_mesh_graph(h, G, blk_ptr, blk_ent)) return rc;
    if (h->pd) {   // LBFGS-PD: the scalar factor of the constant Laplacian instead of the subdomain block solve (dotmi_pd.hip)
        if (int rc = build_pd(h, G.adj_ptr, G.adj_idx)) return rc;
        return build_element_side(h, G.adj_ptr, blk_ptr, blk_ent);
    }
    if (h->hi) {   // LBFGS-HI: the block incomplete Cholesky of H on its own block pattern, no subdomains either (dotmi_ic.hip)
        if (int rc = build_ic(h, G.adj_ptr, G.adj_idx)) return rc;
        return build_element_side(h, G.adj_ptr, blk_ptr, blk_ent);
    }
    choose_subdomains(h);
    const std::vector<std::vector<int>> &sets = h->partVerts;
    const Tuning &tune = h->tune;
    const int p0 = h->p0, p1 = h->p1;
    const bool gsdd = (h->flags & DOTMI_FLAG_GSDD) != 0;
    DevParts &P = h->P;
    P.nParts = p1 - p0;
    h->tileMode = P.nParts > 0;   // (a rank without subdomains plans nothing)
    BlockLayout L;
    choose_block_layout(G, sets, p0, p1,
                        LayoutRules{tune.ndLevels, tune.ndMin, tune.ndMinByUser, tune.twoLevel, !gsdd, false, tune.fuseLog}, L);
    h->nd = L.nd;
    h->twoLevel = L.twoLevel;
    P.nmax = L.nmax;
    RowPlacement rows;
    place_rows(L, sets, p0, p1, rows);
    h->precond_bytes = rows.nnzX * 8;
    // the job table of the back-solve launches (bs_tiles.hpp): tiles per region, wide / narrow / packs, heavy first
    BsTilePlan TP;
    plan_backsolve_tiles(L.nd, [&](int k, int ls) { return 3 * (int)L.region[k][ls].size(); }, P.nParts, P.nmax,
                         BsTileRules{tune.tileRows, tune.tileRowsLong, tune.tilePasses, tune.wavePacks}, TP);
    if (tune.fuseLog)
        fprintf(stderr, "dotmi: back-solve: %d one-tile jobs (%d wide), %d packs of four small tiles%s\n", TP.ntiles, TP.ntilesWide,
                TP.nquad, TP.shallow ? ", shallow launch: long rows in 4-pass tiles" : "");
    FactorStorage F;
    plan_factor_storage(L, rows.dofmap, P.nParts, F);
    if (int rc = check_factors_fit(h, F)) return rc;
    const RowTileArrays rt = row_tile_arrays(F.rtab), rtM = row_tile_arrays(F.rtabM);
    h->rtOff = rt.off;
    h->rtLd = rt.ld;
    h->rtC0 = rt.c0;
    h->rtOffM = rtM.off;
    h->rtLdM = rtM.ld;
    h->rtC0M = rtM.c0;
    h->wTotal = F.wTotal;
    FillLists fill;
    build_fill_lists(G, sets, p0, p1, rows, P.nmax, F, fill);
    P.nfill = (int)fill.fill_src.size();
    P.npad = (int)fill.pad_dst.size();
    if (int rc = upload_backsolve_tables(h, rows.dofmap, TP)) return rc;
    std::vector<int> rptr, ridx;
    build_reduce_lists(TP.ranges, P.nParts, P.nmax, rptr, ridx);
    if (int rc = upload(h, &P.rp_ptr, rptr)) return rc;
    if (int rc = upload(h, &P.rp_idx, ridx)) return rc;
    MergeLists M;
    build_merge_lists(h->nV, sets, p0, p1, rows, P.nmax, P.nbmax, TP.ranges, tune.splitMerge, L.twoLevel, gsdd, M);
    if (int rc = upload_merge_lists(h, M)) return rc;
    if (int rc = upload(h, &P.dup, h->dup)) return rc;
    if (int rc = upload(h, &P.fill_dst, fill.fill_dst)) return rc;
    if (int rc = upload(h, &P.fill_src, fill.fill_src)) return rc;
    if (int rc = upload(h, &P.pad_dst, fill.pad_dst)) return rc;
    if (int rc = dalloc(h, &P.W, std::max<size_t>(F.wTotal, 64))) return rc;
    if (int rc = upload(h, &P.rt, F.rtab)) return rc;
    if (h->tileMode) {
        // the work buffer (H filled in, R in place of it): same layout as the factor buffer W, which only ever holds Q
        if (int rc = dalloc(h, &h->W2, std::max<size_t>(F.wTotal, 64))) return rc;
        FactorSchedule FS;
        plan_factor_schedule(P.nParts, P.nmax, rows.dofmap, fill.fillBlk, rt, rtM, L.twoLevel ? F.leafTile.data() : nullptr, P.W, h->W2,
                             ScheduleRules{tune.tileEagerMin, tune.tileEagerMinRmul, tune.tileEagerMinRmulByUser, tune.tileFlow,
                                           choose_tile_groups(tune, P.nParts), tune.tileHfill != 0},
                             FS);
        if (tune.tileHfill) {
            h->err = build_tile_fill(FS.S, h->W2, fill, rt, rtM);
            if (!h->err.empty()) return DOTMI_E_INVALID;
        }
        if (int rc = upload_factor_schedule(h, FS)) return rc;
    }
    if (int rc = dalloc(h, &P.ppart, (size_t)P.nParts * P.nbmax * P.nmax)) return rc;
    if (int rc = dalloc(h, &P.psub, (size_t)P.nParts * P.nmax)) return rc;
    if (int rc = dalloc(h, &P.rpad, (size_t)P.nParts * P.nmax + 8)) return rc;
    HIPCHECK(h, hipMemset(P.rpad, 0, sizeof(double) * ((size_t)P.nParts * P.nmax + 8)));
    P.tl = DevTwoLevel{};
    if (L.twoLevel) {
        TwoLevelPanels T;
        h->err = plan_two_level_panels(G, L, sets, p0, p1, F, T);
        if (!h->err.empty()) return DOTMI_E_INVALID;
        if (int rc = upload_two_level(h, T)) return rc;
    }
    if (int rc = dalloc(h, &h->info_dev, (size_t)std::max(P.nParts, 1))) return rc;
    HIPCHECK(h, hipHostMalloc((void **)&h->h_info, sizeof(int) * std::max(P.nParts, 1)));
    memset(h->h_info, 0, sizeof(int) * std::max(P.nParts, 1));
    h->partPos = std::move(rows.partPos);
    return build_element_side(h, G.adj_ptr, blk_ptr, blk_ent);
}

LbfgsArgs lbfgs_args(const dotmi_handle *h)
{
    LbfgsArgs L;
    memset(&L, 0, sizeof(L));
    L.m = h->m;
    for (int i = 0; i < h->m; ++i) {
        L.s[i] = h->S[h->order[i]];
        L.y[i] = h->Y[h->order[i]];
        L.ys[i] = h->ys[i];
        for (int j = 0; j < h->m; ++j) L.sy[i][j] = h->sy[i][j];
    }
    return L;
}

}  // namespace dotmi

extern "C" {

const char *dotmi_last_error(const dotmi_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void dotmi_destroy(dotmi_handle *h)
{
    if (!h) return;
    hipSetDevice(h->device);
    if (h->st) hipStreamSynchronize(h->st);
    if (h->comm) ncclCommDestroy(h->comm);
    for (void *p : h->allocs) hipFree(p);
    if (h->arStage) hipHostFree(h->arStage);
    if (h->h_partE) hipHostFree(h->h_partE);
    if (h->h_partR) hipHostFree(h->h_partR);
    if (h->h_alpha) hipHostFree(h->h_alpha);
    if (h->h_ctl) hipHostFree(h->h_ctl);
    if (h->h_pcg) hipHostFree(h->h_pcg);
    if (h->coarse.h_info) hipHostFree(h->coarse.h_info);
    if (h->coarse.ev0) hipEventDestroy(h->coarse.ev0);
    if (h->coarse.ev1) hipEventDestroy(h->coarse.ev1);
    if (h->dposPinned) hipHostFree(h->dposPinned);
    if (h->evDir) hipEventDestroy(h->evDir);
    if (h->h_info) hipHostFree(h->h_info);
    if (h->h_flags) hipHostFree(h->h_flags);
    if (h->ev0) hipEventDestroy(h->ev0);
    if (h->ev1) hipEventDestroy(h->ev1);
    if (h->ev2) hipEventDestroy(h->ev2);
    if (h->evA) hipEventDestroy(h->evA);
    for (hipEvent_t e : h->evP)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : h->tFork) hipEventDestroy(e);
    for (hipEvent_t e : h->tJoin) hipEventDestroy(e);
    if (h->stDiag) hipStreamDestroy(h->stDiag);
    if (h->evGroupFork) hipEventDestroy(h->evGroupFork);
    for (hipEvent_t e : h->evGroupJoin)
        if (e) hipEventDestroy(e);
    for (hipStream_t s : h->stGroup)
        if (s) hipStreamDestroy(s);
    for (hipEvent_t e : h->evPre) hipEventDestroy(e);
    for (hipEvent_t e : h->evAr) hipEventDestroy(e);
    if (h->factorGraph) hipGraphExecDestroy(h->factorGraph);
    if (h->st) hipStreamDestroy(h->st);
    delete h;
}

// the caller's mesh and parameters -> the handle's configuration and host copies (no device call)
static int take_arguments(dotmi_handle *h, const dotmi_mesh *mesh, const dotmi_params *prm)
{
    h->nV = mesh->nV;
    h->nT = mesh->nT;
    h->n = 3 * mesh->nV;
    h->mat = prm->energy;
    h->hist = prm->history;
    h->iterCap = prm->iterCap > 0 ? prm->iterCap : 10000;
    h->dt = prm->dt;
    h->dtUser = prm->dt;
    h->dtSq = prm->dt * prm->dt;
    for (int d = 0; d < 3; ++d) {
        h->grav[d] = prm->gravity[d];
        h->gdtsq[d] = h->dtSq * prm->gravity[d];
    }
    h->relTol = prm->relTol;
    h->alphaMin = prm->alphaMin;
    h->device = prm->device;
    h->rank = prm->rank;
    h->world = prm->world;
    h->flags = prm->flags;
    h->tune = Tuning::from_env();
#ifdef DOTMI_TEST_HOOKS
    h->testIterDelta = Tuning::geti("DOTMI_TEST_ITER_DELTA", 0);
    h->testFailRefresh = Tuning::geti("DOTMI_TEST_FAIL_REFRESH", 0);
#endif
    h->density = mesh->density;
    h->nPartsAll = mesh->nParts;
    h->T.assign(mesh->T, mesh->T + 4 * (size_t)h->nT);
    h->pd = (h->flags & DOTMI_FLAG_LBFGS_PD) != 0;
    h->hi = (h->flags & DOTMI_FLAG_LBFGS_HI) != 0;
    h->newtonPcg = (h->flags & DOTMI_FLAG_NEWTON_PCG) != 0;
    if (h->newtonPcg) {
        const int bad = DOTMI_FLAG_FORCE_DIST | DOTMI_FLAG_OWNER_EXCHANGE | DOTMI_FLAG_GSDD | DOTMI_FLAG_NEWTON | DOTMI_FLAG_LBFGS_PD |
                        DOTMI_FLAG_LBFGS_HI | DOTMI_FLAG_ASYNC_REFRESH;
        if (prm->world > 1 || (h->flags & bad) || mesh->vpart) {
            h->err = "DOTMI_FLAG_NEWTON_PCG: single GPU, host loop, not with DOTMI_FLAG_FORCE_DIST / OWNER_EXCHANGE / GSDD / NEWTON / "
                     "LBFGS_PD / LBFGS_HI / ASYNC_REFRESH or a vertex partition";
            return DOTMI_E_INVALID;
        }
    }
    if (h->flags & DOTMI_FLAG_NEWTON_PCG_DIST) {
        // the same step on sharded subdomains (dotmi_pcg.hip): a flag of its own, as it changes which collectives the communicator
        // carries; on one rank without FORCE_DIST it is DOTMI_FLAG_NEWTON_PCG
        const char *why = (h->flags & DOTMI_FLAG_OWNER_EXCHANGE) ? "not with DOTMI_FLAG_OWNER_EXCHANGE (the vectors of the recurrences are replicated)"
                          : (h->flags & DOTMI_FLAG_GSDD)         ? "not with DOTMI_FLAG_GSDD (a GSDD handle solves one subdomain at a time)"
                          : (h->flags & DOTMI_FLAG_NEWTON)       ? "not with DOTMI_FLAG_NEWTON (a Newton handle factorises H as one subdomain)"
                          : (h->flags & DOTMI_FLAG_LBFGS_PD)     ? "not with DOTMI_FLAG_LBFGS_PD (no Hessian block solve)"
                          : (h->flags & DOTMI_FLAG_LBFGS_HI)     ? "not with DOTMI_FLAG_LBFGS_HI (no Hessian block solve)"
                          : (h->flags & DOTMI_FLAG_ASYNC_REFRESH)
                              ? "not with DOTMI_FLAG_ASYNC_REFRESH (a Newton iteration factorises at its own iterate)"
                          : (h->flags & DOTMI_FLAG_DOT_COARSE) ? "not with DOTMI_FLAG_DOT_COARSE (the sharded PCG has no coarse space)"
                          : mesh->vpart                        ? "not with a vertex partition (vpart): it is single-GPU only"
                                                               : nullptr;
        if (why) {
            h->err = std::string("DOTMI_FLAG_NEWTON_PCG_DIST: ") + why;
            return DOTMI_E_INVALID;
        }
        h->newtonPcg = true;
    }
    if (h->hi) {
        const int bad = DOTMI_FLAG_FORCE_DIST | DOTMI_FLAG_OWNER_EXCHANGE | DOTMI_FLAG_GSDD | DOTMI_FLAG_NEWTON | DOTMI_FLAG_LBFGS_PD |
                        DOTMI_FLAG_ASYNC_REFRESH;
        if (prm->world > 1 || (h->flags & bad) || mesh->vpart) {
            h->err = "DOTMI_FLAG_LBFGS_HI: single GPU, host loop, not with DOTMI_FLAG_FORCE_DIST / OWNER_EXCHANGE / GSDD / NEWTON / "
                     "LBFGS_PD / ASYNC_REFRESH or a vertex partition";
            return DOTMI_E_INVALID;
        }
        h->nPartsAll = 1;
        h->epart.assign(h->nT, 0);   // (unused: no subdomains)
    } else if (h->pd) {
        const int bad = DOTMI_FLAG_FORCE_DIST | DOTMI_FLAG_OWNER_EXCHANGE | DOTMI_FLAG_GSDD | DOTMI_FLAG_NEWTON | DOTMI_FLAG_ASYNC_REFRESH;
        if (prm->world > 1 || (h->flags & bad) || mesh->vpart) {
            h->err = "DOTMI_FLAG_LBFGS_PD: single GPU, host loop, not with DOTMI_FLAG_FORCE_DIST / OWNER_EXCHANGE / GSDD / NEWTON / "
                     "ASYNC_REFRESH or a vertex partition";
            return DOTMI_E_INVALID;
        }
        h->nPartsAll = 1;
        h->epart.assign(h->nT, 0);   // (unused: no subdomains)
    } else if (mesh->vpart) {
        if (prm->world > 1 || (prm->flags & DOTMI_FLAG_FORCE_DIST)) {
            h->err = "a vertex partition (vpart) is single-GPU only";
            return DOTMI_E_INVALID;
        }
        for (int v = 0; v < mesh->nV; ++v)
            if (mesh->vpart[v] < 0 || mesh->vpart[v] >= mesh->nParts) {
                h->err = "vpart out of range";
                return DOTMI_E_INVALID;
            }
        h->vpart.assign(mesh->vpart, mesh->vpart + h->nV);
        h->epart.assign(h->nT, 0);   // unused: the subdomains are vertex sets
    } else if (mesh->epart) {
        h->epart.assign(mesh->epart, mesh->epart + h->nT);
    } else {   // no partition given: the built-in partitioner (the reference calls METIS here, METIS.hpp:109-140)
        h->epart.resize(h->nT);
        partition_elements(mesh->nV, mesh->nT, mesh->T, mesh->X_rest, mesh->nParts, h->epart.data());
    }
    if (h->flags & DOTMI_FLAG_DOT_COARSE) {
        // the term of dotmi_set_dot_coarse from create on (the only way to it on a sharded handle: it changes the payload of a
        // collective, so it is fixed for the life of the communicator); what the setter refuses is refused here
        const char *why = (h->flags & DOTMI_FLAG_OWNER_EXCHANGE)
                              ? "not with DOTMI_FLAG_OWNER_EXCHANGE (its merge in front of the exchange forms z before the coarse solution y exists)"
                          : (h->flags & DOTMI_FLAG_GSDD)       ? "not with DOTMI_FLAG_GSDD (a GSDD handle solves one subdomain at a time)"
                          : (h->flags & DOTMI_FLAG_NEWTON_PCG) ? "not with DOTMI_FLAG_NEWTON_PCG (its coarse term is dotmi_set_pcg_coarse)"
                          : (h->flags & DOTMI_FLAG_NEWTON)     ? "not with DOTMI_FLAG_NEWTON (a Newton handle factorises H as one subdomain)"
                          : (h->flags & DOTMI_FLAG_LBFGS_PD)   ? "not with DOTMI_FLAG_LBFGS_PD (no Hessian block solve)"
                          : (h->flags & DOTMI_FLAG_LBFGS_HI)   ? "not with DOTMI_FLAG_LBFGS_HI (no Hessian block solve)"
                          : (h->flags & DOTMI_FLAG_ASYNC_REFRESH)
                              ? "not with DOTMI_FLAG_ASYNC_REFRESH (the build is judged with the refresh)"
                          : mesh->vpart ? "not with a vertex partition (vpart): the coarse plan works on an element partition"
                                        : nullptr;
        if (why) {
            h->err = std::string("DOTMI_FLAG_DOT_COARSE: ") + why;
            return DOTMI_E_INVALID;
        }
        if (h->nPartsAll > COARSE_MAX_PARTS) {
            h->err = "DOTMI_FLAG_DOT_COARSE: at most " + std::to_string(COARSE_MAX_PARTS) + " subdomains (the coarse matrix is applied "
                     "through a dense inverse factor); " + std::to_string(h->nPartsAll) + " were asked for";
            return DOTMI_E_INVALID;
        }
        h->coarse.dotMode = 1;   // the refresh create ends in builds A0 behind itself, as every later one
    }
    h->fixed.assign(mesh->fixed, mesh->fixed + h->nV);
    h->Xrest.assign(mesh->X_rest, mesh->X_rest + h->n);
    h->mu.assign(mesh->mu, mesh->mu + h->nT);
    h->lam.assign(mesh->lambda, mesh->lambda + h->nT);
    return 0;
}

// which loop runs on this handle (device / host, early order, vertex patches): needs the subdomains' tables (build_device_mesh)
static int choose_loop_form(dotmi_handle *h)
{
    h->gsdd = (h->flags & DOTMI_FLAG_GSDD) != 0;
    h->newton = (h->flags & (DOTMI_FLAG_NEWTON | DOTMI_FLAG_NEWTON_PCG | DOTMI_FLAG_NEWTON_PCG_DIST)) != 0;   // (Newton-PCG: the same loop, dotmi_pcg.hip for the solve)
    // (DOTMI_FLAG_NEWTON_PCG_DIST: the one Newton loop a sharded handle runs -- refactor, trial and backtrack have their sharded branches)
    if (h->newton && ((h->dist && !(h->flags & DOTMI_FLAG_NEWTON_PCG_DIST)) || h->gsdd)) {
        h->err = "DOTMI_FLAG_NEWTON: single GPU, not together with DOTMI_FLAG_GSDD";
        return DOTMI_E_INVALID;
    }
    if (h->gsdd && h->dist) {
        h->err = "DOTMI_FLAG_GSDD: single GPU only";
        return DOTMI_E_INVALID;
    }
    h->devLoop = !h->gsdd && !h->newton && !h->pd && !h->hi && !(h->flags & (DOTMI_FLAG_HOST_LOOP | DOTMI_FLAG_TIME_PHASES));
    // replicated element pass, merged tile partials: the back-solve of the next direction is issued on the trial
    // gradient, beside the controller (enqueue_loop_slot_early, dotmi_devloop.hip); sharded subdomains keep their one collective per iteration
    // (round 4: also with the sharded element pass -- the scatter of -g and H s_new then happen in pair_stats, behind the
    // gradient's all-reduce; DOTMI_EARLY_SHARDED=0 keeps the q-based order there)
    h->earlyBs = h->devLoop && h->tune.earlyBs != 0 &&
                 (h->P.mt_ptr != nullptr || h->P.splitMerge);
    if (h->owner && !(h->earlyBs && h->tune.fuseDir)) {
        h->err = "DOTMI_FLAG_OWNER_EXCHANGE needs the device loop's early order with the fused direction kernel";
        return DOTMI_E_INVALID;
    }
    // the trials' grouping of the energy partials, everywhere: the start-of-step evaluation and the fused-step trials must
    // sum E in the same grouping or an `E > E_cur` verdict can flip at rounding level (the owner exchange runs the fused
    // step on its sharded element pass too)
    if (h->earlyBs && h->tune.fuseStep && (!h->shardElems || h->owner)) h->PT.wgCap = h->PTspec.wgCap = 512;
    // vertex patches: one rank, the early order with both fused kernels (their statements are what k_elemvert.hip keeps), a
    // 256-thread back-solve launch to host the controller, every patch a workgroup of its own, its LDS within 64 KB
    h->vpFits = false;
    // (Stable Neo-Hookean only: its element work is ~1 us of a workgroup's ~12, so carrying every element 1.9 times is free; with
    // the fixed-corotational SVD the doubled element work costs what the saved launch gives -- bunny5K 1.656 -> 1.696 ms, measured)
    // (its log-regularised form as well: no SVD either, and elem_vertex_kernel<2, *> has the registers and LDS of <1, *> and no
    // scratch -- DESIGN section 4)
    const bool closedForm = h->mat == DOTMI_ENERGY_SNH || h->mat == DOTMI_ENERGY_SNH_LOG;
    if (h->earlyBs && !h->dist && h->world == 1 && h->tune.fuseStep && h->tune.fuseDir && h->tune.vertexPatches != 0 &&
        (closedForm || h->tune.vertexPatches > 0) &&
        h->P.ntiles - h->P.ntilesWide + h->P.nquad > 0 && !(h->flags & (DOTMI_FLAG_GSDD | DOTMI_FLAG_NEWTON | DOTMI_FLAG_NEWTON_PCG | DOTMI_FLAG_NEWTON_PCG_DIST | DOTMI_FLAG_HOST_LOOP))) {
        const HostVPatches HV = build_vpatches(h->nV, h->nT, h->T.data(), h->Xrest.data(), 512, 85);
        // (the kernel's static LDS counts against the 64 KB of a workgroup too)
        // the records are chosen per handle, only where their 6 PO doubles still fit: a mesh whose patches fit without them keeps
        // the one-launch form on the flat arrays (orec stays null)
        const bool rec = h->tune.operandRecords != 0 && HV.nPatches > 0 &&
                         elem_vertex_dyn_lds(HV.PV, HV.RUN, HV.PO, true) + ELEM_VERTEX_STATIC_LDS <= 64 * 1024;
        const size_t shm = HV.nPatches > 0 ? elem_vertex_dyn_lds(HV.PV, HV.RUN, HV.PO, rec) + ELEM_VERTEX_STATIC_LDS : 0;
        if (HV.nPatches > 0 && HV.nPatches <= 512 && HV.nPatches <= ELEM_NB_MAX && shm <= 64 * 1024 && HV.PO + 1 <= 256) {
            if (int rc = upload_vpatches(h, HV, h->VP, h->smVP)) return rc;
            if (rec) {
                // the owned vertices' static operands in patch order, from the flat arrays as they are on the device
                std::vector<int> vpp((size_t)h->nV + 1), vpo;
                HIPCHECK(h, hipMemcpy(vpp.data(), h->P.vp_ptr, sizeof(int) * vpp.size(), hipMemcpyDeviceToHost));
                vpo.resize((size_t)std::max(vpp[h->nV], 1));
                HIPCHECK(h, hipMemcpy(vpo.data(), h->P.vp_off, sizeof(int) * (size_t)vpp[h->nV], hipMemcpyDeviceToHost));
                h->vpRec = build_vpatch_records(HV, h->mass.data(), h->fixed.data(), vpp.data(), vpo.data());
                h->vpRecGid = vpatch_own_gid(HV);
                VpOwnRec *d = nullptr;
                if (int rc = upload(h, &d, h->vpRec)) return rc;
                h->VP.orec = d;
            }
            h->vpFits = true;
            if (h->tune.fuseLog)
                fprintf(stderr, "dotmi: vertex patches: %d patches, %.2f x the elements, up to %d owned / %d touched vertices, runs %d, %zu B LDS, operand records %s\n",
                        HV.nPatches, (double)h->VP.nSlotsUsed / std::max(1, h->nT), HV.PO, HV.PV, HV.RUN, shm, rec ? "on" : "off");
        }
    }
    return 0;
}

// the buffers of the loop chosen above
static int alloc_loop_state(dotmi_handle *h)
{
    if (h->dist) {
        // (DOTMI_FLAG_DOT_COARSE: the packet's tail c = Z^T r behind the n sums)
        const size_t nz = (size_t)h->n + dot_coarse_tail(h);
        if (int rc = dalloc(h, &h->zstage, nz)) return rc;
        HIPCHECK(h, hipMemsetAsync(h->zstage, 0, sizeof(double) * nz, h->st));   // (owner exchange: stays zero off the held set)
    }
    if (h->vpFits && h->VP.orec) {   // the pairs as records (DevLoop::hrec): zeroed once, every step starts with an empty history
        const size_t nrec = (size_t)2 * (HIST_MAX + 1) * h->n;
        if (int rc = dalloc(h, &h->hrec, nrec)) return rc;
        HIPCHECK(h, hipMemsetAsync(h->hrec, 0, sizeof(double) * nrec, h->st));
    }
    if (h->earlyBs) {
        if (int rc = dalloc(h, &h->u_old, (size_t)h->n)) return rc;
        for (int sl = 0; sl <= h->hist; ++sl) {
            if (int rc = dalloc(h, &h->MY[sl], (size_t)h->n)) return rc;
            if (int rc = dalloc(h, &h->HS[sl], (size_t)h->n)) return rc;
        }
    }
    h->logCap = std::min(h->iterCap, 10001) + 1;
    h->kindCap = 4096;
    HIPCHECK(h, hipHostMalloc((void **)&h->h_ctl, sizeof(DevLoop)));
    HIPCHECK(h, hipHostMalloc((void **)&h->h_flags, sizeof(int) * 4));
    HIPCHECK(h, hipMalloc((void **)&h->ctl, sizeof(DevLoop)));
    h->allocs.push_back(h->ctl);
    if (int rc = dalloc(h, &h->dlog, (size_t)3 * h->logCap)) return rc;
    HIPCHECK(h, hipMalloc((void **)&h->dkind, sizeof(int) * h->kindCap));
    h->allocs.push_back(h->dkind);
    return 0;
}

static int create_impl(dotmi_handle *h, const dotmi_mesh *mesh, const dotmi_params *prm, const double *x_init)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        h->err = "no HIP device available: libdotmi has no CPU fallback";
        return DOTMI_E_NOGPU;
    }
    if (!mesh || !prm || !x_init || mesh->nV <= 0 || mesh->nT <= 0 || !mesh->X_rest || !mesh->T || !mesh->mu ||
        !mesh->lambda || !mesh->fixed || mesh->nParts < 1 || prm->dt <= 0 ||
        prm->history < 1 || prm->history > HIST_MAX || prm->world < 1 || prm->rank < 0 ||
        prm->rank >= prm->world || (prm->world > 1 && !prm->comm_id && !prm->allreduce) ||
        (prm->energy != DOTMI_ENERGY_FCR && prm->energy != DOTMI_ENERGY_SNH && prm->energy != DOTMI_ENERGY_SNH_LOG)) {
        h->err = "invalid argument";
        return DOTMI_E_INVALID;
    }
    for (int e = 0; e < mesh->nT; ++e) {
        if (mesh->epart && !mesh->vpart && (mesh->epart[e] < 0 || mesh->epart[e] >= mesh->nParts)) {
            h->err = "epart out of range";
            return DOTMI_E_INVALID;
        }
        for (int k = 0; k < 4; ++k)
            if (mesh->T[4 * e + k] < 0 || mesh->T[4 * e + k] >= mesh->nV) {
                h->err = "tet index out of range";
                return DOTMI_E_INVALID;
            }
    }
    if (int rc = take_arguments(h, mesh, prm)) return rc;

    HIPCHECK(h, hipSetDevice(h->device));
    HIPCHECK(h, hipStreamCreate(&h->st));
    HIPCHECK(h, hipEventCreate(&h->ev0));
    HIPCHECK(h, hipEventCreate(&h->ev1));
    HIPCHECK(h, hipEventCreate(&h->ev2));
    HIPCHECK(h, hipEventCreate(&h->evA));
    h->timePhases = (h->flags & DOTMI_FLAG_TIME_PHASES) != 0;
    if (h->timePhases)
        for (auto &e : h->evP) HIPCHECK(h, hipEventCreate(&e));
    h->dist = h->world > 1 || (h->flags & DOTMI_FLAG_FORCE_DIST);
    h->shardElems = h->dist && (h->tune.shardElems >= 0 ? h->tune.shardElems != 0 : h->nT >= 400000);
    h->owner = h->dist && (h->flags & DOTMI_FLAG_OWNER_EXCHANGE);
    if (h->owner) {
        if (h->flags & (DOTMI_FLAG_HOST_LOOP | DOTMI_FLAG_TIME_PHASES | DOTMI_FLAG_GSDD | DOTMI_FLAG_NEWTON)) {
            h->err = "DOTMI_FLAG_OWNER_EXCHANGE: device loop only";
            return DOTMI_E_INVALID;
        }
        h->shardElems = true;   // own elements, own rows, own share of the refresh
    }
    h->arCb = prm->allreduce;
    h->arCtx = prm->allreduce_ctx;
    if (h->dist && !h->arCb) {
        ncclUniqueId id;
        if (h->world > 1) memcpy(&id, prm->comm_id, 128);
        else NCCLCHECK(h, ncclGetUniqueId(&id));
        NCCLCHECK(h, ncclCommInitRank(&h->comm, h->world, id, h->rank));
    }
    {
        void *cd = nullptr;
        HIPCHECK(h, hipMalloc(&cd, sizeof(double) * (RED_K + 8)));
        h->allocs.push_back(cd);
        h->ctrlDev = (double *)cd;
    }

    h->timeStride = h->tune.timeStride;
    if (h->flags & DOTMI_FLAG_TIME_BACKSOLVE) {
        h->evPre.resize(2 * 512);
        for (auto &e : h->evPre) HIPCHECK(h, hipEventCreate(&e));
        if (h->dist) {
            h->evAr.resize(2 * 512);
            for (auto &e : h->evAr) HIPCHECK(h, hipEventCreate(&e));
        }
    }
    host_features(h);
    h->targetGRes = host_target_gres(h);
    if (int rc = build_device_mesh(h)) return rc;
    if (!h->pd && !h->hi)
        if (int rc = pcg_build_scaling(h)) return rc;   // 1 / sqrt(dup) of dotmi_solve_hessian's preconditioner (dotmi_pcg.hip)
    const int n = h->n;
    double **vecs[] = {&h->x, &h->x_trial, &h->xn, &h->v, &h->xt, &h->g, &h->g_trial, &h->p, &h->q, &h->z,
                       &h->Hp, &h->tmpn};
    // (a sharded handle with DOTMI_FLAG_DOT_COARSE: z travels with c = Z^T r in its tail, apply_precond / the q-based slot)
    const size_t nvec = (size_t)n + 8 + dot_coarse_tail(h);
    for (double **pp : vecs) {
        if (int rc = dalloc(h, pp, nvec)) return rc;
        HIPCHECK(h, hipMemsetAsync(*pp, 0, sizeof(double) * nvec, h->st));
    }
    for (int s = 0; s <= h->hist; ++s) {
        if (int rc = dalloc(h, &h->S[s], (size_t)n)) return rc;
        if (int rc = dalloc(h, &h->Y[s], (size_t)n)) return rc;
    }
    if (int rc = dalloc(h, &h->He, (size_t)144 * std::max(h->nHessElems, 1))) return rc;
    if (int rc = dalloc(h, &h->Hval, hval_size(h->M.nnzb))) return rc;
    if (h->owner) {
        if (int rc = dalloc(h, &h->HvalOwn, hval_size(h->M.nnzb))) return rc;
        HIPCHECK(h, hipMemsetAsync(h->HvalOwn, 0, sizeof(double) * hval_size(h->M.nnzb), h->st));
    }
    if (int rc = dalloc(h, &h->partE, (size_t)4 * ELEM_NB_MAX)) return rc;   // (second half: a paired trial's full-step partials)
    double **parts[] = {&h->partR, &h->partC, &h->partS, &h->partG, &h->partGR, &h->partGC, &h->partCT, &h->partST};
    for (double **pp : parts) {
        // (partR: a step on vertex patches leaves one row of statistics per PATCH, up to 512 of them -- k_elemvert.hip)
        const size_t rows = pp == &h->partR ? 512 : NB_RED;
        if (int rc = dalloc(h, pp, rows * RED_K)) return rc;
        HIPCHECK(h, hipMemsetAsync(*pp, 0, sizeof(double) * rows * RED_K, h->st));
    }
    if (int rc = dalloc(h, &h->alpha_dev, 8)) return rc;   // (dalloc counts doubles: [0] the trial's step, [1] a paired trial's full step)
    if (int rc = dalloc(h, &h->gstage, (size_t)n + 2)) return rc;
    HIPCHECK(h, hipMemsetAsync(h->gstage, 0, sizeof(double) * ((size_t)n + 2), h->st));
    HIPCHECK(h, hipHostMalloc((void **)&h->h_partE, sizeof(double) * 2 * ELEM_NB_MAX));
    HIPCHECK(h, hipHostMalloc((void **)&h->h_partR, sizeof(double) * NB_RED * RED_K));
    HIPCHECK(h, hipHostMalloc((void **)&h->h_alpha, sizeof(double) * 8));
    if (int rc = choose_loop_form(h)) return rc;
    if (int rc = alloc_loop_state(h)) return rc;

    // Optimizer.cpp:124-184: result = data0 (+script init), v = 0, x_n = x, x~
    HIPCHECK(h, hipMemcpyAsync(h->x, x_init, sizeof(double) * n, hipMemcpyHostToDevice, h->st));
    HIPCHECK(h, hipMemcpyAsync(h->xn, h->x, sizeof(double) * n, hipMemcpyDeviceToDevice, h->st));
    launch_be_update(h->nV, h->M.fixed, h->x, h->xn, h->v, h->xt, h->dt, h->gdtsq, h->st);
    HIPCHECK(h, hipStreamSynchronize(h->st));
    // LBFGS-PD: the Laplacian's factor (LBFGSTimeStepper::precompute, :113-194); the Hessian is never assembled
    if (h->pd) return pd_factor(h);
    // DOTTimeStepper::precompute (DOTTimeStepper.cpp:150-178); an LBFGS-HI handle's refactor is H and its incomplete factor
    return refactor(h, h->x, nullptr, nullptr);
}

int dotmi_create(const dotmi_mesh *mesh, const dotmi_params *prm, const double *x_init, dotmi_handle **out)
{
    if (!out) return DOTMI_E_INVALID;
    *out = nullptr;
    dotmi_handle *h = new dotmi_handle();
    int rc = create_impl(h, mesh, prm, x_init);
    if (rc != 0) {
        g_create_error = h->err;
        dotmi_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

}  // extern "C"
