// plan_check.cpp -- the host-only planning entries of dotmi_plan.cpp driven the way their Python callers drive them, as a stand-alone
// host program for the address and undefined-behaviour sanitizers (`make plan_check`; links dotmi_plan.cpp's object and nothing else).
// Per entry: the sizes pass with null arrays, the arrays pass into heap buffers of EXACTLY the reported sizes (a write past an end
// is the sanitizer's to report), and one call with an invalid argument that must return DOTMI_E_INVALID.  Two meshes built here: a
// perturbed grid bar of 735 vertices in 6 parts of dotmi_partition (separators, wide and packed back-solve tiles, two chains) and
// a 4 x 2 x 2 bar in 2 parts (the degenerate end).  One line per entry and mesh; a wrong return code ends with a non-zero status.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <vector>

#include "../../include/dotmi.h"

namespace {

int g_failed = 0;

// a heap buffer of exactly n elements (n == 0: a zero-sized allocation, still not writable)
template <class T>
struct Buf {
    std::unique_ptr<T[]> p;
    size_t n;
    explicit Buf(size_t n_, T fill = T()) : p(new T[n_]), n(n_) { std::fill(p.get(), p.get() + n, fill); }
    operator T *() { return p.get(); }
};
using I32 = Buf<int32_t>;
using I64 = Buf<int64_t>;
using U16 = Buf<uint16_t>;
using U8 = Buf<uint8_t>;
using F64 = Buf<double>;

void expect(const char *entry, const char *what, long long got, long long want)
{
    if (got == want) return;
    std::printf("FAIL %-36s %s: returned %lld, expected %lld\n", entry, what, got, want);
    ++g_failed;
}
void invalid(const char *entry, int rc) { expect(entry, "invalid argument", rc, DOTMI_E_INVALID); }

struct Mesh {
    const char *name;
    int nV = 0, nT = 0, nParts = 0;
    std::vector<double> X;
    std::vector<int32_t> T, epart;
};

// a bar of cx x cy x cz unit cells, six tets per cell (the Kuhn split: conforming across cells), the inner vertices moved by up to
// `jitter` of a cell in each direction; every tet positively oriented
Mesh grid_bar(const char *name, int cx, int cy, int cz, double jitter)
{
    Mesh M;
    M.name = name;
    const int nx = cx + 1, ny = cy + 1, nz = cz + 1;
    M.nV = nx * ny * nz;
    uint32_t seed = 12345u;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return ((seed >> 8) & 0xffff) / 65535.0 - 0.5;
    };
    auto vid = [&](int i, int j, int k) { return (i * ny + j) * nz + k; };
    M.X.resize(3 * (size_t)M.nV);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < ny; ++j)
            for (int k = 0; k < nz; ++k) {
                const bool inner = i > 0 && i < cx && j > 0 && j < cy && k > 0 && k < cz;
                const int ijk[3] = {i, j, k};
                for (int d = 0; d < 3; ++d) M.X[3 * (size_t)vid(i, j, k) + d] = ijk[d] + (inner ? 2 * jitter * rnd() : 0.0);
            }
    static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    for (int i = 0; i < cx; ++i)
        for (int j = 0; j < cy; ++j)
            for (int k = 0; k < cz; ++k)
                for (const auto &p : perm) {
                    int c[3] = {i, j, k}, t[4];
                    t[0] = vid(c[0], c[1], c[2]);
                    for (int s = 0; s < 3; ++s) {
                        ++c[p[s]];
                        t[s + 1] = vid(c[0], c[1], c[2]);
                    }
                    double e[3][3];
                    for (int s = 0; s < 3; ++s)
                        for (int d = 0; d < 3; ++d) e[s][d] = M.X[3 * (size_t)t[s + 1] + d] - M.X[3 * (size_t)t[0] + d];
                    const double det = e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                                       e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
                    if (det < 0) std::swap(t[2], t[3]);
                    M.T.insert(M.T.end(), t, t + 4);
                }
    M.nT = (int)M.T.size() / 4;
    return M;
}

// ---- the entries that take a mesh ---------------------------------------------------------------------------------------------------
void check_mesh(Mesh &M, int nParts)
{
    const int nV = M.nV, nT = M.nT;
    const int32_t *T = M.T.data();
    const double *X = M.X.data();
    char line[160];
    auto say = [&](const char *entry) { std::printf("ok   %-36s %-10s %s\n", entry, M.name, line); };

    {   // dotmi_partition
        I32 ep(nT, -1);
        expect("dotmi_partition", "rc", dotmi_partition(nV, nT, T, X, nParts, ep), 0);
        M.epart.assign(ep.p.get(), ep.p.get() + nT);
        M.nParts = nParts;
        std::vector<int> cnt(nParts, 0);
        for (int e = 0; e < nT; ++e)
            if (ep[e] >= 0 && ep[e] < nParts) ++cnt[ep[e]];
        expect("dotmi_partition", "elements in a part", std::accumulate(cnt.begin(), cnt.end(), 0), nT);
        std::vector<int32_t> bad(M.T);
        bad[5] = nV;
        invalid("dotmi_partition", dotmi_partition(nV, nT, bad.data(), X, nParts, ep));
        std::snprintf(line, sizeof line, "%d vertices, %d tets, %d parts", nV, nT, nParts);
        say("dotmi_partition");
    }
    const int32_t *ep = M.epart.data();

    I32 partSize(nParts);
    {   // dotmi_plan_rank (and dotmi_plan_shards behind it), every rank of 1, 2 and 3
        for (int world = 1; world <= 3; ++world)
            for (int rank = 0; rank < world; ++rank) {
                int32_t p0, p1, ne, v0, v1;
                expect("dotmi_plan_rank", "sizes", dotmi_plan_rank(nV, nT, T, ep, nParts, rank, world, &p0, &p1, nullptr, &ne, &v0, &v1, nullptr), 0);
                I32 elems(ne);
                expect("dotmi_plan_rank", "arrays", dotmi_plan_rank(nV, nT, T, ep, nParts, rank, world, &p0, &p1, elems, &ne, &v0, &v1, partSize), 0);
            }
        invalid("dotmi_plan_rank", dotmi_plan_rank(nV, nT, T, ep, nParts, 2, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::snprintf(line, sizeof line, "part 0: %d scalars", (int)partSize[0]);
        say("dotmi_plan_rank");
        I32 first(4);
        expect("dotmi_plan_shards", "rc", dotmi_plan_shards(nParts, partSize, 3, first), 0);
        expect("dotmi_plan_shards", "last", first[3], nParts);
        invalid("dotmi_plan_shards", dotmi_plan_shards(nParts, partSize, 0, first));
        std::snprintf(line, sizeof line, "3 ranks: parts from %d, %d, %d", (int)first[0], (int)first[1], (int)first[2]);
        say("dotmi_plan_shards");
    }

    for (int PE : {256, 512}) {   // dotmi_plan_patches
        int32_t nP, PV, nS;
        expect("dotmi_plan_patches", "sizes",
               dotmi_plan_patches(nV, nT, T, X, PE, &nP, &PV, &nS, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
        I32 elem((size_t)nP * PE), gid((size_t)nP * PV), slot((size_t)nP * PV), cnt(nP), rng(2 * (size_t)nV);
        U16 tl(4 * (size_t)nP * PE), epos(4 * (size_t)nP * PE), cptr((size_t)nP * (PV + 1));
        expect("dotmi_plan_patches", "arrays", dotmi_plan_patches(nV, nT, T, X, PE, &nP, &PV, &nS, elem, tl, epos, gid, slot, cnt, cptr, rng), 0);
        if (PE == 512) {
            invalid("dotmi_plan_patches",
                    dotmi_plan_patches(nV, nT, T, X, 100, &nP, &PV, &nS, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
            std::snprintf(line, sizeof line, "%d patches of %d, %d touched vertices at most", (int)nP, PE, (int)PV);
            say("dotmi_plan_patches");
        }
    }

    {   // dotmi_plan_vpatches, dotmi_plan_vpatch_records
        int32_t hdr[5];
        expect("dotmi_plan_vpatches", "sizes", dotmi_plan_vpatches(nV, nT, T, X, 512, 85, hdr, nullptr, nullptr, nullptr, nullptr), 0);
        const size_t nP = hdr[0], PE = hdr[1], PV = hdr[2], PO = hdr[3];
        I32 owner(nV, -1), elem(nP * PE), eown(nP * PE), runlen(nV);
        expect("dotmi_plan_vpatches", "arrays", dotmi_plan_vpatches(nV, nT, T, X, 512, 85, hdr, owner, elem, eown, runlen), 0);
        invalid("dotmi_plan_vpatches", dotmi_plan_vpatches(nV, nT, T, X, 512, 0, hdr, nullptr, nullptr, nullptr, nullptr));
        std::snprintf(line, sizeof line, "%d patches, PE %d, PV %d, PO %d, RUN %d", hdr[0], hdr[1], hdr[2], hdr[3], hdr[4]);
        say("dotmi_plan_vpatches");

        // a vertex' copies in the subdomains' padded right-hand sides: part p holds its vertices in ascending id, 3 scalars each
        std::vector<std::vector<int>> copies(nV);
        const int nmax = (*std::max_element(partSize.p.get(), partSize.p.get() + nParts) + 63) / 64 * 64;
        for (int p = 0; p < nParts; ++p) {
            std::vector<uint8_t> in(nV, 0);
            for (int e = 0; e < nT; ++e)
                if (ep[e] == p)
                    for (int k = 0; k < 4; ++k) in[T[4 * e + k]] = 1;
            int at = 0;
            for (int v = 0; v < nV; ++v)
                if (in[v]) copies[v].push_back(p * nmax + 3 * at++);
        }
        I32 vpPtr(nV + 1);
        std::vector<int32_t> vpOff;
        for (int v = 0; v < nV; ++v) {
            vpPtr[v] = (int32_t)vpOff.size();
            vpOff.insert(vpOff.end(), copies[v].begin(), copies[v].end());
        }
        vpPtr[nV] = (int32_t)vpOff.size();
        F64 mass(nV);
        U8 fixed(nV), fixed2(nV);
        for (int v = 0; v < nV; ++v) {
            mass[v] = 1.0 + 0.001 * v;
            fixed[v] = v % 11 == 0;
            fixed2[v] = v % 7 == 0;
        }
        const char *E = "dotmi_plan_vpatch_records";
        expect(E, "sizes", dotmi_plan_vpatch_records(nV, nT, T, X, 512, 85, mass, fixed, vpPtr, vpOff.data(), nullptr, hdr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
        for (uint8_t *f2 : {(uint8_t *)nullptr, (uint8_t *)fixed2}) {
            I32 gid(nP * PV), po(nP), rf(nP * PO), rc(nP * PO), ro(4 * nP * PO);
            F64 rm(nP * PO);
            expect(E, "arrays", dotmi_plan_vpatch_records(nV, nT, T, X, 512, 85, mass, fixed, vpPtr, vpOff.data(), f2, hdr, gid, po, rm, rf, rc, ro), 0);
        }
        invalid(E, dotmi_plan_vpatch_records(nV, nT, T, X, 512, 85, nullptr, fixed, vpPtr, vpOff.data(), nullptr, hdr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::snprintf(line, sizeof line, "%d records, %d copies", (int)(nP * PO), (int)vpOff.size());
        say(E);
    }

    for (int two : {0, 1}) {   // dotmi_plan_tile_fill_mesh, both forms, two chains
        const char *E = "dotmi_plan_tile_fill_mesh";
        int64_t c[8];
        const int G = dotmi_plan_tile_fill_mesh(nV, nT, T, X, ep, nParts, 2, two, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        expect(E, "sizes (groups)", G, std::min(2, nParts));
        if (G < 0) continue;
        I64 tasks(10 * c[0]), clear(5 * c[1]), dst(9 * c[3]), pad(c[4]);
        I32 pos(c[2]), src(c[2]), srcs(c[3]);
        expect(E, "arrays", dotmi_plan_tile_fill_mesh(nV, nT, T, X, ep, nParts, 2, two, c, tasks, clear, pos, src, dst, srcs, pad), G);
        if (two) invalid(E, dotmi_plan_tile_fill_mesh(nV, nT, T, X, ep, 0, 2, two, c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::snprintf(line, sizeof line, "form %d: %lld tasks, %lld entries, %lld fill blocks, %d chains", (int)c[7], (long long)c[0],
                      (long long)c[2], (long long)c[3], G);
        say(E);
    }

    const int nOwnedVerts = std::accumulate(partSize.p.get(), partSize.p.get() + nParts, 0) / 3;
    for (const char *form : {"0", "1"}) {   // dotmi_plan_layout: the tree and the positions, both forms (the switch is read per call)
        setenv("DOTMI_TWO_LEVEL", form, 1);
        int32_t nn = 0, nmax = 0;
        expect("dotmi_plan_layout", "sizes", dotmi_plan_layout(nV, nT, T, X, ep, nParts, 0, nParts, -1, -1, 0, nullptr, &nn, &nmax, nullptr), 0);
        I32 nodes(6 * (size_t)nn), pos(nOwnedVerts);
        expect("dotmi_plan_layout", "arrays", dotmi_plan_layout(nV, nT, T, X, ep, nParts, 0, nParts, -1, -1, nn, nodes, &nn, &nmax, pos), 0);
        std::snprintf(line, sizeof line, "DOTMI_TWO_LEVEL=%s: %d nodes, padded size %d", form, (int)nn, (int)nmax);
        say("dotmi_plan_layout");
    }
    unsetenv("DOTMI_TWO_LEVEL");
    {
        int32_t nn = 0, nmax = 0;
        invalid("dotmi_plan_layout", dotmi_plan_layout(nV, nT, T, X, ep, nParts, 0, nParts + 1, -1, -1, 0, nullptr, &nn, &nmax, nullptr));
    }

    for (const char *rows : {"", "32"}) {   // dotmi_plan_backsolve_tiles, with the default tile height and DOTMI_TILE_ROWS
        if (*rows) setenv("DOTMI_TILE_ROWS", rows, 1);
        const char *E = "dotmi_plan_backsolve_tiles";
        int32_t c[8];
        expect(E, "sizes", dotmi_plan_backsolve_tiles(nV, nT, T, X, ep, nParts, 0, nParts, 0, nullptr, c), 0);
        I32 tiles(6 * (size_t)c[0]);
        expect(E, "arrays", dotmi_plan_backsolve_tiles(nV, nT, T, X, ep, nParts, 0, nParts, c[0], tiles, c), 0);
        if (c[0] > 1) invalid(E, dotmi_plan_backsolve_tiles(nV, nT, T, X, ep, nParts, 0, nParts, c[0] - 1, tiles, c));   // (too small a table)
        invalid(E, dotmi_plan_backsolve_tiles(nV, nT, T, X, ep, nParts, 1, 0, 0, nullptr, c));
        std::snprintf(line, sizeof line, "%s%s%d tiles: %d wide, %d narrow, %d packs, %d long", *rows ? "DOTMI_TILE_ROWS=" : "", *rows ? "32: " : "",
                      (int)c[0], (int)c[1], (int)c[2], (int)c[3], (int)c[4]);
        say(E);
    }
    unsetenv("DOTMI_TILE_ROWS");
    {   // dotmi_plan_backsolve_forms
        const char *E = "dotmi_plan_backsolve_forms";
        int32_t c[4];
        expect(E, "sizes", dotmi_plan_backsolve_forms(0, nullptr, c), 0);
        I32 forms(6 * (size_t)c[0]);
        expect(E, "arrays", dotmi_plan_backsolve_forms(c[0], forms, c), 0);
        invalid(E, dotmi_plan_backsolve_forms(c[0] - 1, forms, c));   // (too small a table)
        invalid(E, dotmi_plan_backsolve_forms(0, nullptr, nullptr));
        std::snprintf(line, sizeof line, "%d forms, two-phase kernel %d lanes x %d rows on chunks of %d columns", (int)c[0], (int)c[1], (int)c[2], (int)c[3]);
        say(E);
    }

    {   // dotmi_plan_backsolve_form
        int32_t form = -1;
        int64_t bytes = 0;
        expect("dotmi_plan_backsolve_form", "rc", dotmi_plan_backsolve_form(nV, nT, T, X, ep, nParts, &form, &bytes), 0);
        invalid("dotmi_plan_backsolve_form", dotmi_plan_backsolve_form(nV, nT, T, X, ep, nParts, nullptr, &bytes));
        std::snprintf(line, sizeof line, "form %d, %lld bytes in one pass", (int)form, (long long)bytes);
        say("dotmi_plan_backsolve_form");
    }
    {   // dotmi_plan_ic
        int32_t s[3];
        expect("dotmi_plan_ic", "sizes", dotmi_plan_ic(nV, nT, T, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
        I32 colour(nV), pos(nV), lptr(nV + 1), lidx(s[1]), lsrc(s[1]), dsrc(nV), pptr(s[1] + 1), pa(s[2]), pb(s[2]);
        expect("dotmi_plan_ic", "arrays", dotmi_plan_ic(nV, nT, T, s, colour, pos, lptr, lidx, lsrc, dsrc, pptr, pa, pb), 0);
        invalid("dotmi_plan_ic", dotmi_plan_ic(nV, nT, T, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::snprintf(line, sizeof line, "%d colours, %d lower blocks, %d products", (int)s[0], (int)s[1], (int)s[2]);
        say("dotmi_plan_ic");
    }
    {   // dotmi_plan_coarse
        int32_t s[3];
        const char *E = "dotmi_plan_coarse";
        expect(E, "sizes", dotmi_plan_coarse(nV, nT, T, ep, nParts, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
        I32 pairS(s[0]), pairT(s[0]), pairPtr(s[0] + 1), pairBlk(s[1]), vsPtr(nV + 1), vsIdx(s[2]), svPtr(nParts + 1), svIdx(s[2]);
        expect(E, "arrays", dotmi_plan_coarse(nV, nT, T, ep, nParts, s, pairS, pairT, pairPtr, pairBlk, vsPtr, vsIdx, svPtr, svIdx), 0);
        invalid(E, dotmi_plan_coarse(nV, nT, T, ep, 257, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        invalid(E, dotmi_plan_coarse(nV, nT, T, ep, nParts - 1, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::snprintf(line, sizeof line, "%d pairs, %d entries, %d incidences", (int)s[0], (int)s[1], (int)s[2]);
        say(E);
    }
    {   // dotmi_plan_coarse_hz
        int32_t s[2];
        const char *E = "dotmi_plan_coarse_hz";
        expect(E, "sizes", dotmi_plan_coarse_hz(nV, nT, T, ep, nParts, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
        I32 hzPtr(nV + 1), hzSub(s[0]), hzVert(s[0]), hzBlkPtr(s[0] + 1), hzBlk(s[1]), hzTPtr(nParts + 1), hzTEnt(s[0]);
        expect(E, "arrays", dotmi_plan_coarse_hz(nV, nT, T, ep, nParts, s, hzPtr, hzSub, hzVert, hzBlkPtr, hzBlk, hzTPtr, hzTEnt), 0);
        invalid(E, dotmi_plan_coarse_hz(nV, nT, T, ep, 257, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        invalid(E, dotmi_plan_coarse_hz(nV, nT, T, ep, nParts - 1, s, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        invalid(E, dotmi_plan_coarse_hz(nV, nT, T, ep, nParts, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        std::snprintf(line, sizeof line, "%d entries, %d blocks", (int)s[0], (int)s[1]);
        say(E);
    }
    {   // dotmi_plan_pd
        int32_t padded = 0;
        int64_t bytes = 0;
        expect("dotmi_plan_pd", "rc", dotmi_plan_pd(nV, nT, T, X, &padded, &bytes), 0);
        invalid("dotmi_plan_pd", dotmi_plan_pd(0, nT, T, X, &padded, &bytes));
        std::snprintf(line, sizeof line, "padded size %d, %lld bytes per application", (int)padded, (long long)bytes);
        say("dotmi_plan_pd");
    }
}

// ---- the entries that take blocks of tiles ------------------------------------------------------------------------------------------
void check_blocks()
{
    char line[160];
    auto say = [&](const char *entry) { std::printf("ok   %-36s %-10s %s\n", entry, "blocks", line); };

    {   // one block in the compact layout: two banded leaves (tile rows 0-2, 4-5; row 3 dead), their separator (6, 7)
        const int nt = 8;
        U8 live(nt, 1), pat((size_t)nt * nt, 0);
        I32 c0(nt);
        live[3] = 0;
        const int leafOf[nt] = {0, 0, 0, 0, 4, 4, -1, -1};
        for (int j = 0; j < nt; ++j) {
            c0[j] = leafOf[j] < 0 ? 0 : leafOf[j];
            for (int i = c0[j]; i <= j; ++i)
                if (live[i] && live[j] && (leafOf[j] < 0 ? (i + j) % 3 != 0 || i >= 6 : j - i <= 1)) pat[(size_t)i * nt + j] = 1;
            if (live[j]) pat[(size_t)j * nt + j] = 1;
        }
        for (int eager : {1000, 2}) {
            const char *E = "dotmi_plan_tile_schedule";
            int64_t nTasks, nProds, nLev, storage, scratch;
            I64 rowOff(nt);
            I32 rowLd(nt);
            expect(E, "sizes", dotmi_plan_tile_schedule(nt, live, pat, c0, eager, 1, nullptr, nullptr, &nTasks, &nProds, &nLev, &storage, &scratch, rowOff, rowLd), 0);
            I64 tasks(11 * nTasks), prods(4 * nProds);
            expect(E, "arrays", dotmi_plan_tile_schedule(nt, live, pat, c0, eager, 1, tasks, prods, &nTasks, &nProds, &nLev, &storage, &scratch, rowOff, rowLd), 0);
            int64_t nDeps;
            expect("dotmi_plan_tile_deps", "sizes", dotmi_plan_tile_deps(nt, live, pat, c0, eager, 1, nullptr, nullptr, &nDeps), 0);
            I64 depPtr(nTasks + 1), depIdx(nDeps);
            expect("dotmi_plan_tile_deps", "arrays", dotmi_plan_tile_deps(nt, live, pat, c0, eager, 1, depPtr, depIdx, &nDeps), 0);
            expect("dotmi_plan_tile_deps", "last pointer", depPtr[nTasks], nDeps);
            if (eager == 2) {
                invalid(E, dotmi_plan_tile_schedule(0, live, pat, c0, eager, 1, nullptr, nullptr, &nTasks, &nProds, &nLev, &storage, &scratch, rowOff, rowLd));
                invalid("dotmi_plan_tile_deps", dotmi_plan_tile_deps(nt, nullptr, pat, c0, eager, 1, nullptr, nullptr, &nDeps));
                std::snprintf(line, sizeof line, "%lld tasks, %lld products, %lld levels, %lld doubles", (long long)nTasks, (long long)nProds,
                              (long long)nLev, (long long)storage);
                say(E);
                std::snprintf(line, sizeof line, "%lld edges", (long long)nDeps);
                say("dotmi_plan_tile_deps");
            }
        }
    }
    {   // the two-level form: leaves (0-1, 2-3) in front, their separator (4, 5) behind, its leaf columns in the second range
        const int nt = 6;
        U8 live(nt, 1), pat((size_t)nt * nt, 0), leaf(nt, 1);
        I32 c0(nt), c0m(nt, 0), ntm(nt, 0);
        for (int j = 0; j < nt; ++j) {
            c0[j] = j < 4 ? j / 2 * 2 : 4;
            for (int i = j < 4 ? c0[j] : 0; i <= j; ++i) pat[(size_t)i * nt + j] = 1;
        }
        pat[(size_t)1 * nt + 5] = 0;
        for (int j = 4; j < nt; ++j) {
            leaf[j] = 0;
            ntm[j] = 4;
        }
        const char *E = "dotmi_plan_tile_schedule_two_level";
        int64_t nTasks, nProds, nLev, storage;
        I64 rowOff(nt), rowOffM(nt);
        I32 rowLd(nt), rowLdM(nt);
        expect(E, "sizes", dotmi_plan_tile_schedule_two_level(nt, live, pat, c0, leaf, c0m, ntm, 2, 1, nullptr, nullptr, &nTasks, &nProds, &nLev, &storage,
                                                             rowOff, rowLd, rowOffM, rowLdM), 0);
        I64 tasks(11 * nTasks), prods(4 * nProds);
        expect(E, "arrays", dotmi_plan_tile_schedule_two_level(nt, live, pat, c0, leaf, c0m, ntm, 2, 1, tasks, prods, &nTasks, &nProds, &nLev, &storage,
                                                              rowOff, rowLd, rowOffM, rowLdM), 0);
        invalid(E, dotmi_plan_tile_schedule_two_level(nt, live, pat, c0, nullptr, c0m, ntm, 2, 1, nullptr, nullptr, &nTasks, &nProds, &nLev, &storage,
                                                      rowOff, rowLd, rowOffM, rowLdM));
        std::snprintf(line, sizeof line, "%lld tasks, %lld products, %lld levels, %lld doubles", (long long)nTasks, (long long)nProds, (long long)nLev,
                      (long long)storage);
        say(E);
    }
    {   // dotmi_plan_tile_groups
        const int64_t w[8] = {5, 5, 4, 3, 3, 2, 1, 1};
        I32 g(8);
        expect("dotmi_plan_tile_groups", "groups", dotmi_plan_tile_groups(8, w, 3, g), 3);
        expect("dotmi_plan_tile_groups", "clamped", dotmi_plan_tile_groups(8, w, 16, g), 8);
        invalid("dotmi_plan_tile_groups", dotmi_plan_tile_groups(0, w, 3, g));
        std::snprintf(line, sizeof line, "8 weights in 3 and in 16 -> 8 groups");
        say("dotmi_plan_tile_groups");
    }
    {   // several blocks in one layout: 3-5 live tile columns of 5, every second off-diagonal tile in the pattern
        const int nb = 4, nt = 5, cols[nb] = {3, 5, 4, 5};
        U8 live((size_t)nb * nt, 0), pat((size_t)nb * nt * nt, 0);
        std::vector<int32_t> fillSub;
        std::vector<int64_t> fillDst, padDst;
        std::vector<int32_t> fillSrc;
        int64_t off[nt + 1] = {0};
        for (int j = 0; j < nt; ++j) off[j + 1] = off[j] + 64ll * 64 * (j + 1);
        const int64_t tot = off[nt];
        for (int b = 0; b < nb; ++b)
            for (int j = 0; j < cols[b]; ++j) {
                live[(size_t)b * nt + j] = 1;
                padDst.push_back(b * tot + off[j] + 63ll * 64 * (j + 1) + 64 * j + 63);   // the identity padding of the diagonal tile
                for (int i = 0; i <= j; ++i) {
                    if (i < j && (i + j + b) % 2) continue;
                    pat[((size_t)b * nt + i) * nt + j] = 1;
                    for (int k = 0; k < 3; ++k) fillSub.push_back(b);
                    // 3 x 3 blocks on a grid of three inside the tile (rows and columns 0 .. 62), one scalar in five not stored
                    for (int corner = (i + 2 * j) % 5; corner < 21 * 21; corner += 37) {
                        const int r0 = 64 * j + 3 * (corner / 21), cc = 64 * i + 3 * (corner % 21);
                        for (int rc = 0; rc < 9; ++rc) {
                            const int64_t a = b * tot + off[j] + (int64_t)((r0 + rc / 3) % 64) * 64 * (j + 1) + cc + rc % 3;
                            fillDst.push_back((corner + rc) % 5 == 0 ? -1 : a);
                        }
                        fillSrc.push_back((int32_t)(fillSrc.size() % 5000));
                    }
                }
            }
        {
            const char *E = "dotmi_plan_grouped_tile_schedule";
            const int nFill = (int)fillSub.size();
            int64_t nTasks, nClear;
            const int G = dotmi_plan_grouped_tile_schedule(nb, nt, live, pat, 2, 1, 3, nullptr, &nTasks, nullptr, nullptr, nullptr, &nClear, nFill,
                                                           fillSub.data(), nullptr, nullptr);
            expect(E, "sizes (groups)", G, 3);
            I64 tasks(6 * nTasks), clear(2 * nClear);
            I32 groupOf(nb), groupLevel(G + 1), perm(nFill), start(G + 1);
            expect(E, "arrays", dotmi_plan_grouped_tile_schedule(nb, nt, live, pat, 2, 1, 3, tasks, &nTasks, groupOf, groupLevel, clear, &nClear, nFill,
                                                                fillSub.data(), perm, start), G);
            fillSub[1] = nb;
            invalid(E, dotmi_plan_grouped_tile_schedule(nb, nt, live, pat, 2, 1, 3, nullptr, &nTasks, nullptr, nullptr, nullptr, &nClear, nFill,
                                                        fillSub.data(), nullptr, nullptr));
            std::snprintf(line, sizeof line, "%lld tasks, %lld clear tiles, %d groups", (long long)nTasks, (long long)nClear, G);
            say(E);
        }
        {
            const char *E = "dotmi_plan_tile_fill";
            const int64_t nFill = (int64_t)fillSrc.size(), nPad = (int64_t)padDst.size();
            int64_t c[8];
            const int G = dotmi_plan_tile_fill(nb, nt, live, pat, 2, 1, 2, nFill, fillDst.data(), fillSrc.data(), nPad, padDst.data(), c, nullptr, nullptr,
                                               nullptr, nullptr);
            expect(E, "sizes (groups)", G, 2);
            if (G > 0) {
                I64 tasks(10 * c[0]), clear(5 * c[1]);
                I32 pos(c[2]), src(c[2]);
                expect(E, "arrays", dotmi_plan_tile_fill(nb, nt, live, pat, 2, 1, 2, nFill, fillDst.data(), fillSrc.data(), nPad, padDst.data(), c, tasks, clear,
                                                        pos, src), G);
            }
            invalid(E, dotmi_plan_tile_fill(nb, nt, live, pat, 2, 1, 2, -1, fillDst.data(), fillSrc.data(), nPad, padDst.data(), c, nullptr, nullptr, nullptr,
                                            nullptr));
            fillDst[4] = nb * tot;   // an address behind the buffer
            invalid(E, dotmi_plan_tile_fill(nb, nt, live, pat, 2, 1, 2, nFill, fillDst.data(), fillSrc.data(), nPad, padDst.data(), c, nullptr, nullptr,
                                            nullptr, nullptr));
            std::snprintf(line, sizeof line, "%lld tasks, %lld clear tiles, %lld entries of %lld fill blocks", (long long)c[0], (long long)c[1],
                          (long long)c[2], (long long)nFill);
            say(E);
        }
    }
}

}  // namespace

int main()
{
    Mesh bar = grid_bar("bar735", 20, 6, 4, 0.15), tiny = grid_bar("bar4x2x2", 4, 2, 2, 0.15);
    check_mesh(bar, 6);
    check_mesh(tiny, 2);
    check_blocks();
    if (g_failed) std::printf("plan_check: %d wrong return codes\n", g_failed);
    else std::printf("plan_check: every entry returned what it should\n");
    return g_failed ? 1 : 0;
}
