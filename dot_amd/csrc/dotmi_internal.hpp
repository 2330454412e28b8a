// dotmi_internal.hpp -- device-side data layout and kernel launch prototypes of libdotmi.
#pragma once
#include <hip/hip_runtime.h>

#include "bs_forms.hpp"        // the capacities of the back-solve's form families
#include "lbfgs_history.hpp"   // HIST_MAX
#include "merge_sum.hpp"       // MT_PAD
#include "nd_layout.hpp"
#include "tile_factor.hpp"
#include "time_integration.hpp"   // TitPlan
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

namespace dotmi {

// workgroups of the element pass when the mesh has more patches than that: what is resident at once with the prefetching
// instantiation's registers (Stable Neo-Hookean 158: three per CU; fixed-corotational with its SVD 190: two; the log-regularised
// Stable Neo-Hookean 178, the logarithm's and the division's temporaries on top of the plain form's: two as well) x 256 CUs
inline int elem_wg_cap(int mat) { return mat == 1 ? 768 : 512; }
// Every launcher's dispatch on the runtime material id names the three ids (0 fixed-corotational, 1 Stable Neo-Hookean, 2 its
// log-regularised form) and ends here on anything else: an id the kernels do not know must never run as another material's
// instantiation.  dotmi_create admits no other id, so this is a broken invariant, not an input error.
#define DM_DISPATCH_MAT(mat, CASE)              \
    switch (mat) {                              \
    case 0: CASE(0); break;                     \
    case 1: CASE(1); break;                     \
    case 2: CASE(2); break;                     \
    default: ::dotmi::unknown_material(mat);    \
    }
[[noreturn]] inline void unknown_material(int mat)
{
    fprintf(stderr, "dotmi: no kernel for material id %d\n", mat);
    abort();
}
constexpr int NB_RED = 256;     // blocks of every reducing kernel (fixed => run-to-run bit-identical sums)
constexpr int RED_K = 3 * HIST_MAX + 3;  // partial values per block
// the longest row each family of back-solve forms takes (bs_forms.hpp: the last entry of its table)
constexpr int BS_WAVE = bs_family_capacity(BSF_PACK);   // 256: rows of at most that many columns: four tiles per workgroup, one wavefront each
constexpr int BS_NARROW = bs_family_capacity(BSF_NARROW);   // 3072: longest row the 256-thread form of that kernel takes (two workgroups per
                                // CU; round 5: 2560 -> 3072 with the right-hand side of the sixth chunk's rows in LDS); longer rows go to the
                                // 512-thread form in a launch of their own
constexpr int BS_LONG = bs_family_capacity(BSF_WIDE);   // 5120: longest row (columns) the single-pass back-solve kernel holds in registers
constexpr int ELEM_NB_MAX = 8192; // most workgroups (= partial energy rows) of the element pass; beyond, workgroups loop over patches
constexpr int CHOL_NB = 64;     // tile of the inverse-Cholesky factorisation (LDS resident)

// ---- mesh + topology resident in HBM ------------------------------------------------------------
// Layout of the global Hessian's 3 x 3 blocks (round 6): blocks in groups of eight, a group's 72 doubles entry-major --
// entry e of block b at (b >> 3) * 72 + 8 e + (b & 7).  The eight lanes of a row's group in the SpMV kernels read the same entry
// of eight consecutive blocks with one instruction: 64 contiguous bytes instead of eight words 72 bytes apart.  With block-major
// storage (9 b + e, until round 5) every one of the 27 block loads of a trip touched ~80 lines per wave and the direction kernel
// spent ~7 of its ~12 us in the address path of the vector memory unit (tools/prof_dirstep.sh), not in waiting.
__host__ __device__ inline size_t hval_idx(int blk, int e) { return (size_t)(blk >> 3) * 72 + (size_t)(8 * e + (blk & 7)); }
inline size_t hval_size(int nnzb) { return (size_t)72 * (((size_t)nnzb + 7) / 8); }

struct DevMesh {
    int nV, nT, nTp;        // nTp = nT padded to 64 (SoA stride)
    int4 *T;                // nT   vertex ids
    double *A;              // [9][nTp] rest-shape inverse, SoA (coalesced per-lane loads)
    double *mu, *lam, *vol; // nT
    double *mass;           // nV
    uint8_t *fixed;         // nV
    // block-CSR of the global Hessian: vertex adjacency incl. self, ascending
    int *adj_ptr, *adj_idx;
    int nnzb;
    // per block: contributing (elem*16 + a*4 + b), ascending elem  -> deterministic gather assembly
    int *blk_ptr, *blk_ent;
    int *blk_row;           // nnzb: row vertex of each block
};

// ---- element patches of the element pass (patches.hpp) ---------------------------------------------
struct DevPatches {
    int nPatches = 0, PE = 0, PV = 0, nSlots = 0, nElem = 0;
    int wgCap = 0;                // > 0: every instantiation of the element pass uses at most this many workgroups on this handle
                                  // (one grouping of the energy partials for the start-of-step evaluation and the trials)
    ushort4 *tl = nullptr;        // nPatches*PE: patch-local vertex indices of a slot's corners (x == 0xFFFF: padding slot)
    double *A = nullptr;          // [9][nPatches*PE] rest-shape inverse in patch order, SoA
    double *mu = nullptr, *lam = nullptr, *vol = nullptr;   // nPatches*PE in patch order (0 on padding)
    double mu0 = 0.0, lam0 = 0.0;   // mu == nullptr: every element has these Lame parameters (one material: 16 B per tet not read)
    int *pv_gid = nullptr, *pv_slot = nullptr, *pv_cnt = nullptr;   // nPatches*PV, nPatches*PV, nPatches
    unsigned short *c_ptr = nullptr;   // per patch (PV+1): offsets of the vertices' corner runs
    ushort4 *epos = nullptr;          // nPatches*PE: position of a slot's four corners in their vertices' runs
    int2 *pp_rng = nullptr;       // nV: vertex v owns gpart[3*pp_rng[v].x .. 3*pp_rng[v].y)
    double *gpart = nullptr;      // 3*nSlots per-(patch, vertex) partial gradients, vertex-major
};

// ---- vertex patches (vpatches.hpp): element pass + vertex gather in one launch (k_elemvert.hip) -------------------------------------
struct VpOwnRec;   // vpatches.hpp
struct DevVPatches {
    int nPatches = 0, PE = 0, PV = 0, PO = 0, RUN = 0, nSlotsUsed = 0;
    ushort4 *tl = nullptr, *epos = nullptr;   // nPatches*PE: corners' patch-local vertex indices / positions in their vertices' runs (0xFFFF: not owned)
    double *A = nullptr;                      // [9][nPatches*PE] rest-shape inverse in patch order, SoA
    double *vol = nullptr, *volE = nullptr;   // nPatches*PE: volume (0 on padding) / the same where this patch counts the element's energy, else 0
    double *mu = nullptr, *lam = nullptr;     // nPatches*PE, or nullptr: every element has mu0 / lam0
    double mu0 = 0.0, lam0 = 0.0;
    int *pv_gid = nullptr, *pv_cnt = nullptr, *po_cnt = nullptr;   // touched vertices (owned first) / their number / the owned ones
    unsigned short *c_ptr = nullptr;          // per patch (PO+1): offsets of the owned vertices' runs
    // round 9 (DOTMI_OPERAND_RECORDS bit 0; nullptr: the flat arrays behind the vertex id): per (patch, owned vertex) one VpOwnRec
    // (vpatches.hpp) -- mass, fixed, the vertex' copy count and its first four padded right-hand-side positions; nPatches * PO
    const VpOwnRec *orec = nullptr;
};
// LDS of one elem_vertex_kernel workgroup: xs[3 PV] | gs[3][RUN] | (records: p and x~ of the owned dofs, 3 PO each) | cptr (u16)
inline size_t elem_vertex_dyn_lds(int PV, int RUN, int PO, bool rec)
{
    return sizeof(double) * ((size_t)3 * PV + (size_t)3 * RUN + (rec ? (size_t)6 * PO : 0)) + 2 * (size_t)((PO + 1 + 3) & ~3);
}
constexpr size_t ELEM_VERTEX_STATIC_LDS = sizeof(double) * (4 * RED_K + 8 + 1);   // sm, sme, sh_alpha
struct ElemVertArgs {
    const double *mass, *xt, *p, *hp;
    const double *spmv_partials;   // p.g / p.Hp partials, COLUMN-major [2][NB_RED] (launch_spmv_zp's partialsT)
    const uint8_t *fixed;
    const int *vp_ptr, *vp_off;   // the copies of a vertex in the padded right-hand sides (DevParts)
    double *rpad;
    double *partE, *partR, *alpha_out;
    double dtSq, alpha_min;
    const double *x0;             // ctl == nullptr (start of a step): evaluate here, no step, no pair ...
    double *g0;                   // ... the gradient goes here
};

// ---- factor storage -------------------------------------------------------------------------------
// A subdomain's X_s is kept by 64-row blocks (and H_s, then R, in a work buffer of the same layout: tile_factor.hpp).  Memory
// row i of block J = i / 64, column c (c0 <= c < 64 (J + 1)) is at W[off + (i - 64 J) * ld + (c - c0)].  A block only holds
// what its rows can have non-zero -- from the first column of the rows' tree node to the end of the block's diagonal tile
// (ld = 64 (J + 1) - c0) --, blocks of pure padding rows hold nothing (off = -1): the storage is ~1.2x the structural
// non-zeros the back-solve streams instead of nmax^2 per subdomain.
struct RowTile {
    long long off;
    int ld, c0;
};

// ---- two-level form of the back-solve (round 6; leaves-first layout, nd_layout.hpp) -----------------------------------------
// The factor buffer holds X_DD = chol(H_DD)^-1 of every leaf D, X_GG = the inverse of the separator complement's own factor, and in
// the separator rows' leaf columns M_GD = L_GD X_DD -- non-zero only in the rows of separator vertices NEXT TO leaf D.  One
// application:  c = M_GD r_D (panel rows, twolevel_forward_kernel) -> t_G = r_G - sum c (twolevel_rhs_kernel) -> the one-pass tile
// kernels on the leaves' and the separators' own rows (q_D = X_DD^T X_DD r_D, p_G = X_GG^T X_GG t_G) -> p_D = q_D - M_GD^T p_G
// (twolevel_backward_kernel on the per-subdomain sums psub).  The panels are read twice, everything else once.
struct DevTwoLevel {
    int on;
    int nPanels;                 // (owned subdomain, leaf) pairs with at least one coupled separator row
    int maxRows, maxCols;        // over the panels
    int nItems;                  // twolevel_forward_kernel's work items: (panel, first of eight rows)
    const int2 *item;
    const int4 *panel;           // x = first panel row, y = rows, z = ls * nmax + the leaf's first live column, w = live columns
    const long long *rowSrc;     // per panel row: offset in W of (that separator row, the panel's first column): where the
                                 // factorisation leaves it
    const long long *rowBase;    // per panel row: offset in `packed` of the row's copy (the rows of a panel one behind the other)
    double *packed;              // the panels, packed after every factorisation (twolevel_pack_kernel): what the two kernels stream
    const int *rowPos;           // per panel row: ls * nmax + the separator row's padded position
    double *cbuf;                // per panel row: c = M[row, leaf columns] . r_leaf
    const int *gPtr, *gIdx;      // per padded position (nParts * nmax + 1, CSR): the panel rows whose c is subtracted there
    double *rpad2;               // the right-hand sides with t_G in the separator positions (what the tile kernels read)
};

// ---- subdomains owned by this rank ---------------------------------------------------------------
struct DevParts {
    DevTwoLevel tl;
    int nParts;             // owned
    int nmax;               // padded scalar size of every owned dense block (multiple of 64) = its lda
    int *dofmap;            // owned * nmax: padded local position -> global scalar dof, -1 = padding
    double *W;              // factor storage of the owned subdomains (RowTile): H_s, then X_s = chol(H_s)^-1 with memory
                            // row i = row i of X_s (column-major upper factor Q = R^-1 of H_s = R^T R)
    RowTile *rt;            // owned * (nmax / 64) row blocks
    int ntiles;             // back-solve jobs, heavy first:
    int4 *tile;             //   (part, first row, tile index within the part | rows << 16, first column)
    int nquad;              // behind the ntiles one-tile jobs: nquad packs of four SMALL tiles (rows of at most BS_WAVE columns; one
                            //   wavefront each, backsolve_wave_tile), padded with empty entries (rows = 0): tile[ntiles + 4 k ..]
    int ntilesWide;         // the first ntilesWide tiles have rows of more than BS_NARROW columns (512-thread kernel)
    int maxTileLen;         // longest row of a tile in `tile` (<= BS_LONG: longer tiles are in `ltile`)
    // tiles whose rows exceed BS_LONG columns: two-phase back-solve over column chunks (k_backsolve.hip)
    int nltiles, nlwork;    // long tiles; (long tile, chunk) work items
    int4 *ltile;            // same encoding as `tile`
    int2 *lwork;            // (index into ltile, chunk)
    int maxChunks;          // chunks of the longest long tile
    double *tdots;          // nltiles * maxChunks * 64 chunk partials of the row dot products
    int4 *tileByPart;       // the register-kernel tiles grouped by part (GSDD solves one subdomain at a time)
    int4 *ltileByPart;      // the long-row tiles grouped by part, and their work items (x = index into ltileByPart)
    int2 *lworkByPart;
    int nbmax;              // max row tiles per part
    int2 *trange;           // owned * nbmax: columns [first, end) each tile of a part contributes to
    int *rp_ptr, *rp_idx;   // reduce_partial_p: per part and group of 16 columns (CSR, owned * (nmax / 16 + 1)) the tiles that hold it, ascending
    double *ppart;          // owned * nbmax * nmax partial results of the back-solve tiles
    double *psub;           // owned * nmax per-part results (padded positions)
    double *rpad;           // owned * nmax right-hand sides in padded order (zeros on the padding): what the back-solve
                            // tiles read, contiguous -- filled by build_qpad (loop) or gathered from q (launch_gemv)
    // merge: per vertex list of positions in psub (all parts on this rank), CSR over vertices
    int *vp_ptr, *vp_off;
    // the same merge straight from the tile partials: per global scalar dof (CSR mt_ptr over 3 nV) the offsets into ppart
    // that make up its value, subdomain after subdomain; the first entry of a subdomain is stored complemented (~off)
    int *mt_ptr, *mt_ent;
    // round 6: the same lists INTERLEAVED by wavefront -- entry q of the 64 consecutive dofs [64 w, 64 w + 64) is contiguous at
    // mt_il[mt_wave[w].x + 64 q + lane], q < mt_wave[w].y (the longest list of the 64; shorter ones end in MT_PAD) -- so that a
    // list load of a wave touches two 128-byte lines instead of ~34 (a lane's own list is ~17 x 4 contiguous bytes, the lanes'
    // lists lie one behind the other: every load instruction of the CSR walk strides through 64 x 68 bytes)
    int2 *mt_wave;
    int *mt_il;
    int splitMerge;         // big meshes: no such lists -- reduce_partial_p (coalesced, in the subdomains' own order) leaves psub
                            // and the merge kernels gather from it through vp_ptr / vp_off (round 4: 1 M tets, loop -2 ms)
    int *dup;               // nV (global multiplicity, DOTTimeStepper.cpp:47-56)
    // dense fill list
    int nfill;
    long long *fill_dst;    // per scalar of every 3x3 block (9 nfill): its offset in W, or -1 (not stored)
    int *fill_src;          // block index in Hval
    int npad;               // identity padding entries
    long long *pad_dst;
};

// ---- LBFGS-PD (DOTMI_FLAG_LBFGS_PD, dotmi_pd.hip / k_pd.hip): the scalar factor of the constant Laplacian -------------------------
constexpr int PD_KC = 8;   // columns per thread of an apply work item: an item covers up to 256 x PD_KC columns of a 64-row block
struct PdItem {
    int blk;          // 64-row block of X
    int cs, ce;       // its columns [cs, ce) this item reads
    int nch, first;   // two-pass blocks: chunks of the block and the (long-item) index of its first one
    long long pbase;  // offset of the item's partial z (3 per column) in DevPD::ppart
};
struct DevPD {
    int nmax = 0;                  // padded scalar size (multiple of 64)
    int *cvert = nullptr;          // nmax: padded position -> vertex, -1 = padding
    double *W = nullptr;           // X = chol(L)^-1 (RowTile blocks; the work buffer is dotmi_handle::W2)
    RowTile *rt = nullptr;         // nmax / 64 row blocks
    double *Lval = nullptr;        // L on the vertex adjacency (DevMesh::adj_ptr / adj_idx)
    int *inc_ptr = nullptr, *inc = nullptr;   // per vertex: incident (element << 2 | corner), ascending element
    long long *fill_dst = nullptr;  // per CSR entry of L: its place in the work buffer, or -1
    long long *pad_dst = nullptr;   // identity padding
    int npad = 0;
    PdItem *items = nullptr;        // nOne one-pass items, then nLong chunks of two-pass blocks
    int nOne = 0, nLong = 0;
    double *ppart = nullptr, *tdots = nullptr;
    int *mptr = nullptr;            // per vertex: the partials of its column (CSR over ment, fixed order)
    long long *ment = nullptr;
};

// ---- LBFGS-HI (DOTMI_FLAG_LBFGS_HI, dotmi_ic.hip / k_ic.hip): block IC(0) of H in the multicolour ordering of ic_plan.hpp -----------
struct DevIC {
    int nV = 0, nL = 0;             // vertices; lower blocks (edges of the vertex graph)
    int *vert = nullptr;            // nV: order position -> vertex
    int *lptr = nullptr, *lidx = nullptr;   // per position: its lower blocks' column positions, ascending
    int *lsrc = nullptr, *dsrc = nullptr;   // block of Hval behind a lower block / behind a position's diagonal
    int *pptr = nullptr, *pa = nullptr, *pb = nullptr;   // per lower block: the products L[pa] L[pb]^T, ascending position of k
    int *uptr = nullptr, *ublk = nullptr, *uvert = nullptr;   // per position: the later rows' blocks in its column / those rows' vertices
    double *F = nullptr;            // the factor: nL lower blocks (plan order), then nV lower-triangular diagonals (order position), row-major
    double *yw = nullptr;           // 3 nV: the forward sweep's result in order position
    int *flag = nullptr;            // set by a non-positive pivot
};

struct CoarseMerge;   // (below, with DevCoarse)
struct LbfgsArgs {
    int m;
    const double *s[HIST_MAX];  // chronological, oldest first
    const double *y[HIST_MAX];
    double ys[HIST_MAX];        // y_i . s_i
    double sy[HIST_MAX][HIST_MAX];  // sy[i][j] = s_i . y_j
};

// Canonical order of every host- or controller-side sum over per-block partials: SUM_CHUNKS contiguous
// chunks summed left to right, then the chunk sums left to right.  Host loop and device controller use
// the same order, so they agree bit for bit, and the dependent add chain is short enough for one wave.
constexpr int SUM_CHUNKS = 16;
template <class Get>
__host__ __device__ inline double chunked_sum(int n, Get get)
{
    const int L = (n + SUM_CHUNKS - 1) / SUM_CHUNKS;
    double tot = 0.0;
    for (int c = 0; c < SUM_CHUNKS; ++c) {
        double acc = 0.0;
        const int e = (c + 1) * L < n ? (c + 1) * L : n;
        for (int k = c * L; k < e; ++k) acc += get(k);
        tot += acc;
    }
    return tot;
}

__host__ __device__ inline int pair_band(double a0) { return a0 < 0.7 ? 0 : (a0 < 0.9 ? 1 : 2); }

struct XiArgs {
    double xi[HIST_MAX];
};

// L-BFGS loop state resident in HBM (single-GPU path).  loop_control_kernel advances it after every
// line-search trial exactly as the host loop (run_host_loop) would, and the loop kernels take their
// operands from it, so the host can enqueue iterations ahead of the device instead of synchronising
// once per trial (that round trip was ~30 us of every ~180 us iteration on bar17K).
struct DevLoop {
    int status;  // 0 running, 1 converged, 2 iteration cap, 3 line search collapsed (alpha == 0)
    int phase;   // 0: the next slot computes a new direction; 1: it retries the current one with `alpha`
    int iter, iterCap, hist, halvings, evals, slots;
    int notifyFrom;  // the controller posts {status, slots} to pinned host memory from this slot on (and at the end)
    int pad0;
    double tol, dtSq;
    double alpha;          // step of the next retry
    double E_cur, g2_cur;  // at x_cur
    double E0, g2_0;       // after initX (start of the step)
    double *x_cur, *x_trial, *g_cur, *g_trial;
    int slot;              // free history slot that receives the pair of the running trial
    int order[HIST_MAX + 1];
    double b[HIST_MAX];    // s_i . g_cur
    LbfgsArgs L;           // chronological view of the stored pairs (pointers, ys, sy)
    XiArgs X;              // first half of the two-loop for the next direction
    double *S[HIST_MAX + 1], *Y[HIST_MAX + 1];
    double *log_alpha, *log_E, *log_g2;
    int *slot_kind;        // per slot: 1 new direction, 2 retry (slots after the end are not logged)
    int logCap, kindCap;
    // early back-solve (enqueue_loop_slot_early): u = -M g of the accepted iterate and M y_i of the stored pairs (same slots as Y)
    int pairNew;           // the controller's last accept stored a pair (its M y goes to MY[order[m - 1]])
    int abortEpoch;        // `slots` value of the last slot whose trial was rejected or that ended the loop: the speculative
                           // back-solve of that slot (which knows its epoch) stops when it sees it
    // Held back-solves (round 4): the tiles of a slot whose trial is EXPECTED to be rejected do not start streaming beside
    // the controller; they wait for its verdict (holdVerdict = 2 * slot + (rejected or last iterate)) and leave at once
    // when it is a rejection.  The expectation is what happened to the last trial of the same kind (first trial of an
    // iteration / retry after a halving), kept by the controller; holdNext is its forecast for the slot that follows.
    int holdEnable, holdNext, holdVerdict;
    // Paired trial: the slot evaluated alpha_0 / 2 in full and the energy at alpha_0.  alpha_0 rejected (as expected): the
    // controller goes on with the half step as if a retry slot had run.  alpha_0 acceptable: redo = 1, the next slot evaluates
    // alpha_0 in full as a plain trial (phase 1, alpha = alpha_0) and keeps the statistics of a first trial.
    int redo;
    int heldSlots, heldRejected;   // slots whose tiles were told to wait / of those, rejected (statistics)
    int pairSlots, pairRedo;       // paired slots / of those, the ones whose full step was acceptable (statistics)
    // is "alpha_0 < 1" a sign of a rejection on THIS workload?  Learned from every first trial with alpha_0 < 1, paired or not:
    // one saturating counter (0 .. 3) per band of alpha_0 (< 0.7, < 0.9, < 1); the element pass pairs when the band's counter
    // is 3 (stiff monkey: nine in ten such trials are rejected; refined horse, early steps: one in three -- there a redone
    // slot costs more than a saved retry, so the rule has to be sure)
    int pairCtr[3], pairPad;
    // two-level forecast per kind of trial (0: first trial of an iteration, 1: retry): the last two outcomes of the kind
    // select one of four saturating counters (0 .. 3, >= 2 forecasts a rejection) -- a plain "same as last time" is wrong
    // every time on the alternating pattern stiff steps show (measured: profiles/r04_hold.txt)
    int predHist[2], predCtr[2][4];
    // Speculative unit step (round 6, k_dirstep.hip): the SpMV partial rows the controller of such a step sums for alpha_0, the
    // lower bound of the clamp; statistics: new-direction slots that speculated / of those, redone with alpha_0 < 1; first trials
    // of the step / of those, the ones whose estimate was the unit step (every controller counts these two: the next step's gate)
    const double *specPartials;
    double alphaMin;
    int specSlots, specRedo, firstTrials, unitFirst;
    double *u_old, *MY[HIST_MAX + 1];
    // H s_i of the stored pairs (same slots as S): H p = H z + sum_j delta_j (H s_j), H s_new = alpha H p (spmv_zp_kernel)
    double *HS[HIST_MAX + 1];
    // Round 6: what the loop's kernels used to find by index -- S[slot], HS[order[j]], MY[order[i]] -- RESOLVED by whoever changes
    // slot / order (devloop_resolve: the host at the start of a step, the controller after an accepted trial).  Every kernel of
    // the loop starts with a read of this struct from memory another XCD wrote (~1 us per dependent scalar load): with the
    // pointers resolved and all of a kernel's loop-state loads issued in front of its first branch that is ONE round trip
    // instead of three (tools/prof_loopkern.sh: 2.9 us of the gather's 6.2 and of merge_early's 9.6 were this prologue).
    double *s_new, *y_new, *hs_new;          // S[slot], Y[slot], HS[slot]: the pair of the running trial
    // Round 9 (DOTMI_OPERAND_RECORDS bit 0, vertex patches): the pairs once more as RECORDS -- hrec[vertex][slot 0 .. HIST_MAX]
    // [component] = (s, y), 16 bytes an entry, so that elem_vertex_kernel's lane (vertex, component) reads a stored pair with one
    // 16-byte load instead of two 8-byte gathers from two arrays.  Written by that kernel beside S[slot] / Y[slot] (the flat arrays
    // stay: every other kernel reads them); nothing crosses steps (the history starts empty).  hrec == nullptr: no records.
    // rec_new = hrec + 6 slot, Lrec[i] = hrec + 6 order[i]: an entry is at [(HIST_MAX + 1) * 6 * vertex + 2 * component].
    double *hrec, *rec_new;
    const double *Lrec[HIST_MAX];
    double *my_new;                          // MY[order[m - 1]]: where M y of the newest stored pair goes (merge_early)
    const double *Lmy[HIST_MAX], *Lhs[HIST_MAX];   // chronological views like L.s / L.y: M y_i, H s_i of the stored pairs
};
// the resolved views from slot / order / L.m (host: before the state is uploaded; controller: after it has changed them)
template <class DL>
__host__ __device__ inline void devloop_resolve(DL &C)
{
    C.s_new = C.S[C.slot];
    C.y_new = C.Y[C.slot];
    C.hs_new = C.HS[C.slot];
    const int m = C.L.m;
    for (int i = 0; i < HIST_MAX; ++i) {
        C.Lmy[i] = i < m ? C.MY[C.order[i]] : nullptr;
        C.Lhs[i] = i < m ? C.HS[C.order[i]] : nullptr;
    }
    C.my_new = m > 0 ? C.MY[C.order[m - 1]] : nullptr;
    C.rec_new = C.hrec ? C.hrec + 6 * C.slot : nullptr;
    for (int i = 0; i < HIST_MAX; ++i) C.Lrec[i] = (i < m && C.hrec) ? C.hrec + 6 * C.order[i] : nullptr;
}
// owner exchange: the vertices a rank holds -- the vector kernels of the loop then visit only these (everything else is zero
// and stays zero); v == nullptr: every vertex
struct VList {
    const int *v = nullptr;
    int n = 0;
};
// the forms of the loop controller (k_loopctl.hpp; the instantiations of backsolve_ctl_kernel): plain, a step with paired trials, a
// step that takes the unit step speculatively, a step on vertex patches, a step with paired trials on vertex patches
constexpr int CTL_PLAIN = 0, CTL_PAIR = 1, CTL_SPEC = 2, CTL_VP = 3, CTL_PAIR_VP = 4;
// the controller's operands when it runs as one workgroup of another launch (launch_gemv): the kernel's argument
struct CtlArgs {
    DevLoop *ctl;
    const double *partE, *partR, *alpha_dev;
    int *flags_host;
    int nbE;
    int init;   // bit 0: the evaluation at the start of the step (nothing to decide yet); bit 1: a step with paired trials -- the
                // full step's energy partials follow partE at + 2 ELEM_NB_MAX, alpha_dev[1] > 0 marks a paired slot
};
// ... and what launch_gemv takes: the operands with the form of the controller that reads them (CTL_*: which instantiation it launches).
// The form stays out of the kernel's argument: eight bytes more there cost every back-solve launch 0.6 - 0.8 us (bar17K: 44.5 -> 45.2 us)
struct CtlLaunch {
    CtlArgs a;
    int form;
};

// ---- kernel launchers (k_*.hip) ------------------------------------------------------------------
// Launchers with a trailing `ctl` run in device-loop mode when it is non-null: operands that change from
// iteration to iteration come from *ctl and the kernel returns at once when the loop has ended (or, for
// the direction kernels, when the slot is a line-search retry).
// The operands of the loop's long launchers are host-side records (never kernel parameters): defaults in the struct, the call sites
// name what differs; the builders of dotmi_handle.hpp fill them from the handle.
// x = x0 + alpha * p; alpha = clamp(-pg/pHp) from the SpMV partials when there are any
struct StepForwardArgs {
    const double *x0 = nullptr, *p = nullptr;
    double *x = nullptr;
    const double *spmv_partials = nullptr;   // nullptr: step with `alpha`
    double alpha = 0.0, alpha_min = 0.0;
    double *alpha_out = nullptr, *alpha_out_host = nullptr;
    VList vl;                                // owner exchange: the vertices visited
};
void launch_step_forward(int n, const StepForwardArgs &a, hipStream_t st, const DevLoop *ctl = nullptr);
// element pass: partial energy sums (+ inertia) and, optionally, element gradients
// grad != 0: the per-(patch, vertex) partial gradients go to PT.gpart (read by launch_vertex_gather)
// step (device loop only): the line-search step x_trial = x_cur + alpha p is taken inside the element pass
// (alpha from the SpMV partials as in launch_step_forward) instead of by a launch of its own
struct StepArgs {
    const double *p, *spmv_partials;
    double *alpha_out;       // [0] the step of the trial the gather and the controller work on, [1] paired trial: the full step (else 0)
    // alpha_min < 0: PAIRED launch (DOTMI_PAIR_TRIALS, elem_patch_kernel) with the lower bound -alpha_min -- twice as many
    // workgroups; when the step estimate alpha_0 is below 1 -- the first trial is then rejected nine times out of ten on
    // back-tracking workloads -- the first half evaluates alpha_0 / 2 in full and the second half the ENERGY at alpha_0, into the
    // second half of the partials array (+ 2 ELEM_NB_MAX).  (Packed into the sign: every byte added to the kernel arguments of the
    // loop's kernels showed up as time -- profiles/r05_paired_trials.txt F.)
    double alpha_min;
};
struct ElemPassArgs {
    const double *x = nullptr, *xt = nullptr;
    int v0 = 0, v1 = 0;             // vertex range whose inertia term this launch adds
    int grad = 0;
    double *partials = nullptr;
    const StepArgs *step = nullptr;
    bool pair = false;              // the PAIR instantiations (a step with paired trials): StepArgs::alpha_min < 0 makes it a paired launch
};
// returns the blocks of energy partials written
int launch_elem_pass(const DevMesh &M, const DevPatches &PT, int mat, double dtSq, const ElemPassArgs &a, hipStream_t st,
                     const DevLoop *ctl = nullptr);
// vertex gather of element gradients + inertia; optional L-BFGS pair + stats partials
struct GatherArgs {
    const double *x, *xt, *g_old, *p, *alpha_dev;
    double *g_new, *s_new, *y_new;
    int make_pair;
    int iv0, iv1;  // vertex range whose inertia term m_v (x_v - x~_v) this rank adds
    int stage;     // device loop, sharded element pass: g_new is a staging buffer (kept as passed), no pair
    // early back-solve: -g is also written straight into the padded right-hand sides of every subdomain that holds the
    // vertex (DevParts::vp_ptr / vp_off), so no build_qpad launch stands between the gather and the back-solve
    const int *vp_ptr, *vp_off;
    double *rpad;
    const double *hp;   // early order with the fused direction kernel: H p of the running trial; H s_new = alpha H p goes to
                        // DevLoop::HS[slot] beside s_new
    // owner exchange (DOTMI_FLAG_OWNER_EXCHANGE): this rank adds the inertia term of the vertices it OWNS (instead of a slice
    // [iv0, iv1)) and pair_stats sums its statistics over them only (every vertex counted once over the ranks)
    const uint8_t *ownMask;
    const int *vlist;   // owner exchange: the held vertices (the gather and pair_stats visit only these); nullptr: all
    int nlist;
    // owner exchange with the statistics in the gradient's packet (pre = 1): on the vertices only this rank holds the gather does
    // its whole work (the gradient is complete there); on the shared ones (kind bit 1) this rank's part of the gradient goes to
    // `gshare` and its share of the sums that are linear in the gradient to the partials; pair_stats visits them after the exchange
    const uint8_t *kind;
    int pre;
    double *gshare;
    int wide = -1;      // DOTMI_WIDE_FORMS (Tuning::wideForms): -1 the form by the number of dofs, else the mask whose bit 1 forces it (loop_forms.hpp)
};
void launch_vertex_gather(const DevMesh &M, const DevPatches &PT, const GatherArgs &a, const LbfgsArgs &L,
                          double *partials, hipStream_t st, const DevLoop *ctl = nullptr);
// pair + statistics from already summed gradients (multi-GPU: after the all-reduce of g)
void launch_pair_stats(int n, const GatherArgs &a, const LbfgsArgs &L, double *partials, hipStream_t st,
                       const double *gsrc = nullptr, const DevLoop *ctl = nullptr);
// two-loop, first half:  b_i = s_i . g  partials
void launch_multidot(int n, const double *v, const double *const *vecs, int m, double *partials,
                     hipStream_t st);
// q = -g - sum_j xi_j y_j with xi from partials (b) and SY
void launch_build_q(int n, const double *g, const LbfgsArgs &L, const double *xi_host, double *q,
                    hipStream_t st, const DevLoop *ctl = nullptr);
// subdomain back-solve: psub_s = X_s^T (X_s q[dofmap_s])
// q == nullptr: P.rpad already holds the right-hand sides (launch_build_qpad); else they are gathered from q first
// ca: the loop controller runs as workgroup 0 of the (first) launch, beside the tiles, which then ignore the retry phase
// (the back-solve is speculative: issued on the trial gradient before the controller has accepted the trial); ca->form says which
// controller (CtlLaunch): paired slots (CtlArgs::init bit 1), the unit step taken speculatively (DevLoop::specPartials), statistics in one row
// per vertex patch (CtlArgs::nbE rows)
void launch_gemv(const DevParts &P, const double *q, hipStream_t st, const DevLoop *ctl = nullptr,
                 hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, const CtlLaunch *ca = nullptr, int spec = 0);
// (a.alpha_min < 0: a PAIRED launch -- twice as many workgroups, the second half the energy of the full step: StepArgs::alpha_min)
void launch_elem_vertex(const DevVPatches &VP, int mat, const ElemVertArgs &a, hipStream_t st, const DevLoop *ctl);
bool dirstep_fits(const DevPatches &PT);   // (meshes of at most 512 patches: every patch a workgroup)
// rpad_s[k] = q[dofmap_s[k]] with q = -g - sum_j xi_j y_j formed on the fly (same operations as build_q), 0 on padding
// spec (device loop, early back-solve): 1: rpad = -g_cur, 2: rpad = -g_trial whatever the phase; no history terms
void launch_build_qpad(const DevParts &P, const double *g, const LbfgsArgs &L, const double *xi_host, hipStream_t st,
                       const DevLoop *ctl = nullptr, int spec = 0);
void launch_reduce_partial(const DevParts &P, hipStream_t st, const DevLoop *ctl = nullptr);
void launch_twolevel_pack(const DevParts &P, hipStream_t st);   // after a factorisation (two-level form): the panels' rows -> P.tl.packed
// early back-solve: u = merge(tile partials) / dup = -M g;  M y of the newest pair = u_old - u;  z = u - sum_j xi_j M y_j
// (+ partial dots y_i . z).  Device loop only.  The call sites name what differs from the defaults: {.z = ..., .first = 1, ...}
struct MergeEarlyArgs {
    double *z = nullptr;
    double *partials = nullptr;         // the y_i . z, row-major [NB_RED][RED_K]; nullptr: none (they came with the packet, yz_pre_kernel)
    double *partialsT = nullptr;        // the same once more, column-major
    int first = 0;                      // start of the step: no history, u_old is only set
    const double *zsum = nullptr;       // the all-reduced sum (over all ranks' subdomains) of the undivided partial merges, in a staging
                                        // buffer: the division and the history terms are left.  nullptr: the kernel merges the tiles
    const uint8_t *ownMask = nullptr;   // owner exchange: the y_i . z partials over the vertices this rank owns only
    VList vl;                           // owner exchange: the vertices visited
    // owner exchange with the y_i . z in the packet (pre = 1, zsum = nullptr): before the exchange the whole work on the vertices only this
    // rank holds; on the shared ones (kind bit 1) this rank's part of the sum goes to zshare and its share of y_i . z to the partials;
    // afterwards a launch over the shared vertices (zsum = the unpacked sums, partials = nullptr)
    const uint8_t *kind = nullptr;
    int pre = 0;
    double *zshare = nullptr;
    const CoarseMerge *co = nullptr;    // dotmi_set_dot_coarse: u += Z y behind the division, the COARSE instantiation
    int wide = -1;                      // DOTMI_WIDE_FORMS (Tuning::wideForms): -1 the form by the number of dofs, else the mask whose bit 2 forces it (loop_forms.hpp)
};
void launch_merge_early(const DevMesh &M, const DevParts &P, const MergeEarlyArgs &a, hipStream_t st, const DevLoop *ctl);
// owner exchange: the entries of the vertices held by more than one rank, packed / unpacked (idx: their vertex ids);
// tail: `ntail` further scalars copied from / to tailp behind the packed entries
// red0 / red1: partial arrays whose rows workgroup 0 of the pack sums into the packet's tail (pack[dst ...]): `cols` columns of
// `rows` rows, or (combine) s0 * column 0 + s1 * column 1 into one entry
struct PackRed {
    const double *part;
    int rows, stride, cols, combine, dst;
    double s0, s1;
};
void launch_pack_iface(int nI, const int *idx, const double *src, double *pack, const double *tailp, int ntail, hipStream_t st,
                       const PackRed *red0 = nullptr, const PackRed *red1 = nullptr);
// dst2 / ntail2: the tail behind the first one goes to dst2, with the squares of the packet's summed vector entries added to
// dst2[0] (|g|^2 over the shared vertices)
void launch_unpack_iface(int nI, const int *idx, const double *pack, const uint8_t *heldMask, double *dst, double *tailp, int ntail,
                         hipStream_t st, double *dst2 = nullptr, int ntail2 = 0);
// |v|^2 over the owned vertices -> column 0 of the partial rows;  v := own ? v : 0 (in place)
void launch_masked_norm2(int n, const double *v, const uint8_t *ownMask, double *partials, hipStream_t st, int exact = 0);
void launch_mask_owned(int n, double *v, const uint8_t *ownMask, hipStream_t st);
// one subdomain only (GSDD, DOTTimeStepper.cpp:507-565): psub_s = X_s^T (X_s q[dofmap_s]) for owned part `ls`, whose
// tiles are job[0..njobs); then p = 0 except p[dofs of part ls] = psub_s  (ADMMDDTimeStepper::fill, :1646-1665)
void launch_gemv_part(const DevParts &P, int ls, const int4 *job, int njobs, const int2 *lwork, int nlwork, const double *q,
                      int n, double *p, hipStream_t st);
// z = merge(tile partials, or psub) (/ dup) (+ Z y) (+ partial dots y_i . z)
struct MergeArgs {
    double *z = nullptr;
    double *partials = nullptr;        // the y_i . z (dots)
    bool dots = false;                 // accumulate the y_i . z partials
    bool divide = false;               // divide by dup (false: the undivided sum over this rank's subdomains)
    VList vl;                          // owner exchange: the vertices visited
    const CoarseMerge *co = nullptr;   // dotmi_set_dot_coarse: z += Z y behind the division, the COARSE instantiations
};
void launch_merge(const DevMesh &M, const DevParts &P, const LbfgsArgs &L, const MergeArgs &a, hipStream_t st,
                  const DevLoop *ctl = nullptr);
// partial dots y_i . z only (multi-GPU path after all-reduce)
// p = z + sum_j delta_j s_j, delta from c partials, xi and SY
void launch_build_p(int n, const double *z, const LbfgsArgs &L, const double *c_partials,
                    const double *xi_host, double *p, hipStream_t st, const DevLoop *ctl = nullptr);
// early order, one launch for build_p + spmv_dots: p = z + sum_j delta_j s_j (build_p's statements), H p = H z + sum_j
// delta_j (H s_j) from the cached H s_j, and the partial sums of p.g and p.Hp -- the only sparse product is H z, which
// does not wait for delta
struct SpmvZpArgs {
    const double *Hval = nullptr, *z = nullptr;
    const double *c_partials = nullptr;   // the y_i . z partials ...
    bool ctrans = false;                  // ... column-major (merge_early's partialsT) instead of in rows
    double *p = nullptr, *Hp = nullptr;
    double *partials = nullptr;           // p.g / p.Hp
    double *partialsT = nullptr;          // the same once more, column-major [2][NB_RED]
    int v0 = 0, v1 = -1;                  // rows [v0, v1) only for the product and the dots (sharded rows); v1 < 0: every row
    // owner exchange: the product on the rows of the vertices this rank holds (with ITS elements' part of H), p.Hp over them, p.g over
    // the vertices it owns
    const uint8_t *rowMask = nullptr, *ownMask = nullptr;
    VList vl;
    int wide = -1;                        // DOTMI_WIDE_FORMS (Tuning::wideForms): -1 the form by the number of rows, else the mask whose bit 4 forces it (loop_forms.hpp)
};
void launch_spmv_zp(const DevMesh &M, const SpmvZpArgs &a, hipStream_t st, const DevLoop *ctl);
// the direction kernel and the first trial's element pass at the unit step in one launch of two workgroup populations
// (k_dirstep.hip): replaces launch_spmv_zp + launch_elem_pass in the slots of a speculating step.  Of the two records it fuses it takes
// what its kernel has parameters for: every row, the column-major y_i . z, no twin of the p.g / p.Hp partials; the element pass at
// the step e.step on every vertex, with gradients.  Returns the blocks of energy partials
int launch_dirstep(const DevMesh &M, const DevPatches &PT, int mat, double dtSq, const SpmvZpArgs &d, const ElemPassArgs &e, hipStream_t st,
                   const DevLoop *ctl);
// Hp = H p on rows [v0,v1), partial sums of p.g and p.Hp
void launch_spmv_dots(const DevMesh &M, const double *Hval, const double *p, const double *g, double *Hp,
                      int v0, int v1, double *partials, hipStream_t st, const DevLoop *ctl = nullptr);
// one wavefront: sums the partials of the finished trial and advances *ctl (accept / halve / stop);
// flags_host (pinned, 2 ints) receives {status, slots done}.  init != 0: the partials are those of the evaluation at the
// start of the step (after initX); the controller only records E and |g|^2
void launch_loop_control(DevLoop *ctl, const double *partE, int nbE, const double *partR,
                         const double *alpha_dev, int *flags_host, hipStream_t st, int init = 0);
// element Hessians (12x12 projected), one wavefront per element in the expansion phase
// elist != null: only the listed elements (row i of He = element elist[i]);  blist != null: only the listed blocks, whose
// contribution lists blk_ptr / blk_ent then index by list position and name rows of that compact He
void launch_elem_hessians(const DevMesh &M, int mat, double dtSq, const double *x, double *He,
                          hipStream_t st, const int *elist = nullptr, int nList = 0);
// mass != null: the diagonal term comes from this array instead of the lumped masses (owner exchange: the owner's share)
void launch_assemble(const DevMesh &M, const double *He, double *Hval, hipStream_t st, const int *blist = nullptr,
                     int nList = 0, const int *blk_ptr = nullptr, const int *blk_ent = nullptr, const double *mass = nullptr);
void launch_dense_fill(const DevParts &P, const double *Hval, hipStream_t st);
// one level of the tile schedule (tile_factor.hpp): one workgroup per task
// fastDiag: the diagonal tasks' 16 x 16 bottom steps in the per-lane 8 x 8 form (k_tilefactor.hip, block_chol_inv<N, FAST>; 512 threads)
// fill / Hval: the H tiles' entry lists and the values they index (tasks with init == 2; none without the lists)
void launch_tile_level(const TileTask *tasks, int ntasks, const TileProd *prods, int *info, hipStream_t st, bool fastDiag = true,
                       const TileFillEntry *fill = nullptr, const double *Hval = nullptr);
// the non-diagonal tasks of a level on half tiles, four workgroups per CU (tile_gemm_kernel)
void launch_tile_gemm(const TileTask *tasks, int ntasks, const TileProd *prods, hipStream_t st, const TileFillEntry *fill = nullptr,
                      const double *Hval = nullptr);
void launch_tile_flow(const TileTask *tasks, int ntasks, const TileProd *prods, const int *depPtr, const int *depIdx, int *done,
                      int *next, int epoch, int *info, int nwg, hipStream_t st, double waitMs, bool fastDiag = true,
                      const TileFillEntry *fill = nullptr, const double *Hval = nullptr);
void launch_clear_tiles(double *const *tiles, const int *lds_, int ntiles, hipStream_t st);
// k_pd.hip (LBFGS-PD): L on the device, its fill into the work buffer, z = L^-1 q per coordinate
void launch_pd_assemble(const DevMesh &M, const DevPD &D, double dtSq, hipStream_t st);
void launch_pd_fill(const DevPD &D, int nnz, double *W2, hipStream_t st);
void launch_pd_apply(const DevPD &D, int nV, const double *q, double *z, hipStream_t st);
// k_ic.hip (LBFGS-HI): H's lower blocks and shifted diagonals into the factor storage; per colour [c0, c1) of order positions the
// factorisation, y = L^-1 b (b in vertex order, y in D.yw) and x = L^-T y (x in vertex order)
void launch_ic_fill(const DevIC &D, const double *Hval, double sigma, hipStream_t st);
void launch_ic_factor_colour(const DevIC &D, int c0, int c1, hipStream_t st);
void launch_ic_forward_colour(const DevIC &D, int c0, int c1, const double *b, hipStream_t st);
void launch_ic_backward_colour(const DevIC &D, int c0, int c1, double *x, hipStream_t st);
// small helpers
void launch_init_x(int nV, const uint8_t *fixed, const double *v, double dt, const double *gdtsq,
                   double *x, hipStream_t st);
void launch_be_update(int nV, const uint8_t *fixed, double *x, double *xn, double *v, double *xt,
                      double dt, const double *gdtsq, hipStream_t st);
void launch_scatter_rows(int n, const int *idx, const double *pos, double *x, hipStream_t st);
void launch_copy(int n, const double *src, double *dst, hipStream_t st);
// sharded subdomains, after the all-reduce of the merged sums: z_v /= dup_v and the y_i . z partials
// (co: + (Z y)_v behind the division, DOTMI_FLAG_DOT_COARSE)
void launch_zfinish(int nV, const int *dup, const LbfgsArgs &L, double *z, double *partials, hipStream_t st,
                    const DevLoop *ctl = nullptr, const CoarseMerge *co = nullptr);
// k_reconfig.hip (dotmi_set_lame / dotmi_set_time_step): the per-slot Lame parameters of a patch family from the global
// per-element arrays through the family's slot -> element table (padding slots, -1, get the neutral 1.0 that create gives them)
void launch_gather_lame(const int *slotElem, size_t nSlots, const double *mu, const double *lam, double *mu_s, double *lam_s,
                        hipStream_t st);
// x~ = x_n + dt v + dt^2 g on free vertices, x_n on fixed ones (Optimizer::computeXTilta, Optimizer.cpp:585-610), from the resident state
void launch_x_tilde(int nV, const uint8_t *fixed, const double *xn, const double *v, double dt, const double *gdtsq, double *xt,
                    hipStream_t st);
// ---- BDF2 (dotmi_set_time_integration; time_integration.hpp, k_timeint.hip): what a step under it launches in place of init_x / be_update ----
// the step's end: v+ from x and x^ at the effective step that ends, the shift of the two levels, the next step's x^ and x~ by `next`
void launch_bdf2_update(int nV, const uint8_t *fixed, const double *x, double *xhat, double *xn, double *v, double *xnm1, double *vnm1,
                        double *xt, double dt_eff_done, const TitPlan &next, const double *gdtsq_next, hipStream_t st);
// x^ and x~ again from the stored levels (dt, the integrator or the levels changed between two steps)
void launch_bdf2_predict(int nV, const uint8_t *fixed, const double *xn, const double *v, const double *xnm1,
                         const double *vnm1, double *xhat, double *xt, const TitPlan &p, const double *gdtsq, hipStream_t st);
// the start iterate: x = x~ on free vertices
void launch_bdf2_init_x(int nV, const uint8_t *fixed, const double *xt, double *x, hipStream_t st);

// ---- Newton-PCG (DOTMI_FLAG_NEWTON_PCG, dotmi_solve_hessian; dotmi_pcg.hip / k_pcg.hip): conjugate gradients on H with the block solve ----
// the scalars of a CG iteration, one record per parity of the iteration (k_pcg.hip)
enum { PCG_RUNNING = 0, PCG_CONVERGED = 1, PCG_BREAKDOWN = 2 };
struct PcgRec {
    double gamma, alpha;   // r.w and the step of iteration `iter`
    double rr;             // |r|^2: after iteration `iter` once the solve has ended, after iteration iter - 1 while it runs
    double bb;             // |b|^2
    int iter;              // iterations done
    int state;             // PCG_*
    int pad[6];
};
static_assert(sizeof(PcgRec) == 64, "two records and the |r|^2 columns are read back as one block");
struct DevPcg {
    PcgRec *rec = nullptr;       // [2], and behind them partBT: what the host reads once per batch (PCG_READBACK doubles)
    double *partBT = nullptr;    // [2][NB_RED]: the |r|^2 partials of the even / odd iterations, column-major (write_partials' partialsT)
    double *partAT = nullptr;    // [2][NB_RED]: the gamma / delta partials of the running iteration, column-major
    double *partA = nullptr, *partB = nullptr;   // their row-major twins (NB_RED x RED_K)
    double *isd = nullptr;       // nV: 1 / sqrt(dup)
    double *r = nullptr, *d = nullptr, *Hd = nullptr, *w = nullptr, *s = nullptr;   // 3 nV each, allocated by the first solve
    double *pkt = nullptr;       // sharded Hessian rows: the packet [s (3 nV) | gamma | delta] the ranks sum (first solve; null otherwise)
};
constexpr int PCG_READBACK = 2 * (int)(sizeof(PcgRec) / sizeof(double)) + 2 * NB_RED;
void launch_pcg_init(const DevPcg &C, int n, const double *b, double *u, double *q, hipStream_t st);
void launch_pcg_spmv(const DevMesh &M, const DevPcg &C, const double *Hval, const double *zsum, int it, hipStream_t st);
void launch_pcg_update(const DevPcg &C, int n, double *u, double *q, int it, double rel_tol, hipStream_t st);
// sharded Hessian rows: w whole, s and the gamma / delta partials on the rows [v0, v1) into C.pkt / partA; the update that reads the summed packet
void launch_pcg_spmv_rows(const DevMesh &M, const DevPcg &C, const double *Hval, const double *zsum, int v0, int v1, int it, hipStream_t st);
void launch_pcg_update_packet(const DevPcg &C, int n, double *u, double *q, int it, double rel_tol, hipStream_t st);

// ---- the rigid-mode coarse space of Newton-PCG's preconditioner (dotmi_set_pcg_coarse; dotmi_coarse.hip / k_coarse.hip; lists:
// coarse_plan.hpp): M = M_sym + Z A0^-1 Z^T, A0 = Z^T H Z, six columns of Z per subdomain -------------------------------------------
constexpr int COARSE_MAX_PARTS = 256;   // A0^-1 is kept as a dense inverse factor: nc = 6 nParts <= 1536 (a storage choice)
constexpr int COARSE_NC_MAX = 6 * COARSE_MAX_PARTS;
struct DevCoarse {
    int nParts = 0, nc = 0, ncp = 0, nPairs = 0;   // subdomains; 6 nParts; nc padded to a multiple of 64; coupled pairs (s <= t)
    int *vsPtr = nullptr, *vsIdx = nullptr;        // per vertex: its subdomains, ascending
    int *svPtr = nullptr, *svIdx = nullptr;        // per subdomain: its vertices, ascending
    int2 *pair = nullptr;                          // (s, t) of every pair
    int *pairPtr = nullptr, *pairBlk = nullptr;    // per pair: the H blocks of its sum, ascending
    int *pairAt = nullptr;                         // nParts x nParts: the pair of (s, t), s <= t, or -1
    int *live = nullptr;                           // per subdomain: 0 = dropped (fewer than 3 free vertices): zero columns, identity block
    double *wgt = nullptr;                         // nV: 1 / dup on free vertices, 0 on fixed ones
    double *xf = nullptr, *cen = nullptr;          // the positions (3 nV) and centroids (3 nParts) frozen with the last build
    double *pairA = nullptr;                       // 36 per pair: A0_st, row-major
    double *W = nullptr, *W2 = nullptr;            // ncp x ncp, row-major: X = chol(A0)^-1 (lower triangular) / the work buffer (A0, then R)
    double *c = nullptr, *y = nullptr;             // the running application: Z^T r (ncp) and A0^-1 Z^T r as the parts of the ncp / 64 row
                                                   // blocks of X ((ncp / 64) x ncp; the prolongation adds them)
    int *info = nullptr;                           // the factorisation's pivot report
    // dotmi_set_dot_coarse: the restriction from the padded right-hand sides (DevParts::rpad / dofmap / nmax of the same handle)
    int nmax = 0;
    const int *dofmap = nullptr;
    double4 *rtab = nullptr;                       // nOwn * nmax: (w_v, k_0, k_1, k_2) per padded position (coarse_rtab_kernel)
    // the handle's own subdomains [p0, p0 + nOwn) -- all of them on one rank --: the padded ranges above are theirs, by local index
    int p0 = 0, nOwn = 0;
    // the pairs (s, t), s <= t, this handle assembles: those with s in [as0, as1) -- every pair, unless the Hessian refresh is sharded
    // (then [p0, p0 + nOwn), and pairA is summed over the ranks)
    int as0 = 0, as1 = 0;
    // dotmi_set_dot_coarse_mode, mode 2 (the balanced form): W = H Z as a table of 3 x 6 blocks, one per (vertex, subdomain) entry of
    // coarse_plan.hpp's CoarseHzPlan; nothing of it exists until mode 2 is switched on for the first time
    int nHz = 0;                                        // entries
    int *hzPtr = nullptr, *hzSub = nullptr;             // per vertex: the subdomains of its entries, ascending
    int *hzVert = nullptr;                              // per entry: its vertex
    int *hzBlkPtr = nullptr, *hzBlk = nullptr;          // per entry: its H blocks, ascending (the summation order of coarse_hz_kernel)
    int *hzTPtr = nullptr, *hzTEnt = nullptr;           // per subdomain: its entries in ascending vertex
    double *hz = nullptr;                               // 18 per entry: W[i, t], row-major 3 x 6, rebuilt with A0
    double *cd = nullptr;                               // ncp: Z^T r - W^T u, what the second solve of an application reads
    double *r1 = nullptr;                               // n: the deflated right-hand side r - W y1
};
// what a merge kernel's COARSE instantiation needs for the prolongation  u_v += w_v sum_{s holds v} (t_s + omega_s x (x_v - c_s))
struct CoarseMerge {
    const int *vsPtr, *vsIdx;
    const double *wgt, *xf, *cen, *ypart;
    int nc, ld;
};
void launch_coarse_centroid(const DevCoarse &C, hipStream_t st);
void launch_coarse_assemble(const DevCoarse &C, const DevMesh &M, const double *Hval, hipStream_t st);
void launch_coarse_fill(const DevCoarse &C, hipStream_t st);
void launch_coarse_restrict(const DevCoarse &C, const double *r, hipStream_t st);                       // c = Z^T r
void launch_coarse_solve(const DevCoarse &C, hipStream_t st, const double *c = nullptr);               // y = X^T (X c); c: DevCoarse::c unless given
void launch_coarse_prolong(const DevCoarse &C, int nV, const double *isd, double *zsum, hipStream_t st);   // zsum += (Z y) / isd
void launch_coarse_scale(int n, const double *a, const double *isd, double *out, hipStream_t st);       // out = a (.) isd per vertex
// dotmi_set_dot_coarse: the table of the padded restriction (once per build); c = Z^T r from the padded right-hand sides and the
// solve as kernels of the loop (ctl != nullptr: gated by its status, and by its retry phase unless spec).  c: where Z^T r is written /
// read, DevCoarse::c unless given (a sharded handle: the tail of the vector that is all-reduced between the two)
void launch_coarse_rtab(const DevCoarse &C, hipStream_t st);
void launch_coarse_restrict_pad(const DevCoarse &C, const double *rpad, hipStream_t st, const DevLoop *ctl = nullptr, int spec = 0,
                                double *c = nullptr);
void launch_coarse_solve_loop(const DevCoarse &C, hipStream_t st, const DevLoop *ctl, int spec, const double *c = nullptr);
// dotmi_set_dot_coarse_mode, mode 2: the table W = H Z (once per build, behind the centroids); c = Z^T r on a global vector as a kernel of
// the device loop's q-based order; r1 = r - W y with y the parts DevCoarse::y holds; DevCoarse::cd = c - W^T (zsum / dup).  ctl != nullptr:
// gated by the loop's status and its retry phase
void launch_coarse_hz(const DevCoarse &C, const DevMesh &M, const double *Hval, hipStream_t st);
void launch_coarse_restrict_loop(const DevCoarse &C, const double *r, hipStream_t st, const DevLoop *ctl);
void launch_coarse_deflate(const DevCoarse &C, int n, const double *r, double *r1, hipStream_t st, const DevLoop *ctl = nullptr);
void launch_coarse_restrict_hz(const DevCoarse &C, const int *dup, const double *zsum, hipStream_t st, const DevLoop *ctl = nullptr);
// host: the dense nc x nc matrix from the pairs' blocks, entry by entry as the fill kernel writes it
void coarse_dense_host(int nc, int nParts, const int *pairAt, const int *live, const double *pairA, double *A0);

}  // namespace dotmi
