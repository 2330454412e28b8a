// dotmi_handle.hpp -- the handle behind the C ABI and what the translation units of libdotmi share (private).
//   dotmi_create.hip      setup: mesh features, the planning stages of block_plan.hpp with their uploads, buffers
//   dotmi_plan.cpp        the host-only planning entries (dotmi_plan_*, dotmi_partition): plain C++, includes neither this header nor HIP's runtime API
//   dotmi_refresh.hip     Hessian refresh + subdomain factorisation (issue / finish / asynchronous verdict)
//   dotmi_collectives.hip all-reduce (RCCL or host hook) and the owner exchange's packets
//   dotmi_loop.hip        dotmi_step, what the loop drivers share (trial, line search, block solve), host loop, GSDD, Newton
//   dotmi_devloop.hip     the device-resident L-BFGS-H loop: the stages of a slot in both orders, run_device_loop and its parts
//   dotmi_reconfig.hip    tolerance, time step, materials and the time integration rule changed on a live handle (dotmi_set_rel_tol /
//                         _time_step / _lame / _time_integration / _history; the rule itself: time_integration.hpp, kernels: k_timeint.hip)
//   dotmi_pd.hip / dotmi_ic.hip   the preconditioners of LBFGS-PD (scalar Laplacian) and LBFGS-HI (block incomplete Cholesky of H)
//   dotmi_pcg.hip         Newton-PCG: conjugate gradients on the global H with the block solve (dotmi_solve_hessian, DOTMI_FLAG_NEWTON_PCG)
//   dotmi_coarse.hip      the rigid-mode coarse space of that PCG's preconditioner (dotmi_set_pcg_coarse; lists: coarse_plan.hpp) and of
//                         DOT's own block preconditioner (dotmi_set_dot_coarse)
//   dotmi_api.hip         the remaining ABI entry points (state, kernel-level calls, probes, measurement, handle queries)
//
// Control flow mirrors (paths relative to /root/reference/src)
//   dotmi_create       Optimizer ctor (TimeStepper/Optimizer.cpp:52-196), ADMMDDTimeStepper ctor
//                      (ADMMDDTimeStepper.cpp:44-443: partition -> local maps), DOTTimeStepper ctor +
//                      precompute (DOTTimeStepper.cpp:38-178), Mesh::computeFeatures (Mesh.cpp:589-700)
//   dotmi_step         Optimizer::solve (Optimizer.cpp:327-368) -> DOTTimeStepper::fullyImplicit
//                      (DOTTimeStepper.cpp:273-346) -> solve_oneStep (:384-504) -> Optimizer::lineSearch
//                      (Optimizer.cpp:752-881) ; updateHessianAndFactor (DOTTimeStepper.cpp:349-380)
// The data path is entirely on the device; the host only sequences launches and, in the host-driven loop, evaluates the
// m x m scalar recurrences of the two-loop recursion and takes the accept / halve / converged decisions from one small
// read-back per line-search trial.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/dotmi.h"
#include "dotmi_internal.hpp"
#include "elem_math.hpp"
#include "loop_forms.hpp"
#include "partition.hpp"
#include "patches.hpp"
#include "tuning.hpp"
#include "vpatches.hpp"

namespace dotmi {

extern std::string g_create_error;

inline double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// single wave: out[j] = sum_b partials[b*stride+j]; combine: out[0] = s0*sum0 + s1*sum1   (dotmi_collectives.hip)
__global__ void reduce_rows_kernel(const double *__restrict__ partials, int nblocks, int stride, int K, double s0, double s1,
                                   int combine, double *__restrict__ out);

}  // namespace dotmi

using namespace dotmi;

struct dotmi_handle {
    Tuning tune;
#ifdef DOTMI_TEST_HOOKS
    int testIterDelta = 0;   // fault injection for tests/test_gpu_two_ranks.py (libdotmi_testhooks.so only)
    int testFailRefresh = 0, testRefreshCount = 0;   // DOTMI_TEST_FAIL_REFRESH=k: the k-th factorisation reports a bad pivot
#endif
    // configuration
    int nV = 0, nT = 0, n = 0, mat = 0, hist = 5, iterCap = 10000;
    double dt = 0, dtSq = 0, grav[3] = {0, 0, 0}, gdtsq[3] = {0, 0, 0}, relTol = 1e-5, alphaMin = 0.1;
    double targetGRes = 0, density = 0;
    int device = 0, rank = 0, world = 1, flags = 0;
    bool dist = false;  // world > 1, or DOTMI_FLAG_FORCE_DIST: subdomains (factor + back-solve) are sharded
    // element pass + SpMV rows sharded too (one more all-reduce per trial): only pays on big meshes -- for a
    // 86k-tet mesh the whole element pass is 18 us, cheaper than any collective
    bool shardElems = false;
    std::string err;

    // host copies
    std::vector<int> T, epart, vpart;
    std::vector<uint8_t> fixed;
    std::vector<double> Xrest, A, vol, mass, mu, lam;
    int nPartsAll = 0, p0 = 0, p1 = 0;  // owned global parts [p0,p1)
    std::vector<std::vector<int>> partVerts;  // all parts: ascending global vertex ids
    std::vector<int> dup;
    std::vector<NdNode> nd;                 // nested-dissection layout shared by the owned parts (root = 0)
    std::vector<std::vector<int>> partPos;  // owned parts: padded scalar position of partVerts[p][i]
    std::vector<int> partTilePtr;           // owned parts: range of each part's tiles in DevParts::tileByPart
    std::vector<int> partLworkPtr;          //   and of its long-row work items in DevParts::lworkByPart

    // device
    hipStream_t st = nullptr;
    ncclComm_t comm = nullptr;
    void (*arCb)(void *, double *, int64_t) = nullptr;   // host all-reduce hook (dotmi_params::allreduce) instead of RCCL
    void *arCtx = nullptr;
    double *arStage = nullptr;                          // pinned staging of the hook's payload
    size_t arCap = 0;
    double *ctrlDev = nullptr;                          // RED_K + 2 doubles: control scalars of a trial (rank 0's are used)
    double ctrl[RED_K + 2] = {0};                       // world > 1: [E, alpha, R[0..RED_K)] of the last trial as adopted from rank 0
    DevMesh M{};
    DevParts P{};
    int *elist = nullptr;
    // sharded once-per-step refresh (N > 1 with a sharded element pass): this rank computes the element Hessians of the
    // elements that touch its vertices only and assembles the block rows it reads only
    bool shardHess = false;
    int *hessElems = nullptr, *hessBlk = nullptr, *hessBlkPtr = nullptr, *hessBlkEnt = nullptr;
    int nHessElems = 0, nHessBlk = 0;
    // level-scheduled tile factorisation (tile_factor.hpp)
    bool tileMode = false;
    bool twoLevel = false;                       // the factors are in the two-level form (DevTwoLevel)
    TileTask *ttasks = nullptr;
    TileProd *tprods = nullptr;
    double **tclear = nullptr;
    int *tclearLd = nullptr;
    TileFillEntry *tfill = nullptr;   // DOTMI_TILE_HFILL: the H tiles' entry lists (TileSchedule::fill); the tasks carry their ranges
    bool tileHfill = false;           // the work buffer never holds H: no clear, no fill in front of the factorisation
    std::vector<long long> rtOff;   // host copy of the RowTile table (dotmi_part_matrix)
    std::vector<int> rtLd, rtC0;
    std::vector<long long> rtOffM;  // two-level form: the separators' row blocks' second range (their sub-tree's leaf columns)
    std::vector<int> rtLdM, rtC0M;
    size_t wTotal = 0;
    double *W2 = nullptr;             // tile factorisation: the work buffer (R; with tileHfill off H before it), laid out like P.W (which holds Q only)
    int nTclear = 0;
    std::vector<int> tlevelStart, tlevelDiag;
    // subdomain groups (tile_factor.hpp): group g runs the levels [tgroupLevel[g], tgroupLevel[g + 1]) of the two tables above --
    // group 0 on st, group g > 0 on stGroup[g - 1], one fork in front of all chains and one join behind them (issue_factor)
    std::vector<int> tgroupLevel;
    std::vector<hipStream_t> stGroup;
    hipEvent_t evGroupFork = nullptr;
    std::vector<hipEvent_t> evGroupJoin;
    bool tileSplit = false;
    int predState[10] = {0, 0, 1, 1, 1, 1, 1, 1, 1, 1};   // DevLoop::predHist / predCtr between the steps
    int heldSlots = 0, heldRejected = 0;                  // held back-solves of the last step (DevLoop::holdNext)
    bool tileFlow = false;            // dataflow factorisation (tile_flow_kernel)
    bool fastDiag = false;            // diagonal tasks with the per-lane 8 x 8 bottom steps (block_chol_inv<N, true>)
    int *tdepPtr = nullptr, *tdepIdx = nullptr, *tdone = nullptr, *tnext = nullptr;
    int tileEpoch = 0, nTtasks = 0, tileFlowWg = 0;
    hipStream_t stDiag = nullptr;              // side stream of the diagonal-block tasks
    std::vector<hipEvent_t> tFork, tJoin;      // per level
    double tileFlops = 0;
    DevPatches PT, PTall;   // element patches: this rank's own elements / all elements (same unless shardElems)
    // the patches a SPECULATING step works on (k_dirstep.hip): the launch pays when its three workgroup populations are resident
    // together (512 workgroups at the direction rows' register count), so where the 256-element patches are too many for that
    // (bar17K: 256 + 337 + 68) such a step takes patches of 512 elements (256 + 169 + 68).  One patch set per step -- the
    // start-of-step evaluation, the trials and the gathers of a step agree on the grouping of the energy partials.
    DevPatches PTspec;
    bool specFits = false;
    // vertex patches (vpatches.hpp): the trial's element pass + gather in one launch (k_elemvert.hip); vpFits: this handle's loop may
    // use them (one rank, early order with the fused kernels, every patch a workgroup); vpNow: the running step does (a step that
    // pairs or speculates keeps the element patches -- one patch set per step, so its energies are grouped alike)
    DevVPatches VP;
    bool vpFits = false, vpNow = false;
    // DOTMI_OPERAND_RECORDS: the host copy of VP.orec with its vertex ids (dotmi_refix rewrites the fixed flags and uploads it again)
    // and the history records DevLoop::hrec (3 nV x (HIST_MAX + 1) pairs); empty / null without the records
    std::vector<VpOwnRec> vpRec;
    std::vector<int> vpRecGid;
    double *hrec = nullptr;
    // dotmi_set_lame: per family of patches the slot -> element table (-1: padding) that upload_patches / upload_vpatches fill the
    // per-slot Lame parameters through, kept on the device, and the family's slot arrays (null until a field that is not one
    // material needs them; then kept).  PT and PTspec are entered only where they are patch sets of their own.
    struct SlotMap {
        int *elem = nullptr;
        size_t nSlots = 0;
        double *mu = nullptr, *lam = nullptr;
    };
    SlotMap smAll, smOwn, smSpec, smVP;
    int nOwnElem = 0, v0 = 0, v1 = 0;
    double *x = nullptr, *x_trial = nullptr, *xn = nullptr, *v = nullptr, *xt = nullptr;
    // dotmi_set_time_integration (time_integration.hpp): under BDF2 dt, dtSq, gdtsq above keep meaning "what the launches take", the
    // effective step of the NEXT step; dtUser is the caller's dt, dtPrev the size of the step that led from level n-1 to level n, levels
    // whether that level exists (0: the next step is a backward-Euler start step).  Backward Euler: dtUser = dt, levels = 0.  The level
    // n-1 and x^ of the next step are allocated, zeroed, by the first switch to BDF2
    int tit = TIT_BE, levels = 0;
    double dtUser = 0, dtPrev = 0;
    double *xnm1 = nullptr, *vnm1 = nullptr, *xhat = nullptr;
    double *g = nullptr, *g_trial = nullptr, *p = nullptr, *q = nullptr, *z = nullptr, *Hp = nullptr;
    double *He = nullptr, *Hval = nullptr, *tmpn = nullptr;
    double *S[HIST_MAX + 1] = {nullptr}, *Y[HIST_MAX + 1] = {nullptr};
    // early back-solve (enqueue_loop_slot_early): u = -M g of the current iterate, M y_i of the stored pairs (slots as Y)
    bool refreshPending = false;   // DOTMI_FLAG_ASYNC_REFRESH: the last step's refresh is enqueued, not yet judged / timed
    double carryHess = 0, carryFact = 0;   // device times of a refresh resolved outside dotmi_step (reported by the next step)
    bool earlyBs = false;     // possible on this handle (buffers exist)
    bool earlyNow = false;    // chosen for the running step
    int prevIters = -1, prevHalv = 0;   // last step's iterations / line-search halvings (-1: no step yet)
    double *u_old = nullptr, *MY[HIST_MAX + 1] = {nullptr};
    double *HS[HIST_MAX + 1] = {nullptr};   // H s_i of the stored pairs (fused direction kernel of the early order)
    double *partE = nullptr, *partR = nullptr, *partC = nullptr, *partS = nullptr, *partG = nullptr;
    double *partST = nullptr;   // p.g / p.Hp partials, column-major [2][NB_RED] (spmv_zp_body's partialsT): what elem_vertex_kernel reads
    double *partCT = nullptr;   // the y_i . z partials once more, column-major (write_partials' partialsT): what the one-rank loop's direction kernels read
    bool pairNow = false;       // this step's slots launch the element pass twice as wide (enqueue_loop_slot_early)
    int pairSlots = 0, pairRedo = 0;
    bool specNow = false;       // this step's new-direction slots take the unit step speculatively (launch_dirstep)
    const DevPatches &stepPT() const { return specNow ? PTspec : PT; }   // the element patches of the running step
    int specSlots = 0, specRedo = 0;
    int ctlForm = CTL_PLAIN;    // the controller in the back-solve launch of this step's slots: what pairNow / specNow / vpNow make it
    int prevFirst = 0, prevUnit = 0;   // last step's first trials / of those, the ones whose estimate alpha_0 was the unit step
    int pairState[3] = {1, 1, 1};   // DevLoop::pairCtr, carried from step to step
    double *gstage = nullptr;   // sharded element pass, device loop: [g (n) ; 0 ; E] staging buffer of the gradient all-reduce
    double *zstage = nullptr;   // sharded subdomains, early order: this rank's undivided partial merge, all-reduced in place
    // owner exchange (DOTMI_FLAG_OWNER_EXCHANGE)
    bool owner = false;
    std::vector<int32_t> firstPart;        // parts of rank r: [firstPart[r], firstPart[r + 1])
    uint8_t *ownMask = nullptr, *heldMask = nullptr;   // nV: this rank owns the vertex / holds it in one of its subdomains
    uint8_t *vkind = nullptr;              // nV: bit 0 = owned by this rank, bit 1 = held by more than one rank
    int *sharedList = nullptr;             // the vertices this rank holds together with other ranks, ascending
    int nShared = 0;
    VList shared() const { return VList{sharedList, nShared}; }
    int *ifaceIdx = nullptr;               // the vertices held by more than one rank (the same list on every rank), ascending
    int nIface = 0;
    int *heldList = nullptr;               // the held vertices, ascending: the loop's vector kernels visit only these
    int nHeld = 0;
    VList held() const { return owner ? VList{heldList, nHeld} : VList(); }
    double *xpack = nullptr;               // 3 nIface + 8 + RED_K doubles: the packed entries (+ E, + the statistics) that travel
    double *massOwn = nullptr;             // nV: lumped mass on the owned vertices, 0 elsewhere
    double *HvalOwn = nullptr;             // block-CSR values of this rank's OWN elements' part of H (+ massOwn): alpha_0's p.Hp
    int *ownBlkPtr = nullptr, *ownBlkEnt = nullptr;   // contribution lists of that assembly (over hessBlk)
    double *partGR = nullptr, *partGC = nullptr;      // all-reduced statistics / y_i.z in row 0 of a zeroed partial array
    DevMesh Mown;                          // the mesh with massOwn for mass (element pass of the owner exchange)
    double *alpha_dev = nullptr;
    int *info_dev = nullptr, *h_info = nullptr;  // per owned part: failing pivot (device / pinned copy)
    bool wDirty = false;                         // W has been through a factorisation (targeted clearing applies)
    bool poisoned = false;                       // the last factorisation failed: the factors in W are garbage
    int *didx = nullptr;
    double *dpos = nullptr;
    size_t dcap = 0;
    std::vector<int32_t> didxHost;  // last scripted index set (uploaded only when it changes)
    double *dposPinned = nullptr;
    hipEvent_t evDir = nullptr;
    std::vector<void *> allocs;
    // pinned host
    double *h_partE = nullptr, *h_partR = nullptr, *h_alpha = nullptr;
    // device-resident loop control (single-GPU path)
    bool gsdd = false;   // DOTMI_FLAG_GSDD
    bool newton = false; // DOTMI_FLAG_NEWTON
    bool pd = false;     // DOTMI_FLAG_LBFGS_PD: no subdomain block solve; the scalar factor of L below instead (dotmi_pd.hip)
    DevPD PD;
    // DOTMI_FLAG_LBFGS_HI: no subdomain block solve either; the block incomplete Cholesky factor of H below instead (dotmi_ic.hip),
    // rebuilt by every refresh.  icShift: the diagonal shift of the last successful factorisation (the next one starts from half
    // of it); icAttempts: the attempts that one took
    bool hi = false;
    DevIC IC;
    std::vector<int> icStart;   // nColours + 1: the order positions of every colour
    double icShift = 0.0;
    int icAttempts = 0;
    // DOTMI_FLAG_NEWTON_PCG: `newton` with the PCG of dotmi_pcg.hip in place of the single block-solve application, any number of
    // subdomains; DOTMI_FLAG_NEWTON_PCG_DIST: the same on sharded subdomains.  The PCG's state exists on every handle with H and the
    // block solve (dotmi_solve_hessian): isd from create, the vectors (and the sharded rows' packet) from the first solve; its iterate
    // u is the handle's p
    bool newtonPcg = false;
    DevPcg pcg;
    double *h_pcg = nullptr;                   // pinned: PCG_READBACK doubles, the records and the |r|^2 partials of a batch's end
    double pcgTol = 1e-3;                      // dotmi_set_pcg: the step's relative tolerance, iteration cap, iterations per read-back
    int pcgCap = 500, pcgEvery = 8;   // (8: the best of 1, 2, 4, 8 in profiles/newton_pcg.txt)
    long long pcgSolves = 0, pcgItersTotal = 0;   // dotmi_pcg_info
    int pcgLastIters = 0;
    double pcgLastRes = 0.0;
    // dotmi_set_pcg_coarse: the rigid-mode coarse term of the PCG's preconditioner (dotmi_coarse.hip).  Nothing of it exists until the
    // mode is switched on; every refresh of H marks the coarse matrix stale and the next solve with the mode on rebuilds it
    // dotmi_set_dot_coarse: the same term in DOT's own loop, M' = M + Z A0^-1 Z^T -- one build serves both modes.  With dotMode on the
    // build is enqueued behind every refresh of H (refactor_issue) and judged with it (refactor_finish): the pivot flag comes back
    // with the stream synchronisation the refresh takes anyway
    struct Coarse {
        int mode = 0;                 // dotmi_set_pcg_coarse: 0 off, 1 rigid modes
        int dotMode = 0;              // dotmi_set_dot_coarse: 0 off, 1 rigid modes (additive), 2 rigid modes (balanced: deflation around the block solve)
        bool hzPlanned = false;       // mode 2's lists and buffers exist (the first switch to mode 2)
        bool hzIssued = false;        // the build that is enqueued writes W (coarse_issue -> coarse_finish)
        bool hzBuilt = false;         // the last build also wrote the table W = H Z (it ran with mode 2 on)
        bool pending = false;         // a build is enqueued, its pivot flag not yet read (coarse_issue -> coarse_finish)
        bool uploaded = false;        // the device's weights and live flags are those of wgt / live below
        CoarseMerge cm{};             // the merge kernels' view of the last build (launch_merge / launch_merge_early)
        bool planned = false;         // lists, buffers and the tile schedule exist
        bool stale = true;            // H has been refreshed since the last build
        bool active = false;          // the last build's factorisation succeeded: the solves add the coarse term
        int dropped = 0;              // subdomains with fewer than 3 free vertices at the last build
        long long builds = 0;
        double lastBuildMs = 0.0;
        DevCoarse D;
        TileTask *tasks = nullptr;    // a tile schedule of its own for the one dense block (tile_factor.hpp)
        TileProd *prods = nullptr;
        std::vector<int> levelStart;
        std::vector<int> pairAt, live;   // host copies (dotmi_pcg_coarse_matrix)
        std::vector<double> wgt;
        int *h_info = nullptr;        // pinned: the pivot flag, all a refresh reads back
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
    } coarse;
    bool devLoop = false;
    DevLoop *ctl = nullptr, *h_ctl = nullptr;  // device / pinned staging
    int *h_flags = nullptr;                    // pinned: {status, slots done}, written by the controller
    double *dlog = nullptr;                    // 3 * logCap doubles
    int *dkind = nullptr;
    std::vector<int> slotTimed;                // per enqueued slot: index of its event pair in evPre, or -1
    std::vector<int> slotKind;                 // last step: kind of every enqueued slot (1 = ran a back-solve)
    int logCap = 0, kindCap = 0;
    int logPending = 0;                        // device-loop log entries not fetched yet
    int prevSlots = 0;                         // slots the previous step's loop took (enqueue-ahead horizon)
    int timeStride = 8;                        // DOTMI_FLAG_TIME_BACKSOLVE brackets every timeStride-th back-solve
    int timeCount = 0;
    int nbE = 0;
    long long mergeEntries = 0;   // tile partials the merge sums (for the byte count of dotmi_bench_kernel)
    int M_nbR() const { return NB_RED; }   // rows of the statistics partials

    // L-BFGS host state (chronological)
    int m = 0;
    int order[HIST_MAX + 1] = {0};
    double ys[HIST_MAX] = {0}, sy[HIST_MAX][HIST_MAX] = {{0}}, b[HIST_MAX] = {0};

    // logs / stats
    std::vector<double> log_alpha, log_E, log_g2;
    long long numLineSearch = 0;
    int energy_evals = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, evA = nullptr;
    // DOTMI_FLAG_TIME_PHASES: boundaries of the phases of one line-search trial (host loop: every trial ends in a
    // stream synchronisation, after which the brackets recorded since the last one are read and the events reused)
    bool timePhases = false;
    hipEvent_t evP[8] = {nullptr};
    int evPn = 0;              // boundaries recorded since the last synchronisation
    int evPslot[8] = {0};      // ms_phase slot of the interval that ENDS at boundary k (k >= 1)
    double phaseMs[DOTMI_T_COUNT] = {0};
    // the level launches of the tile factorisation are a fixed sequence on fixed pointers: captured once into a hipGraph and
    // replayed every step (removes the host launch cost between them)
    hipGraphExec_t factorGraph = nullptr;
    int graphState = 0;  // 0 = not tried, 1 = ready, -1 = capture unavailable -> direct launches
    std::vector<hipEvent_t> evPre;  // DOTMI_FLAG_TIME_BACKSOLVE: (start, stop) pairs around each back-solve
    int evUsed = 0;
    // the same flag samples the collectives of the sharded path (every timeStride-th one): (start, stop) pairs + payloads
    std::vector<hipEvent_t> evAr;
    std::vector<size_t> arTimedBytes;
    int evArUsed = 0;
    long long arCount = 0, arCallsStep = 0;
    double arBytesStep = 0;
    int64_t precond_bytes = 0;
    double flopCount = 0, factorFlops = 0;  // running counter of the recursion; FP64 flop of one factorisation
};

#define HIPCHECK(h, call)                                                                         \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                         \
            return DOTMI_E_DEVICE;                                                                \
        }                                                                                         \
    } while (0)
#define NCCLCHECK(h, call)                                                                        \
    do {                                                                                          \
        ncclResult_t r_ = (call);                                                                 \
        if (r_ != ncclSuccess) {                                                                  \
            (h)->err = std::string(#call) + ": " + ncclGetErrorString(r_);                        \
            return DOTMI_E_DEVICE;                                                                \
        }                                                                                         \
    } while (0)

namespace dotmi {

template <class T>
int dalloc(dotmi_handle *h, T **ptr, size_t count)
{
    void *p = nullptr;
    size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    HIPCHECK(h, hipMalloc(&p, bytes));
    h->allocs.push_back(p);
    *ptr = (T *)p;
    return 0;
}

template <class T>
int upload(dotmi_handle *h, T **ptr, const std::vector<T> &v)
{
    int rc = dalloc(h, ptr, v.size());
    if (rc) return rc;
    if (!v.empty()) HIPCHECK(h, hipMemcpy(*ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

// ---- shared between the translation units --------------------------------------------------------------------------
// dotmi_create.hip
int build_device_mesh(dotmi_handle *h);
double host_target_gres(const dotmi_handle *h);
LbfgsArgs lbfgs_args(const dotmi_handle *h);
// dotmi_refresh.hip
int refactor_issue(dotmi_handle *h, const double *x);
int refactor_finish(dotmi_handle *h, double *ms_hess, double *ms_fact);
int refactor(dotmi_handle *h, const double *x, double *ms_hess, double *ms_fact);
int resolve_refresh(dotmi_handle *h, double *ms_hess = nullptr, double *ms_fact = nullptr);
int enter_with_factors(dotmi_handle *h);
int run_factor(dotmi_handle *h);
// dotmi_reconfig.hip (the time integration switch, time_integration.hpp)
bool tit_apply(dotmi_handle *h, const TitPlan &p);   // dt, dtSq, gdtsq, targetGRes <- the plan's effective step; true: it changed
int tit_replan(dotmi_handle *h, bool always);        // between two steps: the plan from the handle's levels, x^ / x~ again, the refresh
// dotmi_pd.hip (LBFGS-PD)
int build_pd(dotmi_handle *h, const std::vector<int> &adj_ptr, const std::vector<int> &adj_idx);
int pd_factor(dotmi_handle *h);
int pd_apply(dotmi_handle *h, const double *q, double *z, const LbfgsArgs &L);
// dotmi_ic.hip (LBFGS-HI)
int build_ic(dotmi_handle *h, const std::vector<int> &adj_ptr, const std::vector<int> &adj_idx);
int ic_refresh(dotmi_handle *h, const double *x, double *ms_hess, double *ms_fact);
int ic_apply(dotmi_handle *h, const double *q, double *z, const LbfgsArgs &L);
// dotmi_pcg.hip (Newton-PCG)
int pcg_build_scaling(dotmi_handle *h);
int pcg_solve(dotmi_handle *h, const double *b, double rel_tol, int max_iter, int check_every, int *iters, double *rel_res);
const char *pcg_refusal(const dotmi_handle *h);   // why this handle has no global solve (nullptr: it has)
// dotmi_coarse.hip (the coarse term of the PCG's preconditioner)
int coarse_refresh(dotmi_handle *h);              // a mode on and stale: rebuild A0 and its inverse factor from the current H and x
int coarse_issue(dotmi_handle *h, const double *x);   // enqueue that build at the positions x (no synchronisation) ...
void coarse_finish(dotmi_handle *h);                  // ... and, after one, take its pivot flag and its time
// dotmi_set_dot_coarse: what the merges of a preconditioner application add (nullptr: mode off, or the last build met a bad pivot)
inline const CoarseMerge *dot_coarse(const dotmi_handle *h)
{
    const dotmi_handle::Coarse &K = h->coarse;
    return (K.dotMode == 1 && K.active && !K.stale) ? &K.cm : nullptr;
}
// mode 2, the balanced form M'' = C + (I - C H) M (I - H C): the same record, for the prolongation behind the merge (nullptr: another
// mode, or the last build met a bad pivot -- then plain M, in the early order).  One rank only (dotmi_set_dot_coarse refuses others)
inline const CoarseMerge *dot_coarse_balanced(const dotmi_handle *h)
{
    const dotmi_handle::Coarse &K = h->coarse;
    return (K.dotMode == 2 && K.active && !K.stale && K.hzBuilt) ? &K.cm : nullptr;
}
// its two halves around the block solve: y1 = A0^-1 Z^T q and the deflated right-hand side r1 = q - W y1 (returned: a buffer of the
// coarse space's own) in front; behind the merge WITHOUT the division (z = the sum over the subdomains), z = z / dup + Z A0^-1 (Z^T q -
// W^T (z / dup)) and the y_i . z partials of L into partC.  ctl: as kernels of the device loop's q-based order
const double *dot_coarse_deflate(dotmi_handle *h, const double *q, const DevLoop *ctl = nullptr);
void dot_coarse_balance(dotmi_handle *h, double *z, const LbfgsArgs &L, const DevLoop *ctl = nullptr);
// the build that a refresh with the mode off has left undone (dotmi_set_dot_coarse only: the PCG builds in its solves)
inline int dot_coarse_refresh(dotmi_handle *h) { return h->coarse.dotMode != 0 ? coarse_refresh(h) : 0; }
// c = Z^T r from the padded right-hand sides, y = A0^-1 c (ctl: as kernels of the device-resident loop; spec: the early order)
void dot_coarse_restrict_solve(dotmi_handle *h, const DevLoop *ctl = nullptr, int spec = 0);
// DOTMI_FLAG_DOT_COARSE on a sharded handle: the two halves around the iteration's collective.  The restriction of the rank's own
// subdomains goes into the dot_coarse_tail doubles behind the n of the vector that travels (zeros for the others' subdomains), the
// all-reduce of n + tail doubles makes c whole and identical on every rank, and every rank solves on it behind the collective
void dot_coarse_restrict(dotmi_handle *h, double *c, const DevLoop *ctl = nullptr, int spec = 0);
void dot_coarse_solve(dotmi_handle *h, const double *c, const DevLoop *ctl = nullptr, int spec = 0);
// what the z packet of a sharded handle carries behind its n entries: nc = 6 nParts doubles with the flag, whether the last build left
// the term active or not (the payload of a collective never depends on a rank's state), else nothing
inline size_t dot_coarse_tail(const dotmi_handle *h) { return (h->dist && h->coarse.dotMode != 0) ? (size_t)6 * h->nPartsAll : 0; }
void coarse_restrict_solve(dotmi_handle *h, const double *r);   // c = Z^T r, y = A0^-1 c
void coarse_prolong(dotmi_handle *h, double *zsum);             // zsum += (Z y) / isd
// dotmi_collectives.hip
int allreduce_sum(dotmi_handle *h, double *dev, size_t n);
int adopt_rank0(dotmi_handle *h, double *vals, int n);
int exchange_iface(dotmi_handle *h, double *vec, double *tailp, int ntail);
int exchange_gradient_packed(dotmi_handle *h, int n, int nbE, const double *partials, int ncols);
int exchange_solve_packed(dotmi_handle *h);
// the merge's sum over the ranks of a sharded handle, and what finishes it
enum RankSumEnd {
    RANKSUM_ZFINISH,       // launch_zfinish on the packet, in place (q-based order, host loop)
    RANKSUM_EARLY,         // the zsum branch of launch_merge_early into h->z (early order)
    RANKSUM_EARLY_FIRST    // ... at the start of the step (MergeEarlyArgs::first)
};
int merge_over_ranks(dotmi_handle *h, const LbfgsArgs &L, double *packet, RankSumEnd end, const DevLoop *ctl, VList vl = VList());
// dotmi_loop.hip
struct Bracket {
    hipEvent_t ev0, ev1;   // DOTMI_FLAG_TIME_BACKSOLVE: the events around a sampled back-solve, else nulls
    int at;                // index of the pair in evPre, or -1
};
struct LoopOut {           // what a loop driver (run_*_loop) hands back to dotmi_step
    double lastE = 0, g2 = 0, E0 = 0, g20 = 0;   // energy and |g|^2 of the last iterate / at the start of the step
    int it = 0;
    long long applies = 0; // Newton-PCG: block-solve applications (the CG iterations of the step's solves)
    bool failed = false;   // the line search ran out of step length
};
int apply_precond(dotmi_handle *h, const double *q, double *z, const LbfgsArgs &L);
Bracket backsolve_bracket(dotmi_handle *h);
int reduce_step_dots(dotmi_handle *h, const double **spart);
void stage_energy(dotmi_handle *h, int nb, double *dst);
// The operand records of the loop's launches (dotmi_internal.hpp), built from the handle once; the call sites set what differs.
// sharded = false: the form of a handle without a sharded element pass, whatever this one is (dotmi_bench_kernel: the sharded stages
// contain collectives, which it does not price)
inline constexpr LbfgsArgs NO_HISTORY{};   // for the launches that take no history, or the device loop's (ctl != nullptr)
GatherArgs gather_args(const dotmi_handle *h);         // what every gather of a step has in common
GatherArgs early_gather_args(const dotmi_handle *h);   // the early order's gather
ElemVertArgs elem_vertex_args(const dotmi_handle *h);
SpmvZpArgs spmv_zp_args(const dotmi_handle *h, bool sharded = true);   // the loop's direction kernel: owner exchange / one rank / sharded rows
StepForwardArgs step_forward_args(const dotmi_handle *h, const double *spmv_partials, double alpha = 0.0);   // x_trial = x + alpha p
// the running step's element pass at x: the mesh (owner exchange: every vertex, with the owner's share of the mass) and the record
struct StepElemPass {
    const DevMesh &M;
    ElemPassArgs a;
};
StepElemPass step_elem_pass(const dotmi_handle *h, const double *x, int grad, bool sharded = true);
// the evaluation entries: the element pass at x on ALL elements, whatever the handle shards (energy partials in h->partE, their block
// count returned) and, with grad, its plain gather into h->g_trial
int eval_all_elements(dotmi_handle *h, const double *x, int grad);
// E = dtSq * sum(elastic) + sum(inertia) from nb blocks of energy partials in h->h_partE, in the canonical order (chunked_sum)
double energy_of_partials(const dotmi_handle *h, int nb);
// sharded element pass (no owner exchange): this rank's partial gradient and energy to the staging buffer, one all-reduce, the pair and
// its statistics from the sum (`pair`: what pair_stats reads); the controller then reads the energy at h->gstage + n as one block
int gradient_over_ranks(dotmi_handle *h, int nb, const GatherArgs &pair);
// dotmi_devloop.hip
int run_device_loop(dotmi_handle *h, LoopOut &r);

}  // namespace dotmi

