/*
 * dotmi.h -- C ABI of the MI355X-native DOT time-step (libdotmi.so).
 *
 * Drop-in boundary for the reference's DOT stepper: a host adapter with the reference's
 * `DOT::Optimizer<3>` surface (src/TimeStepper/Optimizer.hpp:83-112; picked by the factory in
 * src/main.cpp:905-938) forwards to these entry points.  Plain pointers and sizes only; caller
 * owns every host array; the handle owns all device memory and (N>1) the RCCL communicator.
 * One host thread per handle.  No exceptions cross this boundary.
 *
 * Return convention (mirrors Optimizer::solve, Optimizer.cpp:327-368):
 *   0  ok / stepped
 *   2  stepped but hit the iteration cap or the line search underflowed (solve() == 2)
 *  <0  error (DOTMI_E_*); dotmi_last_error() has the text
 *
 * All floating point is FP64; indices are int32; positions / velocities / gradients are
 * nV x 3 row-major (xyz interleaved), exactly the layout of the reference's `velocity` vector
 * (Optimizer.cpp:357) and of `result.V` rows.
 */
#ifndef DOTMI_H
#define DOTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DOTMI_ENERGY_FCR 0 /* FixedCoRotEnergy   (src/Energy/Physics_Elasticity/FixedCoRotEnergy.cpp) */
#define DOTMI_ENERGY_SNH 1 /* StableNHEnergy     (src/Energy/Physics_Elasticity/StableNHEnergy.cpp)  */
/* the log-regularised form that StableNHEnergy.cpp holds beside the plain one and a reference build with SNH_WITHLOG
 * (src/Utils/Types.hpp:36) runs for the script line `energy SNH`: Psi :84-89, dPsi/dsigma :102-114, d2Psi/dsigma2 :134-171,
 * B-left :204-216, dPsi/dF :237-243.  3-D only. */
#define DOTMI_ENERGY_SNH_LOG 2

#define DOTMI_E_INVALID -1  /* bad argument */
#define DOTMI_E_DEVICE -2   /* HIP / RCCL runtime error */
#define DOTMI_E_NOTSPD -3   /* a subdomain Hessian was not positive definite (non-positive pivot);
                               the reference dumps the matrix and exit(-1)s, Optimizer.cpp:301-313 */
#define DOTMI_E_NOGPU -4    /* no usable HIP device: the product path has no CPU fallback */

typedef struct dotmi_handle dotmi_handle;

/* Mesh<3> fields the path consumes (src/Mesh.hpp:38-60): rest positions V_rest, tets F,
 * per-element Lame parameters u / lambda (Mesh.cpp:741-744), density (lumped mass is derived as in
 * Mesh.cpp:552-585), the fixed set isFixedVert (after AnimScripter::initAnimScript,
 * AnimScripter.cpp:29) and the element partition that METIS::partMesh returns
 * (src/Utils/METIS.hpp:109-140, consumed in ADMMDDTimeStepper.cpp:88-262). */
typedef struct {
    int32_t nV, nT;
    const double *X_rest;  /* nV*3 */
    const int32_t *T;      /* nT*4, positive orientation */
    const double *mu;      /* nT */
    const double *lambda;  /* nT */
    double density;
    const uint8_t *fixed;  /* nV, 1 = Dirichlet */
    const int32_t *epart;  /* nT, values in [0,nParts); NULL = partition with dotmi_partition() */
    int32_t nParts;
    const int32_t *vpart;  /* optional, nV values in [0,nParts): a VERTEX partition (METIS::partMesh_nodes,
                              METIS.hpp:161-193).  When given, subdomain s is the vertex set {v : vpart[v] == s} --
                              disjoint blocks of the global Hessian, no interface, no averaging: the block-Jacobi
                              initialiser of LBFGS-JH (LBFGSTimeStepper.cpp:70-90, :240-262, :381-393); epart is then
                              ignored.  Single GPU. */
} dotmi_mesh;

/* Config / Optimizer constants (src/Config.hpp, Optimizer.cpp:98-111, DOTTimeStepper.cpp:45) */
typedef struct {
    int32_t energy;    /* DOTMI_ENERGY_* */
    double dt;         /* Optimizer::setTime */
    double gravity[3]; /* (0,-9.80665,0) unless turnOffGravity */
    double relTol;     /* setRelGL2Tol argument, 1e-5 */
    int32_t history;   /* L-BFGS pairs, 5 */
    int32_t iterCap;   /* 10000 */
    double alphaMin;   /* lower clamp of the initial step length, 0.1 (Optimizer.cpp:1085) */
    int32_t device;    /* HIP device ordinal */
    int32_t rank;      /* this process' rank among `world` cooperating handles */
    int32_t world;     /* 1 = single GPU */
    const void *comm_id; /* world>1: the 128-byte id from dotmi_comm_unique_id (same on all ranks) */
    int32_t flags;     /* DOTMI_FLAG_* */
    /* world>1, optional: a host sum-all-reduce the library calls INSTEAD of RCCL (comm_id may then be NULL): buf holds
     * n doubles in host memory, to be replaced on every rank by the sum over the ranks; every rank calls it with the
     * same n in the same order.  The library stages the payload through pinned host memory.  This is how a
     * deployment without RCCL (or a test: two processes on one GPU over gloo) runs the sharded path. */
    void (*allreduce)(void *ctx, double *buf, int64_t n);
    void *allreduce_ctx;
} dotmi_params;

#define DOTMI_FLAG_FORCE_DIST 4     /* take the sharded code path (element lists, partial sums, RCCL
                                       all-reduces) even with world == 1: lets a 1-GPU box test it */
#define DOTMI_FLAG_TIME_BACKSOLVE 2 /* bracket every 8th launch of the streaming back-solve kernel inside dotmi_step
                                       with HIP events on the handle's stream (an event record costs ~6 us of
                                       stream time); totals land in dotmi_step_stats */
#define DOTMI_FLAG_HOST_LOOP 8      /* drive the L-BFGS loop from the host (one stream synchronisation per
                                     * line-search trial) instead of the device-resident loop control; the
                                     * two produce identical iterates -- kept for A/B tests.  (The sharded
                                     * multi-GPU path runs the device-resident loop too, with deterministic
                                     * slot batches; this flag selects the host loop there as well.) */

#define DOTMI_FLAG_TIME_PHASES 16    /* drive the loop from the host and bracket every phase of an iteration with HIP
                                     * events on the handle's stream; the device times land in
                                     * dotmi_step_stats.ms_phase under the reference's timer_step slots.  Costs
                                     * ~8 event records per iteration: for info.txt, not for benchmarks */

/* indices of dotmi_step_stats.ms_phase = the reference's timer_step activities (src/main.cpp:867-880) */
enum {
    DOTMI_T_MATRIX_COMPUTATION = 0,  /* element Hessians + global assembly (slot started at DOTTimeStepper.cpp:576) */
    DOTMI_T_MATRIX_ASSEMBLY = 1,     /* subdomain matrices (fillInDecomposedHessians, :623) */
    DOTMI_T_SYMBOLIC_FACTORIZATION = 2,
    DOTMI_T_NUMERICAL_FACTORIZATION = 3,
    DOTMI_T_BACKSOLVE = 4,           /* subdomain solves + merge (:404-452) */
    DOTMI_T_LINESEARCH_OTHER = 5,    /* alpha_0 SpMV, stepForward (Optimizer.cpp:756-881) */
    DOTMI_T_MODIFY_GRAD = 6,         /* two-loop, first half (:386-400) */
    DOTMI_T_MODIFY_SEARCHDIR = 7,    /* two-loop, second half (:455-467) */
    DOTMI_T_UPDATE_HISTORY = 8,      /* gradient + (s, y) update (:475-494) */
    DOTMI_T_LINESEARCH_EVAL = 9,     /* energy evaluations of the line search (Optimizer.cpp:791,830) */
    DOTMI_T_FULLYIMPLICIT_ECOMP = 10, /* initX + first energy / gradient (DOTTimeStepper.cpp:288-293) */
    DOTMI_T_SOLVE_EXTRACOMP = 11,    /* BE update, x~ (Optimizer.cpp:353-365) */
    DOTMI_T_COMPGRAD = 12,
    DOTMI_T_CCD = 13,
    DOTMI_T_COUNT = 14
};

#define DOTMI_FLAG_GSDD 32           /* dotmi_step runs the reference's Gauss-Seidel domain-decomposition iteration
                                     * (`timeStepper GSDD <n>`, DOTTimeStepper::solve_oneStep_GSDD,
                                     * DOTTimeStepper.cpp:507-565) on the same factors and kernels instead of
                                     * L-BFGS-H: per iteration one sweep over the subdomains -- solve H_s p_s = -g_s,
                                     * line search from step 1 along p_s, refresh the gradient.  stats.iters = sweeps.
                                     * Single GPU. */

#define DOTMI_FLAG_ASYNC_REFRESH 128 /* dotmi_step returns as soon as the refresh at the end of the step (element Hessians,
                                     * assembly, factorisation: DOTTimeStepper.cpp:349-380) is ENQUEUED instead of waiting
                                     * for it: the caller's work between two steps (moving the handles, writing output)
                                     * overlaps it.  Its device times (ms_hessian, ms_factor) and its verdict
                                     * (DOTMI_E_NOTSPD) are then reported by the NEXT dotmi_step -- whose loop has by then
                                     * run on that factorisation -- or by the next call that needs the factors.  Single
                                     * rank, device loop; ignored otherwise. */
#define DOTMI_FLAG_NEWTON 64         /* dotmi_step runs the reference's projected Newton (`timeStepper Newton`, the base
                                     * Optimizer::fullyImplicit / solve_oneStep, Optimizer.cpp:654-749): every iteration
                                     * re-evaluates the projected Hessian at the current iterate, factorises, solves
                                     * H p = -g and line-searches from step 1; no refresh at the end of the step.  It is
                                     * the reference's method when the mesh is ONE subdomain (nParts = 1); with more
                                     * subdomains the solve is the domain-decomposed block solve instead of H^-1.
                                     * stats.iters = Newton iterations.  Single GPU. */
#define DOTMI_FLAG_OWNER_EXCHANGE 256 /* N > 1 (or DOTMI_FLAG_FORCE_DIST), device loop: owner-computes exchange.  Every rank keeps the
                                      * loop's vectors valid on the vertices of ITS subdomains only (zero elsewhere); the two
                                      * vector all-reduces of an iteration carry just the entries of vertices held by more than one
                                      * rank (packed; interior entries never travel), the dot products ride in the tails of those
                                      * packets (each vertex counted once over the ranks), alpha_0's p.Hp uses each rank's own
                                      * elements' part of H, and the positions are made whole again once per step.  Implies the
                                      * sharded element pass and refresh.  Same iterations as one GPU; tests/test_gpu_two_ranks.py */
#define DOTMI_FLAG_LBFGS_PD 512     /* dotmi_step runs the reference's LBFGS-PD (`timeStepper LBFGS`, LBFGSTimeStepper with D0T_PD,
                                     * LBFGSTimeStepper.cpp:113-194, :338-449): L-BFGS whose initial inverse Hessian is the constant
                                     * projective-dynamics Laplacian L = M + sum_e dt^2 vol_e (2 mu_e + lambda_e) D_e^T D_e (fixed rows and
                                     * columns replaced by the identity), applied to the x, y, z columns separately; the first trial of
                                     * every line search is the unit step.  The handle builds NO subdomain block solve (epart, vpart and
                                     * nParts are ignored: pass NULL / 1) but the scalar nV x nV factor of L, once per create and per
                                     * dotmi_refix; a step refreshes nothing (ms_hessian = ms_factor = 0).  dotmi_apply_precond returns
                                     * L^-1 r per coordinate.  Host-driven loop, single GPU: not with world > 1, FORCE_DIST,
                                     * OWNER_EXCHANGE, GSDD, NEWTON, ASYNC_REFRESH or a vpart.  Entries of the Hessian block solve
                                     * (dotmi_refactor, dotmi_part_matrix, dotmi_spmv, dotmi_probe_direction, the bench entries) return
                                     * DOTMI_E_INVALID on such a handle. */
#define DOTMI_FLAG_LBFGS_HI 1024    /* dotmi_step runs the reference's LBFGS-HI (`timeStepper LBFGSHI`, LBFGSTimeStepper with D0T_HI,
                                     * LBFGSTimeStepper.cpp:214-233, :308-316, :376-378): L-BFGS whose initial inverse Hessian is an
                                     * INCOMPLETE Cholesky factor of the projected Hessian, rebuilt at the end of every step; the first
                                     * trial of every line search is the unit step.  A GPU form of the method, not of
                                     * Eigen::IncompleteCholesky: a block (3 x 3) IC(0) on H's own block pattern in a multicolour
                                     * ordering of the vertex graph (dotmi_plan_ic), one launch per colour, with a diagonal shift
                                     * A_ii += sigma diag(A_ii) on breakdown: the first attempt takes half the last successful shift
                                     * (0 stays 0), a breakdown doubles it from 1e-3, at most 40 attempts, then DOTMI_E_NOTSPD.  The
                                     * reference's iteration counts are therefore not reproduced; the oracle running the same
                                     * preconditioner is (tests/ic_reference.py).  The handle builds NO subdomain block solve (epart,
                                     * vpart and nParts are ignored: pass NULL / 1).  The refresh -- after create, at the end of every
                                     * step, after dotmi_refix, dotmi_refactor, dotmi_set_time_step and dotmi_set_lame -- assembles H
                                     * and factors it: ms_hessian as usual, ms_factor = all attempts, precond_bytes = 72 x (lower
                                     * blocks + diagonals) x 2.  dotmi_apply_precond returns (L L^T)^-1 r; dotmi_spmv works.
                                     * Host-driven loop, single GPU: not with world > 1, FORCE_DIST, OWNER_EXCHANGE, GSDD, NEWTON,
                                     * NEWTON_PCG, LBFGS_PD, ASYNC_REFRESH or a vpart.  dotmi_part_matrix, dotmi_part_size, dotmi_probe_direction,
                                     * dotmi_bench_precond and the bench kinds of the block solve and of the device loop return
                                     * DOTMI_E_INVALID on such a handle. */
#define DOTMI_FLAG_NEWTON_PCG 2048   /* dotmi_step runs projected Newton like DOTMI_FLAG_NEWTON, with H p = -g solved by preconditioned
                                     * conjugate gradients on the subdomain factors instead of by one factor of the whole mesh: any
                                     * nParts >= 1, one subdomain factorisation plus a few dozen streaming block-solve applications per
                                     * Newton iteration.  A GPU form of the method (the reference's Newton is CHOLMOD on one subdomain):
                                     * the preconditioner is the SYMMETRIC scaling D^-1/2 S D^-1/2 of DOT's block solve D^-1 S (which
                                     * is not symmetric and makes plain PCG diverge; they agree where dup = 1), the recurrences are the
                                     * single-reduction form of Chronopoulos and Gear, convergence |r| <= eta |g| is decided on the
                                     * device.  Per iteration: refresh and factorise at x, p = PCG(-g; eta, cap), line search from
                                     * step 1; no refresh at the end of the step.  A solve that stops at its cap or breaks down hands
                                     * over its iterate (a descent direction) and the step goes on.  eta = 1e-3, cap 500, a read-back
                                     * every 8 iterations unless dotmi_set_pcg says otherwise.  stats.iters = Newton iterations,
                                     * stats.backsolve_launches = block-solve applications (the CG iterations of the step's solves).
                                     * Host-driven loop, single GPU: not with world > 1, FORCE_DIST, OWNER_EXCHANGE, GSDD, NEWTON,
                                     * LBFGS_PD, LBFGS_HI, ASYNC_REFRESH or a vpart. */
#define DOTMI_FLAG_DOT_COARSE 4096   /* the rigid-mode coarse term of dotmi_set_dot_coarse, M' = M + Z A0^-1 Z^T, from create on.  One rank
                                     * without FORCE_DIST: dotmi_create followed by dotmi_set_dot_coarse(h, 1); the handle can be toggled
                                     * afterwards.  world > 1 or FORCE_DIST: the only way in, and fixed for the life of the handle -- the
                                     * term changes the payload of a collective, so every rank must pass the flag or none (the setter
                                     * keeps refusing such handles).  There c = Z^T r of a rank's own subdomains rides in the nc = 6 nParts
                                     * doubles behind the n of the one vector the iteration all-reduces anyway (no collective is added),
                                     * every rank solves A0 y = c redundantly behind the collective, and A0 is built on every rank behind
                                     * every refresh -- with a sharded Hessian refresh through one more all-reduce of 36 doubles per
                                     * coupled pair of subdomains (DESIGN.md sections 6 and 9).  dotmi_dot_coarse_info and
                                     * dotmi_pcg_coarse_matrix (the whole A0 on every rank) work on such a handle.  dotmi_create fails
                                     * with DOTMI_E_INVALID and a message for the flag with OWNER_EXCHANGE, GSDD, NEWTON, NEWTON_PCG,
                                     * LBFGS_PD, LBFGS_HI, ASYNC_REFRESH, a vpart, or more than 256 subdomains. */
#define DOTMI_FLAG_NEWTON_PCG_DIST 8192 /* DOTMI_FLAG_NEWTON_PCG's step on handles whose subdomains are sharded: accepted on one rank, with
                                     * FORCE_DIST and with world > 1 (RCCL or the dotmi_params.allreduce hook), in both sharding modes of
                                     * the element pass and the refresh.  One rank without FORCE_DIST: exactly DOTMI_FLAG_NEWTON_PCG
                                     * (bit-identical).  A flag of its own because it changes which collectives the communicator carries:
                                     * every rank must pass it or none.  Per CG iteration, with a replicated Hessian, one all-reduce of
                                     * n doubles (the ranks' shares of zsum = S q); with sharded Hessian rows a second one of n + 2
                                     * doubles, the packet [s = H w on the rank's rows, zeros elsewhere | gamma | delta].  Every
                                     * collective is issued in every enqueued iteration, whatever the device's verdict; after each batch
                                     * of check_every iterations the ranks adopt rank 0's (state, iterations, |r|^2, |b|^2) in one
                                     * collective of 9 doubles and fail together with DOTMI_E_DEVICE when they disagree.  The vectors of
                                     * the recurrences are replicated, so the scalars, the verdict and p are bit-identical on every rank.
                                     * dotmi_set_pcg and dotmi_pcg_info as on one rank; dotmi_set_pcg_coarse stays refused on sharded
                                     * handles.  Over real links its behaviour is unmeasured.  dotmi_create fails
                                     * with DOTMI_E_INVALID and a message for the flag with OWNER_EXCHANGE, GSDD, NEWTON, LBFGS_PD,
                                     * LBFGS_HI, ASYNC_REFRESH, DOT_COARSE or a vpart; together with DOTMI_FLAG_NEWTON_PCG that flag's own
                                     * checks run first. */

typedef struct {
    int32_t iters;       /* L-BFGS iterations (innerIterAmt delta, DOTTimeStepper.cpp:338) */
    int32_t ls_halvings;  /* numOfLineSearch delta (Optimizer.cpp:816) */
    int32_t energy_evals;
    int32_t status;       /* 0 / 2 */
    double E0, g2_0;      /* after initX (iterStats.txt header line, DOTTimeStepper.cpp:299) */
    double E, g2;         /* at exit */
    double ms_total;      /* host wall time of the step */
    double ms_loop;       /* L-BFGS loop */
    double ms_hessian;    /* element Hessians + global assembly + dense gather (device time) */
    double ms_factor;     /* inverse-Cholesky factors of all owned subdomains (device time) */
    double ms_precond;    /* DOTMI_FLAG_TIME_BACKSOLVE: summed device time of the timed backsolve_kernel launches */
    int64_t precond_launches; /* how many launches were timed */
    int64_t precond_bytes; /* algorithmic bytes per back-solve launch: 8 x the structural non-zeros of the
                              block-sparse inverse factors X_s of this rank (each is streamed once) */
    double factor_flops;  /* FP64 flop of one factorisation of this rank's subdomains as executed (GEMMs incl. the
                             identity padding + diagonal blocks): ms_factor's MFMA roofline */
    double ms_phase[DOTMI_T_COUNT]; /* device milliseconds of this step under the reference's timer_step slots.  Always
                             filled: MATRIX_COMPUTATION, MATRIX_ASSEMBLY, NUMERICAL_FACTORIZATION (HIP events of the
                             refresh at the end of the step).  The loop slots (BACKSOLVE ... FULLYIMPLICIT_ECOMP,
                             SOLVE_EXTRACOMP) only with DOTMI_FLAG_TIME_PHASES. */
    /* sharded (N > 1) path: the all-reduces this rank issued during the step, end-of-step refresh included */
    int64_t collective_calls;       /* number of all-reduces */
    int64_t collective_bytes;       /* their summed payload (8 x doubles) */
    double ms_collective;           /* DOTMI_FLAG_TIME_BACKSOLVE + RCCL: summed device time between HIP events put
                                       around every 8th ncclAllReduce on the handle's stream (queueing behind the
                                       slower rank included) */
    int64_t collective_timed;       /* how many were bracketed */
    int64_t collective_timed_bytes; /* and their payload */
    int64_t backsolve_launches;     /* back-solves of the step's loop that ran to their end (= iters) */
    int64_t backsolve_stopped;      /* speculative back-solves the controller stopped: ls_halvings + 1 in a step whose device
                                       loop issued them on the trial gradient (DESIGN.md section 5,
                                       DOTMI_EARLY_BACKSOLVE), else 0 */
    int64_t backsolve_held;         /* slots whose back-solve waited for the controller's verdict instead of streaming beside it
                                       (the trial was expected to be rejected: a two-level forecast from the outcomes of the earlier trials of its kind) */
    int64_t backsolve_held_rejected; /* ... and were rejected: these left without reading a factor (they are part of
                                       backsolve_stopped) */
    int64_t paired_slots;           /* DOTMI_PAIR_TRIALS: slots that evaluated the half step in full and the energy of the full step
                                       (the line search of Optimizer.cpp:806-833 with its first two trials in one launch) */
    int64_t paired_redone;          /* ... whose full step was acceptable after all: evaluated again, in full, by the next slot */
    int64_t spec_slots;             /* DOTMI_SPEC_STEP: new-direction slots that evaluated the unit step beside the direction kernel ... */
    int64_t spec_redone;            /* ... whose step estimate alpha_0 turned out below 1: evaluated again, at alpha_0, by the next slot */
} dotmi_step_stats;

/* ---- lifetime -------------------------------------------------------------------------------- */
/* Builds all device state, computes restTriInv / volumes / lumped mass / tolerance, and performs
 * DOTTimeStepper::precompute (DOTTimeStepper.cpp:150-178): Hessian + subdomain factors at x_init.
 * x_init: nV*3 initial positions (result.V after initAnimScript; usually == X_rest). */
int dotmi_create(const dotmi_mesh *mesh, const dotmi_params *params, const double *x_init,
                 dotmi_handle **out);
void dotmi_destroy(dotmi_handle *h);
const char *dotmi_last_error(const dotmi_handle *h); /* h may be NULL: last create() error */

/* Host-only planning helper (touches no device): splits parts 0..nParts-1 into `world` contiguous
 * groups balanced by sum n_s^2 -- the bytes the back-solve streams per L-BFGS iteration.
 * first_part has world+1 entries; rank r owns parts [first_part[r], first_part[r+1]).  This is the
 * split dotmi_create applies; elements follow their part (ADMMDDTimeStepper.cpp:161). */
int dotmi_plan_shards(int32_t nParts, const int32_t *part_scalar_size, int32_t world, int32_t *first_part);

/* Host-only planning helper (touches no device): everything rank `rank` of `world` owns under dotmi_create's plan --
 * parts [*p0, *p1) (dotmi_plan_shards on the parts' scalar sizes), the elements of those parts (elems: up to nT
 * ids ascending, *n_elems of them; elemList_subdomain of the owned parts, ADMMDDTimeStepper.cpp:161), the vertex slice
 * [*v0, *v1) whose inertia terms / SpMV rows it adds, and part_size[nParts] = 3 x vertices of every part.  Any output
 * pointer may be NULL. */
int dotmi_plan_rank(int32_t nV, int32_t nT, const int32_t *T, const int32_t *epart, int32_t nParts, int32_t rank,
                    int32_t world, int32_t *p0, int32_t *p1, int32_t *elems, int32_t *n_elems, int32_t *v0, int32_t *v1,
                    int32_t *part_size);

/* Host-only planning helper (touches no device): the nested-dissection layout dotmi_create gives the
 * dense blocks of parts [p0,p1).  The reference leaves the ordering of each subdomain matrix to CHOLMOD's
 * analyze step (CHOLMODSolver.cpp:103-141); here every owned subdomain is ordered [A | C | S] recursively
 * (S a vertex separator, no mesh edge between A and C) on one tree shared by the owned parts, region sizes
 * padded to the maximum over the parts.  nodes: n_nodes rows of 6 int32 {off, size, childA, childC, offS,
 * sizeS} (children -1 for a dense leaf, root = row 0); nmax: padded scalar size (multiple of 64);
 * pos: for every part in [p0,p1), for every local vertex in ascending global id, the padded scalar
 * position of its first dof.  levels < 0 / min_split < 128 select the defaults.  nodes, pos may be NULL. */
/* (host only) the element patches of the element pass for all elements of a mesh (dot_amd/csrc/patches.hpp); call with
 * elem == NULL for the sizes first.  tests/test_patches.py */
int dotmi_plan_patches(int32_t nV, int32_t nT, const int32_t *T, const double *X, int32_t PE, int32_t *n_patches, int32_t *pv,
                       int32_t *n_slots, int32_t *elem, uint16_t *tl, uint16_t *epos, int32_t *pv_gid, int32_t *pv_slot,
                       int32_t *pv_cnt, uint16_t *c_ptr, int32_t *pp_rng);
/* (host only, round 6) the VERTEX patches of the one-launch element pass + gather (dot_amd/csrc/vpatches.hpp, k_elemvert.hip): a
 * patch owns up to max_own vertices and carries every element incident to them.  hdr[5] = {patches, PE, most touched vertices, most
 * owned vertices, longest sum of runs}; with owner != NULL also: owner[nV] (the patch that owns a vertex), elem[patches * PE] (global
 * element of every slot, -1 padding), eown[patches * PE] (1: this patch counts the element's energy), runlen[nV] (entries of the
 * vertex' gradient run in its patch).  tests/test_gpu_round6.py / test_host_logic.py */
int dotmi_plan_vpatches(int32_t nV, int32_t nT, const int32_t *T, const double *X, int32_t PE, int32_t max_own, int32_t *hdr,
                        int32_t *owner, int32_t *elem, int32_t *eown, int32_t *runlen);
/* (round 9) which loads the handle's one-launch element pass + gather (elem_vertex_kernel) uses: 1 = the operand records
 * (DOTMI_OPERAND_RECORDS, default, where their LDS fits), 0 = the flat arrays, -1 = the handle has no vertex patches */
int dotmi_operand_records(const dotmi_handle *h);
/* Which forms of its kernels the handle's loop launches, as a bit mask.  Bits 1 / 2 / 4: the vertex gather, the early merge and the
 * direction kernel in their wide form (512 / 512 / 1024 threads per workgroup) instead of the 256-thread one -- chosen by the number of
 * dofs / rows the launch visits (beyond 524 288 dofs, 131 072 dofs and 24 576 rows; under DOTMI_FLAG_OWNER_EXCHANGE those of the held
 * vertices), or forced: the environment variable DOTMI_WIDE_FORMS, read by dotmi_create, is unset or -1 for the rule by size and
 * otherwise this same mask of bits 1 | 2 | 4, a set bit forcing the wide form and a clear bit the narrow one (0: all narrow, 7: all
 * wide; the results agree to rounding).  A bit is only set for a launch the handle's loop contains (the gather's on a device-resident
 * loop, which launches it in the steps that do not run on vertex patches; the other two in the early order).  Bit 8: the merge is
 * split (per-subdomain sums, then a gather: DOTMI_SPLIT_MERGE).  Bits 16-17: the column width of the two-level back-solve's backward
 * kernel, 0 none (one-pass form, or no panels), 1 / 2 / 3 = 32 / 64 / 128 column pairs.  < 0: h is NULL */
int dotmi_loop_forms(const dotmi_handle *h);
/* (host only) the low three bits of dotmi_loop_forms for a launch of ndof_gather and ndof_merge scalar dofs and nrows_spmv block rows
 * under the force value `force` (DOTMI_WIDE_FORMS: -1 by size, else the mask) -- the launchers' own rule, no device touched */
int dotmi_plan_loop_forms(int64_t ndof_gather, int64_t ndof_merge, int64_t nrows_spmv, int32_t force, int32_t *out);
/* (host only, round 9) the static operands of the owned vertices in PATCH order (vpatches.hpp: VpOwnRec, DOTMI_OPERAND_RECORDS), built
 * from the caller's flat arrays as dotmi_create builds them from its own: mass[nV], fixed[nV] and the CSR vp_ptr[nV + 1] / vp_off of a
 * vertex' copies in the padded right-hand sides.  hdr as dotmi_plan_vpatches; with pv_gid != NULL also pv_gid[patches * PV] (touched
 * vertices, the owned ones first, -1 padding), po_cnt[patches] and per record (patches * PO, zeros behind po_cnt): rec_mass, rec_fixed,
 * rec_cnt (copies of the vertex), rec_off[4] (its first four positions, 0 beyond the count).  fixed2 != NULL: the records after
 * dotmi_refix's rewrite of the flags with that mask.  tests/test_operand_records.py */
int dotmi_plan_vpatch_records(int32_t nV, int32_t nT, const int32_t *T, const double *X, int32_t PE, int32_t max_own, const double *mass,
                              const uint8_t *fixed, const int32_t *vp_ptr, const int32_t *vp_off, const uint8_t *fixed2, int32_t *hdr,
                              int32_t *pv_gid, int32_t *po_cnt, double *rec_mass, int32_t *rec_fixed, int32_t *rec_cnt, int32_t *rec_off);
/* (host only) the level schedule of the tile factorisation for one nt x nt tile block with the given upper tile pattern in
 * the compact row-block layout; see dot_amd/csrc/tile_factor.hpp and tests/test_tile_schedule.py */
int dotmi_plan_tile_schedule(int32_t nt, const uint8_t *live, const uint8_t *pattern, const int32_t *c0, int32_t eager_min,
                             int32_t eager_chunk, int64_t *tasks, int64_t *prods, int64_t *n_tasks, int64_t *n_prods,
                             int64_t *n_levels, int64_t *storage, int64_t *scratch_base, int64_t *row_off, int32_t *row_ld);
/* (host only, round 6) that schedule in the TWO-LEVEL form of the block solve (dotmi_backsolve_form = 1) for a leaves-first block:
 * leaf_tile[t] = tile row t belongs to a leaf of the dissection; a separator's row block j keeps the leaf tile columns
 * [c0m[j], c0m[j] + ntm[j]) of its sub-tree in a second storage range (row_off_m / row_ld_m), its main range starts at its
 * sub-tree's first separator column c0[j].  Tiles (leaf i, separator j) receive T_ij = sum over the tiles m >= i of i's leaf of
 * Q_im R_mj (post = store); the inverse's other cross terms do not exist.  tests/test_tile_schedule.py runs it in numpy */
int dotmi_plan_tile_schedule_two_level(int32_t nt, const uint8_t *live, const uint8_t *pattern, const int32_t *c0,
                                       const uint8_t *leaf_tile, const int32_t *c0m, const int32_t *ntm, int32_t eager_min,
                                       int32_t eager_chunk, int64_t *tasks, int64_t *prods, int64_t *n_tasks, int64_t *n_prods,
                                       int64_t *n_levels, int64_t *storage, int64_t *row_off, int32_t *row_ld, int64_t *row_off_m,
                                       int32_t *row_ld_m);
/* (host only) the dependencies of that task list for the dataflow form of the factorisation (DOTMI_TILE_FLOW, one launch of
 * persistent workgroups; tile_flow_kernel): task v waits for dep_idx[dep_ptr[v] .. dep_ptr[v+1]).  Same arguments and task
 * order as dotmi_plan_tile_schedule; dep_idx == NULL returns the count only. */
int dotmi_plan_tile_deps(int32_t nt, const uint8_t *live, const uint8_t *pattern, const int32_t *c0, int32_t eager_min,
                         int32_t eager_chunk, int64_t *dep_ptr, int64_t *dep_idx, int64_t *n_deps);
/* (host only) the subdomain groups of the factorisation's level launches (DOTMI_TILE_GROUPS; dot_amd/csrc/tile_factor.hpp): the
 * subdomains by falling weight, each into the lightest group so far.  group_of[n_parts]; returns the number of groups used (groups
 * clamped to [1, n_parts]) or an error.  tests/test_tile_groups.py */
int dotmi_plan_tile_groups(int32_t n_parts, const int64_t *weight, int32_t groups, int32_t *group_of);
/* (host only) the grouped level table for n_blocks blocks of nt x nt tiles (live[n_blocks * nt], pattern[n_blocks * nt * nt]; every
 * row block stored from tile column 0, the blocks' storage one behind the other): tasks, 6 int64 each in the order of the task array
 * {group, level inside the group, block, offset of the tile written, post, products}; clear, 2 int64 per cleared tile {group,
 * offset}; group_of[n_blocks]; group_level[groups + 1]; and a list of n_fill entries (entry e of block fill_sub[e]) group by group:
 * fill_perm[n_fill], fill_start[groups + 1].  tasks == NULL: the counts only.  Returns the number of groups used or an error. */
int dotmi_plan_grouped_tile_schedule(int32_t n_blocks, int32_t nt, const uint8_t *live, const uint8_t *pattern, int32_t eager_min,
                                     int32_t eager_chunk, int32_t groups, int64_t *tasks, int64_t *n_tasks, int32_t *group_of,
                                     int32_t *group_level, int64_t *clear, int64_t *n_clear, int32_t n_fill, const int32_t *fill_sub,
                                     int32_t *fill_perm, int32_t *fill_start);
/* (host only, round 8) the H tiles' entry lists (DOTMI_TILE_HFILL): with them the first task of an H tile (init = 2) builds the tile
 * in LDS and the refresh neither clears nor fills the work buffer.  For n_blocks blocks in the layout of
 * dotmi_plan_grouped_tile_schedule and the caller's fill lists (fill_dst[9 n_fill]: offsets in the work buffer or -1,
 * fill_src[n_fill]: blocks of Hval, pad_dst[n_pad]: the identity padding).  counts[8] = {tasks, clear tiles, entries, n_fill, n_pad,
 * groups, doubles of one buffer, two-level}; tasks, 10 int64 each {group, level, block, offset of the c tile and of the tile written
 * (each in its own buffer), init, post, first entry, entries, form}; clear, 5 int64 each {group, offset, leading dimension,
 * first entry, entries}; entry_pos / entry_src per entry: k * 65 + j for element (row k, column j) of the column-major tile, and the
 * scalar's index in Hval (-1: 1.0).  tasks == NULL: counts only.  Returns the groups used or an error.  tests/test_tile_fill.py */
int dotmi_plan_tile_fill(int32_t n_blocks, int32_t nt, const uint8_t *live, const uint8_t *pattern, int32_t eager_min,
                         int32_t eager_chunk, int32_t groups, int64_t n_fill, const int64_t *fill_dst, const int32_t *fill_src,
                         int64_t n_pad, const int64_t *pad_dst, int64_t *counts, int64_t *tasks, int64_t *clear, int32_t *entry_pos,
                         int32_t *entry_src);
/* (host only) the same for all parts of a mesh through dotmi_create's own planning stages (two_level: the leaves-first form; the
 * eager rules from DOTMI_TILE_EAGER_MIN / DOTMI_TILE_EAGER_MIN_RMUL, as dotmi_create reads them); also
 * returns the fill lists the entry lists come from: fill_dst[9 counts[3]], fill_src[counts[3]], pad_dst[counts[4]] */
int dotmi_plan_tile_fill_mesh(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, const int32_t *epart, int32_t nParts,
                              int32_t groups, int32_t two_level, int64_t *counts, int64_t *tasks, int64_t *clear, int32_t *entry_pos,
                              int32_t *entry_src, int64_t *fill_dst, int32_t *fill_src, int64_t *pad_dst);
/* (host only) the job table of the back-solve launches dotmi_create builds for parts [p0, p1) of this mesh: how the rows of every
 * tree region are cut into tiles, which launch / kernel form takes them and which workgroup runs them (dot_amd/csrc/bs_tiles.hpp;
 * the reference has no counterpart: CHOLMODSolver::solve, CHOLMODSolver.cpp:149-163, walks CHOLMOD's supernodes).  tiles: up to cap
 * rows of 6 int32 {local part, first row, rows, first column, tile index in the part, job}; job = workgroup of its launch (wide
 * launch: 0 .. n_wide-1; narrow launch: one-tile jobs 0 .. n_narrow-1, then n_narrow + k for the four tiles of pack k; -1: the
 * two-phase kernel of rows beyond 5120 columns).  counts[8] = {tiles, n_wide, n_narrow, n_packs, n_long, nmax, shallow, few}.
 * tiles may be NULL (counts only).  tests/test_host_logic.py */
int dotmi_plan_backsolve_tiles(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, const int32_t *epart, int32_t nParts,
                               int32_t p0, int32_t p1, int32_t cap, int32_t *tiles, int32_t *counts);
/* (host only) the kernel forms those tiles run on, from the table the kernels are instantiated from (dot_amd/csrc/bs_forms.hpp): up to
 * cap rows of 6 int32 {family, lanes, chunks, rows per pass, RLDS, longest row}, family 0 = a wavefront of a pack, 1 = the 256-thread
 * workgroup, 2 = the 512-thread one; a family's forms ascend and a tile takes the first that holds its longest row.
 * counts[4] = {forms, and of the two-phase kernel: lanes, rows per pass, columns per chunk}.  forms may be NULL (counts only).
 * tests/backsolve_cases.py */
int dotmi_plan_backsolve_forms(int32_t cap, int32_t *forms, int32_t *counts);
int dotmi_plan_layout(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, const int32_t *epart,
                      int32_t nParts, int32_t p0, int32_t p1, int32_t levels, int32_t min_split,
                      int32_t node_cap, int32_t *nodes, int32_t *n_nodes, int32_t *nmax, int32_t *pos);

/* Host-only (touches no device): the built-in element partitioner, for meshes that come without the partition METIS
 * gives the reference (METIS::partMesh, src/Utils/METIS.hpp:109-140; block-size runs `DOT -1 <nodes/block>`,
 * src/main.cpp:792-798).  Recursive bisection of the face-adjacency graph of the tets, coordinate split + Fiduccia-
 * Mattheyses refinement of the face cut; seedless and deterministic.  epart: nT values in [0,nParts). */
int dotmi_partition(int32_t nV, int32_t nT, const int32_t *T, const double *X, int32_t nParts, int32_t *epart);

/* world>1: rank 0 calls this and ships the 128 bytes to every rank (e.g. torch.distributed
 * broadcast); all ranks pass it as params.comm_id.  */
int dotmi_comm_unique_id(void *out128);
/* The number of ranks in the handle's RCCL communicator as RCCL itself reports it (ncclCommCount): what a benchmark prints
 * beside the number of processes it believes it started.  1: no communicator (single GPU); -world: the ranks cooperate
 * through the host all-reduce hook of dotmi_params instead of RCCL. */
int32_t dotmi_comm_ranks(const dotmi_handle *h);

/* ---- state ------------------------------------------------------------------------------------ */
/* (x, v[, x_n]) round-trip = what Optimizer::saveStatus / restart carry (Optimizer.cpp:1096-1177) */
int dotmi_set_state(dotmi_handle *h, const double *x, const double *v, const double *x_n /*or NULL*/);
int dotmi_get_state(dotmi_handle *h, double *x, double *v, double *x_tilde /*any may be NULL*/);
/* scripted handle motion for this step: x[idx[k]] = pos[k] (AnimScripter::stepAnimScript,
 * AnimScripter.cpp:456-466) */
int dotmi_set_dirichlet(dotmi_handle *h, int32_t n, const int32_t *idx, const double *pos);
/* fixed set changed (rubberBandPull release): re-pattern + refactor
 * (DOTTimeStepper::updatePrecondMtrAndFactorize, DOTTimeStepper.cpp:185-270) */
int dotmi_refix(dotmi_handle *h, const uint8_t *fixed);

/* ---- tolerance, time step and materials of a live handle --------------------------------------- */
/* Called between steps.  After any of them the handle is the one dotmi_create would have built from the new value, brought to
 * the same state with dotmi_set_state(x, v, x_n) and dotmi_refactor(h, NULL) -- without the planning create repeats (partition
 * tables, dissection layout, tile schedules, patches depend on none of the three).  A refresh a step left running
 * (DOTMI_FLAG_ASYNC_REFRESH) is judged first: its verdict, if it has one, is returned and nothing is changed.  A bad argument
 * (NULL, non-finite, relTol <= 0, dt <= 0, any mu[e] <= 0 or lambda[e] <= 0) returns DOTMI_E_INVALID and changes nothing.  On a
 * sharded handle every rank calls them in the same order with the same values, like dotmi_refix: the refresh ends in a collective. */
/* the next step's tolerance (main.cpp:108-118 sets it per time step from the script's `tol` list); no device work */
int dotmi_set_rel_tol(dotmi_handle *h, double relTol);                           /* Optimizer::setRelGL2Tol, Optimizer.cpp:222-228 */
/* dt, dt^2, gravity dt^2, the tolerance, x~ from the handle's x_n and v (on the device), then what was built with dt: the Hessian
 * and subdomain factors at the current x (LBFGS-PD: L and its factor).  Returns the refresh's code (DOTMI_E_NOTSPD) */
int dotmi_set_time_step(dotmi_handle *h, double dt);                             /* Optimizer::setTime, Optimizer.cpp:249-257 */
/* per-element Lame parameters: the tolerance from element 0, the field in front of every form of the element pass (one material
 * everywhere: as two kernel arguments, like create), then the refresh as above and its return code */
int dotmi_set_lame(dotmi_handle *h, const double *mu, const double *lambda);     /* nT each; dor_set_lame */

/* ---- time integration --------------------------------------------------------------------------- */
/* The reference carries Config::timeIntegrationType and switches on it at the velocity update (Optimizer.cpp:354-361), the predictor
 * (:588-610), the energy (:1188) and the gradient (:1225); its enum has the one entry TIT_BE.  DOTMI_TIT_BDF2 is the second: variable-step
 * BDF2, second order and L-stable.  With w = dt / dt_prev, gamma = (1 + w) / (1 + 2 w), c0 = (1 + w)^2 / (1 + 2 w), c1 = w^2 / (1 + 2 w)
 * (w = 1: 2/3, 4/3, 1/3) and x^ = c0 x_n - c1 x_{n-1}, v^ = c0 v_n - c1 v_{n-1}, a BDF2 step is the backward-Euler step of the
 * effective size dt_e = gamma dt from (x^, v^): x~ = x^ + dt_e v^ + dt_e^2 g on free vertices (fixed ones: their position), the same
 * incremental potential with dt_e for dt, v+ = (x+ - x^) / dt_e on all vertices -- bit for bit what a backward-Euler handle at dt_e
 * computes from dotmi_set_state(x^, v^, NULL).  Energy, gradient, Hessian, factors, tolerance, every stepper's loop, the coarse terms
 * and sharding see dt_e only; only the predictor and the update are BDF2's own (dot_amd/csrc/time_integration.hpp, k_timeint.hip).
 * The first step of a run and the first step after dotmi_set_state have no level n-1: they are backward-Euler steps at dt. */
enum dotmi_time_integration_kind { DOTMI_TIT_BE = 0, DOTMI_TIT_BDF2 = 1 };
/* The integrator of the next steps, on a live handle between two steps (the default is DOTMI_TIT_BE; setting the kind the handle has
 * does nothing at all).  A switch to BDF2 starts with a backward-Euler step at dt (a backward-Euler handle keeps no level n-1); a switch
 * back to backward Euler drops the level.  Where the switch changes the effective step, x~ and what was built with dt are redone as by
 * dotmi_set_time_step, whose return codes these entries share.  Any other id: DOTMI_E_INVALID.  Under BDF2
 *   dotmi_set_time_step   is the variable-step rule with w = dt / dt_prev, not a restart;
 *   dotmi_set_state       drops level n-1: the next step is a start step (dotmi_set_history afterwards gives the level back);
 *   dotmi_get_state       returns BDF2's v and the x~ of the next step;
 *   dotmi_target_gres     is the tolerance at the next step's effective step.
 * On a sharded handle every rank calls it alike (every rank holds whole x and v: nothing is exchanged). */
int dotmi_set_time_integration(dotmi_handle *h, int32_t kind);                  /* Config::timeIntegrationType, Optimizer.cpp:354-361 */
int32_t dotmi_time_integration(const dotmi_handle *h);                          /* the kind; DOTMI_E_INVALID for NULL */
/* the kind, whether level n-1 exists (0 / 1: 0 = the next step is a start step), the effective step the next step's launches take and
 * the size of the step that led from level n-1 to level n (0 without the level).  Any pointer may be NULL. */
int dotmi_time_integration_info(const dotmi_handle *h, int32_t *kind, int32_t *levels, double *dt_eff, double *dt_prev);
/* Level n-1 of a BDF2 handle, for a restart that continues with a BDF2 step instead of a start step (Optimizer::saveStatus carries
 * one level only, Optimizer.cpp:1096-1177): dotmi_get_history returns the number of stored levels (0: nothing written but *dt_prev = 0;
 * 1: x_prev, v_prev, nV*3 each, and the step size between the two levels; any pointer may be NULL).  dotmi_set_history on a BDF2 handle,
 * after dotmi_set_state: the level, then x^, x~ and the refresh at the effective step as above.  DOTMI_E_INVALID for NULL arrays, a
 * non-positive or non-finite dt_prev, and on a backward-Euler handle. */
int dotmi_get_history(dotmi_handle *h, double *x_prev, double *v_prev, double *dt_prev);
int dotmi_set_history(dotmi_handle *h, const double *x_prev, const double *v_prev, double dt_prev);          /* Optimizer.cpp:588-610 */
/* (host only) the rule of one step from (kind, dt, dt_prev, levels in {0, 1}): x^ = c0 x_n - c1 x_{n-1}, dt_eff = gamma dt; backward
 * Euler and levels = 0 give (1, 0, 1, dt).  Any output may be NULL.  tests/test_bdf2_reference.py */
int dotmi_plan_time_integration(int32_t kind, double dt, double dt_prev, int32_t levels, double *c0, double *c1, double *gamma,
                                double *dt_eff);                                                              /* Optimizer.cpp:1188, :1225 */

/* ---- the hot path ----------------------------------------------------------------------------- */
/* One time step = Optimizer::solve(1) minus the script move:
 * DOTTimeStepper::fullyImplicit (DOTTimeStepper.cpp:273-346) + BE update (Optimizer.cpp:354-361); under DOTMI_TIT_BDF2 the BDF2
 * predictor and update around the same loop. */
int dotmi_step(dotmi_handle *h, dotmi_step_stats *stats);
/* per-iteration (alpha, E, ||g||^2) of the last step = iterStats.txt rows (DOTTimeStepper.cpp:304,329) */
int dotmi_last_iter_log(const dotmi_handle *h, int32_t cap, double *alpha, double *E, double *g2);
double dotmi_target_gres(const dotmi_handle *h); /* Optimizer::targetGRes (Optimizer.cpp:613-651) */

/* ---- kernel-level entry points (parity tests, adapters that override single hooks) ------------- */
int dotmi_eval_energy(dotmi_handle *h, const double *x, double *E);        /* Optimizer::computeEnergyVal, :1183 */
int dotmi_eval_gradient(dotmi_handle *h, const double *x, double *g);      /* Optimizer::computeGradient, :1220 */
int dotmi_eval_elem_hessians(dotmi_handle *h, const double *x, double *H); /* Energy::computeElemHessianByPK, Energy.cpp:673; nT*144 */
int dotmi_refactor(dotmi_handle *h, const double *x /*NULL = current*/);   /* DOTTimeStepper::updateHessianAndFactor, :349 */
int dotmi_apply_precond(dotmi_handle *h, const double *r, double *p);      /* DOTTimeStepper.cpp:406-450 */
int dotmi_spmv(dotmi_handle *h, const double *p, double *Hp);              /* LinSysSolver::multiply, CHOLMODSolver.cpp:185 */
/* One iteration of DOTTimeStepper::solve_oneStep up to its first line-search trial (DOTTimeStepper.cpp:386-467,
 * Optimizer::initStepSize :1076-1093, the first computeEnergyVal of lineSearch :791) from a caller-supplied
 * iterate x and m <= history stored pairs (S, Y: m*n each, oldest first): g = gradient at x, q = after the first
 * loop, z = the domain-decomposed block solve of q, p = search direction, alpha0, E(x + alpha0 p).  Any output may
 * be NULL.  Uses the handle's current factors and x~ and leaves its state alone (teacher-forced parity). */
int dotmi_probe_direction(dotmi_handle *h, const double *x, int32_t m, const double *S, const double *Y,
                          double *g, double *q, double *z, double *p, double *alpha0, double *E_trial);
/* derived mesh features, any pointer may be NULL: restTriInv nT*9 row-major, triArea nT, mass nV */
int dotmi_get_features(dotmi_handle *h, double *A, double *vol, double *mass);
/* dense principal sub-matrix R_s H R_s^T currently on the device (n_s = 3*local verts), row-major.
 * `inverse` != 0 returns the stored factor instead: X with H_s^-1 = X^T X (n_s x n_s, row-major).  On the
 * device X is the inverse Cholesky factor in the subdomain's nested-dissection order (lower triangular,
 * block-sparse); both matrices are returned in ascending-vertex order (l2g), i.e. X comes back as
 * P^T X_nd P.  l2g (local vertex -> global) may be NULL. */
int32_t dotmi_part_size(const dotmi_handle *h, int32_t part);
/* padded scalar size of the dense block every subdomain of this rank is stored in (the shared dissection layout: node
 * sizes are the maximum over the subdomains, rounded up to 64) -- what the factorisation's flop count is executed on */
int32_t dotmi_padded_size(const dotmi_handle *h);
/* bytes of HBM that hold the factors X_s of this rank's subdomains (compact 64-row blocks: ~1.2x the structural
 * non-zeros dotmi_step_stats.precond_bytes counts; DOTMI_TILE_FACTOR=0: nParts x padded_size^2 x 8) */
int64_t dotmi_factor_storage_bytes(const dotmi_handle *h);
/* which kernel family factorises this handle's subdomains (for measurement records): 1 = tile tasks, one launch per level
 * (tile_task_kernel), 2 = tile tasks as one dataflow launch (tile_flow_kernel), 3 = one launch pair per level: the diagonal
 * tasks in tile_task_kernel beside the product / row / inverse tasks on half tiles in tile_gemm_kernel (above 64 subdomains) */
int32_t dotmi_factor_kind(const dotmi_handle *h);
/* how many independent launch chains factorise this handle's subdomains: the subdomain groups of kind 1 (DOTMI_TILE_GROUPS: every
 * group's levels on a stream of its own, one fork in front, one join behind); 1 for one chain and for kinds 2 and 3 */
int32_t dotmi_factor_groups(const dotmi_handle *h);
/* which form of the block solve this handle's factors are in: 0 = the explicit inverse X_s = chol(H_s)^-1 of every subdomain,
 * streamed in one pass (p_s = X_s^T X_s r_s); 1 = the two-level form (round 6; default where form 0 would stream 240 MB or more per application over all subdomains of the mesh,
 * DOTMI_TWO_LEVEL): the inverse factors of the dissection's leaves and of the separator complement, and between them the panels
 * L_GD X_DD of the factor itself -- the forward / backward substitution of CHOLMODSolver::solve (CHOLMODSolver.cpp:149-163) across
 * that one boundary.  dotmi_part_matrix(inverse = 1) is an error in form 1 (there is no explicit inverse of a whole subdomain) */
int32_t dotmi_backsolve_form(const dotmi_handle *h);
/* (host only) the form dotmi_create chooses on its own for this mesh and partition, and the bytes per application of form 0 on its own
 * layout (over all subdomains) that decide it; tests/test_host_logic.py pins the choice for the BASELINE workloads */
int dotmi_plan_backsolve_form(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, const int32_t *epart, int32_t nParts,
                              int32_t *form, int64_t *one_pass_bytes);
int dotmi_part_matrix(dotmi_handle *h, int32_t part, int inverse, double *M, int32_t *l2g);
/* (host only) the scalar layout a DOTMI_FLAG_LBFGS_PD handle factors L in (the nested dissection of the whole vertex graph, one unknown
 * per vertex): its padded size and the bytes one application of L^-1 streams from the factor for all three coordinates -- 8 x the
 * structural non-zeros of X, as dotmi_step_stats.precond_bytes counts them (64-row blocks whose rows are longer than 2048 columns take
 * two passes, dots then scatter, and read their rows a second time, like the 3-dof back-solve beyond 5120 columns) */
int dotmi_plan_pd(int32_t nV, int32_t nT, const int32_t *T, const double *Xrest, int32_t *padded, int64_t *apply_bytes);
/* (host only) the plan of a DOTMI_FLAG_LBFGS_HI handle's block incomplete Cholesky (dot_amd/csrc/ic_plan.hpp): the vertex adjacency
 * coloured greedily in ascending vertex id (smallest colour no neighbour holds), the vertices ordered by (colour, id).  sizes[3] =
 * {colours, lower blocks nL, products nP}; call with NULL arrays first.  colour[nV], pos[nV] (order position of a vertex);
 * lptr[nV + 1] / lidx[nL]: per order position its lower neighbours' positions, ascending; lsrc[nL] / dsrc[nV]: the block of the global
 * block-CSR (vertex adjacency incl. self, ascending) behind a lower block / behind a position's diagonal; pptr[nL + 1], pa[nP], pb[nP]:
 * per lower block (i, j) the products L[pa] L[pb]^T = L_ik L_jk^T over the common lower neighbours k, ascending position of k.  Any
 * array may be NULL. */
int dotmi_plan_ic(int32_t nV, int32_t nT, const int32_t *T, int32_t *sizes, int32_t *colour, int32_t *pos, int32_t *lptr,
                  int32_t *lidx, int32_t *lsrc, int32_t *dsrc, int32_t *pptr, int32_t *pa, int32_t *pb);
/* DOTMI_FLAG_LBFGS_HI handles: the last factorisation's colour count, successful shift sigma and number of attempts */
int dotmi_ic_info(dotmi_handle *h, int32_t *colours, double *shift, int32_t *attempts);
/* DOTMI_FLAG_LBFGS_HI handles: the factor's 3 x 3 blocks, row-major, in plan order -- the nL lower blocks, then the nV lower-triangular
 * diagonal blocks by order position.  Returns their number nL + nV (blocks == NULL: only that); cap: room in blocks, in blocks. */
int dotmi_ic_factor(dotmi_handle *h, int32_t cap, double *blocks);
/* Newton-PCG (dot_amd/csrc/dotmi_pcg.hip): solve H u = b with the handle's current global projected Hessian (fixed rows are
 * identity) from u = 0 by conjugate gradients preconditioned with D^-1/2 S D^-1/2, S = the sum of the handle's current subdomain
 * solves.  b, u: nV*3.  Stops when the recursive residual |r| <= rel_tol |b|, after max_iter iterations, or on breakdown (a
 * non-positive or non-finite r.M r or curvature: NaN or rounding, H and the preconditioner being SPD); *iters = iterations done,
 * *rel_res = |r| / |b| at exit (either may be NULL); b = 0 returns u = 0 after 0 iterations.  Two solves of one system are
 * bit-identical, whatever the read-back interval.  Any handle that has both H and the block solve (DOT, two-level form, Newton, a
 * vpart, sharded subdomains in both sharding modes of the refresh -- the collectives of DOTMI_FLAG_NEWTON_PCG_DIST, with or without
 * that flag); on world > 1 EVERY rank must call it together, with the same b, rel_tol and max_iter, and every rank gets the same
 * u.  DOTMI_E_INVALID on LBFGS-PD, LBFGS-HI, GSDD and DOTMI_FLAG_OWNER_EXCHANGE handles, NULL b or u, rel_tol <= 0 or non-finite, max_iter < 1.  Returns 0
 * converged, 2 cap or breakdown (u is the last iterate), < 0 error (DOTMI_E_DEVICE on every rank when the ranks disagree). */
int dotmi_solve_hessian(dotmi_handle *h, const double *b, double *u, double rel_tol, int32_t max_iter, int32_t *iters,
                        double *rel_res);
/* the settings of DOTMI_FLAG_NEWTON_PCG's solves (rel_tol = the forcing term eta, max_iter) and, for dotmi_solve_hessian too, the
 * iterations enqueued between two reads of the device's verdict (check_every >= 1).  A bad value returns DOTMI_E_INVALID and
 * changes nothing.  No device work. */
int dotmi_set_pcg(dotmi_handle *h, double rel_tol, int32_t max_iter, int32_t check_every);
/* counters of the handle's PCG solves since create (steps and dotmi_solve_hessian alike); any pointer may be NULL */
int dotmi_pcg_info(const dotmi_handle *h, int64_t *solves, int64_t *iters_total, int32_t *last_iters, double *last_rel_res);
/* The rigid-mode coarse space of the PCG's preconditioner (dot_amd/csrc/dotmi_coarse.hip, k_coarse.hip; DESIGN.md section 9 -- the
 * reference has no counterpart).  mode 0 = off (the default: the solves run exactly the launches they run without this entry),
 * 1 = M = M_sym + Z A0^-1 Z^T with A0 = Z^T H Z and six columns of Z per subdomain s: on a vertex v of s the block
 * w_v [I | -[x_v - c_s]x], w_v = 1 / dup_v on free vertices and 0 on fixed ones, c_s the w-weighted centroid of s.  Every refresh of H
 * (a Newton iteration, dotmi_refactor, dotmi_refix, dotmi_set_time_step, dotmi_set_lame) marks A0 stale; the next solve with the mode
 * on rebuilds it with x = the handle's current iterate, frozen together with the centroids until the next build.  A subdomain with
 * fewer than 3 free vertices gets zero columns and an identity block.  If A0 still meets a non-positive pivot (collinear free
 * vertices) the coarse term is off until the next successful build: the solves run on M_sym alone, the handle is not poisoned.
 * DOTMI_E_INVALID on the handles dotmi_solve_hessian refuses, on sharded handles (world > 1, DOTMI_FLAG_FORCE_DIST: the sharded PCG
 * has no coarse space) and on a vpart handle, for any other mode, and above 256 subdomains
 * (A0^-1 is applied through a dense inverse factor of dimension 6 nParts <= 1536: a storage choice).  No device work. */
int dotmi_set_pcg_coarse(dotmi_handle *h, int32_t mode);
/* *dim = 6 nParts with the mode on, else 0; the subdomains the last build dropped; *active = 1 when the solves add the coarse term
 * (0 with the mode off, before the first build and after a failed factorisation); the builds since create.  Any pointer may be NULL. */
int dotmi_pcg_coarse_info(const dotmi_handle *h, int32_t *dim, int32_t *dropped_subdomains, int32_t *active, int64_t *builds);
/* the last assembled A0, dense dim x dim, row-major (identity blocks on dropped subdomains) -- for tests, like dotmi_ic_factor.
 * Returns dim (A0 == NULL: only that); cap: room in A0, in doubles; DOTMI_E_INVALID before the first build. */
int dotmi_pcg_coarse_matrix(dotmi_handle *h, int32_t cap, double *A0);
/* one application of the preconditioner exactly as the PCG uses it: w = M_sym r, plus Z A0^-1 Z^T r when the coarse term is active
 * (a stale A0 is rebuilt first).  r, w: nV*3.  Refused like dotmi_solve_hessian, and on sharded handles. */
int dotmi_pcg_apply_precond(dotmi_handle *h, const double *r, double *w);
/* The same rigid-mode coarse term in DOT's own loop (the reference has no counterpart, so iteration counts
 * differ from its: opt-in).  mode 0 = off (the default: every entry runs exactly the launches it runs without this one), 1 = the
 * two-loop recursion of dotmi_step, dotmi_apply_precond and dotmi_probe_direction use  M' = M + Z A0^-1 Z^T  with
 * M = D^-1 sum_s R_s^T H_s^-1 R_s the block preconditioner and Z, A0, the dropped-subdomain and the pivot rule those of
 * dotmi_set_pcg_coarse (one build serves both modes).  A0 is built behind every refresh of H (the end of a step, dotmi_refactor,
 * dotmi_refix, dotmi_set_time_step, dotmi_set_lame) at the positions the refresh was made at, and by this entry when it switches the
 * mode on; its pivot flag is read with the refresh's own synchronisation.  A non-positive pivot switches the term off until the next
 * successful build: the step runs on M, the handle is not poisoned.  A step with the mode on does not take the unit step
 * speculatively (DOTMI_SPEC_STEP).  DOTMI_E_INVALID with a message on a handle of more than one rank, with DOTMI_FLAG_FORCE_DIST,
 * _OWNER_EXCHANGE, _GSDD, _NEWTON, _NEWTON_PCG, _LBFGS_PD, _LBFGS_HI or _ASYNC_REFRESH, on a vpart handle, for any other mode, and
 * above 256 subdomains.  (A sharded handle takes the term at create: DOTMI_FLAG_DOT_COARSE.)  This entry takes 0 and 1 and refuses
 * every other value as it always has; the balanced form is mode 2 of dotmi_set_dot_coarse_mode below. */
int dotmi_set_dot_coarse(dotmi_handle *h, int32_t mode);
/* The coarse term of DOT's own loop by mode (new with this library: the reference has no counterpart, so iteration counts differ from
 * its: opt-in).  mode 0 and mode 1 are dotmi_set_dot_coarse(h, 0 / 1) exactly -- one handle state behind both entries.
 * mode 2 = the balanced form: the same Z and A0 project the coarse space out on both sides of the block solve,
 *     M'' = C + (I - C H) M (I - H C),   C = Z A0^-1 Z^T,
 * applied as  y1 = A0^-1 Z^T r,  r1 = r - W y1,  u = M r1,  y2 = A0^-1 W^T u,  M'' r = u + Z (y1 - y2)  with W = H Z kept as a sparse
 * table of 3 x 6 blocks that is rebuilt with A0 -- no product with H per application.  M'' H Z y = Z y: the coarse space is solved
 * exactly.  Six small launches per application around the unchanged block solve; a step with mode 2 active runs the device loop in
 * its q-based order (the early order forms z inside its merge, before y2 exists).  It about halves mode 1's iterations where the
 * rigid modes carry the error (bars), gains little on stiff meshes and costs more per iteration
 * (profiles/dot_coarse_balanced.txt).  Refused (DOTMI_E_INVALID with a message) where dotmi_set_dot_coarse is, which includes every
 * sharded handle (DOTMI_FLAG_DOT_COARSE stays mode 1), and for any value other than 0, 1, 2.  Switching on a live handle follows one
 * rule: a switch from 0 builds A0 (and W for mode 2) now, 1 -> 2 builds W with a fresh A0, 2 -> 1 keeps the build.
 * (The mode has an entry of its own because dotmi_set_dot_coarse has refused the value 2 since it exists and callers may rely on it.) */
int dotmi_set_dot_coarse_mode(dotmi_handle *h, int32_t mode);
/* the mode the two setters (or DOTMI_FLAG_DOT_COARSE) have left on the handle: 0, 1 or 2 (0 for NULL) */
int32_t dotmi_dot_coarse_mode(const dotmi_handle *h);
/* *dim = 6 nParts with the mode on, else 0; the subdomains the last build dropped; *active = 1 when the applications add the coarse
 * term; the coarse builds since create (both modes); the device time of the last one in ms.  Any pointer may be NULL. */
int dotmi_dot_coarse_info(const dotmi_handle *h, int32_t *dim, int32_t *dropped_subdomains, int32_t *active, int64_t *builds,
                          double *last_build_ms);
/* (host only) the lists of the coarse space (dot_amd/csrc/coarse_plan.hpp) for an element partition epart[nT] into nParts <= 256
 * subdomains.  sizes[3] = {coupled pairs nP, entries nE, (vertex, subdomain) incidences nI}; call with NULL arrays first.
 * pairS[nP], pairT[nP]: every unordered pair of subdomains some H block couples once, s <= t, diagonals included, ordered by (s, t);
 * pairPtr[nP + 1] / pairBlk[nE]: per pair the H blocks (i, j) with i in s and j in t as indices into the global block-CSR (vertex
 * adjacency incl. self, ascending), ascending -- one entry per (H block, s containing i, t containing j, s <= t); vsPtr[nV + 1] /
 * vsIdx[nI]: per vertex its subdomains, ascending; svPtr[nParts + 1] / svIdx[nI]: per subdomain its vertices, ascending.  Any array
 * may be NULL. */
int dotmi_plan_coarse(int32_t nV, int32_t nT, const int32_t *T, const int32_t *epart, int32_t nParts, int32_t *sizes, int32_t *pairS,
                      int32_t *pairT, int32_t *pairPtr, int32_t *pairBlk, int32_t *vsPtr, int32_t *vsIdx, int32_t *svPtr,
                      int32_t *svIdx);
/* (host only) the lists of W = H Z for mode 2 of dotmi_set_dot_coarse_mode (coarse_plan.hpp, CoarseHzPlan), same mesh arguments.
 * sizes[2] = {entries nE, H blocks nB}; call with NULL arrays first.  An entry is a (vertex i, subdomain t) with an H block (i, j),
 * j in t.  hzPtr[nV + 1] / hzSub[nE]: per vertex the subdomains of its entries, ascending; hzVert[nE]: an entry's vertex;
 * hzBlkPtr[nE + 1] / hzBlk[nB]: per entry its H blocks as indices into the global block-CSR, ascending (the summation order of
 * W[i, t]); hzTPtr[nParts + 1] / hzTEnt[nE]: per subdomain its entries in ascending vertex.  Any array may be NULL. */
int dotmi_plan_coarse_hz(int32_t nV, int32_t nT, const int32_t *T, const int32_t *epart, int32_t nParts, int32_t *sizes, int32_t *hzPtr,
                         int32_t *hzSub, int32_t *hzVert, int32_t *hzBlkPtr, int32_t *hzBlk, int32_t *hzTPtr, int32_t *hzTEnt);

/* ---- measurement ------------------------------------------------------------------------------ */
/* Launch the subdomain back-solve kernel `reps` times on the handle's stream between two HIP events
 * and return the average milliseconds per launch and the algorithmic bytes per launch. */
int dotmi_bench_precond(dotmi_handle *h, int32_t reps, double *ms_per_launch, int64_t *bytes_per_launch);
int dotmi_bench_energy(dotmi_handle *h, int32_t reps, double *ms_per_launch, int64_t *bytes_per_launch);
/* The same for every kernel class of the path (SURVEY.md section 8d "per kernel class"): `reps` back-to-back launches on
 * the handle's resident state between two HIP events on the library's stream; bytes = algorithmic bytes of one launch
 * (formulas: DESIGN.md section 4).  Call between steps. */
enum dotmi_bench_kind {
    DOTMI_BENCH_ELEM_ENERGY_GRAD = 0, /* element pass: energy + per-(patch, vertex) partial gradients */
    DOTMI_BENCH_ELEM_ENERGY = 1,      /* element pass, energy only (line-search retries) */
    DOTMI_BENCH_VERTEX_GATHER = 2,    /* vertex pass: gradient + new L-BFGS pair + its 21 statistics */
    DOTMI_BENCH_SPMV_DOTS = 3,        /* H p and the two dots of alpha_0 */
    DOTMI_BENCH_BACKSOLVE = 4,        /* subdomain back-solve (all kernels of one application) */
    DOTMI_BENCH_MERGE = 5,            /* sum over subdomains / dup (+ y_i . z) */
    DOTMI_BENCH_BUILD_QPAD = 6,       /* two-loop first half into the padded right-hand sides */
    DOTMI_BENCH_BUILD_P = 7,          /* two-loop second half */
    DOTMI_BENCH_STEP_FORWARD = 8,     /* x_trial = x + alpha p */
    DOTMI_BENCH_ELEM_HESSIAN = 9,     /* projected 12x12 element Hessians (once per step) */
    DOTMI_BENCH_ASSEMBLE = 10,        /* global block-CSR assembly (once per step) */
    /* the forms the device loop's early order launches (they read the loop state the last step left on the device; the
     * handle must have run a step): */
    DOTMI_BENCH_SPMV_ZP = 11,         /* build_p + SpMV + dots in one launch on cached H s_j */
    DOTMI_BENCH_MERGE_EARLY = 12,     /* tile partials -> u, M y_new, z, y_i . z */
    DOTMI_BENCH_ELEM_STEP = 13,       /* element pass that takes the line-search step itself */
    DOTMI_BENCH_GATHER_EARLY = 14,    /* vertex pass that also writes -g into the padded right-hand sides and H s_new */
    DOTMI_BENCH_DIRSTEP = 15,         /* (round 6) the speculative unit-step launch: direction kernel + element pass + trial point in one launch */
    DOTMI_BENCH_ELEM_VERTEX = 16,     /* (round 6) element pass + step + vertex gather of a trial in one launch on vertex patches */
    DOTMI_BENCH_COUNT = 17
};
int dotmi_bench_kernel(dotmi_handle *h, int32_t kind, int32_t reps, double *ms_per_launch, int64_t *bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* DOTMI_H */
