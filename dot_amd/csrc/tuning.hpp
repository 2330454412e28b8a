// tuning.hpp -- the environment switches of libdotmi as one struct (host only, no HIP): dotmi_create reads them into the handle,
// the planning entries of dotmi_plan.cpp that mirror its choices (dotmi_plan_layout, dotmi_plan_backsolve_tiles) read them the same way.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "nd_layout.hpp"

// ---- tuning / ablation switches -----------------------------------------------------------------------------------
// Read ONCE per dotmi_create from the environment; every one is optional and the defaults are the product path.  They
// exist for the A/B measurements logged under profiles/ (tools/ab.sh) and for tests that force a code path; none changes
// results beyond rounding.  Listed in include/dotmi.h ("Environment") and DESIGN.md section 10.
struct Tuning {
    int ndLevels = -1;        // DOTMI_ND_LEVELS      depth of the nested dissection (-1: nd_default_levels)
    int ndMin = dotmi::ND_MIN_SPLIT; // DOTMI_ND_MIN         smallest region (scalars) that is still split
    bool ndMinByUser = false; //                      (set at all: the depth rule of block_plan.hpp keeps the caller's threshold)
    bool wavePacks = true;    // DOTMI_WAVE_PACKS=0   small back-solve tiles as one-tile jobs like the others instead of four per workgroup
    int tilePasses = 4;       // DOTMI_TILE_PASSES    most passes (of 8 rows) a back-solve tile of rows beyond 1024 columns takes (8: 64-row tiles)
    int tileRows = 0;         // DOTMI_TILE_ROWS      rows per back-solve tile (0: 64, or 32 for few subdomains)
    int tileRowsLong = 0;     // DOTMI_TILE_ROWS_LONG rows per back-solve tile when the rows have more than 1536 columns (0: as the
                              //                      other rows, or ~256 KB tiles where few subdomains leave the launch bound by
                              //                      its longest tile)
    int twoLevel = -1;        // DOTMI_TWO_LEVEL      1: the back-solve in its two-level form (leaves against the separator complement,
                              //                      DevTwoLevel); 0: the explicit inverse in one pass; -1: two-level where one pass would stream >= 240 MB
    int splitMerge = -1;      // DOTMI_SPLIT_MERGE    1 / 0: the merge as reduce_partial_p + a gather from psub (the early order included) /
                              //                      as one walk over the tile partials; default: split from 400 k scalar dofs
    bool fuseLog = false;     // DOTMI_FUSE_LOG       print the fused-leaf units
    bool factorGraph = true;  // DOTMI_FACTOR_GRAPH=0 the level launches of the factorisation issued directly instead of replayed as a hipGraph
    int shardElems = -1;      // DOTMI_SHARD_ELEMS    0 / 1: force the replicated / sharded element pass (-1: by size)
    int shardHess = -1;       // DOTMI_SHARD_HESS     0 / 1: force the replicated / sharded once-per-step phase
    int timeStride = 8;       // DOTMI_TIME_STRIDE    DOTMI_FLAG_TIME_BACKSOLVE brackets every n-th back-solve
    int patchElems = 0;       // DOTMI_PATCH_ELEMS    elements per patch of the element pass (0: default)
    int tileSplit = -1;       // DOTMI_TILE_SPLIT     0 / 1: one task kernel per level / diagonal and half-tile kernels side by side
                              //                      (-1: the latter above 64 subdomains, where the factorisation is throughput-bound)
    int tileGroups = -1;      // DOTMI_TILE_GROUPS    the level launches of the factorisation as G independent chains of subdomain groups,
                              //                      each on a stream of its own (0 / 1: one chain; at most 4; -1: two -- choose_tile_groups)
    int tileHfill = 1;        // DOTMI_TILE_HFILL     1 (default): the first task of an H tile builds it in LDS from the tile's entry list --
                              //                      the refresh neither clears nor fills the work buffer; 0: clear_tiles + dense_fill
                              //                      into the work buffer, which the first task reads back (until round 7)
    int tileEagerMin = 0;     // DOTMI_TILE_EAGER_MIN early products a critical-path tile task may keep
    int fastDiag = 1;         // DOTMI_FAST_DIAG      1 / 0: the diagonal tile tasks' 16 x 16 bottom steps on 4 x 4 blocks every lane factors for
                              //                      itself (12.0 us per 64 x 64 step) / one row per lane with v_readlane operands (15.3 us)
    int tileFlow = -1;        // DOTMI_TILE_FLOW      1: the factorisation as ONE launch of persistent workgroups with per-task
                              //                         dependencies (tile_flow_kernel) instead of one launch per level; 0: never;
                              //                         default: where a level holds fewer tasks than the GPU holds workgroups
    int tileFlowWaitMs = 2000;   // DOTMI_TILE_FLOW_WAIT_MS  a task that waits longer for one of its dependencies gives up (error)
    int tileEagerMinRmul = -1; // DOTMI_TILE_EAGER_MIN_RMUL early products the last task of a Q tile may keep (-1: as the others; 0: none)
    bool tileEagerMinRmulByUser = false;   //           (unset: one up to 64 subdomains, as the others above)
    bool fuseDir = true;      // DOTMI_FUSE_DIR=0     (early order) build_p and spmv_dots as two launches instead of one on cached H s_j
    int wideForms = -1;       // DOTMI_WIDE_FORMS     -1 (default): the vertex gather, the early merge and the direction kernel choose their
                              //                      narrow or wide form by the size of the mesh (loop_forms.hpp); any other value is a bit
                              //                      mask -- 1 gather, 2 early merge, 4 direction kernel -- whose set bits force the wide form
                              //                      (512 / 512 / 1024 threads) and whose clear bits force the narrow one (0: all narrow,
                              //                      7: all wide); reaches the launchers as GatherArgs / MergeEarlyArgs / SpmvZpArgs::wide
    bool fuseStep = true;     // DOTMI_FUSE_STEP=0    (early order) step_forward as a launch of its own instead of inside the element pass
    int pairTrials = -1;      // DOTMI_PAIR_TRIALS    -1 (default): paired line-search trials (StepArgs::pairBlocks) in a step whose predecessor
                              //                      halved in at least a quarter of its iterations; 1: in every step; 0: never
    int vertexPatches = -1;   // DOTMI_VERTEX_PATCHES 0: the element pass and the vertex gather of a trial as two launches on element patches
                              //                      (until round 5); -1 (default): as ONE launch on vertex patches (k_elemvert.hip) where every
                              //                      patch is a workgroup of its own (<= 512 patches, one rank); 1: the same rule (reserved)
    int specStep = 0;         // DOTMI_SPEC_STEP      the unit step taken speculatively beside the direction kernel (k_dirstep.hip): 0 (default)
                              //                      never -- measured: the fused launch is as long as its two parts, profiles/r06_spec_step.txt;
                              //                      -1: in a step whose predecessor's first trials took the unit estimate at least nine times
                              //                      in ten; 1: in every step
    bool earlyHold = true;    // DOTMI_EARLY_HOLD=0   the back-solve of a trial that is expected to be rejected still starts speculatively
    int earlyBs = 2;          // DOTMI_EARLY_BACKSOLVE 0: the back-solve after the controller, on q; 1: speculatively on the trial
                              //                      gradient with the controller inside its launch, in the steps where
                              //                      the last step's counts say it pays (choose_step_forms); 2 (default): in
                              //                      every step
    int operandRecords = 1;   // DOTMI_OPERAND_RECORDS bit 0 (default on): elem_vertex_kernel's per-owned-vertex operands as records --
                              //                      the static ones in patch order (VpOwnRec), the stored pairs as (s, y) entries
                              //                      (DevLoop::hrec), p and x~ of the owned dofs through LDS; 0: the flat arrays behind
                              //                      the vertex id (until round 8).  Bit-identical either way
    static int geti(const char *name, int dflt)
    {
        const char *ev = getenv(name);
        return ev ? atoi(ev) : dflt;
    }
    static Tuning from_env()
    {
        Tuning t;
        t.wavePacks = geti("DOTMI_WAVE_PACKS", 1) != 0;
        t.tilePasses = std::min(8, std::max(1, geti("DOTMI_TILE_PASSES", 4)));
        t.ndLevels = geti("DOTMI_ND_LEVELS", -1);
        if (t.ndLevels < -1) t.ndLevels = 0;
        t.ndMin = std::max(128, geti("DOTMI_ND_MIN", dotmi::ND_MIN_SPLIT));
        t.ndMinByUser = getenv("DOTMI_ND_MIN") != nullptr;
        if (const char *ev = getenv("DOTMI_TILE_ROWS")) t.tileRows = std::min(64, std::max(8, atoi(ev) / 8 * 8));
        t.tileRowsLong = geti("DOTMI_TILE_ROWS_LONG", 0);
        if (t.tileRowsLong > 0) t.tileRowsLong = std::min(64, std::max(8, t.tileRowsLong / 8 * 8));
        t.splitMerge = geti("DOTMI_SPLIT_MERGE", -1);
        t.twoLevel = geti("DOTMI_TWO_LEVEL", -1);
        t.fuseLog = getenv("DOTMI_FUSE_LOG") != nullptr;
        t.factorGraph = geti("DOTMI_FACTOR_GRAPH", 1) != 0;
        t.shardElems = geti("DOTMI_SHARD_ELEMS", -1);
        t.shardHess = geti("DOTMI_SHARD_HESS", -1);
        t.timeStride = std::max(1, geti("DOTMI_TIME_STRIDE", 8));
        t.patchElems = std::max(0, geti("DOTMI_PATCH_ELEMS", 0));
        t.tileSplit = geti("DOTMI_TILE_SPLIT", -1);
        t.tileGroups = geti("DOTMI_TILE_GROUPS", -1);
        t.tileHfill = geti("DOTMI_TILE_HFILL", 1) != 0;
        t.tileEagerMin = std::max(0, geti("DOTMI_TILE_EAGER_MIN", 0));
        t.tileFlow = geti("DOTMI_TILE_FLOW", -1);
        t.fastDiag = geti("DOTMI_FAST_DIAG", 1);
        t.tileFlowWaitMs = std::max(1, geti("DOTMI_TILE_FLOW_WAIT_MS", 2000));
        t.tileEagerMinRmul = geti("DOTMI_TILE_EAGER_MIN_RMUL", -1);
        t.tileEagerMinRmulByUser = getenv("DOTMI_TILE_EAGER_MIN_RMUL") != nullptr;
        t.earlyBs = geti("DOTMI_EARLY_BACKSOLVE", 2) != 0 ? 2 : 0;   // (1, round 3's per-step rule, now means "on")
        t.earlyHold = geti("DOTMI_EARLY_HOLD", 1) != 0;
        t.pairTrials = geti("DOTMI_PAIR_TRIALS", -1);
        t.specStep = geti("DOTMI_SPEC_STEP", 0);
        t.vertexPatches = geti("DOTMI_VERTEX_PATCHES", -1);
        t.fuseStep = geti("DOTMI_FUSE_STEP", 1) != 0;
        t.fuseDir = geti("DOTMI_FUSE_DIR", 1) != 0;
        t.wideForms = geti("DOTMI_WIDE_FORMS", -1);
        if (t.wideForms < -1) t.wideForms = -1;
        t.operandRecords = geti("DOTMI_OPERAND_RECORDS", 1) & 1;
        return t;
    }
};
