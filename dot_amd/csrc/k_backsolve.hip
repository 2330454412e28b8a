// k_backsolve.hip -- subdomain back-solve (DOTTimeStepper.cpp:406-431) and the kernels that run the loop controller (k_loopctl.hpp):
// a launch of its own, or workgroup 0 of the back-solve launch
// (one translation unit per kernel family since round 6: an edit to one family no longer moves the register allocation and
// scalar loads of the others; every unit is compiled once.  Conventions and the reference map: k_device.hpp)
#include "bs_forms.hpp"
#include "k_device.hpp"
#include "k_loopctl.hpp"
#include "loop_forms.hpp"

namespace dotmi {

// the controller as a launch of its own: one workgroup, the plain form (the q-based order; back-solves with no 256-thread launch)
__global__ __launch_bounds__(256) void loop_control_kernel(DevLoop *__restrict__ ctl,
                                                           const double *__restrict__ partE, int nbE,
                                                           const double *__restrict__ partR,
                                                           const double *__restrict__ alpha_dev,
                                                           int *__restrict__ flags_host, int init)
{
    loop_control_body<CTL_PLAIN>(ctl, partE, nbE, partR, alpha_dev, flags_host, init);
}

void launch_loop_control(DevLoop *ctl, const double *partE, int nbE, const double *partR,
                         const double *alpha_dev, int *flags_host, hipStream_t st, int init)
{
    hipLaunchKernelGGL(loop_control_kernel, dim3(1), dim3(256), 0, st, ctl, partE, nbE, partR, alpha_dev, flags_host,
                       init);
}

__global__ __launch_bounds__(256) void gather_pad_kernel(int total, const int *__restrict__ dofmap,
                                                         const double *__restrict__ q, double *__restrict__ rpad)
{
    const int stride = gridDim.x * blockDim.x;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += stride) {
        const int d = dofmap[k];
        rpad[k] = d >= 0 ? q[d] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------
// subdomain back-solve  p_s = H_s^-1 r_s = X^T (X r_s),  X = chol(H_s)^-1  (lower triangular)
//   -- THE HBM-bound kernel of the L-BFGS loop.
// Storage: memory row i holds row i of X, X(i,k) for k <= i, contiguously (zeros for k > i); that is
//   the column-major upper factor Q = R^-1 of H = R^T R that chol_inv_tree() produces.  In the
//   nested-dissection order of the subdomain (nd_layout.hpp) row i is non-zero only from the first
//   column of its tree node on, so X is block-sparse.
// One pass: for every memory row i   t_i = row_i . r   and then   p += t_i * row_i
//   so each stored entry is read from HBM exactly ONCE per back-solve:
//   algorithmic bytes per launch = 8 x the structural non-zeros of all X_s (dotmi_step_stats.precond_bytes).
// A workgroup owns up to BS_ROWS consecutive rows of one tree region of one subdomain and walks them a
// few at a time: the rows sit in VGPRs (16 B per lane per row chunk), their dot products are combined
// with a transposed butterfly (10 shuffles instead of 48) + one LDS exchange, and the rank-k update of
// p is applied from the same registers.  Loads stop at the 128-byte line of each row's diagonal and
// skip the identity-padding columns.  The workgroup's partial p goes to ppart[s][tile][.]; the tiles
// of a subdomain are summed in fixed order by reduce_partial_p_kernel (no atomics, deterministic).
// ------------------------------------------------------------------------------------------------
constexpr int BS_ROWS = 64;   // memory rows per workgroup
typedef double nt_double2 __attribute__((ext_vector_type(2)));

// ---- the tile walk, stated once for the three tile bodies (workgroup tile, wavefront tile, two-phase kernel) -----------------
// The geometry of a tile, from its job record (bs_tiles.hpp: part, first row, tile index in the part | rows << 16, first column)
struct BsTile {
    int s, i0, tileIdx, cb;
    int ns;      // one past the last live row of this tile
    int ncol;    // columns cb <= k < ns can be non-zero in these rows (nested dissection: everything left of the tile's node is
                 // structurally zero); whole 128-byte lines are loaded
    // the tile's rows lie in ONE 64-row block of the factor storage (dotmi_internal.hpp RowTile): row i, column c is at
    // W[rt.off + (i - first row of the block) * rt.ld + (c - rt.c0)] = Ws[i * ldw + c]
    int ldw;
    const double *Ws, *rp;   // rp: the right-hand side in padded order (zeros on the padding)
    const int *dm;
    double *ppart;
    int nmax, nbmax;
    __device__ __forceinline__ double *out() const { return ppart + ((size_t)s * nbmax + tileIdx) * nmax; }   // the tile's partial result
};
__device__ __forceinline__ BsTile bs_tile(const int4 jb, int nmax, const RowTile *rt, const double *W, const int *dofmap, const double *q,
                                          double *ppart, int nbmax)
{
    BsTile g;
    g.s = jb.x, g.i0 = jb.y, g.tileIdx = jb.z & 0xffff, g.cb = jb.w;
    g.ns = g.i0 + (jb.z >> 16);
    g.ncol = min((g.ns + 15) & ~15, nmax);
    const RowTile rb = rt[(size_t)g.s * (nmax >> 6) + (g.i0 >> 6)];
    g.ldw = rb.ld;
    g.Ws = W + (rb.off - (long long)(g.i0 & ~63) * g.ldw - rb.c0);
    g.dm = dofmap + (size_t)g.s * nmax;
    g.rp = q + (size_t)g.s * nmax;
    g.ppart = ppart, g.nmax = nmax, g.nbmax = nbmax;
    return g;
}
// The first column a lane's pair at column c is NOT loaded for: c itself, or never when both columns are identity padding -- padding
// columns of live rows hold zeros (separator rows span the padding of every region): not read.  rhs: also the right-hand side pair.
// (PAIR: the dofmap pair with one 8-byte load; the two-phase kernel keeps its two 4-byte loads)
template <bool PAIR = true>
__device__ __forceinline__ int bs_pair_end(const BsTile &g, int c, double2 *rhs)
{
    int d0, d1;
    if constexpr (PAIR) {
        const int2 dd = (c < g.ncol) ? *reinterpret_cast<const int2 *>(g.dm + c) : make_int2(-1, -1);
        d0 = dd.x, d1 = dd.y;
    } else {
        d0 = (c < g.ncol) ? g.dm[c] : -1, d1 = (c < g.ncol) ? g.dm[c + 1] : -1;
    }
    if (rhs) *rhs = (c < g.ncol) ? *reinterpret_cast<const double2 *>(g.rp + c) : make_double2(0.0, 0.0);
    return (d0 >= 0 || d1 >= 0) ? c : 0x7fffffff;
}
// the first column of pair m of lane `lane` of LANES, from column c0 on
template <int LANES>
__device__ __forceinline__ int bs_col(int c0, int lane, int m) { return c0 + 2 * lane + 2 * LANES * m; }
// SUB rows from row ib on into the registers y[SUB][CH] of the enclosing tile body (its g, ib, cend): the lane's CH pairs, zeros past the
// tile's last row.  A row is zero right of its diagonal: loads stop at the end of its own 128-byte line, not of the tile.
// NT: streamed once per launch by exactly one workgroup: non-temporal, so the 229 MB of factors do not push the small hot arrays of
// the other loop kernels out of the 256 MB Infinity Cache (the two-phase kernel reads its rows twice: plain loads).
// (A macro: from an inlined function the same loads came out with other address arithmetic -- the 256-thread kernels at 256 VGPRs
// instead of 254 with one spilled, the 512-thread kernel with 18 spilled instead of 1.)
#define BS_LOAD_ROWS(SUB_, CH_, LANES_, NT_, c0_, lane_)                                                                     \
    _Pragma("unroll") for (int rr = 0; rr < SUB_; ++rr)                                                                      \
    {                                                                                                                        \
        const double *row = g.Ws + (long long)min(ib + rr, g.ns - 1) * g.ldw;                                                \
        const int rend = ((ib + rr) < g.ns) ? min(g.ncol, (ib + rr + 16) & ~15) : 0;                                         \
        _Pragma("unroll") for (int m = 0; m < CH_; ++m)                                                                      \
        {                                                                                                                    \
            const int c = bs_col<LANES_>(c0_, lane_, m);                                                                     \
            if (cend[m] >= rend) {                                                                                           \
                y[rr][m] = make_double2(0.0, 0.0);                                                                           \
            } else if constexpr (NT_) {                                                                                      \
                const nt_double2 v = __builtin_nontemporal_load(reinterpret_cast<const nt_double2 *>(row + c));              \
                y[rr][m] = make_double2(v.x, v.y);                                                                           \
            } else {                                                                                                         \
                y[rr][m] = *reinterpret_cast<const double2 *>(row + c);                                                      \
            }                                                                                                                \
        }                                                                                                                    \
    }
template <int CH, int LANES>
__device__ __forceinline__ void bs_store(const BsTile &g, int c0, int lane, const double2 (&pacc)[CH])
{
    double *out = g.out();
#pragma unroll
    for (int m = 0; m < CH; ++m) {
        const int c = bs_col<LANES>(c0, lane, m);
        if (c < g.ncol) *reinterpret_cast<double2 *>(out + c) = pacc[m];
    }
}

// One tile with rows of at most 2*THREADS*MAXCH columns, SUB rows in registers at a time.  Short rows
// (the leaves of the dissection) take many rows per pass, long rows few, so that every pass has about
// the same number of bytes in flight: the pass count of a tile -- a chain of HBM latency, butterfly
// and LDS exchange -- is what bounds a tile, not its byte count.
// RLDS (round 5, rows of 2561 .. 3072 columns on the 256-thread kernel): the thread's right-hand side entries live in LDS
// (rs: each thread reads back only what it wrote -- a manual spill of 24 registers) so that six chunks of rows fit the
// register tile at two workgroups per CU; the dot products keep their order of additions (chunk after chunk).
// (The dot products are one statement for both storage kinds, chunk after chunk into each of eight sums.  The update is not: in the
// RLDS branch's order -- all row sums first -- the 512-thread kernel goes from 1 spilled VGPR to 13, so its two branches stay.)
template <int THREADS, int MAXCH, int SUB, bool RLDS>
__device__ __forceinline__ void backsolve_tile(const int4 jb, const int *__restrict__ dofmap, const double *__restrict__ W, int nmax,
                                               const RowTile *__restrict__ rt, const double *__restrict__ q, double *__restrict__ ppart,
                                               int nbmax, double (*sm)[THREADS / 64][32], const int *__restrict__ abortp, int epoch,
                                               int *s_abort, double2 *__restrict__ rs)
{
    constexpr int NW = THREADS / 64;
    const BsTile g = bs_tile(jb, nmax, rt, W, dofmap, q, ppart, nbmax);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double2 r[RLDS ? 1 : MAXCH], pacc[MAXCH];   // (RLDS: both in LDS, rs[.] and rs[THREADS * MAXCH + .])
    int cend[MAXCH];  // first column this thread's pair of chunk m is NOT loaded for: 0 for identity-padding columns
#pragma unroll
    for (int m = 0; m < MAXCH; ++m) {
        double2 rv;
        cend[m] = bs_pair_end(g, bs_col<THREADS>(g.cb, tid, m), &rv);
        if constexpr (RLDS) {
            rs[tid + THREADS * m] = rv;
            rs[THREADS * MAXCH + tid + THREADS * m] = make_double2(0.0, 0.0);
        } else {
            r[m] = rv;
            pacc[m] = make_double2(0.0, 0.0);
        }
    }
#pragma unroll 1
    for (int sb = 0; sb < BS_ROWS / SUB; ++sb) {
        const int ib = g.i0 + sb * SUB;
        if (ib >= g.ns) break;
        // speculative launch: has the controller (workgroup 0 of the launch) rejected the trial meanwhile?  One thread asks,
        // the answer is shared through LDS behind this pass' barrier (double-buffered like sm), so the whole workgroup
        // leaves together
        // (requested here, in front of the pass' row loads; stored to LDS only next to the dot products, so that the
        // asking wave does not wait for the answer before it issues its rows)
        int abortSeen = 0;
        if (abortp && tid == 0) abortSeen = __hip_atomic_load(abortp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double2 y[SUB][MAXCH];
        BS_LOAD_ROWS(SUB, MAXCH, THREADS, true, g.cb, tid);
        const int buf = sb & 1;
#pragma unroll
        for (int gr = 0; gr < SUB / 8; ++gr) {
            double d[8];
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) d[rr] = 0.0;
#pragma unroll
            for (int m = 0; m < MAXCH; ++m) {
                const double2 rv = RLDS ? rs[tid + THREADS * m] : r[m];
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) d[rr] += y[8 * gr + rr][m].x * rv.x + y[8 * gr + rr][m].y * rv.y;
            }
            // transposed butterfly: 8 values over 64 lanes -> lane group lane>>3 holds one row's wave sum
            const double e1 = wave_sum8_transposed(d, tid);
            // lane bits (5,4,3) = (b2,b1,b0): row index = 4*b2 + 2*b1 + b0
            if ((lane & 7) == 0) sm[buf][wv][8 * gr + (lane >> 3)] = e1;
        }
        if (abortp && tid == 0) s_abort[sb & 1] = abortSeen;
        __syncthreads();
        if (abortp && s_abort[sb & 1] == epoch) return;   // the result would not be used
        if constexpr (RLDS) {
            // the same additions in the same order (row after row into each accumulator), the accumulators through LDS
            double t[SUB];
#pragma unroll
            for (int rr = 0; rr < SUB; ++rr) {
                double a = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) a += sm[buf][w][rr];
                t[rr] = a;
            }
#pragma unroll
            for (int m = 0; m < MAXCH; ++m) {
                double2 pa = rs[THREADS * MAXCH + tid + THREADS * m];
#pragma unroll
                for (int rr = 0; rr < SUB; ++rr) {
                    pa.x += t[rr] * y[rr][m].x;
                    pa.y += t[rr] * y[rr][m].y;
                }
                rs[THREADS * MAXCH + tid + THREADS * m] = pa;
            }
        } else {
#pragma unroll
        for (int rr = 0; rr < SUB; ++rr) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += sm[buf][w][rr];
#pragma unroll
            for (int m = 0; m < MAXCH; ++m) {
                pacc[m].x += t * y[rr][m].x;
                pacc[m].y += t * y[rr][m].y;
            }
        }
        }
    }
    if constexpr (RLDS) {
#pragma unroll
        for (int m = 0; m < MAXCH; ++m) pacc[m] = rs[THREADS * MAXCH + tid + THREADS * m];
    }
    bs_store<MAXCH, THREADS>(g, g.cb, tid, pacc);
}

// -DBS_PROFILE (tools/prof_backsolve.sh): per job of the launch its start, end, longest row, rows (negative: a pack; the rows of its
// first tile) and the hardware and XCC id (of a pack: wavefront 0's)
#ifdef BS_PROFILE
__device__ long long g_bs_prof[8192][5];
extern "C" int dotmi_debug_bs_prof(long long *out, int n) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bs_prof), sizeof(long long) * 5 * (size_t)n); }
#endif
__device__ __forceinline__ void bs_prof_begin(int jobIdx, const int4 jb, bool pack)
{
#ifdef BS_PROFILE
    if (threadIdx.x == 0 && jobIdx < 8192) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_bs_prof[jobIdx][0] = wall_clock64();
        g_bs_prof[jobIdx][2] = jb.y + (jb.z >> 16) - jb.w;
        g_bs_prof[jobIdx][3] = pack ? -(jb.z >> 16) : jb.z >> 16;
        g_bs_prof[jobIdx][4] = (long long)hw | ((long long)(xcc & 15) << 32);
    }
#endif
}
__device__ __forceinline__ void bs_prof_end(int jobIdx, bool pack)   // (a pack: wavefront 0 of the four)
{
#ifdef BS_PROFILE
    if (!pack) __syncthreads();
    if (threadIdx.x == 0 && jobIdx < 8192) g_bs_prof[jobIdx][1] = wall_clock64();
#endif
}

// ---- small tiles, one WAVEFRONT each (round 5) -----------------------------------------------------------------------------
// On a deep dissection most tiles are small: bar17K on three levels has 1163 tiles of which 796 have rows of at most 256
// columns -- 68 % of the workgroups for 17 % of the bytes (512 of them average 24 KB), each holding a 252-register slot of the
// launch for ~10 us of latency (descriptor -> right-hand side -> rows -> butterfly -> LDS exchange -> barrier; tools/
// prof_backsolve.sh: every slot of the GPU busy for the whole launch, 3.9 TB/s).  Four such tiles share a workgroup now,
// one wavefront each, with nothing in common: no LDS, no barrier -- lane l holds columns cb + 2 l (+ 128), 16 rows per pass
// in registers, the rows' dot products through the transposed butterfly and v_readlane broadcasts, the rank-16 update from the
// same registers.  The tile's partial result goes where the block form puts it (ppart[s][tile][.]).
__device__ __forceinline__ double bs_readlane(double v, int srclane)
{
    union {
        double d;
        int i[2];
    } u;
    u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], srclane);
    u.i[1] = __builtin_amdgcn_readlane(u.i[1], srclane);
    return u.d;
}
// WCH chunks of 128 columns, WSUB rows per pass: <2, 16> for rows of 129 .. 256 columns, <1, 32> for rows of at most 128 (most
// small tiles: bar17K's 512 tiles of that kind average 24 KB) -- the same registers hold twice the rows, so a 64-row tile is
// a chain of two passes instead of four (the packs were the last finishers of the launch: monkey18K 34.4 us, its last ten
// workgroups packs of 48 .. 80-column tiles that started at 17 us and took 15; profiles/r05_backsolve_tiles.txt G)
template <int WCH, int WSUB>
__device__ __forceinline__ void backsolve_wave_tile_t(const int4 jb, const int *__restrict__ dofmap, const double *__restrict__ W,
                                                      int nmax, const RowTile *__restrict__ rt, const double *__restrict__ q,
                                                      double *__restrict__ ppart, int nbmax, const int *__restrict__ abortp,
                                                      int epoch)
{
    const BsTile g = bs_tile(jb, nmax, rt, W, dofmap, q, ppart, nbmax);
    const int lane = threadIdx.x & 63;
    double2 r[WCH], pacc[WCH];
    int cend[WCH];
#pragma unroll
    for (int m = 0; m < WCH; ++m) {
        cend[m] = bs_pair_end(g, bs_col<64>(g.cb, lane, m), &r[m]);
        pacc[m] = make_double2(0.0, 0.0);
    }
#pragma unroll 1
    for (int ib = g.i0; ib < g.ns; ib += WSUB) {
        int ab = 0;
        if (abortp) ab = __hip_atomic_load(abortp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (answer used behind the loads)
        double2 y[WSUB][WCH];
        BS_LOAD_ROWS(WSUB, WCH, 64, true, g.cb, lane);
        if (abortp && __builtin_amdgcn_readfirstlane(ab) == epoch) return;   // the result would not be used
        // eight rows at a time: their dot products, the wave sums, and at once their rank-8 update (rows ascending into every
        // accumulator, as in the block form) -- only eight row sums are alive
#pragma unroll
        for (int gr = 0; gr < WSUB / 8; ++gr) {
            double d[8];
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < WCH; ++m) acc += y[8 * gr + rr][m].x * r[m].x + y[8 * gr + rr][m].y * r[m].y;
                d[rr] = acc;
            }
            const double e1 = wave_sum8_transposed(d, lane);   // lane 8 k holds the wave sum of row k of the group
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const double t = bs_readlane(e1, 8 * rr);
#pragma unroll
                for (int m = 0; m < WCH; ++m) {
                    pacc[m].x += t * y[8 * gr + rr][m].x;
                    pacc[m].y += t * y[8 * gr + rr][m].y;
                }
            }
        }
    }
    bs_store<WCH, 64>(g, g.cb, lane, pacc);
}

// job jobIdx >= nBig of the 256-thread launch is a pack of four small tiles: the calling wavefront's
__device__ __forceinline__ int4 bs_pack_job(const int4 *__restrict__ job, int nBig, int jobIdx) { return job[nBig + 4 * (jobIdx - nBig) + (threadIdx.x >> 6)]; }
// that tile in the pack family's form
__device__ __forceinline__ void backsolve_pack(int jobIdx, const int4 jb, const int *__restrict__ dofmap,
                                               const double *__restrict__ W, int nmax, const RowTile *__restrict__ rt,
                                               const double *__restrict__ q, double *__restrict__ ppart, int nbmax,
                                               const int *__restrict__ abortp, int epoch)
{
    const int rows = jb.z >> 16;
    if (rows == 0) return;              // padding of the last pack
    if (abortp && __builtin_amdgcn_readfirstlane(__hip_atomic_load(abortp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == epoch)
        return;
    bs_prof_begin(jobIdx, jb, true);
    // (wave-uniform: a tile is one wavefront's)
    bs_select_form<BSF_PACK>(jb.y + rows - jb.w, [&](auto I) __attribute__((always_inline)) {
        constexpr BsForm F = bs_form(BSF_PACK, I);
        backsolve_wave_tile_t<F.chunks, F.sub>(jb, dofmap, W, nmax, rt, q, ppart, nbmax, abortp, epoch);
    });
    bs_prof_end(jobIdx, true);
}

// the tile of job[jobIdx] by the calling workgroup: the form of the workgroup's family (256 threads: narrow, 512: wide) that holds
// its longest row
template <int THREADS>
__device__ __forceinline__ void backsolve_block(int jobIdx, const int4 *__restrict__ job, const int *__restrict__ dofmap,
                                                const double *__restrict__ W, int nmax, const RowTile *__restrict__ rt,
                                                const double *__restrict__ q, double *__restrict__ ppart, int nbmax,
                                                double (*sm)[THREADS / 64][32], const int *__restrict__ abortp, int epoch,
                                                int *s_abort, double2 *__restrict__ rs)
{
    constexpr int FAM = THREADS == BSF_LANES[BSF_NARROW] ? BSF_NARROW : BSF_WIDE;
    static_assert(THREADS == BSF_LANES[FAM], "a workgroup is one of the two block families");
    if (abortp) {   // workgroups that start after the verdict leave at once (one thread asks: a uniform answer)
        if (threadIdx.x == 0) s_abort[2] = __hip_atomic_load(abortp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (s_abort[2] == epoch) return;
    }
    const int4 jb = job[jobIdx];
    const int len = jb.y + (jb.z >> 16) - jb.w;   // longest row of the tile
    bs_prof_begin(jobIdx, jb, false);
    bs_select_form<FAM>(len, [&](auto I) __attribute__((always_inline)) {
        constexpr BsForm F = bs_form(FAM, I);
        backsolve_tile<THREADS, F.chunks, F.sub, F.rlds>(jb, dofmap, W, nmax, rt, q, ppart, nbmax, sm, abortp, epoch, s_abort, rs);
    });
    bs_prof_end(jobIdx, false);
}
// LDS slots of a workgroup family's RLDS forms: a right-hand side pair and an accumulator pair per lane and chunk of the longest such
// form, which is as many as it has columns (1: the family has none)
constexpr int bs_rlds_slots(int fam, int i = 0)
{
    return i == bs_form_count(fam) ? 1 : std::max(bs_form(fam, i).rlds ? bs_form_capacity(fam, i) : 1, bs_rlds_slots(fam, i + 1));
}

// spec: the launch is speculative (early back-solve, enqueue_loop_slot): it runs on the trial gradient before the
// controller has decided about the trial, so the retry phase does not gate it
template <int THREADS>
__global__ __launch_bounds__(THREADS, 2) void backsolve_kernel(const int4 *__restrict__ job, const int *__restrict__ dofmap,
                                                            const double *__restrict__ W, int nmax, const RowTile *__restrict__ rt,
                                                            const double *__restrict__ q, double *__restrict__ ppart, int nbmax,
                                                            const DevLoop *__restrict__ ctl, int spec, int nBig)
{
    __shared__ double sm[2][THREADS / 64][32];
    __shared__ int s_abort[3];
    __shared__ double2 rs[bs_rlds_slots(THREADS == 256 ? BSF_NARROW : BSF_WIDE)];   // (256 threads: rows beyond 2560 columns)
    if (ctl && (ctl->status != 0 || (ctl->phase != 0 && !spec))) return;
    // spec > 0: the slot's epoch (its 1-based index in the step); the controller, which runs meanwhile, publishes the epoch
    // of a slot whose trial it rejects or that ends the loop (DevLoop::abortEpoch)
    const int *abortp = (ctl && spec > 0 && spec < (1 << 30)) ? &ctl->abortEpoch : nullptr;
    if constexpr (THREADS == 256) {
        if ((int)blockIdx.x >= nBig)
            return backsolve_pack(blockIdx.x, bs_pack_job(job, nBig, blockIdx.x), dofmap, W, nmax, rt, q, ppart, nbmax, abortp, spec);
    }
    backsolve_block<THREADS>(blockIdx.x, job, dofmap, W, nmax, rt, q, ppart, nbmax, sm, abortp, spec, s_abort, rs);
}

// The same tiles with the loop controller as workgroup 0 of the launch: the controller's ~7 us (partial sums, the
// decision about the trial, the history update) run beside the ~45 us of streaming instead of in front of them.  The
// tiles read the loop state while workgroup 0 may be rewriting it: whichever value of `status` they see, the result is
// only used (merge_early, after the launch) if the final state says so.
template <int CTL>
__global__ __launch_bounds__(256, 2) void backsolve_ctl_kernel(const int4 *__restrict__ job, const int *__restrict__ dofmap,
                                                            const double *__restrict__ W, int nmax,
                                                            const RowTile *__restrict__ rt, const double *__restrict__ q,
                                                            double *__restrict__ ppart, int nbmax, CtlArgs ca,
                                                            int epoch, int nBig)
{
    __shared__ double sm[2][4][32];
    __shared__ int s_abort[3];
    __shared__ double2 rs[bs_rlds_slots(BSF_NARROW)];
    // (which workgroup hosts the controller makes no difference: index 0 / 256 / 520 / last measured 47.0-47.5 us)
    if (blockIdx.x == 0) {
        if constexpr (CTL == CTL_PAIR || CTL == CTL_PAIR_VP)
            loop_control_body<CTL>(ca.ctl, ca.partE, ca.nbE, ca.partR, ca.alpha_dev, ca.flags_host, ca.init & 1,
                                   (ca.init & 2) ? ca.partE + 2 * ELEM_NB_MAX : nullptr);
        else
            loop_control_body<CTL>(ca.ctl, ca.partE, ca.nbE, ca.partR, ca.alpha_dev, ca.flags_host, ca.init);
        return;
    }
    if (ca.ctl->status != 0) return;
    // (PAIR: a paired slot -- alpha_dev[1] > 0, written by the element pass of this slot -- waits as well: its gather worked on the
    // half step, which only counts if the controller finds the full step's energy too high)
    if (epoch < (1 << 30) && (ca.ctl->holdNext || ((CTL == CTL_PAIR || CTL == CTL_PAIR_VP) && (ca.init & 2) && ca.alpha_dev[1] > 0.0))) {
        // the trial is expected to be rejected (DevLoop::holdNext): wait for the controller's verdict instead of streaming
        // the factors beside it -- a rejection then costs the controller's ~7 us, not a stopped back-solve's ~20.  (A
        // workgroup that starts after the controller has stored its forecast for the NEXT slot reads that one: the verdict
        // is out by then, so it neither waits nor decides anything else than the abort test would.)
        if (threadIdx.x == 0) {
            const long long t0 = wall_clock64();
            int v;
            while (((v = __hip_atomic_load(&ca.ctl->holdVerdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 1) < epoch) {
                __builtin_amdgcn_s_sleep(16);
                if (wall_clock64() - t0 > 200000000ll) break;   // 2 s: go on speculatively (the result is only used if valid)
            }
            s_abort[2] = ((v >> 1) >= epoch && (v & 1)) ? 1 : 0;
        }
        __syncthreads();
        if (s_abort[2]) return;
        __syncthreads();
    }
    const int jobIdx = (int)blockIdx.x - 1;
    if (jobIdx >= nBig)
        return backsolve_pack(jobIdx, bs_pack_job(job, nBig, jobIdx), dofmap, W, nmax, rt, q, ppart, nbmax,
                              epoch < (1 << 30) ? &ca.ctl->abortEpoch : nullptr, epoch);
    backsolve_block<256>(jobIdx, job, dofmap, W, nmax, rt, q, ppart, nbmax, sm, epoch < (1 << 30) ? &ca.ctl->abortEpoch : nullptr, epoch,
                         s_abort, rs);
}

// psub_s[k] = sum over the row tiles b of the part whose column range holds k of ppart[s][b][k]
//   (fixed order b = 0, 1, ..., coalesced in k)
// Round 5: the tiles that can hold a column are LISTED per group of 16 columns (rp_ptr / rp_idx, ascending b; a tile's range
// starts on a multiple of 16, so a listed tile holds the first entry >> 24 columns of the group) instead of testing all
// nbmax tiles of the part for every column -- with three dissection levels a part has ~80 tiles of which ~17 hold a given
// column (1 M tets: 44.4 -> 17.7 us per launch, bunny5K 8 -> 6.6; profiles/r05_factor.txt E).  Same additions, same order.
__global__ __launch_bounds__(256) void reduce_partial_p_kernel(const int *__restrict__ rp_ptr, const int *__restrict__ rp_idx,
                                                               const double *__restrict__ ppart, int nmax,
                                                               int nbmax, double *__restrict__ psub,
                                                               const DevLoop *__restrict__ ctl, int s0)
{
    if (ctl && (ctl->status != 0 || ctl->phase != 0)) return;
    const int s = blockIdx.y + s0;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nmax) return;
    const double *base = ppart + (size_t)s * nbmax * nmax + k;
    const int ng = nmax >> 4;
    const int *pp = rp_ptr + (size_t)s * (ng + 1) + (k >> 4);
    const int e0 = pp[0], e1 = pp[1];
    // a listed tile that ends in front of column k reads a zero instead (select on the address, not a branch around the
    // load), so the loads of a batch are all in flight together
    double acc = 0.0;
    int e = e0;
    for (; e + 8 <= e1; e += 8) {
        int bb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) bb[u] = rp_idx[e + u];
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            // entry = tile | (columns of the group the tile holds, 1 .. 16) << 24
            const double *src = (k & 15) < (bb[u] >> 24) ? base + (size_t)(bb[u] & 0xffffff) * nmax : &g_zero_slot;
            v[u] = *src;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    {
        int bb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) bb[u] = (e + u < e1) ? rp_idx[e + u] : 0;
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double *src = (k & 15) < (bb[u] >> 24) ? base + (size_t)(bb[u] & 0xffffff) * nmax : &g_zero_slot;
            v[u] = *src;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (e + u < e1) acc += v[u];
    }
    psub[(size_t)s * nmax + k] = acc;
}

// ---- rows longer than one workgroup's register tile (subdomains beyond ~1300 vertices: `timeStepper DOT 6` on a
// 17k-vertex mesh gives n_s ~ 9800) -----------------------------------------------------------------------------
// A long tile (<= 64 rows of one tree region) is cut into column chunks of BSL_CW; the single pass becomes two:
//   phase 0  tdots[tile][chunk][row] = row[chunk] . r[chunk]                       (streams the tile once)
//   phase 1  t_row = sum over chunks (fixed order);  ppart[tile][chunk columns] = sum_rows t_row * row[chunk]
//                                                                                  (streams it a second time)
// so these rows cost 2x their bytes.  Only the separator rows of the upper tree levels of big subdomains are that
// long; everything else stays on the single-pass kernel above.
// (BSL_THREADS x BSL_CH pairs = BS_LONG_CHUNK columns per workgroup, BSL_SUB rows per pass: bs_forms.hpp, where the job table counts
// its work items in the same chunk)
template <int PHASE>
__global__ __launch_bounds__(BSL_THREADS) void backsolve_long_kernel(const int4 *__restrict__ ljob, const int2 *__restrict__ lwork,
                                                                     const int *__restrict__ dofmap, const double *__restrict__ W,
                                                                     int nmax, const RowTile *__restrict__ rt,
                                                                     const double *__restrict__ q, double *__restrict__ tdots,
                                                                     int maxChunks, double *__restrict__ ppart, int nbmax,
                                                                     const DevLoop *__restrict__ ctl, int spec)
{
    constexpr int NW = BSL_THREADS / 64;
    __shared__ double sm[2][NW][8];
    __shared__ double tsh[BS_ROWS];
    if (ctl && (ctl->status != 0 || (ctl->phase != 0 && !spec))) return;
    const int2 wk = lwork[blockIdx.x];          // (long-tile index, chunk)
    const BsTile g = bs_tile(ljob[wk.x], nmax, rt, W, dofmap, q, ppart, nbmax);
    const int c0 = g.cb + wk.y * BS_LONG_CHUNK;           // this workgroup's columns [c0, c0 + BS_LONG_CHUNK) ∩ [cb, ncol)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int cend[BSL_CH];
    double2 r[BSL_CH], pacc[BSL_CH];
#pragma unroll
    for (int m = 0; m < BSL_CH; ++m) {
        cend[m] = bs_pair_end<false>(g, bs_col<BSL_THREADS>(c0, tid, m), PHASE == 0 ? &r[m] : nullptr);
        pacc[m] = make_double2(0.0, 0.0);
    }
    if (PHASE == 1) {
        // t_row: the chunk partials of phase 0 in chunk order
        const int nch = (g.ncol - g.cb + BS_LONG_CHUNK - 1) / BS_LONG_CHUNK;
        if (tid < BS_ROWS) {
            double t = 0.0;
            for (int c = 0; c < nch; ++c) t += tdots[((size_t)wk.x * maxChunks + c) * BS_ROWS + tid];
            tsh[tid] = t;
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int sb = 0; sb < BS_ROWS / 8; ++sb) {
        const int ib = g.i0 + sb * 8;
        if (ib >= g.ns) break;
        double2 y[8][BSL_CH];
        BS_LOAD_ROWS(8, BSL_CH, BSL_THREADS, false, c0, tid);
        if (PHASE == 0) {
            const int buf = sb & 1;
            double d[8];
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                double acc = 0.0;
#pragma unroll
                for (int m = 0; m < BSL_CH; ++m) acc += y[rr][m].x * r[m].x + y[rr][m].y * r[m].y;
                d[rr] = wave_sum(acc);
            }
            if (lane == 0) {
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) sm[buf][wv][rr] = d[rr];
            }
            __syncthreads();
            if (tid < 8) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) t += sm[buf][w][tid];
                tdots[((size_t)wk.x * maxChunks + wk.y) * BS_ROWS + 8 * sb + tid] = t;
            }
        } else {
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) {
                const double t = tsh[8 * sb + rr];   // rows past the tile's end were loaded as zeros
#pragma unroll
                for (int m = 0; m < BSL_CH; ++m) {
                    pacc[m].x += t * y[rr][m].x;
                    pacc[m].y += t * y[rr][m].y;
                }
            }
        }
    }
    if (PHASE == 1) bs_store<BSL_CH, BSL_THREADS>(g, c0, tid, pacc);
}

// ---- two-level form (DevTwoLevel, dotmi_internal.hpp): the three kernels around the tile kernels -------------------------------
// Reference role: the forward and backward substitution of CHOLMODSolver::solve (CHOLMODSolver.cpp:149-163) across the boundary
// between a subdomain's leaves and its separators; here with the leaves' inverse factors multiplied in (M_GD = L_GD X_DD).
// c[k] = M[row k, leaf columns] . r_leaf : a WAVEFRONT = eight consecutive rows of a panel (item = (panel, first row): no LDS, no
// barrier, the waves of a workgroup are independent -- a workgroup per panel was a chain of ~4 us steps per wave behind a ~3 us
// start, four rounds of them per CU: 181 us for 662 MB at 1 M tets), two columns per lane (a panel starts on an even column and
// has an even number of them: dotmi_create), the packed rows of a panel one behind the other
__global__ __launch_bounds__(256) void twolevel_forward_kernel(int nItems, const int2 *__restrict__ item, const int4 *__restrict__ panel,
                                                               const long long *__restrict__ rowBase, const double *__restrict__ Mp,
                                                               const double *__restrict__ rpad, double *__restrict__ cbuf,
                                                               const DevLoop *__restrict__ ctl)
{
    if (ctl && ctl->status != 0) return;
    const int lane = threadIdx.x & 63, it = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (it >= nItems) return;
    const int2 im = item[it];
    const int4 pn = panel[im.x];
    constexpr int RW = 8;
    const int k0 = im.y, n2 = pn.w >> 1, nr = min(RW, pn.y - k0);
    const double2 *row0 = reinterpret_cast<const double2 *>(Mp + rowBase[pn.x + k0]);
    const double2 *r2 = reinterpret_cast<const double2 *>(rpad + pn.z);
    double acc[RW];
#pragma unroll
    for (int u = 0; u < RW; ++u) acc[u] = 0.0;
    for (int c = lane; c < n2; c += 64) {
        const double2 rc = r2[c];
        double2 w[RW];
#pragma unroll
        for (int u = 0; u < RW; ++u) w[u] = row0[(size_t)min(u, nr - 1) * n2 + c];
#pragma unroll
        for (int u = 0; u < RW; ++u) {
            acc[u] += w[u].x * rc.x;
            acc[u] += w[u].y * rc.y;
        }
    }
#pragma unroll
    for (int u = 0; u < RW; ++u) {
        const double t = wave_sum(acc[u]);
        if (lane == 0 && u < nr) cbuf[pn.x + k0 + u] = t;
    }
}
// the panels' rows from where the factorisation leaves them (rows of the separators' leaf ranges, a leaf range apart) into one
// packed array, panel after panel, row after row: once per factorisation; workgroup = panel
__global__ __launch_bounds__(256) void twolevel_pack_kernel(const int4 *__restrict__ panel, const long long *__restrict__ rowSrc,
                                                            const long long *__restrict__ rowDst, const double *__restrict__ W,
                                                            double *__restrict__ packed)
{
    const int4 pn = panel[blockIdx.x];
    const int n2 = pn.w >> 1, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = wv; k < pn.y; k += 4) {
        const double2 *src = reinterpret_cast<const double2 *>(W + rowSrc[pn.x + k]);
        double2 *dst = reinterpret_cast<double2 *>(packed + rowDst[pn.x + k]);
        for (int c = lane; c < n2; c += 64) dst[c] = src[c];
    }
}
void launch_twolevel_pack(const DevParts &P, hipStream_t st)
{
    if (P.tl.on && P.tl.nPanels > 0)
        hipLaunchKernelGGL(twolevel_pack_kernel, dim3(P.tl.nPanels), dim3(256), 0, st, P.tl.panel, P.tl.rowSrc, P.tl.rowBase,
                           (const double *)P.W, P.tl.packed);
}
// t = r - sum of the panel rows' c at the separator positions (list order), r itself everywhere else
__global__ __launch_bounds__(256) void twolevel_rhs_kernel(int total, const int *__restrict__ gPtr, const int *__restrict__ gIdx,
                                                           const double *__restrict__ rpad, const double *__restrict__ cbuf,
                                                           double *__restrict__ rpad2, const DevLoop *__restrict__ ctl)
{
    if (ctl && ctl->status != 0) return;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        double v = rpad[i];
        const int e1 = gPtr[i + 1];
        for (int e = gPtr[i]; e < e1; ++e) v -= cbuf[gIdx[e]];
        rpad2[i] = v;
    }
}
// p_leaf -= M[rows, leaf columns]^T p_G[rows] on the per-subdomain sums: workgroup = panel; thread = (column pair, row group):
// CW column pairs across, 256 / CW row groups that take the rows in turns of eight (ascending inside a group, four interleaved
// partial sums each); the groups' sums are added in group order
template <int CW>
__global__ __launch_bounds__(256) void twolevel_backward_kernel(const int4 *__restrict__ panel, const long long *__restrict__ rowBase,
                                                                const int *__restrict__ rowPos, const double *__restrict__ W,
                                                                double *__restrict__ psub, const DevLoop *__restrict__ ctl)
{
    extern __shared__ __attribute__((aligned(16))) double tl_lds[];
    if (ctl && (ctl->status != 0 || ctl->phase != 0)) return;   // (as reduce_partial_p_kernel, whose sums this finishes)
    constexpr int RG = 256 / CW, RB = 8;
    const int4 pn = panel[blockIdx.x];
    const int tid = threadIdx.x, cg = tid % CW, g = tid / CW;
    const int nr = (pn.y + RB - 1) / RB * RB;
    double *pg = tl_lds;
    double2 *part = reinterpret_cast<double2 *>(tl_lds + nr);   // [RG][CW]
    for (int k = tid; k < nr; k += 256) pg[k] = k < pn.y ? psub[rowPos[pn.x + k]] : 0.0;
    __syncthreads();
    const int n2 = pn.w >> 1;
    // (the packed rows of a panel lie one behind the other; the rows past the panel's end -- multiplied by zeros -- re-read its last)
    const double2 *rows = reinterpret_cast<const double2 *>(W + rowBase[pn.x]);
    const int last = pn.y - 1;
    for (int c0 = 0; c0 < n2; c0 += CW) {
        const int c = c0 + cg;
        double2 a[4] = {make_double2(0.0, 0.0), make_double2(0.0, 0.0), make_double2(0.0, 0.0), make_double2(0.0, 0.0)};
        if (c < n2)
            for (int k = RB * g; k < nr; k += RB * RG) {
                double2 w[RB];
#pragma unroll
                for (int u = 0; u < RB; ++u) w[u] = rows[(size_t)min(k + u, last) * n2 + c];
#pragma unroll
                for (int u = 0; u < RB; ++u) {
                    a[u & 3].x += w[u].x * pg[k + u];
                    a[u & 3].y += w[u].y * pg[k + u];
                }
            }
        part[g * CW + cg] = make_double2((a[0].x + a[1].x) + (a[2].x + a[3].x), (a[0].y + a[1].y) + (a[2].y + a[3].y));
        __syncthreads();
        if (g == 0 && c < n2) {
            double2 t = part[cg];
#pragma unroll
            for (int q = 1; q < RG; ++q) {
                t.x += part[q * CW + cg].x;
                t.y += part[q * CW + cg].y;
            }
            double2 *dst = reinterpret_cast<double2 *>(psub + pn.z) + c;
            double2 v = *dst;
            v.x -= t.x;
            v.y -= t.y;
            *dst = v;
        }
        __syncthreads();
    }
}

// A launch with the dispatch's own begin / end time stamps in e0 / e1 (either may be null) when `timed`, a plain launch otherwise.
// Optional events time the streaming kernel alone (the roofline entry of bench.py is about that kernel): they are attached to the
// dispatch itself (hipExtLaunchKernelGGL: the packet's own time stamps, what rocprofv3 reports as the kernel's duration) -- two
// hipEventRecord calls around the launch add ~5 us of barrier packets
// (common_type: the arguments take the kernel's parameter types, not types deduced a second time)
template <class... A>
static void launch_bs(bool timed, hipEvent_t e0, hipEvent_t e1, void (*kernel)(A...), dim3 grid, dim3 block, hipStream_t st,
                      std::common_type_t<A>... args)
{
    if (timed) hipExtLaunchKernelGGL(kernel, grid, block, 0, st, e0, e1, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, st, args...);
}
// rows beyond the register tile: the two-phase kernel on (tile, column chunk) work items
static void launch_long(const DevParts &P, const int4 *ltile, const int2 *lwork, int nlwork, const double *rhs, const DevLoop *ctl,
                        int spec, hipStream_t st)
{
    hipLaunchKernelGGL((backsolve_long_kernel<0>), dim3(nlwork), dim3(BSL_THREADS), 0, st, ltile, lwork, P.dofmap, P.W, P.nmax, P.rt,
                       rhs, P.tdots, P.maxChunks, P.ppart, P.nbmax, ctl, spec);
    hipLaunchKernelGGL((backsolve_long_kernel<1>), dim3(nlwork), dim3(BSL_THREADS), 0, st, ltile, lwork, P.dofmap, P.W, P.nmax, P.rt,
                       rhs, P.tdots, P.maxChunks, P.ppart, P.nbmax, ctl, spec);
}

template <int CTL>
static void launch_gemv_impl(const DevParts &P, const double *q, hipStream_t st, const DevLoop *ctl, hipEvent_t ev0, hipEvent_t ev1,
                             const CtlArgs *ca, int spec)
{
    if (P.ntiles == 0 && P.nquad == 0 && P.nltiles == 0) return;
    if (q) {   // right-hand sides not in padded order yet
        const int total = P.nParts * P.nmax;
        int nb = (total + 255) / 256;
        if (nb > 2048) nb = 2048;
        hipLaunchKernelGGL(gather_pad_kernel, dim3(nb), dim3(256), 0, st, total, P.dofmap, q, P.rpad);
    }
    const double *rhs = P.rpad;
    hipEvent_t evLast = nullptr;   // two-level form: the timed region runs from the forward kernel to the backward kernel
    if (P.tl.on) {   // two-level form: t_G = r_G - M_GD r_D in front of the tile kernels
        if (P.tl.nPanels > 0) {
            launch_bs(ev0 && ev1, ev0, nullptr, twolevel_forward_kernel, dim3((P.tl.nItems + 3) / 4), dim3(256), st, P.tl.nItems,
                      P.tl.item, P.tl.panel, P.tl.rowBase, P.tl.packed, P.rpad, P.tl.cbuf, ctl);
            if (ev0 && ev1) {
                evLast = ev1;
                ev0 = ev1 = nullptr;
            }
        }
        const int total = P.nParts * P.nmax;
        hipLaunchKernelGGL(twolevel_rhs_kernel, dim3(std::min((total + 255) / 256, 4096)), dim3(256), 0, st, total, P.tl.gPtr, P.tl.gIdx,
                           (const double *)P.rpad, (const double *)P.tl.cbuf, P.tl.rpad2, ctl);
        rhs = P.tl.rpad2;
    }
    // wide tiles (rows of 3073..5120 columns) on the 512-thread kernel, the rest on the 256-thread one (two workgroups per
    // CU instead of one); the events (if any) span both launches: start of the first, stop of the last
    // P.tile = [wide tiles | narrow tiles of more than 256 columns | packs of four small tiles]: job k < nN of the narrow launch
    // is one tile, job nN + k the four tiles P.tile[ntiles + 4 k ..] (one wavefront each, backsolve_wave_tile)
    const int nW = P.ntilesWide, nN = P.ntiles - P.ntilesWide, nG = nN + P.nquad;
    const bool timed = (ev0 && ev1) || evLast;
    if (ca && spec <= 0) spec = 1;   // (callers pass the slot's epoch: > 0)
    if (ca && nG == 0)   // no launch of the 256-thread kernel to host it: the controller on its own, in front
        launch_loop_control(ca->ctl, ca->partE, ca->nbE, ca->partR, ca->alpha_dev, ca->flags_host, st, ca->init & 1);
    if (nW > 0)
        launch_bs(timed, ev0, nG > 0 ? nullptr : ev1, backsolve_kernel<512>, dim3(nW), dim3(512), st, P.tile, P.dofmap, P.W, P.nmax,
                  P.rt, rhs, P.ppart, P.nbmax, ctl, spec, nW);
    if (nG > 0 && ca)   // one workgroup more: the controller (backsolve_ctl_kernel)
        launch_bs(timed, nW > 0 ? nullptr : ev0, ev1, backsolve_ctl_kernel<CTL>, dim3(nG + 1), dim3(256), st, P.tile + nW, P.dofmap,
                  P.W, P.nmax, P.rt, rhs, P.ppart, P.nbmax, *ca, spec, nN);
    else if (nG > 0)
        launch_bs(timed, nW > 0 ? nullptr : ev0, ev1, backsolve_kernel<256>, dim3(nG), dim3(256), st, P.tile + nW, P.dofmap, P.W,
                  P.nmax, P.rt, rhs, P.ppart, P.nbmax, ctl, spec, nN);
    if (P.nltiles > 0) launch_long(P, P.ltile, P.lwork, P.nlwork, rhs, ctl, spec, st);
    if (!P.mt_ptr) launch_reduce_partial(P, st, ctl);   // (merge_tiles_kernel sums the tile partials itself)
    if (P.tl.on && P.tl.nPanels > 0)   // p_D = q_D - M_GD^T p_G on the sums just formed
    {
        const size_t shm = 8 * (size_t)((P.tl.maxRows + 7) & ~7) + 16 * 256;   // (dotmi_create refuses panels beyond 7000 rows)
        const int cw = twolevel_backward_cw(P.tl.maxCols);   // (loop_forms.hpp: dotmi_loop_forms reports the same choice)
        const auto backward = cw == 32 ? twolevel_backward_kernel<32> : cw == 64 ? twolevel_backward_kernel<64> : twolevel_backward_kernel<128>;
        hipExtLaunchKernelGGL(backward, dim3(P.tl.nPanels), dim3(256), shm, st, (hipEvent_t) nullptr, evLast, 0, P.tl.panel, P.tl.rowBase,
                              P.tl.rowPos, (const double *)P.tl.packed, P.psub, ctl);
    }
}
// one instantiation per form of the controller (without a controller the form plays no part)
void launch_gemv(const DevParts &P, const double *q, hipStream_t st, const DevLoop *ctl, hipEvent_t ev0, hipEvent_t ev1,
                 const CtlLaunch *cl, int spec)
{
    const CtlArgs *ca = cl ? &cl->a : nullptr;
    switch (cl ? cl->form : CTL_PLAIN) {
    case CTL_PAIR: return launch_gemv_impl<CTL_PAIR>(P, q, st, ctl, ev0, ev1, ca, spec);
    case CTL_SPEC: return launch_gemv_impl<CTL_SPEC>(P, q, st, ctl, ev0, ev1, ca, spec);
    case CTL_VP: return launch_gemv_impl<CTL_VP>(P, q, st, ctl, ev0, ev1, ca, spec);
    case CTL_PAIR_VP: return launch_gemv_impl<CTL_PAIR_VP>(P, q, st, ctl, ev0, ev1, ca, spec);
    default: return launch_gemv_impl<CTL_PLAIN>(P, q, st, ctl, ev0, ev1, ca, spec);
    }
}
// the tile partials of every owned subdomain summed in the subdomains' own order (coalesced) -> psub
void launch_reduce_partial(const DevParts &P, hipStream_t st, const DevLoop *ctl)
{
    if (P.nParts > 0)
        hipLaunchKernelGGL(reduce_partial_p_kernel, dim3((P.nmax + 255) / 256, P.nParts), dim3(256), 0, st, P.rp_ptr, P.rp_idx,
                           P.ppart, P.nmax, P.nbmax, P.psub, ctl, 0);
}

// p[dofmap_s[k]] = psub_s[k] on the live positions of part s (p was cleared by the caller)
__global__ __launch_bounds__(256) void fill_part_kernel(const int *__restrict__ dofmap, const double *__restrict__ psub,
                                                        int nmax, int s, double *__restrict__ p)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nmax) return;
    const int d = dofmap[(size_t)s * nmax + k];
    if (d >= 0) p[d] = psub[(size_t)s * nmax + k];
}

void launch_gemv_part(const DevParts &P, int ls, const int4 *job, int njobs, const int2 *lwork, int nlwork, const double *q,
                      int n, double *p, hipStream_t st)
{
    hipMemsetAsync(p, 0, sizeof(double) * n, st);
    if (njobs <= 0 && nlwork <= 0) return;
    hipLaunchKernelGGL(gather_pad_kernel, dim3((P.nmax + 255) / 256), dim3(256), 0, st, P.nmax, P.dofmap + (size_t)ls * P.nmax,
                       q, P.rpad + (size_t)ls * P.nmax);
    if (njobs > 0) {   // all tiles in one launch: the 256-thread kernel if one of its forms holds the longest row, else the 512-thread one
        const bool narrow = bs_form_index(BSF_NARROW, P.maxTileLen) < bs_form_count(BSF_NARROW);
        launch_bs(false, nullptr, nullptr, narrow ? backsolve_kernel<256> : backsolve_kernel<512>, dim3(njobs),
                  dim3(BSF_LANES[narrow ? BSF_NARROW : BSF_WIDE]), st, job, P.dofmap, P.W, P.nmax, P.rt, P.rpad, P.ppart, P.nbmax, nullptr, 0, njobs);
    }
    if (nlwork > 0) launch_long(P, P.ltileByPart, lwork, nlwork, P.rpad, nullptr, 0, st);
    hipLaunchKernelGGL(reduce_partial_p_kernel, dim3((P.nmax + 255) / 256, 1), dim3(256), 0, st, P.rp_ptr, P.rp_idx, P.ppart,
                       P.nmax, P.nbmax, P.psub, (const DevLoop *)nullptr, ls);
    hipLaunchKernelGGL(fill_part_kernel, dim3((P.nmax + 255) / 256), dim3(256), 0, st, P.dofmap, P.psub, P.nmax, ls, p);
}

}  // namespace dotmi
