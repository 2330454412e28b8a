// k_coarse.hip -- the rigid-mode coarse space of Newton-PCG's preconditioner (dotmi_set_pcg_coarse; host side dotmi_coarse.hip, lists
// coarse_plan.hpp):  M = M_sym + Z A0^-1 Z^T,  A0 = Z^T H Z.  Subdomain s has six columns of Z, three
// translations and three rotations about its weighted centroid c_s; on a vertex v of s they are the 3 x 6 block
//     Z_sv = w_v [ I | -[x_v - c_s]x ],   w_v = 1 / dup_v on free vertices, 0 on fixed ones,
// with x and c frozen at the build (DevCoarse::xf, cen), so A0 and every application use the same Z.
//   once per refresh:   coarse_centroid_kernel, coarse_assemble_kernel (one workgroup per coupled pair of subdomains, the 36 sums of
//                       sum Z_si^T H_ij Z_tj over the pair's H blocks), coarse_fill_kernel (the dense matrix, identity on the padding
//                       and on dropped subdomains); X = chol(A0)^-1 then comes from the tile kernels of k_tilefactor.hip
//   per CG iteration:   coarse_restrict_kernel (c = Z^T r, one workgroup per subdomain), coarse_solve_kernel (y = X^T (X c), one
//                       workgroup per 64 rows of X), coarse_prolong_kernel (zsum += (Z y) / isd, a gather per vertex over its
//                       subdomains ascending)
//   DOT's own loop (dotmi_set_dot_coarse): the same Z, A0 and coarse_solve_kernel in M' = M + Z A0^-1 Z^T; the restriction reads the
//                       subdomains' padded right-hand sides through a table per padded position (coarse_rtab_kernel at the build,
//                       coarse_restrict_pad_kernel per application), the prolongation is inside the merge kernels (k_loopvec.hip, COARSE)
//   sharded handles (DOTMI_FLAG_DOT_COARSE): the table and the restriction over the rank's own subdomains, c in the tail of the vector
//                       the iteration all-reduces (zeros for the others' subdomains), the solve on every rank behind that collective,
//                       the prolongation in zfinish_kernel<DEV, true> / the zsum branch of merge_tiles_early_kernel<NT, true>; with a
//                       sharded Hessian coarse_assemble_kernel sums the pairs whose first subdomain the rank owns, zeros elsewhere
//   the balanced form (dotmi_set_dot_coarse_mode, mode 2): W = H Z as a table of 3 x 6 blocks (coarse_hz_kernel at the build), the deflation
//                       r - W y1 and the restriction c1 - W^T u around the unchanged block solve (coarse_deflate_kernel,
//                       coarse_restrict_hz_kernel; further down, with the sequence)
// Every sum has a fixed shape -- a thread's entries in list order, the lanes by wave_sum's tree, the four waves pairwise -- and
// nothing is added atomically: two builds and two applications are bit-identical.  The reference has no counterpart.
#include "k_device.hpp"

namespace dotmi {

// the sums of N accumulators over a workgroup of 256 threads: sm[4 N + j] holds total j afterwards (sm: 5 N doubles)
template <int N>
__device__ __forceinline__ void coarse_block_sum(const double (&acc)[N], double *sm)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double s = wave_sum(acc[j]);
        if (lane == 0) sm[w * N + j] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int t = threadIdx.x;
        sm[4 * N + t] = (sm[t] + sm[N + t]) + (sm[2 * N + t] + sm[3 * N + t]);
    }
    __syncthreads();
}

// c_s = sum_v w_v x_v / sum_v w_v over the vertices of s (0 for a dropped subdomain)
__global__ __launch_bounds__(256) void coarse_centroid_kernel(const int *__restrict__ svPtr, const int *__restrict__ svIdx,
                                                              const double *__restrict__ wgt, const double *__restrict__ x,
                                                              const int *__restrict__ live, double *__restrict__ cen)
{
    __shared__ double sm[5 * 4];
    const int s = blockIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = svPtr[s] + threadIdx.x; k < svPtr[s + 1]; k += 256) {
        const int v = svIdx[k];
        const double w = wgt[v];
        acc[0] += w * x[3 * v];
        acc[1] += w * x[3 * v + 1];
        acc[2] += w * x[3 * v + 2];
        acc[3] += w;
    }
    coarse_block_sum<4>(acc, sm);
    if (threadIdx.x < 3) cen[3 * s + threadIdx.x] = live[s] ? sm[16 + threadIdx.x] / sm[16 + 3] : 0.0;
}

// A0_st = sum over the pair's H blocks (i, j), i in s, j in t, of Z_si^T H_ij Z_tj = w_i w_j [ H, H B ; A H, A H B ] with
// B = -[x_j - c_t]x (column a: e_a x b) and A = [x_i - c_s]x (row a: (e_a x a)^T); 36 doubles per pair, row-major
__global__ __launch_bounds__(256) void coarse_assemble_kernel(const int2 *__restrict__ pair, const int *__restrict__ pairPtr,
                                                              const int *__restrict__ pairBlk, const int *__restrict__ blk_row,
                                                              const int *__restrict__ adj_idx, const double *__restrict__ Hval,
                                                              const double *__restrict__ wgt, const double *__restrict__ x,
                                                              const double *__restrict__ cen, const int *__restrict__ live,
                                                              int own0, int own1, double *__restrict__ pairA)
{
    __shared__ double sm[5 * 36];
    const int p = blockIdx.x;
    const int2 st = pair[p];
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.0;
    // [own0, own1): the subdomains whose pairs (s, t), s <= t, this rank assembles -- all of them unless the Hessian refresh is sharded
    // (DevCoarse::as0); the other pairs' blocks are written as zeros and come with the all-reduce of pairA, H is not read for them
    if (st.x >= own0 && st.x < own1 && live[st.x] && live[st.y]) {   // (uniform over the workgroup)
        const double cs0 = cen[3 * st.x], cs1 = cen[3 * st.x + 1], cs2 = cen[3 * st.x + 2];
        const double ct0 = cen[3 * st.y], ct1 = cen[3 * st.y + 1], ct2 = cen[3 * st.y + 2];
        for (int e = pairPtr[p] + threadIdx.x; e < pairPtr[p + 1]; e += 256) {
            const int blk = pairBlk[e];
            const int i = blk_row[blk], j = adj_idx[blk];
            const double ww = wgt[i] * wgt[j];
            if (ww == 0.0) continue;   // a fixed end: a zero row or column of Z
            double h[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) h[k] = Hval[hval_idx(blk, k)];
            const double a0 = x[3 * i] - cs0, a1 = x[3 * i + 1] - cs1, a2 = x[3 * i + 2] - cs2;
            const double b0 = x[3 * j] - ct0, b1 = x[3 * j + 1] - ct1, b2 = x[3 * j + 2] - ct2;
            double top[3][6];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                top[r][0] = h[3 * r];
                top[r][1] = h[3 * r + 1];
                top[r][2] = h[3 * r + 2];
                top[r][3] = h[3 * r + 2] * b1 - h[3 * r + 1] * b2;
                top[r][4] = h[3 * r] * b2 - h[3 * r + 2] * b0;
                top[r][5] = h[3 * r + 1] * b0 - h[3 * r] * b1;
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                acc[c] += ww * top[0][c];
                acc[6 + c] += ww * top[1][c];
                acc[12 + c] += ww * top[2][c];
                acc[18 + c] += ww * (a1 * top[2][c] - a2 * top[1][c]);
                acc[24 + c] += ww * (a2 * top[0][c] - a0 * top[2][c]);
                acc[30 + c] += ww * (a0 * top[1][c] - a1 * top[0][c]);
            }
        }
    }
    coarse_block_sum<36>(acc, sm);
    if (threadIdx.x < 36) pairA[(size_t)36 * p + threadIdx.x] = sm[4 * 36 + threadIdx.x];
}

// entry (I, J) of the dense matrix as the factorisation and dotmi_pcg_coarse_matrix see it: the pair's block (transposed below the
// diagonal, a diagonal block from its upper half), the identity on the padding and on a dropped subdomain's block, else zero
__host__ __device__ inline double coarse_entry(int I, int J, int nc, int nParts, const int *pairAt, const int *live, const double *pairA)
{
    if (I >= nc || J >= nc) return I == J ? 1.0 : 0.0;
    int s = I / 6, a = I % 6, t = J / 6, b = J % 6;
    if (!live[s] || !live[t]) return I == J ? 1.0 : 0.0;
    if (s > t || (s == t && a > b)) {
        int k = s;
        s = t;
        t = k;
        k = a;
        a = b;
        b = k;
    }
    const int p = pairAt[(size_t)s * nParts + t];
    return p >= 0 ? pairA[(size_t)36 * p + 6 * a + b] : 0.0;
}

__global__ __launch_bounds__(256) void coarse_fill_kernel(int nc, int ncp, int nParts, const int *__restrict__ pairAt,
                                                          const int *__restrict__ live, const double *__restrict__ pairA,
                                                          double *__restrict__ W2)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= ncp * ncp) return;
    W2[idx] = coarse_entry(idx / ncp, idx % ncp, nc, nParts, pairAt, live, pairA);
}

// c_s = Z_s^T r: the three sums of w_v r_v and of w_v (x_v - c_s) x r_v over the vertices of s
__device__ __forceinline__ void coarse_restrict_body(const int *__restrict__ svPtr, const int *__restrict__ svIdx,
                                                     const double *__restrict__ wgt, const double *__restrict__ x,
                                                     const double *__restrict__ cen, const int *__restrict__ live,
                                                     const double *__restrict__ r, double *__restrict__ c, double *sm)
{
    const int s = blockIdx.x;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live[s]) {
        const double c0 = cen[3 * s], c1 = cen[3 * s + 1], c2 = cen[3 * s + 2];
        for (int k = svPtr[s] + threadIdx.x; k < svPtr[s + 1]; k += 256) {
            const int v = svIdx[k];
            const double w = wgt[v];
            if (w == 0.0) continue;
            const double r0 = r[3 * v], r1 = r[3 * v + 1], r2 = r[3 * v + 2];
            const double d0 = x[3 * v] - c0, d1 = x[3 * v + 1] - c1, d2 = x[3 * v + 2] - c2;
            acc[0] += w * r0;
            acc[1] += w * r1;
            acc[2] += w * r2;
            acc[3] += w * (d1 * r2 - d2 * r1);
            acc[4] += w * (d2 * r0 - d0 * r2);
            acc[5] += w * (d0 * r1 - d1 * r0);
        }
    }
    coarse_block_sum<6>(acc, sm);
    if (threadIdx.x < 6) c[6 * s + threadIdx.x] = sm[4 * 6 + threadIdx.x];
}
__global__ __launch_bounds__(256) void coarse_restrict_kernel(const int *__restrict__ svPtr, const int *__restrict__ svIdx,
                                                              const double *__restrict__ wgt, const double *__restrict__ x,
                                                              const double *__restrict__ cen, const int *__restrict__ live,
                                                              const double *__restrict__ r, double *__restrict__ c)
{
    __shared__ double sm[5 * 6];
    coarse_restrict_body(svPtr, svIdx, wgt, x, cen, live, r, c, sm);
}
// the same restriction as a kernel of the device-resident loop (dotmi_set_dot_coarse_mode, mode 2, the q-based order): gated like
// coarse_solve_loop_kernel with spec == 0 -- past the end of the loop and in a line-search retry it returns at once
__global__ __launch_bounds__(256) void coarse_restrict_loop_kernel(const int *__restrict__ svPtr, const int *__restrict__ svIdx,
                                                                   const double *__restrict__ wgt, const double *__restrict__ x,
                                                                   const double *__restrict__ cen, const int *__restrict__ live,
                                                                   const double *__restrict__ r, double *__restrict__ c,
                                                                   const DevLoop *__restrict__ ctl)
{
    __shared__ double sm[5 * 6];
    if (ctl->status != 0 || ctl->phase != 0) return;
    coarse_restrict_body(svPtr, svIdx, wgt, x, cen, live, r, c, sm);
}

// y = X^T (X c) = sum_r X[r, :]^T (X[r, :] . c) on the nc live rows of the lower-triangular X (leading dimension ld): workgroup g
// owns the 64 rows of row block g, forms their t_r = X[r, :] . c (a wave per 16 rows, their loads side by side, the lanes over the
// columns) and then its part of y, sum over its rows of t_r X[r, k], for the columns k < 64 (g + 1) the block reaches (a thread per
// column, down the 64 rows).  The parts go to ypart[g][k]; their consumer, the prolongation, adds them in ascending g -- the
// convention of every reduction here.  (A first form did both phases in ONE workgroup: 34 us at nc = 192, 81 us at nc = 384,
// more than the block solve itself -- profiles/newton_pcg_coarse.txt.)  The strictly upper part of a diagonal tile holds zeros
// (tile_task_body stores them), the padding rows are the identity on zeros of c.
__device__ __forceinline__ void coarse_solve_body(int nc, int ld, const double *__restrict__ X, const double *__restrict__ c,
                                                  double *__restrict__ ypart, double *sc, double *tv)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x, r0 = 64 * g, ncol = min(64 * (g + 1), nc);
    for (int k = tid; k < ncol; k += 256) sc[k] = c[k];
    __syncthreads();
    double acc[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = 0.0;
    const double *base = X + (size_t)(r0 + 16 * wave) * ld;
    for (int k = lane; k < ncol; k += 64) {
        const double ck = sc[k];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc[u] += base[(size_t)u * ld + k] * ck;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const double t = wave_sum(acc[u]);
        if (lane == 0) tv[16 * wave + u] = r0 + 16 * wave + u < nc ? t : 0.0;
    }
    __syncthreads();
    for (int k = tid; k < ncol; k += 256) {
        const double *col = X + (size_t)r0 * ld + k;
        double a = 0.0;
#pragma unroll 8
        for (int r = 0; r < 64; ++r) a += col[(size_t)r * ld] * tv[r];
        ypart[(size_t)g * ld + k] = a;
    }
}
__global__ __launch_bounds__(256) void coarse_solve_kernel(int nc, int ld, const double *__restrict__ X, const double *__restrict__ c,
                                                           double *__restrict__ ypart)
{
    __shared__ double sc[COARSE_NC_MAX], tv[64];
    coarse_solve_body(nc, ld, X, c, ypart, sc, tv);
}
// the same solve as a kernel of the device-resident loop (dotmi_set_dot_coarse): gated like the back-solve it stands in front of --
// past the end of the loop it returns at once, and in the q-based order (spec == 0) in a line-search retry too; in the early order a
// retry slot solves for its trial's gradient like the back-solve does
__global__ __launch_bounds__(256) void coarse_solve_loop_kernel(int nc, int ld, const double *__restrict__ X, const double *__restrict__ c,
                                                                double *__restrict__ ypart, const DevLoop *__restrict__ ctl, int spec)
{
    __shared__ double sc[COARSE_NC_MAX], tv[64];
    if (ctl->status != 0 || (ctl->phase != 0 && !spec)) return;
    coarse_solve_body(nc, ld, X, c, ypart, sc, tv);
}

// The restriction of DOT's loop reads the right-hand sides where the back-solve reads them: DevParts::rpad, subdomain s in the padded
// positions [s nmax, (s + 1) nmax), every vertex of s in three consecutive ones (block_plan.hpp: place_rows).  Per padded position the
// table holds what its scalar r_a (component a of vertex v) contributes to c_s = Z_s^T r:  w_v r_a to translation a and
// w_v ((x_v - c_s) x r)_b = w_v (k_b r_a) to the rotations, k = (0, d2, -d1), (-d2, 0, d0), (d1, -d0, 0) for a = 0, 1, 2 and
// d = x_v - c_s.  An entry is (w_v, k_0, k_1, k_2); all zero on the padding, on fixed vertices and in a dropped subdomain.  Written
// once per build, behind the centroids.  A sharded handle (DOTMI_FLAG_DOT_COARSE) holds the padded ranges of its own subdomains
// [p0, p0 + nOwn) only: the table has their local index, subdomain p0 + ls in [ls nmax, (ls + 1) nmax)
__global__ __launch_bounds__(256) void coarse_rtab_kernel(int total, int nmax, int p0, const int *__restrict__ dofmap,
                                                          const double *__restrict__ wgt, const double *__restrict__ x,
                                                          const double *__restrict__ cen, const int *__restrict__ live,
                                                          double4 *__restrict__ rtab)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= total) return;
    const int dof = dofmap[k], s = p0 + k / nmax;   // (the table and dofmap are indexed by the rank's own subdomains, cen and live by all)
    double4 t = make_double4(0.0, 0.0, 0.0, 0.0);
    if (dof >= 0 && live[s]) {
        const int v = dof / 3, a = dof - 3 * v;
        const double w = wgt[v];
        if (w != 0.0) {
            const double d0 = x[3 * v] - cen[3 * s], d1 = x[3 * v + 1] - cen[3 * s + 1], d2 = x[3 * v + 2] - cen[3 * s + 2];
            t.x = w;
            t.y = a == 0 ? 0.0 : (a == 1 ? -d2 : d1);
            t.z = a == 0 ? d2 : (a == 1 ? 0.0 : -d0);
            t.w = a == 0 ? -d1 : (a == 1 ? d0 : 0.0);
        }
    }
    rtab[k] = t;
}

// c_s = Z_s^T r from the padded right-hand sides: one workgroup per subdomain over its own contiguous range, the table, the
// right-hand side and the position's component (dofmap) side by side.  DEV: a kernel of the device-resident loop, gated like
// coarse_solve_loop_kernel.  The grid covers every subdomain and c is indexed by the global one; a workgroup whose subdomain this rank
// does not own (outside [p0, p0 + nOwn)) writes its six zeros -- on a sharded handle c is the tail of the vector the iteration
// all-reduces, and the sum over the ranks of (own c_s, zeros elsewhere) is the whole Z^T r, exactly
template <bool DEV>
__global__ __launch_bounds__(256) void coarse_restrict_pad_kernel(int nmax, int p0, int nOwn, const int *__restrict__ dofmap,
                                                                  const double4 *__restrict__ rtab, const double *__restrict__ rpad,
                                                                  double *__restrict__ c, const DevLoop *__restrict__ ctl, int spec)
{
    __shared__ double sm[5 * 6];
    if constexpr (DEV) {
        if (ctl->status != 0 || (ctl->phase != 0 && !spec)) return;
    }
    const int s = blockIdx.x, ls = s - p0;
    if (ls < 0 || ls >= nOwn) {   // (uniform over the workgroup)
        if (threadIdx.x < 6) c[6 * s + threadIdx.x] = 0.0;
        return;
    }
    const size_t base = (size_t)ls * nmax;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < nmax; k += 256) {
        const double4 t = rtab[base + k];
        const double r = rpad[base + k];
        const int dof = dofmap[base + k];
        if (t.x == 0.0) continue;
        const int a = dof % 3;
        const double wr = t.x * r;
        acc[0] += a == 0 ? wr : 0.0;
        acc[1] += a == 1 ? wr : 0.0;
        acc[2] += a == 2 ? wr : 0.0;
        acc[3] += t.x * (t.y * r);
        acc[4] += t.x * (t.z * r);
        acc[5] += t.x * (t.w * r);
    }
    coarse_block_sum<6>(acc, sm);
    if (threadIdx.x < 6) c[6 * s + threadIdx.x] = sm[4 * 6 + threadIdx.x];
}

// zsum_v += (Z y)_v / isd_v with (Z y)_v = w_v sum over the subdomains s of v, ascending, of t_s + omega_s x (x_v - c_s): behind the
// merge, so that pcg_spmv_kernel's w = zsum (.) isd is M_sym r + Z y.  Prologue: y from the row blocks' parts (coarse_solve_kernel),
// every workgroup the same sums in the same order
__global__ __launch_bounds__(256) void coarse_prolong_kernel(int nV, int nc, int ld, const int *__restrict__ vsPtr,
                                                             const int *__restrict__ vsIdx, const double *__restrict__ wgt,
                                                             const double *__restrict__ x, const double *__restrict__ cen,
                                                             const double *__restrict__ ypart, const double *__restrict__ isd,
                                                             double *__restrict__ zsum)
{
    __shared__ double y[COARSE_NC_MAX];
    const int G = (nc + 63) / 64;
    for (int k = threadIdx.x; k < nc; k += 256) {
        double a = 0.0;
        for (int g = k >> 6; g < G; ++g) a += ypart[(size_t)g * ld + k];
        y[k] = a;
    }
    __syncthreads();
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nV) return;
    const double w = wgt[v];
    if (w == 0.0) return;
    const double x0 = x[3 * v], x1 = x[3 * v + 1], x2 = x[3 * v + 2];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = vsPtr[v]; k < vsPtr[v + 1]; ++k) {
        const int s = vsIdx[k];
        const double *ys = y + 6 * s;
        const double d0 = x0 - cen[3 * s], d1 = x1 - cen[3 * s + 1], d2 = x2 - cen[3 * s + 2];
        a0 += ys[0] + (ys[4] * d2 - ys[5] * d1);
        a1 += ys[1] + (ys[5] * d0 - ys[3] * d2);
        a2 += ys[2] + (ys[3] * d1 - ys[4] * d0);
    }
    const double sc = w / isd[v];
    zsum[3 * v] += sc * a0;
    zsum[3 * v + 1] += sc * a1;
    zsum[3 * v + 2] += sc * a2;
}

// ---- the balanced form (dotmi_set_dot_coarse_mode, mode 2):  M'' = C + (I - C H) M (I - H C),  C = Z A0^-1 Z^T ----------------------------
// W = H Z is kept as a table of 3 x 6 blocks, one per (vertex i, subdomain t) that an H block (i, j), j in t, couples (coarse_plan.hpp,
// CoarseHzPlan), so that neither correction multiplies by H:
//     y1 = A0^-1 Z^T r,   r1 = r - W y1,   u = M r1 (the unchanged block solve and merge),   M'' r = u + Z A0^-1 (Z^T r - W^T u).
// (The second coarse solve runs on the difference of the two restrictions: y1 - y2 = A0^-1 (c1 - c2) is then what the existing
// prolongation of the sharded merge, zfinish_kernel<DEV, true>, adds behind the division by the multiplicity and in front of the
// y_i . z sums -- those sums must see the corrected vector.)
//   once per build:     coarse_hz_kernel behind the centroids
//   per application:    coarse_restrict_kernel, coarse_solve_kernel, coarse_deflate_kernel | block solve, merge without the division |
//                       coarse_restrict_hz_kernel, coarse_solve_kernel, zfinish_kernel<DEV, true> (k_loopvec.hip)
// DEV: the twins of the device-resident loop, gated like coarse_solve_loop_kernel in the q-based order (spec == 0).

// W[i, t] = sum over the entry's H blocks (i, j), j in t, in list order of H_ij w_j [ I | -[x_j - c_t]x ]: 18 doubles per entry,
// row-major 3 x 6 (the rows of coarse_assemble_kernel's `top`).  Zero for a dropped subdomain; a fixed vertex's row of H is the
// identity on a vertex of weight zero, so its blocks come out zero by themselves.  A thread per entry
__global__ __launch_bounds__(256) void coarse_hz_kernel(int nHz, const int *__restrict__ hzVert, const int *__restrict__ hzSub,
                                                        const int *__restrict__ hzBlkPtr, const int *__restrict__ hzBlk,
                                                        const int *__restrict__ adj_idx, const double *__restrict__ Hval,
                                                        const double *__restrict__ wgt, const double *__restrict__ x,
                                                        const double *__restrict__ cen, const int *__restrict__ live,
                                                        double *__restrict__ hz)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nHz) return;
    const int t = hzSub[e];
    double acc[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) acc[k] = 0.0;
    if (live[t]) {
        const double ct0 = cen[3 * t], ct1 = cen[3 * t + 1], ct2 = cen[3 * t + 2];
        for (int b = hzBlkPtr[e]; b < hzBlkPtr[e + 1]; ++b) {
            const int blk = hzBlk[b];
            const int j = adj_idx[blk];
            const double w = wgt[j];
            if (w == 0.0) continue;   // a fixed column vertex: a zero row of Z
            double h[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) h[k] = Hval[hval_idx(blk, k)];
            const double b0 = x[3 * j] - ct0, b1 = x[3 * j + 1] - ct1, b2 = x[3 * j + 2] - ct2;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                acc[6 * r] += w * h[3 * r];
                acc[6 * r + 1] += w * h[3 * r + 1];
                acc[6 * r + 2] += w * h[3 * r + 2];
                acc[6 * r + 3] += w * (h[3 * r + 2] * b1 - h[3 * r + 1] * b2);
                acc[6 * r + 4] += w * (h[3 * r] * b2 - h[3 * r + 2] * b0);
                acc[6 * r + 5] += w * (h[3 * r + 1] * b0 - h[3 * r] * b1);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 18; ++k) hz[(size_t)18 * e + k] = acc[k];
}

// y from the row blocks' parts in ascending block order (coarse_prolong_kernel's prologue), by every workgroup alike
__device__ __forceinline__ void coarse_sum_y(int nc, int ld, const double *__restrict__ ypart, double *y)
{
    const int G = (nc + 63) / 64;
    for (int k = threadIdx.x; k < nc; k += 256) {
        double a = 0.0;
        for (int g = k >> 6; g < G; ++g) a += ypart[(size_t)g * ld + k];
        y[k] = a;
    }
    __syncthreads();
}

// r1 = r - W y: a thread per scalar dof, the vertex's entries in list order (subdomains ascending), the six products of an entry
// left to right
template <bool DEV>
__global__ __launch_bounds__(256) void coarse_deflate_kernel(int n, int nc, int ld, const int *__restrict__ hzPtr,
                                                             const int *__restrict__ hzSub, const double *__restrict__ hz,
                                                             const double *__restrict__ ypart, const double *__restrict__ r,
                                                             double *__restrict__ r1, const DevLoop *__restrict__ ctl)
{
    __shared__ double y[COARSE_NC_MAX];
    if constexpr (DEV) {
        if (ctl->status != 0 || ctl->phase != 0) return;
    }
    coarse_sum_y(nc, ld, ypart, y);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int v = k / 3, dd = k - 3 * v;
    double a = 0.0;
    for (int e = hzPtr[v]; e < hzPtr[v + 1]; ++e) {
        const double *row = hz + (size_t)18 * e + 6 * dd;
        const double *ys = y + 6 * hzSub[e];
        a += ((row[0] * ys[0] + row[1] * ys[1]) + (row[2] * ys[2] + row[3] * ys[3])) + (row[4] * ys[4] + row[5] * ys[5]);
    }
    r1[k] = r[k] - a;
}

// cd_t = c_t - (W^T u)_t with u_v = zsum_v / dup_v, the division as the merge makes it: one workgroup per subdomain over its entries
// in ascending vertex (the transposed index), the lanes by wave_sum's tree, the four waves pairwise.  c: Z^T r of the same
// application (coarse_restrict_kernel), so that the second solve gives y1 - y2
template <bool DEV>
__global__ __launch_bounds__(256) void coarse_restrict_hz_kernel(const int *__restrict__ hzTPtr, const int *__restrict__ hzTEnt,
                                                                 const int *__restrict__ hzVert, const double *__restrict__ hz,
                                                                 const int *__restrict__ dup, const double *__restrict__ zsum,
                                                                 const double *__restrict__ c, double *__restrict__ cd,
                                                                 const DevLoop *__restrict__ ctl)
{
    __shared__ double sm[5 * 6];
    if constexpr (DEV) {
        if (ctl->status != 0 || ctl->phase != 0) return;
    }
    const int t = blockIdx.x;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = hzTPtr[t] + threadIdx.x; k < hzTPtr[t + 1]; k += 256) {
        const int e = hzTEnt[k];
        const int v = hzVert[e];
        const int d = dup[v];
        double u0 = zsum[3 * v], u1 = zsum[3 * v + 1], u2 = zsum[3 * v + 2];
        if (d > 1) {
            u0 /= d;
            u1 /= d;
            u2 /= d;
        }
        const double *w = hz + (size_t)18 * e;
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] += (w[a] * u0 + w[6 + a] * u1) + w[12 + a] * u2;
    }
    coarse_block_sum<6>(acc, sm);
    if (threadIdx.x < 6) cd[6 * t + threadIdx.x] = c[6 * t + threadIdx.x] - sm[4 * 6 + threadIdx.x];
}

// out = a (.) isd per vertex (dotmi_pcg_apply_precond: the two scalings around the block solve that the solve's kernels do on the fly)
__global__ __launch_bounds__(256) void coarse_scale_kernel(int n, const double *__restrict__ a, const double *__restrict__ isd,
                                                           double *__restrict__ out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = a[k] * isd[k / 3];
}

void launch_coarse_centroid(const DevCoarse &C, hipStream_t st)
{
    hipLaunchKernelGGL(coarse_centroid_kernel, dim3(C.nParts), dim3(256), 0, st, (const int *)C.svPtr, (const int *)C.svIdx,
                       (const double *)C.wgt, (const double *)C.xf, (const int *)C.live, C.cen);
}
void launch_coarse_assemble(const DevCoarse &C, const DevMesh &M, const double *Hval, hipStream_t st)
{
    hipLaunchKernelGGL(coarse_assemble_kernel, dim3(C.nPairs), dim3(256), 0, st, (const int2 *)C.pair, (const int *)C.pairPtr,
                       (const int *)C.pairBlk, (const int *)M.blk_row, (const int *)M.adj_idx, Hval, (const double *)C.wgt,
                       (const double *)C.xf, (const double *)C.cen, (const int *)C.live, C.as0, C.as1, C.pairA);
}
void launch_coarse_fill(const DevCoarse &C, hipStream_t st)
{
    hipLaunchKernelGGL(coarse_fill_kernel, dim3((C.ncp * C.ncp + 255) / 256), dim3(256), 0, st, C.nc, C.ncp, C.nParts,
                       (const int *)C.pairAt, (const int *)C.live, (const double *)C.pairA, C.W2);
}
void launch_coarse_restrict(const DevCoarse &C, const double *r, hipStream_t st)
{
    hipLaunchKernelGGL(coarse_restrict_kernel, dim3(C.nParts), dim3(256), 0, st, (const int *)C.svPtr, (const int *)C.svIdx,
                       (const double *)C.wgt, (const double *)C.xf, (const double *)C.cen, (const int *)C.live, r, C.c);
}
void launch_coarse_solve(const DevCoarse &C, hipStream_t st, const double *c)
{
    hipLaunchKernelGGL(coarse_solve_kernel, dim3((C.nc + 63) / 64), dim3(256), 0, st, C.nc, C.ncp, (const double *)C.W, c ? c : (const double *)C.c,
                       C.y);
}
void launch_coarse_prolong(const DevCoarse &C, int nV, const double *isd, double *zsum, hipStream_t st)
{
    hipLaunchKernelGGL(coarse_prolong_kernel, dim3((nV + 255) / 256), dim3(256), 0, st, nV, C.nc, C.ncp, (const int *)C.vsPtr,
                       (const int *)C.vsIdx, (const double *)C.wgt, (const double *)C.xf, (const double *)C.cen, (const double *)C.y, isd, zsum);
}
void launch_coarse_rtab(const DevCoarse &C, hipStream_t st)
{
    const int total = C.nOwn * C.nmax;
    if (total == 0) return;   // (a rank without subdomains)
    hipLaunchKernelGGL(coarse_rtab_kernel, dim3((total + 255) / 256), dim3(256), 0, st, total, C.nmax, C.p0, C.dofmap, (const double *)C.wgt,
                       (const double *)C.xf, (const double *)C.cen, (const int *)C.live, C.rtab);
}
void launch_coarse_restrict_pad(const DevCoarse &C, const double *rpad, hipStream_t st, const DevLoop *ctl, int spec, double *c)
{
    if (!c) c = C.c;
    if (ctl)
        hipLaunchKernelGGL(coarse_restrict_pad_kernel<true>, dim3(C.nParts), dim3(256), 0, st, C.nmax, C.p0, C.nOwn, C.dofmap,
                           (const double4 *)C.rtab, rpad, c, ctl, spec);
    else
        hipLaunchKernelGGL(coarse_restrict_pad_kernel<false>, dim3(C.nParts), dim3(256), 0, st, C.nmax, C.p0, C.nOwn, C.dofmap,
                           (const double4 *)C.rtab, rpad, c, ctl, spec);
}
void launch_coarse_solve_loop(const DevCoarse &C, hipStream_t st, const DevLoop *ctl, int spec, const double *c)
{
    hipLaunchKernelGGL(coarse_solve_loop_kernel, dim3((C.nc + 63) / 64), dim3(256), 0, st, C.nc, C.ncp, (const double *)C.W,
                       c ? c : (const double *)C.c, C.y, ctl, spec);
}
void launch_coarse_restrict_loop(const DevCoarse &C, const double *r, hipStream_t st, const DevLoop *ctl)
{
    hipLaunchKernelGGL(coarse_restrict_loop_kernel, dim3(C.nParts), dim3(256), 0, st, (const int *)C.svPtr, (const int *)C.svIdx,
                       (const double *)C.wgt, (const double *)C.xf, (const double *)C.cen, (const int *)C.live, r, C.c, ctl);
}
void launch_coarse_hz(const DevCoarse &C, const DevMesh &M, const double *Hval, hipStream_t st)
{
    if (C.nHz == 0) return;
    hipLaunchKernelGGL(coarse_hz_kernel, dim3((C.nHz + 255) / 256), dim3(256), 0, st, C.nHz, (const int *)C.hzVert, (const int *)C.hzSub,
                       (const int *)C.hzBlkPtr, (const int *)C.hzBlk, (const int *)M.adj_idx, Hval, (const double *)C.wgt,
                       (const double *)C.xf, (const double *)C.cen, (const int *)C.live, C.hz);
}
void launch_coarse_deflate(const DevCoarse &C, int n, const double *r, double *r1, hipStream_t st, const DevLoop *ctl)
{
    const dim3 grid((n + 255) / 256);
    if (ctl)
        hipLaunchKernelGGL(coarse_deflate_kernel<true>, grid, dim3(256), 0, st, n, C.nc, C.ncp, (const int *)C.hzPtr, (const int *)C.hzSub,
                           (const double *)C.hz, (const double *)C.y, r, r1, ctl);
    else
        hipLaunchKernelGGL(coarse_deflate_kernel<false>, grid, dim3(256), 0, st, n, C.nc, C.ncp, (const int *)C.hzPtr, (const int *)C.hzSub,
                           (const double *)C.hz, (const double *)C.y, r, r1, ctl);
}
void launch_coarse_restrict_hz(const DevCoarse &C, const int *dup, const double *zsum, hipStream_t st, const DevLoop *ctl)
{
    if (ctl)
        hipLaunchKernelGGL(coarse_restrict_hz_kernel<true>, dim3(C.nParts), dim3(256), 0, st, (const int *)C.hzTPtr, (const int *)C.hzTEnt,
                           (const int *)C.hzVert, (const double *)C.hz, dup, zsum, (const double *)C.c, C.cd, ctl);
    else
        hipLaunchKernelGGL(coarse_restrict_hz_kernel<false>, dim3(C.nParts), dim3(256), 0, st, (const int *)C.hzTPtr, (const int *)C.hzTEnt,
                           (const int *)C.hzVert, (const double *)C.hz, dup, zsum, (const double *)C.c, C.cd, ctl);
}
void launch_coarse_scale(int n, const double *a, const double *isd, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(coarse_scale_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, a, isd, out);
}

// the host's copy of the dense matrix (dotmi_pcg_coarse_matrix) from the pairs' blocks, entry by entry as coarse_fill_kernel does
void coarse_dense_host(int nc, int nParts, const int *pairAt, const int *live, const double *pairA, double *A0)
{
    for (int I = 0; I < nc; ++I)
        for (int J = 0; J < nc; ++J) A0[(size_t)I * nc + J] = coarse_entry(I, J, nc, nParts, pairAt, live, pairA);
}

}  // namespace dotmi
