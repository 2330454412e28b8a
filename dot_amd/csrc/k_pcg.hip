// k_pcg.hip -- Newton-PCG (DOTMI_FLAG_NEWTON_PCG, dotmi_solve_hessian): the two kernels of a conjugate-gradient iteration on the
// global projected Hessian that are not the block solve.  H u = b from u = 0, preconditioned by the SYMMETRIC scaling of DOT's
// block solve, M_sym = D^-1/2 S D^-1/2 with S = sum_s R_s^T H_s^-1 R_s and D = diag(dup) (DOT's own D^-1 S averages on the left only
// and is no CG preconditioner: DESIGN.md section 9), in the single-reduction recurrences of Chronopoulos and Gear:
//     w = M_sym r,  s = H w,  gamma = r.w,  delta = w.s,  beta = gamma / gamma_old,  alpha = gamma / (delta - beta gamma / alpha_old),
//     d = w + beta d,  Hd = s + beta Hd,  u += alpha d,  r -= alpha Hd
// One iteration is four launches (dotmi_pcg.hip): launch_gemv on q = r (.) isd, launch_merge without the division (zsum = S q),
// pcg_spmv_kernel (w = zsum (.) isd formed on the fly, s, the partials of gamma and delta) and pcg_update_kernel (scalars in every
// workgroup's prologue, the vector updates, q for the next block solve, the partials of |r|^2).  isd = 1 / sqrt(dup) per vertex.
// The scalars of an iteration live in PcgRec, double-buffered by the parity of the iteration: a launch reads the record of the
// iteration before and workgroup 0 writes this iteration's, so no workgroup reads what another is writing; the |r|^2 partials are
// double-buffered the same way (every workgroup reads the last iteration's column while it writes its own row of this one's).
// Convergence, breakdown and the end of the work are decided on the device, in pcg_update_kernel's prologue -- the first launch that
// has the partials of |r|^2, gamma and delta together; from then on the kernels of this unit return at once and u stays as it is,
// so the host may enqueue several iterations between two reads of the record.  Reductions: NB_RED rows through write_partials, summed
// in chunked_sum's order; no atomics; two solves of one system are bit-identical.
// Sharded Hessian rows (DOTMI_FLAG_NEWTON_PCG_DIST, dotmi_solve_hessian on such a handle): pcg_spmv_rows_kernel in place of
// pcg_spmv_kernel -- w whole (pointwise from the already summed zsum), s and the partials of gamma and delta on the rank's rows
// [v0, v1) only, s into the packet [s (n) | gamma | delta] that the ranks sum -- and pcg_update_kernel<true>, which takes s and the
// two scalars from the summed packet.
#include "k_device.hpp"

namespace dotmi {

// chunked_sum (dotmi_internal.hpp) over N columns of NB_RED partials, column-major, by one wave: lane c < SUM_CHUNKS adds chunk c
// left to right, then the chunk sums are added left to right -- the host's additions in the host's order; every lane gets the totals.
// All loads are requested before the first addition.
template <int N>
__device__ __forceinline__ void pcg_sum_columns(const double *const (&col)[N], double (&tot)[N])
{
    constexpr int LR = NB_RED / SUM_CHUNKS;
    static_assert(LR * SUM_CHUNKS == NB_RED && SUM_CHUNKS <= 64, "chunks of equal length, a chunk per lane");
    const int lane = threadIdx.x & 63;
    double v[N][LR];
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int i = 0; i < LR; ++i) v[j][i] = lane < SUM_CHUNKS ? col[j][lane * LR + i] : 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < LR; ++i) acc += v[j][i];
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < SUM_CHUNKS; ++c) t += __shfl(acc, c, 64);
        tot[j] = t;
    }
}

// start of a solve: u = 0, r = b, d = Hd = 0, q = r (.) isd, the partials of |b|^2 as "iteration 0's |r|^2"; record 0 = a running
// solve that has done no iteration
__global__ __launch_bounds__(256) void pcg_init_kernel(int n, const double *__restrict__ b, const double *__restrict__ isd,
                                                       double *__restrict__ u, double *__restrict__ r, double *__restrict__ d,
                                                       double *__restrict__ Hd, double *__restrict__ q, double *__restrict__ partB,
                                                       double *__restrict__ partBT, PcgRec *__restrict__ rec)
{
    __shared__ double sm[4 * RED_K];
    double acc[RED_K];
#pragma unroll
    for (int j = 0; j < RED_K; ++j) acc[j] = 0.0;
    const int stride = gridDim.x * blockDim.x;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const double bk = b[k];
        u[k] = 0.0;
        r[k] = bk;
        d[k] = 0.0;
        Hd[k] = 0.0;
        q[k] = bk * isd[k / 3];
        acc[0] += bk * bk;
    }
    write_partials(acc, 1, partB, sm, partBT);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        PcgRec s;
        s.gamma = 1.0;
        s.alpha = 1.0;
        s.rr = 0.0;
        s.bb = 0.0;
        s.iter = 0;
        s.state = PCG_RUNNING;
        rec[0] = s;
    }
}

// w = zsum (.) isd, s = H w on the rows [v0, v1); partials of gamma = r.w (column 0) and delta = w.s (column 1).  The mapping of
// spmv_dots_kernel (k_loopvec.hip): 8 lanes per block row, SPMV_R rows per lane group and trip with their column loops interleaved,
// Hval entry-major through hval_idx; the column operand is scaled as it is loaded, so no launch exists only to scale.
// it: this iteration (1, 2, ...); a solve that has ended (the record of iteration it - 1) leaves at once.
// One body for both kernels below, so that the two mappings cannot drift apart.
// ROWS = false (pcg_spmv_kernel): every row, [v0, v1) = [0, nV); the rows' lanes write w and s.
// ROWS = true (pcg_spmv_rows_kernel, a handle whose Hessian rows are sharded): Hval holds the rank's rows [v0, v1) of the product
// (and those of its subdomains' vertices), so s and the partials are taken over these rows only; s goes into the packet
// [s (3 nV) | gamma | delta] that one all-reduce sums over the ranks, and the pointwise trips in front of the rows zero the packet
// outside the slice and write w whole -- it is pointwise from the already summed zsum, the same product the rows' lanes form for
// their dots, so the bits agree.  An ended solve leaves the packet as it is: it then travels as scratch (every rank issues the same
// collectives).
template <bool ROWS>
__device__ __forceinline__ void pcg_spmv_body(int nV, int v0, int v1, const int *__restrict__ adj_ptr, const int *__restrict__ adj_idx,
                                              const double *__restrict__ Hval, const double *__restrict__ zsum,
                                              const double *__restrict__ isd, const double *__restrict__ r, double *__restrict__ w,
                                              double *__restrict__ s, double *__restrict__ partA, double *__restrict__ partAT,
                                              const PcgRec *__restrict__ rec, int it, double *sm)
{
    if (rec[(it & 1) ^ 1].state != PCG_RUNNING) return;
    if constexpr (ROWS) {
        const int n = 3 * nV, stride = gridDim.x * blockDim.x;
        for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
            const int v = k / 3;
            w[k] = zsum[k] * isd[v];
            if (v < v0 || v >= v1) s[k] = 0.0;
        }
    }
    double acc[RED_K];
#pragma unroll
    for (int j = 0; j < RED_K; ++j) acc[j] = 0.0;
    const int sub = threadIdx.x & 7;
    const int ngroups = gridDim.x * 32;
    constexpr int R = 3;   // (SPMV_R of the direction kernels)
    for (int vbase = v0 + blockIdx.x * 32 + (threadIdx.x >> 3); vbase < v1; vbase += R * ngroups) {
        double a[R][3], wr[R][3], rr[R][3];
        int kb[R], nk[R], nkmax = 0;
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int v = vbase + u * ngroups;
            kb[u] = nk[u] = 0;
#pragma unroll
            for (int dd = 0; dd < 3; ++dd) a[u][dd] = wr[u][dd] = rr[u][dd] = 0.0;
            if (v < v1) {
                kb[u] = adj_ptr[v];
                nk[u] = adj_ptr[v + 1] - kb[u];
                // the row's own w and r do not depend on the column loop: requested first
                if (sub == 0) {
                    const double sc = isd[v];
                    wr[u][0] = zsum[3 * v] * sc; wr[u][1] = zsum[3 * v + 1] * sc; wr[u][2] = zsum[3 * v + 2] * sc;
                    rr[u][0] = r[3 * v]; rr[u][1] = r[3 * v + 1]; rr[u][2] = r[3 * v + 2];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < R; ++u) nkmax = max(nkmax, nk[u]);
        for (int t = sub; t < nkmax; t += 8) {
            int col[R];
            double h[R][9], pc[R][3], sc[R];
#pragma unroll
            for (int u = 0; u < R; ++u) col[u] = (t < nk[u]) ? adj_idx[kb[u] + t] : -1;
#pragma unroll
            for (int u = 0; u < R; ++u)
                if (t < nk[u]) {
#pragma unroll
                    for (int i = 0; i < 9; ++i) h[u][i] = Hval[hval_idx(kb[u] + t, i)];
                }
#pragma unroll
            for (int u = 0; u < R; ++u)
                if (col[u] >= 0) {
                    const double *zu = zsum + 3 * col[u];
                    sc[u] = isd[col[u]];
                    pc[u][0] = zu[0]; pc[u][1] = zu[1]; pc[u][2] = zu[2];
                }
#pragma unroll
            for (int u = 0; u < R; ++u)
                if (col[u] >= 0) {
                    const double p0 = pc[u][0] * sc[u], p1 = pc[u][1] * sc[u], p2 = pc[u][2] * sc[u];
                    a[u][0] += h[u][0] * p0 + h[u][1] * p1 + h[u][2] * p2;
                    a[u][1] += h[u][3] * p0 + h[u][4] * p1 + h[u][5] * p2;
                    a[u][2] += h[u][6] * p0 + h[u][7] * p1 + h[u][8] * p2;
                }
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int v = vbase + u * ngroups;
            const double a0 = group8_sum(a[u][0]), a1 = group8_sum(a[u][1]), a2 = group8_sum(a[u][2]);
            if (sub == 0 && v < v1) {
                if constexpr (!ROWS) {
                    w[3 * v] = wr[u][0]; w[3 * v + 1] = wr[u][1]; w[3 * v + 2] = wr[u][2];
                }
                s[3 * v] = a0; s[3 * v + 1] = a1; s[3 * v + 2] = a2;
                acc[0] += rr[u][0] * wr[u][0] + rr[u][1] * wr[u][1] + rr[u][2] * wr[u][2];
                acc[1] += wr[u][0] * a0 + wr[u][1] * a1 + wr[u][2] * a2;
            }
        }
    }
    write_partials(acc, 2, partA, sm, partAT);
}

__global__ __launch_bounds__(256) void pcg_spmv_kernel(int nV, const int *__restrict__ adj_ptr, const int *__restrict__ adj_idx,
                                                       const double *__restrict__ Hval, const double *__restrict__ zsum,
                                                       const double *__restrict__ isd, const double *__restrict__ r,
                                                       double *__restrict__ w, double *__restrict__ s, double *__restrict__ partA,
                                                       double *__restrict__ partAT, const PcgRec *__restrict__ rec, int it)
{
    __shared__ double sm[4 * RED_K];
    pcg_spmv_body<false>(nV, 0, nV, adj_ptr, adj_idx, Hval, zsum, isd, r, w, s, partA, partAT, rec, it, sm);
}

__global__ __launch_bounds__(256) void pcg_spmv_rows_kernel(int nV, int v0, int v1, const int *__restrict__ adj_ptr,
                                                            const int *__restrict__ adj_idx, const double *__restrict__ Hval,
                                                            const double *__restrict__ zsum, const double *__restrict__ isd,
                                                            const double *__restrict__ r, double *__restrict__ w,
                                                            double *__restrict__ pkt, double *__restrict__ partA,
                                                            double *__restrict__ partAT, const PcgRec *__restrict__ rec, int it)
{
    __shared__ double sm[4 * RED_K];
    pcg_spmv_body<true>(nV, v0, v1, adj_ptr, adj_idx, Hval, zsum, isd, r, w, pkt, partA, partAT, rec, it, sm);
}

// Iteration `it`.  Prologue (wave 0 of every workgroup, the same arithmetic everywhere): the record of iteration it - 1, the sums of
// this iteration's gamma and delta and of the last iteration's |r|^2; then the verdict --
//   the solve had ended before                          -> nothing (workgroup 0 carries the record over to this parity)
//   |r|^2 <= rel_tol^2 |b|^2                            -> converged after it - 1 iterations
//   gamma or the denominator of alpha not positive / not finite -> breakdown after it - 1 iterations (nothing is divided by them)
//   else beta, alpha and the vector updates of iteration `it`, q = r (.) isd for the next block solve, the partials of |r|^2
// The body's operands of the first trip are requested before the prologue (k_loopvec.hip, build_p_kernel).
// PACKET (sharded Hessian rows): s is the summed packet [s (n) | gamma | delta] and the two scalars are its tail -- the partAT
// columns, which hold this rank's rows only, are not read; |r|^2 stays the redundant sum over the replicated r
template <bool PACKET>
__global__ __launch_bounds__(256) void pcg_update_kernel(int n, const double *__restrict__ isd, const double *__restrict__ w,
                                                         const double *__restrict__ s, double *__restrict__ u, double *__restrict__ r,
                                                         double *__restrict__ d, double *__restrict__ Hd, double *__restrict__ q,
                                                         const double *__restrict__ partAT, double *__restrict__ partB,
                                                         double *__restrict__ partBT, PcgRec *__restrict__ rec, int it, double rel_tol)
{
    __shared__ double sm[4 * RED_K];
    __shared__ double sh_beta, sh_alpha;
    __shared__ int sh_go;
    const int par = it & 1;
    const int stride = gridDim.x * blockDim.x;
    const int k0 = blockIdx.x * blockDim.x + threadIdx.x;
    double wv = 0.0, sv = 0.0, dv = 0.0, hv = 0.0, uv = 0.0, rv = 0.0, iv = 0.0;
    if (k0 < n) {
        wv = w[k0];
        sv = s[k0];
        dv = d[k0];
        hv = Hd[k0];
        uv = u[k0];
        rv = r[k0];
        iv = isd[k0 / 3];
    }
    if (threadIdx.x < 64) {
        const PcgRec prev = rec[par ^ 1];
        double tot[3];
        if constexpr (PACKET) {
            const double *const cols[1] = {partBT + (size_t)(par ^ 1) * NB_RED};
            double t1[1];
            tot[0] = s[n];
            tot[1] = s[n + 1];
            pcg_sum_columns<1>(cols, t1);
            tot[2] = t1[0];
        } else {
            const double *const cols[3] = {partAT, partAT + NB_RED, partBT + (size_t)(par ^ 1) * NB_RED};
            pcg_sum_columns<3>(cols, tot);
        }
        const double gamma = tot[0], delta = tot[1];
        const double rr = prev.state == PCG_RUNNING ? tot[2] : prev.rr;
        const double bb = prev.state != PCG_RUNNING ? prev.bb : (prev.iter == 0 ? rr : prev.bb);
        int state = prev.state;
        double beta = 0.0, alpha = 0.0;
        if (state == PCG_RUNNING) {
            if (rr <= rel_tol * rel_tol * bb) {
                state = PCG_CONVERGED;
            } else if (!(gamma > 0.0) || !(gamma < INFINITY)) {
                state = PCG_BREAKDOWN;
            } else {
                beta = prev.iter == 0 ? 0.0 : gamma / prev.gamma;   // (the last iteration's gamma and alpha passed these tests)
                const double den = prev.iter == 0 ? delta : delta - beta * gamma / prev.alpha;
                if (!(den > 0.0) || !(den < INFINITY) || !(beta < INFINITY)) state = PCG_BREAKDOWN;
                else alpha = gamma / den;
                if (state == PCG_RUNNING && !(alpha < INFINITY)) state = PCG_BREAKDOWN;
            }
        }
        if (threadIdx.x == 0) {
            sh_go = state == PCG_RUNNING;
            sh_beta = beta;
            sh_alpha = alpha;
            if (blockIdx.x == 0) {
                PcgRec out;
                out.gamma = state == PCG_RUNNING ? gamma : prev.gamma;
                out.alpha = state == PCG_RUNNING ? alpha : prev.alpha;
                out.rr = rr;   // |r|^2 after iteration out.iter once the solve has ended; of the iteration before while it runs
                out.bb = bb;
                out.iter = state == PCG_RUNNING ? it : prev.iter;
                out.state = state;
                rec[par] = out;
            }
        }
    }
    __syncthreads();
    if (!sh_go) return;
    const double beta = sh_beta, alpha = sh_alpha;
    double acc[RED_K];
#pragma unroll
    for (int j = 0; j < RED_K; ++j) acc[j] = 0.0;
    for (int k = k0; k < n; k += stride) {
        if (k != k0) {
            wv = w[k];
            sv = s[k];
            dv = d[k];
            hv = Hd[k];
            uv = u[k];
            rv = r[k];
            iv = isd[k / 3];
        }
        const double dn = wv + beta * dv;
        const double hn = sv + beta * hv;
        const double rn = rv - alpha * hn;
        d[k] = dn;
        Hd[k] = hn;
        u[k] = uv + alpha * dn;
        r[k] = rn;
        q[k] = rn * iv;
        acc[0] += rn * rn;
    }
    write_partials(acc, 1, partB, sm, partBT + (size_t)par * NB_RED);
}

void launch_pcg_init(const DevPcg &C, int n, const double *b, double *u, double *q, hipStream_t st)
{
    hipLaunchKernelGGL(pcg_init_kernel, dim3(NB_RED), dim3(256), 0, st, n, b, (const double *)C.isd, u, C.r, C.d, C.Hd, q, C.partB,
                       C.partBT, C.rec);
}
void launch_pcg_spmv(const DevMesh &M, const DevPcg &C, const double *Hval, const double *zsum, int it, hipStream_t st)
{
    hipLaunchKernelGGL(pcg_spmv_kernel, dim3(NB_RED), dim3(256), 0, st, M.nV, (const int *)M.adj_ptr, (const int *)M.adj_idx, Hval, zsum,
                       (const double *)C.isd, (const double *)C.r, C.w, C.s, C.partA, C.partAT, (const PcgRec *)C.rec, it);
}
void launch_pcg_update(const DevPcg &C, int n, double *u, double *q, int it, double rel_tol, hipStream_t st)
{
    hipLaunchKernelGGL(pcg_update_kernel<false>, dim3(NB_RED), dim3(256), 0, st, n, (const double *)C.isd, (const double *)C.w,
                       (const double *)C.s, u, C.r, C.d, C.Hd, q, (const double *)C.partAT, C.partB, C.partBT, C.rec, it, rel_tol);
}
void launch_pcg_spmv_rows(const DevMesh &M, const DevPcg &C, const double *Hval, const double *zsum, int v0, int v1, int it, hipStream_t st)
{
    hipLaunchKernelGGL(pcg_spmv_rows_kernel, dim3(NB_RED), dim3(256), 0, st, M.nV, v0, v1, (const int *)M.adj_ptr, (const int *)M.adj_idx,
                       Hval, zsum, (const double *)C.isd, (const double *)C.r, C.w, C.pkt, C.partA, C.partAT, (const PcgRec *)C.rec, it);
}
void launch_pcg_update_packet(const DevPcg &C, int n, double *u, double *q, int it, double rel_tol, hipStream_t st)
{
    hipLaunchKernelGGL(pcg_update_kernel<true>, dim3(NB_RED), dim3(256), 0, st, n, (const double *)C.isd, (const double *)C.w,
                       (const double *)C.pkt, u, C.r, C.d, C.Hd, q, (const double *)C.partAT, C.partB, C.partBT, C.rec, it, rel_tol);
}

}  // namespace dotmi
