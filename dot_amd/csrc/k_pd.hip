// k_pd.hip -- LBFGS-PD (DOTMI_FLAG_LBFGS_PD): the constant projective-dynamics Laplacian L = M + sum_e w_e D_e^T D_e
// (LBFGSTimeStepper.cpp:113-194) assembled on the device, filled into the scalar factor's work buffer, and the hot path
// z = L^-1 q for the three coordinate columns of q at once (Optimizer::dimSeparatedSolve, Optimizer.cpp:884-957) through the
// explicit inverse factor X (L^-1 = X^T X, the compact 64-row blocks of dotmi_internal.hpp RowTile, scalar nested-dissection order).
// Conventions as in k_device.hpp: fixed reduction shapes, no FP atomics.
#include "k_device.hpp"

namespace dotmi {

// ---- assembly: one thread per vertex row, its incident (element, corner) pairs in ascending element order --------------------
// D_e = [ -A^T 1 | A^T ] (3 x 4, A = restTriInv[e]); (D_e^T D_e)_ab = c_a . c_b with c_0 = -(sum of the rows of A), c_k = row k-1
__global__ __launch_bounds__(256) void pd_assemble_kernel(int nV, const int *__restrict__ adj_ptr, const int *__restrict__ adj_idx,
                                                          const int *__restrict__ inc_ptr, const int *__restrict__ inc,
                                                          const int4 *__restrict__ T, const double *__restrict__ A, int nTp,
                                                          const double *__restrict__ vol, const double *__restrict__ mu,
                                                          const double *__restrict__ lam, const double *__restrict__ mass,
                                                          const uint8_t *__restrict__ fixed, double dtSq, double *__restrict__ Lval)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nV) return;
    const int k0 = adj_ptr[v], k1 = adj_ptr[v + 1];
    for (int k = k0; k < k1; ++k) Lval[k] = 0.0;
    for (int i = inc_ptr[v]; i < inc_ptr[v + 1]; ++i) {
        const int e = inc[i] >> 2, a = inc[i] & 3;
        const int4 t = T[e];
        const int tv[4] = {t.x, t.y, t.z, t.w};
        double Ar[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) Ar[q] = A[(size_t)q * nTp + e];
        double c[4][3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            c[0][d] = -(Ar[d] + Ar[3 + d] + Ar[6 + d]);
            c[1][d] = Ar[d];
            c[2][d] = Ar[3 + d];
            c[3][d] = Ar[6 + d];
        }
        const double w = dtSq * vol[e] * (2.0 * mu[e] + lam[e]);
        for (int b = 0; b < 4; ++b) {
            const double val = w * (c[a][0] * c[b][0] + c[a][1] * c[b][1] + c[a][2] * c[b][2]);
            // column tv[b] in row v (ascending adjacency)
            int lo = k0, hi = k1 - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (adj_idx[mid] < tv[b]) lo = mid + 1;
                else hi = mid;
            }
            Lval[lo] += val;
        }
    }
    // M + D^T W D, then the fixed rows / columns (the reference zeroes them and puts 1 on the diagonal)
    const bool fv = fixed[v] != 0;
    for (int k = k0; k < k1; ++k) {
        const int u = adj_idx[k];
        double val = Lval[k];
        if (u == v) val += mass[v];
        if (fv || fixed[u]) val = 0.0;
        if (fv && u == v) val = 1.0;
        Lval[k] = val;
    }
}

void launch_pd_assemble(const DevMesh &M, const DevPD &D, double dtSq, hipStream_t st)
{
    hipLaunchKernelGGL(pd_assemble_kernel, dim3((M.nV + 255) / 256), dim3(256), 0, st, M.nV, M.adj_ptr, M.adj_idx, D.inc_ptr, D.inc,
                       M.T, M.A, M.nTp, M.vol, M.mu, M.lam, M.mass, M.fixed, dtSq, D.Lval);
}

// ---- scalar fill: every CSR entry of L to its one place in the work buffer (or nowhere: right of its row block), identity on the
// padding ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pd_fill_kernel(int nnz, const long long *__restrict__ dst, const double *__restrict__ Lval,
                                                      int npad, const long long *__restrict__ pad, double *__restrict__ W)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nnz) {
        const long long d = dst[t];
        if (d >= 0) W[d] = Lval[t];
    } else if (t - nnz < npad) {
        W[pad[t - nnz]] = 1.0;
    }
}

void launch_pd_fill(const DevPD &D, int nnz, double *W2, hipStream_t st)
{
    const int tot = nnz + D.npad;
    if (tot > 0)
        hipLaunchKernelGGL(pd_fill_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, nnz, D.fill_dst, D.Lval, D.npad, D.pad_dst, W2);
}

// ---- the hot path: z = X^T (X q) for the three columns of q -------------------------------------------------------------------
// One work item = one 64-row block of X and a range of its columns [cs, ce).  A thread owns the columns cs + tid + 256 k (k < PD_KC)
// and keeps q's three values there; the block's live rows go by in pairs: the pair's entries are loaded ONCE, the six row dots are
// summed over the workgroup (fixed tree), and the same registers then add X_rc t_r into the thread's three column accumulators.
// The partial z of the item's columns goes to ppart (three values per column, interleaved); pd_merge_kernel sums the items that
// cover a column in a fixed order.  Blocks whose rows are longer than one item (PD_KC x 256 columns) take two passes over their
// column chunks: PD_DOTS leaves every chunk's row-dot partials, PD_SCATTER sums them (chunk order) and reads its chunk again.
constexpr int PD_MODE_ONE = 0, PD_MODE_DOTS = 1, PD_MODE_SCATTER = 2;

template <int MODE>
__global__ __launch_bounds__(256) void pd_apply_kernel(const PdItem *__restrict__ items, const double *__restrict__ W,
                                                       const RowTile *__restrict__ rt, const int *__restrict__ cvert,
                                                       const double *__restrict__ q, double *__restrict__ ppart,
                                                       double *__restrict__ tdots)
{
    __shared__ double sm[2][4][6];
    const PdItem it = items[blockIdx.x];
    const int J = it.blk, cs = it.cs, ce = it.ce;
    const RowTile R = rt[J];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double qv[3][PD_KC], za[3][PD_KC];
    int col[PD_KC];
#pragma unroll
    for (int k = 0; k < PD_KC; ++k) {
        col[k] = cs + tid + 256 * k;
        const int vv = col[k] < ce ? cvert[col[k]] : -1;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            qv[d][k] = vv >= 0 ? q[3 * (size_t)vv + d] : 0.0;
            za[d][k] = 0.0;
        }
    }
    const double *Wb = W + R.off - R.c0;
    int buf = 0;
    const int r0 = 64 * J;
    for (int rr = 0; rr < 64; rr += 2) {
        bool live[2];
        double x[2][PD_KC];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = r0 + rr + j;
            live[j] = cvert[r] >= 0;
            const double *row = Wb + (long long)(rr + j) * R.ld;
#pragma unroll
            for (int k = 0; k < PD_KC; ++k) x[j][k] = (live[j] && col[k] < ce && col[k] <= r) ? row[col[k]] : 0.0;
        }
        if (!live[0] && !live[1]) continue;   // (uniform over the workgroup)
        double t[2][3];
        if constexpr (MODE == PD_MODE_SCATTER) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    double s = 0.0;
                    for (int ch = 0; ch < it.nch; ++ch) s += tdots[((size_t)(it.first + ch) * 64 + rr + j) * 3 + d];
                    t[j][d] = s;
                }
        } else {
            double dp[6];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < PD_KC; ++k) s += x[j][k] * qv[d][k];
                    dp[3 * j + d] = wave_sum(s);
                }
            if (lane == 0)
#pragma unroll
                for (int i = 0; i < 6; ++i) sm[buf][w][i] = dp[i];
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 6; ++i) t[i / 3][i % 3] = (sm[buf][0][i] + sm[buf][1][i]) + (sm[buf][2][i] + sm[buf][3][i]);
            buf ^= 1;   // (two buffers: the next pair's stores cannot overtake a slow reader of this one)
            if constexpr (MODE == PD_MODE_DOTS) {
                if (tid < 6) tdots[((size_t)blockIdx.x * 64 + rr + tid / 3) * 3 + tid % 3] = t[tid / 3][tid % 3];
                continue;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int d = 0; d < 3; ++d)
#pragma unroll
                for (int k = 0; k < PD_KC; ++k) za[d][k] += x[j][k] * t[j][d];
    }
    if constexpr (MODE != PD_MODE_DOTS) {
        double *out = ppart + it.pbase;
#pragma unroll
        for (int k = 0; k < PD_KC; ++k)
            if (col[k] < ce)
#pragma unroll
                for (int d = 0; d < 3; ++d) out[3 * (size_t)(col[k] - cs) + d] = za[d][k];
    }
}

// z[v] = sum over the items covering v's column of their partials (list order); fixed rows of L are identity rows
__global__ __launch_bounds__(256) void pd_merge_kernel(int nV, const int *__restrict__ mptr, const long long *__restrict__ ment,
                                                       const double *__restrict__ ppart, double *__restrict__ z)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nV) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = mptr[v]; k < mptr[v + 1]; ++k) {
        const double *p = ppart + ment[k];
        s0 += p[0];
        s1 += p[1];
        s2 += p[2];
    }
    z[3 * (size_t)v] = s0;
    z[3 * (size_t)v + 1] = s1;
    z[3 * (size_t)v + 2] = s2;
}

void launch_pd_apply(const DevPD &D, int nV, const double *q, double *z, hipStream_t st)
{
    if (D.nOne > 0)
        hipLaunchKernelGGL(pd_apply_kernel<PD_MODE_ONE>, dim3(D.nOne), dim3(256), 0, st, D.items, D.W, D.rt, D.cvert, q, D.ppart,
                           D.tdots);
    if (D.nLong > 0) {
        hipLaunchKernelGGL(pd_apply_kernel<PD_MODE_DOTS>, dim3(D.nLong), dim3(256), 0, st, D.items + D.nOne, D.W, D.rt, D.cvert, q,
                           D.ppart, D.tdots);
        hipLaunchKernelGGL(pd_apply_kernel<PD_MODE_SCATTER>, dim3(D.nLong), dim3(256), 0, st, D.items + D.nOne, D.W, D.rt, D.cvert,
                           q, D.ppart, D.tdots);
    }
    hipLaunchKernelGGL(pd_merge_kernel, dim3((nV + 255) / 256), dim3(256), 0, st, nV, D.mptr, D.ment, D.ppart, z);
}

}  // namespace dotmi
