// k_ic.hip -- LBFGS-HI (DOTMI_FLAG_LBFGS_HI): block (3 x 3) incomplete Cholesky IC(0) of the assembled projected Hessian in the
// multicolour ordering of ic_plan.hpp, and the hot path z = (L L^T)^-1 q.  One launch per colour: a colour's vertices share no
// edge, so its rows read earlier colours only (factor, forward sweep) or later ones only (backward sweep), and the launch
// boundary is the only synchronisation.  No atomics, every sum in the plan's list order with plain multiplies and adds
// (-ffp-contract=off), so tests/ic_reference.py restates the arithmetic operation for operation.
//
// Mapping: THREE lanes per vertex, lane r owning row r of every 3 x 3 block of its vertex' row (21 vertices per wavefront, lane 63
// idle).  Row r of L_ij = (A_ij - sum_k L_ik L_jk^T) L_jj^-T needs row r of the row's own earlier blocks only -- the lane's own
// stores -- so the off-diagonal work has no cross-lane dependence; the diagonal block and the two sweeps exchange three values
// per vertex through lane shuffles.  The work is a chain of dependent gathers (index -> block -> neighbour's vector), bound by
// latency and not by bytes: the sweeps read four list entries ahead (indices first, then the values, then the arithmetic in list
// order) so that several gathers are in flight per lane, and three lanes per vertex put three times the waves of a
// thread-per-vertex mapping on a colour of a few hundred vertices.
#include "k_device.hpp"

namespace dotmi {

constexpr int IC_VPW = 21;   // vertices per wavefront (3 lanes each)

// this lane's vertex position p in [c0, c1), its block row r and the first lane of its group; false: nothing to do
__device__ inline bool ic_lane(int c0, int c1, int &p, int &r, int &base)
{
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    r = lane % 3;
    base = lane - r;
    p = c0 + wave * IC_VPW + lane / 3;
    return lane < 3 * IC_VPW && p < c1;
}

static inline dim3 ic_grid(int count) { return dim3((unsigned)(((count + IC_VPW - 1) / IC_VPW + 3) / 4)); }

// ---- fill: lower blocks and diagonals of the global block-CSR -> factor storage (nL lower blocks, then nV diagonals, row-major) --
// the diagonal gets the shift A_ii += sigma diag(A_ii).  Fixed vertices keep the rows Hval already has -- zero couplings, identity
// diagonal -- and their diagonal is shifted like every other: it becomes (1 + sigma) I, so the solve returns r / (1 + sigma)
// there.  The gradient of a fixed vertex is zero, so no search direction sees it; tests/ic_reference.py does the same.
__global__ __launch_bounds__(256) void ic_fill_kernel(int nL, int nV, const int *__restrict__ lsrc, const int *__restrict__ dsrc,
                                                      const double *__restrict__ Hval, double sigma, double *__restrict__ F)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 9ll * ((long long)nL + nV)) return;
    const int b = (int)(t / 9), e = (int)(t % 9);
    if (b < nL) {
        F[t] = Hval[hval_idx(lsrc[b], e)];
    } else {
        double a = Hval[hval_idx(dsrc[b - nL], e)];
        if (e % 4 == 0) a = a + sigma * a;
        F[t] = a;
    }
}

// ---- factorisation of the rows of one colour, positions [c0, c1) -------------------------------------------------------------------
// per lower neighbour j in order: L_ij = (A_ij - sum_k L_ik L_jk^T) L_jj^-T; then L_ii = chol(A_ii - sum_k L_ik L_ik^T).  A
// non-positive pivot of the 3 x 3 Cholesky sets *flag and stores the identity, so no NaN reaches later colours.
__global__ __launch_bounds__(256) void ic_factor_colour_kernel(int c0, int c1, int nL, const int *__restrict__ lptr,
                                                               const int *__restrict__ lidx, const int *__restrict__ pptr,
                                                               const int *__restrict__ pa, const int *__restrict__ pb,
                                                               double *F, int *__restrict__ flag)
{
    int p, r, base;
    if (!ic_lane(c0, c1, p, r, base)) return;
    double *D = F + 9 * (size_t)nL;
    const int s0 = lptr[p], s1 = lptr[p + 1];
    for (int s = s0; s < s1; ++s) {
        double *Ls = F + 9 * (size_t)s + 3 * r;
        double t0 = Ls[0], t1 = Ls[1], t2 = Ls[2];
        const int q1 = pptr[s + 1];
        for (int q = pptr[s]; q < q1; ++q) {
            const double *a = F + 9 * (size_t)pa[q] + 3 * r;   // row r of L_ik: this lane's own earlier store
            const double *b = F + 9 * (size_t)pb[q];           // L_jk: an earlier colour's
            const double a0 = a[0], a1 = a[1], a2 = a[2];
            t0 = t0 - ((a0 * b[0] + a1 * b[1]) + a2 * b[2]);
            t1 = t1 - ((a0 * b[3] + a1 * b[4]) + a2 * b[5]);
            t2 = t2 - ((a0 * b[6] + a1 * b[7]) + a2 * b[8]);
        }
        const double *d = D + 9 * (size_t)lidx[s];   // L_jj, lower triangular: X L_jj^T = T row by row
        const double x0 = t0 / d[0];
        const double x1 = (t1 - x0 * d[3]) / d[4];
        const double x2 = ((t2 - x0 * d[6]) - x1 * d[7]) / d[8];
        Ls[0] = x0;
        Ls[1] = x1;
        Ls[2] = x2;
    }
    // row r of A_ii - sum_k L_ik L_ik^T: the rows c of L_ik come from the group's other lanes
    double *Dp = D + 9 * (size_t)p;
    double e0 = Dp[3 * r], e1 = Dp[3 * r + 1], e2 = Dp[3 * r + 2];
    for (int s = s0; s < s1; ++s) {
        const double *a = F + 9 * (size_t)s + 3 * r;
        const double a0 = a[0], a1 = a[1], a2 = a[2];
        const double b00 = __shfl(a0, base), b01 = __shfl(a1, base), b02 = __shfl(a2, base);
        const double b10 = __shfl(a0, base + 1), b11 = __shfl(a1, base + 1), b12 = __shfl(a2, base + 1);
        const double b20 = __shfl(a0, base + 2), b21 = __shfl(a1, base + 2), b22 = __shfl(a2, base + 2);
        e0 = e0 - ((a0 * b00 + a1 * b01) + a2 * b02);
        e1 = e1 - ((a0 * b10 + a1 * b11) + a2 * b12);
        e2 = e2 - ((a0 * b20 + a1 * b21) + a2 * b22);
    }
    // every lane of the group factors the whole block (lower triangle: entries 00, 10, 11, 20, 21, 22) and stores its row
    const double d00 = __shfl(e0, base);
    const double d10 = __shfl(e0, base + 1), d11 = __shfl(e1, base + 1);
    const double d20 = __shfl(e0, base + 2), d21 = __shfl(e1, base + 2), d22 = __shfl(e2, base + 2);
    bool ok = d00 > 0.0;
    const double l00 = sqrt(d00);
    const double l10 = d10 / l00, l20 = d20 / l00;
    const double p11 = d11 - l10 * l10;
    ok = ok && p11 > 0.0;
    const double l11 = sqrt(p11);
    const double l21 = (d21 - l20 * l10) / l11;
    const double p22 = (d22 - l20 * l20) - l21 * l21;
    ok = ok && p22 > 0.0;
    const double l22 = sqrt(p22);
    double o0, o1, o2;
    if (ok) {
        o0 = r == 0 ? l00 : r == 1 ? l10 : l20;
        o1 = r == 0 ? 0.0 : r == 1 ? l11 : l21;
        o2 = r == 2 ? l22 : 0.0;
    } else {
        o0 = r == 0 ? 1.0 : 0.0;
        o1 = r == 1 ? 1.0 : 0.0;
        o2 = r == 2 ? 1.0 : 0.0;
        if (r == 0) *flag = 1;   // (every writer stores the same value)
    }
    Dp[3 * r] = o0;
    Dp[3 * r + 1] = o1;
    Dp[3 * r + 2] = o2;
}

// ---- forward sweep of one colour: y_i = L_ii^-1 (b_i - sum_{j lower} L_ij y_j) -----------------------------------------------------
// b is read in vertex order (the permutation is the launch's own), y is kept in order position
__global__ __launch_bounds__(256) void ic_forward_colour_kernel(int c0, int c1, int nL, const int *__restrict__ vert,
                                                                const int *__restrict__ lptr, const int *__restrict__ lidx,
                                                                const double *__restrict__ F, const double *__restrict__ b,
                                                                double *y)
{
    int p, r, base;
    if (!ic_lane(c0, c1, p, r, base)) return;
    double t = b[3 * (size_t)vert[p] + r];
    const int s1 = lptr[p + 1];
    for (int s = lptr[p]; s < s1; s += 4) {
        int j[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) j[u] = s + u < s1 ? lidx[s + u] : -1;
        double a[4][3], yj[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j[u] >= 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    a[u][c] = F[9 * (size_t)(s + u) + 3 * r + c];
                    yj[u][c] = y[3 * (size_t)j[u] + c];
                }
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (j[u] >= 0) t = t - ((a[u][0] * yj[u][0] + a[u][1] * yj[u][1]) + a[u][2] * yj[u][2]);
    }
    const double t0 = __shfl(t, base), t1 = __shfl(t, base + 1), t2 = __shfl(t, base + 2);
    const double *d = F + 9 * ((size_t)nL + p);
    const double y0 = t0 / d[0];
    const double y1 = (t1 - d[3] * y0) / d[4];
    const double y2 = ((t2 - d[6] * y0) - d[7] * y1) / d[8];
    y[3 * (size_t)p + r] = r == 0 ? y0 : r == 1 ? y1 : y2;
}

// ---- backward sweep of one colour: x_i = L_ii^-T (y_i - sum_{k upper} L_ki^T x_k), a gather over the upper list --------------------
// x is written (and the later colours' x read) in vertex order
__global__ __launch_bounds__(256) void ic_backward_colour_kernel(int c0, int c1, int nL, const int *__restrict__ vert,
                                                                 const int *__restrict__ uptr, const int *__restrict__ ublk,
                                                                 const int *__restrict__ uvert, const double *__restrict__ F,
                                                                 const double *__restrict__ y, double *x)
{
    int p, r, base;
    if (!ic_lane(c0, c1, p, r, base)) return;
    double t = y[3 * (size_t)p + r];
    const int u1 = uptr[p + 1];
    for (int q = uptr[p]; q < u1; q += 4) {
        int s[4], k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s[u] = q + u < u1 ? ublk[q + u] : -1;
            k[u] = q + u < u1 ? uvert[q + u] : 0;
        }
        double a[4][3], xk[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (s[u] >= 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    a[u][c] = F[9 * (size_t)s[u] + 3 * c + r];   // column r of L_ki
                    xk[u][c] = x[3 * (size_t)k[u] + c];
                }
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (s[u] >= 0) t = t - ((a[u][0] * xk[u][0] + a[u][1] * xk[u][1]) + a[u][2] * xk[u][2]);
    }
    const double t0 = __shfl(t, base), t1 = __shfl(t, base + 1), t2 = __shfl(t, base + 2);
    const double *d = F + 9 * ((size_t)nL + p);
    const double x2 = t2 / d[8];
    const double x1 = (t1 - d[7] * x2) / d[4];
    const double x0 = ((t0 - d[3] * x1) - d[6] * x2) / d[0];
    x[3 * (size_t)vert[p] + r] = r == 0 ? x0 : r == 1 ? x1 : x2;
}

void launch_ic_fill(const DevIC &D, const double *Hval, double sigma, hipStream_t st)
{
    const long long tot = 9ll * ((long long)D.nL + D.nV);
    hipLaunchKernelGGL(ic_fill_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, D.nL, D.nV, D.lsrc, D.dsrc, Hval, sigma,
                       D.F);
}

void launch_ic_factor_colour(const DevIC &D, int c0, int c1, hipStream_t st)
{
    if (c1 <= c0) return;
    hipLaunchKernelGGL(ic_factor_colour_kernel, ic_grid(c1 - c0), dim3(256), 0, st, c0, c1, D.nL, D.lptr, D.lidx, D.pptr, D.pa, D.pb,
                       D.F, D.flag);
}

void launch_ic_forward_colour(const DevIC &D, int c0, int c1, const double *b, hipStream_t st)
{
    if (c1 <= c0) return;
    hipLaunchKernelGGL(ic_forward_colour_kernel, ic_grid(c1 - c0), dim3(256), 0, st, c0, c1, D.nL, D.vert, D.lptr, D.lidx, D.F, b, D.yw);
}

void launch_ic_backward_colour(const DevIC &D, int c0, int c1, double *x, hipStream_t st)
{
    if (c1 <= c0) return;
    hipLaunchKernelGGL(ic_backward_colour_kernel, ic_grid(c1 - c0), dim3(256), 0, st, c0, c1, D.nL, D.vert, D.uptr, D.ublk, D.uvert, D.F,
                       D.yw, x);
}

}  // namespace dotmi
