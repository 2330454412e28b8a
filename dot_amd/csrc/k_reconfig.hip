// k_reconfig.hip -- what a change of the materials or of the time step on a live handle runs on the device (dotmi_reconfig.hip):
// the per-slot Lame parameters of a patch family gathered from the global per-element arrays, and x~ from the resident x_n and v
#include <hip/hip_runtime.h>

#include "dotmi_internal.hpp"

namespace dotmi {

// slot s of a patch family holds element slotElem[s] (-1: padding).  A vertex patch family carries an element in more than
// one slot: every copy is written, because the loop is over the slots.
__global__ void __launch_bounds__(256) gather_lame_kernel(const int *__restrict__ slotElem, size_t nSlots, const double *__restrict__ mu,
                                                          const double *__restrict__ lam, double *__restrict__ mu_s,
                                                          double *__restrict__ lam_s)
{
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nSlots) return;
    const int e = slotElem[s];
    mu_s[s] = e < 0 ? 1.0 : mu[e];
    lam_s[s] = e < 0 ? 1.0 : lam[e];
}

void launch_gather_lame(const int *slotElem, size_t nSlots, const double *mu, const double *lam, double *mu_s, double *lam_s,
                        hipStream_t st)
{
    if (nSlots == 0) return;
    hipLaunchKernelGGL(gather_lame_kernel, dim3((unsigned)((nSlots + 255) / 256)), dim3(256), 0, st, slotElem, nSlots, mu, lam, mu_s,
                       lam_s);
}

struct Vec3Arg {
    double v[3];
};

// the expression of dotmi_set_state and of be_update_kernel, so that the three agree to the bit
__global__ void __launch_bounds__(256) x_tilde_kernel(int nV, const uint8_t *__restrict__ fixed, const double *__restrict__ xn,
                                                      const double *__restrict__ v, double dt, Vec3Arg gdtsq, double *__restrict__ xt)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nV) return;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int k = 3 * i + d;
        const double xv = xn[k];
        xt[k] = fixed[i] ? xv : xv + (v[k] * dt + gdtsq.v[d]);
    }
}

void launch_x_tilde(int nV, const uint8_t *fixed, const double *xn, const double *v, double dt, const double *gdtsq, double *xt,
                    hipStream_t st)
{
    Vec3Arg g = {{gdtsq[0], gdtsq[1], gdtsq[2]}};
    hipLaunchKernelGGL(x_tilde_kernel, dim3((nV + 255) / 256), dim3(256), 0, st, nV, fixed, xn, v, dt, g, xt);
}

}  // namespace dotmi
