// merge_sum.hpp -- the sum behind every merge of the block solve, stated once for the merge kernels of k_loopvec.hip:
//   value of a scalar dof = sum over the subdomains that hold it, in vp order, of (sum over that subdomain's row tiles that hold the
//   column, in tile order from 0.0, of ppart[tile][column])
// in its three storage forms (DevParts; built by build_merge_lists, block_plan.hpp): the CSR list of a dof's tile partials, the same
// lists interleaved by wavefront, and the per-subdomain sums psub (reduce_partial_p_kernel: the inner sums, in tile order) gathered
// through the vertex's copies.  Every form performs the same additions in the same order, so which one a handle chooses never shows
// in a bit of the result.
// Needs neither the HIP runtime nor the handle: merge_check.cpp compiles it with the host compiler and compares the three functions
// bit for bit with the plain two-stage statement on lists build_merge_lists made.
// The form is the device's: a batch of list entries is requested first, then the batch's values, then the adds run in list order --
// one round trip per stage and batch instead of one per entry.
#pragma once

#if defined(__HIPCC__)
#define MERGE_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define MERGE_HD inline
#endif

namespace dotmi {

constexpr int MT_CH = 24;    // list entries in flight per thread (a dof has ~15: two subdomains x ~8 tiles)
constexpr int MT_PAD = -2147483647 - 1;   // end of a dof's interleaved list (no offset, plain or complemented, has this value)
constexpr int PSUB_CH = 4;   // copies of a vertex in flight per thread (a vertex is in 1-3 subdomains, rarely more)

// The CSR walk over mt_ent[e0, e1), the list of one dof (e0 = mt_ptr[k], e1 = mt_ptr[k + 1]): the offsets into ppart that make up its
// value, subdomain after subdomain; the first entry of a subdomain is stored complemented (~off) and closes the subdomain before it.
// Returns u + the sum (an empty list: u + 0.0).
MERGE_HD double merge_sum_csr(int e0, int e1, const int *__restrict__ mt_ent, const double *__restrict__ ppart, double u)
{
    double ps = 0.0;
    for (int e = e0; e < e1; e += MT_CH) {
        int off[MT_CH];
#pragma unroll
        for (int q = 0; q < MT_CH; ++q) off[q] = (e + q < e1) ? mt_ent[e + q] : 0;
        double w[MT_CH];
#pragma unroll
        for (int q = 0; q < MT_CH; ++q) {
            const int o = off[q] < 0 ? ~off[q] : off[q];
            w[q] = (e + q < e1) ? ppart[o] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < MT_CH; ++q)
            if (e + q < e1) {
                if (off[q] < 0 && e + q > e0) {   // a new subdomain starts: close the previous one
                    u += ps;
                    ps = 0.0;
                }
                ps += w[q];
            }
    }
    return u + ps;
}

// The same walk over dof k's list in its wave-interleaved form: entry q of the 64 consecutive dofs [64 w, 64 w + 64) is at
// mt_il[mt_wave[w].x + 64 q + lane], q < mt_wave[w].y (the longest list of the 64; shorter ones end in MT_PAD).  k >> 6 is uniform
// over the wave.  Int2: int2, or any pair of ints named x and y.
template <class Int2>
MERGE_HD double merge_sum_interleaved(int k, const Int2 *__restrict__ mt_wave, const int *__restrict__ mt_il,
                                      const double *__restrict__ ppart, double u)
{
    const Int2 wb = mt_wave[k >> 6];
    const int *__restrict__ lst = mt_il + wb.x + (k & 63);
    double ps = 0.0;
    for (int q0 = 0; q0 < wb.y; q0 += MT_CH) {
        int off[MT_CH];
#pragma unroll
        for (int q = 0; q < MT_CH; ++q) off[q] = (q0 + q < wb.y) ? lst[64 * (q0 + q)] : MT_PAD;
        double w[MT_CH];
#pragma unroll
        for (int q = 0; q < MT_CH; ++q) {
            const int o = off[q] < 0 ? ~off[q] : off[q];
            w[q] = (off[q] != MT_PAD) ? ppart[o] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < MT_CH; ++q)
            if (off[q] != MT_PAD) {
                if (off[q] < 0 && q0 + q > 0) {   // a new subdomain starts: close the previous one
                    u += ps;
                    ps = 0.0;
                }
                ps += w[q];
            }
    }
    return u + ps;
}

// The gather from the subdomains' own sums: u[d] += psub[vp_off[c] + d] for the copies c in [c0, c1) of one vertex (c0 = vp_ptr[v],
// c1 = vp_ptr[v + 1]) in vp order, NC consecutive components from the copy's padded position (NC = 3: a vertex; NC = 1: one dof, with
// psub advanced by the component).  The offsets of a batch first, then its values, then the adds.
template <int NC>
MERGE_HD void merge_sum_psub(int c0, int c1, const int *__restrict__ vp_off, const double *__restrict__ psub, double (&u)[NC])
{
    for (int c = c0; c < c1; c += PSUB_CH) {
        int off[PSUB_CH];
#pragma unroll
        for (int q = 0; q < PSUB_CH; ++q) off[q] = (c + q < c1) ? vp_off[c + q] : -1;
        double w[PSUB_CH][NC];
#pragma unroll
        for (int q = 0; q < PSUB_CH; ++q)
            if (off[q] >= 0) {
#pragma unroll
                for (int d = 0; d < NC; ++d) w[q][d] = psub[off[q] + d];
            }
#pragma unroll
        for (int q = 0; q < PSUB_CH; ++q)
            if (off[q] >= 0) {
#pragma unroll
                for (int d = 0; d < NC; ++d) u[d] += w[q][d];
            }
    }
}

}  // namespace dotmi
