// nlh_kernels_place.h -- where a thread of a (point, row) kernel works, in the two workgroup forms every such kernel has --
// row: a workgroup per (point, block of 256 rows); flat: ppw = 256 / m points per workgroup, short m -- and the problem list
// a wrapping launcher makes for its inner one.  The host side of the forms is nlh_launch.h.
#pragma once
#include "nlh_internal.h"

// thread -> (point q, row i), the point's x staged in LDS (FLAT: the x of the workgroup's ppw points); false: nothing to do.
// The model kernels: k_curve_*, k_expr_*.
template <bool FLAT>
__device__ static inline bool place_staged(int m, int n, int nblk, int ppw, int npoints, const double *__restrict__ X, double *xs, int &q, int &i,
                                           const double *&xq)
{
    if (FLAT) {
        const int q0 = blockIdx.x * ppw, nq = min(ppw, npoints - q0);
        for (int e = threadIdx.x; e < nq * n; e += 256) xs[e] = X[(size_t)q0 * n + e];
        __syncthreads();
        const int lp = threadIdx.x / m;
        q = q0 + lp; i = threadIdx.x - lp * m; xq = xs + lp * n;
        return lp < nq;
    }
    q = blockIdx.x / nblk;
    const int rb = blockIdx.x - q * nblk;
    for (int c = threadIdx.x; c < n; c += 256) xs[c] = X[(size_t)q * n + c];
    __syncthreads();
    i = rb * 256 + threadIdx.x; xq = xs;
    return i < m;
}

// thread -> (point q, row i) and nothing else; q = npoints for a thread beyond the workgroup's points.  The streaming
// kernels of the wrapping launchers: k_pmap_jac, k_loss_jac.
template <bool FLAT>
__device__ static inline void place_row(int m, int nblk, int ppw, int npoints, int &q, int &i)
{
    if (FLAT) {
        const int lp = threadIdx.x / m;
        q = blockIdx.x * ppw + lp; i = threadIdx.x - lp * m;
        if (lp >= ppw) q = npoints;
    } else {
        q = blockIdx.x / nblk;
        i = (blockIdx.x - q * nblk) * 256 + threadIdx.x;
    }
}

// q0 .. q0 + cnt as a problem list (a caller that passed no dprob, for the inner launcher)
static __global__ void __launch_bounds__(256) k_wrap_iota(int cnt, int q0, int32_t *__restrict__ list)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < cnt) list[q] = q0 + q;
}
