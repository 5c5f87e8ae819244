// nlh_kernels_scan.h -- the exclusive scan the lock-step drivers of the scalar-evaluation solvers share (nelder_mead:
// nlh_kernels_nm.h; brent_solver / newton_1var_solver: nlh_kernels_1var.h): per-problem point counts in ascending problem
// order -> the offsets of a compact point list.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Exclusive scan of the per-problem point counts in ascending problem order, in three steps: k_nm_scan_blocks scans each
// run of 1024 problems (off[p]: the offset inside its run, bsum[b]: the run's total), k_nm_scan_top scans the run totals
// (bpre[b], *total), and the driver's emit kernel adds bpre[p / 1024] and stores the final offset back into off[p].
// A driver may run nm_block_excl_scan inside its own 1024-thread kernel instead of k_nm_scan_blocks (the same offsets,
// one launch fewer).
static __device__ inline int32_t nm_wave_incl_scan(int32_t v)
{
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan over the workgroup (1024 threads); *total: the sum.  sh: 16 ints of LDS, free again on return.
static __device__ inline int32_t nm_block_excl_scan(int32_t v, int32_t *sh, int32_t *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int32_t inc = nm_wave_incl_scan(v);
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    if (wv == 0) {
        int32_t t = lane < nw ? sh[lane] : 0;
        t = nm_wave_incl_scan(t);
        if (lane < nw) sh[lane] = t;
    }
    __syncthreads();
    const int32_t base = wv > 0 ? sh[wv - 1] : 0;
    *total = sh[nw - 1];
    __syncthreads();
    return base + inc - v;
}

static __global__ void __launch_bounds__(1024)
k_nm_scan_blocks(int nprob, const int32_t *__restrict__ cnt, int32_t *__restrict__ off, int32_t *__restrict__ bsum)
{
    __shared__ int32_t sh[16];
    const size_t p = (size_t)blockIdx.x * 1024 + threadIdx.x;
    const int32_t v = p < (size_t)nprob ? cnt[p] : 0;
    int32_t tot;
    const int32_t ex = nm_block_excl_scan(v, sh, &tot);
    if (p < (size_t)nprob) off[p] = ex;
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

static __global__ void __launch_bounds__(1024)
k_nm_scan_top(int nb, const int32_t *__restrict__ bsum, int32_t *__restrict__ bpre, int32_t *__restrict__ total)
{
    __shared__ int32_t sh[16];
    int32_t carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int b = b0 + (int)threadIdx.x;
        int32_t tot;
        const int32_t ex = nm_block_excl_scan(b < nb ? bsum[b] : 0, sh, &tot);
        if (b < nb) bpre[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}
