// nlh_kernels_starts.h -- the kernels of the box scan (include/nonlin_hip_starts.h states the arithmetic; nlh_starts.hip launches
// them).  The only floating-point operations are the cost's: everything else moves values or compares them.
#pragma once
#include "nlh_common.h"

static const int STARTS_KEEP = NLH_STARTS_MAX_KEEP;                 // a lane's own list: always this long, in registers

// The launcher's points of one chunk: point q = (p - p0)*C + (c - c0) is candidate c of problem p.  One thread per
// coordinate; the thread of coordinate 0 writes the point's problem.
static __global__ void __launch_bounds__(256) k_starts_points(int n, int p0, int cnt, int c0, int C, const double *__restrict__ cand,
                                                        double *__restrict__ X, int32_t *__restrict__ prob)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)cnt * C * n;
    if (e >= total) return;
    const size_t q = e / n;
    const int d = (int)(e - q * n);
    const int pl = (int)(q / C), c = c0 + (int)(q - (size_t)pl * C);
    X[e] = cand[(size_t)c * n + d];
    if (d == 0) prob[q] = p0 + pl;
}

// cost[q] = sum F_i^2 of point q in the header's order: a wave per point, four points per workgroup; lane j sums the rows
// i = j (mod 64) in ascending i into one accumulator, then the shuffle tree of wave_reduce_sum.  The loads of four steps are
// issued before their adds: with every wave of a CU resident that is 64 KiB of coalesced 8-byte loads in flight per CU.
static __global__ void __launch_bounds__(256) k_starts_cost(int npoints, int m, const double *__restrict__ F, double *__restrict__ cost)
{
    const int lane = threadIdx.x & 63;
    const size_t q = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= (size_t)npoints) return;                               // (a whole wave leaves: no barrier follows)
    const double *__restrict__ f = F + q * (size_t)m;
    double s = 0.0;
    int i = lane;
    for (; i + 192 < m; i += 256) {
        const double a = f[i], b = f[i + 64], c = f[i + 128], d = f[i + 192];
        s = s + a * a;
        s = s + b * b;
        s = s + c * c;
        s = s + d * d;
    }
    for (; i < m; i += 64) {
        const double a = f[i];
        s = s + a * a;
    }
    s = wave_reduce_sum(s);
    if (lane == 0) cost[q] = s;
}

// (cost, index) ascending; the empty entry (+Inf, INT_MAX) is behind every entry that can be kept
__device__ __forceinline__ bool starts_less(double ca, int ia, double cb, int ib) { return ca < cb || (ca == cb && ia < ib); }

// The `keep` best of problem p = what it had (best, idx [nprob][keep], of the chunks before) and the chunk's C costs, one wave
// per problem, four problems per workgroup.  Every lane takes a stride of that list and keeps its own best STARTS_KEEP in
// registers, sorted; then `keep` rounds of a wave-wide minimum over the lanes' heads, the winning lane moving on to its next.
static __global__ void __launch_bounds__(256) k_starts_merge(int cnt, int p0, int C, int c0, int keep, const double *__restrict__ cost,
                                                       double *best, int32_t *idx)
{
    const int lane = threadIdx.x & 63;
    const int pl = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pl >= cnt) return;
    const size_t p = (size_t)p0 + pl;
    double bc[STARTS_KEEP];
    int bi[STARTS_KEEP];
#pragma unroll
    for (int k = 0; k < STARTS_KEEP; ++k) { bc[k] = INFINITY; bi[k] = 0x7fffffff; }
    const double *__restrict__ cc = cost + (size_t)pl * C;
    for (int e = lane; e < keep + C; e += 64) {
        double c;
        int i;
        if (e < keep) { c = best[p * keep + e]; i = idx[p * keep + e]; }
        else { c = cc[e - keep]; i = c0 + (e - keep); }
        if (!(fabs(c) <= DBL_MAX) || i < 0) continue;               // NaN, infinite, an empty slot: never kept
#pragma unroll
        for (int k = 0; k < STARTS_KEEP; ++k)
            if (starts_less(c, i, bc[k], bi[k])) {
                const double tc = bc[k]; const int ti = bi[k];
                bc[k] = c; bi[k] = i; c = tc; i = ti;
            }
    }
    for (int r = 0; r < keep; ++r) {
        double wc = bc[0];
        int wi = bi[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double oc = __shfl_xor(wc, off, 64);
            const int oi = __shfl_xor(wi, off, 64);
            if (starts_less(oc, oi, wc, wi)) { wc = oc; wi = oi; }
        }
        if (wi != 0x7fffffff && wi == bi[0]) {                      // the winner's lane (an index occurs once): its next entry
#pragma unroll
            for (int k = 0; k + 1 < STARTS_KEEP; ++k) { bc[k] = bc[k + 1]; bi[k] = bi[k + 1]; }
            bc[STARTS_KEEP - 1] = INFINITY; bi[STARTS_KEEP - 1] = 0x7fffffff;
        }
        if (lane == 0) {
            best[p * keep + r] = wi == 0x7fffffff ? INFINITY : wc;
            idx[p * keep + r] = wi == 0x7fffffff ? -1 : wi;
        }
    }
}

// best = +Inf, idx = -1: nothing kept yet
static __global__ void __launch_bounds__(256) k_starts_clear(size_t total, double *__restrict__ best, int32_t *__restrict__ idx)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    best[e] = INFINITY;
    idx[e] = -1;
}

// x0 [nprob][keep][n]: the kept candidates' rows of the table, NaN for an empty slot
static __global__ void __launch_bounds__(256) k_starts_finish(size_t total, int n, const double *__restrict__ cand, const int32_t *__restrict__ idx,
                                                        double *__restrict__ x0)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const size_t s = e / n;
    const int i = idx[s];
    x0[e] = i < 0 ? __longlong_as_double(0x7ff8000000000000ll) : cand[(size_t)i * n + (e - s * n)];
}

// which[p] = the k of the smallest finite cost[k][p], the lowest k on a tie, -1 when none is finite
static __global__ void __launch_bounds__(256) k_starts_pick(int nprob, int keep, const double *__restrict__ cost, int32_t *__restrict__ which)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)nprob) return;
    int w = -1;
    double b = INFINITY;
    for (int k = 0; k < keep; ++k) {
        const double c = cost[(size_t)k * nprob + p];
        if (fabs(c) <= DBL_MAX && (w < 0 || c < b)) { w = k; b = c; }
    }
    which[p] = w;
}

// dst [nprob][width] = row which[p] of src [keep][nprob][width], NaN for -1 (and for any k outside 0 .. keep-1: nothing
// outside src is read)
static __global__ void __launch_bounds__(256) k_starts_take(size_t total, int nprob, int keep, int width, const double *__restrict__ src,
                                                      const int32_t *__restrict__ which, double *__restrict__ dst)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int w = which[e / width];
    dst[e] = w < 0 || w >= keep ? __longlong_as_double(0x7ff8000000000000ll) : src[(size_t)w * nprob * width + e];
}
