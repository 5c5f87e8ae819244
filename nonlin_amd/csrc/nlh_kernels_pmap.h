// nlh_kernels_pmap.h -- parameter maps (include/nonlin_hip.h: nlh_pmap_*): the kernels behind the wrapping launchers
// nlh_pmap_device_fcn / nlh_pmap_device_jac and the one-call fits through a map.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off):
//   expand    free p_k = x[index_k], fixed p_k = full_k; tied k:  u = scale_k * p_src;  p_k = u + offset_k   (no chains: the
//             source of a tie is free or fixed, so a thread per (point, k) reads it straight from x or full)
//   gather    x[j] = full[free_to_full[j]]
//   contract  v = Jf[:, free_to_full[j]];  v = v + scale_k * Jf[:, k] for the ties of column j, k ascending
//   cov       cov_full[k][l] = (g_k * cov[j_k][j_l]) * g_l;  sigma_full[k] = fabs(g_k) * sigma[j_k];  +0.0 without a factor
// No sum crosses a row, so the value of a row does not depend on the launch shape it is computed in.
//
// k_pmap_jac is the one that moves bytes: 8 m (columns read) in and 8 m n out per point, nothing reused.  Its shape is
// k_curve_jac's: a thread per (point, row), column-major on both sides (a wave's load or store is 64 consecutive doubles),
// in the two workgroup forms -- row: a workgroup per (point, 256 rows); flat: 256 / m points per workgroup -- and with the free
// columns optionally split over gridDim.y.  The tables (free_to_full, the CSR list of ties per free column) are indexed by
// values that are uniform across the launch, so they are read by scalar loads and live in scalar registers.  A thread's loads
// are issued unconditionally on a clamped (point, row), the first column of the next free parameter ahead of the ties of
// the current one.
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

struct PmapTables {                    // device copies, owned by a context, or by the map for its three batch steps
    int N, n;
    const int32_t *kind, *index;       // [N]
    const double *scale, *offset;      // [N]
    const int32_t *f2f;                // [n]
    const int32_t *tptr, *tk;          // CSR: the ties of free column j are tk[tptr[j] .. tptr[j + 1]), ascending
    const double *ts;                  //      with their scales
    const int32_t *cj;                 // [N] free number of k or of its source; -1: no factor
    const double *cg;                  // [N] the factor g_k
};

// a thread per (point, full parameter)
static __global__ void __launch_bounds__(256)
k_pmap_expand(PmapTables T, int npoints, const int32_t *__restrict__ dprob, const double *__restrict__ X, const double *__restrict__ full,
              int shared_full, double *__restrict__ P)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)npoints * T.N) return;
    const int q = (int)(e / T.N), k = (int)(e - (size_t)q * T.N);
    const size_t row = shared_full ? 0 : (size_t)(dprob ? dprob[q] : q) * T.N;
    const int kd = T.kind[k];
    const int s = kd == NLH_PMAP_TIED ? T.index[k] : k;         // whose value is read: k itself, or the source of its tie
    const double v = T.kind[s] == NLH_PMAP_FREE ? X[(size_t)q * T.n + T.index[s]] : full[row + s];
    if (kd == NLH_PMAP_TIED) {
        const double u = T.scale[k] * v;
        P[e] = u + T.offset[k];
    } else P[e] = v;
}

// a thread per (problem, full parameter): the free ones go to their slot of x
static __global__ void __launch_bounds__(256)
k_pmap_gather(PmapTables T, int nprob, const double *__restrict__ full, double *__restrict__ x)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nprob * T.N) return;
    const int p = (int)(e / T.N), k = (int)(e - (size_t)p * T.N);
    if (T.kind[k] == NLH_PMAP_FREE) x[(size_t)p * T.n + T.index[k]] = full[e];
}

// The contraction.  grid.x: workgroups over (point, row block) -- FLAT: ppw points each --, grid.y: groups of cpg free columns.
template <bool FLAT>
static __global__ void __launch_bounds__(256)
k_pmap_jac(PmapTables T, int m, int nblk, int ppw, int cpg, int npoints, const double *__restrict__ Jf, double *__restrict__ J)
{
    int q, i;
    place_row<FLAT>(m, nblk, ppw, npoints, q, i);
    const bool on = q < npoints && i < m;
    const int qc = min(q, npoints - 1), ic = min(i, m - 1);
    const size_t ms = (size_t)m;
    const double *Jq = Jf + (size_t)qc * ms * T.N + ic;
    double *Oq = J + (size_t)qc * ms * T.n + ic;
    const int j0 = blockIdx.y * cpg, j1 = min(j0 + cpg, T.n);
    if (j0 >= j1) return;
    double nxt = Jq[(size_t)T.f2f[j0] * ms];
    int e1 = T.tptr[j0];
    for (int j = j0; j < j1; ++j) {
        double v = nxt;
        const int e0 = e1;
        e1 = T.tptr[j + 1];
        if (j + 1 < j1) nxt = Jq[(size_t)T.f2f[j + 1] * ms];
        for (int e = e0; e < e1; ++e) v = v + T.ts[e] * Jq[(size_t)T.tk[e] * ms];
        if (on) Oq[(size_t)j * ms] = v;
    }
}

// a thread per entry of cov_full (the first N of a problem also write sigma_full); cov_full or sigma_full may be null
static __global__ void __launch_bounds__(256)
k_pmap_cov(PmapTables T, int nprob, const double *__restrict__ cov, const double *__restrict__ sigma, const int32_t *__restrict__ fail,
           double *__restrict__ covf, double *__restrict__ sigf)
{
    const size_t NN = (size_t)T.N * T.N, per = covf ? NN : (size_t)T.N;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nprob * per) return;
    const int p = (int)(e / per);
    const size_t r = e - (size_t)p * per;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const bool bad = fail && fail[p] != 0;
    if (covf) {
        const int k = (int)(r / T.N), l = (int)(r - (size_t)k * T.N);
        const int jk = T.cj[k], jl = T.cj[l];
        double v = 0.0;
        if (jk >= 0 && jl >= 0) {
            const double c = T.cg[k] * cov[((size_t)p * T.n + jk) * T.n + jl];
            v = c * T.cg[l];
        }
        covf[e] = bad ? nan : v;
    }
    if (sigf && r < (size_t)T.N) {
        const int jk = T.cj[r];
        const double v = jk >= 0 ? fabs(T.cg[r]) * sigma[(size_t)p * T.n + jk] : 0.0;
        sigf[(size_t)p * T.N + r] = bad ? nan : v;
    }
}
