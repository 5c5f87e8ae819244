// nlh_kernels_pin.h -- the pin pair (include/nonlin_hip_profile.h: nlh_pin_*): the kernels behind the wrapping launchers
// nlh_pin_device_fcn / nlh_pin_device_jac.
//
// ONLY COPIES HAPPEN: no kernel here makes a floating-point operation, so a value's bits are those the inner launcher wrote
// or the caller handed in, whatever the launch shape, the slice or the batch.
//   expand    P[q][k] = x[q][k] below pos[w], theta[w] at pos[w], x[q][k - 1] above;  sp[q] = src[w];  pp[q] = pos[w]   (w = lp[q])
//   delete    dJ[q][j] = Jf[q][j] for j < pos[w], Jf[q][j + 1] otherwise
//
// k_pin_jac is the one that moves bytes: 8 m (N - 1) in and out per point, nothing reused, so it needs no LDS and its shape
// is k_pmap_jac's: a thread per (point, row), column-major on both sides (a wave's load or store is 64 consecutive doubles), in
// the two workgroup forms, the columns optionally split over gridDim.y.  It does less than k_pmap_jac: no tie pass, and the
// source column is j or j + 1 by one compare with the point's pos instead of a table entry per column.  The expansion leaves
// the point's pos beside its inner problem in the scratch (pp[q] = pos[lp[q]]), so the one load that stands in front of a
// thread's first column load is a single 4-byte load -- uniform over a workgroup in the row form, over m consecutive lanes in
// the flat form --, not the chain lp[q] -> pos[w].  Loads are issued unconditionally on a clamped (point, row), four columns of
// them ahead of their stores.
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

struct PinTables {                     // the caller's device tables (nlh_pin_wrap, nlh_pin_set)
    int N, nend;
    const int32_t *src, *pos;          // [nend]
    const double *theta;               // [nend]
};

// a thread per (point, inner parameter); the thread of parameter 0 also writes the point's inner problem and its pos
static __global__ void __launch_bounds__(256)
k_pin_expand(PinTables T, int npoints, const int32_t *__restrict__ lp, const double *__restrict__ X, double *__restrict__ P,
             int32_t *__restrict__ sp, int32_t *__restrict__ pp)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)npoints * T.N) return;
    const int q = (int)(e / T.N), k = (int)(e - (size_t)q * T.N);
    const int w = lp[q], ps = T.pos[w];
    const double *xq = X + (size_t)q * (T.N - 1);
    P[e] = k == ps ? T.theta[w] : xq[min(max(k < ps ? k : k - 1, 0), T.N - 2)];    // (clamped: a pos out of range reads inside x)
    if (k == 0) { sp[q] = T.src[w]; pp[q] = ps; }
}

// The deletion of column pos.  grid.x: workgroups over (point, row block) -- FLAT: ppw points each --, grid.y: groups of cpg of
// the N - 1 columns.
template <bool FLAT>
static __global__ void __launch_bounds__(256)
k_pin_jac(int N, const int32_t *__restrict__ pp, int m, int nblk, int ppw, int cpg, int npoints, const double *__restrict__ Jf,
          double *__restrict__ J)
{
    int q, i;
    place_row<FLAT>(m, nblk, ppw, npoints, q, i);
    const bool on = q < npoints && i < m;
    const int qc = min(q, npoints - 1), ic = min(i, m - 1);
    const int n = N - 1;
    const size_t ms = (size_t)m;
    const int ps = pp[qc];
    const double *Jq = Jf + (size_t)qc * ms * N + ic;
    double *Oq = J + (size_t)qc * ms * n + ic;
    const int j0 = blockIdx.y * cpg, j1 = min(j0 + cpg, n);
    int j = j0;
    for (; j + 4 <= j1; j += 4) {
        const double v0 = Jq[(size_t)(j + (j >= ps)) * ms], v1 = Jq[(size_t)(j + 1 + (j + 1 >= ps)) * ms];
        const double v2 = Jq[(size_t)(j + 2 + (j + 2 >= ps)) * ms], v3 = Jq[(size_t)(j + 3 + (j + 3 >= ps)) * ms];
        if (on) {
            Oq[(size_t)j * ms] = v0; Oq[(size_t)(j + 1) * ms] = v1;
            Oq[(size_t)(j + 2) * ms] = v2; Oq[(size_t)(j + 3) * ms] = v3;
        }
    }
    for (; j < j1; ++j) {
        const double v = Jq[(size_t)(j + (j >= ps)) * ms];
        if (on) Oq[(size_t)j * ms] = v;
    }
}
