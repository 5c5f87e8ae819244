// nlh_kernels_group.h -- global fits (include/nonlin_hip.h: nlh_group_*): the kernels behind the wrapping launchers
// nlh_group_device_fcn / nlh_group_device_jac, the three batch steps and the one-call global fits.
//
// A group is G data sets of one inner model with N parameters, S of them shared; L = N - S.  The outer unknowns are
// n = S + G L: the shared parameters in ascending inner index, then per data set g its local ones in ascending inner index.
// Outer point q stands for the inner points q G + g, whose rows i are the outer rows g m + i.
//
// NOTHING HERE COMPUTES: every kernel copies values or writes +0.0 (NaN in k_group_expand behind a failure flag), so every
// result has the bits of its source whatever the launch shape.
//   expand    P[q G + g][k] = X[q][s]  (k the s-th shared parameter)  or  X[q][S + g L + l]  (k the l-th local one)
//   gather    x[p][j] = full[p G + g_j][k_j], g_j = 0 for a shared j
//   scatter   J[q][j][g m + i] = Jf[q G + g][k_j][i] for a shared j and for the local columns of g;  +0.0 in the local
//             columns of every other data set
//
// k_group_jac is the one that moves bytes: 8 G m N in and 8 G m (S + G L) out per outer point, nothing reused.  It is
// store-bound, and at large G most of what it stores is zeros: that is what a dense solver is handed.  Its shape is
// k_pmap_jac's: a thread per INNER (point, row), column-major on both sides (a wave's load or store is 64 consecutive
// doubles), the two workgroup forms of nlh_kernels_place.h over the inner points, the outer columns optionally split over
// gridDim.y.  In the row form a workgroup is one inner point, so its data set is uniform: which columns load and which store
// zero is a scalar branch, and the tables are read by scalar loads.  In the flat form the data set is per thread, and the
// load of a local column sits under the lanes' own condition.  A thread loads each of its N values once, on a clamped
// (point, row), and stores n.
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

struct GroupTables {                   // device copies, owned by a context, or by the group for its three batch steps
    int N, S, L, G, n;
    const int32_t *shared;             // [N] 1: shared
    const int32_t *slot;               // [N] number among the shared, or among the local, parameters
    const int32_t *sidx;               // [S] inner index of shared parameter s
    const int32_t *lidx;               // [L] inner index of local parameter l
};

// A thread per (inner point, inner parameter).  prob (optional): the outer problem of outer point q, for the inner problem
// list `list` (optional) [npoints G].  fail (optional): a non-zero flag of outer point q makes its values NaN.
static __global__ void __launch_bounds__(256)
k_group_expand(GroupTables T, int npoints, const int32_t *__restrict__ prob, const double *__restrict__ X, const int32_t *__restrict__ fail,
               double *__restrict__ P, int32_t *__restrict__ list)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)npoints * T.G * T.N) return;
    const size_t qi = e / T.N;
    const int k = (int)(e - qi * T.N);
    const int q = (int)(qi / T.G), g = (int)(qi - (size_t)q * T.G);
    const int j = T.shared[k] ? T.slot[k] : T.S + g * T.L + T.slot[k];
    const double v = X[(size_t)q * T.n + j];
    P[e] = fail && fail[q] != 0 ? __longlong_as_double(0x7ff8000000000000ll) : v;
    if (list && k == 0) list[qi] = (prob ? prob[q] : q) * T.G + g;
}

// a thread per (group, outer unknown)
static __global__ void __launch_bounds__(256)
k_group_gather(GroupTables T, int ngroup, const double *__restrict__ full, double *__restrict__ x)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)ngroup * T.n) return;
    const size_t p = e / T.n;
    const int j = (int)(e - p * T.n);
    int g = 0, k;
    if (j < T.S) k = T.sidx[j];
    else { g = (j - T.S) / T.L; k = T.lidx[j - T.S - g * T.L]; }
    x[e] = full[(p * T.G + g) * T.N + k];
}

// The scatter.  grid.x: workgroups over INNER (point, row block) -- FLAT: ppw inner points each --, grid.y: groups of cpg outer
// columns.  npin = npoints G inner points.
template <bool FLAT>
static __global__ void __launch_bounds__(256)
k_group_jac(GroupTables T, int m, int nblk, int ppw, int cpg, int npin, const double *__restrict__ Jf, double *__restrict__ J)
{
    int qi, i;
    place_row<FLAT>(m, nblk, ppw, npin, qi, i);
    const bool on = qi < npin && i < m;
    const int qc = min(qi, npin - 1), ic = min(i, m - 1);
    const int q = qc / T.G, g = qc - q * T.G;                   // (row form: uniform across the workgroup)
    const size_t ms = (size_t)m, M = ms * T.G;
    const double *Jq = Jf + (size_t)qc * ms * T.N + ic;
    double *Oq = J + (size_t)q * M * T.n + (size_t)g * ms + ic;
    const int j0 = blockIdx.y * cpg, j1 = min(j0 + cpg, T.n);
    if (j0 >= j1) return;
    // Column j is shared (j < S) or the local column (gp, l), j = S + gp L + l; (gp, l) walk with j.  The value of column
    // j + 1 is loaded before column j is stored: one load in flight per thread beside the store.
    int gp = 0, l = 0;
    if (j0 > T.S) { gp = (j0 - T.S) / T.L; l = j0 - T.S - gp * T.L; }
    auto value = [&](int j) { return j < T.S ? Jq[(size_t)T.sidx[j] * ms] : gp == g ? Jq[(size_t)T.lidx[l] * ms] : 0.0; };
    double nxt = value(j0);
    for (int j = j0; j < j1; ++j) {
        const double v = nxt;
        if (j >= T.S && ++l == T.L) { l = 0; ++gp; }            // (gp, l) of column j + 1
        if (j + 1 < j1) nxt = value(j + 1);
        if (on) Oq[(size_t)j * M] = v;
    }
}
