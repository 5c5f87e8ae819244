// nlh_kernels_bin.h -- bin-integrated fits (include/nonlin_hip_bin.h: nlh_bin_*): the kernel behind the wrapping launchers
// nlh_bin_device_fcn / nlh_bin_device_jac and nlh_bin_apply_batch.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off).  v [0 .. Q m - 1] one column, node
// major -- the model values of a residual call, a column of the inner Jacobian, a column handed to apply --, c the Q weights of
// the rule, s the per-bin scale of the point's problem or none:
//   acc = +0.0;  for q = 0 .. Q-1 ascending:  t = c[q] * v[q m + i];  acc = acc + t
//   g = s ? s[i] * acc : acc
//   residual: out_i = g - y_i, with weights w_i * out_i;  Jacobian: g, with weights w_i * g;  a bin with w_i == 0.0 is STORED
//   as +0.0.  apply: g.
// One thread owns the whole chain of an output, so its bits depend on nothing but the column and the rule.
//
// k_bin is a streaming kernel: 8 (Q + 1) m ncol bytes per point and 2 Q operations per output, nothing reused, so bytes bind.
// Its shape is k_loss_jac's: a thread per (point, bin), the columns in a loop, in the two workgroup forms -- row: a workgroup
// per (point, 256 bins); flat: 256 / m points per workgroup -- and with the columns optionally split over gridDim.y.  Node
// major makes a wave's load of one node plane 64 consecutive doubles: no staging.  The loads of four nodes are issued before
// the first of their multiplies, so that a thread has four planes in flight.
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

struct BinArgs {
    const double *s;                   // [m] or [nprob][m], or null
    const double *y;                   // [nprob][m], residual calls only
    const double *w;                   // [nprob][m] or null
    const int32_t *dprob;              // point q is problem dprob[q]; null: q
    int32_t Q, shared_s;
    double c[NLH_BIN_MAX_Q];
};

// what a call is: the residual (out = g - y) or a Jacobian / apply (g), both with weights
#define BIN_FCN 0
#define BIN_JAC 1

// V [npoints][ncol][Q m] -> O [npoints][ncol][m].  grid.x: workgroups over (point, block of 256 bins) -- FLAT: ppw points
// each --, grid.y: groups of cpg columns.
template <bool FLAT>
static __global__ void __launch_bounds__(256)
k_bin(BinArgs A, int mode, int m, int ncol, int nblk, int ppw, int cpg, int npoints, const double *__restrict__ V, double *__restrict__ O)
{
    int q, i;
    place_row<FLAT>(m, nblk, ppw, npoints, q, i);
    const int j0 = blockIdx.y * cpg, j1 = min(j0 + cpg, ncol);
    if (q >= npoints || i >= m || j0 >= j1) return;              // (no barrier below)
    const size_t ms = (size_t)m, p = (size_t)(A.dprob ? A.dprob[q] : q);
    const int Q = A.Q;
    const size_t at = p * ms + i;
    const bool scaled = A.s != nullptr;
    const double sc = scaled ? A.s[A.shared_s ? (size_t)i : at] : 1.0;
    const double yi = mode == BIN_FCN ? A.y[at] : 0.0;
    const bool weighted = A.w != nullptr;
    const double wi = weighted ? A.w[at] : 1.0;
    const double *v = V + ((size_t)q * ncol + j0) * (ms * Q) + i;
    double *o = O + ((size_t)q * ncol + j0) * ms + i;
    for (int j = j0; j < j1; ++j, v += ms * Q, o += ms) {
        double acc = 0.0;
        int k = 0;
        for (; k + 4 <= Q; k += 4) {
            const double *vk = v + (size_t)k * ms;
            const double v0 = vk[0], v1 = vk[ms], v2 = vk[2 * ms], v3 = vk[3 * ms];
            const double t0 = A.c[k] * v0, t1 = A.c[k + 1] * v1, t2 = A.c[k + 2] * v2, t3 = A.c[k + 3] * v3;
            acc = acc + t0; acc = acc + t1; acc = acc + t2; acc = acc + t3;
        }
        for (; k < Q; ++k) {
            const double t = A.c[k] * v[(size_t)k * ms];
            acc = acc + t;
        }
        double g = scaled ? sc * acc : acc;
        if (mode == BIN_FCN) g = g - yi;
        if (weighted) g = wi == 0.0 ? 0.0 : wi * g;
        *o = g;
    }
}
