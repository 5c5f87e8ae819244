// nlh_kernels_loss.h -- robust losses (include/nonlin_hip.h: nlh_loss_*): the kernels behind the wrapping launchers
// nlh_loss_device_fcn / nlh_loss_device_jac and nlh_loss_apply_batch.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off).  c the scale, r the inner
// residual, u = r / c, a = fabs(u):
//   LINEAR    out = r                                                            g = 1.0            wgt = 1.0
//   HUBER     a <= 1.0: out = r (bit for bit)                                    g = 1.0            wgt = 1.0
//             else (NaN lands here): v = 2.0*a; v = v - 1.0; s = sqrt(v);
//                       out = c*copysign(s, u)                                   g = 1.0/s          wgt = 1.0/a
//   SOFT_L1   z = u*u; s = sqrt(1.0 + z); k = sqrt(2.0/(s + 1.0)); out = c*(u*k) g = 1.0/(s*k)      wgt = 1.0/s
//   CAUCHY    z = u*u;  z == 0.0: out = r                                        g = 1.0            wgt = 1.0
//             else l = log1p(z); s = sqrt(l); out = c*copysign(s, u)             q = 1.0 + z; wgt = 1.0/q; g = (wgt*a)/s
// A scale that is not finite or not positive makes out, g and wgt NaN (every kind but LINEAR, which reads no scale).
// J'[i][j] = g_i * J[i][j]: one multiply per entry; no sum crosses a row, so the value of a row does not depend on the launch
// shape it is computed in.
//
// k_loss_jac is the one that moves bytes: 8 m (2 n + 1) per point (r and the n columns in, the n columns out), nothing reused.
// Its shape is k_pmap_jac's: a thread per (point, row), column-major (a wave's load or store is 64 consecutive doubles), in the
// two workgroup forms -- row: a workgroup per (point, 256 rows); flat: 256 / m points per workgroup -- and with the columns
// optionally split over gridDim.y.  A thread loads r, forms g once and scales its columns in place, four at a time: the four
// loads are issued before the first store, unconditionally on a clamped (point, row).
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

struct LossArgs {
    int kind;                          // NLH_LOSS_*
    int shared_scale;
    const double *scale;               // [nprob], or [1] with shared_scale
    const int32_t *dprob;              // point q reads scale[dprob[q]]; null: scale[q]
};

static __device__ __forceinline__ double loss_scale_of(const LossArgs &A, int q)
{
    return A.scale[A.shared_scale ? 0 : (A.dprob ? A.dprob[q] : q)];
}

// out, g, wgt of one residual (the table above)
static __device__ __forceinline__ void loss_eval(int kind, double c, double r, double &out, double &g, double &wgt)
{
    out = r; g = 1.0; wgt = 1.0;
    if (kind == NLH_LOSS_LINEAR) return;
    if (!(c > 0.0) || c > DBL_MAX) {
        out = g = wgt = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double u = r / c;
    const double a = fabs(u);
    if (kind == NLH_LOSS_HUBER) {
        if (a <= 1.0) return;
        double v = 2.0 * a;
        v = v - 1.0;
        const double s = sqrt(v);
        out = c * copysign(s, u);
        g = 1.0 / s;
        wgt = 1.0 / a;
    } else if (kind == NLH_LOSS_SOFT_L1) {
        const double z = u * u;
        const double s = sqrt(1.0 + z);
        const double k = sqrt(2.0 / (s + 1.0));
        out = c * (u * k);
        g = 1.0 / (s * k);
        wgt = 1.0 / s;
    } else {
        const double z = u * u;
        if (z == 0.0) return;
        const double l = log1p(z);
        const double s = sqrt(l);
        out = c * copysign(s, u);
        const double q = 1.0 + z;
        wgt = 1.0 / q;
        g = (wgt * a) / s;
    }
}

// in place on the inner launcher's F [npoints][m]: a thread per (point, row)
static __global__ void __launch_bounds__(256) k_loss_fcn(LossArgs A, int m, int npoints, double *__restrict__ F)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)npoints * m) return;
    const int q = (int)(e / m);
    double out, g, wgt;
    loss_eval(A.kind, loss_scale_of(A, q), F[e], out, g, wgt);
    F[e] = out;
}

// nlh_loss_apply_batch: a thread per (problem, row); every output may be null, out may be r itself
static __global__ void __launch_bounds__(256)
k_loss_apply(LossArgs A, int m, int nprob, const double *r, double *out, double *__restrict__ g, double *__restrict__ wgt)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nprob * m) return;
    const int p = (int)(e / m);
    double o, gg, w;
    loss_eval(A.kind, loss_scale_of(A, p), r[e], o, gg, w);
    if (out) out[e] = o;
    if (g) g[e] = gg;
    if (wgt) wgt[e] = w;
}

// The row scaling, in place on J [npoints][n][m] with the inner residual R [npoints][m].  grid.x: workgroups over (point, row
// block) -- FLAT: ppw points each --, grid.y: groups of cpg columns.
template <bool FLAT>
static __global__ void __launch_bounds__(256)
k_loss_jac(LossArgs A, int m, int n, int nblk, int ppw, int cpg, int npoints, const double *__restrict__ R, double *J)
{
    int q, i;
    place_row<FLAT>(m, nblk, ppw, npoints, q, i);
    const bool on = q < npoints && i < m;
    const int qc = min(q, npoints - 1), ic = min(i, m - 1);
    const size_t ms = (size_t)m;
    const int j0 = blockIdx.y * cpg, j1 = min(j0 + cpg, n);
    if (j0 >= j1) return;
    double *Jq = J + ((size_t)qc * n + j0) * ms + ic;
    double out, g, wgt;
    loss_eval(A.kind, loss_scale_of(A, qc), R[(size_t)qc * ms + ic], out, g, wgt);
    int j = j0;
    for (; j + 4 <= j1; j += 4, Jq += 4 * ms) {
        const double v0 = Jq[0], v1 = Jq[ms], v2 = Jq[2 * ms], v3 = Jq[3 * ms];
        if (on) {
            Jq[0] = g * v0; Jq[ms] = g * v1; Jq[2 * ms] = g * v2; Jq[3 * ms] = g * v3;
        }
    }
    const int rem = j1 - j;                                       // 0 .. 3: loads first here too
    const double v0 = rem > 0 ? Jq[0] : 0.0, v1 = rem > 1 ? Jq[ms] : 0.0, v2 = rem > 2 ? Jq[2 * ms] : 0.0;
    if (on) {
        if (rem > 0) Jq[0] = g * v0;
        if (rem > 1) Jq[ms] = g * v1;
        if (rem > 2) Jq[2 * ms] = g * v2;
    }
}
