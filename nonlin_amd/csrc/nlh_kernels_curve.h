// nlh_kernels_curve.h -- the built-in curve models (include/nonlin_hip.h: nlh_curve_*): sums of K Gaussian or Lorentzian
// peaks, or of K exponential decays, on a polynomial baseline of degree B (-1: none), as residual and Jacobian kernels
// behind the launchers nlh_curve_device_fcn / nlh_curve_device_jac.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off, the device library's exp):
//   parameters  the K components in order, then c_0 .. c_B
//   gauss   (a, mu, sigma)  d = (t - mu) / sigma;  e = exp(-0.5 * (d * d));  term = a * e
//                           partials  e;  g = ((a * e) * d) / sigma;  g * d
//   lorentz (a, mu, w)      d = (t - mu) / w;  q = 1.0 + d * d;  term = a / q
//                           partials  1.0 / q;  g = ((2.0 * a) * d) / ((w * q) * q);  g * d
//   expdecay (a, k)         e = exp(-(k * t));  term = a * e
//                           partials  e;  -((a * t) * e)
//   model sum   s = 0;  s = s + term_k, k ascending
//   baseline    b = c_B;  b = b * t + c_j, j = B - 1 .. 0;  s = s + b        partials  p = 1;  column = p;  p = p * t, j ascending
//   residual    r = s - y;  r = w * r with weights;  every Jacobian entry is multiplied once by w with weights
// No sum crosses a row, so the value of a row does not depend on the launch shape it is computed in.
//
// Two workgroup forms, the same bits:
//   row   a workgroup per (point, block of 256 rows), the point's x staged once in LDS (n * 8 bytes) -- k_dqv_fcn's shape;
//   flat  short data (m <= 128): 256 / m points per workgroup, thread -> (point, row), their x in LDS -- a 64-row problem
//         would otherwise leave three quarters of every workgroup idle.
// A thread's loads of t, y, w are issued unconditionally (clamped index) ahead of the arithmetic; the Jacobian goes out
// column-major (ld = m): consecutive threads write consecutive rows of a column.
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

struct CurveData {                     // what the kernels read: nlh_curve_ctx without the kind
    int K, B, shared_t, m;
    const double *t, *y, *w;           // y, w may be null (model values: nlh_curve_eval_batch)
};

template <int KIND> struct CurveP { static const int value = KIND == NLH_CURVE_EXPDECAY ? 2 : 3; };

// model value at abscissa t for parameters x
template <int KIND>
__device__ static inline double curve_value(int K, int B, const double *x, double t)
{
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
        if (KIND == NLH_CURVE_GAUSS) {
            const double d = (t - x[3 * k + 1]) / x[3 * k + 2];
            const double e = exp(-0.5 * (d * d));
            s = s + x[3 * k] * e;
        } else if (KIND == NLH_CURVE_LORENTZ) {
            const double d = (t - x[3 * k + 1]) / x[3 * k + 2];
            const double q = 1.0 + d * d;
            s = s + x[3 * k] / q;
        } else {
            const double e = exp(-(x[2 * k + 1] * t));
            s = s + x[2 * k] * e;
        }
    }
    if (B >= 0) {
        const double *c = x + CurveP<KIND>::value * K;
        double b = c[B];
        for (int j = B - 1; j >= 0; --j) b = b * t + c[j];
        s = s + b;
    }
    return s;
}

template <int KIND, bool FLAT>
static __global__ void __launch_bounds__(256)
k_curve_fcn(CurveData cd, int n, int nblk, int ppw, int npoints, const int32_t *__restrict__ dprob, const double *__restrict__ X,
            double *__restrict__ F)
{
    extern __shared__ double xs[];
    int q, i;
    const double *xq;
    const bool on = place_staged<FLAT>(cd.m, n, nblk, ppw, npoints, X, xs, q, i, xq);
    const int qc = min(q, npoints - 1), ic = min(i, cd.m - 1);
    const int p = dprob ? dprob[qc] : qc;
    const size_t at = (size_t)p * cd.m + ic;
    const double t = cd.t[cd.shared_t ? (size_t)ic : at];
    const double y = cd.y ? cd.y[at] : 0.0;
    const double w = cd.w ? cd.w[at] : 1.0;
    if (!on) return;
    double r = curve_value<KIND>(cd.K, cd.B, xq, t);
    if (cd.y) r = r - y;
    if (cd.w) r = w * r;
    F[(size_t)q * cd.m + i] = r;
}

template <int KIND, bool FLAT>
static __global__ void __launch_bounds__(256)
k_curve_jac(CurveData cd, int n, int nblk, int ppw, int npoints, const int32_t *__restrict__ dprob, const double *__restrict__ X,
            double *__restrict__ J)
{
    extern __shared__ double xs[];
    int q, i;
    const double *xq;
    const bool on = place_staged<FLAT>(cd.m, n, nblk, ppw, npoints, X, xs, q, i, xq);
    const int qc = min(q, npoints - 1), ic = min(i, cd.m - 1);
    const int p = dprob ? dprob[qc] : qc;
    const size_t at = (size_t)p * cd.m + ic;
    const double t = cd.t[cd.shared_t ? (size_t)ic : at];
    const double w = cd.w ? cd.w[at] : 1.0;
    if (!on) return;
    const size_t m = (size_t)cd.m;
    const bool hw = cd.w != nullptr;
    double *Jq = J + (size_t)q * m * n + i;
    for (int k = 0; k < cd.K; ++k) {
        if (KIND == NLH_CURVE_GAUSS) {
            const double a = xq[3 * k], sg = xq[3 * k + 2];
            const double d = (t - xq[3 * k + 1]) / sg;
            const double e = exp(-0.5 * (d * d));
            const double g = ((a * e) * d) / sg;
            const double gd = g * d;
            Jq[(size_t)(3 * k) * m] = hw ? w * e : e;
            Jq[(size_t)(3 * k + 1) * m] = hw ? w * g : g;
            Jq[(size_t)(3 * k + 2) * m] = hw ? w * gd : gd;
        } else if (KIND == NLH_CURVE_LORENTZ) {
            const double a = xq[3 * k], wd = xq[3 * k + 2];
            const double d = (t - xq[3 * k + 1]) / wd;
            const double qq = 1.0 + d * d;
            const double da = 1.0 / qq;
            const double g = ((2.0 * a) * d) / ((wd * qq) * qq);
            const double gd = g * d;
            Jq[(size_t)(3 * k) * m] = hw ? w * da : da;
            Jq[(size_t)(3 * k + 1) * m] = hw ? w * g : g;
            Jq[(size_t)(3 * k + 2) * m] = hw ? w * gd : gd;
        } else {
            const double a = xq[2 * k];
            const double e = exp(-(xq[2 * k + 1] * t));
            const double dk = -((a * t) * e);
            Jq[(size_t)(2 * k) * m] = hw ? w * e : e;
            Jq[(size_t)(2 * k + 1) * m] = hw ? w * dk : dk;
        }
    }
    double pw = 1.0;
    double *Jb = Jq + (size_t)(CurveP<KIND>::value * cd.K) * m;
    for (int j = 0; j <= cd.B; ++j) {
        Jb[(size_t)j * m] = hw ? w * pw : pw;
        pw = pw * t;
    }
}
