// nlh_kernels_pois.h -- Poisson likelihood fits (include/nonlin_hip.h: nlh_pois_*): the kernels behind the wrapping launchers
// nlh_pois_device_fcn / nlh_pois_device_jac and nlh_pois_apply_batch.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off).  r the inner residual model - y of
// an UNWEIGHTED inner model, y the count of the row, w its mask entry (when a mask is given), f = mu_floor:
//   f not finite or not positive                                       out = g = NaN, every row
//   masked (w == 0.0)                                                  out = +0.0, g = 0.0; the Jacobian row is stored as +0.0
//   w neither 0.0 nor 1.0, y < 0.0 or y not finite                     out = g = NaN
//   mu = r + y; low = mu < f; rr = low ? f - y : r
//   y == 0.0    D = 2.0*rr; s = sqrt(D); d = s; g = 1.0/s
//   y >  0.0    e = rr/y; a = fabs(e); t = rr + y; u = t/y
//               a <= 2^-6:  q = 1.0/13; then for k = 12 .. 2: q = e*q; q = 1.0/k - q;  z = e*e; h = z*q
//               else:       l = (e < -0.5) ? log(u) : log1p(e); h = e - l
//               D = 2.0*y; D = D*h; s = sqrt(D); d = copysign(s, e)
//               g = (e == 0.0) ? 1.0/sqrt(y) : a/(u*s)
//   low: v = mu - f; v = g*v; out = d + v      else: out = d
// J'[i][j] = g_i * J[i][j]: one multiply per entry; no sum crosses a row, so the value of a row does not depend on the launch
// shape it is computed in.  D is the row's deviance 2 [mu - y + y log(y / mu)] at max(mu, f); sum out^2 is -2 log L up to a
// constant of the data, and below the floor out continues d linearly with its slope there (C1).
//
// k_pois_jac is the one that moves bytes: 8 m (2 n + 3) per point (r, y, w and the n columns in, the n columns out), nothing
// reused.  Its shape is k_loss_jac's: a thread per (point, row), column-major, in the two workgroup forms, the columns
// optionally split over gridDim.y.  A thread forms g once -- the branches of the table diverge per lane, once per n columns --
// and the column loop has one factor and one select: four loads issued before the first store, unconditionally on a clamped
// (point, row).
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

struct PoisArgs {
    const double *y;                   // [nprob][m] counts
    const double *w;                   // [nprob][m] mask of 0.0 / 1.0, or null
    const int32_t *dprob;              // point q reads row dprob[q] of y and w; null: row q
    double mu_floor;
};

// out, g, D of one row (the table above); returns whether the row is masked
static __device__ __forceinline__ bool pois_eval(double f, bool has_w, double w, double y, double r, double &out, double &g, double &D)
{
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (!(f > 0.0) || f > DBL_MAX) { out = g = D = nan; return false; }
    if (has_w && w == 0.0) { out = 0.0; g = 0.0; D = 0.0; return true; }
    if ((has_w && w != 1.0) || !(y >= 0.0) || y > DBL_MAX) { out = g = D = nan; return false; }
    const double mu = r + y;
    const bool low = mu < f;
    const double rr = low ? f - y : r;
    double d;
    if (y == 0.0) {
        D = 2.0 * rr;
        const double s = sqrt(D);
        d = s;
        g = 1.0 / s;
    } else {
        const double e = rr / y;
        const double a = fabs(e);
        const double t = rr + y;
        const double u = t / y;
        double h;
        if (a <= 0.015625) {
            double q = 1.0 / 13;
            q = e * q; q = 1.0 / 12 - q;
            q = e * q; q = 1.0 / 11 - q;
            q = e * q; q = 1.0 / 10 - q;
            q = e * q; q = 1.0 / 9 - q;
            q = e * q; q = 1.0 / 8 - q;
            q = e * q; q = 1.0 / 7 - q;
            q = e * q; q = 1.0 / 6 - q;
            q = e * q; q = 1.0 / 5 - q;
            q = e * q; q = 1.0 / 4 - q;
            q = e * q; q = 1.0 / 3 - q;
            q = e * q; q = 1.0 / 2 - q;
            const double z = e * e;
            h = z * q;
        } else {
            const double l = (e < -0.5) ? log(u) : log1p(e);
            h = e - l;
        }
        D = 2.0 * y;
        D = D * h;
        const double s = sqrt(D);
        d = copysign(s, e);
        if (e == 0.0) g = 1.0 / sqrt(y);
        else { const double us = u * s; g = a / us; }
    }
    out = d;
    if (low) {
        double v = mu - f;
        v = g * v;
        out = d + v;
    }
    return false;
}

static __device__ __forceinline__ bool pois_row(const PoisArgs &A, int q, int i, int m, double r, double &out, double &g, double &D)
{
    const size_t at = (size_t)(A.dprob ? A.dprob[q] : q) * m + i;
    return pois_eval(A.mu_floor, A.w != nullptr, A.w ? A.w[at] : 1.0, A.y[at], r, out, g, D);
}

// in place on the inner launcher's F [npoints][m]: a thread per (point, row)
static __global__ void __launch_bounds__(256) k_pois_fcn(PoisArgs A, int m, int npoints, double *__restrict__ F)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)npoints * m) return;
    const int q = (int)(e / m);
    double out, g, D;
    pois_row(A, q, (int)(e - (size_t)q * m), m, F[e], out, g, D);
    F[e] = out;
}

// nlh_pois_apply_batch: a thread per (problem, row); every output may be null, out may be r itself
static __global__ void __launch_bounds__(256)
k_pois_apply(PoisArgs A, int m, int nprob, const double *r, double *out, double *__restrict__ g, double *__restrict__ dev)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nprob * m) return;
    const int p = (int)(e / m);
    double o, gg, D;
    pois_row(A, p, (int)(e - (size_t)p * m), m, r[e], o, gg, D);
    if (out) out[e] = o;
    if (g) g[e] = gg;
    if (dev) dev[e] = D;
}

// The row scaling, in place on J [npoints][n][m] with the inner residual R [npoints][m].  grid.x: workgroups over (point, row
// block) -- FLAT: ppw points each --, grid.y: groups of cpg columns.
template <bool FLAT>
static __global__ void __launch_bounds__(256)
k_pois_jac(PoisArgs A, int m, int n, int nblk, int ppw, int cpg, int npoints, const double *__restrict__ R, double *J)
{
    int q, i;
    place_row<FLAT>(m, nblk, ppw, npoints, q, i);
    const bool on = q < npoints && i < m;
    const int qc = min(q, npoints - 1), ic = min(i, m - 1);
    const size_t ms = (size_t)m;
    const int j0 = blockIdx.y * cpg, j1 = min(j0 + cpg, n);
    if (j0 >= j1) return;
    double *Jq = J + ((size_t)qc * n + j0) * ms + ic;
    double out, g, D;
    const bool z = pois_row(A, qc, ic, m, R[(size_t)qc * ms + ic], out, g, D);   // masked: zeros are stored, nothing is multiplied
    int j = j0;
    for (; j + 4 <= j1; j += 4, Jq += 4 * ms) {
        const double v0 = Jq[0], v1 = Jq[ms], v2 = Jq[2 * ms], v3 = Jq[3 * ms];
        if (on) {
            Jq[0] = z ? 0.0 : g * v0; Jq[ms] = z ? 0.0 : g * v1; Jq[2 * ms] = z ? 0.0 : g * v2; Jq[3 * ms] = z ? 0.0 : g * v3;
        }
    }
    const int rem = j1 - j;                                       // 0 .. 3: loads first here too
    const double v0 = rem > 0 ? Jq[0] : 0.0, v1 = rem > 1 ? Jq[ms] : 0.0, v2 = rem > 2 ? Jq[2 * ms] : 0.0;
    if (on) {
        if (rem > 0) Jq[0] = z ? 0.0 : g * v0;
        if (rem > 1) Jq[ms] = z ? 0.0 : g * v1;
        if (rem > 2) Jq[2 * ms] = z ? 0.0 : g * v2;
    }
}
