// nlh_kernels_fit.h -- the two small kernels of the fit + errors pipeline (nlh_fit.hip), a thread per problem: the rows that
// count as degrees of freedom, and what a one-call fit does to the covariance chain's output.
#pragma once
#include "nlh_internal.h"

// rows with w != 0 of every problem (the degrees of freedom of a fit on zero-padded data are that count minus n)
static __global__ void __launch_bounds__(64)
k_fit_count(int nprob, int m, const double *__restrict__ w, int32_t *__restrict__ cnt)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= nprob) return;
    int c = 0;
    for (int i = 0; i < m; ++i) c += w[(size_t)p * m + i] != 0.0;
    cnt[p] = c;
}

// What a one-call fit does after the covariance chain: a problem that did not solve gets NaN and rank -1; with weights,
// chi2 = (sum of f_i^2, i ascending, sequential) / dof and every entry of cov is multiplied once by (m - n) / dof before
// sigma_i = sqrt(cov(i,i)) is taken.  unscaled (a Poisson fit, whose covariance carries no chi2): chi2 as above, cov and sigma
// as they are.  Any of cov, sigma, chi2, rank may be null.
static __global__ void __launch_bounds__(64)
k_fit_post(int nprob, int m, int n, const int32_t *__restrict__ status, const int32_t *__restrict__ nz, const double *__restrict__ f,
           double *__restrict__ cov, double *__restrict__ sigma, double *__restrict__ chi2, int32_t *__restrict__ rank, int unscaled)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= nprob) return;
    const size_t nn = (size_t)n * n;
    if (status[p] != 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        if (cov) for (size_t e = 0; e < nn; ++e) cov[p * nn + e] = nan;
        if (sigma) for (int j = 0; j < n; ++j) sigma[(size_t)p * n + j] = nan;
        if (chi2) chi2[p] = nan;
        if (rank) rank[p] = -1;
        return;
    }
    if (!nz) return;
    const double dof = (double)(nz[p] - n);
    if (chi2) {
        const double *fp = f + (size_t)p * m;
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = s + fp[i] * fp[i];
        chi2[p] = s / dof;
    }
    if (unscaled) return;
    const double scale = (double)(m - n) / dof;
    if (cov)
        for (size_t e = 0; e < nn; ++e) {
            const double v = cov[p * nn + e] * scale;
            cov[p * nn + e] = v;
            if (sigma && e / n == e % n) sigma[(size_t)p * n + e / n] = sqrt(v);
        }
}
