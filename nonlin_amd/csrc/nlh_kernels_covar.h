// nlh_kernels_covar.h -- MINPACK's covar on the pivoted R of lmfactor: cov = P (R^T R)^-1 P^T, batched over independent
// problems.  (nonlin v2.2.0 has no such routine; lss_solve modernises MINPACK's lmder, and covar is lmder's companion.)
//
// covar, 0-based, on the n x n upper triangle r (column-major, diagonal = rdiag), ipvt, tol:
//   tolr = tol |r(0,0)|;  l = number of leading k with |r(k,k)| > tolr (stops at the first failure);
//   1. the inverse of the leading l x l block, column by column:  r(k,k) = 1 / r(k,k);  for j < k ascending:
//      temp = r(k,k) r(j,k), r(j,k) = 0, r(i,k) = r(i,k) - temp r(i,j) for i <= j;
//   2. the upper triangle of R^-1 R^-T, k ascending:  r(i,j) = r(i,j) + r(j,k) r(i,k) for i <= j < k, then
//      r(i,k) = r(k,k) r(i,k) for i <= k;
//   3. cov(ipvt(i), ipvt(j)) = cov(ipvt(j), ipvt(i)) = r(i,j) (i <= j), 0 for the columns j >= l.
// Every element is a chain of separate multiplies and adds in a fixed order (-ffp-contract=off, no fma), and that order
// survives parallelisation without a reduction across lanes:
//   inv(i,k) = ((0 - t_i inv(i,i)) - t_(i+1) inv(i,i+1)) - ... - t_(k-1) inv(i,k-1),  t_j = (1 / r(k,k)) r(j,k):
//              row i of the inverse needs row i's earlier columns and the original R only  -> a thread per row;
//   c(i,j)   = inv(j,j) inv(i,j) + inv(j,j+1) inv(i,j+1) + ... + inv(j,l-1) inv(i,l-1)      -> a thread per element.
// Forms (the same bits; tests/test_gpu_covar.py holds each to tests/covar_restatement.py):
//   k_covar_lane         a lane per problem, the loops above as written, on a lane-minor LDS window (element e of lane q
//                        at e * 64 + q: conflict-free), staged in and out with coalesced accesses; n <= CV_LANE_MAX;
//   k_covar_wg<.., false> a workgroup per problem (up to 32 columns: 64 / n problems per one-wave workgroup; one wave up
//                        to 64 rows, a wave per 64 rows above, at most 1024 threads), the inverse packed (upper triangle,
//                        element (i, j) at j (j + 1) / 2 + i: the rows of a column are consecutive) in LDS;
//   k_covar_wg<.., true>  the same with the packed inverse in a global-memory window of the handle: any n.
// No form writes outside cov / rank: an ipvt entry outside [0, n) (a caller's error) is skipped, not followed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CV_LANE_MAX 8
#define CV_AHEAD 8                  // steps of a chain whose operands are fetched before the chain runs them

// ---------------------------------------------------------------------------------------------------------------------
// lane per problem
// ---------------------------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(64)
k_covar_lane(int64_t nprob, int n, const double *__restrict__ R, const int32_t *__restrict__ ipvt, double tol,
             double *__restrict__ cov, int32_t *__restrict__ rank)
{
    extern __shared__ double cvw[];                              // [n n + n][64]: r, then wa
    const int lane = threadIdx.x, nn = n * n;
    const int64_t pb = (int64_t)blockIdx.x * 64;
    const int cnt = (int)(nprob - pb < 64 ? nprob - pb : 64);
    const double *Rb = R + (size_t)pb * nn;
    for (int e = lane; e < cnt * nn; e += 64) {
        const int q = e / nn, idx = e - q * nn;
        cvw[idx * 64 + q] = Rb[e];
    }
    __syncthreads();
    if (lane < cnt) {
#define CVR(i, j) cvw[((j) * n + (i)) * 64 + lane]
#define CVWA(j) cvw[(nn + (j)) * 64 + lane]
        const int32_t *ip = ipvt + (size_t)(pb + lane) * n;
        const double tolr = tol * fabs(CVR(0, 0));
        int l = 0;
        for (int k = 0; k < n; ++k) {
            if (fabs(CVR(k, k)) <= tolr) break;
            CVR(k, k) = 1.0 / CVR(k, k);
            for (int j = 0; j < k; ++j) {
                const double temp = CVR(k, k) * CVR(j, k);
                CVR(j, k) = 0.0;
                for (int i = 0; i <= j; ++i) CVR(i, k) = CVR(i, k) - temp * CVR(i, j);
            }
            l = k + 1;
        }
        for (int k = 0; k < l; ++k) {
            for (int j = 0; j < k; ++j) {
                const double temp = CVR(j, k);
                for (int i = 0; i <= j; ++i) CVR(i, j) = CVR(i, j) + temp * CVR(i, k);
            }
            const double temp = CVR(k, k);
            for (int i = 0; i <= k; ++i) CVR(i, k) = temp * CVR(i, k);
        }
        for (int j = 0; j < n; ++j) {                            // the strict lower triangle and wa receive the covariance
            const int jj = ip[j];
            const bool sing = j >= l;
            for (int i = 0; i <= j; ++i) {
                if (sing) CVR(i, j) = 0.0;
                const int ii = ip[i];
                if ((unsigned)ii >= (unsigned)n || (unsigned)jj >= (unsigned)n) continue;
                if (ii > jj) CVR(ii, jj) = CVR(i, j);
                if (ii < jj) CVR(jj, ii) = CVR(i, j);
            }
            if ((unsigned)jj < (unsigned)n) CVWA(jj) = CVR(j, j);
        }
        for (int j = 0; j < n; ++j) {
            for (int i = 0; i < j; ++i) CVR(i, j) = CVR(j, i);
            CVR(j, j) = CVWA(j);
        }
        rank[pb + lane] = l;
#undef CVR
#undef CVWA
    }
    __syncthreads();
    double *Cb = cov + (size_t)pb * nn;
    for (int e = lane; e < cnt * nn; e += 64) {
        const int q = e / nn, idx = e - q * nn;
        Cb[e] = cvw[idx * 64 + q];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// workgroup per problem (GROUPED: G problems per one-wave workgroup, TP = n threads each)
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t cv_at(int i, int j) { return (size_t)j * (size_t)(j + 1) / 2 + (size_t)i; }

template <bool GROUPED, bool GLOBAL>
static __global__ void __launch_bounds__(1024)
k_covar_wg(int64_t p0, int64_t nprob, int n, int G, int TP, const double *__restrict__ R, const int32_t *__restrict__ ipvt,
           double tol, double *__restrict__ cov, int32_t *__restrict__ rank, double *__restrict__ W, size_t wstride)
{
    extern __shared__ double cvl[];
    const int g = GROUPED ? (int)threadIdx.x / TP : 0;
    const int t = GROUPED ? (int)threadIdx.x - g * TP : (int)threadIdx.x;
    const int64_t slot = GROUPED ? (int64_t)blockIdx.x * G + g : (int64_t)blockIdx.x;
    const int64_t p = p0 + slot;
    const bool live = (!GROUPED || g < G) && p < nprob;
    const size_t tri = cv_at(0, n);
    double *inv = GLOBAL ? W + (size_t)slot * wstride : cvl + (size_t)g * tri;
    const double *Rp = R + (size_t)(live ? p : 0) * n * n;
    const int32_t *ip = ipvt + (size_t)(live ? p : 0) * n;
    int l = 0;
    if (live) {
        const double tolr = tol * fabs(Rp[0]);
        for (int k = 0; k < n; ++k) {
            if (fabs(Rp[(size_t)k * n + k]) <= tolr) break;
            l = k + 1;
        }
        // the inverse: this thread's rows, TP rows of the workgroup at a time; (k, j) run the same for every row of a
        // chunk (t_j comes from one address), a row joins its chain at j = i
        // Loads are issued unconditionally, eight steps at a time, ahead of the chain that uses them: a row that has not
        // joined yet (j < i) reads an in-range element it then ignores (il: the row index kept inside the triangle).
        for (int c0 = 0; c0 < l; c0 += TP) {
            const int i = c0 + t, il = i < n ? i : n - 1;
            for (int k = c0; k < l; ++k) {
                const double *rk = Rp + (size_t)k * n;
                const double d = 1.0 / rk[k];
                double acc = 0.0;
                int j = c0;
                for (; j + CV_AHEAD <= k; j += CV_AHEAD) {
                    double r[CV_AHEAD], v[CV_AHEAD];
#pragma unroll
                    for (int u = 0; u < CV_AHEAD; ++u) { r[u] = rk[j + u]; v[u] = inv[cv_at(il, j + u)]; }
#pragma unroll
                    for (int u = 0; u < CV_AHEAD; ++u) {
                        const double tj = d * r[u];
                        if (j + u >= i) acc = acc - tj * v[u];
                    }
                }
                for (; j < k; ++j) {
                    const double tj = d * rk[j], v = inv[cv_at(il, j)];
                    if (j >= i) acc = acc - tj * v;
                }
                if (i < k) inv[cv_at(i, k)] = acc;
                else if (i == k) inv[cv_at(k, k)] = d;
            }
        }
    }
    __syncthreads();                                             // (global window: a workgroup's own writes, visible after the barrier)
    if (!live) return;
    if (t == 0) rank[p] = l;
    double *Cp = cov + (size_t)p * n * n;
    // the product and the scatter: element e = j (j + 1) / 2 + i of the upper triangle, TP elements at a time
    int j = 0, i = t;
    while (i > j) { i -= j + 1; ++j; }
    while (j < n) {
        double c = 0.0;
        if (j < l) {
            c = inv[cv_at(j, j)] * inv[cv_at(i, j)];
            int k = j + 1;
            for (; k + CV_AHEAD <= l; k += CV_AHEAD) {
                double a[CV_AHEAD], b[CV_AHEAD];
#pragma unroll
                for (int u = 0; u < CV_AHEAD; ++u) { a[u] = inv[cv_at(j, k + u)]; b[u] = inv[cv_at(i, k + u)]; }
#pragma unroll
                for (int u = 0; u < CV_AHEAD; ++u) c = c + a[u] * b[u];
            }
            for (; k < l; ++k) c = c + inv[cv_at(j, k)] * inv[cv_at(i, k)];
        }
        const int ii = ip[i], jj = ip[j];
        if ((unsigned)ii < (unsigned)n && (unsigned)jj < (unsigned)n) {
            Cp[(size_t)ii * n + jj] = c;
            Cp[(size_t)jj * n + ii] = c;
        }
        i += TP;
        while (j < n && i > j) { i -= j + 1; ++j; }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// what nlh_lm_covariance* adds: the reduced chi-square, the scaling, the standard errors
// ---------------------------------------------------------------------------------------------------------------------
// chi2[p] = (sum of f_i^2, i ascending, one thread's plain sum) / (m - n)
static __global__ void __launch_bounds__(64)
k_covar_chi2(int nprob, int m, int n, const double *__restrict__ f, double *__restrict__ chi2)
{
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= nprob) return;
    const double *fp = f + (size_t)p * m;
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = s + fp[i] * fp[i];
    chi2[p] = s / (double)(m - n);
}

// cov = cov * chi2 (chi2 != nullptr), sigma_i = sqrt(cov(i,i)) (sigma != nullptr)
static __global__ void __launch_bounds__(256)
k_covar_scale(size_t total, int n, double *__restrict__ cov, const double *__restrict__ chi2, double *__restrict__ sigma)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const size_t nn = (size_t)n * n, p = e / nn, idx = e - p * nn;
    double v = cov[e];
    if (chi2) { v = v * chi2[p]; cov[e] = v; }
    const size_t r = idx / n, c = idx - r * n;
    if (sigma && r == c) sigma[p * n + r] = sqrt(v);
}
