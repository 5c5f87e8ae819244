// nlh_kernels_boot_ci.h -- the kernels of the studentised and the BCa interval (include/nonlin_hip_boot_ci.h states the
// arithmetic; nlh_boot_ci.hip launches them), on nlh_kernels_boot.h's validity pass, ballot + prefix and launch style.  One
// IEEE operation per step; host and device share ppnd16 and the level arithmetic.
#pragma once
#include "nlh_kernels_boot.h"

__host__ __device__ __forceinline__ double boot_nan() { return (double)NAN; }
__host__ __device__ __forceinline__ bool boot_finite(double v) { return fabs(v) <= DBL_MAX; }

// Horner from the highest coefficient down: one multiplication and one addition per step
__host__ __device__ __forceinline__ double boot_horner8(const double *c, double r)
{
    double s = c[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) s = s * r + c[k];
    return s;
}

// Wichura's AS 241, PPND16.  p inside (0, 1); the central branch reaches no library function.
__host__ __device__ inline double boot_ppnd16(double p)
{
    const double A[8] = {2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                         1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0};
    const double B[8] = {5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                         5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0};
    const double Cc[8] = {7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
                          3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0};
    const double D[8] = {1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                         6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0};
    const double E[8] = {2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                         2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0};
    const double F[8] = {2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                         1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0};
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return (boot_horner8(A, r) * q) / boot_horner8(B, r);
    }
    double r = q <= 0.0 ? p : 1.0 - p;
    r = sqrt(-log(r));
    double z;
    if (r <= 5.0) {
        r = r - 1.6;
        z = boot_horner8(Cc, r) / boot_horner8(D, r);
    } else {
        r = r - 5.0;
        z = boot_horner8(E, r) / boot_horner8(F, r);
    }
    return q < 0.0 ? -z : z;
}

// The levels of `bca` for one pair with cnt > 0 and a finite xhat: z0, alpha[2] and the flag bits 1, 2, 4.
__host__ __device__ inline int boot_bca_levels(int c2, int cnt, double a, double qlo, double qhi, double zlo, double zhi, double *z0,
                                               double *alpha)
{
    int flag = 0;
    if (!boot_finite(a)) {
        flag |= NLH_BCA_NO_ACCEL;
        a = 0.0;
    }
    alpha[0] = qlo;
    alpha[1] = qhi;
    if (c2 == 0 || c2 == 2 * cnt) {
        *z0 = c2 == 0 ? -(double)INFINITY : (double)INFINITY;
        return flag | NLH_BCA_DEGENERATE;
    }
    const double u = (double)c2 / (double)(2 * cnt);
    const double z = boot_ppnd16(u);
    *z0 = z;
    const double zz[2] = {zlo, zhi};
    for (int t = 0; t < 2; ++t) {
        const double s = z + zz[t];
        const double den = 1.0 - a * s;
        if (!(den > 0.0)) {
            flag |= NLH_BCA_BAD_DENOM;
            continue;
        }
        const double w = z + s / den;
        alpha[t] = 0.5 * erfc(-(w * 0.70710678118654752));
    }
    return flag;
}

// summary's quantile of the sorted xc[0 .. cnt-1], cnt > 0, k kept inside 0 .. cnt-1
__device__ __forceinline__ double boot_quantile(const double *xc, int cnt, double q)
{
    const double h = q * (double)(cnt - 1);
    int k = (int)floor(h);
    k = k < 0 ? 0 : (k > cnt - 1 ? cnt - 1 : k);
    const double g = h - (double)k;
    const int k1 = k + 1 < cnt ? k + 1 : cnt - 1;
    return xc[k] + g * (xc[k1] - xc[k]);
}

// k_boot_summary's rank sort of xc[0 .. cnt-1] in LDS, in place: element e goes to the number of elements that are below it,
// or equal to it and before it -- stable, no padding --, every thread holding up to 16 elements in registers while all of
// them read the same x_f.  Every thread of the 256 calls this after a barrier that covers xc; it ends with one.
__device__ __forceinline__ void boot_rank_sort(double *xc, int cnt)
{
    const int tid = threadIdx.x;
    const int PER = NLH_BOOT_MAX_REP / 256;
    double v[PER];
    int below[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int e = tid + 256 * q;
        v[q] = e < cnt ? xc[e] : 0.0;
        below[q] = 0;
    }
    const int mine = (cnt - tid + 255) / 256;                        // how many elements this thread holds (<= 0: none)
    if (mine > 0)
        for (int f = 0; f < cnt; ++f) {
            const double xf = xc[f];
#pragma unroll
            for (int q = 0; q < PER; ++q) below[q] += (xf < v[q] || (xf == v[q] && f < tid + 256 * q)) ? 1 : 0;
        }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q)
        if (tid + 256 * q < cnt) xc[below[q]] = v[q];
    __syncthreads();
}

// One workgroup per (problem, parameter), as k_boot_summary.  A replica counts for this pair when k_boot_valid's byte is set
// AND its own standard error is finite and > 0: the two are combined at load, and the ballot + prefix runs on the result.
static __global__ void __launch_bounds__(256) k_boot_student(int nrep, int nprob, int n, const double *__restrict__ xs,
                                                       const double *__restrict__ sigs, const unsigned char *__restrict__ valid,
                                                       const double *__restrict__ x, const double *__restrict__ sigma, double qlo,
                                                       double qhi, double *__restrict__ lo, double *__restrict__ hi,
                                                       int32_t *__restrict__ nvalid_t)
{
    __shared__ double xc[NLH_BOOT_MAX_REP];
    __shared__ unsigned long long mask[NLH_BOOT_MAX_REP / 64];
    __shared__ int base[NLH_BOOT_MAX_REP / 64 + 1];
    const int tid = threadIdx.x;
    const int p = (int)(blockIdx.x / (unsigned)n), j = (int)(blockIdx.x - (unsigned)p * (unsigned)n);
    const size_t o = (size_t)p * n + j;
    const double xh = x[o], sg = sigma[o];
    const int cnt = boot_active(nrep, [&](int b) {
        if (!valid[(size_t)b * nprob + p]) return false;
        const double s = sigs[((size_t)b * nprob + p) * n + j];
        return s > 0.0 && s <= DBL_MAX;
    }, mask, base);
    for (int b = tid; b < nrep; b += 256)
        if (boot_is_active(b, mask)) {
            const size_t e = ((size_t)b * nprob + p) * n + j;
            xc[boot_rank(b, mask, base)] = (xs[e] - xh) / sigs[e];
        }
    __syncthreads();
    boot_rank_sort(xc, cnt);
    if (tid != 0) return;
    nvalid_t[o] = cnt;
    if (cnt == 0 || !boot_finite(xh) || !(sg > 0.0 && sg <= DBL_MAX)) {
        lo[o] = boot_nan();
        hi[o] = boot_nan();
        return;
    }
    const double tlo = boot_quantile(xc, cnt, qlo), thi = boot_quantile(xc, cnt, qhi);
    lo[o] = xh - thi * sg;
    hi[o] = xh - tlo * sg;
}

// One workgroup per (problem, parameter), as k_boot_summary.  c2 is counted before the sort, in integers: the ballots of
// `below xhat` and `equal to xhat` over the valid values, a popcount each.
static __global__ void __launch_bounds__(256) k_boot_bca(int nrep, int nprob, int n, const double *__restrict__ xs,
                                                   const unsigned char *__restrict__ valid, const double *__restrict__ x,
                                                   const double *__restrict__ accel, double qlo, double qhi, double zlo, double zhi,
                                                   double *__restrict__ lo, double *__restrict__ hi, double *__restrict__ z0,
                                                   double *__restrict__ alo, double *__restrict__ ahi, int32_t *__restrict__ flags,
                                                   int32_t *__restrict__ nvalid)
{
    __shared__ double xc[NLH_BOOT_MAX_REP];
    __shared__ unsigned long long mask[NLH_BOOT_MAX_REP / 64];
    __shared__ int base[NLH_BOOT_MAX_REP / 64 + 1];
    __shared__ int cw[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int p = (int)(blockIdx.x / (unsigned)n), j = (int)(blockIdx.x - (unsigned)p * (unsigned)n);
    const size_t o = (size_t)p * n + j;
    const double xh = x[o];
    const int cnt = boot_active(nrep, [&](int b) { return valid[(size_t)b * nprob + p] != 0; }, mask, base);
    for (int b = tid; b < nrep; b += 256)
        if (boot_is_active(b, mask)) xc[boot_rank(b, mask, base)] = xs[((size_t)b * nprob + p) * n + j];
    __syncthreads();
    int c = 0;
    for (int e0 = 0; e0 < cnt; e0 += 256) {                          // (the same trips for every thread: ballots inside)
        const int e = e0 + tid;
        const double v = e < cnt ? xc[e] : 0.0;
        c += 2 * __popcll(__ballot(e < cnt && v < xh)) + __popcll(__ballot(e < cnt && v == xh));
    }
    if (lane == 0) cw[tid >> 6] = c;
    __syncthreads();                                                 // (boot_rank_sort starts by reading xc only)
    boot_rank_sort(xc, cnt);
    if (tid != 0) return;
    if (j == 0) nvalid[p] = cnt;
    if (cnt == 0 || !boot_finite(xh)) {
        lo[o] = boot_nan();
        hi[o] = boot_nan();
        z0[o] = boot_nan();
        alo[o] = boot_nan();
        ahi[o] = boot_nan();
        flags[o] = NLH_BCA_NO_REPLICA;
        return;
    }
    double z, alpha[2];
    flags[o] = boot_bca_levels(cw[0] + cw[1] + cw[2] + cw[3], cnt, accel[o], qlo, qhi, zlo, zhi, &z, alpha);
    z0[o] = z;
    alo[o] = alpha[0];
    ahi[o] = alpha[1];
    lo[o] = boot_quantile(xc, cnt, alpha[0]);
    hi[o] = boot_quantile(xc, cnt, alpha[1]);
}

// ok [m][nprob] (a byte each): is deletion i of problem p valid -- row i active and every one of the n refitted parameters
// finite: once per (p, i), so that the n waves of a problem do not each test the row again
static __global__ void __launch_bounds__(256) k_boot_jack_valid(size_t total, int m, int nprob, int n, const double *__restrict__ xjack,
                                                          const double *__restrict__ w, unsigned char *__restrict__ ok)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const size_t i = e / (size_t)nprob, p = e - i * (size_t)nprob;
    const double *__restrict__ x = xjack + e * (size_t)n;
    bool good = !w || w[p * (size_t)m + i] != 0.0;
    for (int j = 0; j < n; ++j) good = good && fabs(x[j]) <= DBL_MAX;
    ok[e] = good ? 1 : 0;
}

// One wave per (problem, parameter), four of them in a workgroup: lane l takes the deletions i = l (mod 64) in ascending i --
// the partials of the stated sum --, and wave_reduce_sum is its tree.  Three passes over the column: the count and the sum,
// then S2 and S3 together.
static __global__ void __launch_bounds__(256) k_boot_accel(int m, int nprob, int n, const double *__restrict__ xjack,
                                                     const unsigned char *__restrict__ ok, double *__restrict__ accel,
                                                     int32_t *__restrict__ njack)
{
    const int lane = threadIdx.x & 63;
    const size_t o = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= (size_t)nprob * n) return;                              // (a whole wave leaves together)
    const int p = (int)(o / (size_t)n), j = (int)(o - (size_t)p * n);
    const size_t stride = (size_t)nprob * n;
    const double *__restrict__ col = xjack + (size_t)p * n + j;
    const unsigned char *__restrict__ okp = ok + p;
    int c = 0;
    double s = 0.0;
    for (int i = lane; i < m; i += 64)
        if (okp[(size_t)i * nprob]) {
            s = s + col[(size_t)i * stride];
            ++c;
        }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    c = __shfl(c, 0, 64);
    s = wave_reduce_sum(s);
    if (lane == 0 && j == 0) njack[p] = c;
    if (c < 2) {
        if (lane == 0) accel[o] = 0.0;
        return;
    }
    const double mean = __shfl(s, 0, 64) / (double)c;
    double s2 = 0.0, s3 = 0.0;
    for (int i = lane; i < m; i += 64)
        if (okp[(size_t)i * nprob]) {
            const double d = mean - col[(size_t)i * stride];
            const double dd = d * d;
            s2 = s2 + dd;
            s3 = s3 + dd * d;
        }
    s2 = wave_reduce_sum(s2);
    s3 = wave_reduce_sum(s3);
    if (lane != 0) return;
    double a = 0.0;
    if (s2 != 0.0) {
        a = s3 / (6.0 * (s2 * __dsqrt_rn(s2)));
        if (!boot_finite(a)) a = 0.0;
    }
    accel[o] = a;
}

// A pure store stream: blockIdx.y = the deletion r, a thread one unit of V adjacent rows of the slab [nprob][m] (V = 2: one
// 16-byte store; the host gives V = 2 only for an even m and a 16-byte aligned output).
template <int V>
static __global__ void __launch_bounds__(256) k_boot_jackknife(int nprob, int m, int row0, const double *__restrict__ w,
                                                         double *__restrict__ wout)
{
    const unsigned per = (unsigned)(m / V);
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= (unsigned)nprob * per) return;
    const unsigned p = u / per, iu = u - p * per;
    const int del = row0 + (int)blockIdx.y;
    const size_t e = (size_t)p * m + (size_t)iu * V;
    double out[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        out[v] = w ? w[e + v] : 1.0;
        if ((int)(iu * V) + v == del) out[v] = 0.0;
    }
    double *dst = wout + (size_t)blockIdx.y * ((size_t)nprob * m) + e;
    if (V == 2) *reinterpret_cast<double2 *>(dst) = make_double2(out[0], out[V - 1]);
    else dst[0] = out[0];
}
