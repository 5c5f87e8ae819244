// nlh_kernels_guess.h -- starting values for the built-in curve models (include/nonlin_hip_guess.h: nlh_curve_guess_batch): the
// kernels of the nonlinear stage -- mu and width of each peak, k of each decay.  The linear stage is nlh_sep_solve_batch.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off); the header states it, and
// tests/guess_restatement.py restates it in numpy.  One workgroup of 256 threads per problem.  The valid rows (w != 0) are
// compacted into LDS once; every floating-point sum is a per-row one a single thread forms in ascending order (the means of
// the detrend, a row's smoothing window, a chunk of the prefix sum, the chunk totals), and what crosses threads is exact in any
// order: an argmax (value, then lowest index), a lowest and a highest index.  So the bits do not depend on the launch.
//   peaks   LDS: t' [m], s [m] (y', then d, then s, in place: a thread keeps the smoothed values of its rows in registers
//           across the barrier) and the dead mask [m bytes]: 2 * 8 m + m bytes, 139,264 at m = 8192.  The peel loop re-reads s
//           K times from LDS, never from global memory.
//   decays  LDS: t' [m], y' [m] (then S1 in place).  The panel [S1 (S2) u^0 .. u^deg | f0 = -y'] goes to global memory in the
//           layout k_sep_solve reads (column-major per problem, ld = m, rows >= mv +0.0), k_sep_solve factors and solves it
//           -- there is no second QR --, and k_guess_rates turns the coefficients into rates.
// A thread owns the rows tid (mod 256) of the element-wise steps and chunk tid of the prefix sum.
#pragma once
#include "nlh_internal.h"

static const int GUESS_RPT = NLH_GUESS_MAX_M / 256;     // rows a thread owns at most

struct GuessData {
    int K, B, shared_t, m, n, smooth;
    const double *t, *y, *w;           // w may be null
};

__device__ __forceinline__ double guess_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ bool guess_finite(double v) { return fabs(v) <= DBL_MAX; }

// The valid rows of problem p, ascending, into tv and yv; returns their number mv, and in *bad whether the problem is not
// guessed (mv < n, a value that is not finite, t' not strictly ascending).  cnt: 257 ints of LDS.  Ends on a barrier.
__device__ static int guess_compact(const GuessData &gd, int p, double *tv, double *yv, int *cnt, int *bad)
{
    const int tid = threadIdx.x, m = gd.m;
    const double *t = gd.t + (gd.shared_t ? (size_t)0 : (size_t)p * m);
    const double *y = gd.y + (size_t)p * m;
    int mv = m;
    if (!gd.w) {
        for (int i = tid; i < m; i += 256) { tv[i] = t[i]; yv[i] = y[i]; }
    } else {
        const double *w = gd.w + (size_t)p * m;
        const int c = (m + 255) / 256, lo = min(tid * c, m), hi = min(lo + c, m);
        int k = 0;
        for (int i = lo; i < hi; ++i) k += w[i] != 0.0 ? 1 : 0;
        cnt[tid + 1] = k;
        __syncthreads();
        if (tid == 0) {
            cnt[0] = 0;
            for (int j = 1; j <= 256; ++j) cnt[j] += cnt[j - 1];
        }
        __syncthreads();
        int at = cnt[tid];
        for (int i = lo; i < hi; ++i)
            if (w[i] != 0.0) { tv[at] = t[i]; yv[at] = y[i]; ++at; }
        mv = cnt[256];
    }
    __syncthreads();
    int b = mv < gd.n ? 1 : 0;
    for (int i = tid; i < mv; i += 256) {
        const double a = tv[i];
        if (!guess_finite(a) || !guess_finite(yv[i])) b = 1;
        if (i > 0 && !(a > tv[i - 1])) b = 1;
    }
    *bad = __syncthreads_or(b);
    return mv;
}

// The peaks of one problem: alpha [nprob][2 K] = (mu_0, width_0, mu_1, ..), flag [nprob].
template <int KIND>
static __global__ void __launch_bounds__(256)
k_guess_peaks(GuessData gd, double *__restrict__ alpha, int32_t *__restrict__ flag)
{
    extern __shared__ double guess_lds[];
    __shared__ int cnt[257];
    __shared__ double rv[4], mean[4], c_mu, c_F;
    __shared__ int ri[4], jr, jl;
    const int m = gd.m, p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    double *tv = guess_lds, *sv = guess_lds + m;
    unsigned char *dead = (unsigned char *)(guess_lds + 2 * (size_t)m);
    double *ap = alpha + (size_t)p * 2 * gd.K;
    int bad;
    const int mv = guess_compact(gd, p, tv, sv, cnt, &bad);
    if (bad) {
        for (int k = tid; k < 2 * gd.K; k += 256) ap[k] = guess_nan();
        if (tid == 0) flag[p] = NLH_GUESS_NONE;
        return;
    }
    // detrend
    if (gd.B >= 0) {
        const int E = max(1, mv / 16);
        if (tid < 4) {                                              // yl, yr, tl, tr
            const double *a = (tid & 2) ? tv : sv;
            const int o = (tid & 1) ? mv - E : 0;
            double s = 0.0;
            for (int i = 0; i < E; ++i) s = s + a[o + i];
            mean[tid] = s / (double)E;
        }
        __syncthreads();
        const double yl = mean[0], yr = mean[1], tl = mean[2], tr = mean[3];
        if (gd.B == 0) {
            const double off = 0.5 * (yl + yr);
            for (int i = tid; i < mv; i += 256) sv[i] = sv[i] - off;
        } else {
            const double c1 = (yr - yl) / (tr - tl);
            const double c0 = yl - c1 * tl;
            for (int i = tid; i < mv; i += 256) sv[i] = sv[i] - (c0 + c1 * tv[i]);
        }
        __syncthreads();
    }
    // smooth
    const int h = gd.smooth;
    if (h > 0) {
        double reg[GUESS_RPT];
#pragma unroll
        for (int k = 0; k < GUESS_RPT; ++k) {
            const int i = tid + 256 * k;
            reg[k] = 0.0;
            if (i < mv) {
                const int lo = max(0, i - h), hi = min(mv - 1, i + h);
                double s = 0.0;
                for (int j = lo; j <= hi; ++j) s = s + sv[j];
                reg[k] = s / (double)(hi - lo + 1);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < GUESS_RPT; ++k) {
            const int i = tid + 256 * k;
            if (i < mv) sv[i] = reg[k];
        }
    }
    for (int i = tid; i < mv; i += 256) dead[i] = 0;
    if (tid == 0) { jr = mv; jl = -1; }
    __syncthreads();
    const double span = tv[mv - 1] - tv[0];
    int fl = 0;                                                     // (thread 0's is the problem's)
    for (int k = 0; k < gd.K; ++k) {
        // argmax over the live rows: the value, then the lowest index
        double bv = -INFINITY;
        int bi = INT_MAX;
        for (int i = tid; i < mv; i += 256) {
            double v = sv[i];
            if (dead[i] || v != v) v = -INFINITY;
            if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double v2 = __shfl_down(bv, off, 64);
            const int i2 = __shfl_down(bi, off, 64);
            if (v2 > bv || (v2 == bv && i2 < bi)) { bv = v2; bi = i2; }
        }
        if (lane == 0) { rv[wid] = bv; ri[wid] = bi; }
        __syncthreads();
        bv = rv[0]; bi = ri[0];
        for (int w = 1; w < 4; ++w)
            if (rv[w] > bv || (rv[w] == bv && ri[w] < bi)) { bv = rv[w]; bi = ri[w]; }
        const int ist = bi;
        const double a = bv, half = 0.5 * a;
        // the crossings: the lowest row above and the highest row below that is dead or under half
        if (a > 0.0) {
            int up = mv, dn = -1;
            for (int i = tid; i < mv; i += 256)
                if (dead[i] || sv[i] < half) {
                    if (i > ist) up = min(up, i);
                    if (i < ist) dn = max(dn, i);
                }
            if (up < mv) atomicMin(&jr, up);
            if (dn >= 0) atomicMax(&jl, dn);
        }
        __syncthreads();
        if (tid == 0) {
            const double mu = tv[ist];
            double F = 0.0;
            bool ok = false;
            if (a > 0.0) {
                const bool hr = jr < mv && !dead[jr], hl = jl >= 0 && !dead[jl];
                double tR = 0.0, tL = 0.0;
                if (hr) tR = tv[jr - 1] + ((tv[jr] - tv[jr - 1]) * (sv[jr - 1] - half)) / (sv[jr - 1] - sv[jr]);
                if (hl) tL = tv[jl + 1] - ((tv[jl + 1] - tv[jl]) * (sv[jl + 1] - half)) / (sv[jl + 1] - sv[jl]);
                if (hr && hl) F = tR - tL;
                else if (hr) F = 2.0 * (tR - mu);
                else if (hl) F = 2.0 * (mu - tL);
                ok = (hr || hl) && F > 0.0 && F <= DBL_MAX;
            }
            if (!ok) { F = 0.5 * span; fl |= NLH_GUESS_FALLBACK; }
            c_mu = mu; c_F = F;
            ap[2 * k] = mu;
            ap[2 * k + 1] = KIND == NLH_CURVE_GAUSS ? F / 2.3548200450309493 : 0.5 * F;
            jr = mv; jl = -1;
        }
        __syncthreads();
        const double mu = c_mu, F = c_F;
        if (KIND == NLH_CURVE_GAUSS) {
            const double lim = 1.5 * F;
            for (int i = tid; i < mv; i += 256)
                if (fabs(tv[i] - mu) <= lim) dead[i] = 1;
        } else {
            const double wd = 0.5 * F;
            for (int i = tid; i < mv; i += 256) {
                const double dd = (tv[i] - mu) / wd;
                sv[i] = sv[i] - a / (1.0 + dd * dd);
                if (i == ist) dead[i] = 1;
            }
        }
        __syncthreads();
    }
    if (tid == 0) flag[p] = fl;
}

// The panel of one decay problem (p = p0 + blockIdx.x; JF, F0: the slice's, indexed by blockIdx.x): JF [L][m], F0 [m],
// L = 2 K + B + 1; span [nprob], flag [nprob].
static __global__ void __launch_bounds__(256)
k_guess_decay_panel(GuessData gd, int p0, double *__restrict__ JF, double *__restrict__ F0, double *__restrict__ span,
                    int32_t *__restrict__ flag)
{
    extern __shared__ double guess_lds[];
    __shared__ int cnt[257];
    __shared__ double tot[256], off[256];
    const int m = gd.m, q = blockIdx.x, p = p0 + q, tid = threadIdx.x, K = gd.K;
    const int L = 2 * K + gd.B + 1;
    const size_t ms = (size_t)m;
    double *tv = guess_lds, *yv = guess_lds + m;
    double *Jq = JF + (size_t)q * L * ms, *fq = F0 + (size_t)q * ms;
    int bad;
    const int mv = guess_compact(gd, p, tv, yv, cnt, &bad);
    if (bad) {                                                      // an all-zero panel: every column dead, nothing to wait for
        for (int i = tid; i < m; i += 256) {
            fq[i] = 0.0;
            for (int k = 0; k < L; ++k) Jq[(size_t)k * ms + i] = 0.0;
        }
        if (tid == 0) { flag[p] = NLH_GUESS_NONE; span[p] = 0.0; }
        return;
    }
    const double t0 = tv[0];
    for (int i = tid; i < m; i += 256) {
        const bool on = i < mv;
        fq[i] = on ? -yv[i] : 0.0;
        const double u = on ? tv[i] - t0 : 0.0;
        double pw = 1.0;
        for (int j = 0; j <= K + gd.B; ++j) {
            Jq[(size_t)(K + j) * ms + i] = on ? pw : 0.0;
            pw = pw * u;
        }
    }
    // S1 from y', then S2 from S1: trapezoids, a chunk per thread, the chunk totals in order
    const int c = (mv + 255) / 256, lo = min(tid * c, mv), hi = min(lo + c, mv);
    for (int pass = 0; pass < K; ++pass) {
        double reg[GUESS_RPT];
        double l = 0.0;
#pragma unroll
        for (int r = 0; r < GUESS_RPT; ++r) {
            const int i = lo + r;
            reg[r] = 0.0;
            if (i < hi) {
                const double qi = i == 0 ? 0.0 : (0.5 * (yv[i] + yv[i - 1])) * (tv[i] - tv[i - 1]);
                l = l + qi;
                reg[r] = l;
            }
        }
        tot[tid] = l;
        __syncthreads();                                            // (and every read of yv is done)
        if (tid == 0) {
            double o = 0.0;
            off[0] = 0.0;
            for (int j = 1; j < 256; ++j) { o = o + tot[j - 1]; off[j] = o; }
        }
        __syncthreads();
        const double o = off[tid];
        double *col = Jq + (size_t)pass * ms;
#pragma unroll
        for (int r = 0; r < GUESS_RPT; ++r) {
            const int i = lo + r;
            if (i < hi) { const double S = o + reg[r]; yv[i] = S; col[i] = S; }
        }
        for (int i = mv + tid; i < m; i += 256) col[i] = 0.0;
        __syncthreads();
    }
    if (tid == 0) { flag[p] = 0; span[p] = tv[mv - 1] - tv[0]; }
}

// A thread per problem of the slice: the rates from the regression's coefficients C [cnt][L] and its live columns.
static __global__ void __launch_bounds__(256)
k_guess_rates(int K, int L, int cnt, int p0, const double *__restrict__ C, const int32_t *__restrict__ rank,
              const double *__restrict__ span, double *__restrict__ alpha, int32_t *__restrict__ flag)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= cnt) return;
    const int p = p0 + q;
    double *ap = alpha + (size_t)p * K;
    if (flag[p] & NLH_GUESS_NONE) {
        for (int k = 0; k < K; ++k) ap[k] = guess_nan();
        return;
    }
    const double *c = C + (size_t)q * L;
    const double sp = span[p];
    double k1, k2 = 1.0;
    if (K == 1) k1 = -c[0];
    else {
        const double A = c[0], Bc = c[1];
        const double disc = A * A + 4.0 * Bc;
        const double r = sqrt(disc);
        k1 = 0.5 * (r - A);
        k2 = (-Bc) / k1;
    }
    if (!(rank[q] == L && k1 > 0.0 && k1 <= DBL_MAX && k2 > 0.0 && k2 <= DBL_MAX)) {
        k1 = K == 1 ? 2.0 / sp : 8.0 / sp;
        k2 = 1.0 / sp;
        flag[p] |= NLH_GUESS_FALLBACK;
    }
    ap[0] = k1;
    if (K == 2) ap[1] = k2;
}

// A thread per problem: NaN rows for the problems that were not guessed, the dead columns of the linear solve, the flags out.
static __global__ void __launch_bounds__(256)
k_guess_finish(int N, int L, int nprob, const int32_t *__restrict__ rank, const int32_t *__restrict__ fl, double *__restrict__ x,
               int32_t *__restrict__ flag)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nprob) return;
    int f = fl[p];
    if (f & NLH_GUESS_NONE) {
        f = NLH_GUESS_NONE;
        for (int k = 0; k < N; ++k) x[(size_t)p * N + k] = guess_nan();
    } else if (rank[p] < L) f |= NLH_GUESS_RANKDEF;
    if (flag) flag[p] = f;
}
