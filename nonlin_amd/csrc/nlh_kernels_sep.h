// nlh_kernels_sep.h -- separable fits (include/nonlin_hip.h: nlh_sep_*): the kernels behind the wrapping launchers
// nlh_sep_device_fcn / nlh_sep_device_jac and nlh_sep_solve_batch.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off); the header states it, and
// tests/sep_restatement.py restates it in numpy.  In short, per point, on the m x (L + 1) panel [Phi | f0]:
//   sum       every sum over rows: 256 partials, partial j = +0.0, then s = s + a*b over rows i = j (mod 256) ascending; the
//             partials combine as block_reduce_sum does at 256 threads (shuffle tree inside each 64, then the four in order)
//   norm0_l   sqrt(sum of w_i*w_i over all rows) of column l before any reflector
//   column l at row position r (= live columns so far):  sigma = sum_{i>r} w_i*w_i;  norm = sqrt(w_r*w_r + sigma);
//             dead (skipped, no reflector, c_l = +0.0) when norm <= 2^-40 * norm0_l;  else beta = -copysign(norm, w_r),
//             v_i = w_i / (w_r - beta),  tau = (beta - w_r) / beta,  R_rr = beta
//   apply     to a column x:  s = x_r + sum_{i>r} v_i*x_i;  s = tau*s;  x_r = x_r - s;  x_i = x_i - s*v_i
//   solve     z = -(Q^T f0);  j descending over the live columns:  s = z_j;  s = s - R_jk*c_k, k ascending;  c_j = s / R_jj
//   project   a column of D: the live reflectors in order, the leading rank entries to +0.0, the reflectors in reverse
// A thread owns the rows i = tid (mod 256) of every column, whatever the form: the sums do not depend on where the panel
// lives (LDS: copied in once; global: the context's scratch, re-read through L2), on the slice or on the launch.
//
// One workgroup of 256 threads per point.  Every reflector costs one pass over the remaining columns: a thread forms its
// partial of every column, the four waves reduce them with shuffles, and ONE pair of barriers serves all the columns of a
// pass (red holds a value per wave and column).  Row r of a column is not rewritten in the solve kernel -- R lives in LDS --,
// so a pass has no write that another thread reads before the next pair of barriers.
#pragma once
#include "nlh_internal.h"

struct SepTables {                     // passed by value: nothing of a separable object lives in device memory
    int N, L, n;
    int32_t lin[NLH_SEP_MAX_L];        // ascending full indices of the linear parameters
};

// full index k -> its nonlinear number j >= 0, or -1 - l for linear parameter l
__device__ __forceinline__ int sep_slot(const SepTables &T, int k)
{
    int before = 0;
    for (int l = 0; l < T.L; ++l) {
        if (T.lin[l] == k) return -1 - l;
        if (T.lin[l] < k) ++before;
    }
    return k - before;
}

// nonlinear number j -> full index
__device__ __forceinline__ int sep_full(const SepTables &T, int j)
{
    int k = j;
    for (int l = 0; l < T.L; ++l)
        if (T.lin[l] <= k) ++k;
    return k;
}

// a thread per (point, full parameter): p = (c = +0.0, alpha)
static __global__ void __launch_bounds__(256)
k_sep_expand0(SepTables T, int npoints, const double *__restrict__ X, double *__restrict__ P)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)npoints * T.N) return;
    const int q = (int)(e / T.N), k = (int)(e - (size_t)q * T.N);
    const int s = sep_slot(T, k);
    P[e] = s >= 0 ? X[(size_t)q * T.n + s] : 0.0;
}

// a thread per (problem, full parameter): the nonlinear ones go to their slot of x
static __global__ void __launch_bounds__(256)
k_sep_gather(SepTables T, int nprob, const double *__restrict__ full, double *__restrict__ x)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nprob * T.N) return;
    const int p = (int)(e / T.N), k = (int)(e - (size_t)p * T.N);
    const int s = sep_slot(T, k);
    if (s >= 0) x[(size_t)p * T.n + s] = full[e];
}

static const int SEP_RW = NLH_SEP_MAX_L + 1;    // columns a pass can hold: the L of Phi and f0; or 32 of D

// The four wave sums of a column, in ascending order, from +0.0: what block_reduce_sum returns.
__device__ __forceinline__ double sep_red4(const double *red, int k)
{
    double r = 0.0;
    for (int w = 0; w < 4; ++w) r = r + red[w * SEP_RW + k];
    return r;
}

// Basis and solve of one point.  JF: the inner Jacobian at p0 = (0, alpha), [npoints][N][m]; its linear columns are Phi and,
// on exit with keep_v, hold the reflectors below their row positions.  F0 [npoints][m].  Out: PH [npoints][N] = (c, alpha),
// TAU [npoints][L] (+0.0: a dead column), rank [npoints] (may be null).
template <bool LDS>
static __global__ void __launch_bounds__(256)
k_sep_solve(SepTables T, int m, int keep_v, double *JF, double *F0, const double *__restrict__ X,
            double *__restrict__ PH, double *__restrict__ TAU, int32_t *__restrict__ rank)
{
    extern __shared__ double sep_panel[];
    __shared__ double red[4 * SEP_RW];
    __shared__ double Rm[NLH_SEP_MAX_L * SEP_RW];      // R and, in column L, Q^T f0: row position x column
    __shared__ double nrm0[NLH_SEP_MAX_L], ctau[NLH_SEP_MAX_L], chat[NLH_SEP_MAX_L];
    __shared__ int rpos[NLH_SEP_MAX_L];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int L = T.L;
    const size_t ms = (size_t)m;
    double *Jq = JF + (size_t)q * T.N * ms;
    double *fq = F0 + (size_t)q * ms;
    // column k of the panel: k < L a column of Phi, k = L f0 (global form: where the inner launchers left them, in scratch)
    auto col = [&](int k) -> double * {
        if constexpr (LDS) return sep_panel + (size_t)k * ms;
        else return k < L ? Jq + (size_t)T.lin[k] * ms : fq;
    };
    if constexpr (LDS) {
        for (int k = 0; k <= L; ++k) {
            const double *src = k < L ? Jq + (size_t)T.lin[k] * ms : fq;
            for (int i = tid; i < m; i += 256) sep_panel[(size_t)k * ms + i] = src[i];
        }
    }
    // the norms before any reflector
    for (int l = 0; l < L; ++l) {
        const double *w = col(l);
        double s = 0.0;
        for (int i = tid; i < m; i += 256) s = s + w[i] * w[i];
        s = wave_reduce_sum(s);
        if (lane == 0) red[wid * SEP_RW + l] = s;
    }
    __syncthreads();
    if (tid < L) nrm0[tid] = sqrt(sep_red4(red, tid));
    int r = 0;
    for (int l = 0; l < L; ++l) {
        double *w = col(l);
        double s = 0.0;
        for (int i = tid; i < m; i += 256)
            if (i > r) s = s + w[i] * w[i];
        s = wave_reduce_sum(s);
        __syncthreads();                                          // red's last readers are done; the panel's last writes are in
        if (lane == 0) red[wid * SEP_RW] = s;
        __syncthreads();
        const double sigma = sep_red4(red, 0);
        const double wr = w[r];
        const double norm = sqrt(wr * wr + sigma);
        if (norm <= 0x1p-40 * nrm0[l]) {                          // dead: uniform across the workgroup
            if (tid == 0) { ctau[l] = 0.0; rpos[l] = -1; }
            continue;
        }
        const double beta = -copysign(norm, wr);
        const double d = wr - beta;
        const double tau = (beta - wr) / beta;
        for (int i = tid; i < m; i += 256)
            if (i > r) w[i] = w[i] / d;
        if (tid == 0) { ctau[l] = tau; rpos[l] = r; Rm[r * SEP_RW + l] = beta; }
        // the pass over the remaining columns and f0: a thread reads v and x at its own rows only
        for (int k = l + 1; k <= L; ++k) {
            const double *x = col(k);
            double p = 0.0;
            for (int i = tid; i < m; i += 256)
                if (i > r) p = p + w[i] * x[i];
            p = wave_reduce_sum(p);
            if (k == l + 1) __syncthreads();                      // sigma's readers are done with red
            if (lane == 0) red[wid * SEP_RW + k] = p;
        }
        __syncthreads();
        for (int k = l + 1; k <= L; ++k) {
            double *x = col(k);
            double sk = x[r] + sep_red4(red, k);
            sk = tau * sk;
            for (int i = tid; i < m; i += 256)
                if (i > r) x[i] = x[i] - sk * w[i];
            if (tid == 0) Rm[r * SEP_RW + k] = x[r] - sk;         // row r itself stays as it was: nobody reads it again
        }
        ++r;
    }
    __syncthreads();
    if (tid == 0) {                                               // back-substitution on the live columns
        for (int j = L - 1; j >= 0; --j) {
            if (rpos[j] < 0) { chat[j] = 0.0; continue; }
            const int rj = rpos[j];
            double s = -Rm[rj * SEP_RW + L];
            for (int k = j + 1; k < L; ++k)
                if (rpos[k] >= 0) s = s - Rm[rj * SEP_RW + k] * chat[k];
            chat[j] = s / Rm[rj * SEP_RW + j];
        }
        if (rank) rank[q] = r;
    }
    __syncthreads();
    for (int k = tid; k < T.N; k += 256) {
        const int s = sep_slot(T, k);
        PH[(size_t)q * T.N + k] = s >= 0 ? X[(size_t)q * T.n + s] : chat[-1 - s];
    }
    if (tid < L) TAU[(size_t)q * L + tid] = ctau[tid];
    if constexpr (LDS) {
        if (keep_v)
            for (int k = 0; k < L; ++k) {
                double *dst = Jq + (size_t)T.lin[k] * ms;
                for (int i = tid; i < m; i += 256) dst[i] = sep_panel[(size_t)k * ms + i];
            }
    }
}

// One reflector on the cn columns X[k*m ..] of a pass: v its vector (rows > rp), the owner of row rp is thread rp.
__device__ __forceinline__ void sep_apply(const double *v, int rp, double tau, double *X, int cn, int m, double *red, double *xr)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const size_t ms = (size_t)m;
    __syncthreads();                                              // the last pass's writes are in; red and xr are free
    for (int k = 0; k < cn; ++k) {
        const double *x = X + (size_t)k * ms;
        double p = 0.0;
        for (int i = tid; i < m; i += 256)
            if (i > rp) p = p + v[i] * x[i];
        p = wave_reduce_sum(p);
        if (lane == 0) red[wid * SEP_RW + k] = p;
        if (tid == rp) xr[k] = x[rp];
    }
    __syncthreads();
    for (int k = 0; k < cn; ++k) {
        double *x = X + (size_t)k * ms;
        double s = xr[k] + sep_red4(red, k);
        s = tau * s;
        for (int i = tid; i < m; i += 256)
            if (i > rp) x[i] = x[i] - s * v[i];
        if (tid == rp) x[rp] = xr[k] - s;
    }
}

// Kaufman's projection of one point's nonlinear columns.  JV: as k_sep_solve left it (the reflectors in its linear columns),
// TAU [npoints][L]; JD: the inner Jacobian at (c, alpha), [npoints][N][m]; J: [npoints][n][m].  blockIdx.y: a group of cg <= 32
// columns.
template <bool LDS>
static __global__ void __launch_bounds__(256)
k_sep_project(SepTables T, int m, int cg, const double *__restrict__ JV, const double *__restrict__ TAU, const double *__restrict__ JD,
              double *J)
{
    extern __shared__ double sep_panel[];
    __shared__ double red[4 * SEP_RW], xr[SEP_RW], ctau[NLH_SEP_MAX_L];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int L = T.L;
    const size_t ms = (size_t)m;
    const int c0 = blockIdx.y * cg, cn = min(cg, T.n - c0);
    const double *Vq = JV + (size_t)q * T.N * ms;
    const double *Dq = JD + (size_t)q * T.N * ms;
    double *Oq = J + ((size_t)q * T.n + c0) * ms;
    double *X;
    if constexpr (LDS) X = sep_panel + (size_t)L * ms;
    else X = Oq;
    if (tid < L) ctau[tid] = TAU[(size_t)q * L + tid];
    if constexpr (LDS)
        for (int l = 0; l < L; ++l) {
            const double *src = Vq + (size_t)T.lin[l] * ms;
            for (int i = tid; i < m; i += 256) sep_panel[(size_t)l * ms + i] = src[i];
        }
    for (int k = 0; k < cn; ++k) {
        const double *src = Dq + (size_t)sep_full(T, c0 + k) * ms;
        for (int i = tid; i < m; i += 256) X[(size_t)k * ms + i] = src[i];
    }
    __syncthreads();
    auto vcol = [&](int l) -> const double * {
        if constexpr (LDS) return sep_panel + (size_t)l * ms;
        else return Vq + (size_t)T.lin[l] * ms;
    };
    int r = 0;
    for (int l = 0; l < L; ++l) {
        const double tau = ctau[l];
        if (tau == 0.0) continue;
        sep_apply(vcol(l), r, tau, X, cn, m, red, xr);
        ++r;
    }
    if (tid < r)                                                  // (a thread's own rows)
        for (int k = 0; k < cn; ++k) X[(size_t)k * ms + tid] = 0.0;
    for (int l = L - 1; l >= 0; --l) {
        const double tau = ctau[l];
        if (tau == 0.0) continue;
        --r;
        sep_apply(vcol(l), r, tau, X, cn, m, red, xr);
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int k = 0; k < cn; ++k)
            for (int i = tid; i < m; i += 256) Oq[(size_t)k * ms + i] = X[(size_t)k * ms + i];
    }
}
