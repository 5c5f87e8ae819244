// nlh_kernels_boot.h -- the kernels of the bootstrap (include/nonlin_hip_boot.h states the arithmetic; nlh_boot.hip launches
// them).  The generator is integer arithmetic mod 2^64; the floating-point steps are one IEEE operation each.
#pragma once
#include "nlh_common.h"

static const uint64_t BOOT_G = 0x9E3779B97F4A7C15ULL;
static const int BOOT_RPW = 64;                                     // the most replicas one workgroup writes: their keys' LDS

// the finaliser of splitmix64 (sm64_u's three lines), the key of a stream, a draw of it, an index below cnt
__host__ __device__ __forceinline__ uint64_t boot_mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t boot_key(uint64_t seed, uint64_t p, uint64_t b)
{
    return boot_mix(boot_mix(seed + BOOT_G * (p + 1)) + BOOT_G * (b + 1));
}
__host__ __device__ __forceinline__ uint64_t boot_draw(uint64_t key, uint64_t k) { return boot_mix(key + BOOT_G * (k + 1)); }
__host__ __device__ __forceinline__ uint32_t boot_index(uint64_t z, uint32_t cnt) { return (uint32_t)(((z >> 32) * (uint64_t)cnt) >> 32); }

// Which of `count` items are active, as the 64-bit words of a wave's ballots: word wd covers the items 64 wd .. 64 wd + 63,
// base[wd] = the active items before it, base[nwords] = all of them.  The active number of item i is then boot_rank(i).
// flag(i): is item i active.  Every thread of the 256 calls this; it ends with a barrier.
template <class Flag>
__device__ __forceinline__ int boot_active(int count, Flag flag, unsigned long long *mask, int *base)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwords = (count + 63) >> 6;
    for (int wd = wave; wd < nwords; wd += 4) {
        const int i = wd * 64 + lane;
        const unsigned long long b = __ballot(i < count && flag(i));
        if (lane == 0) mask[wd] = b;
    }
    __syncthreads();
    for (int t = threadIdx.x; t <= nwords; t += 256) {
        int s = 0;
        for (int u = 0; u < t; ++u) s += __popcll(mask[u]);
        base[t] = s;
    }
    __syncthreads();
    return base[nwords];
}
__device__ __forceinline__ bool boot_is_active(int i, const unsigned long long *mask) { return (mask[i >> 6] >> (i & 63)) & 1ull; }
__device__ __forceinline__ int boot_rank(int i, const unsigned long long *mask, const int *base)
{
    return base[i >> 6] + __popcll(mask[i >> 6] & ((1ull << (i & 63)) - 1ull));
}

// The replicas rep0 + r0 .. of problem blockIdx.x, r0 = blockIdx.y * rpw, at most rpw <= BOOT_RPW of them: one workgroup reads
// the problem's mu, y, w once, finds its active rows (ballot + prefix) and keeps what the replicas share in LDS -- the active
// residuals (residual: 8 cnt bytes) or the draw counts (pairs: an int per active row and concurrent replica) --; what is
// left is a stream of stores.  A thread owns V adjacent rows (V = 2: one 16-byte store; the host gives V = 2 only for an
// even m and 16-byte aligned outputs) of 256 >> tsh concurrent replicas: 1 << tsh threads span a problem's rows, so that a
// short problem fills the workgroup with several replicas.  A row's own values stay in registers across the replicas.
template <int KIND, int V>
static __global__ void __launch_bounds__(256) k_boot_resample(uint64_t seed, int nprob, long long prob0, int m, int rep0, int nrep, int rpw,
                                                        int tsh, const double *__restrict__ mu, const double *__restrict__ y,
                                                        const double *__restrict__ w, int centre, double *__restrict__ yout,
                                                        double *__restrict__ wout)
{
    extern __shared__ __align__(16) unsigned char boot_lds[];
    __shared__ unsigned long long mask[NLH_BOOT_MAX_ROWS / 64];
    __shared__ int base[NLH_BOOT_MAX_ROWS / 64 + 1];
    __shared__ uint64_t keys[BOOT_RPW];
    __shared__ double ebar;
    const int tid = threadIdx.x, lane = tid & 63;
    const int p = blockIdx.x, r0 = blockIdx.y * rpw, R = min(rpw, nrep - r0);
    const size_t row0 = (size_t)p * m;
    if (KIND != NLH_BOOT_PAIRS) mu += row0;
    y += row0;
    if (w) w += row0;
    const uint64_t pk = boot_mix(seed + BOOT_G * ((uint64_t)prob0 + (uint64_t)p + 1));
    if (tid < R) keys[tid] = boot_mix(pk + BOOT_G * ((uint64_t)rep0 + (uint64_t)(r0 + tid) + 1));
    const int cnt = boot_active(m, [&](int i) { return !w || w[i] != 0.0; }, mask, base);      // (the barrier covers keys)
    const int tpr = 1 << tsh, col = tid & (tpr - 1), slot = tid >> tsh, nslot = 256 >> tsh, mh = m / V;
    const size_t rstride = (size_t)nprob * m;                        // from one replica to the next
    double *const yo = yout + ((size_t)r0 * nprob + p) * m;
    double *const wo = KIND == NLH_BOOT_PAIRS ? wout + ((size_t)r0 * nprob + p) * m : nullptr;

    if (KIND == NLH_BOOT_RESIDUAL) {
        double *ec = reinterpret_cast<double *>(boot_lds);           // [cnt]: the residuals of the active rows, by active number
        for (int i = tid; i < m; i += 256)
            if (boot_is_active(i, mask)) {
                const double d = y[i] - mu[i];
                ec[boot_rank(i, mask, base)] = w ? w[i] * d : d;
            }
        __syncthreads();
        if (centre && cnt > 0) {
            if (tid < 64) {                                          // the cost's order: lane j the active rows i = j (mod 64)
                double s = 0.0;
                for (int i = lane; i < m; i += 64)
                    if (boot_is_active(i, mask)) s = s + ec[boot_rank(i, mask, base)];
                s = wave_reduce_sum(s);
                if (lane == 0) ebar = s / (double)cnt;
            }
            __syncthreads();
            const double eb = ebar;
            for (int a = tid; a < cnt; a += 256) ec[a] = ec[a] - eb;
            __syncthreads();
        }
        for (int u = col; u < mh; u += tpr) {
            double mi[V], yi[V], wi[V];
            uint64_t gk[V];
            bool act[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int i = u * V + v;
                mi[v] = mu[i];
                yi[v] = y[i];
                wi[v] = w ? w[i] : 1.0;
                act[v] = boot_is_active(i, mask);
                gk[v] = BOOT_G * ((uint64_t)boot_rank(i, mask, base) + 1);
            }
            for (int r = slot; r < R; r += nslot) {
                const uint64_t key = keys[r];
                double out[V];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    out[v] = yi[v];
                    if (act[v]) {
                        const double e = ec[boot_index(boot_mix(key + gk[v]), (uint32_t)cnt)];
                        out[v] = w ? mi[v] + e / wi[v] : mi[v] + e;
                    }
                }
                double *dst = yo + (size_t)r * rstride + (size_t)u * V;
                if (V == 2) *reinterpret_cast<double2 *>(dst) = make_double2(out[0], out[V - 1]);
                else dst[0] = out[0];
            }
        }
    } else if (KIND == NLH_BOOT_WILD) {
        for (int u = col; u < mh; u += tpr) {
            double plus[V], minus[V];
            uint64_t gk[V];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int i = u * V + v;
                const double d = y[i] - mu[i];
                const bool a = boot_is_active(i, mask);
                plus[v] = a ? mu[i] + d : y[i];
                minus[v] = a ? mu[i] - d : y[i];
                gk[v] = BOOT_G * ((uint64_t)i + 1);
            }
            for (int r = slot; r < R; r += nslot) {
                const uint64_t key = keys[r];
                double out[V];
#pragma unroll
                for (int v = 0; v < V; ++v) out[v] = (boot_mix(key + gk[v]) >> 63) ? minus[v] : plus[v];
                double *dst = yo + (size_t)r * rstride + (size_t)u * V;
                if (V == 2) *reinterpret_cast<double2 *>(dst) = make_double2(out[0], out[V - 1]);
                else dst[0] = out[0];
            }
        }
    } else {
        int *cs = reinterpret_cast<int *>(boot_lds) + (size_t)slot * m;      // [nslot][m]: this slot's counts, by active number
        for (int rb = 0; rb < R; rb += nslot) {                      // (the same trips for every thread: barriers inside)
            const int r = rb + slot;
            const bool on = r < R;
            for (int a = col; a < cnt; a += tpr) cs[a] = 0;
            __syncthreads();
            if (on) {
                const uint64_t key = keys[r];
                for (int k = col; k < cnt; k += tpr) atomicAdd(&cs[boot_index(boot_draw(key, (uint64_t)k), (uint32_t)cnt)], 1);
            }
            __syncthreads();
            if (on)
                for (int u = col; u < mh; u += tpr) {
                    double yv[V], wv[V];
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const int i = u * V + v;
                        yv[v] = y[i];
                        wv[v] = w ? w[i] : 1.0;
                        if (boot_is_active(i, mask)) {
                            const double s = __dsqrt_rn((double)cs[boot_rank(i, mask, base)]);
                            wv[v] = w ? wv[v] * s : s;
                        }
                    }
                    const size_t o = (size_t)r * rstride + (size_t)u * V;
                    if (V == 2) {
                        *reinterpret_cast<double2 *>(yo + o) = make_double2(yv[0], yv[V - 1]);
                        *reinterpret_cast<double2 *>(wo + o) = make_double2(wv[0], wv[V - 1]);
                    } else {
                        yo[o] = yv[0];
                        wo[o] = wv[0];
                    }
                }
            __syncthreads();
        }
    }
}

// ---- Poisson bootstrap (include/nonlin_hip_boot_pois.h states the arithmetic; host and device share these functions) ----
static const double BOOT_POIS_EPS = 0x1p-60;
// What a row's draws share: the mode, the weights below it, all weights, the ends of the two walks and r = 1/mu.  T > 0: an
// ordinary row; T == 0: a zero row (its draws are +0.0); T < 0: a row that copies y (inactive or bad).
struct boot_pois {
    double M, L, T, kmin, kmax, r;
};
__host__ __device__ __forceinline__ bool boot_pois_bad(double mu) { return !(mu >= 0.0 && mu <= (double)NLH_BOOT_POIS_MAX_MEAN); }
// mu: inside (0, NLH_BOOT_POIS_MAX_MEAN].  `!(q >= EPS)` is `q < EPS` for every number and also ends the loop on a NaN, which no
// such mu produces: q stays inside (0, 1].
__host__ __device__ __forceinline__ boot_pois boot_pois_setup(double mu)
{
    boot_pois s;
    const double M = floor(mu), r = 1.0 / mu;
    double L = 0.0, q = 1.0, nd = 0.0;
    for (double k = M; k >= 1.0; k = k - 1.0) {
        q = (q * k) * r;
        if (!(q >= BOOT_POIS_EPS)) break;
        L = L + q;
        nd = nd + 1.0;
    }
    double U = 1.0, nu = 0.0;
    q = 1.0;
    for (double k = M + 1.0;; k = k + 1.0) {
        q = (q * mu) / k;
        if (!(q >= BOOT_POIS_EPS)) break;
        U = U + q;
        nu = nu + 1.0;
    }
    s.M = M;
    s.L = L;
    s.T = L + U;
    s.kmin = M - nd;
    s.kmax = M + nu;
    s.r = r;
    return s;
}
// the draw of an ordinary row from z = boot_draw(key, row): k moves by one per step and stays inside [kmin, kmax]
__host__ __device__ __forceinline__ double boot_pois_draw(const boot_pois &s, double mu, uint64_t z)
{
    const double u = (double)(z >> 11) * 0x1p-53, t = u * s.T;
    double k, q, r;
    if (t < s.L) {
        r = s.L - t;
        k = s.M - 1.0;
        q = s.M * s.r;
        while (r > q && k > s.kmin) {
            r = r - q;
            q = (q * k) * s.r;
            k = k - 1.0;
        }
    } else {
        r = t - s.L;
        k = s.M;
        q = 1.0;
        while (r >= q && k < s.kmax) {
            r = r - q;
            k = k + 1.0;
            q = (q * mu) / k;
        }
    }
    return k;
}
// a row's setup by its class; a zero or copying row runs no loop
__host__ __device__ __forceinline__ boot_pois boot_pois_row(bool active, double mu)
{
    if (active && !boot_pois_bad(mu) && mu != 0.0) return boot_pois_setup(mu);
    boot_pois s = {0.0, 0.0, active && mu == 0.0 ? 0.0 : -1.0, 0.0, 0.0, 0.0};
    return s;
}

// k_boot_resample's skeleton for the Poisson replicas: one workgroup per (problem blockIdx.x, block blockIdx.y of at most rpw <=
// BOOT_RPW replicas), the replicas' keys in LDS, boot_active for the mask, a thread owning V adjacent rows (V = 2: one 16-byte
// store) of 256 >> tsh concurrent replicas.  A thread keeps its rows' setup in registers across its replicas.  Where a short
// problem fills the workgroup with several replica slots (256 >> tsh > 1, which implies m <= 256), the setup -- 18 sqrt(mu)
// steps against a draw's 0.8 sqrt(mu) -- is made ONCE per row, by thread i for row i, and handed to the slots through 48 m
// bytes of dynamic LDS; otherwise every row has one owner and LDS is not used for it.  The workgroups of blockIdx.y == 0 count
// their problem's bad rows.
// No input can make this kernel spin: boot_pois_setup runs only for a mu inside (0, 2^24], where its first loop ends at k = 1 at
// the latest and its second because q shrinks by mu/k <= (M+1)/(M+2) per step from the second step on (and a NaN would end
// it, too); the draws' walks move k by one per step inside [kmin, kmax].  The lanes of a wave walk different lengths: the
// draw of (seed, p, b, i) is the interface, so nothing is reordered to balance them.
template <int V>
static __global__ void __launch_bounds__(256) k_boot_poisson(uint64_t seed, int nprob, long long prob0, int m, int rep0, int nrep, int rpw,
                                                       int tsh, const double *__restrict__ mu, const double *__restrict__ y,
                                                       const double *__restrict__ w, double *__restrict__ yout, int32_t *__restrict__ bad)
{
    extern __shared__ __align__(16) unsigned char boot_lds[];
    __shared__ unsigned long long mask[NLH_BOOT_MAX_ROWS / 64];
    __shared__ int base[NLH_BOOT_MAX_ROWS / 64 + 1];
    __shared__ uint64_t keys[BOOT_RPW];
    __shared__ int nbad;
    const int tid = threadIdx.x;
    const int p = blockIdx.x, r0 = blockIdx.y * rpw, R = min(rpw, nrep - r0);
    const size_t row0 = (size_t)p * m;
    mu += row0;
    y += row0;
    if (w) w += row0;
    const uint64_t pk = boot_mix(seed + BOOT_G * ((uint64_t)prob0 + (uint64_t)p + 1));
    if (tid < R) keys[tid] = boot_mix(pk + BOOT_G * ((uint64_t)rep0 + (uint64_t)(r0 + tid) + 1));
    if (tid == 0) nbad = 0;
    boot_active(m, [&](int i) { return !w || w[i] != 0.0; }, mask, base);                       // (the barriers cover keys and nbad)
    const int tpr = 1 << tsh, col = tid & (tpr - 1), slot = tid >> tsh, nslot = 256 >> tsh, mh = m / V;
    const size_t rstride = (size_t)nprob * m;                        // from one replica to the next
    double *const yo = yout + ((size_t)r0 * nprob + p) * m;
    if (blockIdx.y == 0) {                                           // (the same branch for the whole workgroup)
        int c = 0;
        for (int i = tid; i < m; i += 256) c += boot_is_active(i, mask) && boot_pois_bad(mu[i]) ? 1 : 0;
        if (c) atomicAdd(&nbad, c);
        __syncthreads();
        if (tid == 0) bad[p] = nbad;
    }
    const bool staged = nslot > 1;                                   // m <= 256: the host gave 6 m doubles of dynamic LDS
    double *const sh = reinterpret_cast<double *>(boot_lds);         // [6][m]: M, L, T, kmin, kmax, r by row
    if (staged) {
        if (tid < m) {
            const boot_pois s = boot_pois_row(boot_is_active(tid, mask), mu[tid]);
            sh[tid] = s.M;
            sh[m + tid] = s.L;
            sh[2 * m + tid] = s.T;
            sh[3 * m + tid] = s.kmin;
            sh[4 * m + tid] = s.kmax;
            sh[5 * m + tid] = s.r;
        }
        __syncthreads();
    }
    for (int u = col; u < mh; u += tpr) {
        boot_pois st[V];
        double mi[V], yi[V];
        uint64_t gk[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int i = u * V + v;
            mi[v] = mu[i];
            yi[v] = y[i];
            gk[v] = BOOT_G * ((uint64_t)i + 1);
            if (staged) {
                st[v].M = sh[i];
                st[v].L = sh[m + i];
                st[v].T = sh[2 * m + i];
                st[v].kmin = sh[3 * m + i];
                st[v].kmax = sh[4 * m + i];
                st[v].r = sh[5 * m + i];
            } else
                st[v] = boot_pois_row(boot_is_active(i, mask), mi[v]);
        }
        for (int r = slot; r < R; r += nslot) {
            const uint64_t key = keys[r];
            double out[V];
#pragma unroll
            for (int v = 0; v < V; ++v)
                out[v] = st[v].T > 0.0 ? boot_pois_draw(st[v], mi[v], boot_mix(key + gk[v])) : st[v].T == 0.0 ? 0.0 : yi[v];
            double *dst = yo + (size_t)r * rstride + (size_t)u * V;
            if (V == 2) *reinterpret_cast<double2 *>(dst) = make_double2(out[0], out[V - 1]);
            else dst[0] = out[0];
        }
    }
}

// valid [nrep][nprob] (a byte each): is every one of the n parameters of replica b of problem p finite
static __global__ void __launch_bounds__(256) k_boot_valid(size_t total, int n, const double *__restrict__ xs, unsigned char *__restrict__ valid)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const double *__restrict__ x = xs + e * (size_t)n;
    bool ok = true;
    for (int j = 0; j < n; ++j) ok = ok && fabs(x[j]) <= DBL_MAX;
    valid[e] = ok ? 1 : 0;
}

// One workgroup per (problem, parameter): the valid values in replica order into LDS (ballot + prefix), a rank sort in place --
// element e goes to the number of elements that are below it, or equal to it and before it: stable, no padding, every
// thread holding up to 16 elements in registers while all of them read the same x_f --, then wave 0 sums in the cost's
// order and its lane 0 takes the quantiles.
static __global__ void __launch_bounds__(256) k_boot_summary(int nrep, int nprob, int n, const double *__restrict__ xs,
                                                       const unsigned char *__restrict__ valid, double qlo, double qhi,
                                                       double *__restrict__ mean, double *__restrict__ sd, double *__restrict__ lo,
                                                       double *__restrict__ hi, int32_t *__restrict__ nvalid)
{
    __shared__ double xc[NLH_BOOT_MAX_REP];
    __shared__ unsigned long long mask[NLH_BOOT_MAX_REP / 64];
    __shared__ int base[NLH_BOOT_MAX_REP / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63;
    const int p = (int)(blockIdx.x / (unsigned)n), j = (int)(blockIdx.x - (unsigned)p * (unsigned)n);
    const int cnt = boot_active(nrep, [&](int b) { return valid[(size_t)b * nprob + p] != 0; }, mask, base);
    for (int b = tid; b < nrep; b += 256)
        if (boot_is_active(b, mask)) xc[boot_rank(b, mask, base)] = xs[((size_t)b * nprob + p) * n + j];
    __syncthreads();
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
    if (tid >= 64) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const size_t o = (size_t)p * n + j;
    if (lane == 0 && j == 0) nvalid[p] = cnt;
    if (cnt == 0) {
        if (lane == 0) { mean[o] = nan; sd[o] = nan; lo[o] = nan; hi[o] = nan; }
        return;
    }
    double s = 0.0;
    for (int i = lane; i < cnt; i += 64) s = s + xc[i];
    s = wave_reduce_sum(s);
    const double mn = __shfl(s, 0, 64) / (double)cnt;
    double q2 = 0.0;
    for (int i = lane; i < cnt; i += 64) {
        const double d = xc[i] - mn;
        q2 = q2 + d * d;
    }
    q2 = wave_reduce_sum(q2);
    if (lane != 0) return;
    mean[o] = mn;
    sd[o] = cnt > 1 ? __dsqrt_rn(q2 / (double)(cnt - 1)) : nan;
    const double qq[2] = {qlo, qhi};
    double *const dst[2] = {lo, hi};
    for (int t = 0; t < 2; ++t) {
        const double h = qq[t] * (double)(cnt - 1);
        int k = (int)floor(h);
        k = k < 0 ? 0 : (k > cnt - 1 ? cnt - 1 : k);
        const double g = h - (double)k;
        const int k1 = k + 1 < cnt ? k + 1 : cnt - 1;
        dst[t][o] = xc[k] + g * (xc[k1] - xc[k]);
    }
}
