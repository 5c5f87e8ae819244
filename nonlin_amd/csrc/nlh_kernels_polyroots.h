// nlh_kernels_polyroots.h -- polynomial%roots (src/nonlin_polynomials.f90:357-381) for a batch of real polynomials: the
// eigenvalues of the companion matrix of :346-353 by DGEBAL's balancing and DLAHQR's double-shift QR, and the batched
// Horner evaluation of :283-286 / :317-320.  tests/polyroots_restatement.py states the same algorithm statement by
// statement in plain Python; every form below performs those scalar operations in that order (the wave forms spread the
// independent element updates of one reflector, and of one balancing scale, over lanes and never re-associate a sum).
//
// One algorithm (pr_solve), written once over a matrix policy:
//   PrLaneMat  lane per polynomial: the window of lane l lives in LDS lane-minor, element (r, c) at
//              ((r-1) m + (c-1)) 64 + l doubles, so a wave's ds_read_b64 / ds_write_b64 touches 64 consecutive doubles;
//              loops run 0, 1, 2, ...; nothing is shared between lanes and there is no wave-wide operation.
//   PrWaveMat  wave per polynomial (one wave per workgroup): the window is dense row-major with an odd leading dimension
//              (column walks spread over the banks) in LDS or in global memory; the scalar bookkeeping (shifts,
//              deflation tests, reflectors, balancing sums) is computed by every lane from the same values, so control
//              flow is wave-uniform; the 3-row / 3-column updates and the row / column scalings run lane = column /
//              lane = row with a barrier between dependent phases.
// Matrices are 1-based as in LAPACK.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static const int PR_LANE_MAX = 8;        // lane form: (m m + m) 64 doubles of LDS per wave, 36 KiB at m = 8
static const int PR_WAVE_LDS_MAX = 128;  // wave form in LDS: 129 128 + 128 doubles = 130 KiB of the 158 KiB a launch may ask for
static const int PR_MAX_ORDER = 256;     // wave form on a global-memory window; beyond: NLH_ARRAY_SIZE_ERROR

#define PR_EPS 2.220446049250313e-16     /* DLAMCH('P') */
#define PR_SAFMIN 2.2250738585072014e-308 /* DLAMCH('S') */

struct PrLaneMat {
    double *base;                        // LDS, already offset by the lane
    int m;
    static constexpr bool wave = false;
    __device__ void dims(int m_) { m = m_; }
    __device__ double get(int r, int c) const { return base[((r - 1) * m + (c - 1)) * 64]; }
    __device__ void set(int r, int c, double v) const { base[((r - 1) * m + (c - 1)) * 64] = v; }
    __device__ double sget(int i) const { return base[(m * m + (i - 1)) * 64]; }
    __device__ void sset(int i, double v) const { base[(m * m + (i - 1)) * 64] = v; }
    __device__ int first() const { return 0; }
    __device__ int step() const { return 1; }
    __device__ void sync() const {}
    __device__ bool writer() const { return true; }
};

struct PrWaveMat {
    double *base;                        // LDS or global, this polynomial's window
    int ld, m, lane;
    static constexpr bool wave = true;
    __device__ void dims(int m_) { m = m_; ld = m_ | 1; }
    __device__ double get(int r, int c) const { return base[(r - 1) * ld + (c - 1)]; }
    __device__ void set(int r, int c, double v) const { base[(r - 1) * ld + (c - 1)] = v; }
    __device__ double sget(int i) const { return base[m * ld + (i - 1)]; }
    __device__ void sset(int i, double v) const { base[m * ld + (i - 1)] = v; }
    __device__ int first() const { return lane; }
    __device__ int step() const { return 64; }
    __device__ void sync() const { __syncthreads(); }   // one wave per workgroup: orders the lanes' window accesses
    __device__ bool writer() const { return lane == 0; }
};
// doubles of window storage one polynomial of order n needs in the wave forms
static inline size_t pr_wave_doubles(int n) { return (size_t)(n | 1) * n + n; }

__device__ __forceinline__ double pr_sign(double a, double b) { return copysign(fabs(a), b); }
__device__ __forceinline__ double pr_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double pr_min(double a, double b) { return b < a ? b : a; }

// DLAPY2 (no NaN reaches it)
__device__ __forceinline__ double pr_lapy2(double x, double y)
{
    const double xabs = fabs(x), yabs = fabs(y);
    const double w = pr_max(xabs, yabs), z = pr_min(xabs, yabs);
    if (z == 0.0) return w;
    const double q = z / w;
    return w * sqrt(1.0 + q * q);
}

// DNRM2 (reference BLAS, scaled sum of squares) of the nx = 1 or 2 entries below a reflector's head
__device__ __forceinline__ double pr_nrm2(int nx, double x1, double x2)
{
    if (nx == 1) return fabs(x1);
    double scale = 0.0, ssq = 1.0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const double x = t ? x2 : x1;
        if (x != 0.0) {
            const double absxi = fabs(x);
            if (scale < absxi) {
                const double q = scale / absxi;
                ssq = 1.0 + ssq * (q * q);
                scale = absxi;
            } else {
                const double q = absxi / scale;
                ssq = ssq + q * q;
            }
        }
    }
    return scale * sqrt(ssq);
}

// DLARFG for nr = 2 or 3: alpha -> beta, (x1, x2) -> v(2), v(3); returns tau
__device__ __forceinline__ double pr_larfg(int nr, double &alpha, double &x1, double &x2)
{
    const double rf_safmin = PR_SAFMIN / (PR_EPS * 0.5);           // DLAMCH('S') / DLAMCH('E')
    const double rf_rsafmn = 1.0 / rf_safmin;
    double xnorm = pr_nrm2(nr - 1, x1, x2);
    if (xnorm == 0.0) return 0.0;
    double beta = -pr_sign(pr_lapy2(alpha, xnorm), alpha);
    int knt = 0;
    if (fabs(beta) < rf_safmin) {
        do {
            knt += 1;
            x1 = x1 * rf_rsafmn;
            x2 = x2 * rf_rsafmn;
            beta = beta * rf_rsafmn;
            alpha = alpha * rf_rsafmn;
        } while (fabs(beta) < rf_safmin && knt < 20);
        xnorm = pr_nrm2(nr - 1, x1, x2);
        beta = -pr_sign(pr_lapy2(alpha, xnorm), alpha);
    }
    const double tau = (beta - alpha) / beta;
    const double sc = 1.0 / (alpha - beta);
    x1 = x1 * sc;
    x2 = x2 * sc;
    for (int t = 0; t < knt; ++t) beta = beta * rf_safmin;
    alpha = beta;
    return tau;
}

// DLANV2, eigenvalues only
__device__ __forceinline__ void pr_lanv2(double a, double b, double c, double d, double &rt1r, double &rt1i, double &rt2r,
                                         double &rt2i)
{
    if (c == 0.0) {
    } else if (b == 0.0) {
        const double temp = d;
        d = a;
        a = temp;
        b = -c;
        c = 0.0;
    } else if ((a - d) == 0.0 && signbit(b) != signbit(c)) {
    } else {
        double temp = a - d;
        double p = 0.5 * temp;
        const double bcmax = pr_max(fabs(b), fabs(c));
        const double bcmis = pr_min(fabs(b), fabs(c)) * copysign(1.0, b) * copysign(1.0, c);
        const double scale = pr_max(fabs(p), bcmax);
        double z = (p / scale) * p + (bcmax / scale) * bcmis;
        if (z >= 4.0 * PR_EPS) {
            z = p + pr_sign(sqrt(scale) * sqrt(z), p);
            a = d + z;
            d = d - (bcmax / z) * bcmis;
            b = b - c;
            c = 0.0;
        } else {
            const double sigma = b + c;
            const double tau = pr_lapy2(sigma, temp);
            const double cs = sqrt(0.5 * (1.0 + fabs(sigma) / tau));
            const double sn = -(p / (tau * cs)) * copysign(1.0, sigma);
            const double aa = a * cs + b * sn;
            const double bb = -a * sn + b * cs;
            const double cc = c * cs + d * sn;
            const double dd = -c * sn + d * cs;
            a = aa * cs + cc * sn;
            b = bb * cs + dd * sn;
            c = -aa * sn + cc * cs;
            d = -bb * sn + dd * cs;
            temp = 0.5 * (a + d);
            a = temp;
            d = temp;
            if (c != 0.0) {
                if (b != 0.0) {
                    if (signbit(b) == signbit(c)) {
                        const double sab = sqrt(fabs(b));
                        const double sac = sqrt(fabs(c));
                        p = pr_sign(sab * sac, c);
                        a = temp + p;
                        d = temp - p;
                        b = b - c;
                        c = 0.0;
                    }
                } else {
                    b = -c;
                    c = 0.0;
                }
            }
        }
    }
    rt1r = a;
    rt2r = d;
    if (c == 0.0) {
        rt1i = 0.0;
        rt2i = 0.0;
    } else {
        rt1i = sqrt(fabs(b)) * sqrt(fabs(c));
        rt2i = -rt1i;
    }
}

// The scaling loop of DGEBAL (one-norm sums, radix 2, factor 0.95) on the window [1, m].
template <class M> __device__ void pr_balance(const M &H, int m)
{
    const double sfmin1 = PR_SAFMIN / PR_EPS, sfmax1 = 1.0 / sfmin1, sfmin2 = sfmin1 * 2.0, sfmax2 = 1.0 / sfmin2;
    for (int i = 1 + H.first(); i <= m; i += H.step()) H.sset(i, 1.0);
    H.sync();
    bool noconv;
    do {
        noconv = false;
        for (int i = 1; i <= m; ++i) {
            double c = 0.0, r = 0.0, ca = 0.0, ra = 0.0;
            for (int j = 1; j <= m; ++j) {
                const double cji = fabs(H.get(j, i)), rij = fabs(H.get(i, j));
                if (j != i) {
                    c = c + cji;
                    r = r + rij;
                }
                ca = pr_max(ca, cji);
                ra = pr_max(ra, rij);
            }
            if (c == 0.0 || r == 0.0) continue;
            double g = r / 2.0, f = 1.0;
            const double s = c + r;
            while (!(c >= g || pr_max(pr_max(f, c), ca) >= sfmax2 || pr_min(pr_min(r, g), ra) <= sfmin2)) {
                f = f * 2.0;
                c = c * 2.0;
                ca = ca * 2.0;
                r = r / 2.0;
                g = g / 2.0;
                ra = ra / 2.0;
            }
            g = c / 2.0;
            while (!(g < r || pr_max(r, ra) >= sfmax2 || pr_min(pr_min(pr_min(f, c), g), ca) <= sfmin2)) {
                f = f / 2.0;
                c = c / 2.0;
                g = g / 2.0;
                ca = ca / 2.0;
                r = r * 2.0;
                ra = ra * 2.0;
            }
            if ((c + r) >= 0.95 * s) continue;
            const double sci = H.sget(i);
            if (f < 1.0 && sci < 1.0) {
                if (f * sci <= sfmin1) continue;
            }
            if (f > 1.0 && sci > 1.0) {
                if (sci >= sfmax1 / f) continue;
            }
            g = 1.0 / f;
            H.sync();                                              // every lane has read scale(i)
            if (H.writer()) H.sset(i, sci * f);
            noconv = true;
            for (int j = 1 + H.first(); j <= m; j += H.step()) H.set(i, j, H.get(i, j) * g);
            H.sync();
            for (int j = 1 + H.first(); j <= m; j += H.step()) H.set(j, i, H.get(j, i) * f);
            H.sync();
        }
    } while (noconv);
}

// DLAHQR on the window [1, nh], WANTT = WANTZ = .false.; eigenvalue i goes to z[2 (i-1)], z[2 (i-1) + 1].  Returns 0, or
// the i for which rows 1..i have not converged within 30 max(10, nh) sweeps in total.
template <class M> __device__ int pr_hqr(const M &H, int nh, double *z)
{
    const bool w = H.writer();
    if (nh == 1) {
        if (w) { z[0] = H.get(1, 1); z[1] = 0.0; }
        return 0;
    }
    const double ulp = PR_EPS;
    const double smlnum = PR_SAFMIN * ((double)nh / ulp);
    const int itmax = 30 * (nh > 10 ? nh : 10);
    int sweeps = 0;
    int i = nh;
    while (i >= 1) {
        int l = 1, its = 0;
        for (;;) {
            int k = i;
            while (k > l) {                                        // a small subdiagonal element
                const double hkk1 = fabs(H.get(k, k - 1));
                if (hkk1 <= smlnum) break;
                double tst = fabs(H.get(k - 1, k - 1)) + fabs(H.get(k, k));
                if (tst == 0.0) {
                    if (k - 2 >= 1) tst = tst + fabs(H.get(k - 1, k - 2));
                    if (k + 1 <= nh) tst = tst + fabs(H.get(k + 1, k));
                }
                if (hkk1 <= ulp * tst) {                           // Ahues & Tisseur
                    const double hk1k = fabs(H.get(k - 1, k));
                    const double ab = pr_max(hkk1, hk1k);
                    const double ba = pr_min(hkk1, hk1k);
                    const double dkk = fabs(H.get(k, k));
                    const double ddf = fabs(H.get(k - 1, k - 1) - H.get(k, k));
                    const double aa = pr_max(dkk, ddf);
                    const double bb = pr_min(dkk, ddf);
                    const double s = aa + ab;
                    if (ba * (ab / s) <= pr_max(smlnum, ulp * (bb * (aa / s)))) break;
                }
                k -= 1;
            }
            l = k;
            if (l > 1) H.set(l, l - 1, 0.0);
            if (l >= i - 1) break;
            if (sweeps >= itmax) return i;
            sweeps += 1;
            double h11, h12, h21, h22, s;
            if (its == 10) {                                       // exceptional shift
                s = fabs(H.get(l + 1, l)) + fabs(H.get(l + 2, l + 1));
                h11 = 0.75 * s + H.get(l, l);
                h12 = -0.4375 * s;
                h21 = s;
                h22 = h11;
            } else if (its == 20) {
                s = fabs(H.get(i, i - 1)) + fabs(H.get(i - 1, i - 2));
                h11 = 0.75 * s + H.get(i, i);
                h12 = -0.4375 * s;
                h21 = s;
                h22 = h11;
            } else {
                h11 = H.get(i - 1, i - 1);
                h21 = H.get(i, i - 1);
                h12 = H.get(i - 1, i);
                h22 = H.get(i, i);
            }
            s = fabs(h11) + fabs(h12) + fabs(h21) + fabs(h22);
            double rt1r, rt1i, rt2r, rt2i;
            if (s == 0.0) {
                rt1r = 0.0;
                rt1i = 0.0;
                rt2r = 0.0;
                rt2i = 0.0;
            } else {
                h11 = h11 / s;
                h21 = h21 / s;
                h12 = h12 / s;
                h22 = h22 / s;
                const double tr = (h11 + h22) / 2.0;
                const double det = (h11 - tr) * (h22 - tr) - h12 * h21;
                const double rtdisc = sqrt(fabs(det));
                if (det >= 0.0) {
                    rt1r = tr * s;
                    rt2r = rt1r;
                    rt1i = rtdisc * s;
                    rt2i = -rt1i;
                } else {
                    rt1r = tr + rtdisc;
                    rt2r = tr - rtdisc;
                    if (fabs(rt1r - h22) <= fabs(rt2r - h22)) {
                        rt1r = rt1r * s;
                        rt2r = rt1r;
                    } else {
                        rt2r = rt2r * s;
                        rt1r = rt2r;
                    }
                    rt1i = 0.0;
                    rt2i = 0.0;
                }
            }
            int m = i - 2;
            double v1, v2, v3;
            for (;;) {                                             // two consecutive small subdiagonal elements
                const double hmm = H.get(m, m);
                const double hm1m = H.get(m + 1, m);
                const double hm1m1 = H.get(m + 1, m + 1);
                double h21s = fabs(hm1m);
                s = fabs(hmm - rt2r) + fabs(rt2i) + h21s;
                h21s = hm1m / s;
                v1 = h21s * H.get(m, m + 1) + (hmm - rt1r) * ((hmm - rt2r) / s) - rt1i * (rt2i / s);
                v2 = h21s * (hmm + hm1m1 - rt1r - rt2r);
                v3 = h21s * H.get(m + 2, m + 1);
                s = fabs(v1) + fabs(v2) + fabs(v3);
                v1 = v1 / s;
                v2 = v2 / s;
                v3 = v3 / s;
                if (m == l) break;
                if (fabs(H.get(m, m - 1)) * (fabs(v2) + fabs(v3)) <=
                    ulp * fabs(v1) * (fabs(H.get(m - 1, m - 1)) + fabs(hmm) + fabs(hm1m1)))
                    break;
                m -= 1;
            }
            H.sync();                                              // every lane has its scalars before a lane writes
            for (int k2 = m; k2 <= i - 1; ++k2) {                  // the double-shift QR step
                const int nr = (i - k2 + 1) < 3 ? (i - k2 + 1) : 3;
                if (k2 > m) {
                    v1 = H.get(k2, k2 - 1);
                    v2 = H.get(k2 + 1, k2 - 1);
                    v3 = nr == 3 ? H.get(k2 + 2, k2 - 1) : 0.0;
                }
                const double t1 = pr_larfg(nr, v1, v2, v3);
                if (k2 > m) {
                    H.set(k2, k2 - 1, v1);
                    H.set(k2 + 1, k2 - 1, 0.0);
                    if (k2 < i - 1) H.set(k2 + 2, k2 - 1, 0.0);
                } else if (m > l) {
                    H.set(k2, k2 - 1, H.get(k2, k2 - 1) * (1.0 - t1));
                }
                const double t2 = t1 * v2;
                if (nr == 3) {
                    const double t3 = t1 * v3;
                    for (int j = k2 + H.first(); j <= i; j += H.step()) {
                        const double a0 = H.get(k2, j), a1 = H.get(k2 + 1, j), a2 = H.get(k2 + 2, j);
                        const double sm = a0 + v2 * a1 + v3 * a2;
                        H.set(k2, j, a0 - sm * t1);
                        H.set(k2 + 1, j, a1 - sm * t2);
                        H.set(k2 + 2, j, a2 - sm * t3);
                    }
                    H.sync();
                    const int jhi = (k2 + 3) < i ? (k2 + 3) : i;
                    for (int j = l + H.first(); j <= jhi; j += H.step()) {
                        const double a0 = H.get(j, k2), a1 = H.get(j, k2 + 1), a2 = H.get(j, k2 + 2);
                        const double sm = a0 + v2 * a1 + v3 * a2;
                        H.set(j, k2, a0 - sm * t1);
                        H.set(j, k2 + 1, a1 - sm * t2);
                        H.set(j, k2 + 2, a2 - sm * t3);
                    }
                    H.sync();
                } else {
                    for (int j = k2 + H.first(); j <= i; j += H.step()) {
                        const double a0 = H.get(k2, j), a1 = H.get(k2 + 1, j);
                        const double sm = a0 + v2 * a1;
                        H.set(k2, j, a0 - sm * t1);
                        H.set(k2 + 1, j, a1 - sm * t2);
                    }
                    H.sync();
                    for (int j = l + H.first(); j <= i; j += H.step()) {
                        const double a0 = H.get(j, k2), a1 = H.get(j, k2 + 1);
                        const double sm = a0 + v2 * a1;
                        H.set(j, k2, a0 - sm * t1);
                        H.set(j, k2 + 1, a1 - sm * t2);
                    }
                    H.sync();
                }
            }
            its += 1;
        }
        if (l == i) {
            if (w) { z[2 * (i - 1)] = H.get(i, i); z[2 * (i - 1) + 1] = 0.0; }
        } else {
            double rt1r, rt1i, rt2r, rt2i;
            pr_lanv2(H.get(i - 1, i - 1), H.get(i - 1, i), H.get(i, i - 1), H.get(i, i), rt1r, rt1i, rt2r, rt2i);
            if (w) {
                z[2 * (i - 2)] = rt1r; z[2 * (i - 2) + 1] = rt1i;
                z[2 * (i - 1)] = rt2r; z[2 * (i - 1) + 1] = rt2i;
            }
        }
        i = l - 1;
    }
    return 0;
}

__device__ __forceinline__ bool pr_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN

// One polynomial: a[0..n] (constant first) -> z[n][2], *info.
template <class M> __device__ void pr_solve(M &H, int n, const double *a, double *z, int32_t *info)
{
    const bool w = H.writer();
    int bad = 0;
    for (int i = 0; i <= n; ++i)
        if (!pr_finite(a[i])) bad = NLH_INVALID_INPUT_ERROR;
    const double lead = a[n];
    if (!bad && lead == 0.0) bad = NLH_DIVIDE_BY_ZERO_ERROR;
    int kz = 0;
    if (!bad) {
        bool counting = true;
        for (int i = 1; i <= n; ++i) {
            const double c = -a[i - 1] / lead;                     // :351
            if (!pr_finite(c)) bad = NLH_INVALID_INPUT_ERROR;
            if (counting && i <= n - 1 && c == 0.0) kz = i;        // DGEBAL's isolated rows: leading zeros of the column
            else counting = false;
        }
    }
    if (bad) {
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        for (int i = H.first(); i < 2 * n; i += H.step()) z[i] = qnan;
        if (w) *info = bad;
        return;
    }
    const int m = n - kz;
    H.dims(m);
    if (w)
        for (int i = m + 1; i <= n; ++i) { z[2 * (i - 1)] = 0.0; z[2 * (i - 1) + 1] = 0.0; }   // the isolated diagonal entries
    for (int r = 1; r <= m; ++r)
        for (int c = 1 + H.first(); c <= m; c += H.step()) H.set(r, c, 0.0);
    H.sync();
    for (int i = 1 + H.first(); i <= m; i += H.step()) {
        H.set(i, m, -a[kz + i - 1] / lead);
        if (i < m) H.set(i + 1, i, 1.0);                           // :352
    }
    H.sync();
    if (m > 1) pr_balance(H, m);
    const int fail = pr_hqr(H, m, z);
    if (fail) {
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        H.sync();
        for (int i = H.first(); i < 2 * fail; i += H.step()) z[i] = qnan;
    }
    if (w) *info = fail ? NLH_CONVERGENCE_ERROR : 0;
}

// lane per polynomial; dynamic LDS: (n n + n) 64 doubles
__global__ __launch_bounds__(64) void k_polyroots_lane(int32_t nprob, int32_t n, const double *__restrict__ coef,
                                                       double *__restrict__ z, int32_t *__restrict__ info)
{
    extern __shared__ double pr_lds[];
    const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (p >= (size_t)nprob) return;                                // no wave-wide operation follows
    PrLaneMat H;
    H.base = pr_lds + threadIdx.x;
    H.m = n;
    pr_solve(H, n, coef + p * (size_t)(n + 1), z + p * 2 * (size_t)n, info + p);
}

// wave per polynomial, one wave per workgroup; the window in dynamic LDS (pr_wave_doubles(n) doubles) or, GLOBAL, in
// win [nprob][pr_wave_doubles(n)].  The problem index is blockIdx.x + p0 (the host slices a batch past the grid limit).
template <bool GLOBAL>
__global__ __launch_bounds__(64) void k_polyroots_wave(int32_t p0, int32_t n, const double *__restrict__ coef,
                                                       double *__restrict__ z, int32_t *__restrict__ info, double *win,
                                                       size_t win_stride)
{
    extern __shared__ double pr_lds[];
    const size_t p = (size_t)p0 + blockIdx.x;
    PrWaveMat H;
    H.base = GLOBAL ? win + (size_t)blockIdx.x * win_stride : pr_lds;
    H.lane = threadIdx.x;
    H.dims(n);
    pr_solve(H, n, coef + p * (size_t)(n + 1), z + p * 2 * (size_t)n, info + p);
}

// Horner, real x (:283-286): dcoef [nprob][order + 1], dx, dy [nprob][npts]; one thread per point
__global__ void k_poly_eval(size_t total, int32_t npts, int32_t order, const double *__restrict__ coef,
                            const double *__restrict__ x, double *__restrict__ y)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const double *c = coef + (t / (size_t)npts) * (size_t)(order + 1);
    const double xv = x[t];
    double yv;
    if (order == 0) {
        yv = c[0];
    } else {
        yv = c[order] * xv + c[order - 1];
        for (int j = order - 2; j >= 0; --j) yv = yv * xv + c[j];
    }
    y[t] = yv;
}

// Horner, complex x (:317-320): y x is the four-multiply form, the real coefficient joins the real part only
__global__ void k_poly_eval_complex(size_t total, int32_t npts, int32_t order, const double *__restrict__ coef,
                                    const double *__restrict__ x, double *__restrict__ y)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const double *c = coef + (t / (size_t)npts) * (size_t)(order + 1);
    const double xr = x[2 * t], xi = x[2 * t + 1];
    double yr, yi;
    if (order == 0) {
        yr = c[0];
        yi = 0.0;
    } else {
        yr = c[order] * xr + c[order - 1];
        yi = c[order] * xi;
        for (int j = order - 2; j >= 0; --j) {
            const double tr = yr * xr - yi * xi;
            const double ti = yr * xi + yi * xr;
            yr = tr + c[j];
            yi = ti;
        }
    }
    y[2 * t] = yr;
    y[2 * t + 1] = yi;
}
