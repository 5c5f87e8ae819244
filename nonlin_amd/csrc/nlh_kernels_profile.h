// nlh_kernels_profile.h -- the root finder of the profile-likelihood interval (include/nonlin_hip_profile.h: nlh_profile_*): a
// thread per end.  The arithmetic is the header's, one IEEE operation per statement (-ffp-contract=off); an end reads and
// writes its own entries alone, so its result does not depend on the launch shape or on which other ends are active.
#pragma once
#include "nlh_internal.h"

static __device__ inline bool prof_finite(double v) { return fabs(v) <= DBL_MAX; }
static __device__ inline double prof_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// theta clipped to the side's bound
static __device__ inline double prof_clip(double theta, double bound, int s)
{
    if (s == 0) return theta < bound ? bound : theta;
    return theta > bound ? bound : theta;
}

static __device__ inline void prof_finish(const nlh_profile_state &st, size_t e, int code, double end)
{
    st.flag[e] = st.flag[e] | code;
    st.end[e] = end;
    st.phase[e] = NLH_PROFILE_DONE;
}

// a thread per end e = (p*n + j)*2 + s; the thread of (j, s) = (0, 0) also writes the problem's delta.  xl, xu: device copies
// of the box, or null
static __global__ void __launch_bounds__(256)
k_profile_start(int nprob, int m, int n, const double *__restrict__ x, const double *__restrict__ sigma, const int32_t *__restrict__ ddof,
                double crit, double rc, int scaled, const double *__restrict__ xl, const double *__restrict__ xu, nlh_profile_state st)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nprob * n * 2) return;
    const int s = (int)(e & 1);
    const size_t pj = e >> 1;
    const int p = (int)(pj / n), j = (int)(pj - (size_t)p * n);
    const double C0 = st.C0[p];
    const int dof = ddof ? ddof[p] : m - n;
    double delta = crit;
    if (scaled) {
        delta = crit * C0;
        delta = delta / (double)dof;
    }
    if (j == 0 && s == 0) st.delta[p] = delta;
    const double xh = x[pj], sg = sigma[pj];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double bound = s ? (xu ? xu[j] : inf) : (xl ? xl[j] : -inf);
    const double w = rc * sg;
    double theta = s ? xh + w : xh - w;
    theta = prof_clip(theta, bound, s);
    st.xhat[e] = xh; st.width[e] = w; st.bound[e] = bound;
    st.a[e] = xh; st.ga[e] = -delta; st.b[e] = prof_nan(); st.gb[e] = prof_nan();
    st.theta[e] = theta; st.end[e] = prof_nan();
    st.phase[e] = NLH_PROFILE_EXPAND; st.flag[e] = 0; st.last[e] = 0; st.nexp[e] = 0; st.nev[e] = 0; st.nfail[e] = 0;
    const bool ok = prof_finite(xh) && prof_finite(sg) && sg > 0.0 && prof_finite(C0) && C0 > 0.0 && prof_finite(delta) && delta > 0.0 &&
                    dof > 0 && prof_finite(crit) && crit > 0.0;
    if (!ok) prof_finish(st, e, NLH_PROFILE_NO_START, prof_nan());
    else if (s ? xh >= bound : xh <= bound) prof_finish(st, e, NLH_PROFILE_ON_BOUND, bound);
}

// a thread per active end (the entries of act are distinct); n: the unknowns, so that end e belongs to problem e / (2 n)
static __global__ void __launch_bounds__(256)
k_profile_step(int nend, int n, int nact, const int32_t *__restrict__ act, const double *__restrict__ cost, const int32_t *__restrict__ fail,
               nlh_profile_state st, double tol, double xtol, int max_expand, int maxit)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nact) return;
    const int ei = act[i];
    if (ei < 0 || ei >= nend) return;
    const size_t e = (size_t)ei;
    if (st.phase[e] == NLH_PROFILE_DONE) return;
    const int s = ei & 1, p = ei / (2 * n);
    const double c = cost[i];
    const int nev = st.nev[e] + 1;
    st.nev[e] = nev;
    double theta = st.theta[e], a = st.a[e], b = st.b[e], ga = st.ga[e], gb = st.gb[e];
    if ((fail && fail[i] != 0) || !prof_finite(c)) {
        const int nf = st.nfail[e] + 1;
        st.nfail[e] = nf;
        if (nf > 3) { prof_finish(st, e, NLH_PROFILE_FIT_FAILED, prof_nan()); return; }
        double d = theta - a;
        d = d * 0.5;
        theta = a + d;
        st.theta[e] = theta;
        if (nev >= maxit) prof_finish(st, e, NLH_PROFILE_MAXIT, theta);
        return;
    }
    st.nfail[e] = 0;
    const double C0 = st.C0[p], delta = st.delta[p];
    const double t = tol * delta;
    double g = c - C0;
    g = g - delta;
    if (c < C0 - t) st.flag[e] = st.flag[e] | NLH_PROFILE_LOWER;
    if (fabs(g) <= t) { prof_finish(st, e, NLH_PROFILE_OK, theta); return; }
    const double xh = st.xhat[e], bound = st.bound[e];
    int last = st.last[e];
    if (st.phase[e] == NLH_PROFILE_EXPAND) {
        if (g < 0.0) {
            st.a[e] = theta; st.ga[e] = g;
            const int nx = st.nexp[e];
            if (theta == bound) { prof_finish(st, e, NLH_PROFILE_OPEN_AT_BOUND, bound); return; }
            if (nx >= max_expand) {
                const double inf = __longlong_as_double(0x7ff0000000000000ll);
                prof_finish(st, e, NLH_PROFILE_OPEN, s ? inf : -inf);
                return;
            }
            st.nexp[e] = nx + 1;
            double d = theta - xh;
            d = 2.0 * d;
            theta = xh + d;
            theta = prof_clip(theta, bound, s);
            st.theta[e] = theta;
            if (nev >= maxit) prof_finish(st, e, NLH_PROFILE_MAXIT, theta);
            return;
        }
        b = theta; gb = g; last = 1;
        st.phase[e] = NLH_PROFILE_BRACKET;
    } else if (g < 0.0) {
        a = theta; ga = g;
        if (last == -1) gb = gb * 0.5;
        last = -1;
    } else {
        b = theta; gb = g;
        if (last == 1) ga = ga * 0.5;
        last = 1;
    }
    st.a[e] = a; st.ga[e] = ga; st.b[e] = b; st.gb[e] = gb; st.last[e] = last;
    double u = a * gb, v = b * ga;
    u = u - v;
    v = gb - ga;
    theta = u / v;
    double d = b - a;
    if (!((theta > a && theta < b) || (theta < a && theta > b))) {
        double hd = d * 0.5;
        theta = a + hd;
    }
    st.theta[e] = theta;
    if (fabs(d) <= xtol * st.width[e]) { prof_finish(st, e, NLH_PROFILE_OK, theta); return; }
    if (nev >= maxit) prof_finish(st, e, NLH_PROFILE_MAXIT, theta);
}

// how many ends still run: one count per workgroup, then one atomic add of it (integers: the order does not matter)
static __global__ void __launch_bounds__(256) k_profile_left(int nend, const int32_t *__restrict__ phase, int32_t *left)
{
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < nend && phase[e] != NLH_PROFILE_DONE) atomicAdd(&cnt, 1);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(left, cnt);
}
