// nlh_kernels_1var.h -- brent_solver%solve (brent_solve, src/nonlin_solve.f90:643-835) and newton_1var_solver%solve
// (newt1var_solve, :840-1032, with fcn1var_helper%diff, src/nonlin_single_var.f90:154-200) as a LOCK-STEP BATCH of
// scalar equations.  One lane per problem: the state is a handful of doubles and counters, kept in structure-of-arrays
// layout so that a wave's loads and stores coalesce.  A round: k_r1_advance consumes the values of the previous round's
// points, runs the reference's statements until the problem needs new values or stops, writes how many points it needs
// next and scans those counts over its 1024-thread block; k_nm_scan_top scans the block totals; k_r1_emit lays the
// points out in ascending problem order.  Every operation is the reference's, in its order (-ffp-contract=off): a
// problem's bits do not depend on the batch it is solved in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nlh_kernels_scan.h"

enum R1Kind : int32_t { R1_BRENT = 0, R1_NEWTON = 1 };

enum R1Phase : int32_t {
    R1_START = 0,        // (the first advance: the limits are read, the two endpoints are due)
    R1_ENDS = 1,         // f at both limits due (brent :717-718, newton :903-904)
    R1_MID = 2,          // newton: f (and f') at the midpoint due (:936-937)
    R1_STEP = 3,         // f at the new b (brent :804); newton: f and f' at the new x (:972-973)
    R1_FINAL = 4,        // newton with f present: the extra evaluation after the loop (:1011-1014), value discarded
    R1_DONE = 5
};

// bits of R1Soa::bits
enum : int32_t { R1_FCNVRG = 1, R1_XCNVRG = 2, R1_DCNVRG = 4, R1_FLAG = 8, R1_INVALID = 16 };

// The state slots.  Brent: the reference's names.  Newton: its names where they differ.
// (fb and newton's df are never carried over: each round's value replaces them.)
enum { BR_A = 0, BR_B, BR_C, BR_FA, BR_FC, BR_D, BR_E, BR_XM, R1_NSLOT };
enum { NW_X = 0, NW_XL, NW_XH, NW_FF, NW_DX, NW_DXOLD };

struct R1Soa {
    double *s[R1_NSLOT];           // [R1_NSLOT][np]
    double *pt0, *pt1;             // the points of the next round (pt1: the second limit, or x + h of a forward difference)
    double *fo;                    // f at the end (brent: fb :820; newton: ff :1017, or the endpoint's value :906-923)
    int32_t *phase, *iter, *neval, *ndiff, *bits;
};

struct R1Opts {
    double ftol, xtol, dtol;
    int32_t max_evals, user_diff, want_f, pad;
};

// The print_status block an advance produced (the host-callback form only)
struct R1Print {
    int32_t due, iter, neval, njac;
    double xnorm, fnorm;
};

#define R1_EPS      2.220446049250313e-16    // epsilon(1d0)
#define R1_SQRT_EPS 1.4901161193847656e-08   // sqrt(epsilon(1d0)) (f1h_diff_fcn :180-181), exact

static __device__ inline void r1_print(R1Print *pr, int p, int32_t iter, int32_t neval, int32_t njac, double xn, double fn)
{
    if (pr) { R1Print r; r.due = 1; r.iter = iter; r.neval = neval; r.njac = njac; r.xnorm = xn; r.fnorm = fn; pr[p] = r; }
}

// brent_solve from the consumed values up to the next evaluation.  Returns the number of points due.
static __device__ inline int32_t brent_advance(int p, bool first, const R1Opts &o, const double *__restrict__ lim,
                                               const double *__restrict__ fs, const int32_t *__restrict__ off, R1Soa &S,
                                               double *__restrict__ x, R1Print *pr)
{
    const int32_t phase = first ? (int32_t)R1_START : S.phase[p];
    if (phase == R1_DONE) return 0;
    if (phase == R1_START) {
        const double l1 = lim[2 * (size_t)p], l2 = lim[2 * (size_t)p + 1];
        x[p] = 0.0;                                                  // :691
        const double a = l2 < l1 ? l2 : l1, b = l2 > l1 ? l2 : l1;  // :692-693
        S.iter[p] = 0; S.neval[p] = 0; S.ndiff[p] = 0;
        if (fabs(a - b) < R1_EPS) {                                  // :713 (absolute epsilon)
            S.bits[p] = R1_INVALID; S.fo[p] = 0.0; S.phase[p] = R1_DONE;
            return 0;
        }
        S.bits[p] = 0;
        S.pt0[p] = a; S.pt1[p] = b; S.phase[p] = R1_ENDS;
        return 2;
    }
    double a, b, c, fa, fb, fc, d, e;
    int32_t iter = S.iter[p], neval, bits = 0;
    const double *v = fs + off[p];
    if (phase == R1_ENDS) {
        a = S.pt0[p]; b = S.pt1[p];
        c = d = e = 0.0;        // read unset on the first pass when fb == 0 exactly (ftol <= 0) or fb is NaN
        fa = v[0];                                                   // :717
        fb = v[1];                                                   // :718
        neval = 2;                                                   // :719
        fc = fb;                                                     // :720
    } else {
        a = S.s[BR_A][p]; b = S.s[BR_B][p]; c = S.s[BR_C][p]; fa = S.s[BR_FA][p];
        fc = S.s[BR_FC][p]; d = S.s[BR_D][p]; e = S.s[BR_E][p];
        fb = v[0];                                                   // :804
        neval = S.neval[p] + 1;                                      // :805
        r1_print(pr, p, iter, neval, 0, S.s[BR_XM][p], fb);          // :808-810
        if (neval >= o.max_evals) bits = R1_FLAG;                    // :813-816
    }
    int32_t due = 0;
    if (!bits) {
        iter = iter + 1;                                             // :723
        if ((fb > 0.0 && fc >= 0.0) || (fb < 0.0 && fc < 0.0)) {    // :726-727
            c = a; fc = fa; d = b - a; e = d;                        // :728-731
        }
        if (fabs(fc) < fabs(fb)) {                                   // :733-740
            a = b; b = c; c = a; fa = fb; fb = fc; fc = fa;
        }
        const double tol1 = 2.0 * R1_EPS * fabs(b) + 0.5 * o.xtol;   // :743
        const double xm = 0.5 * (c - b);                             // :744
        if (fabs(fb) < o.ftol) {                                     // :745-749
            x[p] = b; bits = R1_FCNVRG;
        } else if (fabs(xm) <= tol1) {                               // :750-754
            x[p] = b; bits = R1_XCNVRG;
        } else {
            if (fabs(e) >= tol1 && fabs(fa) > fabs(fb)) {            // :757
                const double s = fb / fa;                            // :760
                double pp, q;
                if (fabs(a - c) < R1_EPS) {                          // :761 (a == c)
                    pp = 2.0 * xm * s;                               // :762
                    q = 1.0 - s;                                     // :763
                } else {
                    q = fa / fc;                                     // :765
                    const double r = fb / fc;                        // :766
                    pp = s * (2.0 * xm * q * (q - r) - (b - a) * (r - 1.0));   // :767
                    q = (q - 1.0) * (r - 1.0) * (s - 1.0);           // :768
                }
                if (pp > 0.0) q = -q;                                // :772
                pp = fabs(pp);                                       // :773
                const double mn1 = 3.0 * xm * q - fabs(tol1 * q);    // :774
                const double mn2 = fabs(e * q);                      // :775
                const double temp = mn1 < mn2 ? mn1 : mn2;           // :776-780
                if (2.0 * pp < temp) { e = d; d = pp / q; }          // :781-785
                else { d = xm; e = d; }                              // :786-789
            } else {
                d = xm; e = d;                                       // :791-794
            }
            a = b;                                                   // :797
            fa = fb;                                                 // :798
            if (fabs(d) > tol1) b = b + d;                           // :799-800
            else b = b + copysign(tol1, xm);                         // :802: sign(tol1, xm), a negative zero included
            S.s[BR_XM][p] = xm;
            S.pt0[p] = b;
            due = 1;
        }
    }
    S.s[BR_A][p] = a; S.s[BR_B][p] = b; S.s[BR_C][p] = c; S.s[BR_FA][p] = fa; S.s[BR_FC][p] = fc;
    S.s[BR_D][p] = d; S.s[BR_E][p] = e;
    S.iter[p] = iter; S.neval[p] = neval;
    if (due) { S.phase[p] = R1_STEP; return 1; }
    S.bits[p] = bits; S.fo[p] = fb; S.phase[p] = R1_DONE;            // :820
    return 0;
}

// f1h_diff_fcn's step (:189-191): h = sqrt(eps) |x|, sqrt(eps) when h < eps
static __device__ inline double r1_fd_step(double xv)
{
    double h = R1_SQRT_EPS * fabs(xv);
    if (h < R1_EPS) h = R1_SQRT_EPS;
    return h;
}

// newt1var_solve from the consumed values up to the next evaluation.  Returns the number of points due: 2 in round 0,
// then 2 per iteration with forward differences (x, x + h), 1 with the user's derivative, 1 for the final evaluation.
static __device__ inline int32_t newton_advance(int p, bool first, const R1Opts &o, const double *__restrict__ lim,
                                                const double *__restrict__ fs, const double *__restrict__ ds,
                                                const int32_t *__restrict__ off, R1Soa &S, double *__restrict__ x, R1Print *pr)
{
    const int32_t phase = first ? (int32_t)R1_START : S.phase[p];
    if (phase == R1_DONE) return 0;
    if (phase == R1_START) {
        const double l1 = lim[2 * (size_t)p], l2 = lim[2 * (size_t)p + 1];
        const double x1 = l2 < l1 ? l2 : l1, x2 = l2 > l1 ? l2 : l1;  // :893-894
        S.iter[p] = 0; S.neval[p] = 0; S.ndiff[p] = 0;
        if (fabs(x1 - x2) < R1_EPS) {                                // :899: x untouched
            S.bits[p] = R1_INVALID; S.fo[p] = 0.0; S.phase[p] = R1_DONE;
            return 0;
        }
        S.bits[p] = 0;
        S.pt0[p] = x1; S.pt1[p] = x2; S.phase[p] = R1_ENDS;
        return 2;
    }
    const double *v = fs + off[p];
    if (phase == R1_FINAL) {                                         // :1011-1014: counted, the value discarded
        S.neval[p] = S.neval[p] + 1;
        x[p] = S.s[NW_X][p];
        S.fo[p] = S.s[NW_FF][p];                                     // :1017
        S.phase[p] = R1_DONE;
        return 0;
    }
    double xv, xl, xh, ff, df, dx, dxold;
    int32_t iter = S.iter[p], neval = S.neval[p], ndiff = S.ndiff[p], bits = 0;
    bool top = true;
    if (phase == R1_ENDS) {
        const double x1 = S.pt0[p], x2 = S.pt1[p];
        const double fl = v[0], fh = v[1];                           // :903-904
        neval = 2;                                                   // :905
        if (fabs(fl) < o.ftol || fabs(fh) < o.ftol) {                // :906-923: return at once
            const bool lo = fabs(fl) < o.ftol;
            x[p] = lo ? x1 : x2;
            S.fo[p] = lo ? fl : fh;
            S.neval[p] = 2; S.bits[p] = R1_FCNVRG; S.phase[p] = R1_DONE;
            return 0;
        }
        if (fl < 0.0) { xl = x1; xh = x2; }                          // :926-932
        else { xl = x2; xh = x1; }
        xv = 0.5 * (x1 + x2);                                        // :933
        dxold = fabs(x2 - x1);                                       // :934
        dx = dxold;                                                  // :935
        ff = 0.0; df = 0.0;
        top = false;                                                 // f and f' at the midpoint first (:936-937)
    } else {
        xv = S.s[NW_X][p]; xl = S.s[NW_XL][p]; xh = S.s[NW_XH][p]; dx = S.s[NW_DX][p]; dxold = S.s[NW_DXOLD][p];
        ff = v[0];                                                   // :936 / :972
        df = o.user_diff ? ds[off[p]] : (v[1] - ff) / r1_fd_step(xv);   // :937 / :973 (f1h_diff_fcn :198)
        neval = neval + 1;                                           // :938 / :974
        ndiff = ndiff + 1;                                           // :939 / :975
        if (phase == R1_STEP) {
            if (fabs(ff) < o.ftol) bits = R1_FCNVRG;                 // :978-981
            else if (fabs(dx) < o.xtol) bits = R1_XCNVRG;            // :982-985
            else if (fabs(df) < o.dtol) bits = R1_DCNVRG;            // :986-989
            else {
                if (ff < 0.0) xl = xv;                               // :992-997
                else xh = xv;
                r1_print(pr, p, iter, neval, ndiff, dx, ff);         // :999-1001
                if (neval >= o.max_evals) bits = R1_FLAG;            // :1004-1007
            }
        }
        top = bits == 0;
    }
    if (top) {
        iter = iter + 1;                                             // :942
        if ((((xv - xh) * df - ff) * ((xv - xl) * df - ff) > 0.0) || (fabs(2.0 * ff) > fabs(dxold * df))) {   // :946-948
            dxold = dx;                                              // :950
            dx = 0.5 * (xh - xl);                                    // :951
            xv = xl + dx;                                            // :952
            if (fabs(xl - xv) < o.xtol) bits = R1_XCNVRG;            // :953-957: no evaluation at the new x
        } else {
            dxold = dx;                                              // :960
            dx = ff / df;                                            // :961
            const double temp = xv;                                  // :962
            xv = xv - dx;                                            // :963
            if (fabs(temp - xv) < o.xtol) bits = R1_XCNVRG;          // :964-968: no evaluation at the new x
        }
    }
    S.s[NW_X][p] = xv; S.s[NW_XL][p] = xl; S.s[NW_XH][p] = xh; S.s[NW_FF][p] = ff;
    S.s[NW_DX][p] = dx; S.s[NW_DXOLD][p] = dxold;
    S.iter[p] = iter; S.neval[p] = neval; S.ndiff[p] = ndiff;
    if (!bits) {                                                     // f (and f') at x due
        S.pt0[p] = xv;
        S.phase[p] = phase == R1_ENDS ? R1_MID : R1_STEP;
        if (o.user_diff) return 1;
        S.pt1[p] = xv + r1_fd_step(xv);                              // :191: temp = x + h
        return 2;
    }
    S.bits[p] = bits;
    if (o.want_f) { S.pt0[p] = xv; S.phase[p] = R1_FINAL; return 1; }
    x[p] = xv;
    S.fo[p] = ff;
    S.phase[p] = R1_DONE;
    return 0;
}

// One advance of every problem, then the exclusive scan of the counts over the block (off[p]: the offset inside its run
// of 1024 problems, bsum[b]: the run's total).  off[p] holds, on entry, where the values of the last round's points are.
template <int KIND>
static __global__ void __launch_bounds__(1024)
k_r1_advance(int nprob, int first, R1Opts o, const double *__restrict__ lim, const double *__restrict__ fs,
             const double *__restrict__ ds, int32_t *__restrict__ off, R1Soa S, double *__restrict__ x,
             R1Print *__restrict__ pr, int32_t *__restrict__ cnt, int32_t *__restrict__ bsum)
{
    __shared__ int32_t sh[16];
    const int p = blockIdx.x * 1024 + threadIdx.x;
    int32_t c = 0;
    if (p < nprob) {
        if (pr) pr[p].due = 0;
        c = KIND == R1_BRENT ? brent_advance(p, first != 0, o, lim, fs, off, S, x, pr)
                             : newton_advance(p, first != 0, o, lim, fs, ds, off, S, x, pr);
    }
    int32_t tot;
    const int32_t ex = nm_block_excl_scan(c, sh, &tot);
    if (p < nprob) { off[p] = ex; cnt[p] = c; }
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// The points of the round into the compact list: problem p's cnt[p] points from off[p] + bpre[p / 1024] on, each with
// its problem index (pbase + p: the index in the caller's batch).  dneed (or NULL): whether the point wants the user's
// derivative too (newton's iterations; not its endpoints or its final evaluation).
static __global__ void __launch_bounds__(256)
k_r1_emit(int nprob, int32_t pbase, const double *__restrict__ pt0, const double *__restrict__ pt1,
          const int32_t *__restrict__ phase, const int32_t *__restrict__ cnt, int32_t *__restrict__ off,
          const int32_t *__restrict__ bpre, double *__restrict__ xs, int32_t *__restrict__ dprob, int32_t *__restrict__ dneed)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= nprob) return;
    const int32_t c = cnt[p];
    const int32_t o = off[p] + bpre[p >> 10];
    off[p] = o;                                                      // (what the next advance reads its values at)
    if (c == 0) return;
    xs[o] = pt0[p];
    dprob[o] = pbase + p;
    if (c > 1) { xs[o + 1] = pt1[p]; dprob[o + 1] = pbase + p; }
    if (dneed) {
        const int32_t ph = phase[p], need = ph == R1_MID || ph == R1_STEP;
        dneed[o] = need;
        if (c > 1) dneed[o + 1] = 0;
    }
}
