/* nonlin_hip_guess.h -- a part of the C ABI of libnonlin_hip.so: starting values for the built-in curve models.
 * include/nonlin_hip.h includes this file, and this file includes that one, so either gives the whole ABI. */
#ifndef NONLIN_HIP_GUESS_H
#define NONLIN_HIP_GUESS_H

#include "nonlin_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- starting values for the built-in curve models (no counterpart in nonlin v2.2.0): x0 for nlh_curve_fit_batch and its
 * variants from the data alone, batched, deterministic, on the device.  Two stages.  The NONLINEAR stage estimates mu and the
 * width of each peak, or k of each decay (ncomp <= 2).  The LINEAR stage is nlh_sep_solve_batch on nlh_curve_device_fcn /
 * nlh_curve_device_jac over the caller's t, y, w with the amplitudes and the baseline coefficients declared linear: x is the
 * best linear fit at the guessed nonlinear values, weights honoured.  Peaks are positive (no dips); components come out in the
 * order found.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation, no library function but sqrt:
 *   valid rows  those with w != 0 (all without weights), compacted in ascending index to t', y' of length mv; the nonlinear
 *               stage sees only these and reads w only as that mask.  NLH_GUESS_NONE, the whole row of x NaN, when mv < n, a
 *               valid t' or y' is not finite, or t' is not strictly ascending.
 *   every sum   below is sequential: s = +0.0, then s = s + a_i in ascending i
 *   PEAKS (NLH_CURVE_GAUSS, NLH_CURVE_LORENTZ)
 *   detrend     E = max(1, mv/16) (integer division); yl, tl = (sum over the first E rows)/E of y', t'; yr, tr the same over
 *               the last E.  B = -1: d = y'.  B = 0: d = y' - 0.5*(yl + yr).  B >= 1: c1 = (yr - yl)/(tr - tl);
 *               c0 = yl - c1*tl;  d = y' - (c0 + c1*t')
 *   smooth      h = smooth: s_i = (sum of d over max(0, i-h) .. min(mv-1, i+h)) / count; h = 0: s = d
 *   component   k = 0 .. K-1.  Every row starts live.  i* = the argmax of s over the live rows that are not NaN, the lowest
 *               index on ties (no such row: i* = 0 and a = -inf);  a = s[i*];  half = 0.5*a;  mu = t'[i*].
 *               Right crossing: the lowest j > i* that is dead or has s_j < half; if it is live
 *               tR = t'[j-1] + ((t'[j] - t'[j-1])*(s[j-1] - half))/(s[j-1] - s[j]); dead or past the end: none.  Left
 *               crossing: the highest j < i* that is dead or has s_j < half; if it is live
 *               tL = t'[j+1] - ((t'[j+1] - t'[j])*(s[j+1] - half))/(s[j+1] - s[j]).
 *               F = tR - tL with both;  2.0*(tR - mu) or 2.0*(mu - tL) with one.  With none, with a <= 0 or with F not
 *               positive and finite: F = 0.5*(t'[mv-1] - t'[0]) and the flag NLH_GUESS_FALLBACK.
 *   width       GAUSS: sigma = F/2.3548200450309493; then every row with |t' - mu| <= 1.5*F is dead.
 *               LORENTZ: w = 0.5*F; then s = s - a/(1.0 + dd*dd) with dd = (t' - mu)/w on every row, and row i* is dead.
 *   DECAYS (NLH_CURVE_EXPDECAY, K <= 2): the integral-equation regression
 *   integrate   q_0 = +0.0;  q_i = (0.5*(y'_i + y'_{i-1}))*(t'_i - t'_{i-1}).  S1 = the inclusive prefix sum of q in this one
 *               order: c = ceil(mv/256); chunk j = the rows [j*c, min((j+1)*c, mv)); inside a chunk l = +0.0, l = l + q_i
 *               ascending; o_0 = +0.0, o_j = o_{j-1} + (the last l of chunk j-1);  S1_i = o_j + l_i.  K = 2: S2 the same from
 *               S1 in the place of y'.
 *   panel       m rows; columns S1, (S2), u^0 .. u^deg with u = t'_i - t'_0, deg = K + B, the powers by p = 1; column = p;
 *               p = p*u;  f0 = -y';  rows >= mv are +0.0 everywhere
 *   regress     c = exactly the unpivoted Householder QR and solve of nlh_sep_* (nonlin_hip.h) on [panel | f0]: its sum order, its
 *               dead-column rule, its back-substitution (the same device routine)
 *   rates       K = 1: k = -c_0.  K = 2: A = c_0, Bc = c_1;  disc = A*A + 4.0*Bc;  r = sqrt(disc);  k_1 = 0.5*(r - A);
 *               k_2 = (-Bc)/k_1 (the fast rate first).  A rate that is not finite and positive, or a dead panel column:
 *               span = t'[mv-1] - t'[0], k = 2.0/span (K = 1) or (8.0/span, 1.0/span), and NLH_GUESS_FALLBACK
 *   LINEAR STAGE, all kinds: dfull of nlh_sep_solve_batch at the guessed values is x; rank < the linear parameters:
 *               NLH_GUESS_RANKDEF (the dead amplitude is +0.0).  NLH_GUESS_NONE problems are NaN and carry no other flag.
 * One workgroup of 256 threads per problem; the valid rows, s and the dead mask live in LDS (17 m bytes, so m <= 8192).  The
 * only floating-point sums are the per-row ones above; what crosses threads -- the argmax, the crossing searches -- is exact
 * in any order, so a problem's bits do not depend on the launch, the batch or the slice.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (a bad kind or counts, a NULL dt, dy or dx, smooth < 0,
 * m > NLH_GUESS_MAX_M, peaks with K + B + 1 > NLH_SEP_MAX_L, decays with K > 2); NLH_UNDERDEFINED_PROBLEM_ERROR (m < n).
 * dt [nprob][m] (shared_t: [m]), dy, dw (NULL: no weights) [nprob][m], dx [nprob][n] out, dflag [nprob] out (may be NULL):
 * DEVICE arrays on the handle's stream. ---- */
#define NLH_GUESS_MAX_M 8192
#define NLH_GUESS_FALLBACK 1   /* some nonlinear value is the documented fallback */
#define NLH_GUESS_RANKDEF  2   /* the linear solve found a dead column: that amplitude is +0.0 */
#define NLH_GUESS_NONE     4   /* not guessed: the row of x is NaN */
int nlh_curve_guess_batch(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *dt,
                          int32_t shared_t, const double *dy, const double *dw, int32_t smooth, double *dx, int32_t *dflag);
/* ... behind HOST arrays t, y, w, x, flag; synchronises the stream. */
int nlh_curve_guess_batch_h(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *t,
                            int32_t shared_t, const double *y, const double *w, int32_t smooth, double *x, int32_t *flag);

#ifdef __cplusplus
}
#endif
#endif /* NONLIN_HIP_GUESS_H */
