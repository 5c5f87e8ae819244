/* nonlin_hip_profile.h -- a part of the C ABI of libnonlin_hip.so: profile-likelihood intervals -- the pin pair, a pair of wrapping
 * launchers that holds one parameter per wrapped problem at its own value on shared data, and the lock-step root finder that
 * drives the pinned refits of every end of every interval at once.  include/nonlin_hip.h includes this file, and this file
 * includes that one, so either gives the whole ABI. */
#ifndef NONLIN_HIP_PROFILE_H
#define NONLIN_HIP_PROFILE_H

#include "nonlin_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the pin pair (no counterpart in nonlin v2.2.0): around any inner launcher pair over N unknowns and nprob problems, a
 * batch of `nend` wrapped problems of n = N - 1 unknowns.  Three DEVICE tables of length nend describe it, indexed by the
 * wrapped problem w = dprob ? dprob[q] : q of a point q:
 *   src[w]    (int32) the inner problem whose data the wrapped problem uses, 0 .. nprob - 1
 *   pos[w]    (int32) which of the N inner unknowns is pinned, 0 .. N - 1
 *   theta[w]  its value
 * ONLY COPIES HAPPEN: no floating-point operation is made on a parameter, a residual or a derivative.
 *   expand    P [npoints][N]:  P[q][k] = x[q][k] for k < pos[w],  theta[w] for k == pos[w],  x[q][k - 1] for k > pos[w]
 *   problems  a scratch list sp[q] = src[w]: the inner launchers are called with dprob = sp and n = N, so every layer inside --
 *             curve, formula, bin, conv, Poisson, loss, map -- selects the data of problem src[w]: any number of wrapped
 *             problems refit against the nprob data sets with no copy of y, t, weights, taps or scales
 *   fcn       expand; the inner fcn straight into the caller's dF
 *   jac       expand; the inner jac into scratch Jf [npoints][N][m]; dJ [npoints][N - 1][m]: column j of a point is column j of
 *             Jf for j < pos[w], column j + 1 otherwise.  With a NULL inner jac it returns NLH_UNDEFINED_FUNCTION_ERROR.
 * So, with a constant pos, a row's bits are those of nlh_pmap_device_fcn / _jac under a map with that one parameter fixed and
 * full = theta, on data replicated by hand.
 * Scratch belongs to the context, by the rules of nlh_pmap_wrap: one buffer per stream, grown on demand, kept until
 * nlh_pin_unwrap, at most 1 GiB; a call that needs more runs in slices of points, with the same bits.  The environment variable
 * NLH_PIN_SCRATCH (bytes, read at every call) lowers the cap: tests.  The launchers never synchronise and may be called from
 * several host threads on different streams.
 * nlh_pin_wrap: N the inner unknowns.  Errors: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (a NULL out, N < 2, nend < 0, a NULL
 * table); NLH_UNDEFINED_FUNCTION_ERROR (a NULL fcn).  nlh_pin_set swaps the three tables and nend between solves -- never while
 * a launcher of the context is being called --; it touches no scratch and launches nothing.  Errors: NLH_INVALID_INPUT_ERROR
 * (no live context, nend < 0, a NULL table).  The tables stay the caller's, are read by the launchers' kernels, and must live
 * until the work that reads them is done.  An entry of pos or src out of range is the caller's error: it is not checked on the
 * device.  The launchers refuse before any launch: n != N - 1, m < 1, a NULL dX or output: NLH_INVALID_INPUT_ERROR. ---- */
typedef struct nlh_pin_ctx nlh_pin_ctx;
int  nlh_pin_wrap(nlh_handle *h, int32_t N, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx, int32_t nend,
                  const int32_t *dsrc, const int32_t *dpos, const double *dtheta, nlh_pin_ctx **out);
int  nlh_pin_set(nlh_pin_ctx *c, int32_t nend, const int32_t *dsrc, const int32_t *dpos, const double *dtheta);
void nlh_pin_unwrap(nlh_pin_ctx *c);
int  nlh_pin_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF);
int  nlh_pin_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ);

/* ---- the root finder of the profile-likelihood interval (MINOS; lmfit's conf_interval): for every problem p, parameter j and
 * side s (0: below the fit, 1: above) the value theta of parameter j at which the cost of the refit of all the OTHER parameters
 * has risen by delta over the fit's cost C0.  An end is e = (p*n + j)*2 + s; every per-end array is [nprob][n][2].  The caller
 * makes the refits (the pin pair and any solver) and hands their costs in; all ends advance in lock step.  No Fortran binding.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, nothing fused; rc = sqrt(crit) is taken once, on the
 * host.  The state is plain DEVICE arrays the caller owns: */
typedef struct nlh_profile_state {
    double *C0, *delta;                  /* [nprob]  the fit's cost; the rise that defines the interval */
    double *xhat, *width, *bound;        /* per end: x_j of the fit; rc*sigma_j; the side's bound (-Inf / +Inf: none) */
    double *theta;                       /* per end: the trial value the next refit is pinned at */
    double *a, *ga, *b, *gb;             /* per end: the bracket -- a inside (g < 0), b outside (g > 0) -- and its g */
    double *end;                         /* per end: the result */
    int32_t *phase, *flag, *last, *nexp, *nev, *nfail;   /* per end */
} nlh_profile_state;
/*   phase       NLH_PROFILE_EXPAND, NLH_PROFILE_BRACKET, NLH_PROFILE_DONE
 *   flag        of a finished end, one of the codes below, plus the bit NLH_PROFILE_LOWER; 0 while the end runs
 *   last        the side of the bracket the last evaluation replaced: -1 a, +1 b, 0 none yet
 *   nexp, nev, nfail   doublings made; evaluations handed in, failed ones included; failed refits in a row
 * start         C0[p] = the cost of fcn at x[p] (one call, point q of problem q) by the stated order of nlh_starts_cost_batch;
 *               dof = ddof ? ddof[p] : m - n;   delta[p] = scaled ? (crit*C0)/dof : crit;   per end:
 *                   xhat = x[p][j];  width = rc*sigma[p][j];  bound = s ? xu[j] : xl[j]  (a NULL xl or xu: -Inf, +Inf)
 *                   a = xhat;  ga = -delta;  b = gb = NaN;  last = nexp = nev = nfail = 0
 *                   theta = s ? xhat + width : xhat - width,  then clipped:  s = 0: theta < bound gives bound;  s = 1: theta > bound
 *               NLH_PROFILE_NO_START, end NaN:  xhat, sigma, C0 or delta not finite, sigma, C0 or delta <= 0, dof <= 0, crit not
 *               finite or <= 0.  Otherwise NLH_PROFILE_ON_BOUND, end = bound:  s = 0: xhat <= bound;  s = 1: xhat >= bound.
 *               Both are finished at once; every other end is in phase EXPAND.
 * step          of an active end with the cost c of its refit at theta and fail != 0 for a refit that did not end well:
 *                   nev = nev + 1
 *               failed (fail != 0, or c not finite):  nfail = nfail + 1;  nfail > 3: NLH_PROFILE_FIT_FAILED, end NaN;  else
 *                   d = theta - a;  d = d*0.5;  theta = a + d   -- the bracket is left alone, and nothing below happens
 *               else  nfail = 0;   t = tol*delta;   g = (c - C0) - delta;   c < C0 - t sets the bit NLH_PROFILE_LOWER (the x handed
 *                   in was not the minimum);   |g| <= t:  NLH_PROFILE_OK, end = theta.   Otherwise
 *               EXPAND, g < 0:   a = theta;  ga = g;   theta == bound: NLH_PROFILE_OPEN_AT_BOUND, end = bound;   nexp >= max_expand:
 *                   NLH_PROFILE_OPEN, end = s ? +Inf : -Inf;   else nexp = nexp + 1;  d = theta - xhat;  d = 2*d;  theta = xhat + d,
 *                   clipped as at the start
 *               EXPAND, g > 0:   b = theta;  gb = g;  last = +1;  phase = BRACKET;  then the false position below
 *               BRACKET (Illinois):  g < 0:  a = theta;  ga = g;  if last == -1:  gb = gb*0.5;   last = -1
 *                                    g > 0:  b = theta;  gb = g;  if last == +1:  ga = ga*0.5;   last = +1
 *               false position:  u = a*gb;  v = b*ga;  u = u - v;  v = gb - ga;  theta = u/v;   a theta that is not strictly between
 *                   a and b (rounding):  d = b - a;  d = d*0.5;  theta = a + d.    |b - a| <= xtol*width:  NLH_PROFILE_OK, end = theta
 *               an end still running with nev >= maxit:  NLH_PROFILE_MAXIT, end = theta (in BRACKET the last false position)
 * The result of an end depends on its own costs alone: not on which other ends are active, nor on the launch shape. */
#define NLH_PROFILE_EXPAND 0
#define NLH_PROFILE_BRACKET 1
#define NLH_PROFILE_DONE 2
#define NLH_PROFILE_OK 0
#define NLH_PROFILE_OPEN 1
#define NLH_PROFILE_OPEN_AT_BOUND 2
#define NLH_PROFILE_ON_BOUND 3
#define NLH_PROFILE_MAXIT 4
#define NLH_PROFILE_FIT_FAILED 5
#define NLH_PROFILE_NO_START 6
#define NLH_PROFILE_NOT_FREE 7        /* set by the one-call profiles of a mapped fit at fixed and tied positions, never here */
#define NLH_PROFILE_LOWER 16

/* start.  fcn, ctx: the UNPINNED residual launcher over n unknowns and m rows.  dx, dsigma [nprob][n], ddof [nprob] (int32) or NULL:
 * DEVICE arrays on the handle's stream; xl, xu: HOST arrays [n] or NULL, one box for every problem.  Errors, in this order:
 * NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (nprob < 0, m < 1, n < 1, a NULL dx, dsigma, st or array of st, nprob*n*2 above
 * 2^31 - 1); NLH_UNDEFINED_FUNCTION_ERROR (a NULL fcn); the launcher's own nonzero return.  nprob == 0: 0. */
int nlh_profile_start_batch_device(nlh_handle *h, nlh_device_vecfcn fcn, void *ctx, int32_t nprob, int32_t m, int32_t n,
                                   const double *dx, const double *dsigma, const int32_t *ddof, double crit, int32_t scaled,
                                   const double *xl, const double *xu, const nlh_profile_state *st);
/* step.  dact [nact] (int32): the active ends, each at most once; dcost [nact], dfail [nact] (int32) or NULL (none failed): the
 * refits' costs, entry i that of end dact[i].  An entry of dact that is out of range or names a finished end is skipped.
 * *nleft: how many of the nprob*n*2 ends are still running after the step; the stream is synchronised to read it.  Errors:
 * NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (nprob < 0, n < 1, nprob*n*2 above 2^31 - 1, nact < 0, a NULL dact or dcost with
 * nact > 0, a NULL st, array of st or nleft, tol or xtol negative or not finite, max_expand < 0, maxit < 1). */
int nlh_profile_step_batch(nlh_handle *h, int32_t nprob, int32_t n, int32_t nact, const int32_t *dact, const double *dcost,
                           const int32_t *dfail, const nlh_profile_state *st, double tol, double xtol, int32_t max_expand,
                           int32_t maxit, int32_t *nleft);

#ifdef __cplusplus
}
#endif
#endif /* NONLIN_HIP_PROFILE_H */
