/* nonlin_hip_starts.h -- a part of the C ABI of libnonlin_hip.so: starts, the batched box scan that makes starting values for
 * any device model.  include/nonlin_hip.h includes this file, and this file includes that one, so either gives the whole ABI. */
#ifndef NONLIN_HIP_STARTS_H
#define NONLIN_HIP_STARTS_H

#include "nonlin_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- starts (no counterpart in nonlin v2.2.0): the cost sum F_i^2 of a residual launcher at the candidate points of a box,
 * for every problem of a batch at once, and the `keep` best candidates of each problem as starting values.  One box serves
 * every problem, as xl / xu of the one-call fits do.  No Fortran binding.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation:
 *   radical inverse  the unit coordinate u of candidate c in dimension d is the radical inverse of i = c + 1 in base p = p_d, the
 *               d-th prime (2, 3, 5, .. 131: at most NLH_STARTS_MAX_N dimensions):
 *                   f = 1.0/p;  r = +0.0;  while i > 0:  r = r + f*(i mod p);  i = i div p;  f = f/p
 *               (the Halton sequence, unscrambled: candidate 0 is (1/2, 1/3, 1/5, ..)).  It degrades as n grows -- high
 *               dimensions are correlated over the first candidates --: scan few dimensions (a separable model's nonlinear
 *               ones) or give the known parameters a tight box.
 *   linear      v = lo + u*(hi - lo)
 *   log         (logscale[d] != 0, needs 0 < lo):  v = lo*exp(u*log(hi/lo)), exp and log the host's libm
 *   clamp       either form: v < lo gives lo, v > hi gives hi.  lo == hi is allowed: the dimension is constant.
 *   cost        of a point's residuals F_0 .. F_{m-1}: 64 partials, partial j = +0.0 and then s = s + F_i*F_i over the rows
 *               i = j (mod 64) in ascending i; then for off = 32, 16, 8, 4, 2, 1:  s_j = s_j + s_{j+off} for j < off; the
 *               cost is s_0 (the lanes of one wave, combined as block_reduce_sum's shuffle tree combines them).
 *   selection   per problem the `keep` smallest FINITE costs with their candidate indices, ordered by (cost, index)
 *               ascending; a cost that is NaN or infinite is never kept.  (cost, index) is a total order on what can be kept,
 *               so the result does not depend on the chunks, the slices, the batch or the launch shape.  Fewer than `keep`
 *               finite costs: the remaining slots have cost +Inf, index -1 and a row of NaN.
 * nlh_starts_candidates: HOST code, no device.  cand [count][n] = the candidates first .. first + count - 1 of the box xl, xu
 * [n]; logscale [n] or NULL (every dimension linear).  Returns 0, or NLH_INVALID_INPUT_ERROR for: n < 1 or
 * n > NLH_STARTS_MAX_N, a NULL xl or xu (cand with count > 0), a bound that is not finite, lo > hi, a log dimension with
 * lo <= 0, count < 0, first < 0, first + count > NLH_STARTS_MAX_CAND.  A refused call writes nothing. ---- */
#define NLH_STARTS_MAX_N 32
#define NLH_STARTS_MAX_KEEP 8
#define NLH_STARTS_MAX_CAND 1048576
int nlh_starts_candidates(int32_t n, int32_t first, int32_t count, const double *xl, const double *xu, const int32_t *logscale,
                          double *cand);

/* The scan.  fcn, ctx: any residual launcher over n unknowns and m rows -- a user's, a model's, or one composed with the
 * wrapping launchers --; it is called with points in problem-major order, point q = (p - p0)*C + (c - c0) of a slice of
 * problems from p0 and a chunk of C candidates from c0, dprob[q] = p.  The residuals F [points][m] of one launcher call stay
 * within 256 MiB; the environment variable NLH_STARTS_POINTS, read at every call, sets the most points of one launcher
 * call instead (tests).  xl, xu, logscale: HOST arrays [n] as above.  dx0 [nprob][keep][n], dcost [nprob][keep],
 * dindex [nprob][keep] (int32): DEVICE arrays on the handle's stream, out.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (a NULL fcn, xl, xu, dx0, dcost or dindex, nprob < 0,
 * m < 1, ncand < 1, keep < 1, keep > NLH_STARTS_MAX_KEEP, keep > ncand, and everything nlh_starts_candidates(n, 0, ncand, ..)
 * refuses); the launcher's own nonzero return, passed through as it is.  A refused call writes nothing.  nprob == 0: 0. */
int nlh_starts_search_batch_device(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, void *ctx,
                                   const double *xl, const double *xu, const int32_t *logscale, int32_t ncand, int32_t keep,
                                   double *dx0, double *dcost, int32_t *dindex);
/* ... behind HOST arrays x0, cost, index; synchronises the stream.  (The launcher's data stay what they are: device data.) */
int nlh_starts_search_batch_device_h(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, void *ctx,
                                     const double *xl, const double *xu, const int32_t *logscale, int32_t ncand, int32_t keep,
                                     double *x0, double *cost, int32_t *index);

/* The pieces of a multi-start pick, DEVICE arrays on the handle's stream.  Errors of each: NLH_ERR_BAD_HANDLE, then
 * NLH_INVALID_INPUT_ERROR (a NULL array, a negative count, m < 1, width < 1, keep outside 1 .. NLH_STARTS_MAX_KEEP); a count
 * of 0 returns 0.
 * cost: dcost[q] = the cost, as stated above, of dF [npoints][m]. */
int nlh_starts_cost_batch(nlh_handle *h, int32_t npoints, int32_t m, const double *dF, double *dcost);
/* pick: dwhich[p] (int32) = the k of the smallest finite dcost[k][p], dcost [keep][nprob], the lowest k on a tie, -1 when
 * none is finite. */
int nlh_starts_pick_batch(nlh_handle *h, int32_t nprob, int32_t keep, const double *dcost, int32_t *dwhich);
/* take: ddst [nprob][width] = row dwhich[p] of dsrc [keep][nprob][width], NaN for -1. */
int nlh_starts_take_batch(nlh_handle *h, int32_t nprob, int32_t keep, int32_t width, const double *dsrc, const int32_t *dwhich,
                          double *ddst);

#ifdef __cplusplus
}
#endif
#endif /* NONLIN_HIP_STARTS_H */
