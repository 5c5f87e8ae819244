/* nonlin_hip_boot.h -- a part of the C ABI of libnonlin_hip.so: bootstrap, the resampled-data confidence intervals of any fit.
 * include/nonlin_hip.h includes this file, and this file includes that one, so either gives the whole ABI. */
#ifndef NONLIN_HIP_BOOT_H
#define NONLIN_HIP_BOOT_H

#include "nonlin_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- bootstrap (no counterpart in nonlin v2.2.0): nrep resampled copies ("replicas") of every data set of a batch, made on
 * the device from the data and the fitted values, and the reduction of the nrep parameter sets that the refits of those
 * replicas give to a mean, a standard deviation and a percentile interval per parameter.  The refits themselves are the
 * library's ordinary batched fits: a block of replicas is an ordinary batch.  No Fortran binding.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- integers mod 2^64 in the generator, one IEEE operation per step and no fused
 * operation elsewhere:
 *   mix         mix(z):  z = (z xor (z >> 30))*0xBF58476D1CE4E5B9;  z = (z xor (z >> 27))*0x94D049BB133111EB;
 *               z = z xor (z >> 31)      (the finaliser of splitmix64);  G = 0x9E3779B97F4A7C15
 *   stream key  of problem p -- its index in the caller's WHOLE data: a slice passes prob0 -- and replica b:
 *                   key = mix(mix(seed + G*(p + 1)) + G*(b + 1))
 *   draw        k of that stream:  z = mix(key + G*(k + 1));   an index below cnt:  j = ((z >> 32)*cnt) >> 32;   a sign: bit
 *               63 of z.  No floating point is involved, so a replica depends on (seed, p, b) alone: not on the batch, the
 *               slice, the chunks or the launch shape.
 *   active rows the rows with w != 0 (every row without weights), cnt of them, numbered 0 .. cnt-1 in ascending row order.
 *               cnt == 0: every kind's replica is a copy of the data (and of the weights).
 *   residual    e_i = w_i*(y_i - mu_i)  (y_i - mu_i without weights) on the active rows.  With centre != 0:  e_i = e_i - ebar,
 *               ebar = S/cnt, S the sum of the e_i in the order of the starts cost (nonlin_hip_starts.h): 64 partials, partial
 *               j = +0.0 and then s = s + e_i over the ACTIVE rows i = j (mod 64) in ascending i; then for off = 32, 16, .. 1:
 *               s_j = s_j + s_{j+off} for j < off; S = s_0.  The active row i, of active number a, takes draw k = a, an index j
 *               below cnt, and  y*_i = mu_i + e_J/w_i  (mu_i + e_J without weights), J the active row of number j.  An
 *               inactive row copies y_i.
 *   wild        the active row i takes the sign of draw k = i (its ROW number):  d = y_i - mu_i;  y*_i = mu_i + d with the
 *               bit clear, mu_i - d with it set.  Weights only say which rows are active; an inactive row copies y_i.  For
 *               noise whose size varies along the rows.
 *   pairs       the draws k = 0 .. cnt-1, each an index below cnt; c_a = how often a was drawn (an integer histogram: the
 *               order of the additions cannot matter);  w*_i = w_i*sqrt(c_a)  (sqrt(c_a) without weights) for the active row i
 *               of number a,  w*_i = w_i  for an inactive one;  y* = y.
 *   summary     a replica of a problem is VALID when all n of its parameters are finite; cnt of the nrep are.  Per problem and
 *               parameter the valid values are sorted ascending by IEEE <, equal values (+0.0 and -0.0 are equal) in
 *               ascending replica order: x_0 .. x_{cnt-1}.   mean = S/cnt,  S = the sum of the x_i in that order, 64 partials
 *               and the tree as above (i the position in the sorted order);   sd = sqrt(Q/(cnt - 1)),  Q the same sum of
 *               d_i*d_i,  d_i = x_i - mean.   q_lo = (1 - level)/2 and q_hi = 1 - q_lo, computed on the host; a quantile q is
 *                   h = q*(cnt - 1);  k = floor(h);  g = h - k;  v = x_k + g*(x_{min(k+1, cnt-1)} - x_k)
 *               cnt == 0: mean, sd, lo and hi are NaN.  cnt == 1: the same formulas, which give NaN for sd (0/0).
 * nlh_boot_draws: HOST code, no device.  out [count] = the draws k = first .. first + count - 1 of the stream (seed, p, b): the
 * indices below cnt, or with cnt == 0 the sign bits as 0 / 1.  Returns 0, or NLH_INVALID_INPUT_ERROR for: p < 0, b < 0,
 * first < 0, count < 0, first + count > NLH_BOOT_MAX_ROWS, cnt < 0, cnt > NLH_BOOT_MAX_ROWS, a NULL out with count > 0.  A
 * refused call writes nothing. ---- */
#define NLH_BOOT_RESIDUAL 0
#define NLH_BOOT_WILD 1
#define NLH_BOOT_PAIRS 2
#define NLH_BOOT_MAX_ROWS 16384
#define NLH_BOOT_MAX_REP 4096
int nlh_boot_draws(uint64_t seed, int64_t p, int32_t b, int32_t first, int32_t count, int32_t cnt, int32_t *out);

/* The replicas b = rep0 .. rep0 + nrep - 1 of the problems prob0 .. prob0 + nprob - 1 of the caller's whole data, of which the
 * arrays hold that slice.  DEVICE arrays on the handle's stream: dmu (fitted values), dy (data), dw (weights, or NULL: none)
 * [nprob][m], in; dyout [nrep][nprob][m], out, replica-major: a block of replicas is a batch of nrep*nprob problems for a
 * fit.  dwout [nrep][nprob][m]: out, written by NLH_BOOT_PAIRS only, which needs it; the other kinds do not look at it.
 * dmu is not read by NLH_BOOT_PAIRS and may be NULL there.  centre is read by NLH_BOOT_RESIDUAL only.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (a kind that is none of the three, nprob < 0, nrep < 0,
 * nrep > NLH_BOOT_MAX_REP, m < 1, m > NLH_BOOT_MAX_ROWS, prob0 < 0, rep0 < 0, rep0 + nrep > 2^31 - 1, a NULL dy or dyout, a
 * NULL dmu unless pairs, a NULL dwout with pairs).  A refused call writes nothing.  nprob == 0 or nrep == 0: 0. */
int nlh_boot_resample_batch(nlh_handle *h, int32_t kind, uint64_t seed, int32_t nprob, int64_t prob0, int32_t m, int32_t rep0,
                            int32_t nrep, const double *dmu, const double *dy, const double *dw, int32_t centre, double *dyout,
                            double *dwout);

/* The reduction of dxs [nrep][nprob][n], the parameters the refits of the replicas gave (a failed refit: a row that holds a
 * NaN), to dmean, dsd, dlo, dhi [nprob][n] and dnvalid [nprob] (int32), as stated under `summary`; lo and hi are the q_lo and
 * q_hi quantiles of `level`.  DEVICE arrays on the handle's stream.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (nrep < 1, nrep > NLH_BOOT_MAX_REP, nprob < 0, n < 1, a
 * level that is not inside (0, 1), a NULL array); NLH_ARRAY_SIZE_ERROR (nprob*n or nprob*nrep of 2^31 or more).  A refused call
 * writes nothing.  nprob == 0: 0. */
int nlh_boot_summary_batch(nlh_handle *h, int32_t nrep, int32_t nprob, int32_t n, const double *dxs, double level, double *dmean,
                           double *dsd, double *dlo, double *dhi, int32_t *dnvalid);

#ifdef __cplusplus
}
#endif
#endif /* NONLIN_HIP_BOOT_H */
