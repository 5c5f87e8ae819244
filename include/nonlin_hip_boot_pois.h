/* nonlin_hip_boot_pois.h -- a part of the C ABI of libnonlin_hip.so: the Poisson bootstrap, the parametric count replicas of a
 * fit of counting data (stat = Poisson).  include/nonlin_hip.h includes this file, and this file includes that one, so either
 * gives the whole ABI.  It continues nonlin_hip_boot.h -- the generator, the stream keys and the summary are stated there --
 * and is a header of its own because that one lists exactly the entry points of the resampling kinds. */
#ifndef NONLIN_HIP_BOOT_POIS_H
#define NONLIN_HIP_BOOT_POIS_H

#include "nonlin_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Poisson bootstrap (no counterpart in nonlin v2.2.0): replica b of problem p holds, in every active row i, a count
 * y*_i ~ Poisson(mu_i) drawn from the fitted value mu_i; the refits minimise the same deviance as the fit.  The resampling
 * kinds of nonlin_hip_boot.h are wrong for counts -- a resampled residual added to a fitted value is not a count and can be
 * negative --, which is why nlh_boot_resample_batch has no fourth kind and this is a function of its own.  No Fortran binding.
 * THE ARITHMETIC IS PART OF THE INTERFACE, as there: integers mod 2^64 from mix / key / draw of nonlin_hip_boot.h, then + - * /,
 * floor and comparisons, one IEEE operation per step, no library function and no fused operation.  That excludes exp, log and
 * lgamma and with them the usual rejection samplers; what is left is inversion FROM THE MODE with unnormalised weights --
 * weight 1 at M = floor(mu), every other weight from its neighbour's: below the mode by two multiplications, the second with the
 * reciprocal r = 1/mu taken once per row, above it by one multiplication and one division by k --, which needs no normalising
 * constant and walks O(sqrt(mu)) steps per draw.
 *   EPS = 2^-60
 *   setup       of a row, from mu alone (the same for every replica):
 *                   M = floor(mu);  r = 1/mu
 *                   L = 0; q = 1; nd = 0;  for k = M, M-1, .., 1:  q = (q*k)*r;  if q < EPS stop;  L = L + q;  nd = nd + 1
 *                   U = 1; q = 1; nu = 0;  for k = M+1, M+2, ..:   q = (q*mu)/k;  if q < EPS stop;  U = U + q;  nu = nu + 1
 *                   T = L + U;  kmin = M - nd;  kmax = M + nu
 *               (L: the weights below the mode, descending from M-1; U: the mode's and those above it)
 *   draw        of row i -- draw k = i, the ROW number, of the stream (seed, p, b), as `wild` takes it --:
 *                   z = mix(key + G*(i + 1));   u = (z >> 11)*2^-53;   t = u*T
 *                   if t < L:  s = L - t;  k = M - 1;  q = M*r;   while s >  q and k > kmin:  s = s - q;  q = (q*k)*r;   k = k - 1
 *                   else:      s = t - L;  k = M;      q = 1;     while s >= q and k < kmax:  s = s - q;  k = k + 1;  q = (q*mu)/k
 *                   y*_i = (double)k
 *               Both walks end for every input: the guards keep k inside [kmin, kmax], a subset of [0, M + nu], and every step
 *               moves k by one.  (In exact arithmetic q falls strictly once k has left M -- k < mu below the mode, k > mu
 *               above it --, so the guards only catch what rounding leaves of s at the end of a tail.)  The setup's loops
 *               end, too: the first at k = 1 at the latest, the second because mu/k <= (M+1)/(M+2) < 1 from its second
 *               step on while q >= EPS is far above the subnormal numbers: about 9 sqrt(mu) + 60 steps at the most.
 *               Why r and not a division by mu below the mode: the fp64 division is the walks' cost, and the steps below the
 *               mode all divide by the same mu.  On an MI355X (profiles/boot_pois_rate.txt) 16,384 x 128 rows x 64 replicas took
 *               0.886, 2.54, 10.9 and 108 ms at mu ~ 5, 50, 1000 and 10^5 with (q*k)/mu and take 0.71, 1.83, 7.46 and 72.9 ms with
 *               (q*k)*r (a short shape, 128 x 32 x 64, is some microseconds slower with r: the file has both).  The steps above the mode divide by k, which changes, and keep their division.  r carries one rounding
 *               more into every weight below the mode: a relative 2^-53 per step over at most 9 sqrt(mu) steps, below 1e-11,
 *               far inside what 10^5 draws can tell (the chi-square table of DESIGN.md 4o was made with r).
 *   rows        inactive: w_i == 0 (no row is inactive without weights; with stat = Poisson the weights are its 0 / 1 mask):
 *               a copy of y_i.   zero: mu_i == 0, of either sign: +0.0.   bad: an ACTIVE row whose mu_i is a NaN, below 0 or
 *               above NLH_BOOT_POIS_MAX_MEAN = 2^24: a copy of y_i, and one more in the problem's count of bad rows.  ordinary:
 *               every other row, drawn as above.  Above 2^24 the skewness 1/sqrt(mu) is below 2.5e-4 and the walk above 3,000
 *               steps: there NLH_BOOT_WILD with the weights 1/sqrt(mu) serves.
 *   A replica depends on (seed, p, b, mu) alone: not on the batch, the slice, the chunks or the launch shape.
 * nlh_boot_poisson_draws: HOST code, no device.  out [count]: out[j] = the draw of row first + j of the stream (seed, p, b) for
 * the mean mu[j]; a bad mu[j] gives a NaN (there is no y to copy).  Returns 0, or NLH_INVALID_INPUT_ERROR for: p < 0, b < 0,
 * first < 0, count < 0, first + count > NLH_BOOT_MAX_ROWS, a NULL mu or a NULL out with count > 0.  A refused call writes
 * nothing. ---- */
#define NLH_BOOT_POIS_MAX_MEAN 16777216
int nlh_boot_poisson_draws(uint64_t seed, int64_t p, int32_t b, int32_t first, int32_t count, const double *mu, double *out);

/* The replicas b = rep0 .. rep0 + nrep - 1 of the problems prob0 .. prob0 + nprob - 1 of the caller's whole data, of which the
 * arrays hold that slice, in the layout of nlh_boot_resample_batch.  DEVICE arrays on the handle's stream: dmu (fitted values),
 * dy (data), dw (weights, or NULL: none) [nprob][m], in; dyout [nrep][nprob][m], out, replica-major; dbad [nprob] (int32), out:
 * the number of bad rows of each problem -- the same for every replica, written once per call.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (nprob < 0, nrep < 0, nrep > NLH_BOOT_MAX_REP, m < 1,
 * m > NLH_BOOT_MAX_ROWS, prob0 < 0, rep0 < 0, rep0 + nrep > 2^31 - 1, a NULL dmu, dy, dyout or dbad).  A refused call writes
 * nothing.  nprob == 0 or nrep == 0: 0, and nothing is written. */
int nlh_boot_poisson_batch(nlh_handle *h, uint64_t seed, int32_t nprob, int64_t prob0, int32_t m, int32_t rep0, int32_t nrep,
                           const double *dmu, const double *dy, const double *dw, double *dyout, int32_t *dbad);

#ifdef __cplusplus
}
#endif
#endif /* NONLIN_HIP_BOOT_POIS_H */
