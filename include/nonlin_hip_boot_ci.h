/* nonlin_hip_boot_ci.h -- a part of the C ABI of libnonlin_hip.so: the studentised (bootstrap-t) and the BCa (bias-corrected and
 * accelerated) intervals of the bootstrap.  include/nonlin_hip.h includes this file, and this file includes that one, so either
 * gives the whole ABI.  It continues nonlin_hip_boot.h: `summary's sort`, `summary's quantile` and `the 64-partial sum and tree`
 * mean exactly what that header states under `summary` and `residual`. */
#ifndef NONLIN_HIP_BOOT_CI_H
#define NONLIN_HIP_BOOT_CI_H

#include "nonlin_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the two textbook corrections of the percentile interval (no counterpart in nonlin v2.2.0), as reductions of the refits
 * that the bootstrap already makes: the bootstrap-t interval, studentised by every refit's own standard error, and the BCa
 * interval, whose acceleration comes from a delete-one jackknife -- m more refits per data set, each with one row's weight
 * set to zero.  The refits are the library's ordinary batched fits.  No Fortran binding.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation.  q_lo = (1 - level)/2 and
 * q_hi = 1 - q_lo are computed on the host.
 *   student     xs, sigs [nrep][nprob][n]: the refits and their standard errors; x, sigma [nprob][n]: the fit handed in.
 *               Replica b is VALID for the pair (p, j) when all n of xs[b][p] are finite (summary's rule: a row counts whole)
 *               and sigs[b][p][j] is finite and > 0; cnt_t[p][j] of the nrep are.  t_b = (xs_b - x)/sigs_b over the valid
 *               replicas, sorted with summary's sort; T_lo and T_hi are summary's quantiles of q_lo and q_hi;
 *                   lo = x - T_hi*sigma;   hi = x - T_lo*sigma
 *               cnt_t == 0, an x or a sigma that is not finite, or sigma <= 0: lo and hi are NaN.
 *   jackknife   for the rows row0 .. row0 + nrows - 1:  wout[r][p][i] = +0.0 for i == row0 + r, otherwise w[p][i] (1.0 where
 *               there are no weights).  Row-major over the deletions: a block of deletions is a batch for a fit.
 *   accel       xjack [m][nprob][n]: the refits with row i deleted.  Deletion i of problem p is VALID when row i is active
 *               (w[p][i] != 0, or no weights) and all n of xjack[i][p] are finite; njack[p] of the m are.  Per (p, j):
 *               mean = S/njack, S the 64-partial sum and tree of the values over the valid i (partial i mod 64, ascending i);
 *               d_i = mean - xjack_i;  S2 the same sum of d_i*d_i;  S3 the same sum of (d_i*d_i)*d_i;
 *                   a = S3/(6.0*(S2*sqrt(S2)))
 *               njack < 2, S2 == 0 or an a that is not finite: a = +0.0.
 *   ppnd16      Wichura's algorithm AS 241 (Applied Statistics 37 (1988) 477-484), z = ppnd16(p) for 0 < p < 1, every
 *               polynomial in Horner form from the highest coefficient down, one multiplication and one addition per step:
 *                 q = p - 0.5.  |q| <= 0.425:  r = 0.180625 - q*q;  z = (A(r)*q)/B(r)    -- no library function is reached --
 *                 A = 2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
 *                     1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0
 *                 B = 5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
 *                     5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0
 *                 otherwise  r = p for q <= 0 and 1.0 - p for q > 0;  r = sqrt(-log(r))  with the library's log and sqrt;
 *                 r <= 5.0:  r = r - 1.6;  z = C(r)/D(r);   r > 5.0:  r = r - 5.0;  z = E(r)/F(r);   q < 0: z = -z
 *                 C = 7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
 *                     3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0
 *                 D = 1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
 *                     6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0
 *                 E = 2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
 *                     2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0
 *                 F = 2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
 *                     1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0
 *   bca         validity and sort are summary's: cnt valid replicas, sorted x_0 .. x_{cnt-1}; xhat = x[p][j], the fit handed in.
 *                 c2 = 2*#{x_b < xhat} + #{x_b == xhat}  (an integer);  u = c2/(2*cnt);  z0 = ppnd16(u)
 *               and for each z of z_lo = ppnd16(q_lo), z_hi = ppnd16(q_hi) (computed on the host by the same routine):
 *                 s = z0 + z;  den = 1.0 - a*s;  w = z0 + s/den;  alpha = 0.5*erfc(-(w*0.70710678118654752))
 *               with the library's erfc; lo and hi are summary's quantile formula at alpha_lo and alpha_hi (k kept inside
 *               0 .. cnt-1).  flags, an int32 per pair, OR-ed, looked at in this order:
 *                 NLH_BCA_NO_REPLICA (8)  cnt == 0 or an xhat that is not finite: lo, hi, z0, alpha_lo, alpha_hi are NaN and no
 *                                         other bit is set
 *                 NLH_BCA_NO_ACCEL (2)    the a handed in is not finite: a is taken as 0
 *                 NLH_BCA_DEGENERATE (1)  c2 == 0 or c2 == 2*cnt: z0 = -Inf or +Inf is stored and both alphas are q_lo / q_hi --
 *                                         the percentile interval; bit 4 is then not looked at
 *                 NLH_BCA_BAD_DENOM (4)   not den > 0 at either end: that end's alpha is the unadjusted q
 *               What is exact: c2, cnt, u, the flags, and z0 where |u - 0.5| <= 0.425.  What goes through a library function
 *               -- z0 in the tails (log), alpha (erfc), z_lo and z_hi (the host's log) -- is the device's or the host's
 *               library's: with erfc and log good to 8 ulp an error of z0 enters alpha with a factor of at most
 *               0.4*(1 + 1/den^2), so that for |a*(z0 + z)| <= 1/2 and 0 < c2 < 2*cnt two implementations' alphas agree
 *               within 2^-44 absolute; lo and hi are exact GIVEN the alphas that come back with them. ---- */
#define NLH_BCA_DEGENERATE 1
#define NLH_BCA_NO_ACCEL 2
#define NLH_BCA_BAD_DENOM 4
#define NLH_BCA_NO_REPLICA 8

/* nlh_boot_bca_levels: HOST code, no device -- ppnd16 and the level arithmetic of `bca` for one pair, the same source the device
 * compiles: *z0, *alpha_lo, *alpha_hi and *flag of (c2, cnt, a, level).  Returns 0, or NLH_INVALID_INPUT_ERROR for: cnt < 0,
 * cnt > NLH_BOOT_MAX_REP, c2 < 0, c2 > 2*cnt, a level that is not inside (0, 1), a NULL output.  A refused call writes nothing.
 * cnt == 0: NaN and NLH_BCA_NO_REPLICA. */
int nlh_boot_bca_levels(int32_t c2, int32_t cnt, double a, double level, double *z0, double *alpha_lo, double *alpha_hi, int32_t *flag);

/* `student`: DEVICE arrays on the handle's stream: dxs, dsigs [nrep][nprob][n], dx, dsigma [nprob][n], in; dlo, dhi [nprob][n]
 * and dnvalid_t [nprob][n] (int32: cnt_t), out.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (nrep < 1, nrep > NLH_BOOT_MAX_REP, nprob < 0, n < 1, a
 * level that is not inside (0, 1), a NULL array); NLH_ARRAY_SIZE_ERROR (nprob*n or nprob*nrep of 2^31 or more).  A refused call
 * writes nothing.  nprob == 0: 0. */
int nlh_boot_student_batch(nlh_handle *h, int32_t nrep, int32_t nprob, int32_t n, const double *dxs, const double *dsigs,
                           const double *dx, const double *dsigma, double level, double *dlo, double *dhi, int32_t *dnvalid_t);

/* `jackknife`: DEVICE arrays on the handle's stream: dw [nprob][m] (or NULL: no weights), in; dwout [nrows][nprob][m], out.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (nprob < 0, m < 1, m > NLH_BOOT_MAX_ROWS, row0 < 0,
 * nrows < 0, row0 + nrows > m, a NULL dwout); NLH_ARRAY_SIZE_ERROR (nprob*m of 2^31 or more).  A refused call writes nothing.
 * nprob == 0 or nrows == 0: 0. */
int nlh_boot_jackknife_batch(nlh_handle *h, int32_t nprob, int32_t m, int32_t row0, int32_t nrows, const double *dw, double *dwout);

/* `accel`: DEVICE arrays on the handle's stream: dxjack [m][nprob][n], dw [nprob][m] (or NULL: every row is active), in; daccel
 * [nprob][n] and dnjack [nprob] (int32), out.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (m < 1, m > NLH_BOOT_MAX_ROWS, nprob < 0, n < 1, a NULL
 * dxjack, daccel or dnjack); NLH_ARRAY_SIZE_ERROR (nprob*n or nprob*m of 2^31 or more).  A refused call writes nothing.
 * nprob == 0: 0. */
int nlh_boot_accel_batch(nlh_handle *h, int32_t m, int32_t nprob, int32_t n, const double *dxjack, const double *dw, double *daccel,
                         int32_t *dnjack);

/* `bca`: DEVICE arrays on the handle's stream: dxs [nrep][nprob][n], dx, daccel [nprob][n], in; dlo, dhi, dz0, dalpha_lo,
 * dalpha_hi [nprob][n], dflags [nprob][n] (int32) and dnvalid [nprob] (int32: summary's cnt), out.
 * Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (nrep < 1, nrep > NLH_BOOT_MAX_REP, nprob < 0, n < 1, a
 * level that is not inside (0, 1), a NULL array); NLH_ARRAY_SIZE_ERROR (nprob*n or nprob*nrep of 2^31 or more).  A refused call
 * writes nothing.  nprob == 0: 0. */
int nlh_boot_bca_batch(nlh_handle *h, int32_t nrep, int32_t nprob, int32_t n, const double *dxs, const double *dx, const double *daccel,
                       double level, double *dlo, double *dhi, double *dz0, double *dalpha_lo, double *dalpha_hi, int32_t *dflags,
                       int32_t *dnvalid);

#ifdef __cplusplus
}
#endif
#endif /* NONLIN_HIP_BOOT_CI_H */
