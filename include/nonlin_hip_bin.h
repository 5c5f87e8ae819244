/* nonlin_hip_bin.h -- a part of the C ABI of libnonlin_hip.so: bin-integrated fits, the quadrature of any device model over
 * the bins of a histogram or the pixels of an image.  include/nonlin_hip.h includes this file, and this file includes that
 * one, so either gives the whole ABI. */
#ifndef NONLIN_HIP_BIN_H
#define NONLIN_HIP_BIN_H

#include "nonlin_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- bin-integrated fits (no counterpart in nonlin v2.2.0): ANY device model integrated (or averaged) over the bins its data
 * were recorded in.  The count in a bin of a histogram is the integral of the density over the bin, and a pixel records the
 * mean of the image over its area; the model value at the bin centre times the width is biased as soon as a bin is not narrow
 * against the feature (README, the study table: Sheppard's correction).  Like a convolution, this is a pair of wrapping
 * launchers around any inner launcher pair, so everything that takes launchers works through it; a convolution, a loss, the
 * Poisson pair, a map or a group wrap the binned pair, not the other way round.
 * A problem has m bins and a rule of Q nodes, 1 <= Q <= NLH_BIN_MAX_Q.  The inner pair is bound on Q m rows, NODE-MAJOR: inner
 * row q m + i is node q of bin i (so that the node plane q of consecutive bins is consecutive doubles).  It must return MODEL
 * VALUES: bind it with y = 0 and without weights (v - 0.0 keeps every bit of v).  The wrapper is given dy [nprob][m], optional
 * weights dw [nprob][m] (NULL: none), the rule's weights c [Q] by value and an optional per-bin scale s on the DEVICE, [m]
 * for every problem (shared_s != 0) or [nprob][m], or NULL: none; point q belongs to problem p = dprob ? dprob[q] : q and reads
 * row p of dy, dw and s.
 * THE ARITHMETIC IS PART OF THE INTERFACE -- one IEEE operation per step, no fused operation.  Per output, one bin i of one
 * column v [0 .. Q m - 1] (the model values, or one column of the inner Jacobian):
 *   acc = +0.0
 *   for q = 0 .. Q-1 ascending:   t = c[q] * v[q m + i];  acc = acc + t
 *   g = s ? s[i] * acc : acc
 *   residual    F[i] = g - y[i];  with weights F[i] = w[i] * F[i]
 *   Jacobian    J[k][i] = g over column k of the inner Jacobian; with weights w[i] * g
 *   weights     a bin with w[i] == 0.0 is STORED as +0.0 in dF and in every column of dJ, not multiplied
 *   apply       g
 * No sum crosses threads: every output is one sequential chain, so its bits depend on neither the batch, the workgroup form,
 * the column split, the slice nor dprob, and a numpy restatement reproduces them bit for bit.
 * With the Gauss-Legendre rule (xi_q, c_q) of nlh_bin_rule on [-1, 1] and a bin lo .. hi -- mid = 0.5 (lo + hi), half =
 * 0.5 (hi - lo), the nodes at mid + half xi_q --, s = half gives the integral over the bin, and c halved with s = NULL the
 * mean over it (the halving is exact).  A rule of two variables is the tensor product, Q = Qx Qy nodes, s = half_x half_y.
 * Not here: model objects and a Fortran binding, the bootstrap of a binned fit, nlh_curve_guess_batch on binned data
 * (guess on the bin centres and divide the amplitudes by the width), and adaptive rules. ---- */
#define NLH_BIN_MAX_Q 16
typedef struct nlh_bin {
    int32_t Q;             /* nodes per bin, 1 .. NLH_BIN_MAX_Q */
    double c[NLH_BIN_MAX_Q]; /* the rule's weights; c[Q ..] are not read */
    const double *s;       /* device pointer: the per-bin scale, or NULL: none */
    int32_t shared_s;      /* s is [m], one for every problem; otherwise [nprob][m] */
} nlh_bin;
typedef struct nlh_bin_ctx nlh_bin_ctx;

/* Gauss-Legendre nodes xi [Q] (ascending) and weights c [Q] on [-1, 1] for Q = 1 .. 8, literal constants of the library (a
 * rule of Q nodes integrates polynomials up to degree 2 Q - 1 exactly).  A node is the double nearest the exact value.  The
 * weights are the doubles of numpy.polynomial.legendre.leggauss, the reference they are held to within 2^-52: symmetric,
 * their sequential sum within an ulp of 2, each within 1e-15 of the exact weight (for Q >= 5 that is several ulp of the
 * smallest weights -- the reference's own error, far below what a rule of so few nodes leaves of an integral).  HOST code, no
 * device.  Returns 0, or NLH_INVALID_INPUT_ERROR for Q outside 1 .. 8 or a NULL array; a refused call writes nothing. */
int  nlh_bin_rule(int32_t Q, double *xi, double *c);

/* The wrapping launchers.  nlh_bin_wrap makes their context on the handle's device; *bn is copied, while its s, the inner
 * pair (fcn, jac -- NULL: none --, inner_ctx), dy and dw stay the caller's and must outlive the context.
 *   nlh_bin_device_fcn  called with m bins: the inner fcn with Q m rows into scratch V [npoints][Q m]; then the table's
 *                       residual into the caller's dF [npoints][m].
 *   nlh_bin_device_jac  the inner jac with Q m rows into scratch Jf [npoints][n][Q m]; then the table's Jacobian into
 *                       dJ [npoints][n][m]; every entry is written.  With a NULL inner jac it returns
 *                       NLH_UNDEFINED_FUNCTION_ERROR: pass a NULL jacfcn to the solver instead (forward differences of the
 *                       wrapped residual).
 * Both enqueue only on the stream handed in, never synchronise and may be called from several host threads on different
 * streams.  A malformed context, n < 1, m < 1 or a Q outside 1 .. NLH_BIN_MAX_Q returns NLH_INVALID_INPUT_ERROR before any
 * launch; no points: 0; then Q m > 2^31 - 1: NLH_ARRAY_SIZE_ERROR.  An inner error comes back as it is, with no further
 * launch.  When dprob is NULL the launchers build a problem list of their own.  Scratch belongs to the context, exactly as a
 * convolution's: one buffer per stream, grown on demand, kept until nlh_bin_unwrap, at most 1 GiB per call; a call that needs
 * more runs in slices of points -- the same bits.  NLH_BIN_SCRATCH = bytes lowers the cap, NLH_BIN_FORM = row | flat forces a
 * workgroup form for the sizes it can hold (flat: m <= 256), NLH_BIN_SPLIT = number of column groups overrides the column
 * split (environment, read at each call; tests).
 * Errors of nlh_bin_wrap: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR (a NULL out, dy or bn, Q outside 1 .. NLH_BIN_MAX_Q);
 * NLH_UNDEFINED_FUNCTION_ERROR (a NULL fcn). */
int  nlh_bin_wrap(nlh_handle *h, const nlh_bin *bn, const double *dy, const double *dw, nlh_device_vecfcn fcn,
                  nlh_device_jacfcn jac, void *inner_ctx, nlh_bin_ctx **out);
void nlh_bin_unwrap(nlh_bin_ctx *c);
int  nlh_bin_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF);
int  nlh_bin_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ);
/* The bare reduction g of arbitrary columns dv [nprob][ncol][Q m] on the DEVICE (the handle's stream) into dout
 * [nprob][ncol][m], dout != dv; problem p uses the scale of p.  The binned model for plotting is nlh_curve_eval_batch (or the
 * formula's) at the nodes followed by this with ncol = 1.  Errors, in this order: NLH_ERR_BAD_HANDLE; NLH_INVALID_INPUT_ERROR
 * (nprob < 0, m < 1, ncol < 1, a NULL bn, a bad Q); NLH_ARRAY_SIZE_ERROR (Q m > 2^31 - 1, or more workgroups than a launch
 * holds); nprob == 0: 0; NLH_INVALID_INPUT_ERROR (a NULL dv or dout, dout == dv). */
int  nlh_bin_apply_batch(nlh_handle *h, const nlh_bin *bn, int32_t nprob, int32_t m, int32_t ncol, const double *dv, double *dout);

#ifdef __cplusplus
}
#endif
#endif /* NONLIN_HIP_BIN_H */
