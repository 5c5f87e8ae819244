// nlh_profile.hip -- profile-likelihood intervals (include/nonlin_hip_profile.h: nlh_profile_*; kernels: nlh_kernels_profile.h):
// the start of every end from the fit -- the unpinned launcher at x, its cost by nlh_starts_cost_batch's order -- and the
// lock-step step of the root finder.  The refits between two steps are the caller's: the pin pair (nlh_pin.hip) under any solver.
#include "nlh_internal.h"
#include "nlh_kernels_place.h"
#include "nlh_kernels_profile.h"

static bool profile_state_ok(const nlh_profile_state *st)
{
    return st && st->C0 && st->delta && st->xhat && st->width && st->bound && st->theta && st->a && st->ga && st->b && st->gb && st->end &&
           st->phase && st->flag && st->last && st->nexp && st->nev && st->nfail;
}

static bool profile_ends_ok(int32_t nprob, int32_t n) { return nprob >= 0 && n >= 1 && (int64_t)nprob * n * 2 <= 0x7fffffff; }

int nlh_profile_start_batch_device(nlh_handle *h, nlh_device_vecfcn fcn, void *ctx, int32_t nprob, int32_t m, int32_t n,
                                   const double *dx, const double *dsigma, const int32_t *ddof, double crit, int32_t scaled,
                                   const double *xl, const double *xu, const nlh_profile_state *st)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (m < 1 || !profile_ends_ok(nprob, n) || !dx || !dsigma || !profile_state_ok(st)) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t fb = sizeof(double) * (size_t)nprob * m, bb = sizeof(double) * (size_t)n;
    int rc;
    if ((rc = ensure(h, h->profW, fb + 2 * bb + sizeof(int32_t) * (size_t)nprob))) return rc;
    double *F = (double *)h->profW.p, *dxl = xl ? F + (size_t)nprob * m : nullptr, *dxu = xu ? F + (size_t)nprob * m + n : nullptr;
    if (xl) HIPCHK(h, hipMemcpyAsync(dxl, xl, bb, hipMemcpyHostToDevice, s));
    if (xu) HIPCHK(h, hipMemcpyAsync(dxu, xu, bb, hipMemcpyHostToDevice, s));
    if (xl || xu) HIPCHK(h, hipStreamSynchronize(s));                // (the host arrays are the caller's to reuse on return)
    // one call, point q of problem q (a model's launchers want the list): nprob * n is inside a launcher's 31-bit point counts
    int32_t *list = (int32_t *)(F + (size_t)nprob * m + 2 * (size_t)n);
    hipLaunchKernelGGL(k_wrap_iota, dim3((unsigned)((nprob + 255) / 256)), dim3(256), 0, s, nprob, 0, list);
    if ((rc = fcn(ctx, s, nprob, list, n, dx, m, F))) {
        h->err = "profile: the user's launcher returned " + std::to_string(rc);
        return rc;
    }
    if ((rc = nlh_starts_cost_batch(h, nprob, m, F, st->C0))) return rc;
    const size_t nend = (size_t)nprob * n * 2;
    hipLaunchKernelGGL(k_profile_start, dim3((unsigned)((nend + 255) / 256)), dim3(256), 0, s, nprob, m, n, dx, dsigma, ddof, crit, sqrt(crit),
                       scaled != 0, dxl, dxu, *st);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_profile_step_batch(nlh_handle *h, int32_t nprob, int32_t n, int32_t nact, const int32_t *dact, const double *dcost,
                           const int32_t *dfail, const nlh_profile_state *st, double tol, double xtol, int32_t max_expand,
                           int32_t maxit, int32_t *nleft)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!profile_ends_ok(nprob, n) || nact < 0 || (nact > 0 && (!dact || !dcost)) || !profile_state_ok(st) || !nleft ||
        !(tol >= 0.0) || !std::isfinite(tol) || !(xtol >= 0.0) || !std::isfinite(xtol) || max_expand < 0 || maxit < 1)
        return NLH_INVALID_INPUT_ERROR;
    *nleft = 0;
    const int nend = nprob * n * 2;
    if (nend == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc;
    if ((rc = ensure(h, h->profW, sizeof(int32_t)))) return rc;
    // the count lives at the end of the buffer: the start's residuals and box, at its head, are dead by now
    int32_t *left = (int32_t *)((char *)h->profW.p + h->profW.bytes - sizeof(int32_t) * 2);
    HIPCHK(h, hipMemsetAsync(left, 0, sizeof(int32_t), s));
    if (nact > 0)
        hipLaunchKernelGGL(k_profile_step, dim3((unsigned)((nact + 255) / 256)), dim3(256), 0, s, nend, n, nact, dact, dcost, dfail, *st, tol, xtol,
                           max_expand, maxit);
    hipLaunchKernelGGL(k_profile_left, dim3((unsigned)((nend + 255) / 256)), dim3(256), 0, s, nend, st->phase, left);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(nleft, left, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}
