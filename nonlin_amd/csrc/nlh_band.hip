// nlh_band.hip -- confidence and prediction bands (include/nonlin_hip.h: nlh_propagate*): the parameter covariance of a fit
// propagated through any vector function of the parameters, sd_i = sqrt(G_i C G_i^T) -- the delta method (kernel and
// arithmetic: nlh_kernels_band.h; the workgroup forms and the scratch cap: nlh_launch.h).  Here: which form a call runs, the
// launch, and the chain around it -- the values F(x), the Jacobian by vfh_jac_fcn's rule, the kernel -- for device
// launchers and behind host arrays.  The Jacobian lives in the handle's bdW, which nothing else uses: a band between two
// solves leaves their buffers alone.  The bands of the built-in models are nlh_curve_band_batch (nlh_curve.hip) and
// nlh_expr_band_batch (nlh_expr.hip), a model object's is nlh_dq_model_propagate (nlh_model.hip): all of them this chain.
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_band.h"

void nlh_band_init_device(int lds_max)
{
    (void)hipFuncSetAttribute((const void *)k_band<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_band<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
}

static inline size_t band_tri_bytes(int32_t n) { return sizeof(double) * ((size_t)n * ((size_t)n + 1) / 2); }

// The form a launch runs.  Row: a workgroup per (point, 256 rows), the point's packed triangle in LDS while it fits the cap
// (n <= 200), read from global memory beyond.  Flat: several points per workgroup, each one's triangle in LDS -- as many
// points as 256 threads and the cap hold; by default while that is two or more.  NLH_BAND_FORM = row | flat (environment,
// read at every call; tests) forces a form for the sizes it can hold (flat: m <= 256, n <= 200).
struct BandForm { bool flat, clds; int ppw, nblk; size_t lds; };
static BandForm band_form(int m, int n)
{
    BandForm f;
    const size_t tb = band_tri_bytes(n);
    f.clds = lds_fits((const void *)k_band<false, true>, tb);
    const int fit = f.clds ? (int)std::min<size_t>(256, (size_t)NLH_LDS_MAX / tb) : 0;
    const int ppw = m <= 256 ? std::min(256 / m, fit) : 0;       // points of a flat workgroup; 0: flat cannot hold the size
    f.flat = ppw >= 1 && launch_flat("NLH_BAND_FORM", m);
    if (f.flat && ppw < 2) {                                     // a single point per workgroup: only when asked for
        const char *e = getenv("NLH_BAND_FORM");
        f.flat = e && !strcmp(e, "flat");
    }
    f.ppw = f.flat ? ppw : 1;
    f.nblk = f.flat ? 1 : (m + 255) / 256;
    f.lds = f.flat ? tb * (size_t)ppw : (f.clds ? tb : 0);
    return f;
}

int nlh_propagate(nlh_handle *h, int32_t npoints, int32_t m, int32_t n, const double *dJ, const double *dcov, const double *dnoise,
                  double *dsd)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (npoints < 0 || m < 1 || n < 1) return NLH_INVALID_INPUT_ERROR;
    if (npoints == 0) return 0;
    if (!dJ || !dcov || !dsd) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    const BandForm f = band_form(m, n);
    const size_t wgs = f.flat ? ((size_t)npoints + f.ppw - 1) / f.ppw : (size_t)npoints * f.nblk;
    if (wgs > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    const dim3 grid((unsigned)wgs);
    hipStream_t s = h->stream;
    if (f.flat) hipLaunchKernelGGL((k_band<true, true>), grid, dim3(256), f.lds, s, m, n, f.nblk, f.ppw, npoints, dJ, dcov, dnoise, dsd);
    else if (f.clds) hipLaunchKernelGGL((k_band<false, true>), grid, dim3(256), f.lds, s, m, n, f.nblk, f.ppw, npoints, dJ, dcov, dnoise, dsd);
    else hipLaunchKernelGGL((k_band<false, false>), grid, dim3(256), 0, s, m, n, f.nblk, f.ppw, npoints, dJ, dcov, dnoise, dsd);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the chain
// ---------------------------------------------------------------------------------------------------------------------
int nlh_propagate_batch_device(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn,
                               void *ctx, const double *dx, const double *dcov, const double *dnoise, double *dval, double *dsd)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (nprob < 0 || m < 1 || n < 1) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    if (!dx || !dcov || !dsd) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    const ResidualSource rs = ResidualSource::launchers(fcn, jacfcn, ctx);
    // scratch of a problem: its Jacobian, and F(x) for the forward differences when the caller keeps no values
    const bool ownf = !jacfcn && !dval;
    const size_t mn = (size_t)m * n, per = sizeof(double) * (mn + (ownf ? (size_t)m : 0));
    const int32_t slice = (int32_t)std::min<size_t>((size_t)slice_panel(m, n), std::max<size_t>(1, scratch_cap("NLH_BAND_SCRATCH") / per));
    return lockstep_slices(nprob, slice, [&](int32_t p0, int32_t cnt) {
        int rc;
        if ((rc = ensure(h, h->bdW, per * (size_t)cnt))) return rc;
        double *J = (double *)h->bdW.p, *f = dval ? dval + (size_t)p0 * m : (ownf ? J + mn * (size_t)cnt : nullptr);
        const ResidualSource r = rs.shifted(p0, m, n);
        const double *xs = dx + (size_t)p0 * n;
        if (f && (rc = residual_eval(h, r, cnt, m, n, xs, f, nullptr, nullptr, -1))) return rc;
        if ((rc = residual_jacobian(h, r, cnt, m, n, xs, f, J, nullptr, nullptr, -1, false, false, true))) return rc;
        return nlh_propagate(h, cnt, m, n, J, dcov + (size_t)p0 * n * n, dnoise ? dnoise + p0 : nullptr, dsd + (size_t)p0 * m);
    });
}

int nlh_propagate_batch_device_h(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn, nlh_device_jacfcn jacfcn,
                                 void *ctx, const double *x, const double *cov, const double *noise, double *val, double *sd)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (nprob < 0 || m < 1 || n < 1) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    if (!x || !cov || !sd) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t c = (size_t)nprob, nn = (size_t)n * n;
    int rc;
    if ((rc = ensure(h, h->bdH, sizeof(double) * c * ((size_t)n + nn + 1 + 2 * (size_t)m)))) return rc;
    double *dx = (double *)h->bdH.p, *dcov = dx + c * n, *dnoise = dcov + c * nn, *dval = dnoise + c, *dsd = dval + c * m;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(dx, x, sizeof(double) * c * n, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(dcov, cov, sizeof(double) * c * nn, hipMemcpyHostToDevice, s));
    if (noise) HIPCHK(h, hipMemcpyAsync(dnoise, noise, sizeof(double) * c, hipMemcpyHostToDevice, s));
    if ((rc = nlh_propagate_batch_device(h, nprob, m, n, fcn, jacfcn, ctx, dx, dcov, noise ? dnoise : nullptr, val ? dval : nullptr, dsd)))
        return rc;
    if (val) HIPCHK(h, hipMemcpyAsync(val, dval, sizeof(double) * c * m, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(sd, dsd, sizeof(double) * c * m, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}
