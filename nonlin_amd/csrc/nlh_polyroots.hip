// nlh_polyroots.hip -- polynomial%roots (src/nonlin_polynomials.f90:357-381) and polynomial%evaluate (:241-321), batched
// over independent polynomials of one order.  The kernels and the algorithm are in nlh_kernels_polyroots.h; here: which
// form a call runs (lane per polynomial, wave per polynomial on an LDS window, the same on a global-memory window), the
// launches, and the host-array front end.
#include "nlh_internal.h"
#include "nlh_kernels_polyroots.h"

void nlh_polyroots_init_device(int lds_max)
{
    (void)hipFuncSetAttribute((const void *)k_polyroots_lane, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_polyroots_wave<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
}

enum { PR_LANE = 1, PR_WAVE = 2, PR_GLOBAL = 3 };

// The form a call of this order runs.  NLH_POLYROOTS_FORM = lane | wave | global (read at every call; tests) moves an
// order to a later form than its own; a form that cannot hold the order hands it to the next one.
static int pr_form(int32_t order)
{
    int want = 0;
    if (const char *e = getenv("NLH_POLYROOTS_FORM")) {
        if (!strcmp(e, "lane")) want = PR_LANE;
        else if (!strcmp(e, "wave")) want = PR_WAVE;
        else if (!strcmp(e, "global")) want = PR_GLOBAL;
    }
    int form = order <= PR_LANE_MAX ? PR_LANE : (order <= PR_WAVE_LDS_MAX ? PR_WAVE : PR_GLOBAL);
    if (want > form) form = want;
    return form;
}

// Workgroups of one launch of the wave forms, and bytes of global window one launch may hold.
static const int32_t PR_WAVE_SLICE = 1 << 30;
static const size_t PR_GLOBAL_WINDOW_BYTES = (size_t)1 << 30;

int nlh_poly_roots_batch(nlh_handle *h, int32_t nprob, int32_t order, const double *dcoef, double *dz, int32_t *dinfo)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (order < 0 || nprob < 0) return NLH_INVALID_INPUT_ERROR;
    if (order > PR_MAX_ORDER) return NLH_ARRAY_SIZE_ERROR;
    if (nprob < 1 || order == 0) return 0;                         // :373
    if (!dcoef || !dz || !dinfo) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int form = pr_form(order);
    Timed timed(h, NLH_K_POLYROOTS);
    if (form == PR_LANE) {
        const size_t lds = sizeof(double) * 64 * ((size_t)order * order + order);
        if (!lds_fits((const void *)k_polyroots_lane, lds)) return NLH_ARRAY_SIZE_ERROR;
        const unsigned blocks = (unsigned)(((size_t)nprob + 63) / 64);
        hipLaunchKernelGGL(k_polyroots_lane, dim3(blocks), dim3(64), lds, s, nprob, order, dcoef, dz, dinfo);
    } else if (form == PR_WAVE) {
        const size_t lds = sizeof(double) * pr_wave_doubles(order);
        if (!lds_fits((const void *)k_polyroots_wave<false>, lds)) return NLH_ARRAY_SIZE_ERROR;
        for (int64_t p0 = 0; p0 < nprob; p0 += PR_WAVE_SLICE) {
            const int32_t cnt = (int32_t)std::min<int64_t>(PR_WAVE_SLICE, nprob - p0);
            hipLaunchKernelGGL(k_polyroots_wave<false>, dim3((unsigned)cnt), dim3(64), lds, s, (int32_t)p0, order, dcoef, dz,
                               dinfo, (double *)nullptr, (size_t)0);
        }
    } else {
        const size_t stride = pr_wave_doubles(order);
        const int64_t fit = (int64_t)std::max<size_t>(1, PR_GLOBAL_WINDOW_BYTES / (sizeof(double) * stride));
        const int32_t slice = (int32_t)std::min<int64_t>(fit, nprob);
        int rc;
        if ((rc = ensure(h, h->W2, sizeof(double) * stride * (size_t)slice))) return rc;
        for (int64_t p0 = 0; p0 < nprob; p0 += slice) {            // one stream: a slice's windows are free when the next starts
            const int32_t cnt = (int32_t)std::min<int64_t>(slice, nprob - p0);
            hipLaunchKernelGGL(k_polyroots_wave<true>, dim3((unsigned)cnt), dim3(64), 0, s, (int32_t)p0, order, dcoef, dz, dinfo,
                               (double *)h->W2.p, stride);
        }
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Host-array front end for one polynomial (what polynomial%roots marshals to): coef [order + 1], z [order][2].
int nlh_poly_roots(nlh_handle *h, int32_t order, const double *coef, double *z, int32_t *info)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (order < 0) return NLH_INVALID_INPUT_ERROR;
    if (order > PR_MAX_ORDER) return NLH_ARRAY_SIZE_ERROR;
    if (info) *info = 0;
    if (order == 0) return 0;                                      // :373
    if (!coef || !z || !info) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h, h->xdev, sizeof(double) * ((size_t)3 * order + 2)))) return rc;
    double *dc = (double *)h->xdev.p, *dz = dc + order + 1;
    int32_t *di = (int32_t *)(dz + 2 * (size_t)order);
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(dc, coef, sizeof(double) * (order + 1), hipMemcpyHostToDevice, s));
    if ((rc = nlh_poly_roots_batch(h, 1, order, dc, dz, di))) return rc;
    HIPCHK(h, hipMemcpyAsync(z, dz, sizeof(double) * 2 * (size_t)order, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(info, di, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}

// points of one launch of the evaluation kernels
static const size_t PR_EVAL_SLICE = (size_t)1 << 30;

static int pr_eval(nlh_handle *h, bool cplx, int32_t nprob, int32_t order, int32_t npts, const double *dcoef, const double *dx,
                   double *dy)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (order < 0 || nprob < 0 || npts < 0) return NLH_INVALID_INPUT_ERROR;
    if (nprob < 1 || npts < 1) return 0;
    if (!dcoef || !dx || !dy) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    // a slice is a whole number of polynomials, so that a point's polynomial is its index / npts within the slice
    const size_t per = std::max<size_t>(1, PR_EVAL_SLICE / (size_t)npts);
    const size_t w = cplx ? 2 : 1;
    for (size_t p0 = 0; p0 < (size_t)nprob; p0 += per) {
        const size_t cnt = std::min(per, (size_t)nprob - p0), total = cnt * (size_t)npts, off = p0 * (size_t)npts;
        const unsigned blocks = (unsigned)((total + 255) / 256);
        if (cplx)
            hipLaunchKernelGGL(k_poly_eval_complex, dim3(blocks), dim3(256), 0, h->stream, total, npts, order,
                               dcoef + p0 * (size_t)(order + 1), dx + w * off, dy + w * off);
        else
            hipLaunchKernelGGL(k_poly_eval, dim3(blocks), dim3(256), 0, h->stream, total, npts, order,
                               dcoef + p0 * (size_t)(order + 1), dx + off, dy + off);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_poly_eval_batch(nlh_handle *h, int32_t nprob, int32_t order, int32_t npts, const double *dcoef, const double *dx,
                        double *dy)
{
    return pr_eval(h, false, nprob, order, npts, dcoef, dx, dy);
}

int nlh_poly_eval_complex_batch(nlh_handle *h, int32_t nprob, int32_t order, int32_t npts, const double *dcoef,
                                const double *dz, double *dy)
{
    return pr_eval(h, true, nprob, order, npts, dcoef, dz, dy);
}
