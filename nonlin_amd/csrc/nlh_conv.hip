// nlh_conv.hip -- instrument-response fits (include/nonlin_hip.h: nlh_conv_*): any device model convolved with a kernel along
// its rows, as a pair of wrapping launchers around any UNWEIGHTED inner launcher pair (kernels and arithmetic:
// nlh_kernels_conv.h; scratch and slice loop: nlh_launch.h).  Here: the check of a transform, the wrapping context, the
// launch shapes of the two workgroup forms, the launchers and nlh_conv_apply_batch.
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_conv.h"

static const uint32_t CONV_MAGIC = 0x766e6f63u;

struct nlh_conv_ctx : WrapCtx {
    nlh_conv cv{};
    const double *dy = nullptr, *dw = nullptr;
};

void conv_ctx_rebind(nlh_conv_ctx *c, const double *dy, const double *dw, const double *dk) { c->dy = dy; c->dw = dw; c->cv.k = dk; }

bool nlh_conv_ok(const nlh_conv *cv)
{
    return cv && cv->k && cv->L >= 1 && cv->L <= NLH_CONV_MAX_L && cv->origin >= 0 && cv->origin < cv->L &&
           (cv->ext == NLH_CONV_ZERO || cv->ext == NLH_CONV_HOLD);
}

bool nlh_conv_data_ok(const nlh_conv *cv, const double *y, size_t nprob, size_t m)
{
    const size_t taps = (size_t)cv->L * (cv->shared_k ? 1 : nprob);
    for (size_t j = 0; j < taps; ++j)
        if (!std::isfinite(cv->k[j])) return false;
    for (size_t i = 0; i < nprob * m; ++i)
        if (!std::isfinite(y[i])) return false;
    return true;
}

int nlh_conv_wrap(nlh_handle *h, const nlh_conv *cv, const double *dy, const double *dw, nlh_device_vecfcn fcn, nlh_device_jacfcn jac,
                  void *inner_ctx, nlh_conv_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !dy || !nlh_conv_ok(cv)) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    nlh_conv_ctx *c = nullptr;
    if (const int rc = wrap_new(h, CONV_MAGIC, fcn, jac, inner_ctx, &c)) return rc;
    c->cv = *cv; c->dy = dy; c->dw = dw;
    *out = c;
    return 0;
}

void nlh_conv_unwrap(nlh_conv_ctx *c)
{
    if (c && c->magic == CONV_MAGIC) wrap_release(c);
}

// One launch: V [npoints][ncol][m] -> O, out of place.  Flat: 256 / m points per workgroup, a column at a time.  Row: tiles
// of T rows (whole quads, at most CONV_T), cpp columns per pass -- the 256 / (T / 4) that fill the workgroup, or as many as the
// LDS holds with their halos.  The columns are dealt over gridDim.y while the launch has fewer than four workgroups per
// compute unit (NLH_CONV_SPLIT: that many groups).
static int conv_launch(int cus, const ConvArgs &A, int mode, int m, int ncol, int npoints, const double *V, double *O, hipStream_t s)
{
    const bool flat = launch_flat("NLH_CONV_FORM", m);
    const int T = std::min(CONV_T, (m + 3) & ~3), ntile = (m + T - 1) / T;
    const int ppw = flat ? 256 / m : 1;
    const size_t wgs = flat ? (size_t)(npoints + ppw - 1) / ppw : (size_t)npoints * ntile;
    if (wgs > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    size_t groups = 1;
    const size_t want = (size_t)4 * cus;
    if (wgs < want) groups = (want + wgs - 1) / wgs;
    if (const char *e = getenv("NLH_CONV_SPLIT")) {
        const int v = atoi(e);
        if (v >= 1) groups = (size_t)v;
    }
    groups = std::min<size_t>(groups, std::min<size_t>((size_t)ncol, 65535));
    const int cpg = (ncol + (int)groups - 1) / (int)groups;
    const dim3 grid((unsigned)wgs, (unsigned)((ncol + cpg - 1) / cpg));
    if (flat) {
        hipLaunchKernelGGL(k_conv_flat, grid, dim3(256), 0, s, A, mode, m, ncol, ppw, cpg, npoints, V, O);
    } else {
        const int col = conv_col_lds(T, A.L);
        const int cpp = std::max(1, std::min(std::min(256 / (T / 4), CONV_COLS_LDS / col), cpg));
        const size_t lds = sizeof(double) * (size_t)(((A.L + 1) & ~1) + cpp * col);
        hipLaunchKernelGGL(k_conv_row, grid, dim3(256), lds, s, A, mode, m, ncol, T, ntile, cpp, cpg, npoints, V, O);
    }
    return 0;
}

// Both launchers.  What they check themselves is refused before any launch; an inner error comes back as it is, with no
// further launch.  Scratch: the inner residual R [m] or the inner Jacobian Jf [n][m] of a point, and a problem list -- for the
// inner launcher and for the rows of y, w and k -- when the caller passed none.
static int conv_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                     double *out)
{
    nlh_conv_ctx *c = wrap_ctx<nlh_conv_ctx>(ctx, CONV_MAGIC);
    int end;
    if (wrap_refused(c, c && c->dy && nlh_conv_ok(&c->cv) && n >= 1 && m >= 1 && dX && out, jac, npoints, &end)) return end;
    hipStream_t s = (hipStream_t)hip_stream;
    ConvArgs A;
    A.k = c->cv.k; A.L = c->cv.L; A.origin = c->cv.origin; A.ext = c->cv.ext; A.shared_k = c->cv.shared_k;
    A.y = jac ? nullptr : c->dy; A.w = c->dw;
    const size_t per = jac ? (size_t)m * n : (size_t)m;
    return wrap_slices(c->scratch, "NLH_CONV_SCRATCH", c->device, s, per, npoints, m, dprob,
                       [&](double *S, int, int q0, int cnt, const int32_t *lp) {
        A.dprob = lp;
        const double *Xs = dX + (size_t)q0 * n;
        int rc;
        if (!jac) {
            if ((rc = c->fcn(c->inner, hip_stream, cnt, lp, n, Xs, m, S))) return rc;
            return conv_launch(c->cus, A, CONV_FCN, m, 1, cnt, S, out + (size_t)q0 * m, s);
        }
        if ((rc = c->jac(c->inner, hip_stream, cnt, lp, n, Xs, m, S))) return rc;
        return conv_launch(c->cus, A, CONV_JAC, m, n, cnt, S, out + (size_t)q0 * m * n, s);
    });
}

int nlh_conv_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return conv_call(false, ctx, hip_stream, npoints, dprob, n, dX, m, dF);
}

int nlh_conv_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ)
{
    return conv_call(true, ctx, hip_stream, npoints, dprob, n, dX, m, dJ);
}

int nlh_conv_apply_batch(nlh_handle *h, const nlh_conv *cv, int32_t nprob, int32_t m, int32_t ncol, const double *dv, double *dout)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 0 || m < 1 || ncol < 1 || !nlh_conv_ok(cv)) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    if (!dv || !dout || dv == dout) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    ConvArgs A;
    A.k = cv->k; A.L = cv->L; A.origin = cv->origin; A.ext = cv->ext; A.shared_k = cv->shared_k;
    A.y = nullptr; A.w = nullptr; A.dprob = nullptr;
    if (const int rc = conv_launch(device_cus(h->device), A, CONV_JAC, m, ncol, nprob, dv, dout, h->stream)) return rc;
    HIPCHK(h, hipGetLastError());
    return 0;
}
