// nlh_loss.hip -- robust losses (include/nonlin_hip.h: nlh_loss_*): Huber, soft-L1 and Cauchy fits for any device model, as a
// pair of wrapping launchers around any inner launcher pair (kernels and arithmetic: nlh_kernels_loss.h; scratch, grid and
// slice loop: nlh_launch.h).  Here: the wrapping context, the launchers, nlh_loss_apply_batch, and the checked upload of host
// scales.  The one-call fits with a loss are the pipeline of nlh_fit.hip; the model object is nlh_loss_model_create
// (nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_loss.h"

static const uint32_t LOSS_MAGIC = 0x73736f6cu;

struct nlh_loss_ctx : WrapCtx {
    int kind = NLH_LOSS_LINEAR;
    const double *dscale = nullptr;
    int shared_scale = 0;
};

void loss_ctx_rebind(nlh_loss_ctx *c, const double *dscale) { c->dscale = dscale; }

bool nlh_loss_kind_ok(int32_t kind) { return kind >= NLH_LOSS_LINEAR && kind <= NLH_LOSS_CAUCHY; }

// host scales: finite and positive, every one (LINEAR reads none)
bool nlh_loss_scale_ok(int32_t kind, const double *scale, size_t cnt)
{
    if (kind == NLH_LOSS_LINEAR) return true;
    if (!scale) return false;
    for (size_t p = 0; p < cnt; ++p)
        if (!(scale[p] > 0.0) || !std::isfinite(scale[p])) return false;
    return true;
}

int nlh_loss_wrap(nlh_handle *h, int32_t kind, const double *dscale, int32_t shared_scale, nlh_device_vecfcn fcn, nlh_device_jacfcn jac,
                  void *inner_ctx, nlh_loss_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !nlh_loss_kind_ok(kind)) return NLH_INVALID_INPUT_ERROR;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (kind != NLH_LOSS_LINEAR && !dscale) return NLH_INVALID_INPUT_ERROR;
    nlh_loss_ctx *c = nullptr;
    if (const int rc = wrap_new(h, LOSS_MAGIC, fcn, jac, inner_ctx, &c)) return rc;
    c->kind = kind; c->dscale = dscale; c->shared_scale = shared_scale != 0;
    *out = c;
    return 0;
}

void nlh_loss_unwrap(nlh_loss_ctx *c)
{
    if (c && c->magic == LOSS_MAGIC) wrap_release(c);
}

static void loss_launch_jac(const nlh_loss_ctx *c, const LossArgs &A, int m, int n, int npoints, const double *R, double *J, hipStream_t s)
{
    const JacGrid g = jac_grid("NLH_LOSS_FORM", "NLH_LOSS_SPLIT", c->cus, m, n, npoints);
    if (g.flat) hipLaunchKernelGGL(k_loss_jac<true>, g.grid, dim3(256), 0, s, A, m, n, g.nblk, g.ppw, g.cpg, npoints, R, J);
    else hipLaunchKernelGGL(k_loss_jac<false>, g.grid, dim3(256), 0, s, A, m, n, g.nblk, g.ppw, g.cpg, npoints, R, J);
}

// Both launchers.  What they check themselves is refused before any launch; an inner error comes back as it is, with no
// further launch.  Scratch: the inner residual R of a Jacobian call, and a problem list for the inner launcher when the caller
// passed none.
static int loss_call(bool jac, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                     double *out)
{
    nlh_loss_ctx *c = wrap_ctx<nlh_loss_ctx>(ctx, LOSS_MAGIC);
    int end;
    if (wrap_refused(c, n >= 1 && m >= 1 && dX && out, jac, npoints, &end)) return end;
    const bool lin = c->kind == NLH_LOSS_LINEAR;                  // no kernel of the table, no R: the inner pair's output as it is
    hipStream_t s = (hipStream_t)hip_stream;
    const bool needR = jac && !lin;
    LossArgs A;
    A.kind = c->kind; A.shared_scale = c->shared_scale; A.scale = c->dscale;
    return wrap_slices(c->scratch, "NLH_LOSS_SCRATCH", c->device, s, needR ? (size_t)m : 0, npoints, m, dprob,
                       [&](double *R, int, int q0, int cnt, const int32_t *lp) {
        A.dprob = lp;
        const double *Xs = dX + (size_t)q0 * n;
        int rc;
        if (!jac) {
            double *F = out + (size_t)q0 * m;
            if ((rc = c->fcn(c->inner, hip_stream, cnt, lp, n, Xs, m, F))) return rc;
            if (!lin) hipLaunchKernelGGL(k_loss_fcn, dim3((unsigned)(((size_t)cnt * m + 255) / 256)), dim3(256), 0, s, A, m, cnt, F);
        } else {
            double *J = out + (size_t)q0 * m * n;
            if (!lin && (rc = c->fcn(c->inner, hip_stream, cnt, lp, n, Xs, m, R))) return rc;
            if ((rc = c->jac(c->inner, hip_stream, cnt, lp, n, Xs, m, J))) return rc;
            if (!lin) loss_launch_jac(c, A, m, n, cnt, R, J, s);
        }
        return 0;
    });
}

int nlh_loss_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return loss_call(false, ctx, hip_stream, npoints, dprob, n, dX, m, dF);
}

int nlh_loss_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ)
{
    return loss_call(true, ctx, hip_stream, npoints, dprob, n, dX, m, dJ);
}

int nlh_loss_apply_batch(nlh_handle *h, int32_t kind, int32_t nprob, int32_t m, const double *dscale, int32_t shared_scale, const double *dr,
                         double *dout, double *dg, double *dwgt)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!nlh_loss_kind_ok(kind) || nprob < 0 || m < 1) return NLH_INVALID_INPUT_ERROR;
    if (((size_t)nprob * m + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0 || (!dout && !dg && !dwgt)) return 0;
    if (!dr || (kind != NLH_LOSS_LINEAR && !dscale)) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    LossArgs A;
    A.kind = kind; A.shared_scale = shared_scale != 0; A.scale = dscale; A.dprob = nullptr;
    hipLaunchKernelGGL(k_loss_apply, dim3((unsigned)(((size_t)nprob * m + 255) / 256)), dim3(256), 0, h->stream, A, m, nprob, dr, dout, dg, dwgt);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// Host scales are checked here (finite, positive) and get a device copy, the caller's to hipFree (nlh_internal.h: the
// host-array fits and the model object)
int nlh_loss_scale_upload(nlh_handle *h, int32_t loss, const double *scale, size_t cnt, double **dscale)
{
    *dscale = nullptr;
    if (!nlh_loss_scale_ok(loss, scale, cnt)) return NLH_INVALID_INPUT_ERROR;
    if (loss == NLH_LOSS_LINEAR) return 0;                        // reads no scale
    return nlh_upload(h, "the scales of a loss", {{scale, sizeof(double) * cnt}}, (void **)dscale);
}
