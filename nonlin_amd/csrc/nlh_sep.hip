// nlh_sep.hip -- separable fits (include/nonlin_hip.h: nlh_sep_*): variable projection for any device model, as a pair of
// wrapping launchers around any inner launcher pair (kernels and arithmetic: nlh_kernels_sep.h; scratch and slice loop:
// nlh_launch.h).  Here: the object that names the linear parameters (host code; needs no GPU), the wrapping context, the
// launchers, and the two steps around a solve made by hand, gather and solve.
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_sep.h"

// ---------------------------------------------------------------------------------------------------------------------
// the object
// ---------------------------------------------------------------------------------------------------------------------
struct nlh_sep {
    int32_t nfull = 0, nlin = 0;
    std::vector<int32_t> lin, nl;      // ascending full indices: the linear parameters, the nonlinear ones
};

int nlh_sep_create(int32_t nfull, int32_t nlin, const int32_t *lin, nlh_sep **sp)
{
    if (!sp) return NLH_INVALID_INPUT_ERROR;
    *sp = nullptr;
    if (nlin < 1 || nlin > NLH_SEP_MAX_L || nfull - nlin < 1 || nfull > NLH_PMAP_MAX_N || !lin) return NLH_INVALID_INPUT_ERROR;
    for (int l = 0; l < nlin; ++l)
        if (lin[l] < 0 || lin[l] >= nfull || (l && lin[l] <= lin[l - 1])) return NLH_INVALID_INPUT_ERROR;
    nlh_sep *s = new nlh_sep();
    s->nfull = nfull; s->nlin = nlin;
    s->lin.assign(lin, lin + nlin);
    for (int k = 0, l = 0; k < nfull; ++k)
        if (l < nlin && lin[l] == k) ++l;
        else s->nl.push_back(k);
    *sp = s;
    return 0;
}

void nlh_sep_destroy(nlh_sep *sp) { delete sp; }

void nlh_sep_shape(const nlh_sep *sp, int32_t *nfull, int32_t *nlin, int32_t *nnonlin)
{
    if (nfull) *nfull = sp ? sp->nfull : 0;
    if (nlin) *nlin = sp ? sp->nlin : 0;
    if (nnonlin) *nnonlin = sp ? sp->nfull - sp->nlin : 0;
}

int nlh_sep_tables(const nlh_sep *sp, int32_t *lin, int32_t *nonlin)
{
    if (!sp) return NLH_INVALID_INPUT_ERROR;
    if (lin) memcpy(lin, sp->lin.data(), sizeof(int32_t) * sp->lin.size());
    if (nonlin) memcpy(nonlin, sp->nl.data(), sizeof(int32_t) * sp->nl.size());
    return 0;
}

static SepTables sep_tables(const nlh_sep *sp)
{
    SepTables T{};
    T.N = sp->nfull; T.L = sp->nlin; T.n = sp->nfull - sp->nlin;
    for (int l = 0; l < T.L; ++l) T.lin[l] = sp->lin[l];
    return T;
}

// ---------------------------------------------------------------------------------------------------------------------
// the wrapping context
// ---------------------------------------------------------------------------------------------------------------------
static const uint32_t SEP_MAGIC = 0x70655373u;

struct nlh_sep_ctx : WrapCtx {         // (cus: never read)
    SepTables T{};
};

void nlh_sep_init_device(int lds_max)
{
    (void)hipFuncSetAttribute((const void *)k_sep_solve<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_sep_project<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
}

int nlh_sep_wrap(nlh_handle *h, const nlh_sep *sp, nlh_device_vecfcn fcn, nlh_device_jacfcn jac, void *inner_ctx, nlh_sep_ctx **out)
{
    if (out) *out = nullptr;
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!out || !sp) return NLH_INVALID_INPUT_ERROR;
    if (!fcn || !jac) return NLH_UNDEFINED_FUNCTION_ERROR;       // the linear columns of the inner Jacobian are the basis
    nlh_sep_ctx *c = nullptr;
    if (const int rc = wrap_new(h, SEP_MAGIC, fcn, jac, inner_ctx, &c)) return rc;
    c->T = sep_tables(sp);
    *out = c;
    return 0;
}

void nlh_sep_unwrap(nlh_sep_ctx *c)
{
    if (c && c->magic == SEP_MAGIC) wrap_release(c);
}

// The form of a call: lds while m (L + 1 + n) doubles -- the panel [Phi | f0] and the columns of D -- fit a workgroup's LDS
// beside the kernels' own; NLH_SEP_FORM = global forces the other (lds cannot be forced where it does not fit).  Measured at
// 4,096 x (m = 2048, L = 6, n = 6): with the panel alone in LDS (114 KB, one workgroup per compute unit) the pair of kernels
// took 1.07 times what the global form takes there, so the rule is not relaxed to the panel.
static bool sep_form_lds(const SepTables &T, int m)
{
    const char *e = getenv("NLH_SEP_FORM");
    if (e && !strcmp(e, "global")) return false;
    const size_t dyn = sizeof(double) * (size_t)m * ((size_t)T.L + 1 + (size_t)T.n);
    return lds_fits((const void *)k_sep_solve<true>, dyn) && lds_fits((const void *)k_sep_project<true>, dyn);
}

// Both launchers and the solve step.  What they check themselves is refused before any launch.  An inner launcher can refuse
// only once it is called: by then only the context's scratch has been written, nothing of the caller's, and the call
// returns the inner error without a further launch.
enum { SEP_FCN, SEP_JAC, SEP_SOLVE };
static int sep_call(int mode, void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m,
                    double *out, int32_t *drank)
{
    nlh_sep_ctx *c = wrap_ctx<nlh_sep_ctx>(ctx, SEP_MAGIC);
    int end;
    if (wrap_refused(c, c && c->jac && n == c->T.n && m >= c->T.N && dX && out, false, npoints, &end)) return end;
    const SepTables &T = c->T;
    hipStream_t s = (hipStream_t)hip_stream;
    const size_t N = (size_t)T.N, L = (size_t)T.L, ms = (size_t)m;
    const bool jac = mode == SEP_JAC, solve = mode == SEP_SOLVE;
    const bool lds = sep_form_lds(T, m);
    const int cg = std::min(32, T.n);                             // columns of D per workgroup of the projection
    // scratch per point: p0 [N], the inner Jacobian at p0 [N][m], f0 [m], tau [L], p^ [N] (the solve step: the caller's), and
    // for a Jacobian call the inner Jacobian at p^ [N][m]
    const size_t per = N + N * ms + ms + L + (solve ? 0 : N) + (jac ? N * ms : 0);
    return wrap_slices(c->scratch, "NLH_SEP_SCRATCH", c->device, s, per, npoints, m, dprob,
                       [&](double *base, int slice, int q0, int cnt, const int32_t *lp) {
        const size_t sl = (size_t)slice;
        double *P0 = base, *JF = P0 + sl * N, *F0 = JF + sl * N * ms, *TAU = F0 + sl * ms, *PH = TAU + sl * L;
        double *JD = PH + sl * N;
        if (solve) PH = out + (size_t)q0 * N;
        const double *Xs = dX + (size_t)q0 * n;
        hipLaunchKernelGGL(k_sep_expand0, dim3((unsigned)(((size_t)cnt * N + 255) / 256)), dim3(256), 0, s, T, cnt, Xs, P0);
        if (const int rc = c->jac(c->inner, hip_stream, cnt, lp, T.N, P0, m, JF)) return rc;
        if (const int rc = c->fcn(c->inner, hip_stream, cnt, lp, T.N, P0, m, F0)) return rc;
        int32_t *rk = drank ? drank + q0 : nullptr;
        if (lds) hipLaunchKernelGGL(k_sep_solve<true>, dim3(cnt), dim3(256), sizeof(double) * ms * (L + 1), s, T, m, jac ? 1 : 0, JF, F0, Xs, PH, TAU, rk);
        else hipLaunchKernelGGL(k_sep_solve<false>, dim3(cnt), dim3(256), 0, s, T, m, jac ? 1 : 0, JF, F0, Xs, PH, TAU, rk);
        if (solve) return 0;
        if (!jac) return c->fcn(c->inner, hip_stream, cnt, lp, T.N, PH, m, out + (size_t)q0 * ms);
        if (const int rc = c->jac(c->inner, hip_stream, cnt, lp, T.N, PH, m, JD)) return rc;
        double *J = out + (size_t)q0 * ms * n;
        const dim3 grid((unsigned)cnt, (unsigned)((T.n + cg - 1) / cg));
        if (lds) hipLaunchKernelGGL(k_sep_project<true>, grid, dim3(256), sizeof(double) * ms * (L + cg), s, T, m, cg, JF, TAU, JD, J);
        else hipLaunchKernelGGL(k_sep_project<false>, grid, dim3(256), 0, s, T, m, cg, JF, TAU, JD, J);
        return 0;
    });
}

int nlh_sep_device_fcn(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dF)
{
    return sep_call(SEP_FCN, ctx, hip_stream, npoints, dprob, n, dX, m, dF, nullptr);
}

int nlh_sep_device_jac(void *ctx, void *hip_stream, int32_t npoints, const int32_t *dprob, int32_t n, const double *dX, int32_t m, double *dJ)
{
    return sep_call(SEP_JAC, ctx, hip_stream, npoints, dprob, n, dX, m, dJ, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------------
// gather, solve
// ---------------------------------------------------------------------------------------------------------------------
int nlh_sep_gather_batch(nlh_handle *h, const nlh_sep *sp, int32_t nprob, const double *dfull, double *dx)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!sp || nprob < 0) return NLH_INVALID_INPUT_ERROR;
    if (((size_t)nprob * sp->nfull + 255) / 256 > 0x7fffffffu) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0) return 0;
    if (!dfull || !dx) return NLH_INVALID_INPUT_ERROR;
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(k_sep_gather, dim3((unsigned)(((size_t)nprob * sp->nfull + 255) / 256)), dim3(256), 0, h->stream, sep_tables(sp), nprob,
                       dfull, dx);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_sep_solve_batch(nlh_handle *h, nlh_sep_ctx *c, int32_t nprob, int32_t m, const double *dalpha, double *dfull, int32_t *drank)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!c || c->magic != SEP_MAGIC || nprob < 0 || c->device != h->device) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    if (m < c->T.N || !dalpha || !dfull) return NLH_INVALID_INPUT_ERROR;
    const int rc = sep_call(SEP_SOLVE, c, h->stream, nprob, nullptr, c->T.n, dalpha, m, dfull, drank);
    if (rc == NLH_OUT_OF_MEMORY_ERROR || rc == NLH_ARRAY_SIZE_ERROR) return rc;      // the scratch of the call
    if (rc) return launcher_failed(h, rc, "separable solve", "inner launcher");
    HIPCHK(h, hipGetLastError());
    return 0;
}
