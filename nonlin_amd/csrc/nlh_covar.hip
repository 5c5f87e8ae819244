// nlh_covar.hip -- parameter covariance of a least-squares fit, batched: MINPACK's covar on the pivoted R that
// nlh_lmfactor_exact produces (nlh_covar, kernels and algorithm in nlh_kernels_covar.h), and the chain a user runs after
// least_squares_solver%solve: F(x), a fresh Jacobian by vfh_jac_fcn's rule, lmfactor, covar, the reduced chi-square, the
// scaling and the standard errors (nlh_lm_covariance*).  Here: which form a call runs, the launches, the workspaces (the
// handle's cvW / cvT / cvH, which nothing else uses: a covariance between two solves leaves their buffers alone), and the
// front ends for device launchers, host arrays and host callbacks (model objects: nlh_dq_model_lm_covariance, nlh_model.hip).
#include "nlh_internal.h"
#include "nlh_kernels_covar.h"

void nlh_covar_init_device(int lds_max)
{
    (void)hipFuncSetAttribute((const void *)k_covar_lane, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_covar_wg<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_covar_wg<false, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
}

enum { CV_LANE = 1, CV_LDS = 2, CV_GLOBAL = 3 };
static const int CV_GROUP_MAX = 32;          // up to here 64 / n problems share a one-wave workgroup

static inline size_t cv_tri(int32_t n) { return (size_t)n * ((size_t)n + 1) / 2; }
static inline int cv_groups(int32_t n) { return n <= CV_GROUP_MAX ? 64 / n : 1; }

// Dynamic LDS of the workgroup form for n columns: what the host compares with the cap before it launches.
int64_t nlh_covar_lds_bytes(int32_t n)
{
    if (n < 1) return 0;
    return (int64_t)(sizeof(double) * cv_tri(n) * (size_t)cv_groups(n));
}

// The form a call runs.  By default: lane per problem up to CV_LANE_MAX columns, the LDS form while its window fits the
// cap, the global-memory window beyond (switch points: profiles/covar_rate.txt).  NLH_COVAR_FORM = lane | lds | global
// (read at every call; tests) forces a form for the sizes that form can hold.
static int cv_form(int32_t n)
{
    const bool lane_ok = n <= CV_LANE_MAX;
    const bool lds_ok = lds_fits((const void *)(n <= CV_GROUP_MAX ? k_covar_wg<true, false> : k_covar_wg<false, false>),
                                 (size_t)nlh_covar_lds_bytes(n));
    if (const char *e = getenv("NLH_COVAR_FORM")) {
        if (!strcmp(e, "lane") && lane_ok) return CV_LANE;
        if (!strcmp(e, "lds") && lds_ok) return CV_LDS;
        if (!strcmp(e, "global")) return CV_GLOBAL;
    }
    return lane_ok ? CV_LANE : (lds_ok ? CV_LDS : CV_GLOBAL);
}

static const size_t CV_GLOBAL_WINDOW_BYTES = (size_t)1 << 30;
static const int64_t CV_SLICE = (int64_t)1 << 30;               // workgroups of one launch

int nlh_covar(nlh_handle *h, int32_t nprob, int32_t n, const double *dR, const int32_t *dipvt, double tol, double *dcov,
              int32_t *drank)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 0 || n < 1) return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0) return 0;
    if (!dR || !dipvt || !dcov || !drank) return NLH_INVALID_INPUT_ERROR;
    if (!(tol > 0.0)) tol = DBL_EPSILON;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int form = cv_form(n);
    Timed timed(h, NLH_K_COVAR);
    if (form == CV_LANE) {
        const size_t lds = sizeof(double) * 64 * ((size_t)n * n + n);
        if (!lds_fits((const void *)k_covar_lane, lds)) return NLH_ARRAY_SIZE_ERROR;
        for (int64_t p0 = 0; p0 < nprob; p0 += CV_SLICE) {
            const int64_t cnt = std::min<int64_t>(CV_SLICE, nprob - p0);
            hipLaunchKernelGGL(k_covar_lane, dim3((unsigned)((cnt + 63) / 64)), dim3(64), lds, s, cnt, n, dR + (size_t)p0 * n * n,
                               dipvt + (size_t)p0 * n, tol, dcov + (size_t)p0 * n * n, drank + p0);
        }
    } else if (form == CV_LDS) {
        const size_t lds = (size_t)nlh_covar_lds_bytes(n);
        if (n <= CV_GROUP_MAX) {
            const int G = cv_groups(n);
            if (!lds_fits((const void *)k_covar_wg<true, false>, lds)) return NLH_ARRAY_SIZE_ERROR;
            const int64_t blocks = ((int64_t)nprob + G - 1) / G;
            hipLaunchKernelGGL((k_covar_wg<true, false>), dim3((unsigned)blocks), dim3(64), lds, s, (int64_t)0, (int64_t)nprob, n, G, n,
                               dR, dipvt, tol, dcov, drank, (double *)nullptr, (size_t)0);
        } else {
            if (!lds_fits((const void *)k_covar_wg<false, false>, lds)) return NLH_ARRAY_SIZE_ERROR;
            const int T = std::min(1024, (n + 63) / 64 * 64);
            hipLaunchKernelGGL((k_covar_wg<false, false>), dim3((unsigned)nprob), dim3(T), lds, s, (int64_t)0, (int64_t)nprob, n, 1, T,
                               dR, dipvt, tol, dcov, drank, (double *)nullptr, (size_t)0);
        }
    } else {
        const size_t stride = cv_tri(n);
        const int64_t fit = (int64_t)std::max<size_t>(1, CV_GLOBAL_WINDOW_BYTES / (sizeof(double) * stride));
        const int64_t slice = std::min<int64_t>(fit, nprob);
        int rc;
        if ((rc = ensure(h, h->cvT, sizeof(double) * stride * (size_t)slice))) return rc;
        const int T = std::min(1024, (n + 63) / 64 * 64);
        for (int64_t p0 = 0; p0 < nprob; p0 += slice) {            // one stream: a slice's windows are free when the next starts
            const int64_t cnt = std::min<int64_t>(slice, nprob - p0);
            hipLaunchKernelGGL((k_covar_wg<false, true>), dim3((unsigned)cnt), dim3(T), 0, s, p0, p0 + cnt, n, 1, T, dR, dipvt, tol,
                               dcov, drank, (double *)h->cvT.p, stride);
        }
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the chain
// ---------------------------------------------------------------------------------------------------------------------
struct CvWs {                          // carved from h->cvW for cnt problems
    double *f, *J, *P, *R, *rdiag, *acnorm, *qtf, *wa4, *chi2;
    int32_t *ipvt, *rank;
};

static int cv_workspace(nlh_handle *h, int cnt, int m, int n, bool panel, CvWs &w)
{
    const size_t c = (size_t)cnt, mn = (size_t)m * n;
    const size_t doubles = c * (2 * (size_t)m + mn + (panel ? mn : 0) + (size_t)n * n + 3 * (size_t)n + 1);
    int rc;
    if ((rc = ensure(h, h->cvW, sizeof(double) * doubles + sizeof(int32_t) * c * ((size_t)n + 1) + 64))) return rc;
    double *q = (double *)h->cvW.p;
    w.f = q; q += c * m;
    w.wa4 = q; q += c * m;
    w.J = q; q += c * mn;
    w.P = panel ? q : nullptr; q += panel ? c * mn : 0;
    w.R = q; q += c * n * n;
    w.rdiag = q; q += c * n;
    w.acnorm = q; q += c * n;
    w.qtf = q; q += c * n;
    w.chi2 = q; q += c;
    w.ipvt = (int32_t *)q;
    w.rank = w.ipvt + c * n;
    return 0;
}

static int cv_check(int32_t m, int32_t n, int32_t scaled)
{
    if (m < 1 || n < 1) return NLH_INVALID_INPUT_ERROR;
    if (scaled && m <= n) return NLH_INVALID_INPUT_ERROR;       // no degree of freedom to estimate the variance from
    if (m < n) return NLH_UNDERDEFINED_PROBLEM_ERROR;           // src/nonlin_least_squares.f90:189
    return 0;
}

// lmfactor of w.J (with Q^T f of w.f), covar, chi2, the scaling and sigma for cnt problems: device outputs, any of dsigma,
// drank, dchi2 NULL.
static int cv_tail(nlh_handle *h, int cnt, int m, int n, CvWs &w, int32_t scaled, double tol, double *dcov, double *dsigma,
                   int32_t *drank, double *dchi2)
{
    int rc;
    // (R's lower triangle is never read; lmfactor writes the upper one and the diagonal)
    if ((rc = nlh_lmfactor_exact(h, cnt, m, n, w.J, w.f, w.R, w.ipvt, w.rdiag, w.acnorm, w.qtf, w.wa4))) return rc;
    if ((rc = nlh_covar(h, cnt, n, w.R, w.ipvt, tol, dcov, drank ? drank : w.rank))) return rc;
    double *chi2 = dchi2 ? dchi2 : w.chi2;
    if (scaled || dchi2)
        hipLaunchKernelGGL(k_covar_chi2, dim3((cnt + 63) / 64), dim3(64), 0, h->stream, cnt, m, n, (const double *)w.f, chi2);
    if (scaled || dsigma) {
        const size_t total = (size_t)cnt * n * n;
        hipLaunchKernelGGL(k_covar_scale, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, total, n, dcov,
                           scaled ? (const double *)chi2 : (const double *)nullptr, dsigma);
    }
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_lm_covariance_batch_device(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                                   nlh_device_jacfcn jacfcn, void *ctx, const double *dx, int32_t scaled, double tol, double *dcov,
                                   double *dsigma, int32_t *drank, double *dchi2)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (nprob <= 0) return 0;
    if (!dx || !dcov) return NLH_INVALID_INPUT_ERROR;
    int rc = cv_check(m, n, scaled);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const ResidualSource rs = ResidualSource::launchers(fcn, jacfcn, ctx);
    return lockstep_slices(nprob, slice_panel(m, n), [&](int32_t p0, int32_t cnt) {
        int rcs;
        CvWs w;
        if ((rcs = cv_workspace(h, cnt, m, n, false, w))) return rcs;
        const ResidualSource r = rs.shifted(p0, m, n);
        const double *xs = dx + (size_t)p0 * n;
        if ((rcs = residual_eval(h, r, cnt, m, n, xs, w.f, nullptr, nullptr, -1))) return rcs;
        if ((rcs = residual_jacobian(h, r, cnt, m, n, xs, w.f, w.J, nullptr, nullptr, -1, false, false, true))) return rcs;
        return cv_tail(h, cnt, m, n, w, scaled, tol, dcov + (size_t)p0 * n * n, dsigma ? dsigma + (size_t)p0 * n : nullptr,
                       drank ? drank + p0 : nullptr, dchi2 ? dchi2 + p0 : nullptr);
    });
}

// device staging of the host-array forms (h->cvH): x, cov, sigma, chi2, rank for nprob problems
struct CvHost { double *x, *cov, *sigma, *chi2; int32_t *rank; };

static int cv_host_stage(nlh_handle *h, int32_t nprob, int32_t n, CvHost &d)
{
    const size_t c = (size_t)nprob;
    int rc;
    if ((rc = ensure(h, h->cvH, sizeof(double) * c * ((size_t)n * n + 2 * (size_t)n + 1) + sizeof(int32_t) * c))) return rc;
    d.x = (double *)h->cvH.p;
    d.cov = d.x + c * n;
    d.sigma = d.cov + c * n * n;
    d.chi2 = d.sigma + c * n;
    d.rank = (int32_t *)(d.chi2 + c);
    return 0;
}

static int cv_host_fetch(nlh_handle *h, int32_t nprob, int32_t n, const CvHost &d, double *cov, double *sigma, int32_t *rank,
                         double *chi2)
{
    const size_t c = (size_t)nprob;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(cov, d.cov, sizeof(double) * c * n * n, hipMemcpyDeviceToHost, s));
    if (sigma) HIPCHK(h, hipMemcpyAsync(sigma, d.sigma, sizeof(double) * c * n, hipMemcpyDeviceToHost, s));
    if (rank) HIPCHK(h, hipMemcpyAsync(rank, d.rank, sizeof(int32_t) * c, hipMemcpyDeviceToHost, s));
    if (chi2) HIPCHK(h, hipMemcpyAsync(chi2, d.chi2, sizeof(double) * c, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return 0;
}

int nlh_lm_covariance_batch_device_h(nlh_handle *h, int32_t nprob, int32_t m, int32_t n, nlh_device_vecfcn fcn,
                                     nlh_device_jacfcn jacfcn, void *ctx, const double *x, int32_t scaled, double tol, double *cov,
                                     double *sigma, int32_t *rank, double *chi2)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (nprob <= 0) return 0;
    if (!x || !cov) return NLH_INVALID_INPUT_ERROR;
    int rc = cv_check(m, n, scaled);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    CvHost d;
    if ((rc = cv_host_stage(h, nprob, n, d))) return rc;
    HIPCHK(h, hipMemcpyAsync(d.x, x, sizeof(double) * (size_t)nprob * n, hipMemcpyHostToDevice, h->stream));
    if ((rc = nlh_lm_covariance_batch_device(h, nprob, m, n, fcn, jacfcn, ctx, d.x, scaled, tol, d.cov, sigma ? d.sigma : nullptr,
                                             d.rank, d.chi2))) return rc;
    return cv_host_fetch(h, nprob, n, d, cov, sigma, rank, chi2);
}

// One problem, HOST callbacks: fcn at x, then vfh_jac_fcn (the user's jacobianfcn, or the n perturbed evaluations in
// ascending j with x perturbed in place and restored) -- the reference's order; everything after that on the device.
int nlh_lm_covariance(nlh_handle *h, int32_t m, int32_t n, nlh_vecfcn fcn, nlh_jacfcn jacfcn, void *ctx, double *x,
                      int32_t scaled, double tol, double *cov, double *sigma, int32_t *rank, double *chi2)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (!fcn) return NLH_UNDEFINED_FUNCTION_ERROR;
    if (!x || !cov) return NLH_INVALID_INPUT_ERROR;
    int rc = cv_check(m, n, scaled);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t mn = (size_t)m * n;
    CvWs w;
    CvHost d;
    if ((rc = cv_workspace(h, 1, m, n, true, w))) return rc;
    if ((rc = cv_host_stage(h, 1, n, d))) return rc;
    if ((rc = ensure_pinned(h, sizeof(double) * (mn + m)))) return rc;
    double *hP = (double *)h->pinned, *hf = hP + mn;
    hipStream_t s = h->stream;
    fcn(ctx, n, x, m, hf);
    HIPCHK(h, hipMemcpyAsync(w.f, hf, sizeof(double) * m, hipMemcpyHostToDevice, s));
    if (jacfcn) {                                                // src/nonlin_multi_eqn_mult_var.f90:241-243
        jacfcn(ctx, n, x, m, hP);
        HIPCHK(h, hipMemcpyAsync(w.J, hP, sizeof(double) * mn, hipMemcpyHostToDevice, s));
    } else {
        for (int j = 0; j < n; ++j) {                            // :267-273
            const double temp = x[j];
            double hh = NLH_SQRT_EPS * fabs(temp);
            if (hh == 0.0) hh = NLH_SQRT_EPS;
            x[j] = temp + hh;
            fcn(ctx, n, x, m, hP + (size_t)j * m);
            x[j] = temp;
        }
        HIPCHK(h, hipMemcpyAsync(w.P, hP, sizeof(double) * mn, hipMemcpyHostToDevice, s));
        HIPCHK(h, hipMemcpyAsync(d.x, x, sizeof(double) * n, hipMemcpyHostToDevice, s));
        launch_fd(h, 1, m, n, w.P, w.f, d.x, w.J, nullptr, -1);  // :274
    }
    if ((rc = cv_tail(h, 1, m, n, w, scaled, tol, d.cov, sigma ? d.sigma : nullptr, d.rank, d.chi2))) return rc;
    return cv_host_fetch(h, 1, n, d, cov, sigma, rank, chi2);
}
