// nlh_guess.hip -- starting values for the built-in curve models (include/nonlin_hip_guess.h: nlh_curve_guess_batch; kernels and
// arithmetic: nlh_kernels_guess.h).  Two stages: the nonlinear values -- mu and width of each peak from the detrended, smoothed
// data; k of each decay from the integral-equation regression, whose least squares is k_sep_solve on a panel of the call's own
// --, then the amplitudes and the baseline by nlh_sep_solve_batch on the curve launchers over the caller's t, y, w.
#include "nlh_internal.h"
#include "nlh_launch.h"
#include "nlh_kernels_sep.h"
#include "nlh_kernels_guess.h"

void nlh_guess_init_device(int lds_max)
{
    (void)hipFuncSetAttribute((const void *)k_guess_peaks<NLH_CURVE_GAUSS>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_guess_peaks<NLH_CURVE_LORENTZ>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_guess_decay_panel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_sep_solve<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
}

// What is refused before anything else is looked at, in the header's order; 0: the call goes on.
static int guess_refused(const nlh_handle *h, int32_t kind, int32_t K, int32_t B, int32_t nprob, int32_t m, const double *t, const double *y,
                         int32_t smooth, const double *x)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    const int32_t n = nlh_curve_nparams(kind, K, B);
    if (n < 0 || nprob < 0 || m < 1 || !t || !y || !x || smooth < 0 || m > NLH_GUESS_MAX_M) return NLH_INVALID_INPUT_ERROR;
    if (kind == NLH_CURVE_EXPDECAY ? K > 2 : K + B + 1 > NLH_SEP_MAX_L) return NLH_INVALID_INPUT_ERROR;
    if (m < n) return NLH_UNDERDEFINED_PROBLEM_ERROR;
    return 0;
}

// The decays' regression in slices of problems: a slice's panel [cnt][L + 1][m] stays inside this many bytes.
static const size_t GUESS_PANEL_BYTES = (size_t)256 << 20;

static int guess_decays(nlh_handle *h, const GuessData &gd, int nprob, double *alpha, int32_t *fl, double *span)
{
    const int K = gd.K, L = 2 * K + gd.B + 1, m = gd.m;
    const size_t ms = (size_t)m, per = sizeof(double) * ((size_t)(L + 1) * ms + 2 * (size_t)L) + sizeof(int32_t);
    const int slice = (int)std::max<size_t>(1, std::min<size_t>((size_t)nprob, GUESS_PANEL_BYTES / per));
    int rc;
    if ((rc = ensure(h, h->guessP, (size_t)slice * per + 64))) return rc;
    double *JF = (double *)h->guessP.p, *F0 = JF + (size_t)slice * L * ms, *C = F0 + (size_t)slice * ms, *TAU = C + (size_t)slice * L;
    int32_t *rank = (int32_t *)(TAU + (size_t)slice * L);
    SepTables T{};                                                  // every column of the panel is a linear one
    T.N = L; T.L = L; T.n = 0;
    for (int l = 0; l < L; ++l) T.lin[l] = l;
    const size_t lds_panel = sizeof(double) * 2 * ms, lds_solve = sizeof(double) * ms * (size_t)(L + 1);
    if (!lds_fits((const void *)k_guess_decay_panel, lds_panel)) return NLH_ARRAY_SIZE_ERROR;
    const bool lds = lds_fits((const void *)k_sep_solve<true>, lds_solve);
    for (int p0 = 0; p0 < nprob; p0 += slice) {
        const int cnt = std::min(slice, nprob - p0);
        hipLaunchKernelGGL(k_guess_decay_panel, dim3(cnt), dim3(256), lds_panel, h->stream, gd, p0, JF, F0, span, fl);
        if (lds) hipLaunchKernelGGL(k_sep_solve<true>, dim3(cnt), dim3(256), lds_solve, h->stream, T, m, 0, JF, F0, (const double *)nullptr, C, TAU, rank);
        else hipLaunchKernelGGL(k_sep_solve<false>, dim3(cnt), dim3(256), 0, h->stream, T, m, 0, JF, F0, (const double *)nullptr, C, TAU, rank);
        hipLaunchKernelGGL(k_guess_rates, dim3((cnt + 255) / 256), dim3(256), 0, h->stream, K, L, cnt, p0, C, rank, span, alpha, fl);
    }
    return 0;
}

int nlh_curve_guess_batch(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *dt,
                          int32_t shared_t, const double *dy, const double *dw, int32_t smooth, double *dx, int32_t *dflag)
{
    int rc;
    if ((rc = guess_refused(h, kind, ncomp, nbase, nprob, m, dt, dy, smooth, dx))) return rc;
    if (nprob == 0) return 0;
    const int32_t n = nlh_curve_nparams(kind, ncomp, nbase);
    const bool decay = kind == NLH_CURVE_EXPDECAY;
    const int nn = decay ? ncomp : 2 * ncomp, L = n - nn;
    HIPCHK(h, hipSetDevice(h->device));
    // alpha [nprob][nn], span [nprob], the nonlinear stage's flags and the linear stage's live columns [nprob] each
    const size_t np = (size_t)nprob;
    if ((rc = ensure(h, h->guessA, sizeof(double) * (np * nn + np) + 2 * sizeof(int32_t) * np))) return rc;
    double *alpha = (double *)h->guessA.p, *span = alpha + np * nn;
    int32_t *fl = (int32_t *)(span + np), *rank = fl + np;
    GuessData gd;
    gd.K = ncomp; gd.B = nbase; gd.shared_t = shared_t != 0; gd.m = m; gd.n = n; gd.smooth = std::min(smooth, m);
    gd.t = dt; gd.y = dy; gd.w = dw;
    if (decay) {
        if ((rc = guess_decays(h, gd, nprob, alpha, fl, span))) return rc;
    } else {
        const size_t lds = sizeof(double) * 2 * (size_t)m + (size_t)m;
        const void *k = kind == NLH_CURVE_GAUSS ? (const void *)k_guess_peaks<NLH_CURVE_GAUSS> : (const void *)k_guess_peaks<NLH_CURVE_LORENTZ>;
        if (!lds_fits(k, lds)) return NLH_ARRAY_SIZE_ERROR;         // (m <= NLH_GUESS_MAX_M fits: asked all the same before the launch)
        if (kind == NLH_CURVE_GAUSS) hipLaunchKernelGGL(k_guess_peaks<NLH_CURVE_GAUSS>, dim3(nprob), dim3(256), lds, h->stream, gd, alpha, fl);
        else hipLaunchKernelGGL(k_guess_peaks<NLH_CURVE_LORENTZ>, dim3(nprob), dim3(256), lds, h->stream, gd, alpha, fl);
    }
    HIPCHK(h, hipGetLastError());
    // the linear stage: the amplitudes and the baseline at alpha, on the caller's own t, y, w
    std::vector<int32_t> lin;
    const int per = decay ? 2 : 3;
    for (int c = 0; c < ncomp; ++c) lin.push_back(per * c);
    for (int k = per * ncomp; k < n; ++k) lin.push_back(k);
    nlh_sep *sp = nullptr;
    if (nlh_sep_create(n, L, lin.data(), &sp)) return NLH_INVALID_INPUT_ERROR;
    nlh_curve_ctx cc;
    cc.kind = kind; cc.ncomp = ncomp; cc.nbase = nbase; cc.shared_t = shared_t != 0; cc.m = m; cc.dt = dt; cc.dy = dy; cc.dw = dw;
    nlh_sep_ctx *sc = nullptr;
    rc = nlh_sep_wrap(h, sp, nlh_curve_device_fcn, nlh_curve_device_jac, &cc, &sc);
    if (!rc) rc = nlh_sep_solve_batch(h, sc, nprob, m, alpha, dx, rank);
    if (!rc) {
        hipLaunchKernelGGL(k_guess_finish, dim3((nprob + 255) / 256), dim3(256), 0, h->stream, n, L, nprob, rank, fl, dx, dflag);
        if (hipGetLastError() != hipSuccess) { h->err = "curve guess: launch failed"; rc = NLH_ERR_HIP; }
    }
    nlh_sep_unwrap(sc);                                             // (frees the context's scratch: waits for the work that uses it)
    nlh_sep_destroy(sp);
    return rc;
}

int nlh_curve_guess_batch_h(nlh_handle *h, int32_t kind, int32_t ncomp, int32_t nbase, int32_t nprob, int32_t m, const double *t,
                            int32_t shared_t, const double *y, const double *w, int32_t smooth, double *x, int32_t *flag)
{
    int rc;
    if ((rc = guess_refused(h, kind, ncomp, nbase, nprob, m, t, y, smooth, x))) return rc;
    if (nprob == 0) return 0;
    const size_t n = (size_t)nlh_curve_nparams(kind, ncomp, nbase), pm = (size_t)nprob * m;
    const size_t tb = sizeof(double) * (shared_t ? (size_t)m : pm), yb = sizeof(double) * pm, wb = w ? yb : 0;
    const size_t xb = sizeof(double) * (size_t)nprob * n, fb = sizeof(int32_t) * (size_t)nprob;
    HIPCHK(h, hipSetDevice(h->device));
    if ((rc = ensure(h, h->guessH, tb + yb + wb + xb + fb))) return rc;
    char *base = (char *)h->guessH.p;
    double *dt = (double *)base, *dy = (double *)(base + tb), *dw = w ? (double *)(base + tb + yb) : nullptr;
    double *dx = (double *)(base + tb + yb + wb);
    int32_t *df = (int32_t *)(base + tb + yb + wb + xb);
    HIPCHK(h, hipMemcpyAsync(dt, t, tb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dy, y, yb, hipMemcpyHostToDevice, h->stream));
    if (w) HIPCHK(h, hipMemcpyAsync(dw, w, wb, hipMemcpyHostToDevice, h->stream));
    if ((rc = nlh_curve_guess_batch(h, kind, ncomp, nbase, nprob, m, dt, shared_t, dy, dw, smooth, dx, df))) return rc;
    HIPCHK(h, hipMemcpyAsync(x, dx, xb, hipMemcpyDeviceToHost, h->stream));
    if (flag) HIPCHK(h, hipMemcpyAsync(flag, df, fb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}
