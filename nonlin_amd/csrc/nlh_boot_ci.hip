// nlh_boot_ci.hip -- the studentised and the BCa interval of the bootstrap (include/nonlin_hip_boot_ci.h: nlh_boot_student_batch,
// nlh_boot_jackknife_batch, nlh_boot_accel_batch, nlh_boot_bca_batch, nlh_boot_bca_levels; kernels: nlh_kernels_boot_ci.h).  The
// refusals follow nlh_boot_summary_batch; the fits between the calls are the caller's.
#include "nlh_internal.h"
#include "nlh_kernels_boot_ci.h"

static bool boot_level_ok(double level) { return level > 0.0 && level < 1.0; }

int nlh_boot_bca_levels(int32_t c2, int32_t cnt, double a, double level, double *z0, double *alpha_lo, double *alpha_hi, int32_t *flag)
{
    if (cnt < 0 || cnt > NLH_BOOT_MAX_REP || c2 < 0 || c2 > 2 * cnt || !boot_level_ok(level) || !z0 || !alpha_lo || !alpha_hi || !flag)
        return NLH_INVALID_INPUT_ERROR;
    if (cnt == 0) {
        *z0 = *alpha_lo = *alpha_hi = boot_nan();
        *flag = NLH_BCA_NO_REPLICA;
        return 0;
    }
    const double qlo = (1.0 - level) / 2.0, qhi = 1.0 - qlo;
    double alpha[2];
    *flag = boot_bca_levels(c2, cnt, a, qlo, qhi, boot_ppnd16(qlo), boot_ppnd16(qhi), z0, alpha);
    *alpha_lo = alpha[0];
    *alpha_hi = alpha[1];
    return 0;
}

// nlh_boot_summary_batch's validity pass: h->bootV [nrep][nprob], a byte each
static int boot_valid_pass(nlh_handle *h, int nrep, int nprob, int n, const double *dxs, unsigned char **valid)
{
    int rc;
    const size_t total = (size_t)nrep * nprob;
    if ((rc = ensure(h, h->bootV, total))) return rc;
    *valid = (unsigned char *)h->bootV.p;
    hipLaunchKernelGGL(k_boot_valid, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, total, n, dxs, *valid);
    return 0;
}

int nlh_boot_student_batch(nlh_handle *h, int32_t nrep, int32_t nprob, int32_t n, const double *dxs, const double *dsigs,
                           const double *dx, const double *dsigma, double level, double *dlo, double *dhi, int32_t *dnvalid_t)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nrep < 1 || nrep > NLH_BOOT_MAX_REP || nprob < 0 || n < 1 || !boot_level_ok(level) || !dxs || !dsigs || !dx || !dsigma || !dlo ||
        !dhi || !dnvalid_t)
        return NLH_INVALID_INPUT_ERROR;
    if ((int64_t)nprob * n > 0x7fffffffLL || (int64_t)nprob * nrep > 0x7fffffffLL) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    unsigned char *valid;
    if ((rc = boot_valid_pass(h, nrep, nprob, n, dxs, &valid))) return rc;
    const double qlo = (1.0 - level) / 2.0, qhi = 1.0 - qlo;
    hipLaunchKernelGGL(k_boot_student, dim3((unsigned)((size_t)nprob * n)), dim3(256), 0, h->stream, nrep, nprob, n, dxs, dsigs, valid, dx,
                       dsigma, qlo, qhi, dlo, dhi, dnvalid_t);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_boot_bca_batch(nlh_handle *h, int32_t nrep, int32_t nprob, int32_t n, const double *dxs, const double *dx, const double *daccel,
                       double level, double *dlo, double *dhi, double *dz0, double *dalpha_lo, double *dalpha_hi, int32_t *dflags,
                       int32_t *dnvalid)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nrep < 1 || nrep > NLH_BOOT_MAX_REP || nprob < 0 || n < 1 || !boot_level_ok(level) || !dxs || !dx || !daccel || !dlo || !dhi ||
        !dz0 || !dalpha_lo || !dalpha_hi || !dflags || !dnvalid)
        return NLH_INVALID_INPUT_ERROR;
    if ((int64_t)nprob * n > 0x7fffffffLL || (int64_t)nprob * nrep > 0x7fffffffLL) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    unsigned char *valid;
    if ((rc = boot_valid_pass(h, nrep, nprob, n, dxs, &valid))) return rc;
    const double qlo = (1.0 - level) / 2.0, qhi = 1.0 - qlo;
    hipLaunchKernelGGL(k_boot_bca, dim3((unsigned)((size_t)nprob * n)), dim3(256), 0, h->stream, nrep, nprob, n, dxs, valid, dx, daccel, qlo,
                       qhi, boot_ppnd16(qlo), boot_ppnd16(qhi), dlo, dhi, dz0, dalpha_lo, dalpha_hi, dflags, dnvalid);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_boot_jackknife_batch(nlh_handle *h, int32_t nprob, int32_t m, int32_t row0, int32_t nrows, const double *dw, double *dwout)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 0 || m < 1 || m > NLH_BOOT_MAX_ROWS || row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > m || !dwout)
        return NLH_INVALID_INPUT_ERROR;
    if ((int64_t)nprob * m > 0x7fffffffLL) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0 || nrows == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    // 16-byte stores where every row of the output starts on 16 bytes
    const int V = m % 2 == 0 && (uintptr_t)dwout % 16 == 0 ? 2 : 1;
    const size_t units = (size_t)nprob * (m / V);
    hipLaunchKernelGGL(V == 2 ? k_boot_jackknife<2> : k_boot_jackknife<1>, dim3((unsigned)((units + 255) / 256), (unsigned)nrows), dim3(256),
                       0, h->stream, nprob, m, row0, dw, dwout);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_boot_accel_batch(nlh_handle *h, int32_t m, int32_t nprob, int32_t n, const double *dxjack, const double *dw, double *daccel,
                         int32_t *dnjack)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (m < 1 || m > NLH_BOOT_MAX_ROWS || nprob < 0 || n < 1 || !dxjack || !daccel || !dnjack) return NLH_INVALID_INPUT_ERROR;
    if ((int64_t)nprob * n > 0x7fffffffLL || (int64_t)nprob * m > 0x7fffffffLL) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    const size_t total = (size_t)m * nprob, pairs = (size_t)nprob * n;
    if ((rc = ensure(h, h->bootV, total))) return rc;
    unsigned char *ok = (unsigned char *)h->bootV.p;
    hipLaunchKernelGGL(k_boot_jack_valid, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, total, m, nprob, n, dxjack, dw, ok);
    hipLaunchKernelGGL(k_boot_accel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, h->stream, m, nprob, n, dxjack, ok, daccel, dnjack);
    HIPCHK(h, hipGetLastError());
    return 0;
}
