// nlh_boot.hip -- bootstrap (include/nonlin_hip_boot.h: nlh_boot_*; kernels: nlh_kernels_boot.h): the generator's draws on the
// host, the resampling kernel's launch shape, and the summary of the refits.  The fits between the two are the caller's.
// Also the Poisson bootstrap (include/nonlin_hip_boot_pois.h: nlh_boot_poisson_*): its draws on the host and its kernel's launch.
#include "nlh_internal.h"
#include "nlh_kernels_boot.h"

void nlh_boot_init_device(int lds_max)
{
    (void)hipFuncSetAttribute((const void *)k_boot_resample<NLH_BOOT_RESIDUAL, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_boot_resample<NLH_BOOT_RESIDUAL, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_boot_resample<NLH_BOOT_PAIRS, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipFuncSetAttribute((const void *)k_boot_resample<NLH_BOOT_PAIRS, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
}

int nlh_boot_draws(uint64_t seed, int64_t p, int32_t b, int32_t first, int32_t count, int32_t cnt, int32_t *out)
{
    if (p < 0 || b < 0 || first < 0 || count < 0 || (int64_t)first + count > NLH_BOOT_MAX_ROWS || cnt < 0 || cnt > NLH_BOOT_MAX_ROWS ||
        (count > 0 && !out))
        return NLH_INVALID_INPUT_ERROR;
    const uint64_t key = boot_key(seed, (uint64_t)p, (uint64_t)b);
    for (int32_t k = 0; k < count; ++k) {
        const uint64_t z = boot_draw(key, (uint64_t)first + (uint64_t)k);
        out[k] = cnt ? (int32_t)boot_index(z, (uint32_t)cnt) : (int32_t)(z >> 63);
    }
    return 0;
}

// The resampling kernel of a kind and a store width
typedef void (*boot_kernel)(uint64_t, int, long long, int, int, int, int, int, const double *, const double *, const double *, int, double *,
                            double *);
static boot_kernel boot_pick(int kind, int V)
{
    switch (kind) {
    case NLH_BOOT_RESIDUAL: return V == 2 ? k_boot_resample<NLH_BOOT_RESIDUAL, 2> : k_boot_resample<NLH_BOOT_RESIDUAL, 1>;
    case NLH_BOOT_WILD: return V == 2 ? k_boot_resample<NLH_BOOT_WILD, 2> : k_boot_resample<NLH_BOOT_WILD, 1>;
    default: return V == 2 ? k_boot_resample<NLH_BOOT_PAIRS, 2> : k_boot_resample<NLH_BOOT_PAIRS, 1>;
    }
}

int nlh_boot_resample_batch(nlh_handle *h, int32_t kind, uint64_t seed, int32_t nprob, int64_t prob0, int32_t m, int32_t rep0,
                            int32_t nrep, const double *dmu, const double *dy, const double *dw, int32_t centre, double *dyout,
                            double *dwout)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (kind < NLH_BOOT_RESIDUAL || kind > NLH_BOOT_PAIRS || nprob < 0 || nrep < 0 || nrep > NLH_BOOT_MAX_REP || m < 1 ||
        m > NLH_BOOT_MAX_ROWS || prob0 < 0 || rep0 < 0 || (int64_t)rep0 + nrep > 0x7fffffffLL || !dy || !dyout ||
        (kind != NLH_BOOT_PAIRS && !dmu) || (kind == NLH_BOOT_PAIRS && !dwout))
        return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0 || nrep == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    // 16-byte stores where every row of the outputs starts on 16 bytes; 1 << tsh threads span a problem's m / V units
    const bool pairs = kind == NLH_BOOT_PAIRS;
    const int V = m % 2 == 0 && (uintptr_t)dyout % 16 == 0 && (!pairs || (uintptr_t)dwout % 16 == 0) ? 2 : 1;
    int tsh = 0;
    while (tsh < 8 && (1 << tsh) < m / V) ++tsh;
    // replicas per workgroup: as many as the keys' LDS holds, fewer while the grid would be under 2048 workgroups
    int groups = (int)std::min<int64_t>(nrep, std::max<int64_t>((nrep + BOOT_RPW - 1) / BOOT_RPW, (2048 + (int64_t)nprob - 1) / nprob));
    const int rpw = (nrep + groups - 1) / groups;
    groups = (nrep + rpw - 1) / rpw;
    const size_t lds = kind == NLH_BOOT_RESIDUAL ? sizeof(double) * (size_t)m : pairs ? sizeof(int) * (size_t)(256 >> tsh) * m : 0;
    hipLaunchKernelGGL(boot_pick(kind, V), dim3((unsigned)nprob, (unsigned)groups), dim3(256), lds, h->stream, seed, nprob,
                       (long long)prob0, m, rep0, nrep, rpw, tsh, dmu, dy, dw, centre, dyout, dwout);
    HIPCHK(h, hipGetLastError());
    return 0;
}

// ---- Poisson bootstrap (include/nonlin_hip_boot_pois.h) ----
int nlh_boot_poisson_draws(uint64_t seed, int64_t p, int32_t b, int32_t first, int32_t count, const double *mu, double *out)
{
    if (p < 0 || b < 0 || first < 0 || count < 0 || (int64_t)first + count > NLH_BOOT_MAX_ROWS || (count > 0 && (!mu || !out)))
        return NLH_INVALID_INPUT_ERROR;
    const uint64_t key = boot_key(seed, (uint64_t)p, (uint64_t)b);
    for (int32_t j = 0; j < count; ++j) {
        const boot_pois s = boot_pois_row(true, mu[j]);
        out[j] = s.T > 0.0 ? boot_pois_draw(s, mu[j], boot_draw(key, (uint64_t)first + (uint64_t)j))
                           : s.T == 0.0 ? 0.0 : (double)NAN;
    }
    return 0;
}

int nlh_boot_poisson_batch(nlh_handle *h, uint64_t seed, int32_t nprob, int64_t prob0, int32_t m, int32_t rep0, int32_t nrep,
                           const double *dmu, const double *dy, const double *dw, double *dyout, int32_t *dbad)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nprob < 0 || nrep < 0 || nrep > NLH_BOOT_MAX_REP || m < 1 || m > NLH_BOOT_MAX_ROWS || prob0 < 0 || rep0 < 0 ||
        (int64_t)rep0 + nrep > 0x7fffffffLL || !dmu || !dy || !dyout || !dbad)
        return NLH_INVALID_INPUT_ERROR;
    if (nprob == 0 || nrep == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    // nlh_boot_resample_batch's launch shape; several replica slots (tsh < 8, so m <= 256) share a row's setup through LDS
    const int V = m % 2 == 0 && (uintptr_t)dyout % 16 == 0 ? 2 : 1;
    int tsh = 0;
    while (tsh < 8 && (1 << tsh) < m / V) ++tsh;
    int groups = (int)std::min<int64_t>(nrep, std::max<int64_t>((nrep + BOOT_RPW - 1) / BOOT_RPW, (2048 + (int64_t)nprob - 1) / nprob));
    const int rpw = (nrep + groups - 1) / groups;
    groups = (nrep + rpw - 1) / rpw;
    const size_t lds = tsh < 8 ? 6 * sizeof(double) * (size_t)m : 0;
    hipLaunchKernelGGL(V == 2 ? k_boot_poisson<2> : k_boot_poisson<1>, dim3((unsigned)nprob, (unsigned)groups), dim3(256), lds, h->stream,
                       seed, nprob, (long long)prob0, m, rep0, nrep, rpw, tsh, dmu, dy, dw, dyout, dbad);
    HIPCHK(h, hipGetLastError());
    return 0;
}

int nlh_boot_summary_batch(nlh_handle *h, int32_t nrep, int32_t nprob, int32_t n, const double *dxs, double level, double *dmean,
                           double *dsd, double *dlo, double *dhi, int32_t *dnvalid)
{
    if (!h) return NLH_ERR_BAD_HANDLE;
    if (nrep < 1 || nrep > NLH_BOOT_MAX_REP || nprob < 0 || n < 1 || !(level > 0.0 && level < 1.0) || !dxs || !dmean || !dsd || !dlo ||
        !dhi || !dnvalid)
        return NLH_INVALID_INPUT_ERROR;
    if ((int64_t)nprob * n > 0x7fffffffLL || (int64_t)nprob * nrep > 0x7fffffffLL) return NLH_ARRAY_SIZE_ERROR;
    if (nprob == 0) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    const size_t total = (size_t)nrep * nprob;
    if ((rc = ensure(h, h->bootV, total))) return rc;
    unsigned char *valid = (unsigned char *)h->bootV.p;
    const double qlo = (1.0 - level) / 2.0, qhi = 1.0 - qlo;
    hipLaunchKernelGGL(k_boot_valid, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, total, n, dxs, valid);
    hipLaunchKernelGGL(k_boot_summary, dim3((unsigned)((size_t)nprob * n)), dim3(256), 0, h->stream, nrep, nprob, n, dxs, valid, qlo, qhi,
                       dmean, dsd, dlo, dhi, dnvalid);
    HIPCHK(h, hipGetLastError());
    return 0;
}
