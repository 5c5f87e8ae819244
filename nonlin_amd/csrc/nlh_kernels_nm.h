// nlh_kernels_nm.h -- nelder_mead%solve (nm_solve, src/nonlin_optimize.f90:104-340, with nm_extrapolate :343-399) as a
// LOCK-STEP BATCH: every problem carries a phase, one round hands the user's objective every point any problem needs
// next (the n + 1 vertices of the initial simplex, one trial point, or the n new vertices of a shrink), and the advance
// kernel of the following round consumes the values and runs the reference's statements up to the next evaluation.
// One 64-lane wave per problem, four problems per 256-thread block: lane 0 walks the scalar logic (the ranking scan with
// its order-dependent tie rules, the decisions, f and the counters -- on a copy of f in LDS); the lanes stride
// over coordinates for the vertex arithmetic, which no decision depends on.  Every operation is the reference's, in its
// order (separate multiply and subtract under -ffp-contract=off; pcent sums the vertices in ascending order): the batch
// is bit-identical to a sequential restatement of nm_solve, whatever the batch it is solved in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum NmPhase : int32_t {
    NM_INIT = 0,         // the n + 1 vertices of the simplex are due (:216-219)
    NM_REFLECT = 1,      // trial point at fac = -1 due (:275-276)
    NM_EXPAND = 2,       // fac = 2 (:277-282)
    NM_CONTRACT = 3,     // fac = 0.5 (:283-289)
    NM_SHRINK = 4,       // the n vertices i /= ilo, already moved halfway to ilo, are due (:290-299)
    NM_DONE = 5
};

struct NmState {
    double fsave, fval, rtol;         // fval: f(1) of the initial simplex until convergence (:220, :266) -- the stale value
    double pr_fval, pr_rtol;          // the status block (:306-313) of the iteration that ended in the last advance
    int32_t phase, ilo, ihi, ihi2;
    int32_t iter, neval, flag, fcnvrg;
    int32_t print_due, pr_iter, pr_neval, pad;
};

struct NmOpts {
    double ftol, init_size;
    int32_t max_evals, build;         // build: make the initial simplex from x (:183-213); 0: the caller's simplex
};

// The initial simplex (:205-213) and a fresh state.  One wave per problem.
static __global__ void __launch_bounds__(256)
k_nm_reset(int nprob, int n, NmOpts o, const double *__restrict__ x, double *__restrict__ sim, NmState *__restrict__ st,
           int32_t *__restrict__ cnt)
{
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= nprob) return;
    const size_t npts = (size_t)n + 1;
    if (o.build) {
        double *s = sim + (size_t)p * npts * n;
        const double *xp = x + (size_t)p * n;
        for (int i = lane; i < n; i += 64) {
            const double xi = xp[i];
            s[i] = xi;                                               // :206
            for (size_t v = 1; v < npts; ++v) s[v * n + i] = xi;     // :207-209
            s[(size_t)(i + 1) * n + i] = xi + o.init_size;           // :210-212
        }
    }
    if (lane == 0) {
        NmState z;
        z.fsave = z.fval = z.rtol = z.pr_fval = z.pr_rtol = 0.0;
        z.phase = NM_INIT;
        z.ilo = z.ihi = z.ihi2 = 0;
        z.iter = z.neval = z.flag = z.fcnvrg = 0;
        z.print_due = z.pr_iter = z.pr_neval = z.pad = 0;
        st[p] = z;
        cnt[p] = n + 1;
    }
}

// Vertices whose f a wave keeps in LDS while lane 0 ranks them (8 KiB per 4-wave block); beyond, f stays in global memory
// (no bound on n).
#define NM_F_LDS 256

// LDS written by some lanes of a wave, then read by others: order the wave's accesses.
static __device__ inline void nm_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// What the lanes do after lane 0 has decided: the accepted trial replaces the high vertex (:390-397), pcent is summed
// afresh (after the first evaluations, :222-224, and after a shrink, :300-302), then the next action.
enum NmAction : int32_t { NA_NONE = 0, NA_TRIAL = 1, NA_SHRINK = 2, NA_CONVERGED = 3 };

// One advance: consume the values the last round evaluated (fs at off[p]: the scan of that round), run nm_solve's
// statements up to the next function evaluation, record how many points come next.
static __global__ void __launch_bounds__(256)
k_nm_advance(int nprob, int n, NmOpts o, const double *__restrict__ fs, const int32_t *__restrict__ off, double *__restrict__ sim,
             double *__restrict__ f, double *__restrict__ pcent, double *__restrict__ work, double *__restrict__ x,
             NmState *__restrict__ st, int32_t *__restrict__ cnt)
{
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= nprob) return;
    const int32_t phase = st[p].phase;
    if (phase == NM_DONE) {
        if (lane == 0) { cnt[p] = 0; st[p].print_due = 0; }
        return;
    }
    const int npts = n + 1;
    double *s = sim + (size_t)p * npts * n;
    double *fg = f + (size_t)p * npts;
    double *pc = pcent + (size_t)p * n;
    double *w = work + (size_t)p * n;
    // lane 0's scalar logic is a chain of dependent loads of f: up to NM_F_LDS vertices it runs on a copy in LDS
    __shared__ double fsh[4][NM_F_LDS];
    const bool in_lds = npts <= NM_F_LDS;
    double *fp = in_lds ? fsh[threadIdx.x >> 6] : fg;
    if (in_lds) {
        for (int i = lane; i < npts; i += 64) fp[i] = fg[i];
        nm_wave_sync();
    }
    int32_t acc = -1, resum = 0, action = NA_NONE, aidx = 0, facc = 0;
    if (lane == 0) {
        NmState c = st[p];
        const double *v = fs + off[p];
        bool end_iter = false;
        c.print_due = 0;
        switch (phase) {
        case NM_INIT:
            for (int i = 0; i < npts; ++i) fp[i] = v[i];             // :216-218
            c.neval = npts;                                          // :219
            c.fval = fp[0];                                          // :220
            resum = 1;                                               // :222-224
            break;
        case NM_REFLECT:
        case NM_EXPAND:
        case NM_CONTRACT: {
            const double ytry = v[0];                                // nm_extrapolate :388-389
            c.neval = c.neval + 1;
            if (ytry < fp[c.ihi]) { fp[c.ihi] = ytry; acc = c.ihi; } // :390-397
            if (phase == NM_REFLECT) {
                if (ytry <= fp[c.ilo]) { action = NA_TRIAL; facc = NM_EXPAND; }        // :277-282
                else if (ytry >= fp[c.ihi2]) { c.fsave = fp[c.ihi]; action = NA_TRIAL; facc = NM_CONTRACT; }   // :283-287
                else end_iter = true;
                aidx = c.ihi;
            } else if (phase == NM_CONTRACT && ytry >= c.fsave) {
                action = NA_SHRINK; aidx = c.ilo;                    // :288-297
            } else end_iter = true;
            break;
        }
        case NM_SHRINK: {
            int k = 0;
            for (int i = 0; i < npts; ++i)
                if (i != c.ilo) fp[i] = v[k++];                      // :296
            c.neval = c.neval + npts;                                // :299: npts, not npts - 1
            resum = 1;                                               // :300-302
            end_iter = true;
            break;
        }
        default: break;
        }
        if (end_iter) {
            c.print_due = 1;                                         // :306-313 (the stale fval)
            c.pr_iter = c.iter; c.pr_neval = c.neval; c.pr_fval = c.fval; c.pr_rtol = c.rtol;
        }
        bool top = phase == NM_INIT;
        if (end_iter) {
            if (c.neval >= o.max_evals) { c.flag = 1; c.phase = NM_DONE; action = NA_NONE; }   // :316-319
            else top = true;
        }
        if (top) {
            c.iter = c.iter + 1;                                     // :230
            int ilo = 0, ihi, ihi2;                                  // :233-249, 0-based
            if (fp[0] > fp[1]) { ihi = 0; ihi2 = 1; } else { ihi = 1; ihi2 = 0; }
            for (int i = 0; i < npts; ++i) {
                if (fp[i] <= fp[ilo]) ilo = i;
                if (fp[i] > fp[ihi]) { ihi2 = ihi; ihi = i; }
                else if (fp[i] > fp[ihi2]) { if (i != ihi) ihi2 = i; }
            }
            c.ilo = ilo; c.ihi = ihi; c.ihi2 = ihi2;
            c.rtol = fabs(fp[ihi] - fp[ilo]);                        // :256
            if (c.rtol < o.ftol) {                                   // :257-269
                const double swp = fp[0]; fp[0] = fp[ilo]; fp[ilo] = swp;
                c.fval = fp[0];
                c.fcnvrg = 1;
                c.phase = NM_DONE;
                action = NA_CONVERGED; aidx = ilo;
            } else {
                action = NA_TRIAL; facc = NM_REFLECT; aidx = ihi;    // :273-274
            }
        }
        if (action == NA_TRIAL) c.phase = facc;
        else if (action == NA_SHRINK) c.phase = NM_SHRINK;
        cnt[p] = action == NA_TRIAL ? 1 : (action == NA_SHRINK ? n : 0);
        st[p] = c;
    }
    if (in_lds) {
        nm_wave_sync();
        for (int i = lane; i < npts; i += 64) fg[i] = fp[i];
    }
    acc = __shfl(acc, 0, 64);
    resum = __shfl(resum, 0, 64);
    action = __shfl(action, 0, 64);
    aidx = __shfl(aidx, 0, 64);
    facc = __shfl(facc, 0, 64);
    for (int i = lane; i < n; i += 64) {
        if (acc >= 0) {                                              // :392-397
            const double wi = w[i];
            pc[i] = (pc[i] + wi) - s[(size_t)acc * n + i];
            s[(size_t)acc * n + i] = wi;
        }
        if (action == NA_SHRINK) {                                   // :291-297 (the midpoint before its evaluation)
            const double lo = s[(size_t)aidx * n + i];
            for (int v = 0; v < npts; ++v)
                if (v != aidx) s[(size_t)v * n + i] = 0.5 * (s[(size_t)v * n + i] + lo);
        }
        if (resum) {                                                 // pcent(i) = sum(simplex(i,:)), ascending
            double t = 0.0;
            for (int v = 0; v < npts; ++v) t = t + s[(size_t)v * n + i];
            pc[i] = t;
        }
        if (action == NA_TRIAL) {                                    // nm_extrapolate :382-386
            const double fac = facc == NM_REFLECT ? -1.0 : (facc == NM_EXPAND ? 2.0 : 0.5);
            const double fac1 = (1.0 - fac) / (double)n, fac2 = fac1 - fac;
            w[i] = pc[i] * fac1 - s[(size_t)aidx * n + i] * fac2;
        } else if (action == NA_CONVERGED) {                         // :258-265
            const double a = s[i];
            s[i] = s[(size_t)aidx * n + i];
            s[(size_t)aidx * n + i] = a;
            x[(size_t)p * n + i] = s[i];
        }
    }
}

#include "nlh_kernels_scan.h"   // nm_block_excl_scan, k_nm_scan_blocks, k_nm_scan_top

// The points of the round into the compact staging list: problem p's cnt[p] points from off[p] on, each with its
// problem index (pbase + p: the index in the caller's batch) -- every vertex (NM_INIT), the trial point, or the
// vertices i /= ilo in ascending order (NM_SHRINK).
static __global__ void __launch_bounds__(256)
k_nm_emit(int nprob, int n, int32_t pbase, const double *__restrict__ sim, const double *__restrict__ work,
          const NmState *__restrict__ st, const int32_t *__restrict__ cnt, int32_t *__restrict__ off,
          const int32_t *__restrict__ bpre, double *__restrict__ xs, int32_t *__restrict__ dprob)
{
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= nprob) return;
    const int32_t c = cnt[p];
    const int32_t o32 = off[p] + bpre[p >> 10];
    if (lane == 0) off[p] = o32;                                     // (what the next advance reads its values at)
    if (c == 0) return;
    const int32_t phase = st[p].phase, ilo = st[p].ilo;
    const size_t o = (size_t)o32;
    for (int32_t k = lane; k < c; k += 64) dprob[o + k] = pbase + p;
    const size_t npts = (size_t)n + 1;
    if (phase == NM_INIT || phase == NM_SHRINK) {
        const double *s = sim + (size_t)p * npts * n;
        const size_t tot = (size_t)c * n;
        for (size_t e = lane; e < tot; e += 64) {
            const size_t k = e / n, i = e - k * n;
            const size_t v = (phase == NM_SHRINK && k >= (size_t)ilo) ? k + 1 : k;
            xs[(o + k) * n + i] = s[v * n + i];
        }
    } else {
        const double *w = work + (size_t)p * n;
        for (int i = lane; i < n; i += 64) xs[o * n + i] = w[i];
    }
}
