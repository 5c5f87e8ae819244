// nlh_kernels_band.h -- the delta method (include/nonlin_hip.h: nlh_propagate): the standard deviation of every row of a
// vector function of fitted parameters, sd_i = sqrt(J_i C J_i^T), from the function's Jacobian J at the solution and the
// parameter covariance C.  The kernel behind nlh_propagate, nlh_propagate_batch_device, nlh_curve_band_batch,
// nlh_expr_band_batch and nlh_dq_model_propagate.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off).  Row i of point p, J_k = J[p][k][i]:
//   v = 0
//   for j = 0 .. n-1:   s = 0;  s = s + C[j][k]*J_k for k = 0 .. j-1;  s = 2.0*s;  s = s + C[j][j]*J_j;  v = v + J_j*s
//   v = v + noise[p] when noise is given;  v < 0.0: v = 0.0 (a NaN passes);  sd = sqrt(v)
// Only C[j][k] with k <= j is read.  No sum crosses a thread -- one thread owns one (point, row) -- so a row's bits do not
// depend on the form, the launch shape or the slice it is computed in.
//
// Shape: k_loss_jac's.  A thread per (point, row), J column-major (a wave's load is 64 consecutive doubles), two workgroup
// forms -- row: a workgroup per (point, 256 rows); flat: ppw points per workgroup, short m.  The packed lower triangle of a
// point's C, n (n + 1) / 2 doubles, is staged in LDS (row j at j (j + 1) / 2): in the row form every lane reads the same
// address, a broadcast; beyond the LDS cap (n > 200) the row form reads C[j][k] from global memory, again one address per
// workgroup.
//
// A thread needs its J_k n (n + 1) / 2 times.  The columns go in blocks of BAND_JB = 16: the block's own J_j and its sixteen
// running sums s_j live in registers (compile-time indices, the loops over the block fully unrolled); for the columns k in
// front of the block J_k is loaded ONCE per block and feeds the sixteen sums, each still the plain sum over k ascending.
// So up to 16 parameters -- where fits live -- J is read exactly once, 8 m n bytes per point, and beyond that a thread loads
// n + 16 (B - 1) B / 2 doubles for B = ceil(n / 16) blocks instead of n (n + 1) / 2, the re-reads from L1 / L2.  The last
// block of an n that is no multiple of 16 runs its surplus sums on the clamped row n - 1 and drops them.
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"
#include <type_traits>

#define BAND_JB 16

static __device__ __forceinline__ size_t band_tri(int j) { return (size_t)j * ((size_t)j + 1) / 2; }

// FLAT: nlh_kernels_place.h.  CLDS: the triangle in LDS (tri = n (n + 1) / 2 doubles per point of the workgroup); otherwise
// from cov itself (row form only).
template <bool FLAT, bool CLDS>
static __global__ void __launch_bounds__(256)
k_band(int m, int n, int nblk, int ppw, int npoints, const double *__restrict__ J, const double *__restrict__ cov,
       const double *__restrict__ noise, double *__restrict__ sd)
{
    extern __shared__ double tri_s[];
    int q, i;
    place_row<FLAT>(m, nblk, ppw, npoints, q, i);
    const size_t tri = band_tri(n), nn = (size_t)n * n;
    const double *C;                                             // this thread's matrix (where its row j starts: crow)
    if (CLDS) {
        const int q0 = FLAT ? blockIdx.x * ppw : q;              // (row form: q is the workgroup's one point, < npoints)
        const int nq = FLAT ? min(ppw, npoints - q0) : 1;
        for (size_t e = threadIdx.x; e < (size_t)nq * nn; e += 256) {
            const int lp = (int)(e / nn);
            const int r = (int)(e - (size_t)lp * nn);
            const int j = r / n, k = r - j * n;
            if (k <= j) tri_s[(size_t)lp * tri + band_tri(j) + k] = cov[(size_t)q0 * nn + e];
        }
        __syncthreads();
        C = tri_s + (size_t)(q - q0) * tri;
    } else {
        C = cov + (size_t)min(q, npoints - 1) * nn;
    }
    if (q >= npoints || i >= m) return;
    // where row j of this thread's matrix starts: packed in LDS, the full matrix's row in global memory
    typedef typename std::conditional<CLDS, int, size_t>::type off_t;
    auto crow = [&](int j) { return CLDS ? (off_t)band_tri(j) : (off_t)((size_t)j * n); };
    const size_t ms = (size_t)m;
    const double *Jq = J + (size_t)q * ms * n + i;
    double v = 0.0;
    for (int j0 = 0; j0 < n; j0 += BAND_JB) {
        const int nb = min(BAND_JB, n - j0);
        double Jb[BAND_JB], s[BAND_JB];
        off_t Cr[BAND_JB];
#pragma unroll
        for (int t = 0; t < BAND_JB; ++t) {
            const int jc = min(j0 + t, n - 1);
            Jb[t] = Jq[(size_t)jc * ms];
            Cr[t] = crow(jc);
            s[t] = 0.0;
        }
        for (int k = 0; k < j0; ++k) {                           // the columns in front of the block: one load of J_k, sixteen sums
            const double Jk = Jq[(size_t)k * ms];
#pragma unroll
            for (int t = 0; t < BAND_JB; ++t) s[t] = s[t] + C[Cr[t] + k] * Jk;
        }
#pragma unroll
        for (int t = 0; t < BAND_JB; ++t) {
            if (t < nb) {
#pragma unroll
                for (int u = 0; u < t; ++u) s[t] = s[t] + C[Cr[t] + j0 + u] * Jb[u];
                s[t] = 2.0 * s[t];
                s[t] = s[t] + C[Cr[t] + j0 + t] * Jb[t];
                v = v + Jb[t] * s[t];
            }
        }
    }
    if (noise) v = v + noise[q];
    if (v < 0.0) v = 0.0;
    sd[(size_t)q * ms + i] = sqrt(v);
}
