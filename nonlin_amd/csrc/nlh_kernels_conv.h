// nlh_kernels_conv.h -- instrument-response fits (include/nonlin_hip.h: nlh_conv_*): the kernels behind the wrapping launchers
// nlh_conv_device_fcn / nlh_conv_device_jac and nlh_conv_apply_batch.
//
// THE ARITHMETIC IS PART OF THE INTERFACE (one IEEE operation per step, -ffp-contract=off).  v [0 .. m-1] one column -- the
// model values mu_s = r_s + y_s of a residual call, a column of the inner Jacobian, a column handed to apply --, kp the
// L taps of the point's problem, o = origin:
//   acc = +0.0;  for j = 0 .. L-1 ascending:  s = i + o - j
//       ZERO: s outside 0 .. m-1: the tap is skipped          HOLD: s = min(max(s, 0), m-1)
//       t = kp[j] * v[s];  acc = acc + t
//   residual: out_i = acc - y_i, with weights w_i * out_i;  Jacobian: acc, with weights w_i * acc;  a row with w_i == 0.0 is
//   STORED as +0.0.  apply: acc.
// One thread owns the whole chain of an output, so its bits depend on nothing but the column and the taps.
//
// k_conv_row, the one that does the arithmetic: a workgroup per (point, tile of T rows, group of columns).  T is a multiple of
// 4, at most CONV_T = 1024; a thread computes 4 consecutive rows of one column from a sliding register window, so a tap step
// costs one LDS read of the column (and one broadcast read of the tap) for 4 multiplies and 4 adds.  With T / 4 < 256 threads
// per column a pass of the workgroup takes 256 / (T / 4) columns at once (as many as the LDS holds).  Staged in LDS per pass:
// the taps, and per column the tile plus its halo of L - 1 rows -- clamped (HOLD) or zero (ZERO) outside 0 .. m-1 -- in FOUR
// PLANES: staged element u' lies in plane u' & 3 at slot u' >> 2.  The element a thread needs next moves down by one per tap,
// so through the planes 2, 1, 0, 3 and one slot down every four taps; the column is shifted by sh = ((4 - L) & 3) + 4 elements
// so that this cycle starts in the same plane for every L, and the loop over the taps, unrolled by four, reads through four
// pointers that step once per four taps -- no index arithmetic per tap.  The lanes of a wave read consecutive slots of one
// plane, 32 lanes 64 banks: no conflict, whatever the plane stride; the stride is 4 mod 16 slots so that the 16 lanes of a
// staging store, which cycle through the planes, meet no bank twice either.
// ZERO and the skipped tap: acc starts at +0.0 and a sum of doubles rounds to -0.0 only from two -0.0, so acc is never
// -0.0, and adding the +-0.0 that a finite tap times a staged zero gives changes no bit of it: with finite taps the halo's
// zeros ARE the skip.  A tap that is not finite would turn them into NaN, so a workgroup that staged one takes the checked
// loop, which selects per output.  (HOLD stages the clamped rows themselves and never needs it.)
//
// k_conv_flat, short m: 256 / m points per workgroup, a thread per (point, row), the column of every point staged whole (no
// halo: the row index is clamped or tested per tap), the taps read through the cache.
#pragma once
#include "nlh_internal.h"
#include "nlh_kernels_place.h"

#define CONV_T 1024                                            // the largest row tile
// slots of a plane for W staged elements: a quarter of them, rounded up to 4 mod 16
static __host__ __device__ inline int conv_plane(int W) { const int s = (W + 3) >> 2; return s + ((4 - s) & 15); }
// LDS doubles of one column of a tile of T rows (whole quads) with L taps: the tile, its halo and the shift of at most 7
static __host__ __device__ inline int conv_col_lds(int T, int L) { return 4 * conv_plane(T + L - 1 + 7); }
// ... of the columns of a pass: one column at the largest tile and the most taps (smaller ones: as many as fit)
#define CONV_COLS_LDS (4 * 516)

struct ConvArgs {
    const double *k;                   // [L] or [nprob][L]
    const double *y;                   // [nprob][m], residual calls only
    const double *w;                   // [nprob][m] or null
    const int32_t *dprob;              // point q is problem dprob[q]; null: q
    int32_t L, origin, ext, shared_k;
};

// what a call is: the residual (mu = r + y staged, out = acc - y), a Jacobian (columns as they are), both with weights
#define CONV_FCN 0
#define CONV_JAC 1

static __device__ __forceinline__ double conv_finish(int mode, double acc, const double *y, const double *w, size_t at)
{
    double o = acc;
    if (mode == CONV_FCN) o = acc - y[at];
    if (w) {
        const double wi = w[at];
        o = wi == 0.0 ? 0.0 : wi * o;
    }
    return o;
}

// One thread's four chains.  col: the column's plane 0; PS: slots of a plane; slot: quad + A, where 4 A + 3 = L - 1 + sh is
// the staged offset of row 0's element at tap 0 (plane 3); sb: the row s that element stands for.
template <bool CHECK>
static __device__ __forceinline__ void conv_chain(const double *ks, const double *col, int PS, int slot, int L, int m, int sb, double (&acc)[4])
{
    const double *p0 = col + slot, *p1 = p0 + PS, *p2 = p1 + PS, *p3 = p2 + PS;
    double w0 = p3[0], w1 = p0[1], w2 = p1[1], w3 = p2[1];       // rows 0 .. 3 at tap 0
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
    // a tap: the four products and sums; then the window moves down by one element, NEXT being row 0's at the next tap
#define CONV_TAP(KJ, J, NEXT)                                                                   \
    {                                                                                           \
        const double kj = (KJ);                                                                 \
        const double t0 = kj * w0, t1 = kj * w1, t2 = kj * w2, t3 = kj * w3;                    \
        if (CHECK) {                                                                            \
            const int s = sb - (J);                                                             \
            acc[0] = (unsigned)s < (unsigned)m ? acc[0] + t0 : acc[0];                          \
            acc[1] = (unsigned)(s + 1) < (unsigned)m ? acc[1] + t1 : acc[1];                    \
            acc[2] = (unsigned)(s + 2) < (unsigned)m ? acc[2] + t2 : acc[2];                    \
            acc[3] = (unsigned)(s + 3) < (unsigned)m ? acc[3] + t3 : acc[3];                    \
        } else {                                                                                \
            acc[0] = acc[0] + t0; acc[1] = acc[1] + t1; acc[2] = acc[2] + t2; acc[3] = acc[3] + t3; \
        }                                                                                       \
        w3 = w2; w2 = w1; w1 = w0; w0 = (NEXT);                                                 \
    }
    int j = 0;
#pragma unroll 2
    for (; j + 4 <= L; j += 4) {
        const double4 k4 = *(const double4 *)(ks + j);                // (16-byte aligned: two ds_read_b128 for four taps)
        const double k0 = k4.x, k1 = k4.y, k2 = k4.z, k3 = k4.w;
        CONV_TAP(k0, j, p2[0])
        CONV_TAP(k1, j + 1, p1[0])
        CONV_TAP(k2, j + 2, p0[0])
        CONV_TAP(k3, j + 3, p3[-1])
        --p0; --p1; --p2; --p3;
    }
    // (the element read after the last tap is not used; the shift of at least 4 keeps it inside the column)
    if (j < L) { CONV_TAP(ks[j], j, p2[0]) ++j; }
    if (j < L) { CONV_TAP(ks[j], j, p1[0]) ++j; }
    if (j < L) { CONV_TAP(ks[j], j, p0[0]) }
#undef CONV_TAP
}

// V, O [npoints][ncol][m]; grid.x = npoints * ntile, grid.y groups of cpg columns; T rows per tile, cpp columns per pass.
// Dynamic LDS: the taps (L doubles, rounded up to an even count), then cpp columns of conv_col_lds(T, L) doubles at most.
static __global__ void __launch_bounds__(256)
k_conv_row(ConvArgs A, int mode, int m, int ncol, int T, int ntile, int cpp, int cpg, int npoints, const double *__restrict__ V,
           double *__restrict__ O)
{
    extern __shared__ __attribute__((aligned(16))) double conv_lds[];
    const int q = blockIdx.x / ntile;
    const int i0 = (blockIdx.x - q * ntile) * T;
    const int j0 = blockIdx.y * cpg, j1 = min(j0 + cpg, ncol);
    if (q >= npoints || j0 >= j1) return;                        // (uniform)
    const int L = A.L;
    double *ks = conv_lds, *cols = conv_lds + ((L + 1) & ~1);
    const size_t p = (size_t)(A.dprob ? A.dprob[q] : q), ms = (size_t)m;
    const double *kp = A.shared_k ? A.k : A.k + p * L;
    const int rows = min(T, m - i0);                             // of this tile
    const int W = ((rows + 3) & ~3) + L - 1;                     // staged rows of a column: whole quads and the halo
    const int sh = ((4 - L) & 3) + 4;                            // ... which lie from staged element sh on
    const int PS = conv_plane(W + sh), cs = 4 * PS;              // slots of a plane; doubles of a column
    const int s0 = i0 + A.origin - (L - 1);                      // the row that staged element sh stands for
    const bool zero = A.ext == NLH_CONV_ZERO;
    int bad = 0;
    for (int j = threadIdx.x; j < L; j += 256) {
        const double kj = kp[j];
        ks[j] = kj;
        bad |= !(fabs(kj) <= DBL_MAX);
    }
    const int anybad = __syncthreads_or(bad);
    const int TQ = T >> 2;                                       // threads of a column
    const int c = threadIdx.x / TQ, quad = threadIdx.x - c * TQ;
    const double *yq = A.y ? A.y + p * ms : nullptr, *wq = A.w ? A.w + p * ms : nullptr;
    for (int jc = j0; jc < j1; jc += cpp) {
        const int nc = min(cpp, j1 - jc);
        if (jc > j0) __syncthreads();                            // (the last pass's reads)
        for (int e = threadIdx.x; e < nc * W; e += 256) {
            const int cc = e / W, u = e - cc * W;
            int s = s0 + u;
            const bool in = (unsigned)s < (unsigned)m;
            s = min(max(s, 0), m - 1);
            double v = V[((size_t)q * ncol + jc + cc) * ms + s];
            if (mode == CONV_FCN) v = v + yq[s];
            const int us = u + sh;
            cols[cc * cs + (us & 3) * PS + (us >> 2)] = (zero && !in) ? 0.0 : v;
        }
        __syncthreads();
        const int i = i0 + 4 * quad;
        if (c < nc && 4 * quad < rows) {
            double acc[4];
            // the outside of a ZERO tile: zeros in LDS, which finite taps leave without trace
            const bool edge = zero && (s0 < 0 || i0 + rows - 1 + A.origin > m - 1);
            const int slot = quad + ((L - 1 + sh) >> 2);
            if (edge && anybad) conv_chain<true>(ks, cols + c * cs, PS, slot, L, m, i + A.origin, acc);
            else conv_chain<false>(ks, cols + c * cs, PS, slot, L, m, i + A.origin, acc);
            double *Oq = O + ((size_t)q * ncol + jc + c) * ms;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (i + r < m) Oq[i + r] = conv_finish(mode, acc[r], yq, wq, (size_t)(i + r));
        }
    }
}

// grid.x workgroups of ppw points, grid.y groups of cpg columns; m <= 256
static __global__ void __launch_bounds__(256)
k_conv_flat(ConvArgs A, int mode, int m, int ncol, int ppw, int cpg, int npoints, const double *__restrict__ V, double *__restrict__ O)
{
    __shared__ double cols[256];
    const int lp = threadIdx.x / m, i = threadIdx.x - lp * m;
    const int q = blockIdx.x * ppw + lp;
    const bool on = lp < ppw && q < npoints;
    const int j0 = blockIdx.y * cpg, j1 = min(j0 + cpg, ncol);
    const int qc = min(q, npoints - 1);
    const size_t p = (size_t)(A.dprob ? A.dprob[qc] : qc), ms = (size_t)m;
    const int L = A.L, o = A.origin;
    const double *kp = A.shared_k ? A.k : A.k + p * L;
    const double *yq = A.y ? A.y + p * ms : nullptr, *wq = A.w ? A.w + p * ms : nullptr;
    const bool zero = A.ext == NLH_CONV_ZERO;
    const double *col = cols + lp * m;
    for (int jc = j0; jc < j1; ++jc) {
        __syncthreads();                                         // (the last column's reads)
        if (on) {
            double v = V[((size_t)q * ncol + jc) * ms + i];
            if (mode == CONV_FCN) v = v + yq[i];
            cols[threadIdx.x] = v;
        }
        __syncthreads();
        if (!on) continue;
        double acc = 0.0;
        if (zero) {
            // s = i + o - j in 0 .. m-1: j from i + o - (m-1) to i + o
            const int ja = max(0, i + o - (m - 1)), jb = min(L - 1, i + o);
            for (int j = ja; j <= jb; ++j) {
                const double t = kp[j] * col[i + o - j];
                acc = acc + t;
            }
        } else {
            for (int j = 0; j < L; ++j) {
                const double t = kp[j] * col[min(max(i + o - j, 0), m - 1)];
                acc = acc + t;
            }
        }
        O[((size_t)q * ncol + jc) * ms + i] = conv_finish(mode, acc, yq, wq, (size_t)i);
    }
}
