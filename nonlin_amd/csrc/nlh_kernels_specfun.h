// nlh_kernels_specfun.h -- the special functions of the formula models (include/nonlin_hip.h: nlh_faddeeva*, the
// instructions ERF ERFC ERFCX VOIGT): the Faddeeva function w(z) = exp(-z^2) erfc(-iz), Im z >= 0, and the Voigt profile
// with its three partial derivatives on top of it.
//
// THE ARITHMETIC IS PART OF THE INTERFACE; the table is in include/nonlin_hip.h and the functions below are it, line for
// line: one IEEE operation per step (-ffp-contract=off), no library function, complex products and the quotient spelled in
// real operations in a fixed order.  Host callers (nlh_faddeeva) and the kernels (k_faddeeva, expr_run) run this same text.
//
// w(z) is Weideman's rational approximation (SIAM J. Numer. Anal. 31 (1994) 1497) with N = 40 terms: one formula over the
// whole upper half plane, no branch, no region switch, so that a fitter's objective stays smooth.  L and the coefficients
// are literal constants; the kernels read them with a uniform index, so the loads are scalar.
#pragma once
#include <math.h>

#define NLH_FADDEEVA_N 40
#define NLH_SF_C1      1.1283791670955126      /* 2/sqrt(pi) */
#define NLH_SF_SQRT2   1.4142135623730951
#define NLH_SF_SQRTPI  1.772453850905516
#define NLH_SF_ISQRTPI 0.5641895835477563     /* 1/sqrt(pi) */
#define NLH_FADDEEVA_L 0x1.545ef5c0f51a0p+2    /* sqrt(N/sqrt(2)) = 5.3182958969449885 */

// the coefficients of p, highest power first (Horner's order): the discrete Fourier coefficients of Weideman's recipe with
// M = 2N sample points on each side (a constexpr table: the same object in host code and, in constant memory, in kernels)
static constexpr double NLH_FADDEEVA_A[NLH_FADDEEVA_N] = {
    -0x1.f447ea2000000p-50, 0x1.5a5bf5499999ap-50, 0x1.9f0597ae33333p-47, -0x1.78fc220426666p-48,
    -0x1.3e74182bb9000p-44, 0x1.f069afb7d4000p-47, 0x1.fe7fd42896200p-42, 0x1.0ef74e7fe4c0dp-43,
    -0x1.993999999999ap-39, -0x1.7fe6666666666p-39, 0x1.37a199999999ap-36, 0x1.3177333333333p-35,
    -0x1.8e3fccccccccdp-34, -0x1.87c8266666666p-32, 0x1.cfaf933333333p-33, 0x1.9ec2b5999999ap-29,
    0x1.bea44b0000000p-29, -0x1.3aa8ef499999ap-26, -0x1.10ce7cee9999ap-24, 0x1.e7dc944000000p-27,
    0x1.3d67caa3b999ap-21, 0x1.8e3de3131d666p-20, -0x1.1e27ead3ade66p-20, -0x1.2e1d6585adec8p-16,
    -0x1.d50873c0a9b66p-15, -0x1.4a752dec263c0p-15, 0x1.cd2bcc00e1d5ap-12, 0x1.629a596ed49c6p-9,
    0x1.49424ba5ffea3p-7, 0x1.de75e8cc4682ap-6, 0x1.26308597ddc86p-4, 0x1.3d86fe9e6a9edp-3,
    0x1.33178328c1600p-2, 0x1.0da572e19e018p-1, 0x1.b1c67c927e9f3p-1, 0x1.41a238f009d09p+0,
    0x1.b9b2b4b25d642p+0, 0x1.19cb343b58fc6p+1, 0x1.4edadccb56adbp+1, 0x1.7326e55b41214p+1,
};

// w(zr + i zi) for zi >= 0.  With D = L - iz = dr + i di and Nn = L + iz = nr + i ni:
//   Z = Nn/D;  p = Horner over the coefficients in Z;  1/D = conj(D)/|D|^2;  w = 2 p (1/D)^2 + (1/sqrt(pi)) (1/D)
__host__ __device__ static inline void faddeeva_w(double zr, double zi, double *wr, double *wi)
{
    const double dr = NLH_FADDEEVA_L + zi, di = -zr;
    const double nr = NLH_FADDEEVA_L - zi, ni = zr;
    const double den = dr * dr + di * di;
    const double Zr = (nr * dr + ni * di) / den;
    const double Zi = (ni * dr - nr * di) / den;
    double pr = NLH_FADDEEVA_A[0], pi = 0.0;
#pragma unroll 8
    for (int k = 1; k < NLH_FADDEEVA_N; ++k) {
        const double tr = pr * Zr - pi * Zi;
        const double ti = pr * Zi + pi * Zr;
        pr = tr + NLH_FADDEEVA_A[k];
        pi = ti;
    }
    const double ir = dr / den, ii = -(di / den);
    const double qr = ir * ir - ii * ii;
    const double qi = 2.0 * (ir * ii);
    *wr = 2.0 * (pr * qr - pi * qi) + NLH_SF_ISQRTPI * ir;
    *wi = 2.0 * (pr * qi + pi * qr) + NLH_SF_ISQRTPI * ii;
}

// The Voigt profile V(x; sigma, gamma) = Re w(z)/(|sigma| sqrt(2 pi)), z = (x + i |gamma|)/(|sigma| sqrt(2)), and its
// partials by x, sigma and gamma (the header's VOIGT table).  w' = -2 z w + i C1.  The sigma partial is the sum of two
// terms that cancel in the Lorentzian wings (|x| >> sigma: V + Re(z w')/nrm -> the small Gaussian correction of a
// Lorentzian that does not depend on sigma), so its error relative to itself grows there; relative to V(0)/sigma it stays
// small (DESIGN 4e has the measured figures).
__host__ __device__ static inline double voigt_eval(double x, double sigma, double gamma, double *gx, double *gs, double *gg)
{
    const double s = fabs(sigma), g = fabs(gamma);
    const double u = s * NLH_SF_SQRT2;
    const double zr = x / u, zi = g / u;
    double wr, wi;
    faddeeva_w(zr, zi, &wr, &wi);
    const double nrm = u * NLH_SF_SQRTPI;
    const double v = wr / nrm;
    const double dwr = -(2.0 * (zr * wr - zi * wi));
    const double dwi = NLH_SF_C1 - 2.0 * (zr * wi + zi * wr);
    const double un = u * nrm;
    *gx = dwr / un;
    const double s1 = -((v + (zr * dwr - zi * dwi) / nrm) / s);
    const double g1 = -(dwi / un);
    *gs = sigma < 0.0 ? -s1 : s1;
    *gg = gamma < 0.0 ? -g1 : g1;
    return v;
}

#if defined(__HIPCC__)
// w at count points, a thread per element; Im z < 0 is outside the domain (the values are then not w)
static __global__ void __launch_bounds__(256)
k_faddeeva(long long count, const double *__restrict__ re, const double *__restrict__ im, double *__restrict__ wre, double *__restrict__ wim)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double wr, wi;
    faddeeva_w(re[i], im[i], &wr, &wi);
    wre[i] = wr;
    wim[i] = wi;
}
#endif
