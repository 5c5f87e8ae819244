"""Writes tests/golden/specfun_reference.npz: reference values of erf, erfc, erfcx, the Faddeeva function w(z) and the Voigt
profile with its three partials, computed with mpmath at 40 digits and rounded to the nearest double.  The tests read the
file only; mpmath (1.3.0 made it) is needed to regenerate it, scipy (1.15.3), when present, cross-checks w.

  erf_a [3000]; erf, erfc, erfcx [3000]       |a| <= 26, half of the arguments within [-1.5, 1.5], some tiny, 0 included
  w_re, w_im [3000]; w_wr, w_wi               z = x + iy, |x| <= 1e4 (x = 0 included), 1e-8 <= y <= 1e3, both log-uniform
  v_x, v_s, v_g [2400]; v, v_gx, v_gs, v_gg   x in [-30, 30] (x = 0 included), sigma in [0.03, 10], gamma in [1e-6, 10]
  v_peak [2400]                               V(0; sigma, gamma), the scale the errors are measured against
Run: python tests/golden/make_specfun_reference.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 40
SQRTPI = mp.sqrt(mp.pi)


def w_of(z):
    return mp.exp(-z * z) * mp.erfc(-1j * z)


def voigt(x, s, g):
    """V and its partials by x, sigma, gamma from w and w' = -2 z w + 2i/sqrt(pi)."""
    u = s * mp.sqrt(2)
    z = mp.mpc(x, g) / u
    w = w_of(z)
    dw = -2 * z * w + 2j / SQRTPI
    nrm = u * SQRTPI
    v = w.real / nrm
    return v, dw.real / (u * nrm), -(v + (z * dw).real / nrm) / s, -dw.imag / (u * nrm)


def main():
    rng = np.random.default_rng(20261019)
    out = {}
    a = np.concatenate([rng.uniform(-26.0, 26.0, 1300), rng.uniform(-1.5, 1.5, 1500),
                        rng.choice([-1.0, 1.0], 190) * 10.0 ** rng.uniform(-12, -2, 190),
                        [0.0, 26.0, -26.0, 0.5, -0.5, 1.0, -1.0, 5.0, -5.0, 6.0]])
    out["erf_a"] = a
    out["erf"] = np.array([float(mp.erf(mp.mpf(float(v)))) for v in a])
    out["erfc"] = np.array([float(mp.erfc(mp.mpf(float(v)))) for v in a])
    out["erfcx"] = np.array([float(mp.exp(mp.mpf(float(v)) ** 2) * mp.erfc(mp.mpf(float(v)))) for v in a])

    n = 3000
    x = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3, 4, n)
    y = 10.0 ** rng.uniform(-8, 3, n)
    x[:40] = 0.0
    x[40:400] = rng.uniform(-6.0, 6.0, 360)                          # the region where neither asymptote holds
    y[40:400] = 10.0 ** rng.uniform(-3, 1, 360)
    w = [w_of(mp.mpc(float(p), float(q))) for p, q in zip(x, y)]
    out["w_re"], out["w_im"] = x, y
    out["w_wr"], out["w_wi"] = np.array([float(v.real) for v in w]), np.array([float(v.imag) for v in w])
    try:
        from scipy.special import wofz
        ref = wofz(x + 1j * y)
        got = out["w_wr"] + 1j * out["w_wi"]
        assert (np.abs(got - ref) <= 1e-13 * np.abs(ref)).all(), float((np.abs(got - ref) / np.abs(ref)).max())
    except ImportError:
        pass

    n = 2400
    vx = rng.uniform(-30.0, 30.0, n)
    vx[:60] = 0.0
    vs = 10.0 ** rng.uniform(np.log10(0.03), 1.0, n)
    vg = 10.0 ** rng.uniform(-6.0, 1.0, n)
    vals = np.array([[float(r) for r in voigt(mp.mpf(float(p)), mp.mpf(float(q)), mp.mpf(float(r_)))] for p, q, r_ in zip(vx, vs, vg)])
    out["v_x"], out["v_s"], out["v_g"] = vx, vs, vg
    out["v"], out["v_gx"], out["v_gs"], out["v_gg"] = (np.ascontiguousarray(vals[:, k]) for k in range(4))
    out["v_peak"] = np.array([float(voigt(mp.mpf(0), mp.mpf(float(q)), mp.mpf(float(r_)))[0]) for q, r_ in zip(vs, vg)])
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "specfun_reference.npz"), **out)


if __name__ == "__main__":
    main()
