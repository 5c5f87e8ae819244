"""Writes tests/golden/specfun2_reference.npz: reference values of j0, j1, i0e, i1e, lgamma, digamma, expm1 and log1p,
computed with mpmath at 40 digits and rounded to the nearest double.  The tests read the file only; mpmath (1.3.0 made it)
is needed to regenerate it.

  j_a [2680]; j0, j1          [-200, 200] uniform, 0 included, and the first 20 zeros of each function, both signs: the double
                              nearest the zero and points 1e-9, 1e-6, 1e-3 to either side
  ie_a [9218]; i0e, i1e       +-[1e-8, 1e6] log-uniform, both sides of the switch at 8 (8 itself, its neighbours, 8 -+ 1e-6), 0;
                              then [-8, 8] uniform, 6000 points of a generator of their own (the series' rounding error is
                              largest at the ends of their ranges, which a log-uniform sample hardly visits), and both
                              sides of i1e's switch at 1
  lg_a [3008]; lgamma, digamma  [1e-3, 1e6] log-uniform, [0.5, 12] uniform, and 1, 2, 10 (digamma's switch), the digamma root
                              1.4616321449683623 and its neighbours
  em_a [3002]; expm1          +-[1e-18, 30] log-uniform, +-1e-18
  lp_a [3002]; log1p          [1e-18, 30] and -[1e-18, 1) log-uniform, +-1e-18
Run: python tests/golden/make_specfun2_reference.py"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 40


def f64(v):
    return float(v)


def ie(nu, a):
    x = mp.mpf(float(a))
    return mp.exp(-abs(x)) * mp.besseli(nu, x)


def main():
    rng = np.random.default_rng(20261020)
    out = {}

    zeros = []
    for nu in (0, 1):
        for k in range(1, 21):
            z = float(mp.besseljzero(nu, k))
            for s in (1.0, -1.0):
                zeros += [s * z] + [s * (z + d) for d in (1e-9, -1e-9, 1e-6, -1e-6, 1e-3, -1e-3)]
    a = np.concatenate([rng.uniform(-200.0, 200.0, 2119), [0.0], zeros])
    out["j_a"] = a
    out["j0"] = np.array([f64(mp.besselj(0, mp.mpf(float(v)))) for v in a])
    out["j1"] = np.array([f64(mp.besselj(1, mp.mpf(float(v)))) for v in a])

    lo8, hi8 = np.nextafter(8.0, 0.0), np.nextafter(8.0, 9.0)
    a = np.concatenate([rng.choice([-1.0, 1.0], 3200) * 10.0 ** rng.uniform(-8, 6, 3200),
                        [0.0, 8.0, -8.0, lo8, -lo8, hi8, -hi8, 8.0 - 1e-6, 8.0 + 1e-6, 1e-8, 1e6, -1e6],
                        np.random.default_rng(20261021).uniform(-8.0, 8.0, 6000),
                        [1.0, -1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 1.0 - 1e-6, 1.0 + 1e-6]])
    out["ie_a"] = a
    out["i0e"] = np.array([f64(ie(0, v)) for v in a])
    out["i1e"] = np.array([f64(ie(1, v)) for v in a])

    root = float(mp.findroot(mp.digamma, 1.46))
    a = np.concatenate([10.0 ** rng.uniform(-3, 6, 1800), rng.uniform(0.5, 12.0, 1200),
                        [1.0, 2.0, 10.0, root, np.nextafter(root, 0.0), np.nextafter(root, 2.0), 1e-3, 1e6]])
    out["lg_a"] = a
    out["lgamma"] = np.array([f64(mp.loggamma(mp.mpf(float(v)))) for v in a])
    out["digamma"] = np.array([f64(mp.digamma(mp.mpf(float(v)))) for v in a])

    a = np.concatenate([rng.choice([-1.0, 1.0], 3000) * 10.0 ** rng.uniform(-18, np.log10(30.0), 3000), [1e-18, -1e-18]])
    out["em_a"] = a
    out["expm1"] = np.array([f64(mp.expm1(mp.mpf(float(v)))) for v in a])

    a = np.concatenate([10.0 ** rng.uniform(-18, np.log10(30.0), 1500), -(10.0 ** rng.uniform(-18, 0, 1500)), [1e-18, -1e-18]])
    a = a[a > -1.0]
    out["lp_a"] = a
    out["log1p"] = np.array([f64(mp.log1p(mp.mpf(float(v)))) for v in a])

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "specfun2_reference.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
