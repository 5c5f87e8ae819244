"""Writes tests/golden/covar_vectors.npz: Lorentzian Jacobians at the true parameters (the curve fitter's case:
tests/user_models.py, analytic derivatives), and for each the inverse of J^T J and cond_2(J)^2 computed with mpmath at
60 digits -- the accuracy yardstick of tests/test_covar_cpu.py, which needs neither mpmath nor scipy to read it.

    python tests/golden/make_covar_vectors.py
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import user_models as um  # noqa: E402

CASES = [(64, 1), (256, 2), (512, 4), (1024, 8)]          # (m, peaks): n = 3, 6, 12, 24


def lorentz_jacobian(x, t):
    m, n = len(t), len(x)
    J = np.empty((m, n))
    for k in range(0, n, 3):
        a, c, w = x[k], x[k + 1], x[k + 2]
        d = (t - c) / w
        q = 1.0 + d * d
        J[:, k] = 1.0 / q
        J[:, k + 1] = a * 2.0 * d / (w * q * q)
        J[:, k + 2] = a * 2.0 * d * d / (w * q * q)
    return J


def main():
    mp.mp.dps = 60
    out = {}
    for m, K in CASES:
        t, _, xt, _ = um.lorentz_problems(1, m, K, seed=100 + K)
        J = lorentz_jacobian(xt[0], t[0])
        n = J.shape[1]
        Jm = mp.matrix(J.tolist())
        G = Jm.T * Jm
        Ginv = G ** -1
        ev = mp.eigsy(G, eigvals_only=True)
        cond2sq = max(ev) / min(ev)
        out[f"J_{n}"] = J
        out[f"ref_{n}"] = np.array([[float(Ginv[i, j]) for j in range(n)] for i in range(n)])
        out[f"cond2sq_{n}"] = np.float64(float(cond2sq))
        print(m, n, float(cond2sq))
    np.savez_compressed(os.path.join(HERE, "covar_vectors.npz"), **out)


if __name__ == "__main__":
    main()
