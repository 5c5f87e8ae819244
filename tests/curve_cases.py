"""Seeded problem generator and the case list of the curve-model tests (tests/test_curve_cpu.py, tests/test_gpu_curve.py,
profiles/scripts/curve_rate.py), modelled on user_models.lorentz_problems.  Test infrastructure, not part of the product."""
import numpy as np

import curve_restatement as R

# (kind, K, B, m): 64 problems each, seed 2025.  On the CPU reference path every one of them returns 0 with forward
# differences and with the analytic Jacobian, in 3 - 8 Jacobian evaluations -- except gauss (6, 0, 1000), whose tail needs
# some hundreds: a heterogeneous batch, never asserted close to x_true.
CASES = [("gauss", 1, -1, 64), ("gauss", 3, 1, 400), ("gauss", 6, 0, 1000),
         ("lorentz", 4, -1, 512), ("lorentz", 2, 2, 301),
         ("expdecay", 1, 0, 200), ("expdecay", 2, 0, 400), ("expdecay", 3, -1, 1000)]
NPROB, SEED, MAX_EVALS = 64, 2025, 500
LONG_TAILED = ("gauss", 6, 0, 1000)


def curve_problems(kind, K, B, m, nprob=NPROB, seed=SEED, sigma=1e-3, spread=0.05):
    """nprob data sets of a model on m abscissae in [0, 1] (jittered per problem): t, y [nprob, m], x_true, x0 [nprob, n]."""
    kd = R.KINDS[kind]
    rng = np.random.default_rng(seed)
    P, n = R.nper(kd), R.nparams(kd, K, B)
    t = np.tile(np.linspace(0.0, 1.0, m), (nprob, 1)) + rng.uniform(-0.2, 0.2, (nprob, m)) / m
    xt = np.empty((nprob, n))
    xt[:, 0:P * K:P] = rng.uniform(0.5, 1.5, (nprob, K))
    if kd == R.EXPDECAY:
        xt[:, 1:P * K:P] = 1.5 * 3.0 ** np.arange(K) * rng.uniform(0.8, 1.2, (nprob, K))
    else:
        xt[:, 1:P * K:P] = (np.arange(K) + 0.5) / K + rng.uniform(-0.15, 0.15, (nprob, K)) / K
        width = rng.uniform(0.15, 0.35, (nprob, K)) / K
        xt[:, 2:P * K:P] = width if kd == R.LORENTZ else 0.5 * width
    if B >= 0:
        xt[:, P * K:] = rng.uniform(-0.2, 0.2, (nprob, B + 1))
    y = np.empty((nprob, m))
    for p in range(nprob):
        y[p] = R.model(kd, K, B, xt[p], t[p]) + sigma * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + spread * rng.uniform(-1, 1, (nprob, n)))
    return np.ascontiguousarray(t), np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


def sample(jacobian_counts, at_least=32):
    """Indices of a sample of a batch: a problem of every distinct jacobian_count (the first of each), then the lowest
    indices not yet taken, up to at_least problems (the whole batch when it is smaller)."""
    jc = list(jacobian_counts)
    seen, pick = set(), []
    for p, c in enumerate(jc):
        if c not in seen:
            seen.add(c)
            pick.append(p)
    for p in range(len(jc)):
        if len(pick) >= min(at_least, len(jc)):
            break
        if p not in pick:
            pick.append(p)
    return sorted(pick)
