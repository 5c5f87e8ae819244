"""The cases of the global-fit tests (tests/test_group_cpu.py, tests/test_gpu_group.py, profiles/scripts/group_rate.py):
groups of Lorentzian spectra whose truth obeys the sharing, and the decay study of the issue that motivates the feature.
Test infrastructure, not part of the product."""
import numpy as np

import curve_cases as CC
import curve_restatement as R

# (kind, K, B, m, G, shared): two Lorentzians on a constant with the peak positions common to the group -- the non-leading
# (1, 4) of N = 7 --, and one Lorentzian on a line with a common width
CASES = [("lorentz", 2, 0, 200, 3, (1, 4)), ("lorentz", 1, 1, 64, 5, (2,))]
NGROUP, SEED, MAX_EVALS = 6, 2026, CC.MAX_EVALS


def problems(kind, K, B, m, G, shared, ngroup=NGROUP, seed=SEED, sigma=1e-3):
    """curve_cases.curve_problems for ngroup * G data sets with the true shared parameters of every group those of its data
    set 0, y = model + sigma U(-1, 1) and x0 = x_true (1 + 0.05 U(-1, 1)) regenerated from a seeded generator: t, y [ngroup G,
    m], x_true, x0 [ngroup G, N].  x0 is per data set: a global fit starts a shared parameter from data set 0's value."""
    kd = R.KINDS[kind]
    nprob = ngroup * G
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob, seed=seed)
    sh = list(shared)
    for p in range(nprob):
        xt[p, sh] = xt[p - p % G, sh]
    rng = np.random.default_rng(seed + 1)
    for p in range(nprob):
        y[p] = R.model(kd, K, B, xt[p], t[p]) + sigma * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + 0.05 * rng.uniform(-1, 1, xt.shape))
    return t, np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


# the study: 150 groups of G = 8 decays a exp(-k t) + c on 64 points in [0, 4], k = 1 shared, a ~ U(40, 60), c = 0.5, noise 1
STUDY = dict(ngroup=150, G=8, m=64, seed=7)


def study_data(ngroup, G, m, seed):
    """t [m], y [ngroup G, m], x_true [ngroup G, 3] = (a, k, c)."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 4.0, m)
    xt = np.empty((ngroup * G, 3))
    xt[:, 0] = rng.uniform(40.0, 60.0, ngroup * G)
    xt[:, 1] = 1.0
    xt[:, 2] = 0.5
    y = xt[:, :1] * np.exp(-(xt[:, 1:2] * t)) + xt[:, 2:3] + rng.standard_normal((ngroup * G, m))
    return t, y, xt
