"""The cases of the parameter-map tests (tests/test_pmap_cpu.py, tests/test_gpu_pmap.py, profiles/scripts/pmap_rate.py):
the two Lorentzian cases of curve_cases whose truth is made to obey a tie between the widths, and three maps over them.
Test infrastructure, not part of the product."""
import numpy as np

import curve_cases as CC
import curve_restatement as R
import pmap_restatement as PR

CASES = [("lorentz", 4, -1, 512), ("lorentz", 2, 2, 301)]
MAPS = ("fixed_baseline", "tied_widths", "both")
# the five (case, map) pairs: a case without a baseline has no baseline to fix
PAIRS = [(c, mp) for c in CASES for mp in MAPS if not (mp == "fixed_baseline" and c[2] < 0)]
NPROB, SEED, MAX_EVALS = CC.NPROB, CC.SEED, CC.MAX_EVALS


def width_scale(k):
    """Width of peak k (0-based) over the width of peak 0."""
    return 1.0 + 0.25 * k


def problems(kind, K, B, m, nprob=NPROB, seed=SEED):
    """curve_cases.curve_problems with the true widths of peaks 2 .. K replaced by width_scale(k) * w_1, so that the truth
    obeys the tie, y = model + 1e-3 U(-1, 1) and x0 = x_true (1 + 0.05 U(-1, 1)) regenerated from a seeded generator."""
    kd = R.KINDS[kind]
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob, seed=seed)
    for k in range(1, K):
        xt[:, 3 * k + 2] = width_scale(k) * xt[:, 2]
    rng = np.random.default_rng(seed + 1)
    for p in range(nprob):
        y[p] = R.model(kd, K, B, xt[p], t[p]) + 1e-3 * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + 0.05 * rng.uniform(-1, 1, xt.shape))
    return t, np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


def map_spec(name, K, B):
    """(fixed, tied) of a map by name for a K-peak model with baseline degree B."""
    base = [3 * K + j for j in range(B + 1)]
    widths = {3 * k + 2: (2, width_scale(k), 0.0) for k in range(1, K)}
    if name == "fixed_baseline":
        return base, {}
    if name == "tied_widths":
        return [], widths
    if name == "both":
        return base + [1], widths
    raise KeyError(name)


def full_start(T, xt, x0):
    """The full parameters a fit starts from: x0, with the fixed ones at their true values."""
    full = x0.copy()
    fx = T[0] == PR.FIXED
    full[:, fx] = xt[:, fx]
    return np.ascontiguousarray(full)
