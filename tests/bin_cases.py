"""The cases of the bin-integrated fits' tests (tests/test_bin_cpu.py, tests/test_gpu_bin.py, profiles/scripts/bin_rate.py): the
chosen list of launch shapes of the kernel, the Gaussian histogram -- counts in bins of width h of a Gaussian density --, and
the study on the CPU oracle whose results are recorded in tests/golden/bin_study.json (tests/golden/make_bin_study.py rewrites
it): the bias of the fitted width under the centre value times the bin width and under Gauss-Legendre rules of 2 .. 4 nodes,
noise-free and with Poisson noise.  Test infrastructure, not part of the product."""
import math
import os

import numpy as np

import bin_restatement as BR
import curve_restatement as R
import pois_restatement as PR

HERE = os.path.dirname(os.path.abspath(__file__))
STUDY_GOLDEN = os.path.join(HERE, "golden", "bin_study.json")

# the Gauss-Legendre rules as numpy gives them: the reference tests/test_bin_cpu.py holds the library's own literals to
leggauss = np.polynomial.legendre.leggauss


def lib_rule(order):
    """(xi, c) of nlh_bin_rule: the rule the device uses, so that a restated callback has its bits (host code, no GPU)."""
    from nonlin_amd import _lib
    return _lib.bin_rule(order)


def _launch_cases():
    """(m, Q, n): a chosen list, not a product.  Every m of the list -- odd m misaligns the node planes; 128 / 129 and
    256 / 257 are the edges of the flat form and of the row block -- with Q and n cycling through theirs alongside, twice
    round with the cycles shifted, so that every Q meets every n and both forms."""
    ms = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000]
    Qs = [1, 2, 3, 5, 16]
    ns = [1, 3, 9]
    out = []
    for c, m in enumerate(ms):
        out.append((m, Qs[c % 5], ns[c % 3]))
    for c, m in enumerate(ms):
        out.append((m, Qs[(c + 2) % 5], ns[(c + 1) % 3]))
    out += [(1000, 16, 9), (257, 16, 3), (1, 16, 9)]
    seen, uniq = set(), []
    for case in out:
        if case not in seen:
            seen.add(case)
            uniq.append(case)
    return uniq


LAUNCH_CASES = _launch_cases()


def case_id(case):
    m, Q, n = case
    return f"m{m}-Q{Q}-n{n}"


def rule(Q, seed=0):
    """The weights of a launch case: the library's rule up to 8 nodes, a random one beyond."""
    if Q <= 8:
        return lib_rule(Q)[1]
    return np.random.default_rng(seed + Q).uniform(0.05, 0.3, Q)


# ---- a spectrum in bins: the exp-free solves --------------------------------------------------------------------------
def line_problems(K, B, m, nprob, order=3, seed=2031, sigma=1e-3, shared=(), G=1):
    """Lorentzian spectra recorded in bins: lo, hi [nprob, m] (the bins around curve_cases' abscissae, each as wide as the
    spacing), y [nprob, m] (the restated order-`order` integral of the model over every bin plus sigma U(-1, 1)), x_true, x0
    [nprob, n].  shared, G: the true shared parameters of every G consecutive data sets are those of the first."""
    import curve_cases as CC
    t, y, xt, x0 = CC.curve_problems("lorentz", K, B, m, nprob=nprob, seed=seed)
    for p in range(nprob):
        xt[p, list(shared)] = xt[p - p % G, list(shared)]
    rng = np.random.default_rng(seed + 1)
    h = np.gradient(t, axis=1)
    lo, hi = t - 0.5 * h, t + 0.5 * h
    xi, c = lib_rule(order)
    tq = BR.nodes(lo, hi, xi)
    half = 0.5 * (hi - lo)
    y = np.empty((nprob, m))
    for p in range(nprob):
        y[p] = BR.reduce(R.model(R.LORENTZ, K, B, xt[p], tq[p]), c, half[p]) + sigma * rng.uniform(-1, 1, m) * h[p]
    x0 = xt * (1.0 + 0.05 * rng.uniform(-1, 1, xt.shape))
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi), np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


def line_callbacks(K, B, lo, hi, y, w, analytic, order=3):
    """(fcn, jac) of one problem for the oracle: the Lorentzian restatement at the nodes, then the restated transform."""
    xi, c = lib_rule(order)
    tq, half = BR.nodes(lo, hi, xi), 0.5 * (hi - lo)

    def fcn(x, out):
        out[:] = BR.residual(R.model(R.LORENTZ, K, B, np.array(x), tq), y, w, c, half)

    def jac(x, J):
        J[:, :] = BR.jacobian(R.jacobian(R.LORENTZ, K, B, np.array(x), tq).T, w, c, half).T
    return fcn, (jac if analytic else None)


# ---- the Gaussian histogram ------------------------------------------------------------------------------------------
M, N = 24, 3                                    # bins; parameters (amplitude, centre, width) of the library's Gaussian
COUNTS = 20000.0
HS = (1.0, 1.5, 2.0)                            # bin width over sigma
ORDERS = (1, 2, 3, 4)
NOISY_H, NOISY_NPROB, SEED = 1.5, 200, 11
MU = 0.2                                        # the centre, in bin widths off the middle edge


def edges(h):
    """M + 1 edges of bins of width h around 0."""
    return h * (np.arange(M + 1) - M / 2)


def truth(h, counts=COUNTS):
    """(amplitude, centre, width) of the density of `counts` events, sigma = 1: area = a sigma sqrt(2 pi)."""
    return np.array([counts / math.sqrt(2.0 * math.pi), MU * h, 1.0])


def exact_counts(h, x=None):
    """The exact integral of the density over every bin (erf)."""
    a, mu, s = truth(h) if x is None else x
    e = edges(h)
    cdf = np.array([0.5 * (1.0 + math.erf((v - mu) / (s * math.sqrt(2.0)))) for v in e])
    return a * s * math.sqrt(2.0 * math.pi) * (cdf[1:] - cdf[:-1])


def sheppard(h):
    """The relative bias of the width that Sheppard's correction predicts for the centre value: sqrt(1 + h^2 / 12) - 1."""
    return math.sqrt(1.0 + h * h / 12.0) - 1.0


def callbacks(h, y, order, poisson):
    """(fcn, jac) of one histogram for the oracle: the Gaussian restatement at the nodes of the order-`order` rule, the
    restated transform (integral mode) and, with poisson, the restated Poisson deviance."""
    e = edges(h)
    xi, c = lib_rule(order)
    tq, half = BR.nodes(e[:-1], e[1:], xi), 0.5 * (e[1:] - e[:-1])

    def fcn(x, out):
        r = BR.residual(R.model(R.GAUSS, 1, -1, np.array(x), tq), y, None, c, half)
        out[:] = PR.residual(y, None, PR.MU_FLOOR, r) if poisson else r

    def jac(x, J):
        Jb = BR.jacobian(R.jacobian(R.GAUSS, 1, -1, np.array(x), tq).T, None, c, half).T
        if poisson:
            r = BR.residual(R.model(R.GAUSS, 1, -1, np.array(x), tq), y, None, c, half)
            Jb = PR.jacobian(y, None, PR.MU_FLOOR, r, Jb)
        J[:, :] = Jb
    return fcn, jac


START = np.array([1.1, 1.0, 1.15])              # the start: these times the truth (the centre: the truth plus 0.1)


def _fit(oracle, h, y, order, poisson):
    fcn, jac = callbacks(h, y, order, poisson)
    x0 = truth(h) * START + np.array([0.0, 0.1, 0.0])
    rc, xo, fo, ib = oracle.lm_solve(fcn, M, N, x0, jac=jac, opts=oracle.default_options())
    return rc, xo


def noisy_histograms(h=NOISY_H, nprob=NOISY_NPROB, seed=SEED):
    """nprob Poisson histograms [nprob, M] of the exact counts."""
    rng = np.random.default_rng(seed)
    return rng.poisson(np.tile(exact_counts(h), (nprob, 1))).astype(np.float64)


def study(oracle):
    """The table of the README.  Noise-free: exact bin integrals, unweighted lm_solve under default options, the relative
    bias of the fitted width per h / sigma and order (order 1 is the centre value times the width).  Noisy: NOISY_NPROB Poisson
    histograms at h = NOISY_H sigma under the Poisson deviance, order 1 and order 3: failures, the mean of the fitted width
    with its standard error, its scatter."""
    out = {"m": M, "counts": COUNTS, "mu_in_bins": MU, "seed": SEED, "noise_free": {}, "noisy": {"h": NOISY_H, "nprob": NOISY_NPROB}}
    for h in HS:
        y = exact_counts(h)
        row = {"sheppard": sheppard(h)}
        for order in ORDERS:
            rc, xo = _fit(oracle, h, y, order, False)
            assert rc == 0, (h, order, rc)
            row[f"order{order}"] = float(xo[2] - 1.0)
        out["noise_free"][f"h{h:g}"] = row
    ys = noisy_histograms()
    for order in (1, 3):
        ss, bad = [], 0
        for y in ys:
            rc, xo = _fit(oracle, NOISY_H, y, order, True)
            if rc != 0 or not np.isfinite(xo).all():
                bad += 1
            else:
                ss.append(xo[2])
        ss = np.array(ss)
        out["noisy"][f"order{order}"] = {"failed": int(bad), "sigma_mean": float(ss.mean()),
                                         "sigma_stderr": float(ss.std(ddof=1) / np.sqrt(len(ss))), "sigma_scatter": float(ss.std(ddof=1))}
    return out
