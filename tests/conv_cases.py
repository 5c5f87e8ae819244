"""The cases of the instrument-response tests (tests/test_conv_cpu.py, tests/test_gpu_conv.py, profiles/scripts/conv_rate.py):
the chosen list of launch shapes of the kernels, and the photon-counting decay behind an instrument response -- a single
exponential on a constant baseline, binned, convolved with a Gaussian response, with Poisson noise -- with the two studies on
the CPU oracle whose results are recorded under tests/golden/: reconvolution against tail fitting, and what a last-bit change
of exp does to a fit.  Test infrastructure, not part of the product.
    python tests/conv_cases.py      re-measures both studies and rewrites the two golden files."""
import json
import os

import numpy as np

import conv_restatement as CR
import curve_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
EXT = {"zero": CR.ZERO, "hold": CR.HOLD}
ROW_TILE = 1024                                 # CONV_T of nonlin_amd/csrc/nlh_kernels_conv.h: the largest row tile


def origins(L):
    """Causal, one on, centred, anti-causal -- those that differ."""
    return sorted({0, min(1, L - 1), (L - 1) // 2, L - 1})


def _launch_cases():
    """(m, L, origin, extend, n, shared kernel): a chosen list, not a product.  Every L of the list with every origin, the m, n
    and the extension cycling through theirs alongside; L = m and L > m with every origin under both extensions; and the
    largest configuration of each form -- the row form at its largest tile with the most taps (and one tile more), the flat form
    at its largest m with the most taps, and the row form forced on a few rows with the most taps, where the LDS, not the
    workgroup, limits the columns of a pass."""
    T = ROW_TILE
    ms = [1, 2, 63, 64, 65, 128, 129, 256, 257, T - 1, T, T + 1, 2 * T + 1]
    ns = [1, 3, 4, 5, 9]
    out, c = [], 0
    for L in (1, 2, 3, 4, 5, 31, 32, 33, CR.MAX_L):
        for o in origins(L):
            m = ms[c % len(ms)]
            n = ns[c % len(ns)] if L < CR.MAX_L or m < 300 else 3
            out.append((m, L, o, ("zero", "hold")[c % 2], n, c % 3 != 0))
            c += 1
    for m, L in ((64, 64), (5, 9)):
        for o in origins(L):
            for ext in ("zero", "hold"):
                out.append((m, L, o, ext, ns[c % len(ns)], c % 3 != 0))
                c += 1
    out += [(2 * T + 1, CR.MAX_L, 0, "zero", 3, True), (2 * T + 1, CR.MAX_L, CR.MAX_L - 1, "hold", 3, False),
            (T, CR.MAX_L, 511, "zero", 1, True), (256, CR.MAX_L, 0, "hold", 4, False), (256, CR.MAX_L, 1023, "zero", 3, True),
            (128, CR.MAX_L, 511, "zero", 9, True), (1, CR.MAX_L, 7, "hold", 9, False), (2, CR.MAX_L, 0, "zero", 5, True),
            (63, CR.MAX_L, 1000, "zero", 9, False)]
    seen, uniq = set(), []
    for case in out:
        if case not in seen:
            seen.add(case)
            uniq.append(case)
    return uniq


LAUNCH_CASES = _launch_cases()


def case_id(case):
    m, L, o, ext, n, shared = case
    return f"m{m}-L{L}-o{o}-{ext}-n{n}-{'shared' if shared else 'per'}"


# ---- a spectrum behind a line shape: the exp-free solves --------------------------------------------------------------
LINE_ORIGIN, LINE_EXTEND = 4, "hold"


def line_shape():
    """A centred 9-tap line shape (origin 4): binomial-like taps with a skew, divided by their sequential sum."""
    g = np.array([1.0, 6.0, 20.0, 50.0, 70.0, 45.0, 22.0, 8.0, 2.0])
    tot = 0.0
    for v in g:
        tot = tot + v
    return g / tot


def line_problems(K, B, m, nprob, seed=2027, sigma=1e-3, shared=(), G=1):
    """curve_cases.curve_problems of a Lorentzian model seen through line_shape(): t, y [nprob, m], x_true, x0 [nprob, n], y the
    convolved model plus sigma U(-1, 1).  shared, G: the true shared parameters of every G consecutive data sets are those of
    the first."""
    import curve_cases as CC
    t, y, xt, x0 = CC.curve_problems("lorentz", K, B, m, nprob=nprob, seed=seed)
    for p in range(nprob):
        xt[p, list(shared)] = xt[p - p % G, list(shared)]
    rng = np.random.default_rng(seed + 1)
    k = line_shape()
    for p in range(nprob):
        y[p] = CR.convolve(R.model(R.LORENTZ, K, B, xt[p], t[p]), k, LINE_ORIGIN, EXT[LINE_EXTEND]) + sigma * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + 0.05 * rng.uniform(-1, 1, xt.shape))
    return t, np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


def line_callbacks(K, B, t, y, w, analytic):
    """(fcn, jac) of one problem for the oracle: the Lorentzian restatement, then the restated transform."""
    k, e = line_shape(), EXT[LINE_EXTEND]

    def fcn(x, out):
        out[:] = CR.residual(R.residual(R.LORENTZ, K, B, x, t, y), y, w, k, LINE_ORIGIN, e)

    def jac(x, J):
        J[:, :] = CR.jacobian(R.jacobian(R.LORENTZ, K, B, x, t).T, w, k, LINE_ORIGIN, e).T
    return fcn, (jac if analytic else None)


# ---- the decay behind an instrument response --------------------------------------------------------------------------
KIND, K, B = "expdecay", 1, 0                   # parameters: a, k, c0
FORMULA, PARAMS = "a*exp(-(k*t)) + c", ("a", "k", "c")
M, N = 128, 3
BIN = 1.0 / 16.0
IRF_L, IRF_SIGMA, IRF_CENTRE = 32, 2.5, 10      # taps, width and centre in bins: a causal kernel (origin 0)
ORIGIN, EXTEND = 0, "zero"
TRUTHS = ((2000.0, 4.0, 0.5), (200.0, 1.0, 0.5))    # a lifetime of 4 bins, comparable to the response; and a slow decay
START = (0.9, 1.1, 1.0)                         # the start of the study: these times the truth
SEED = 7
STUDY_NPROB, PERT_NPROB = 200, 24
STUDY_GOLDEN = os.path.join(HERE, "golden", "conv_study.json")
PERT_GOLDEN = os.path.join(HERE, "golden", "conv_perturbation.json")
STUDY_FITS = ((0, "reconvolution", None), (0, "tail20", 20), (0, "tail32", 32), (1, "reconvolution", None), (1, "tail32", 32))


def irf():
    """The response: a Gaussian of IRF_SIGMA bins centred on tap IRF_CENTRE, IRF_L taps, divided by its sequential sum."""
    j = np.arange(IRF_L)
    g = np.exp(-0.5 * ((j - IRF_CENTRE) / IRF_SIGMA) ** 2)
    tot = 0.0
    for v in g:
        tot = tot + v
    return g / tot


def decay_model(x, t, exp=np.exp):
    """curve_restatement.model(EXPDECAY, 1, 0, x, t) with the exponential handed in."""
    e = exp(-(x[1] * t))
    s = np.zeros(np.shape(t)) + x[0] * e
    return s + np.full(np.shape(t), x[2])


def decay_jacobian(x, t, exp=np.exp):
    """curve_restatement.jacobian(EXPDECAY, 1, 0, x, t) as [n, m] (rows last), with the exponential handed in."""
    e = exp(-(x[1] * t))
    return np.stack([e, -((x[0] * t) * e), np.ones(np.shape(t))])


def decay_problems(truth, nprob, seed=SEED, spread=0.0, start=None):
    """t, y [nprob, M] (counts), x_true, x0 [nprob, 3]: truth (a (1 + spread U(-1, 1)), k, c), y Poisson of the model
    convolved with irf(); x0 = start * truth, or within 10 % of the truth."""
    rng = np.random.default_rng(seed)
    k = irf()
    t = np.tile(BIN * np.arange(M), (nprob, 1))
    xt, x0, y = np.empty((nprob, 3)), np.empty((nprob, 3)), np.empty((nprob, M))
    for p in range(nprob):
        xt[p] = [truth[0] * (1.0 + spread * rng.uniform(-1, 1)), truth[1], truth[2]]
        y[p] = rng.poisson(CR.convolve(decay_model(xt[p], t[p]), k, ORIGIN, EXT[EXTEND])).astype(np.float64)
        x0[p] = xt[p] * (np.array(start) if start is not None else 1.0 + 0.1 * rng.uniform(-1, 1, 3))
    return np.ascontiguousarray(t), y, xt, x0


def callbacks(t, y, analytic, tail=None, exp=np.exp):
    """(fcn, jac, m) of one problem for the oracle's solvers, unweighted.  tail None: the restated reconvolution -- the inner
    residual model - y, then conv_restatement.residual / jacobian with irf(); tail = b: the plain decay on the rows from bin b
    on."""
    if tail is not None:
        tt, yy = t[tail:], y[tail:]

        def fcn(x, out):
            out[:] = decay_model(x, tt, exp) - yy

        def jac(x, J):
            J[:, :] = decay_jacobian(x, tt, exp).T
        return fcn, (jac if analytic else None), len(tt)
    k, e = irf(), EXT[EXTEND]

    def fcn(x, out):
        out[:] = CR.residual(decay_model(x, t, exp) - y, y, None, k, ORIGIN, e)

    def jac(x, J):
        J[:, :] = CR.jacobian(decay_jacobian(x, t, exp), None, k, ORIGIN, e).T
    return fcn, (jac if analytic else None), len(t)


def study(oracle, nprob=STUDY_NPROB, seed=SEED):
    """The table of the README: STUDY_NPROB decays per truth, lm_solve under default options, analytic Jacobian, unweighted,
    from START times the truth: failures, the mean of k with its standard error, and its scatter, for reconvolution and
    for fits of the tail."""
    out = {"nprob": nprob, "m": M, "bin": BIN, "seed": seed, "taps": IRF_L, "sigma_bins": IRF_SIGMA, "centre_bin": IRF_CENTRE, "fits": {}}
    data = [decay_problems(tr, nprob, seed=seed, start=START) for tr in TRUTHS]
    for which, name, tail in STUDY_FITS:
        t, y, xt, x0 = data[which]
        ks, bad = [], 0
        for p in range(nprob):
            fcn, jac, m = callbacks(t[p], y[p], True, tail)
            rc, xo, fo, ib = oracle.lm_solve(fcn, m, N, x0[p], jac=jac, opts=oracle.default_options())
            if rc != 0 or not np.isfinite(xo).all():
                bad += 1
            else:
                ks.append(xo[1])
        ks = np.array(ks)
        out["fits"][f"truth{which}_{name}"] = {"truth": list(TRUTHS[which]), "failed": int(bad), "k_mean": float(ks.mean()),
                                               "k_stderr": float(ks.std(ddof=1) / np.sqrt(len(ks))), "k_scatter": float(ks.std(ddof=1))}
    return out


def _ulp_noise(fn, rng):
    """fn with every result moved by -1, 0 or +1 ulp at random."""
    def g(v):
        out = fn(v)
        k = rng.integers(-1, 2, np.shape(out))
        return np.where(k < 0, np.nextafter(out, -np.inf), np.where(k > 0, np.nextafter(out, np.inf), out))
    return g


def family(nprob=PERT_NPROB, seed=SEED):
    """The decay family of the solves: the first nprob / 2 problems at each truth, amplitudes spread by 30 %, starts within 10 %."""
    parts = [decay_problems(tr, nprob // 2, seed=seed, spread=0.3) for tr in TRUTHS]
    return tuple(np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(4))


def perturbation_study(oracle, nprob=PERT_NPROB, seed=SEED):
    """Every problem of the family solved twice by reconvolution, with numpy's exp and with each call's results moved by -1, 0
    or +1 ulp at random: the worst relative change of a component of x, per Jacobian mode."""
    out = {"nprob": nprob, "seed": seed}
    t, y, xt, x0 = family(nprob, seed)
    for analytic in (True, False):
        rng = np.random.default_rng(seed + 1)
        worst = 0.0
        for p in range(nprob):
            xs = []
            for noisy in (False, True):
                fcn, jac, m = callbacks(t[p], y[p], analytic, exp=_ulp_noise(np.exp, rng) if noisy else np.exp)
                rc, xo, fo, ib = oracle.lm_solve(fcn, m, N, x0[p], jac=jac, opts=oracle.default_options())
                assert rc == 0, (analytic, p, rc)
                xs.append(xo)
            worst = max(worst, float(np.max(np.abs(xs[1] - xs[0]) / np.abs(xs[0]))))
        out["analytic" if analytic else "fd"] = worst
    return out


def recorded_tolerance(analytic):
    """What the GPU comparisons of exp-carrying fits allow between the device's x and the oracle's: 4 x the recorded worst
    change, the factor tests/pois_cases.py uses (the device library's error pattern is not the random one)."""
    with open(PERT_GOLDEN) as fh:
        rec = json.load(fh)
    return 4.0 * rec["analytic" if analytic else "fd"]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import pyoracle
    pyoracle.lib()
    for path, fn in ((STUDY_GOLDEN, study), (PERT_GOLDEN, perturbation_study)):
        res = fn(pyoracle)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print(path, json.dumps(res, indent=1, sort_keys=True))
