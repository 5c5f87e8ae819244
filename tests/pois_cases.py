"""The cases of the Poisson-fit tests (tests/test_pois_cpu.py, tests/test_gpu_pois.py, profiles/scripts/pois_rate.py): single
exponential decays on a constant baseline, binned into m = 64 channels on t = 0 .. 4, with Poisson noise -- the photon-counting
decay the feature is for.  Also the two studies on the CPU oracle whose results are recorded under tests/golden/: the bias of
the three estimators, and what a last-bit change of log1p / log does to a fit.  Test infrastructure, not part of the product.
    python tests/pois_cases.py      re-measures both studies and rewrites the two golden files."""
import json
import os

import numpy as np

import curve_restatement as R
import pois_restatement as PR

HERE = os.path.dirname(os.path.abspath(__file__))
KIND, K, B = "expdecay", 1, 0                   # parameters: a, k, c0
FORMULA, PARAMS = "a*exp(-(k*t)) + c", ("a", "k", "c")
M, N = 64, 3
AMPLITUDES = (50.0, 1000.0)                     # the decay family: a = AMPLITUDES[i] * (1 +- 0.3)
RATE, BASE = 1.0, 0.5
SEED = 11
BIAS_GOLDEN = os.path.join(HERE, "golden", "pois_bias_study.json")
PERT_GOLDEN = os.path.join(HERE, "golden", "pois_perturbation.json")
BIAS_NPROB, PERT_NPROB = 300, 24
# The area rule sum mu = sum y holds at the exact maximum of a Poisson likelihood whose model has a free additive constant.
# What the oracle's LM leaves of it on this family under default options, measured: 3.6e-7 (a ~ 50) and 1.9e-9 (a ~ 1000),
# analytic and forward differences alike; ten times that is asserted, of the oracle in tests/test_pois_cpu.py and of the device
# in tests/test_gpu_pois.py.
AREA_BOUND = {50.0: 3.6e-6, 1000.0: 1.9e-8}


def decay_problems(a, nprob, seed=SEED, spread=0.3, m=M):
    """t, y [nprob, m] (counts), x_true, x0 [nprob, 3]: truth (a (1 + spread U(-1, 1)), RATE, BASE), y Poisson of the model,
    x0 within 10 % of the truth."""
    rng = np.random.default_rng(seed)
    t = np.tile(np.linspace(0.0, 4.0, m), (nprob, 1))
    xt, x0, y = np.empty((nprob, 3)), np.empty((nprob, 3)), np.empty((nprob, m))
    for p in range(nprob):
        xt[p] = [a * (1.0 + spread * rng.uniform(-1, 1)), RATE, BASE]
        y[p] = rng.poisson(R.model(R.EXPDECAY, K, B, xt[p], t[p])).astype(np.float64)
        x0[p] = xt[p] * (1.0 + 0.1 * rng.uniform(-1, 1, 3))
    return np.ascontiguousarray(t), y, xt, x0


def ls_weights(y):
    """What a user of weighted least squares passes for counts: 1 / sqrt(max(y, 1))."""
    return 1.0 / np.sqrt(np.maximum(y, 1.0))


def callbacks(t, y, estimator, analytic, w=None, f=PR.MU_FLOOR, log1p=np.log1p, log=np.log, touched=None):
    """(fcn, jac) of one problem for the oracle's solvers.  estimator: "poisson" (the restated deviance residual; w: the 0 / 1
    mask), "wls" (weighted least squares with ls_weights) or "ls".  touched: a list that gets True whenever a model value
    falls below the floor."""
    kd = R.EXPDECAY
    if estimator == "poisson":
        def fcn(x, out):
            r = R.residual(kd, K, B, x, t, y)
            if touched is not None and ((r + y) < f).any():
                touched.append(True)
            out[:] = PR.residual(y, w, f, r, log1p=log1p, log=log)

        def jac(x, J):
            J[:, :] = PR.jacobian(y, w, f, R.residual(kd, K, B, x, t, y), R.jacobian(kd, K, B, x, t), log1p=log1p, log=log)
    else:
        wl = ls_weights(y) if estimator == "wls" else None

        def fcn(x, out):
            out[:] = R.residual(kd, K, B, x, t, y, wl)

        def jac(x, J):
            J[:, :] = R.jacobian(kd, K, B, x, t, wl)
    return fcn, (jac if analytic else None)


def bias_study(oracle, a=50.0, nprob=BIAS_NPROB, seed=SEED):
    """The table of the README: mean relative bias, its standard error and the relative scatter of the decay rate k and the
    baseline c for the three estimators, truth (a, 1, 0.5), analytic Jacobian, default options."""
    t, y, xt, x0 = decay_problems(a, nprob, seed=seed, spread=0.0)
    out = {"a": a, "nprob": nprob, "m": M, "seed": seed, "estimators": {}}
    for est in ("wls", "ls", "poisson"):
        xs, bad = np.empty((nprob, 3)), 0
        for p in range(nprob):
            fcn, jac = callbacks(t[p], y[p], est, True)
            rc, xo, fo, ib = oracle.lm_solve(fcn, M, N, x0[p], jac=jac, opts=oracle.default_options())
            bad += rc != 0
            xs[p] = xo
        rel = (xs - xt) / xt
        out["estimators"][est] = {"failed": int(bad),
                                  "k_bias": float(rel[:, 1].mean()), "k_stderr": float(rel[:, 1].std(ddof=1) / np.sqrt(nprob)),
                                  "k_scatter": float(rel[:, 1].std(ddof=1)),
                                  "c_bias": float(rel[:, 2].mean()), "c_stderr": float(rel[:, 2].std(ddof=1) / np.sqrt(nprob))}
    return out


def _ulp_noise(fn, rng):
    """fn with every result moved by -1, 0 or +1 ulp at random."""
    def g(v):
        out = fn(v)
        k = rng.integers(-1, 2, np.shape(out))
        return np.where(k < 0, np.nextafter(out, -np.inf), np.where(k > 0, np.nextafter(out, np.inf), out))
    return g


def perturbation_study(oracle, nprob=PERT_NPROB, seed=SEED):
    """Every problem of the family's first nprob solved twice, with numpy's log1p / log and with each call's result moved by
    -1, 0 or +1 ulp at random: the worst relative change of a component of x, per amplitude and Jacobian."""
    out = {"nprob": nprob, "seed": seed, "worst": {}}
    for a in AMPLITUDES:
        t, y, xt, x0 = decay_problems(a, nprob, seed=seed)
        for analytic in (True, False):
            rng = np.random.default_rng(seed + 1)
            worst = 0.0
            for p in range(nprob):
                xs = []
                for noisy in (False, True):
                    l1, l = (_ulp_noise(np.log1p, rng), _ulp_noise(np.log, rng)) if noisy else (np.log1p, np.log)
                    fcn, jac = callbacks(t[p], y[p], "poisson", analytic, log1p=l1, log=l)
                    rc, xo, fo, ib = oracle.lm_solve(fcn, M, N, x0[p], jac=jac, opts=oracle.default_options())
                    assert rc == 0, (a, analytic, p, rc)
                    xs.append(xo)
                worst = max(worst, float(np.max(np.abs(xs[1] - xs[0]) / np.abs(xs[0]))))
            out["worst"][f"a{int(a)}_{'analytic' if analytic else 'fd'}"] = worst
    out["analytic"] = max(v for k, v in out["worst"].items() if k.endswith("analytic"))
    out["fd"] = max(v for k, v in out["worst"].items() if k.endswith("fd"))
    return out


def recorded_tolerance(analytic):
    """What the GPU comparisons allow between the device's x and the oracle's: 4 x the recorded worst change, the margin being
    there because the device library's error pattern is not the random one."""
    with open(PERT_GOLDEN) as fh:
        rec = json.load(fh)
    return 4.0 * rec["analytic" if analytic else "fd"]


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import pyoracle
    pyoracle.lib()
    for path, study in ((BIAS_GOLDEN, bias_study), (PERT_GOLDEN, perturbation_study)):
        res = study(pyoracle)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print(path, json.dumps(res, indent=1, sort_keys=True))
