"""What the tests of the Poisson bootstrap share: the study of the photon-counting decay a*exp(-k*t) + c on 64 bins (pois_cases'
family, at the bias study's truth (50, 1, 0.5) and at one ten times weaker in a) -- the deviance fit on the CPU oracle's LM, the
Gaussian interval x +- 1.96 sigma of the inverse Fisher information (J'^T J')^-1 as the library's one-call fits return it, and
the percentile interval of the restatement's Poisson replicas, each refitted with the same deviance -- and the golden file's
name.  Run as a script it records tests/golden/boot_pois_study.json (`python tests/boot_pois_cases.py [processes]`).  Test
infrastructure, not part of the product."""
import json
import math
import os

import numpy as np

import boot_pois_restatement as BP
import boot_restatement as B
import curve_restatement as R
import pois_cases as PC
import pois_restatement as PR

HERE = os.path.dirname(os.path.abspath(__file__))
STUDY_GOLDEN = os.path.join(HERE, "golden", "boot_pois_study.json")
TRUTHS = ((50.0, PC.RATE, PC.BASE), (5.0, PC.RATE, PC.BASE))
NDATA, M = 300, PC.M
NREP, LEVEL, BOOT_SEED = 200, 0.95, 23
NGPU = 64                                       # the first data sets of a truth: what tests/test_gpu_boot_pois.py repeats on the device
ROWS = ("gauss", "percentile")
PARAMS = PC.PARAMS


def problems(ti):
    """t [NDATA, M], y (counts), the truth, x0 of truth number ti: pois_cases' decays without spread, as its bias study draws
    them."""
    return PC.decay_problems(TRUTHS[ti][0], NDATA, seed=PC.SEED, spread=0.0)


def fit(oracle, t, yp, x0):
    """The oracle's LM on the deviance residuals of the counts yp from x0 (analytic Jacobian, default options): x, or None when
    it did not end with status 0 and finite."""
    fcn, jac = PC.callbacks(t, yp, "poisson", True)
    with np.errstate(all="ignore"):
        rc, x, fv, ib = oracle.lm_solve(fcn, M, PC.N, np.array(x0, dtype=np.float64), jac=jac, opts=oracle.default_options())
    return x if rc == 0 and np.isfinite(x).all() and np.isfinite(fv).all() else None


def fisher_sigma(t, yp, x):
    """sqrt of the diagonal of (J'^T J')^-1, J' the Jacobian of the deviance residuals at x: the inverse Fisher information."""
    Jp = PR.jacobian(yp, None, PR.MU_FLOOR, R.residual(R.EXPDECAY, PC.K, PC.B, x, t, yp), R.jacobian(R.EXPDECAY, PC.K, PC.B, x, t))
    return np.sqrt(np.diag(np.linalg.inv(Jp.T @ Jp)))


def one(oracle, ti, p, data=None):
    """Data set p of truth ti: {"gauss": [0/1 per parameter], "percentile": the same, "ratio": sd_boot / sigma per parameter,
    "nvalid"}.  The replicas are those of problem p under BOOT_SEED, drawn from the fitted values of the fit."""
    t, y, xt, x0 = data or problems(ti)
    x = fit(oracle, t[p], y[p], x0[p])
    assert x is not None, (ti, p)
    sg = fisher_sigma(t[p], y[p], x)
    mu = R.model(R.EXPDECAY, PC.K, PC.B, x, t[p])
    ys, bad = BP.poisson(BOOT_SEED, mu[None], y[p][None], None, NREP, prob0=p)
    assert bad[0] == 0, (ti, p)
    xs = np.full((NREP, 1, 3), np.nan)
    for b in range(NREP):
        got = fit(oracle, t[p], ys[b, 0], x)
        if got is not None:
            xs[b, 0] = got
    lo, hi, _, sd, nvalid = B.summary(xs, LEVEL)
    return {"gauss": [int(x[j] - 1.96 * sg[j] <= xt[p, j] <= x[j] + 1.96 * sg[j]) for j in range(3)],
            "percentile": [int(lo[0, j] <= xt[p, j] <= hi[0, j]) for j in range(3)],
            "ratio": [float(sd[0, j] / sg[j]) for j in range(3)], "nvalid": int(nvalid[0])}


def _worker(job):
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import pyoracle
    pyoracle.lib()
    return one(pyoracle, *job)


def median_stderr(v):
    """The median of v and its standard error by the normal-theory rule 1.2533 s / sqrt(n)."""
    v = np.asarray(v, dtype=np.float64)
    return float(np.median(v)), float(1.2533 * v.std(ddof=1) / math.sqrt(len(v)))


def summarise(res):
    """The recorded form of one truth's results (a list of one()'s dicts, in data-set order)."""
    n = len(res)
    out = {"coverage": {}, "stderr": {}, "covered": {}}
    for r in ROWS:
        out["covered"][r] = {q: "".join(str(d[r][j]) for d in res) for j, q in enumerate(PARAMS)}
        out["coverage"][r] = {q: s.count("1") / n for q, s in out["covered"][r].items()}
        out["stderr"][r] = {q: math.sqrt(c * (1.0 - c) / n) for q, c in out["coverage"][r].items()}
    out["ratio"] = {q: [float(d["ratio"][j]).hex() for d in res] for j, q in enumerate(PARAMS)}
    for name, k in (("median_ratio", n), ("median_ratio_first%d" % NGPU, NGPU)):
        out[name] = {q: dict(zip(("median", "stderr"), median_stderr([d["ratio"][j] for d in res[:k]]))) for j, q in enumerate(PARAMS)}
    out["nvalid"] = [d["nvalid"] for d in res]
    out["min_valid"] = min(out["nvalid"])
    return out


def record(processes=1):
    jobs = [(ti, p) for ti in range(len(TRUTHS)) for p in range(NDATA)]
    if processes > 1:
        import multiprocessing
        with multiprocessing.Pool(processes) as pool:
            res = pool.map(_worker, jobs, chunksize=4)
    else:
        res = [_worker(j) for j in jobs]
    out = {"seed": PC.SEED, "ndata": NDATA, "m": M, "nrep": NREP, "level": LEVEL, "boot_seed": BOOT_SEED,
           "model": "a*exp(-k*t)+c, t in [0, 4], 64 bins, Poisson counts", "truths": [list(v) for v in TRUTHS],
           "study": [summarise(res[ti * NDATA:(ti + 1) * NDATA]) for ti in range(len(TRUTHS))]}
    with open(STUDY_GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return out


if __name__ == "__main__":
    import sys
    rec = record(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
    for truth, s in zip(rec["truths"], rec["study"]):
        print(truth, json.dumps({k: s[k] for k in ("coverage", "stderr", "median_ratio", "median_ratio_first%d" % NGPU, "min_valid")}, indent=1))
