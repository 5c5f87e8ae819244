"""What the tests of the bootstrap share: the decay family of the study -- its data, the fit on the CPU oracle's
least_squares_solver, the Gaussian interval of s^2 (J^T J)^-1 and the percentile interval of each kind from the restatement's
replicas -- and the golden file's name.  Run as a script it records tests/golden/boot_study.json.  Test infrastructure, not part
of the product."""
import json
import math
import os

import numpy as np

import boot_restatement as B

HERE = os.path.dirname(os.path.abspath(__file__))
STUDY_GOLDEN = os.path.join(HERE, "golden", "boot_study.json")
# a*exp(-k*t) + c on 32 points of [0, 1] with k ~ U(0.4, 0.9): the window covers 0.4 .. 0.9 lifetimes
SEED, NDATA, M, NOISE = 20261027, 400, 32, 0.05
NREP, LEVEL, BOOT_SEED = 200, 0.95, 17
MAX_EVALS = 200
ROWS = ("gauss", "residual", "wild", "pairs")
PARAMS = ("a", "k", "c")


def problems(ndata=NDATA):
    """t [M], y [ndata, M], the truth [ndata, 3] as (a, k, c): a ~ U(2, 5), k ~ U(0.4, 0.9), c ~ U(-1, 1), Gaussian noise of
    0.05.  The first ndata of the study's (one generator, drawn in full)."""
    rng = np.random.default_rng(SEED)
    t = np.linspace(0.0, 1.0, M)
    xt = np.stack([rng.uniform(2.0, 5.0, NDATA), rng.uniform(0.4, 0.9, NDATA), rng.uniform(-1.0, 1.0, NDATA)], axis=1)
    y = model(xt, t) + NOISE * rng.standard_normal((NDATA, M))
    return t, y[:ndata], xt[:ndata]


def model(x, t):
    x = np.atleast_2d(x)
    return x[:, 0:1] * np.exp(-x[:, 1:2] * t[None, :]) + x[:, 2:3]


def jacobian(x, t):
    e = np.exp(-x[1] * t)
    return np.stack([e, -x[0] * t * e, np.ones(len(t))], axis=1)


def fit(oracle, t, yp, wp, x0):
    """The oracle's lm_solve of w*(model - y) from x0: x, or None when it did not end finite."""
    def ff(x, o):
        with np.errstate(over="ignore", invalid="ignore"):
            o[:] = wp * (model(x, t)[0] - yp)

    def fj(x, J):
        with np.errstate(over="ignore", invalid="ignore"):
            J[:, :] = wp[:, None] * jacobian(x, t)
    rc, x, fv, ib = oracle.lm_solve(ff, M, 3, np.array(x0, dtype=np.float64), jac=fj, opts=oracle.default_options(max_evals=MAX_EVALS))
    return x if np.isfinite(x).all() and np.isfinite(fv).all() else None


def gauss_interval(t, yp, x):
    """x -+ 1.96 sigma, sigma^2 the diagonal of s^2 (J^T J)^-1 at x, s^2 = sum r^2 / (M - 3)."""
    r = model(x, t)[0] - yp
    J = jacobian(x, t)
    cov = (r @ r) / (M - 3) * np.linalg.inv(J.T @ J)
    sg = np.sqrt(np.diag(cov))
    return x - 1.96 * sg, x + 1.96 * sg


def boot_interval(oracle, kind, t, yp, x, p):
    """The percentile interval of the kind's NREP replicas of data set p, each refitted from x; a failed refit is a NaN row."""
    one = np.ones(M)
    mu = model(x, t)[0]
    xs = np.full((NREP, 1, 3), np.nan)
    for b in range(NREP):
        ys, ws = B.resample_one(B.KINDS[kind], BOOT_SEED, p, b, mu, yp, None, True)
        got = fit(oracle, t, ys, one if ws is None else ws, x)
        if got is not None:
            xs[b, 0] = got
    lo, hi, _, _, nvalid = B.summary(xs, LEVEL)
    return lo[0], hi[0], int(nvalid[0])


def run_study(oracle, ndata=NDATA):
    """row -> parameter -> the data sets (0 / 1 each, in order) whose interval holds the truth; and the valid refits."""
    t, y, xt = problems(ndata)
    rows = {r: {q: [] for q in PARAMS} for r in ROWS}
    nvalid = {r: [] for r in ROWS[1:]}
    for p in range(ndata):
        x = fit(oracle, t, y[p], np.ones(M), xt[p])
        iv = {"gauss": gauss_interval(t, y[p], x)}
        for kind in ROWS[1:]:
            lo, hi, nv = boot_interval(oracle, kind, t, y[p], x, p)
            iv[kind] = (lo, hi)
            nvalid[kind].append(nv)
        for r in ROWS:
            for j, q in enumerate(PARAMS):
                rows[r][q].append(int(iv[r][0][j] <= xt[p, j] <= iv[r][1][j]))
    return rows, nvalid


def record(oracle):
    rows, nvalid = run_study(oracle)
    cover = {r: {q: sum(v) / NDATA for q, v in rows[r].items()} for r in ROWS}
    out = {"seed": SEED, "ndata": NDATA, "m": M, "noise": NOISE, "nrep": NREP, "level": LEVEL, "boot_seed": BOOT_SEED,
           "max_evals": MAX_EVALS, "model": "a*exp(-k*t)+c, t in [0, 1], k in [0.4, 0.9]",
           "coverage": cover,
           "stderr": {r: {q: math.sqrt(c * (1.0 - c) / NDATA) for q, c in cover[r].items()} for r in ROWS},
           "min_valid": {r: int(min(v)) for r, v in nvalid.items()},
           "covered": {r: {q: "".join(str(b) for b in v) for q, v in rows[r].items()} for r in ROWS}}
    with open(STUDY_GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import pyoracle
    pyoracle.lib()
    rec = record(pyoracle)
    print(json.dumps({"coverage": rec["coverage"], "stderr": rec["stderr"], "min_valid": rec["min_valid"]}, indent=1))
