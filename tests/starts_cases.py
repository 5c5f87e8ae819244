"""What the tests of starts share: the sinusoid family of the study -- its data, the boxes, the scan by the restatement, the fits
on the CPU oracle's least_squares_solver -- and the golden file's name.  Run as a script it records
tests/golden/starts_study.json.  Test infrastructure, not part of the product."""
import json
import math
import os

import numpy as np

import sep_cases as SC
import sep_restatement as SR
import starts_restatement as S

HERE = os.path.dirname(os.path.abspath(__file__))
STUDY_GOLDEN = os.path.join(HERE, "golden", "starts_study.json")
SEED, NPROB, M, NOISE = 20261024, 60, 256, 0.3
MAX_EVALS = 100
# the full model a*sin(w*t + ph) + c over (a, w, ph, c): a is scanned in the logarithm
FULL_LOWER, FULL_UPPER, FULL_LOG = (0.1, 1.0, -math.pi, -2.0), (10.0, 60.0, math.pi, 2.0), (0,)
FULL_NCAND, FULL_KEEP = (64, 256, 1024, 4096), (1, 4)
# the projected model a*sin(w*t) + b*cos(w*t) + c over (a, w, b, c): a, b, c are linear, w alone is scanned
SEP_LINEAR, SEP_LOWER, SEP_UPPER = (0, 2, 3), (1.0,), (60.0,)
SEP_NCAND = (16, 64, 256)
SEP_FORMULA, SEP_PARAMS = "a*sin(w*t)+b*cos(w*t)+c", ("a", "w", "b", "c")


def problems(nprob=NPROB):
    """t [M], y [nprob, M], the truth [nprob, 4] as (a, w, ph, c): w ~ U(5, 50), a ~ U(1, 5), ph ~ U(-3, 3), c ~ U(-1, 1),
    Gaussian noise of 0.3, 256 points of [0, 10].  The first nprob of the study's 60 (one generator, drawn in full)."""
    rng = np.random.default_rng(SEED)
    t = np.linspace(0.0, 10.0, M)
    xt = np.stack([rng.uniform(1.0, 5.0, NPROB), rng.uniform(5.0, 50.0, NPROB), rng.uniform(-3.0, 3.0, NPROB),
                   rng.uniform(-1.0, 1.0, NPROB)], axis=1)
    y = full_model(xt, t) + NOISE * rng.standard_normal((NPROB, M))
    return t, y[:nprob], xt[:nprob]


def full_model(x, t):
    x = np.atleast_2d(x)
    return x[:, 0:1] * np.sin(x[:, 1:2] * t[None, :] + x[:, 2:3]) + x[:, 3:4]


def full_jacobian(x, t):
    arg = x[1] * t + x[2]
    return np.stack([np.sin(arg), (x[0] * t) * np.cos(arg), x[0] * np.cos(arg), np.ones(len(t))], axis=1)


def sep_model(p, t):
    return p[0] * np.sin(p[1] * t) + p[2] * np.cos(p[1] * t) + p[3]


def sep_jacobian(p, t):
    s, c = np.sin(p[1] * t), np.cos(p[1] * t)
    return np.stack([s, t * (p[0] * c - p[2] * s), c, np.ones(len(t))], axis=1)


def truth_cost(t, y, xt):
    """The cost at the truth of every problem: what a fit has to come within 1.05 x of."""
    return np.sum((full_model(xt, t) - y) ** 2, axis=1)


def _solve(oracle, ff, fj, n, x0):
    rc, x, fv, ib = oracle.lm_solve(ff, M, n, np.array(x0, dtype=np.float64), jac=fj, opts=oracle.default_options(max_evals=MAX_EVALS))
    return float(fv @ fv) if np.isfinite(fv).all() else math.inf


def fit_full(oracle, t, yp, x0):
    """The final cost of the oracle's lm_solve on the full model from x0."""
    def ff(x, o):
        with np.errstate(over="ignore", invalid="ignore"):
            o[:] = full_model(x, t)[0] - yp

    def fj(x, J):
        with np.errstate(over="ignore", invalid="ignore"):
            J[:, :] = full_jacobian(x, t)
    return _solve(oracle, ff, fj, 4, x0)


def sep_callbacks(t, yp):
    return (lambda p: sep_model(p, t) - yp), (lambda p: sep_jacobian(p, t))


def fit_sep(oracle, t, yp, w0):
    """The final cost of the oracle's lm_solve over w alone, a, b, c projected out (the separable restatement, Kaufman)."""
    of, oj = SC.oracle_callbacks(*sep_callbacks(t, yp), 4, SEP_LINEAR, True)
    return _solve(oracle, of, oj, 1, [w0])


def scan_full(t, y, ncand):
    """costs [nprob, ncand] of the full model at the candidates of the box, and the table."""
    table = S.candidates(FULL_LOWER, FULL_UPPER, FULL_LOG, 0, ncand)
    model = full_model(table, t)
    return np.stack([S.cost(model - y[p][None, :]) for p in range(len(y))]), table


def scan_sep(t, y, ncand):
    """costs [nprob, ncand] of the projected model at the candidates of w's box, and the table [ncand, 1]."""
    table = S.candidates(SEP_LOWER, SEP_UPPER, (), 0, ncand)
    costs = np.empty((len(y), ncand))
    for p in range(len(y)):
        fcn, jac = sep_callbacks(t, y[p])
        costs[p] = S.cost(np.stack([SR.residual(fcn, jac, 4, SEP_LINEAR, table[c]) for c in range(ncand)]))
    return costs, table


def centre(lower, upper, log=()):
    """The point of the box at u = 1/2 in every dimension, by the candidates' own maps."""
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    return np.array([lo[d] * math.exp(0.5 * math.log(hi[d] / lo[d])) if d in log else lo[d] + 0.5 * (hi[d] - lo[d]) for d in range(len(lo))])


def run_study(oracle, nprob=NPROB, full_ncand=FULL_NCAND, sep_ncand=SEP_NCAND):
    """row -> the problems (0 / 1 each, in order) whose best fit ends within 1.05 x the cost at the truth.  The candidates of a
    smaller scan are the first of a larger one, so each model is scanned once, at its largest count."""
    t, y, xt = problems(nprob)
    cap = 1.05 * truth_cost(t, y, xt)
    rows = {}
    c4 = centre(FULL_LOWER, FULL_UPPER, FULL_LOG)
    rows["full_centre"] = [int(fit_full(oracle, t, y[p], c4) <= cap[p]) for p in range(nprob)]
    costs, table = scan_full(t, y, max(full_ncand))
    for nc in full_ncand:
        x0, _, idx = S.search(costs[:, :nc], table, max(FULL_KEEP))
        final = np.array([[fit_full(oracle, t, y[p], x0[p, k]) if idx[p, k] >= 0 else math.inf for k in range(max(FULL_KEEP))]
                          for p in range(nprob)])
        for keep in FULL_KEEP:
            rows[f"full_{nc}_keep{keep}"] = [int(final[p, :keep].min() <= cap[p]) for p in range(nprob)]
    rows["sep_centre"] = [int(fit_sep(oracle, t, y[p], centre(SEP_LOWER, SEP_UPPER)[0]) <= cap[p]) for p in range(nprob)]
    costs, table = scan_sep(t, y, max(sep_ncand))
    for nc in sep_ncand:
        x0, _, idx = S.search(costs[:, :nc], table, 1)
        rows[f"sep_{nc}"] = [int(idx[p, 0] >= 0 and fit_sep(oracle, t, y[p], x0[p, 0, 0]) <= cap[p]) for p in range(nprob)]
    return rows


def record(oracle):
    rows = run_study(oracle)
    out = {"seed": SEED, "nprob": NPROB, "m": M, "noise": NOISE, "max_evals": MAX_EVALS,
           "success": "final cost <= 1.05 x the cost at the truth",
           "reached": {k: int(sum(v)) for k, v in rows.items()}, "problems": {k: "".join(str(b) for b in v) for k, v in rows.items()}}
    with open(STUDY_GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import pyoracle
    pyoracle.lib()
    print(json.dumps(record(pyoracle)["reached"], indent=1))
