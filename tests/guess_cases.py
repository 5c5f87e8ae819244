"""What the tests of curve_guess share: the four studies of the issue -- their data, the guess from the restatement, the fit
from it on the CPU oracle's least_squares_solver -- and the shapes and data of the GPU comparisons.  Run as a script it
records tests/golden/guess_study.json.  Test infrastructure, not part of the product."""
import json
import os

import numpy as np

import curve_restatement as R
import guess_restatement as G

HERE = os.path.dirname(os.path.abspath(__file__))
STUDY_GOLDEN = os.path.join(HERE, "golden", "guess_study.json")
MAX_EVALS = 500
CAP = 0.05                # the share of problems that may end above 1.05 x the cost at the truth or carry FALLBACK


def decay_study():
    """(a) 300 decays a e^(-k t) + c at the truth (50, 1, 0.5): 64 bins of 1/8, Poisson counts."""
    rng = np.random.default_rng(20261020)
    t = np.arange(64) * 0.125
    xt = np.tile(np.array([50.0, 1.0, 0.5]), (300, 1))
    y = np.stack([rng.poisson(R.model(R.EXPDECAY, 1, 0, xt[p], t)).astype(np.float64) for p in range(300)])
    return R.EXPDECAY, 1, 0, t, y, xt


def biexp_study():
    """(b) 200 biexponentials of the separable fits' study: (600, 1.5, 400, 0.3, 20) U(0.8, 1.2), 128 points of [0, 8]."""
    import sep_cases as SC
    t, y, xt, _ = SC.study_problems()
    return R.EXPDECAY, 2, 0, t, y, xt


def peak_study(kind, seed):
    """(c), (d) 200 two-peak spectra on 128 points of [-5, 5], a constant baseline, unit Gaussian noise."""
    rng = np.random.default_rng(seed)
    t = np.linspace(-5.0, 5.0, 128)
    n = 200
    xt = np.stack([rng.uniform(40, 60, n), rng.uniform(-2.5, -1.5, n), rng.uniform(0.4, 0.7, n),
                   rng.uniform(20, 30, n), rng.uniform(1.5, 2.5, n), rng.uniform(0.4, 0.7, n), rng.uniform(1, 3, n)], axis=1)
    y = np.stack([R.model(kind, 2, 0, xt[p], t) + rng.standard_normal(128) for p in range(n)])
    return kind, 2, 0, t, y, xt


STUDIES = {"a_decay": decay_study, "b_biexp": biexp_study, "c_gauss2": lambda: peak_study(R.GAUSS, 20261021),
           "d_lorentz2": lambda: peak_study(R.LORENTZ, 20261022)}


def run_study(oracle, name):
    """Every problem guessed by the restatement (numpy's least squares for the linear stage, smooth = 2) and fitted from the
    guess by the oracle's lm_solve: how many end within 1.05 x the cost at the truth, how many carry FALLBACK, how many
    fail either way, and the evaluations."""
    kind, K, B, t, y, xt = STUDIES[name]()
    nprob, m = y.shape
    n = R.nparams(kind, K, B)
    opts = oracle.default_options(max_evals=MAX_EVALS)
    reached = fallback = failed = 0
    evals = []
    for p in range(nprob):
        x0, flag = G.guess(kind, K, B, t, y[p])

        def ff(x, o, yp=y[p]):
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                o[:] = R.residual(kind, K, B, x, t, yp)

        def fj(x, J):
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                J[:, :] = R.jacobian(kind, K, B, x, t)
        truth = float(np.sum(R.residual(kind, K, B, xt[p], t, y[p]) ** 2))
        rc, x, fv, ib = oracle.lm_solve(ff, m, n, x0, jac=fj, opts=opts)
        ok = bool(np.isfinite(fv).all() and fv @ fv <= 1.05 * truth)
        fb = bool(flag & G.FALLBACK)
        reached += ok
        fallback += fb
        failed += (not ok) or fb
        evals.append(ib["fcn_count"] + ib["jacobian_count"])
    return {"nprob": nprob, "m": m, "reached": int(reached), "fallback": int(fallback), "failed": int(failed),
            "mean_evals": float(np.mean(evals)), "max_evals": int(max(evals))}


PARENT_GOLDEN = os.path.join(HERE, "golden", "guess_parent_fit.npz")


def parent_fit_case():
    """The call whose results tests/golden/guess_parent_fit.npz records on the commit before curve_guess: the first 64
    problems of study (b) from the truth times U(0.8, 1.2).  Returns (kind, K, B, t, y, x0)."""
    kind, K, B, t, y, xt = biexp_study()
    rng = np.random.default_rng(20261023)
    return kind, K, B, t, y[:64], xt[:64] * rng.uniform(0.8, 1.2, (64, 5))


def run_parent_fit(ds, x0="case"):
    """curve_fit_batch on parent_fit_case (x0: the case's own, or None) as numpy arrays by name."""
    import torch
    kind, K, B, t, y, x0c = parent_fit_case()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ds.device)
    x, fvec, sigma, cov, chi2, rank, ibs, status = ds.curve_fit_batch(kind, dev(t), dev(y), dev(x0c) if x0 == "case" else x0, ncomp=K,
                                                                      baseline=B)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in dict(x=x, fvec=fvec, sigma=sigma, cov=cov, chi2=chi2, rank=rank).items()}
    out["status"] = np.array(status, dtype=np.int32)
    out["evals"] = np.array([ib["fcn_count"] + ib["jacobian_count"] for ib in ibs], dtype=np.int32)
    return out


def record(oracle):
    out = {"max_evals_option": MAX_EVALS, "cap": CAP, "studies": {name: run_study(oracle, name) for name in STUDIES}}
    with open(STUDY_GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return out


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import pyoracle
    pyoracle.lib()
    print(json.dumps(record(pyoracle), indent=1))
