"""The coverage study of the studentised and the BCa interval: the Gaussian, percentile, bootstrap-t and BCa interval of the same
fit side by side on the two families whose percentile interval the earlier studies found short -- the 400 short-window decays
of boot_cases (kind "residual", 200 replicas: the replicas of boot_study.json) and the 300 photon-counting decays of
boot_pois_cases at the truth (5, 1, 0.5) (Poisson replicas: those of boot_pois_study.json) --, everything on the CPU oracle's
solver over tests/boot_ci_restatement.py.  The refits' standard errors are each family's own sigma at the refit; the delete-one
refits start from the fit.  Run as a script it records tests/golden/boot_ci_study.json (`python tests/boot_ci_cases.py
[processes]`).  Test infrastructure, not part of the product."""
import json
import math
import os

import numpy as np

import boot_cases as BC
import boot_pois_cases as BPC
import boot_pois_restatement as BP
import boot_restatement as B
import boot_ci_restatement as R
import curve_restatement as CR
import pois_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
STUDY_GOLDEN = os.path.join(HERE, "golden", "boot_ci_study.json")
FAMILIES = ("decay", "poisson")
NDATA = {"decay": BC.NDATA, "poisson": BPC.NDATA}
ROWS = ("gauss", "percentile", "student", "bca")
PARAMS = ("a", "k", "c")
NREP, LEVEL = 200, 0.95
POIS_TRUTH = 1                                  # boot_pois_cases.TRUTHS[1] = (5, 1, 0.5)
NFIRST = 40                                     # the data sets per family that the test recomputes
FLAGS = (("degenerate", R.DEGENERATE), ("no_accel", R.NO_ACCEL), ("bad_denom", R.BAD_DENOM), ("no_replica", R.NO_REPLICA))
assert (BC.NREP, BC.LEVEL, BPC.NREP, BPC.LEVEL) == (NREP, LEVEL, NREP, LEVEL)


def data(family):
    return BC.problems() if family == "decay" else BPC.problems(POIS_TRUTH)


def _decay_sigma(t, yp, x):
    """boot_cases.gauss_interval's sigma: sqrt of the diagonal of s^2 (J^T J)^-1 at x."""
    r = BC.model(x, t)[0] - yp
    J = BC.jacobian(x, t)
    return np.sqrt(np.diag((r @ r) / (BC.M - 3) * np.linalg.inv(J.T @ J)))


def _sigma_or_nan(fn, *args):
    try:
        with np.errstate(all="ignore"):
            return fn(*args)
    except np.linalg.LinAlgError:
        return np.full(3, np.nan)


def _pois_fit(oracle, t, yp, x0, mask):
    fcn, jac = PC.callbacks(t, yp, "poisson", True, w=mask)
    with np.errstate(all="ignore"):
        rc, x, fv, ib = oracle.lm_solve(fcn, BPC.M, PC.N, np.array(x0, dtype=np.float64), jac=jac, opts=oracle.default_options())
    return x if rc == 0 and np.isfinite(x).all() and np.isfinite(fv).all() else None


def refits(oracle, family, p, dat):
    """(truth, x, sigma [3], xs, sigs [NREP, 1, 3], xjack [m, 1, 3]) of data set p: the fit, the refits of its replicas with
    their own sigma, and the delete-one refits; a failed refit is a NaN row."""
    if family == "decay":
        t, y, xt = dat
        m, one = BC.M, np.ones(BC.M)
        x = BC.fit(oracle, t, y[p], one, xt[p])
        sg = _decay_sigma(t, y[p], x)
        mu = BC.model(x, t)[0]
        replica = lambda b: B.resample_one(B.RESIDUAL, BC.BOOT_SEED, p, b, mu, y[p], None, True)[0]
        fit = lambda ys, w: BC.fit(oracle, t, ys, w, x)
        sigma = lambda ys, xr: _decay_sigma(t, ys, xr)
    else:
        t, y, xt, x0 = dat
        t, m = t[p], BPC.M
        x = BPC.fit(oracle, t, y[p], x0[p])
        assert x is not None, p
        sg = BPC.fisher_sigma(t, y[p], x)
        mu = CR.model(CR.EXPDECAY, PC.K, PC.B, x, t)
        ystar, bad = BP.poisson(BPC.BOOT_SEED, mu[None], y[p][None], None, NREP, prob0=p)
        assert bad[0] == 0, p
        replica = lambda b: ystar[b, 0]
        fit = lambda ys, w: BPC.fit(oracle, t, ys, x) if w is None else _pois_fit(oracle, t, ys, x, w)
        sigma = lambda ys, xr: BPC.fisher_sigma(t, ys, xr)
    xs, sigs, xjack = np.full((NREP, 1, 3), np.nan), np.full((NREP, 1, 3), np.nan), np.full((m, 1, 3), np.nan)
    for b in range(NREP):
        ys = replica(b)
        got = fit(ys, None if family == "poisson" else np.ones(m))
        if got is not None:
            xs[b, 0], sigs[b, 0] = got, _sigma_or_nan(sigma, ys, got)
    wj = R.jackknife(None, 1, m)
    for i in range(m):
        got = fit(y[p], wj[i, 0])
        if got is not None:
            xjack[i, 0] = got
    return xt[p], x, sg, xs, sigs, xjack


def one(oracle, family, p, dat=None):
    """Data set p of a family: per row and parameter `cover` -- "1" the interval holds the truth, "a" the truth lies above it,
    "b" below it, "n" the interval is a NaN -- and `half`, (hi - lo)/2 in units of sigma; and the counts."""
    xt, x, sg, xs, sigs, xjack = refits(oracle, family, p, dat or data(family))
    iv = {"gauss": (x - 1.96 * sg, x + 1.96 * sg)}
    lo, hi, _, _, nvalid = B.summary(xs, LEVEL)
    iv["percentile"] = (lo[0], hi[0])
    lo, hi, nvalid_t = R.student(xs, sigs, x[None], sg[None], LEVEL)
    iv["student"] = (lo[0], hi[0])
    accel, njack = R.accel(xjack)
    lo, hi, _, _, _, flags, _ = R.bca(xs, x[None], accel, LEVEL)
    iv["bca"] = (lo[0], hi[0])
    out = {"cover": {}, "half": {}, "nvalid": int(nvalid[0]), "nvalid_t": [int(v) for v in nvalid_t[0]], "njack": int(njack[0]),
           "flags": [int(v) for v in flags[0]]}
    for r in ROWS:
        lo, hi = iv[r]
        out["cover"][r] = "".join("n" if not (np.isfinite(lo[j]) and np.isfinite(hi[j])) else "1" if lo[j] <= xt[j] <= hi[j] else
                                  "a" if xt[j] > hi[j] else "b" for j in range(3))
        out["half"][r] = [float((hi[j] - lo[j]) / 2.0 / sg[j]).hex() for j in range(3)]
    return out


def summarise(res):
    """The recorded form of a family's results (a list of one()'s dicts, in data-set order): the per-data-set records by row
    and parameter -- the half-widths of the first NFIRST data sets only, which a test recomputes; of all of them their median
    --, and what the README's table shows."""
    n = len(res)
    out = {"cover": {r: {q: "".join(d["cover"][r][j] for d in res) for j, q in enumerate(PARAMS)} for r in ROWS},
           "half_first": {r: {q: [d["half"][r][j] for d in res[:NFIRST]] for j, q in enumerate(PARAMS)} for r in ROWS},
           "median_half": {r: {q: float(np.nanmedian([float.fromhex(d["half"][r][j]) for d in res])) for j, q in enumerate(PARAMS)}
                           for r in ROWS},
           "nvalid": [d["nvalid"] for d in res], "nvalid_t": [d["nvalid_t"] for d in res], "njack": [d["njack"] for d in res],
           "flags": [d["flags"] for d in res]}
    out.update(table(out, n))
    return out


def table(rec, n):
    """coverage, its standard error, the shares of data sets with the truth above / below the interval, the minimum counts and the count of each BCa flag -- from a family's per-data-set records."""
    t = {"coverage": {}, "stderr": {}, "above": {}, "below": {}}
    for r in ROWS:
        cov = {q: s.count("1") / n for q, s in rec["cover"][r].items()}
        t["coverage"][r] = cov
        t["stderr"][r] = {q: math.sqrt(c * (1.0 - c) / n) for q, c in cov.items()}
        t["above"][r] = {q: s.count("a") / n for q, s in rec["cover"][r].items()}
        t["below"][r] = {q: s.count("b") / n for q, s in rec["cover"][r].items()}
    t["min_valid"] = min(rec["nvalid"])
    t["min_valid_t"] = min(min(v) for v in rec["nvalid_t"])
    t["min_jack"] = min(rec["njack"])
    t["flag_count"] = {name: {q: sum(1 for f in rec["flags"] if f[j] & bit) for j, q in enumerate(PARAMS)} for name, bit in FLAGS}
    return t


def _worker(job):
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import pyoracle
    pyoracle.lib()
    return one(pyoracle, *job)


def record(processes=1):
    jobs = [(f, p) for f in FAMILIES for p in range(NDATA[f])]
    if processes > 1:
        import multiprocessing
        with multiprocessing.Pool(processes) as pool:
            res = pool.map(_worker, jobs, chunksize=2)
    else:
        res = [_worker(j) for j in jobs]
    out = {"nrep": NREP, "level": LEVEL, "rows": list(ROWS), "families": {
        "decay": {"model": "a*exp(-k*t)+c, t in [0, 1], k in [0.4, 0.9], Gaussian noise 0.05: the data of boot_study.json", "ndata": BC.NDATA,
                  "m": BC.M, "kind": "residual", "boot_seed": BC.BOOT_SEED},
        "poisson": {"model": "a*exp(-k*t)+c, t in [0, 4], 64 bins, Poisson counts: the data of boot_pois_study.json", "ndata": BPC.NDATA,
                    "m": BPC.M, "truth": list(BPC.TRUTHS[POIS_TRUTH]), "boot_seed": BPC.BOOT_SEED}}}
    k = 0
    for f in FAMILIES:
        out["families"][f].update(summarise(res[k:k + NDATA[f]]))
        k += NDATA[f]
    with open(STUDY_GOLDEN, "w") as fh:
        fh.write(_dump(out, 0) + "\n")
    return out


def _dump(v, depth):
    """JSON with a line per entry down to the families' fields and everything below on its line: a file a diff can show."""
    if isinstance(v, dict) and depth < 3:
        pad = " " * (depth + 1)
        return "{\n" + ",\n".join(pad + json.dumps(k) + ": " + _dump(x, depth + 1) for k, x in v.items()) + "\n" + " " * depth + "}"
    return json.dumps(v, separators=(",", ":"))


if __name__ == "__main__":
    import sys
    rec = record(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
    for f in FAMILIES:
        print(f, json.dumps({k: rec["families"][f][k] for k in ("coverage", "stderr", "above", "below", "median_half", "min_valid",
                                                              "min_valid_t", "min_jack", "flag_count")}, indent=1))
