"""What the tests of the profile-likelihood intervals share: the two families of the study -- Michaelis-Menten curves
vmax*s/(km+s) on 16 points with Gaussian noise of two sizes, fitted by least squares, and the photon-counting decays of the
Poisson bootstrap study (boot_pois_cases.problems), fitted with the deviance --, each data set's fit on the CPU oracle's LM, its
Gaussian interval x +- sqrt(crit)*sigma and its profile interval by tests/profile_restatement.py over the same solver; the
synthetic costs of the step tests; and the golden file's name.  Run as a script it records tests/golden/profile_study.json
(`python tests/profile_cases.py [processes]`).  Test infrastructure, not part of the product."""
import json
import math
import os

import numpy as np

import boot_pois_cases as BC
import curve_restatement as R
import expr_restatement as ER
import pois_cases as PC
import pois_restatement as PO
import profile_restatement as PR
import starts_restatement as S

HERE = os.path.dirname(os.path.abspath(__file__))
STUDY_GOLDEN = os.path.join(HERE, "golden", "profile_study.json")
LEVEL = 0.95
CRIT = PR.crit_of(LEVEL)
TOL, XTOL, MAX_EXPAND, MAXIT = 0.01, 1e-3, 8, 30
# Michaelis-Menten
MM_FORMULA, MM_VARS, MM_PARAMS = "vmax*s/(km+s)", ("s",), ("vmax", "km")
MM_M, MM_N, MM_TRUTH, MM_SIGMAS, MM_NDATA, MM_SEED = 16, 2, (10.0, 4.0), (0.3, 0.15), 2000, 20261021
NGPU = 64                                       # the first data sets of a family: what tests/test_gpu_profile.py repeats on the device
CHECK = (0, 1, 150, 299)                        # the data sets tests/test_profile_cpu.py recomputes to the recorded bits
ROWS = ("gauss", "profile")
FAMILIES = [("mm", k) for k in range(len(MM_SIGMAS))] + [("decay", k) for k in range(len(BC.TRUTHS))]


def mm_expr():
    import nonlin_amd as nl
    return nl.Expr(MM_FORMULA, MM_VARS, MM_PARAMS)


def mm_problems(si, ndata=MM_NDATA):
    """s [MM_M], y [ndata, MM_M], x0 [ndata, 2] (the truth) of noise size MM_SIGMAS[si]."""
    rng = np.random.default_rng(MM_SEED + si)
    s = np.linspace(0.25, 4.0, MM_M)
    mu = MM_TRUTH[0] * s / (MM_TRUTH[1] + s)
    y = mu[None, :] + MM_SIGMAS[si] * rng.standard_normal((ndata, MM_M))
    return s, np.ascontiguousarray(y), np.tile(np.array(MM_TRUTH), (ndata, 1))


def mm_callbacks(prog, s, y):
    """residual(p, full), jacobian(p, full) of the data sets y [nprob, m] for profile_restatement.oracle_solve."""
    tv = [s]
    return (lambda p, full: ER.residual(prog, full, tv, y[p])), (lambda p, full: ER.jacobian(prog, full, tv))


def decay_callbacks(t, y):
    """The same for the deviance residuals of the counts y [nprob, m] at t [nprob, m]."""
    kd, f = R.EXPDECAY, PO.MU_FLOOR
    res = lambda p, full: PO.residual(y[p], None, f, R.residual(kd, PC.K, PC.B, full, t[p], y[p]))
    jac = lambda p, full: PO.jacobian(y[p], None, f, R.residual(kd, PC.K, PC.B, full, t[p], y[p]), R.jacobian(kd, PC.K, PC.B, full, t[p]))
    return res, jac


def family(fam, prog=None):
    """(m, N, truth, residual, jacobian, x0 [ndata, N], scaled) of a family of FAMILIES."""
    kind, k = fam
    if kind == "mm":
        s, y, x0 = mm_problems(k)
        res, jac = mm_callbacks(prog if prog is not None else mm_expr().program(), s, y)
        return MM_M, MM_N, np.array(MM_TRUTH), res, jac, x0, True
    t, y, xt, x0 = BC.problems(k)
    res, jac = decay_callbacks(t, y)
    return PC.M, PC.N, np.array(BC.TRUTHS[k]), res, jac, x0, False


def fit(oracle, m, N, res, jac, p, x0):
    """The oracle's LM on problem p from x0 (analytic Jacobian, default options): (x, fvec, sigma), sigma from s^2 (J^T J)^-1
    with s^2 = sum fvec^2 / (m - N) when scaled, from (J^T J)^-1 otherwise -- or None when the fit did not end with status 0."""
    def f(x, out):
        out[:] = res(p, x)

    def j(x, J):
        J[:, :] = jac(p, x)
    with np.errstate(all="ignore"):
        rc, x, fv, ib = oracle.lm_solve(f, m, N, np.array(x0, dtype=np.float64), jac=j, opts=oracle.default_options())
    if rc != 0 or not (np.isfinite(x).all() and np.isfinite(fv).all()):
        return None
    return x, fv


def sigma_of(jac, p, x, fv, m, N, scaled):
    J = jac(p, x)
    cov = np.linalg.inv(J.T @ J)
    if scaled:
        cov = cov * (float(fv @ fv) / (m - N))
    return np.sqrt(np.diag(cov))


def one(oracle, fam, p, data=None):
    """Data set p of a family: x, sigma, the profile's lo, hi, flags, nev."""
    m, N, truth, res, jac, x0, scaled = data or family(fam)
    got = fit(oracle, m, N, res, jac, p, x0[p])
    assert got is not None, (fam, p)
    x, fv = got
    sg = sigma_of(jac, p, x, fv, m, N, scaled)
    solve = PR.oracle_solve(oracle, m, N, lambda _, full: res(p, full), lambda _, full: jac(p, full))
    lo, hi, flags, nev, _ = PR.drive(x[None], sg[None], S.cost(fv[None]), m, solve, CRIT, TOL, XTOL, MAX_EXPAND, MAXIT, scaled=scaled)
    return {"x": x.tolist(), "sigma": sg.tolist(), "lo": lo[0].tolist(), "hi": hi[0].tolist(), "flags": flags[0].tolist(), "nev": nev[0].tolist()}


def _worker(job):
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import pyoracle
    pyoracle.lib()
    fam, p0, p1 = job
    data = family(fam)
    return [one(pyoracle, fam, p, data) for p in range(p0, p1)]


def _hex(v):
    return [float(a).hex() for a in v]


def summarise(fam, res):
    """The recorded form of one family's results (a list of one()'s dicts, in data-set order)."""
    truth = np.array(MM_TRUTH if fam[0] == "mm" else BC.TRUTHS[fam[1]])
    names = MM_PARAMS if fam[0] == "mm" else PC.PARAMS
    n, z = len(res), math.sqrt(CRIT)
    x, sg, lo, hi = (np.array([d[k] for d in res], dtype=np.float64) for k in ("x", "sigma", "lo", "hi"))
    flags, nev = np.array([d["flags"] for d in res]), np.array([d["nev"] for d in res])
    ends = {"gauss": (x - z * sg, x + z * sg), "profile": (lo, hi)}
    out = {"family": list(fam), "ndata": n, "params": list(names), "truth": truth.tolist()}
    for r in ROWS:
        a, b = ends[r]
        with np.errstate(invalid="ignore"):
            below, above = truth[None, :] < a, truth[None, :] > b          # (a NaN end compares false: it counts as covering)
        # per parameter, per data set: 'c' covered, 'a' the truth above the interval, 'b' below it
        marks = {q: "".join("a" if above[d, j] else "b" if below[d, j] else "c" for d in range(n)) for j, q in enumerate(names)}
        out[r] = {"marks": marks}
        for key, ch in (("covers", "c"), ("truth_above", "a"), ("truth_below", "b")):
            out[r][key] = {q: s.count(ch) / n for q, s in marks.items()}
            out[r][key + "_stderr"] = {q: math.sqrt(v * (1.0 - v) / n) for q, v in out[r][key].items()}
    with np.errstate(invalid="ignore"):
        dn, up = (x - lo) / sg, (hi - x) / sg
    fin = lambda v: v[np.isfinite(v)]
    out["median_halfwidth_sigma"] = {q: {"below": float(np.median(fin(dn[:, j]))), "above": float(np.median(fin(up[:, j])))}
                                     for j, q in enumerate(names)}
    out["mean_refits_per_end"] = float(nev.mean())
    out["flag_counts"] = {PR_FLAG_NAMES[c & 15] + ("+LOWER" if c & PR.LOWER else ""): int((flags == c).sum()) for c in sorted(set(flags.reshape(-1).tolist()))}
    out["check"] = {str(p): {k: _hex(res[p][k]) for k in ("x", "sigma", "lo", "hi")} | {k: res[p][k] for k in ("flags", "nev")}
                    for p in CHECK if p < n}
    return out


PR_FLAG_NAMES = ("OK", "OPEN", "OPEN_AT_BOUND", "ON_BOUND", "MAXIT", "FIT_FAILED", "NO_START", "NOT_FREE")


def ndata_of(fam):
    return MM_NDATA if fam[0] == "mm" else BC.NDATA


def record(processes=1, block=25):
    jobs = [(fam, p0, min(p0 + block, ndata_of(fam))) for fam in FAMILIES for p0 in range(0, ndata_of(fam), block)]
    if processes > 1:
        import multiprocessing
        with multiprocessing.Pool(processes) as pool:
            parts = pool.map(_worker, jobs, chunksize=1)
    else:
        parts = [_worker(j) for j in jobs]
    by = {fam: [] for fam in FAMILIES}
    for job, part in zip(jobs, parts):
        by[job[0]].extend(part)
    out = {"level": LEVEL, "crit": float(CRIT).hex(), "tol": TOL, "xtol": XTOL, "max_expand": MAX_EXPAND, "maxit": MAXIT,
           "mm": {"formula": MM_FORMULA, "m": MM_M, "s": [0.25, 4.0], "truth": list(MM_TRUTH), "sigmas": list(MM_SIGMAS), "seed": MM_SEED},
           "decay": {"model": "a*exp(-k*t)+c, t in [0, 4], 64 bins, Poisson counts", "truths": [list(v) for v in BC.TRUTHS], "seed": PC.SEED},
           "study": [summarise(fam, by[fam]) for fam in FAMILIES]}
    with open(STUDY_GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return out


# ---- the synthetic costs of the step tests (tests/test_profile_cpu.py, tests/test_gpu_profile.py) ----------------------------
def synthetic(nend_target, seed=5):
    """A batch of nprob problems of n = 2 parameters whose ends have synthetic costs: (x, sigma, C0, lower, upper, cost) with
    cost(e, theta, st) -> (cost, fail) of end e at theta.  The kinds cycle over the ends: quadratic wells of a different width
    per side (some found at once, some after doublings, some by the bracket), a flat cost (open), one behind a bound, a cost
    that fails every call, one that fails twice and then answers, and a cost below C0."""
    nprob = max(1, -(-nend_target // 4))
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.0, 3.0, (nprob, 2))
    sigma = rng.uniform(0.05, 0.2, (nprob, 2))
    C0 = rng.uniform(5.0, 20.0, nprob)
    nend = nprob * 4
    wfac = rng.choice([1.0, 0.55, 1.7, 6.0, 40.0], nend)       # the well's true width in units of the first step
    kinds = (np.arange(nend) // 4 + np.arange(nend)) % 8       # (every kind meets every (parameter, side) over the problems)
    calls = np.zeros(nend, dtype=np.int64)
    lower, upper = np.array([0.5, -np.inf]), np.array([np.inf, 3.5])
    x[0, 1] = upper[1]                                          # a fit on its bound: ON_BOUND above, an ordinary end below
    if nprob >= 2:
        sigma[-1, 0] = 0.0                                      # no standard error: NO_START on both sides

    def cost(e, theta, st):
        p = e // 4
        calls[e] += 1
        k = kinds[e]
        if k == 3:
            return C0[p], 0                                     # flat: the end is open
        if k == 5:
            return np.nan, 1                                    # every refit fails
        if k == 6 and calls[e] <= 2:
            return 1.0, 1                                       # two failures, then the well
        if k == 7:
            return C0[p] - 0.5 * st["delta"][p], 0              # below the fit's cost: never rises
        w = wfac[e] * st["width"][e]
        u = (theta - st["xhat"][e]) / w
        return C0[p] + st["delta"][p] * (u * u), 0
    return x, sigma, C0, lower, upper, cost, wfac, kinds


if __name__ == "__main__":
    import sys
    rec = record(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
    for s in rec["study"]:
        print(s["family"], json.dumps({k: s[k] for k in ("gauss", "profile", "median_halfwidth_sigma", "mean_refits_per_end", "flag_counts")
                                       if k not in ROWS} | {r: {k: v for k, v in s[r].items() if k != "marks"} for r in ROWS}, indent=1))
