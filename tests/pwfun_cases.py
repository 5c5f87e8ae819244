"""The formulas and the seeded problem generators of the piecewise-model tests (tests/test_pwfun_cpu.py,
tests/test_gpu_pwfun.py, profiles/scripts/pwfun_rate.py): pow, atan2, min, max and where.  Every predicate here (b > a,
b < a, c >= 0) compares values that exact operations make of data and parameters, so the device and numpy select alike in
every row and no row is excluded.  Test infrastructure, not part of the product."""
import json
import os

import numpy as np

import pwfun_restatement as W

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (formula, vars, params, t range, (low, high) of every true parameter)
FORMULAS = {
    "hinge": ("b+s1*t+s2*max(t-t0,0)", "t", "b,s1,s2,t0", (0.0, 4.0), [(0.5, 1.5), (0.3, 0.9), (0.8, 1.6), (1.5, 2.5)]),
    "powerlaw": ("a*pow(t,b)+c", "t", "a,b,c", (0.0, 4.0), [(0.8, 1.6), (0.4, 1.8), (0.1, 0.4)]),
    "stretched": ("a*exp(-pow(t/tau,beta))+c", "t", "a,tau,beta,c", (0.0, 6.0), [(0.8, 1.6), (0.8, 1.6), (0.6, 1.4), (0.05, 0.2)]),
    # the forms the two above replace (rates; the recorded study)
    "hinge_abs": ("b+s1*t+s2*(0.5*((t-t0)+abs(t-t0)))", "t", "b,s1,s2,t0", (0.0, 4.0), [(0.5, 1.5), (0.3, 0.9), (0.8, 1.6), (1.5, 2.5)]),
    "powerlaw_explog": ("a*exp(b*log(t))+c", "t", "a,b,c", (0.0, 4.0), [(0.8, 1.6), (0.4, 1.8), (0.1, 0.4)]),
    # the phase of a damped resonance, continuous through w = w0 where atan(g*w/(w0^2-w^2)) jumps
    "phase": ("p0-atan2(g*w,w0*w0-w*w)", "w", "p0,g,w0", (0.2, 4.0), [(-0.2, 0.2), (0.2, 0.8), (1.5, 2.5)]),
    # ten parameters (two Jacobian passes at 8 columns a pass), exact operations and selections only: two hinges, a
    # saturating term and a ramp that starts at t3
    "piecewise": ("b+s1*max(t-t1,0)+s2*max(t-t2,0)+min(c1*t,c2)+where(t-t3,a1*(t-t3)+a2,0)", "t", "b,s1,t1,s2,t2,c1,c2,t3,a1,a2",
                  (0.0, 10.0), [(0.5, 1.5), (0.3, 0.9), (1.5, 2.5), (0.8, 1.6), (5.5, 6.5), (0.5, 1.0), (2.0, 4.0), (7.0, 8.0), (0.5, 1.0), (0.2, 0.4)]),
}
EXACT = ("hinge", "piecewise")
WITH_FUNCTIONS = ("powerlaw", "stretched", "phase")

# Presence patterns of a binary function's tangent -- on a only, on b only, on both -- and of WHERE's: (formula, params).
# The predicates compare exact values of t and the parameters.
PATTERNS = [(f"{f}({a},{b})", p) for f in ("pow", "atan2", "min", "max")
            for a, b, p in (("t+p", "1.5", "p"), ("t+0.5", "q", "q"), ("t+p", "q", "p,q"), ("p*t+0.25", "p+q", "p,q"))]
PATTERNS += [("where(t-p,2*t,q)", "p,q"), ("where(t-p,q*t,3)", "p,q"), ("where(t-p,1+t,2)", "p"), ("where(t-1.25,p*t,q-t)", "p,q"),
             ("where(p-t,q*q,q)", "p,q")]
PATTERN_X = {"p": 1.25, "q": 0.75}

NPROB, SEED, MAX_EVALS = 8, 2028, 500
# test_pwfun_cpu.py::test_fits_on_the_oracle: 64 problems of each, drawn from one generator in this order
FIT_SEED, FIT_NPROB = 2028, 64
FIT_CASES = (("hinge", 200), ("powerlaw", 64), ("stretched", 128))
# test_gpu_pwfun.py::test_recovery: 64 noisy power laws on the fit grid (t = 0 in it), Gaussian noise of standard deviation
# RECOVERY_NOISE.  RECOVERY_N: in how many of them the CPU oracle's fit has every parameter within 3 standard errors of its
# generating value (test_pwfun_cpu.py::test_recovery_seed_on_the_oracle asserts it); the device is held to RECOVERY_N - 4.
RECOVERY_SEED, RECOVERY_NOISE, RECOVERY_M, RECOVERY_NPROB, RECOVERY_N = 7, 0.01, 64, 64, 64


def compile_formula(name):
    import nonlin_amd as nl
    f, v, p = FORMULAS[name][:3]
    return nl.Expr(f, v, p)


def program(name):
    e = compile_formula(name)
    prog = e.program()
    e.close()
    return prog


def grid(name, m):
    """The fit grid: m points from end to end of the formula's range, t = 0 among them where the range starts there."""
    lo, hi = FORMULAS[name][3]
    return np.linspace(lo, hi, m)


def abscissae(name, m, nprob, rng):
    """t [1, nprob, m]: a jittered grid inside the formula's range."""
    lo, hi = FORMULAS[name][3]
    step = (hi - lo) / m
    t = np.tile(np.linspace(lo + 0.25 * step, hi - 0.25 * step, m), (nprob, 1)) + rng.uniform(-0.2, 0.2, (nprob, m)) * step
    return np.ascontiguousarray(t[None])


def problems(name, m, nprob=NPROB, seed=SEED, sigma=1e-3, spread=0.03, prog=None, zero=False):
    """nprob data sets of a formula on m rows, as specfun_cases.problems: prog, t [1, nprob, m], y [nprob, m], x_true,
    x0 [nprob, n].  Uniform noise, sigma times the largest value.  zero: the first abscissa of every problem is the range's
    start (t = 0)."""
    prog = prog or program(name)
    rng = np.random.default_rng(seed)
    box = np.array(FORMULAS[name][4])
    t = abscissae(name, m, nprob, rng)
    if zero:
        t[0, :, 0] = FORMULAS[name][3][0]
    xt = rng.uniform(box[:, 0], box[:, 1], (nprob, len(box)))
    y = np.empty((nprob, m))
    for p in range(nprob):
        y[p] = W.value(prog, xt[p], t[:, p])
        y[p] += sigma * np.abs(y[p]).max() * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + spread * rng.uniform(-1, 1, xt.shape))
    return prog, t, np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


def draw(name, t, rng, nprob, prog, sigma=1e-3, spread=0.03, gaussian=None):
    """nprob problems on the shared grid t from a running generator, per problem the truth first, then the noise, then the
    start: y [nprob, m], x_true, x0 [nprob, n]."""
    box = np.array(FORMULAS[name][4])
    m, n = len(t), len(box)
    y, xt, x0 = np.empty((nprob, m)), np.empty((nprob, n)), np.empty((nprob, n))
    for p in range(nprob):
        xt[p] = rng.uniform(box[:, 0], box[:, 1])
        y[p] = W.value(prog, xt[p], [t])
        y[p] += gaussian * rng.standard_normal(m) if gaussian is not None else sigma * np.abs(y[p]).max() * rng.uniform(-1, 1, m)
        x0[p] = xt[p] * (1.0 + spread * rng.uniform(-1, 1, n))
    return y, xt, x0


def fit_problems():
    """{name: (prog, t [m], y, x_true, x0)} of FIT_CASES, all drawn from np.random.default_rng(FIT_SEED) in that order."""
    rng = np.random.default_rng(FIT_SEED)
    out = {}
    for name, m in FIT_CASES:
        prog, t = program(name), grid(name, m)
        out[name] = (prog, t) + draw(name, t, rng, FIT_NPROB, prog)
    return out


def recovery_problems(prog=None):
    prog = prog or program("powerlaw")
    t = grid("powerlaw", RECOVERY_M)
    return (prog, t) + draw("powerlaw", t, np.random.default_rng(RECOVERY_SEED), RECOVERY_NPROB, prog, gaussian=RECOVERY_NOISE)


def oracle_fit(oracle, prog, t, y, x0, analytic, max_evals=MAX_EVALS):
    """One problem on the CPU oracle with the restatement as callback: (rc, x, fvec, ib)."""
    m, n = len(y), len(x0)
    fcn = lambda x, f: f.__setitem__(slice(None), W.residual(prog, x, [t], y))
    jac = (lambda x, J: J.__setitem__((slice(None), slice(None)), W.jacobian(prog, x, [t]))) if analytic else None
    return oracle.lm_solve(fcn, m, n, x0, jac=jac, opts=oracle.default_options(max_evals=max_evals))


def study(oracle):
    """The recorded study (tests/golden/pwfun_study.json): the power-law data of fit_problems fitted as a*pow(t,b)+c and as
    a*exp(b*log(t))+c with the analytic Jacobian, on the grid with its t = 0 row and without it.  Per (form, grid): how many
    of the 64 fits fail (rc != 0 or a non-finite x), and mean and standard deviation of b - b_true over those that do not."""
    prog, t, y, xt, x0 = fit_problems()["powerlaw"]
    out = {}
    for form in ("powerlaw", "powerlaw_explog"):
        fprog = prog if form == "powerlaw" else program(form)
        for rows, lo in (("with_t0", 0), ("without_t0", 1)):
            db, failed = [], 0
            for p in range(len(y)):
                rc, x, f, ib = oracle_fit(oracle, fprog, t[lo:], y[p][lo:], x0[p], True)
                if rc != 0 or not np.isfinite(x).all():
                    failed += 1
                else:
                    db.append(x[1] - xt[p][1])
            out[f"{form}/{rows}"] = {"failed": failed, "fitted": len(db), "b_bias": float(np.mean(db)) if db else None,
                                     "b_scatter": float(np.std(db)) if db else None}
    return out


def recorded_study():
    with open(os.path.join(HERE, "golden", "pwfun_study.json")) as fh:
        return json.load(fh)
