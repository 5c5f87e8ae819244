"""The formulas, the seeded problem generators, the fixture and the recorded figures of the tests of j0, j1, i0e, i1e,
lgamma, expm1 and log1p (tests/test_specfun2_cpu.py, tests/test_gpu_specfun2.py, profiles/scripts/specfun2_rate.py).  Test
infrastructure, not part of the product."""
import os

import numpy as np

import specfun2_restatement as S2

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -52

# name: (formula, vars, params, t range, (low, high) of every true parameter)
FORMULAS = {
    # the Airy pattern of a circular aperture; the grids start off the axis (2 j1(u)/u is 0/0 at u = 0)
    "airy": ("a*(2*j1(k*r)/(k*r))^2+b", "r", "a,k,b", (0.05, 10.0), [(2.0, 4.0), (0.8, 1.6), (0.05, 0.2)]),
    "airy_def": ("u = k*r; a*(2*j1(u)/u)^2+b", "r", "a,k,b", (0.05, 10.0), [(2.0, 4.0), (0.8, 1.6), (0.05, 0.2)]),
    "vonmises": ("a*exp(kappa*(cos(t-mu)-1))/(2*pi*i0e(kappa))", "t", "a,kappa,mu", (-3.14, 3.14), [(2.0, 4.0), (1.0, 4.0), (-0.5, 0.5)]),
    "gammapdf": ("n*exp((k-1)*log(t)-t/th-lgamma(k)-k*log(th))", "t", "n,k,th", (0.1, 12.0), [(200.0, 400.0), (2.0, 4.0), (0.8, 1.6)]),
    "planck": ("a*t^3/expm1(b*t)+c*log1p(d*t)", "t", "a,b,c,d", (0.05, 8.0), [(2.0, 4.0), (0.8, 1.6), (0.5, 1.0), (0.2, 0.6)]),
    # i0e and i1e only: the bit-exact class.  toy: a Rician-like mixture; bessel10: ten parameters (two Jacobian passes at 8
    # columns a pass), arguments of both signs, through 0 and on both sides of the switch at |a| = 8
    "toy": ("a*i0e(k*t)+b*i1e(k*t)+c", "t", "a,k,b,c", (0.1, 10.0), [(2.0, 4.0), (0.5, 2.0), (1.0, 2.0), (0.05, 0.2)]),
    "bessel10": ("a1*i0e(k1*(t-m1))+a2*i1e(k2*(t-m2))+a3*i0e(k3*t)*i1e(t-m3)+c", "t", "a1,k1,m1,a2,k2,m2,a3,k3,m3,c", (0.0, 10.0),
                 [(2.0, 4.0), (1.5, 2.5), (4.0, 6.0), (1.0, 2.0), (1.5, 2.5), (2.0, 3.0), (0.5, 1.5), (0.5, 1.5), (6.0, 8.0), (0.05, 0.2)]),
    # twelve parameters, every library function of the set
    "mixed": ("a*j0(k*(t-t0))+b*j1(q*t)+n*exp((s-1)*log(t)-t/th-lgamma(s)-s*log(th))+c*expm1(-d*t)+e*log1p(f*t)", "t",
              "a,k,t0,b,q,n,s,th,c,d,e,f", (0.1, 10.0),
              [(1.0, 2.0), (1.5, 2.5), (4.0, 6.0), (1.0, 2.0), (0.8, 1.6), (5.0, 10.0), (2.0, 4.0), (0.8, 1.6), (0.5, 1.0), (0.2, 0.6),
               (0.5, 1.0), (0.2, 0.6)]),
}
EXACT = ("toy", "bessel10")
WITH_FUNCTIONS = ("airy", "vonmises", "gammapdf", "planck", "mixed")

NPROB, SEED, MAX_EVALS = 8, 2029, 500

# |restatement - fixture| of the stated arithmetic, the maxima measured on the committed fixture by
# test_specfun2_cpu.py::test_restatement_against_the_fixture, rounded up in the third digit, and the bounds, 4 x each (the
# margin of specfun_cases.py: another sample, not another algorithm).  i0e, i1e: |dv|/|v| (3.50 and 1.67 ulp; the condition
# is 8 ulp; the fixture samples [-8, 8] uniformly as well, where the series' rounding error peaks); digamma: |dv|/max(|v|, 1) (7.0 ulp: the up to ten reciprocals of the recurrence).  The restatement's bits are
# the device's for i0e and i1e, so these are the device's accuracy.
MEASURED = {"i0e": 7.78e-16, "i1e": 3.71e-16, "digamma": 1.56e-15}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}
CONDITION = 8.0 * U                                                   # i0e, i1e: the loosest figure accepted for a stated function

# test_gpu_specfun2.py::test_fits_against_oracle: the device's x against the CPU oracle's with the restatement as callback.
# FIT_SHIFT: the largest |dx|/max(|x|, 1) by which the oracle's x moves when every library function of the restated formula
# is moved by U_F + NUMPY_F ulp of its scale, either way (fit_shift below, the measured maxima rounded up in the third digit;
# test_specfun2_cpu.py::test_fit_tolerance holds the record to the measurement); FIT_TOL = 4 x that.  The wrapped cases --
# the projected Airy fit, the gamma pdf as a Poisson likelihood -- are measured with per-result noise as well.
# SHIFT_FLOOR: two converged solves of one problem differ by a few ulp of x whatever is shifted (a solve stops on a small
# relative step, not at a fixed point), so a measured shift below 16 ulp is that noise and is recorded as 16 ulp.  The gamma
# pdf's Poisson fit is there (8.0e-16 measured: the shifts average out over the 129 counts).  Its comparison on the device
# differs from the oracle's by the deviance wrapper's own log and log1p as well, which fit_shift does not move: the tolerance
# the Poisson tests take from their perturbation study for exactly that (pois_cases.recorded_tolerance) is added.
FIT_M, FIT_NPROB = 129, 8
SHIFT_FLOOR = 16.0 * U
FIT_SHIFT = {"airy": 3.14e-10, "vonmises": 1.53e-10, "airy/sep": 3.62e-10, "gammapdf/pois": SHIFT_FLOOR}
FIT_TOL = {k: 4.0 * v for k, v in FIT_SHIFT.items()}


def _add_the_wrappers_own_functions():
    import pois_cases
    FIT_TOL["gammapdf/pois"] += pois_cases.recorded_tolerance(True)


_add_the_wrappers_own_functions()

# test_gpu_specfun2.py::test_recovery: 64 noisy data sets of each, Gaussian noise; RECOVERY_N: in how many of them the CPU
# oracle's fit has every parameter within 3 standard errors of its generating value
# (test_specfun2_cpu.py::test_recovery_seed_on_the_oracle asserts the count); the device is held to 4 fewer.
RECOVERY = {"airy": dict(seed=7, noise=0.02, m=128, nprob=64), "gammapdf": dict(seed=7, noise=1.0, m=128, nprob=64)}
RECOVERY_N = {"airy": 64, "gammapdf": 64}

_FIXTURE = None


def fixture():
    """tests/golden/specfun2_reference.npz as a dict of read-only arrays (tests/golden/make_specfun2_reference.py made it)."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(os.path.join(HERE, "golden", "specfun2_reference.npz")) as z:
            _FIXTURE = {k: z[k] for k in z.files}
        for v in _FIXTURE.values():
            v.setflags(write=False)
    return _FIXTURE


# function: (arguments' key, the scale its error is measured against, of (a, reference))
MEASURES = {
    "j0": ("j_a", lambda a, v: S2.envelope(a)), "j1": ("j_a", lambda a, v: S2.envelope(a)),
    "i0e": ("ie_a", lambda a, v: np.abs(v)), "i1e": ("ie_a", lambda a, v: np.abs(v)),
    "lgamma": ("lg_a", lambda a, v: np.maximum(np.abs(v), 1.0)), "digamma": ("lg_a", lambda a, v: np.maximum(np.abs(v), 1.0)),
    "expm1": ("em_a", lambda a, v: np.abs(v)), "log1p": ("lp_a", lambda a, v: np.abs(v)),
}


def error(name, got):
    """(the largest error of got against the fixture in the function's measure, the argument it is at).  A reference of 0
    (i1e(0)) must be met exactly and is left out of the quotient."""
    fx = fixture()
    key, scale = MEASURES[name]
    a, ref = fx[key], fx[name]
    got = np.asarray(got, dtype=np.float64)
    zero = ref == 0.0
    assert (got[zero] == 0.0).all(), name
    s = scale(a, ref)
    err = np.where(zero, 0.0, np.abs(got - ref) / np.where(zero, 1.0, s))
    k = int(np.argmax(err))
    return float(err[k]), float(a[k])


def compile_formula(name):
    import nonlin_amd as nl
    f, v, p = FORMULAS[name][:3]
    return nl.Expr(f, v, p)


def program(name):
    e = compile_formula(name)
    prog = e.program()
    e.close()
    return prog


def abscissae(name, m, nprob, rng):
    """t [1, nprob, m]: a jittered grid inside the formula's range."""
    lo, hi = FORMULAS[name][3]
    step = (hi - lo) / m
    t = np.tile(np.linspace(lo + 0.25 * step, hi - 0.25 * step, m), (nprob, 1)) + rng.uniform(-0.2, 0.2, (nprob, m)) * step
    return np.ascontiguousarray(t[None])


def problems(name, m, nprob=NPROB, seed=SEED, sigma=1e-3, spread=0.03, prog=None, gaussian=None):
    """nprob data sets of a formula on m rows, as specfun_cases.problems: prog, t [1, nprob, m], y [nprob, m], x_true,
    x0 [nprob, n].  Noise: uniform, sigma times the largest value -- or, with gaussian, normal of that standard deviation."""
    prog = prog or program(name)
    rng = np.random.default_rng(seed)
    box = np.array(FORMULAS[name][4])
    t = abscissae(name, m, nprob, rng)
    xt = rng.uniform(box[:, 0], box[:, 1], (nprob, len(box)))
    y = np.empty((nprob, m))
    for p in range(nprob):
        y[p] = S2.value(prog, xt[p], t[:, p])
        y[p] += gaussian * rng.standard_normal(m) if gaussian is not None else sigma * np.abs(y[p]).max() * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + spread * rng.uniform(-1, 1, xt.shape))
    return prog, t, np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


def recovery_problems(name, prog=None):
    r = RECOVERY[name]
    return problems(name, r["m"], nprob=r["nprob"], seed=r["seed"], prog=prog, gaussian=r["noise"])


def poisson_problems(prog=None):
    """The fit problems of the gamma-pdf model with Poisson counts in place of the noisy values."""
    prog, t, y, xt, x0 = problems("gammapdf", FIT_M, nprob=FIT_NPROB, prog=prog)
    rng = np.random.default_rng(SEED + 1)
    y = np.stack([rng.poisson(S2.value(prog, xt[p], t[:, p])) for p in range(FIT_NPROB)]).astype(np.float64)
    return prog, t, np.ascontiguousarray(y), xt, x0


def wrapped_callbacks(prog, tv, y, kind=None, analytic=True, F=S2._Plain):
    """(fcn, jac) for the oracle's solvers: the restated formula (function table F) alone, or inside the restated projection
    of the Airy pattern's a and b (kind "sep": tests/sep_restatement.py) or the restated Poisson deviance (kind "pois":
    tests/pois_restatement.py, no mask, the default floor)."""
    res = lambda x: S2.residual(prog, x, tv, y, F=F)
    jac = lambda x: S2.jacobian(prog, x, tv, F=F)
    if kind == "sep":
        import sep_cases
        return sep_cases.oracle_callbacks(res, jac, 3, [0, 2], analytic)
    if kind == "pois":
        import pois_restatement as PR
        f = lambda x, out: out.__setitem__(slice(None), PR.residual(y, None, PR.MU_FLOOR, res(x)))
        j = lambda x, J: J.__setitem__((slice(None), slice(None)), PR.jacobian(y, None, PR.MU_FLOOR, res(x), jac(x)))
    else:
        f = lambda x, out: out.__setitem__(slice(None), res(x))
        j = lambda x, J: J.__setitem__((slice(None), slice(None)), jac(x))
    return f, (j if analytic else None)


def oracle_fit(oracle, prog, tv, y, x0, analytic, max_evals=MAX_EVALS, F=S2._Plain, kind=None):
    """One problem on the CPU oracle with the restatement as callback: (rc, x, fvec, ib)."""
    f, j = wrapped_callbacks(prog, tv, y, kind, analytic, F)
    return oracle.lm_solve(f, len(y), len(x0), x0, jac=j, opts=oracle.default_options(max_evals=max_evals))


def standard_errors(prog, x, tv, y):
    m, n = len(y), len(x)
    f, J = S2.residual(prog, x, tv, y), S2.jacobian(prog, x, tv)
    return np.sqrt(np.diag(np.linalg.inv(J.T @ J)) * (f @ f) / (m - n))


def shifted(sign, rng=None):
    """The restatement's function table with every library function moved by (U_F + NUMPY_F) ulp of its scale, up (+1) or
    down (-1): the distance the device's function may be from this file's.  With rng, every result is moved by its own
    uniform draw from that interval instead (the model of pois_cases._ulp_noise).  i0e, i1e and the exact operations stay."""
    P = S2._Plain

    def k(f, v):
        s = sign if rng is None else rng.uniform(-1.0, 1.0, np.shape(v))
        return s * (S2.U_F[f] + S2.NUMPY_F.get(f, 1)) * U

    def rel(name, f):
        def g(a, *r):
            v = f(a, *r)
            return v * (1.0 + k(name, v))
        return staticmethod(g)

    def scaled(name, f, scale):
        def g(a):
            v = f(a)
            return v + k(name, v) * scale(a, v)
        return staticmethod(g)

    class _Shifted(P):
        exp, log, sin, cos = rel("exp", P.exp), rel("log", P.log), rel("sin", P.sin), rel("cos", P.cos)
        expm1, log1p = rel("expm1", P.expm1), rel("log1p", P.log1p)
        j0 = scaled("j0", P.j0, lambda a, v: S2.envelope(a))
        j1 = scaled("j1", P.j1, lambda a, v: S2.envelope(a))
        lgamma = scaled("lgamma", P.lgamma, lambda a, v: np.maximum(np.abs(v), 1.0))
    return _Shifted


def fit_shift(oracle, case, analytic=True):
    """The largest |dx|/max(|x|, 1) over the FIT_NPROB problems of a fit case and the shifts: up and down for "airy" and
    "vonmises"; for the wrapped cases "airy/sep" and "gammapdf/pois", whose solves converge past a uniform shift's reach,
    also two seeded draws of per-result noise."""
    name, kind = (case.split("/") + [None])[:2]
    prog, t, y, xt, x0 = poisson_problems() if kind == "pois" else problems(name, FIT_M, nprob=FIT_NPROB)
    if kind == "sep":
        x0 = np.ascontiguousarray(x0[:, [1]])
    tables = [shifted(1.0), shifted(-1.0)] + ([shifted(0.0, np.random.default_rng(s)) for s in (1, 2)] if kind else [])
    worst = 0.0
    for p in range(FIT_NPROB):
        rc, x, f, ib = oracle_fit(oracle, prog, t[:, p], y[p], x0[p], analytic, kind=kind)
        assert rc == 0, (case, p, rc)
        for F in tables:
            rs, xs, fs, ibs = oracle_fit(oracle, prog, t[:, p], y[p], x0[p], analytic, F=F, kind=kind)
            assert rs == 0, (case, p, rs)
            worst = max(worst, float((np.abs(xs - x) / np.maximum(np.abs(x), 1.0)).max()))
    return worst
