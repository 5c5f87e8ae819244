"""The formulas, the seeded problem generators and the fixture of the special-function tests (tests/test_specfun_cpu.py,
tests/test_gpu_specfun.py, profiles/scripts/specfun_rate.py).  Test infrastructure, not part of the product."""
import os

import numpy as np

import specfun_restatement as S

HERE = os.path.dirname(os.path.abspath(__file__))

# name: (formula, vars, params, t range, (low, high) of every true parameter).  VOIGT_ONLY: no library function -- the device
# gives the restatement's bits and the CPU oracle with the restatement as callback is the device's solve bit for bit.
FORMULAS = {
    "voigt1": ("a*voigt(t-mu,s,g)+c", "t", "a,mu,s,g,c", (0.0, 10.0), [(2.0, 4.0), (4.5, 5.5), (0.35, 0.6), (0.3, 0.55), (0.05, 0.2)]),
    "lorentz1": ("a/(1.0+((t-mu)/w)*((t-mu)/w))+c+0*q", "t", "a,mu,w,q,c", (0.0, 10.0),
                 [(2.0, 4.0), (4.5, 5.5), (0.35, 0.6), (0.3, 0.55), (0.05, 0.2)]),         # the same parameter count (rate comparison)
    "doublet": ("a1*voigt(t-m1,s1,g1)+a2*voigt(t-m2,s2,g2)+c", "t", "a1,m1,s1,g1,a2,m2,s2,g2,c", (0.0, 10.0),
                [(2.0, 4.0), (3.2, 3.8), (0.35, 0.6), (0.3, 0.55), (2.0, 4.0), (6.2, 6.8), (0.35, 0.6), (0.3, 0.55), (0.05, 0.2)]),
    # exponentially modified Gaussian: area a, rate k, written with erfcx so that it neither overflows nor cancels
    "emg": ("a*0.5*k*exp(-0.5*((t-mu)/s)^2)*erfcx((s*k-(t-mu)/s)/sqrt(2))+c", "t", "a,mu,s,k,c", (0.0, 10.0),
            [(2.0, 4.0), (3.0, 4.0), (0.3, 0.6), (0.6, 1.5), (0.05, 0.2)]),
    # an exponential decay seen through a Gaussian response of width s (the TCSPC closed form).  With erfcx it holds near the
    # rise and for wide responses, but exp(..) underflows while erfcx overflows once (t-t0)/s passes about 37: the range stops
    # at t = 6.  With erfc it holds down the whole tail (it is the form to fit a decay with).
    "decay_irf": ("0.5*a*exp(-0.5*((t-t0)/s)^2)*erfcx((k*s-(t-t0)/s)/sqrt(2))+b", "t", "a,k,t0,s,b", (0.0, 6.0),
                  [(50.0, 200.0), (0.4, 1.2), (1.5, 2.5), (0.2, 0.4), (1.0, 5.0)]),
    "decay_erfc": ("0.5*a*exp(-k*(t-t0))*exp(0.5*(k*s)^2)*erfc((k*s-(t-t0)/s)/sqrt(2))+b", "t", "a,k,t0,s,b", (0.0, 10.0),
                   [(50.0, 200.0), (0.4, 1.2), (1.5, 2.5), (0.15, 0.4), (1.0, 5.0)]),
    "edge": ("a*0.5*(1+erf((t-t0)/(s*sqrt(2))))+b*erfc((t-t1)/w)+c", "t", "a,t0,s,b,t1,w,c", (0.0, 10.0),
             [(0.8, 1.6), (2.5, 3.5), (0.3, 0.8), (0.3, 0.9), (6.5, 7.5), (0.5, 1.2), (0.05, 0.2)]),
}
VOIGT_ONLY = ("voigt1", "doublet")
WITH_FUNCTIONS = ("emg", "decay_irf", "decay_erfc", "edge")

# The seven presence patterns of VOIGT's tangent (which of x, sigma, gamma carry one) and a parameter that reaches two
# operands: (formula, params)
PATTERNS = [("voigt(t-mu,0.5,0.1)", "mu"), ("voigt(t,s,0.1)", "s"), ("voigt(t,0.5,g)", "g"), ("voigt(t-mu,s,0.1)", "mu,s"),
            ("voigt(t-mu,0.5,g)", "mu,g"), ("voigt(t,s,g)", "s,g"), ("voigt(t-mu,s,g)", "mu,s,g"), ("voigt(t-mu,s,0.5*s)", "mu,s")]
PATTERN_X = {"mu": 4.7, "s": 0.45, "g": 0.35}

NPROB, SEED, MAX_EVALS = 8, 2027, 500
# test_gpu_specfun.py::test_recovery: 64 noisy single peaks, m = 200, Gaussian noise of standard deviation RECOVERY_NOISE; with
# this seed the CPU oracle's fit has every parameter within 3 standard errors of its generating value in 64 of the 64
# problems (test_specfun_cpu.py::test_recovery_seed_on_the_oracle holds it to >= 60)
RECOVERY_SEED, RECOVERY_NOISE, RECOVERY_M, RECOVERY_NPROB = 7, 0.01, 200, 64

# |restatement - fixture|, the maxima measured on the committed fixture, rounded up in the third digit, and the bounds, 4 x each: the margin covers
# another sample, not another algorithm.  w: |dw|/|w|; the Voigt value over the peak value V(0; sigma, gamma); each partial
# over V(0)/sigma.
MEASURED = {"w": 1.28e-15, "v": 1.04e-15, "gx": 4.29e-14, "gs": 2.57e-11, "gg": 5.43e-14}
BOUND = {k: 4.0 * v for k, v in MEASURED.items()}

# ERF-family arguments the device functions are measured over: the fixture's (|a| <= 26, dense near 0)
_FIXTURE = None


def fixture():
    """tests/golden/specfun_reference.npz as a dict of arrays (tests/golden/make_specfun_reference.py made it)."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(os.path.join(HERE, "golden", "specfun_reference.npz")) as z:
            _FIXTURE = {k: z[k] for k in z.files}
        for v in _FIXTURE.values():
            v.setflags(write=False)
    return _FIXTURE


def compile_formula(name):
    import nonlin_amd as nl
    f, v, p = FORMULAS[name][:3]
    return nl.Expr(f, v, p)


def abscissae(name, m, nprob, rng):
    """t [1, nprob, m]: a jittered grid over the formula's range."""
    lo, hi = FORMULAS[name][3]
    step = (hi - lo) / m
    t = np.tile(np.linspace(lo + 0.25 * step, hi - 0.25 * step, m), (nprob, 1)) + rng.uniform(-0.2, 0.2, (nprob, m)) * step
    return np.ascontiguousarray(t[None])


def problems(name, m, nprob=NPROB, seed=SEED, sigma=1e-3, spread=0.03, prog=None, gaussian=None):
    """nprob data sets of a formula on m rows: prog, t [1, nprob, m], y [nprob, m], x_true, x0 [nprob, n].  Noise: uniform,
    sigma times the largest value -- or, with gaussian, normal of that standard deviation."""
    if prog is None:
        e = compile_formula(name)
        prog = e.program()
        e.close()
    rng = np.random.default_rng(seed)
    box = np.array(FORMULAS[name][4])
    t = abscissae(name, m, nprob, rng)
    xt = rng.uniform(box[:, 0], box[:, 1], (nprob, len(box)))
    y = np.empty((nprob, m))
    for p in range(nprob):
        y[p] = S.value(prog, xt[p], t[:, p])
        y[p] += gaussian * rng.standard_normal(m) if gaussian is not None else sigma * np.abs(y[p]).max() * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + spread * rng.uniform(-1, 1, xt.shape))
    return prog, t, np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)
