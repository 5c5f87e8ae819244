"""The formulas, the seeded problem generator and the argument ranges of the formula-model tests (tests/test_expr_cpu.py,
tests/test_gpu_expr.py, profiles/scripts/expr_rate.py).  Test infrastructure, not part of the product."""
import numpy as np

import expr_restatement as R

# name: (formula, vars, params, t range, (low, high) of every true parameter).  EXP_FREE: no library function -- the device
# gives the restatement's bits and the CPU oracle with the restatement as callback is the device's solve bit for bit.
FORMULAS = {
    "mm": ("vmax*s/(km+s)", "s", "vmax,km", (0.05, 4.0), [(0.8, 1.6), (0.3, 0.9)]),
    "hill": ("vmax*s^3/(k^3+s^3)", "s", "vmax,k", (0.05, 3.0), [(0.8, 1.6), (0.8, 1.4)]),
    "lorentz2": ("0+a1/(1.0+((t-m1)/w1)*((t-m1)/w1))+a2/(1.0+((t-m2)/w2)*((t-m2)/w2))", "t", "a1,m1,w1,a2,m2,w2", (0.0, 1.0),
                 [(0.5, 1.5), (0.2, 0.3), (0.08, 0.16), (0.5, 1.5), (0.7, 0.8), (0.08, 0.16)]),
    "rational": ("(p0+p1*t+p2*t^2)/(1+q1*t+q2*t^2)", "t", "p0,p1,p2,q1,q2", (0.0, 2.0),
                 [(0.5, 1.5), (-0.5, 0.5), (0.3, 0.9), (0.2, 0.6), (0.3, 0.9)]),
    "roots": ("a*sqrt(abs(t-mu)+w^2)-b/(1+t^2)^-2+(-c)^3*t-+t/pi", "t", "a,mu,w,b,c", (0.0, 2.0),
              [(0.5, 1.5), (0.7, 1.3), (0.3, 0.6), (0.2, 0.6), (0.3, 0.9)]),
    "gauss2d": ("b+a*exp(-((x-x0)^2+(y-y0)^2)/(2*s^2))", "x,y", "a,x0,y0,s,b", (0.0, 14.0),
                [(50.0, 200.0), (5.5, 8.5), (5.5, 8.5), (1.2, 2.2), (5.0, 20.0)]),
    "dsine": ("a*exp(-g*t)*sin(2*pi*f*t+ph)+c", "t", "a,g,f,ph,c", (0.0, 4.0),
              [(0.8, 1.6), (0.3, 0.8), (1.0, 1.6), (-0.5, 0.5), (-0.3, 0.3)]),
    "logistic": ("L/(1+exp(-k*(t-t0)))", "t", "L,k,t0", (0.0, 10.0), [(0.8, 1.6), (0.8, 1.6), (4.0, 6.0)]),
    "stretched": ("a*(1+t/t0)^-1.5+c*t^0.7", "t", "a,t0,c", (0.05, 5.0), [(0.8, 1.6), (0.8, 1.6), (0.1, 0.4)]),
    "mixed": ("a*tanh(k*(t-1))+b*atan(t/w)+c*log(1+d*t)+cos(f*t)", "t", "a,k,b,w,c,d,f", (0.0, 3.0),
              [(0.5, 1.5), (0.5, 1.5), (0.5, 1.5), (0.5, 1.5), (0.5, 1.5), (0.5, 1.5), (0.5, 3.0)]),
}
EXP_FREE = ("mm", "hill", "lorentz2", "rational", "roots")
WITH_FUNCTIONS = ("gauss2d", "dsine", "logistic", "stretched", "mixed")
# the exp-free cases the solvers are held to the oracle on, (name, m): with NPROB, SEED, sigma and spread below the
# reference's lss_solve returns 0 for every problem in 1 .. 30 Jacobian evaluations, forward differences or analytic
# (tests/test_expr_cpu.py::test_reference_solver_fits_the_generated_cases checks exactly that)
SOLVE_CASES = [("mm", 64), ("hill", 200), ("lorentz2", 301), ("rational", 256)]
NPROB, SEED, MAX_EVALS = 64, 2026, 500

# Arguments test_function_accuracy measures the device functions over: what the formulas above hand them on the generated
# data, with a margin (pow: base range and the exponents).
ACCURACY_RANGES = {"exp": (-60.0, 12.0), "log": (0.05, 50.0), "sin": (-50.0, 50.0), "cos": (-50.0, 50.0), "tanh": (-5.0, 5.0),
                   "atan": (-20.0, 20.0), "pow": (0.02, 10.0)}
POW_EXPONENTS = (0.7, -0.3, -1.5, -2.5, 0.5, 1.5)


def compile_formula(name):
    import nonlin_amd as nl
    f, v, p = FORMULAS[name][:3]
    return nl.Expr(f, v, p)


def abscissae(name, m, nprob, rng):
    """t [nvar, nprob, m]: a jittered grid over the formula's range; two variables: the pixels of a square of side sqrt(m)."""
    lo, hi = FORMULAS[name][3]
    nvar = len(FORMULAS[name][1].split(","))
    if nvar == 2:
        side = int(round(m ** 0.5))
        assert side * side == m
        g = np.linspace(lo, hi, side)
        xx, yy = np.meshgrid(g, g, indexing="xy")
        t = np.stack([np.tile(xx.ravel(), (nprob, 1)), np.tile(yy.ravel(), (nprob, 1))])
        return np.ascontiguousarray(t)
    step = (hi - lo) / m
    t = np.tile(np.linspace(lo + 0.25 * step, hi - 0.25 * step, m), (nprob, 1)) + rng.uniform(-0.2, 0.2, (nprob, m)) * step
    return np.ascontiguousarray(t[None])


def expr_problems(name, m, nprob=NPROB, seed=SEED, sigma=1e-3, spread=0.05, prog=None):
    """nprob data sets of a formula on m rows: prog, t [nvar, nprob, m], y [nprob, m], x_true, x0 [nprob, n]."""
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
        y[p] = R.value(prog, xt[p], t[:, p])
        y[p] += sigma * np.abs(y[p]).max() * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + spread * rng.uniform(-1, 1, xt.shape))
    return prog, t, np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)
