"""Formulas with definitions (include/nonlin_hip.h: name = expr; ...), their seeded data and the restatement of a whole point
list (tests/test_defs_cpu.py, tests/test_gpu_defs.py, profiles/scripts/defs_rate.py).  EXACT: no library function, so the
device is held to the restatement of the expanded program bit for bit (tests/defs_restatement.py); the others are held bit
for bit to the device's own run of the substituted formula.  Test infrastructure, not part of the product."""
import numpy as np

import defs_restatement as D
import expr_limit_cases as LC
import pwfun_restatement as PW

_P32 = ",".join("p%d" % k for k in range(32))
LN2 = "0.6931471805599453"


def _pvoigt(k):
    return "a%d*(e%d/(1+q%d)+(1-e%d)*exp(-%s*q%d))" % (k, k, k, k, LN2, k)


def pvoigt(peaks):
    """peaks pseudo-Voigt peaks on a constant: q_k = ((t-m_k)/w_k)^2 is written once and used twice."""
    return ("".join("q%d = ((t-m%d)/w%d)^2; " % (k, k, k) for k in range(1, peaks + 1))
            + "+".join(_pvoigt(k) for k in range(1, peaks + 1)) + "+c")


def rot2d_sum(peaks):
    """peaks rotated elliptical Gaussians on a constant."""
    d = "".join("dx%d = x-x%d; dy%d = y-y%d; c%d = cos(th%d); s%d = sin(th%d); u%d = dx%d*c%d + dy%d*s%d; v%d = dy%d*c%d - dx%d*s%d; "
                .replace("%d", str(k)) for k in range(1, peaks + 1))
    return d + "b+" + "+".join("a%d*exp(-(u%d^2/(2*sx%d^2) + v%d^2/(2*sy%d^2)))".replace("%d", str(k)) for k in range(1, peaks + 1))


def emg_sum(peaks):
    """peaks exponentially modified Gaussians on a constant."""
    return ("".join("z%d = (t-m%d)/s%d; " % (k, k, k) for k in range(1, peaks + 1))
            + "+".join("a%d*0.5*k%d*exp(-0.5*z%d^2)*erfcx((s%d*k%d-z%d)/sqrt(2))".replace("%d", str(k)) for k in range(1, peaks + 1)) + "+c")


ROT2D = """dx = x-x0; dy = y-y0; c = cos(th); s = sin(th);
           u = dx*c + dy*s;  v = dy*c - dx*s;
           b + a*exp(-(u^2/(2*sx^2) + v^2/(2*sy^2)))"""
# the same model with only the two library calls named: a frame of 8 instead of 12
ROT2D_CS = """c = cos(th); s = sin(th);
              b + a*exp(-(((x-x0)*c + (y-y0)*s)^2/(2*sx^2) + ((y-y0)*c - (x-x0)*s)^2/(2*sy^2)))"""
# frame 16: eight definitions under an expression eight deep; one definition more is refused
_DEF8 = "".join("d%d = p%d*t+p%d; " % (k, k, k + 8) for k in range(8))
_DEEP8 = "d0+(d1+(d2+(d3+(d4+(d5+(d6*d7+p16))))))"
FRAME16 = _DEF8 + _DEEP8
FRAME17 = _DEF8 + "d8 = p17*t; " + _DEEP8
# 56 instructions as written, 321 with u substituted
OVER256 = "u = " + "+".join("p%d*t" % k for k in range(10)) + "; u*u-u/(1+u*u)+u*u*u"

# name: (formula, vars, params, variable range, (low, high) of every true parameter)
FORMULAS = {
    "gauss_u": ("u = (t-mu)/s; a*exp(-u^2/2)+c", "t", "a,mu,s,c", (0.0, 2.0), [(0.5, 1.5), (0.8, 1.2), (0.2, 0.4), (0.1, 0.3)]),
    "chain": ("u = t-mu; v = u/s; a/(1+v*v)+c", "t", "a,mu,s,c", (0.0, 2.0), [(0.5, 1.5), (0.8, 1.2), (0.2, 0.4), (0.1, 0.3)]),
    "bare_param": ("k = a; k*t+k*b", "t", "a,b", (0.0, 2.0), [(0.5, 1.5), (0.5, 1.5)]),
    "bare_const": ("h = 0.5; h*a*t+h", "t", "a", (0.0, 2.0), [(0.5, 1.5)]),
    "unused": ("z = b*t; a*t+1", "t", "a,b,c", (0.0, 2.0), [(0.5, 1.5)] * 3),
    "lower": ("u = a*t; (u-b)*(b-u)", "t", "a,b", (0.0, 2.0), [(0.5, 1.5), (0.5, 1.5)]),
    "voigt_mid": ("w = s+0.1; a*voigt(t-mu, w, g)+c", "t", "a,mu,s,g,c", (0.0, 2.0),
                  [(0.5, 1.5), (0.8, 1.2), (0.2, 0.4), (0.1, 0.3), (0.1, 0.3)]),
    "where_mid": ("u = a*t; where(t-b, u, c)", "t", "a,b,c", (0.0, 2.0), [(0.5, 1.5), (0.8, 1.2), (0.5, 1.5)]),
    "unary": ("u = a*t+b; abs(u)+u^2-(-u)", "t", "a,b", (-1.0, 1.0), [(0.5, 1.5), (-0.5, 0.5)]),
    "rot2d_rational": ("dx = x-x0; dy = y-y0; u = dx*c + dy*s; v = dy*c - dx*s; b + a/(1+u^2/(2*sx^2)+v^2/(2*sy^2))", "x,y",
                       "a,x0,y0,sx,sy,c,s,b", (0.0, 14.0),
                       [(50.0, 200.0), (5.5, 8.5), (5.5, 8.5), (1.2, 2.2), (2.4, 3.4), (0.7, 0.9), (0.4, 0.6), (5.0, 20.0)]),
    "frame16": (FRAME16, "t", _P32, (0.0, 1.0), [(0.5, 1.5)] * 32),
    "over256": (OVER256, "t", ",".join("p%d" % k for k in range(10)), (0.0, 1.0), [(0.5, 1.5)] * 10),
    "rot2d": (ROT2D, "x,y", "a,x0,y0,sx,sy,th,b", (0.0, 14.0),
              [(50.0, 200.0), (5.5, 8.5), (5.5, 8.5), (1.2, 2.2), (2.4, 3.4), (0.2, 1.2), (5.0, 20.0)]),
    "rot2d_cs": (ROT2D_CS, "x,y", "a,x0,y0,sx,sy,th,b", (0.0, 14.0),
                 [(50.0, 200.0), (5.5, 8.5), (5.5, 8.5), (1.2, 2.2), (2.4, 3.4), (0.2, 1.2), (5.0, 20.0)]),
    "emg": (emg_sum(1), "t", "a1,k1,m1,s1,c", (0.0, 10.0), [(0.5, 1.5), (0.8, 1.6), (3.0, 5.0), (0.4, 0.8), (0.1, 0.3)]),
    "pvoigt2": (pvoigt(2), "t", "a1,m1,w1,e1,a2,m2,w2,e2,c", (0.0, 10.0),
                [(0.5, 1.5), (2.5, 3.5), (0.4, 0.8), (0.3, 0.7), (0.5, 1.5), (6.5, 7.5), (0.4, 0.8), (0.3, 0.7), (0.1, 0.3)]),
}
SMALL = ("gauss_u", "chain", "bare_param", "bare_const", "unused", "lower", "voigt_mid", "where_mid", "unary")
MODELS = ("rot2d", "rot2d_cs", "emg", "pvoigt2")                    # the models profiles/scripts/defs_rate.py times
# no library function (voigt is stated arithmetic): the restatement's bits
EXACT = ("chain", "bare_param", "bare_const", "unused", "lower", "voigt_mid", "where_mid", "unary", "rot2d_rational", "frame16",
         "over256")
# sums of peaks of the three models: (formula of K peaks, vars, parameter list of K peaks)
PEAKS = {"rot2d": (rot2d_sum, "x,y", lambda K: ",".join("a%d,x%d,y%d,sx%d,sy%d,th%d".replace("%d", str(k)) for k in range(1, K + 1)) + ",b"),
         "emg": (emg_sum, "t", lambda K: ",".join("a%d,k%d,m%d,s%d".replace("%d", str(k)) for k in range(1, K + 1)) + ",c"),
         "pvoigt": (pvoigt, "t", lambda K: ",".join("a%d,m%d,w%d,e%d".replace("%d", str(k)) for k in range(1, K + 1)) + ",c")}


def compile_formula(name, substituted=False):
    import nonlin_amd as nl
    f, v, p = FORMULAS[name][:3]
    return nl.Expr(D.substituted(f) if substituted else f, v, p)


def expanded(e):
    return D.expand(e.program(), e.roots()[0])


def problems(name, m, nprob=5, seed=2026, sigma=1e-3, spread=0.03):
    """nprob data sets of a formula on m rows: the expanded program, t [nvar, nprob, m], y [nprob, m], x_true, x0 [nprob, n].
    One variable: a jittered grid over the range; two: uniform draws from it."""
    e = compile_formula(name)
    prog = expanded(e)
    f, v, p, (lo, hi), box = FORMULAS[name]
    rng = np.random.default_rng(seed)
    nvar = e.nvar
    e.close()
    if nvar == 1:
        step = (hi - lo) / m
        t = (np.tile(np.linspace(lo + 0.25 * step, hi - 0.25 * step, m), (nprob, 1)) + rng.uniform(-0.2, 0.2, (nprob, m)) * step)[None]
    else:
        t = rng.uniform(lo, hi, (nvar, nprob, m))
    box = np.array(box)
    xt = rng.uniform(box[:, 0], box[:, 1], (nprob, len(box)))
    y = np.empty((nprob, m))
    for q in range(nprob):
        y[q] = PW.value(prog, xt[q], t[:, q])
        y[q] += sigma * np.abs(y[q]).max() * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + spread * rng.uniform(-1, 1, xt.shape))
    return prog, np.ascontiguousarray(t), np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


restate = LC.restate                                                # F [npoints, m], J [npoints, n, m] of a whole point list


def most_peaks(make, vars, params_of):
    """(with definitions, substituted): the largest number of peaks of make(peaks) that compiles each way."""
    import nonlin_amd as nl
    best = [0, 0]
    for which in (0, 1):
        for peaks in range(1, 17):
            f = make(peaks)
            try:
                nl.Expr(D.substituted(f) if which else f, vars, params_of(peaks)).close()
            except ValueError:
                break
            best[which] = peaks
    return tuple(best)
