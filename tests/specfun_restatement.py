"""The formula models with their special functions (include/nonlin_hip.h: NLH_EXPR_ERF .. NLH_EXPR_VOIGT, nlh_faddeeva)
restated in numpy: the whole instruction set -- the 18 instructions as tests/expr_restatement.py has them, then ERF, ERFC,
ERFCX and VOIGT -- following the header's tables literally, one IEEE operation per step.  faddeeva_w is the header's
arithmetic of w(z) in real operations, on the constants nlh_faddeeva_table hands back, so that the host entry, the batch
kernel and a formula whose only function is voigt give these bits.  It works in any dtype numpy computes in: the
complex-step check of tests/test_specfun_cpu.py runs it on complex "reals".

The running bound (expr_restatement.Num) extends to erf, erfc, erfcx and exp: (U_F + NUMPY_F) 2^-52 |v| per call plus the
conditioning term.  U_F: the device function's error in ulp, the maximum tests/test_gpu_specfun.py::
test_erf_family_accuracy measured on an MI355X against the 40-digit fixture, rounded up (profiles/specfun_accuracy.txt).
NUMPY_F: this file's own side, measured against the same fixture by tests/test_specfun_cpu.py -- 1 ulp for math.erf, 2 for
math.erfc (the C library's), 8 for erfcx, which numpy lacks and which is computed here as Re w(i|a|) (for a < 0 as
2 exp(a^2) - erfcx(-a) with the square split exactly).  VOIGT is exact arithmetic: it
propagates nothing and needs operands that carry no error (a formula that feeds a library function into voigt has no
running bound here).  Test infrastructure, not part of the product."""
import math

import numpy as np

import expr_restatement as R
from expr_restatement import Num, U

OPS = R.OPS + ("ERF", "ERFC", "ERFCX", "VOIGT")
ERF, ERFC, ERFCX, VOIGT = range(18, 22)
C1, SQRT2, SQRTPI, ISQRTPI = 1.1283791670955126, 1.4142135623730951, 1.772453850905516, 0.5641895835477563
N = 40

U_F = dict(R.U_F, erf=1, erfc=2, erfcx=2)
NUMPY_F = {"erf": 1, "erfc": 2, "erfcx": 8}


# --------------------------------------------------------------------------------------------- the Faddeeva function
def weideman_table(n=N):
    """(L, a [n], highest power first) by Weideman's recipe: the FFT of exp(-t^2)(L^2 + t^2) at t = L tan(theta/2), M = 2n
    sample points on each side."""
    M = 2 * n
    k = np.arange(-M + 1, M)
    L = np.sqrt(n / np.sqrt(2.0))
    t = L * np.tan(k * np.pi / M / 2.0)
    f = np.concatenate(([0.0], np.exp(-t * t) * (L * L + t * t)))
    a = np.real(np.fft.fft(np.fft.fftshift(f))) / (2 * M)
    return float(L), np.ascontiguousarray(a[1:n + 1][::-1])


_TABLE = None


def table():
    """The library's constants (nlh_faddeeva_table): what the arithmetic below runs on."""
    global _TABLE
    if _TABLE is None:
        from nonlin_amd import _lib
        _TABLE = _lib.faddeeva_table()
    return _TABLE


def faddeeva_w(zr, zi):
    """(wr, wi) = w(zr + i zi), the header's operations in the header's order."""
    L, a = table()
    dr, di = L + zi, -zr
    nr, ni = L - zi, zr
    den = dr * dr + di * di
    Zr = (nr * dr + ni * di) / den
    Zi = (ni * dr - nr * di) / den
    pr, pi = a[0] + 0.0 * Zr, 0.0 * Zr
    for k in range(1, N):
        tr = pr * Zr - pi * Zi
        ti = pr * Zi + pi * Zr
        pr = tr + a[k]
        pi = ti
    ir, ii = dr / den, -(di / den)
    qr = ir * ir - ii * ii
    qi = 2.0 * (ir * ii)
    return 2.0 * (pr * qr - pi * qi) + ISQRTPI * ir, 2.0 * (pr * qi + pi * qr) + ISQRTPI * ii


def _abs(a):
    return np.where(a.real < 0, -a, a) if np.iscomplexobj(a) else np.abs(a)


def voigt(x, sigma, gamma):
    """(v, gx, gs, gg): the VOIGT table -- the value and the partials by x, sigma, gamma."""
    s, g = _abs(sigma), _abs(gamma)
    u = s * SQRT2
    zr, zi = x / u, g / u
    wr, wi = faddeeva_w(zr, zi)
    nrm = u * SQRTPI
    v = wr / nrm
    dwr = -(2.0 * (zr * wr - zi * wi))
    dwi = C1 - 2.0 * (zr * wi + zi * wr)
    un = u * nrm
    gx = dwr / un
    gs = -((v + (zr * dwr - zi * dwi) / nrm) / s)
    gg = -(dwi / un)
    return v, gx, np.where(np.real(sigma) < 0, -gs, gs), np.where(np.real(gamma) < 0, -gg, gg)


# --------------------------------------------------------------------------------------------- erf, erfc, erfcx in numpy
_erf = np.vectorize(math.erf, otypes=[np.float64])
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def _two_prod(a, b):
    """a*b = p + e exactly (Dekker: no fused operation needed)."""
    p = a * b
    c = 134217729.0
    ah = c * a - (c * a - a); al = a - ah
    bh = c * b - (c * b - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def erfcx(a):
    """exp(a^2) erfc(a): Re w(i|a|) on the imaginary axis; for a < 0, 2 exp(a^2) - erfcx(-a) with a^2 split exactly."""
    a = np.asarray(a, dtype=np.float64)
    pos = faddeeva_w(np.zeros_like(a), np.abs(a))[0]
    p, e = _two_prod(a, a)
    with np.errstate(over="ignore"):
        big = 2.0 * (np.exp(p) * (1.0 + e))
    return np.where(a < 0.0, big - pos, pos)


def _lib(name, f, dabs):
    def g(a):
        v = f(a.v)
        return Num(v, (U_F[name] + NUMPY_F[name]) * U * np.abs(v) + dabs(a.v, v) * a.e)
    return g


class _Plain(R._Plain):
    erf, erfc, erfcx = staticmethod(_erf), staticmethod(_erfc), staticmethod(erfcx)


class _Tracked(R._Tracked):
    erf = staticmethod(_lib("erf", _erf, lambda a, v: C1 * np.exp(-(a * a))))
    erfc = staticmethod(_lib("erfc", _erfc, lambda a, v: C1 * np.exp(-(a * a))))
    erfcx = staticmethod(_lib("erfcx", erfcx, lambda a, v: np.abs((2.0 * a) * v - C1)))


def _exact_operand(a):
    if isinstance(a, Num):
        if (a.e != 0.0).any():
            raise NotImplementedError("voigt of an operand that carries an error: no running bound")
        return a.v
    return a


# --------------------------------------------------------------------------------------------- the interpreter
def run(prog, x, tv, j=None, F=_Plain):
    """One pass over the program (op, arg, consts, mask) for parameters x [n] and variables tv [nvar][rows]: (value, tangent
    for column j or None where it is absent -- always None with j = None).  expr_restatement.run with four more ops."""
    op, arg, consts, mask = prog
    tracked = F is _Tracked
    shape = np.shape(tv[0].v if isinstance(tv[0], Num) else tv[0])
    lift = (lambda s: Num(np.full(shape, s))) if tracked else (lambda s: np.full(shape, s, dtype=np.result_type(x, np.float64)))
    wrap = (lambda v: Num(v)) if tracked else (lambda v: v)
    vs, ds = [], []
    for pc in range(len(op)):
        o, k = int(op[pc]), int(arg[pc])
        if o == R.CONST:
            vs.append(lift(consts[k])); ds.append(None)
        elif o == R.VAR:
            vs.append(tv[k] if tracked else np.asarray(tv[k])); ds.append(None)
        elif o == R.PARAM:
            vs.append(lift(x[k])); ds.append(lift(1.0) if j is not None and k == j else None)
        elif o in (R.ADD, R.SUB, R.MUL, R.DIV):
            b, db = vs.pop(), ds.pop()
            a, da = vs.pop(), ds.pop()
            ha, hb = da is not None, db is not None
            d = None
            if o == R.ADD:
                v = a + b
                if ha or hb:
                    d = da + db if ha and hb else (da if ha else db)
            elif o == R.SUB:
                v = a - b
                if ha or hb:
                    d = da - db if ha and hb else (da if ha else -db)
            elif o == R.MUL:
                v = a * b
                if ha or hb:
                    d = da * b + a * db if ha and hb else (da * b if ha else a * db)
            else:
                v = q = a / b
                if ha or hb:
                    d = (da - q * db) / b if ha and hb else (da / b if ha else -((q * db) / b))
            vs.append(v); ds.append(d)
        elif o == VOIGT:
            c, dc = vs.pop(), ds.pop()
            b, db = vs.pop(), ds.pop()
            a, da = vs.pop(), ds.pop()
            v, gx, gs, gg = (wrap(r) for r in voigt(_exact_operand(a), _exact_operand(b), _exact_operand(c)))
            d = None
            for g, t in ((gx, da), (gs, db), (gg, dc)):              # the present ones, in this order, summed left to right
                if t is not None:
                    d = g * t if d is None else d + g * t
            vs.append(v); ds.append(d)
        else:
            a, da = vs.pop(), ds.pop()
            d = None
            if o == R.NEG:
                v = -a
                if da is not None:
                    d = -da
            elif o == R.IPOW:
                u = v = a
                for _ in range(abs(k) - 1):
                    u = v
                    v = v * a
                if k < 0:
                    v = 1.0 / v
                if da is not None:
                    d = (float(abs(k)) * u) * da
                    if k < 0:
                        d = -(d * (v * v))
            elif o == R.POWC:
                c = float(consts[k])
                v = F.pow(a, c)
                if da is not None:
                    d = (c * F.pow(a, c - 1.0)) * da
            elif o == R.EXP:
                v = F.exp(a)
                if da is not None:
                    d = v * da
            elif o == R.LOG:
                v = F.log(a)
                if da is not None:
                    d = da / a
            elif o == R.SQRT:
                v = F.sqrt(a)
                if da is not None:
                    d = da / (2.0 * v)
            elif o == R.SIN:
                v = F.sin(a)
                if da is not None:
                    d = F.cos(a) * da
            elif o == R.COS:
                v = F.cos(a)
                if da is not None:
                    d = -(F.sin(a) * da)
            elif o == R.TANH:
                v = F.tanh(a)
                if da is not None:
                    d = (1.0 - v * v) * da
            elif o == R.ATAN:
                v = F.atan(a)
                if da is not None:
                    d = da / (1.0 + a * a)
            elif o == R.ABS:
                v = F.abs(a)
                if da is not None:
                    d = R._where(F.negative(a), -da, da, R._Tracked if tracked else R._Plain)
            elif o == ERF:
                v = F.erf(a)
                if da is not None:
                    d = (C1 * F.exp(-(a * a))) * da
            elif o == ERFC:
                v = F.erfc(a)
                if da is not None:
                    d = -((C1 * F.exp(-(a * a))) * da)
            elif o == ERFCX:
                v = F.erfcx(a)
                if da is not None:
                    d = ((2.0 * a) * v - C1) * da
            else:
                raise ValueError(f"opcode {o}")
            vs.append(v); ds.append(d)
        assert j is None or (ds[-1] is not None) == bool((int(mask[pc]) >> j) & 1), (pc, j)
    assert len(vs) == 1
    return vs[0], ds[0]


def value(prog, x, tv):
    return run(prog, x, tv)[0]


def residual(prog, x, tv, y, w=None):
    r = value(prog, x, tv) - y
    if w is not None:
        r = w * r
    return r


def jacobian(prog, x, tv, w=None):
    """The analytic Jacobian as a (rows, n) array; a column the formula does not depend on is +0.0 (times w)."""
    cols = []
    for j in range(len(x)):
        d = run(prog, x, tv, j)[1]
        if d is None:
            d = np.zeros(np.shape(tv[0]))
        cols.append(w * d if w is not None else d)
    return np.stack(cols, axis=1)


def residual_bound(prog, x, tv, y, w=None):
    """(residual, bound of |device - numpy|) per row."""
    r = run(prog, x, [Num(t) for t in tv], F=_Tracked)[0] - Num(y)
    if w is not None:
        r = Num(w) * r
    return r.v, r.e


def jacobian_bound(prog, x, tv, w=None):
    """(Jacobian, bound), both (rows, n)."""
    vals, errs = [], []
    for j in range(len(x)):
        d = run(prog, x, [Num(t) for t in tv], j, F=_Tracked)[1]
        if d is None:
            d = Num(np.zeros(np.shape(tv[0])))
        if w is not None:
            d = Num(w) * d
        vals.append(d.v); errs.append(d.e)
    return np.stack(vals, axis=1), np.stack(errs, axis=1)
