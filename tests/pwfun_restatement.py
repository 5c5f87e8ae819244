"""The formula models with a fitted exponent, the four-quadrant angle and the selections (include/nonlin_hip.h:
NLH_EXPR_POW .. NLH_EXPR_WHERE) restated in numpy: the whole instruction set -- the 22 instructions as
tests/specfun_restatement.py has them, then POW, ATAN2, MIN, MAX and WHERE -- following the header's table literally, one
IEEE operation per step.  MIN, MAX and WHERE are selections: a formula that uses only them beside the exact operations
(or voigt) gives the device's bits.  Real dtypes only (a comparison has no complex form).

The running bound (expr_restatement.Num) extends to the two library functions: (U_F + 1) 2^-52 |v| per call -- the device
function's error in ulp and 1 ulp for numpy's -- plus the conditioning term of each operand that carries an error.  A
selection passes the value and the bound of the selected operand; the predicate must be exact (tests/pwfun_cases.py chooses
its formulas so), and a predicate that carries an error is refused.  Test infrastructure, not part of the product."""
import numpy as np

import expr_restatement as R
import specfun_restatement as S
from expr_restatement import Num, U

EXPR_EXTENDED_OPS = ("POW", "ATAN2", "MIN", "MAX", "WHERE")
OPS = S.OPS + EXPR_EXTENDED_OPS
POW, ATAN2, MIN, MAX, WHERE = range(22, 27)

# pow: the device function POWC calls (expr_restatement.U_F: 2 ulp), measured again with a fitted exponent by
# tests/test_gpu_pwfun.py::test_pow_and_atan2_accuracy: 1.282 ulp.  atan2: the maximum that test measured on an MI355X
# against numpy.longdouble over [-20, 20]^2 away from the origin, 1.563 ulp, rounded up to an integer
# (profiles/pwfun_accuracy.txt).
U_F = dict(S.U_F, atan2=2)


def _quiet(f):
    def g(*a, **k):
        with np.errstate(all="ignore"):
            return f(*a, **k)
    return g


class _Plain(S._Plain):
    @staticmethod
    def pow2(a, b):
        return np.power(a, b)

    @staticmethod
    def atan2(a, b):
        return np.arctan2(a, b)

    @staticmethod
    def val(a):
        return a

    @staticmethod
    def select(s, a, b):
        return np.where(s, a, b)


class _Tracked(S._Tracked):
    @staticmethod
    def pow2(a, b):
        """pow of two operands: the conditioning terms |b a^(b-1)| err(a) and |v log a| err(b), each only where its operand
        carries an error (at a = 0 they are 0 times infinity otherwise)."""
        v = np.power(a.v, b.v)
        ca = np.where(a.e > 0.0, np.abs(b.v * np.power(a.v, b.v - 1.0)) * a.e, 0.0)
        cb = np.where(b.e > 0.0, np.abs(v * np.log(a.v)) * b.e, 0.0)
        return Num(v, (U_F["pow"] + 1) * U * np.abs(v) + ca + cb)

    @staticmethod
    def atan2(a, b):
        v = np.arctan2(a.v, b.v)
        den = a.v * a.v + b.v * b.v
        return Num(v, (U_F["atan2"] + 1) * U * np.abs(v) + (np.abs(b.v) * a.e + np.abs(a.v) * b.e) / den)

    @staticmethod
    def val(a):
        """The value a predicate compares: exact, or the device may select otherwise."""
        if (a.e != 0.0).any():
            raise NotImplementedError("a selection whose predicate carries an error: no running bound")
        return a.v

    @staticmethod
    def select(s, a, b):
        return Num(np.where(s, a.v, b.v), np.where(s, a.e, b.e))


@_quiet
def run(prog, x, tv, j=None, F=_Plain):
    """One pass over the program (op, arg, consts, mask) for parameters x [n] and variables tv [nvar][rows]: (value, tangent
    for column j or None where it is absent -- always None with j = None).  specfun_restatement.run with five more ops."""
    op, arg, consts, mask = prog
    tracked = F is _Tracked
    shape = np.shape(tv[0].v if isinstance(tv[0], Num) else tv[0])
    lift = (lambda s: Num(np.full(shape, s))) if tracked else (lambda s: np.full(shape, s, dtype=np.float64))
    wrap = (lambda v: Num(v)) if tracked else (lambda v: v)
    eq0 = (lambda a: a.v == 0.0) if tracked else (lambda a: a == 0.0)     # POW's two guards: on the value as computed
    vs, ds = [], []
    for pc in range(len(op)):
        o, k = int(op[pc]), int(arg[pc])
        if o == R.CONST:
            vs.append(lift(consts[k])); ds.append(None)
        elif o == R.VAR:
            vs.append(tv[k] if tracked else np.asarray(tv[k])); ds.append(None)
        elif o == R.PARAM:
            vs.append(lift(x[k])); ds.append(lift(1.0) if j is not None and k == j else None)
        elif o in (R.ADD, R.SUB, R.MUL, R.DIV, POW, ATAN2, MIN, MAX):
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
            elif o == R.DIV:
                v = q = a / b
                if ha or hb:
                    d = (da - q * db) / b if ha and hb else (da / b if ha else -((q * db) / b))
            elif o == POW:
                v = F.pow2(a, b)
                if ha:
                    ga = b * F.pow2(a, b - 1.0)
                    ta = F.select(eq0(da), lift(0.0), ga * da)
                if hb:
                    gb = F.select(eq0(v), lift(0.0), v * F.log(a))
                    tb = gb * db
                if ha or hb:
                    d = ta + tb if ha and hb else (ta if ha else tb)
            elif o == ATAN2:
                v = F.atan2(a, b)
                den = a * a + b * b
                if ha or hb:
                    d = (b * da - a * db) / den if ha and hb else ((b * da) / den if ha else -((a * db) / den))
            else:
                s = F.val(b) > F.val(a) if o == MAX else F.val(b) < F.val(a)
                v = F.select(s, b, a)
                if ha or hb:
                    d = F.select(s, db if hb else lift(0.0), da if ha else lift(0.0))
            vs.append(v); ds.append(d)
        elif o == WHERE:
            b, db = vs.pop(), ds.pop()
            a, da = vs.pop(), ds.pop()
            c, dc = vs.pop(), ds.pop()
            s = F.val(c) >= 0.0
            v = F.select(s, a, b)
            d = None
            if da is not None or db is not None or dc is not None:        # (dc itself is never read)
                d = F.select(s, da if da is not None else lift(0.0), db if db is not None else lift(0.0))
            vs.append(v); ds.append(d)
        elif o == S.VOIGT:
            c, dc = vs.pop(), ds.pop()
            b, db = vs.pop(), ds.pop()
            a, da = vs.pop(), ds.pop()
            v, gx, gs, gg = (wrap(r) for r in S.voigt(S._exact_operand(a), S._exact_operand(b), S._exact_operand(c)))
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
            elif o == S.ERF:
                v = F.erf(a)
                if da is not None:
                    d = (S.C1 * F.exp(-(a * a))) * da
            elif o == S.ERFC:
                v = F.erfc(a)
                if da is not None:
                    d = -((S.C1 * F.exp(-(a * a))) * da)
            elif o == S.ERFCX:
                v = F.erfcx(a)
                if da is not None:
                    d = ((2.0 * a) * v - S.C1) * da
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
