"""The formula models (include/nonlin_hip.h: nlh_expr_*) restated in numpy: an interpreter of a dumped postfix program
(nonlin_amd.Expr.program()) that follows the header's table literally -- one IEEE operation per step, tangents in forward
mode with structural zeros (an absent operand is dropped, never multiplied) -- so that a formula without library
functions gives the bits of the device kernels.  It works on arrays of rows and in any dtype numpy computes in, complex x
included (the complex-step check of tests/test_expr_cpu.py).

The same interpreter run on Num objects carries a first-order running bound of |device - numpy| beside every value:
  exact operations (+ - * /, NEG, IPOW's products, sqrt, abs) propagate the incoming error to first order and add one
  rounding of the result, 2^-52 |v|, only where an operand already carries an error: a program of exact operations has
  bound 0, that is bit equality;
  a library function f adds (U_F[f] + 1) 2^-52 |v| -- the device function's error in ulp, measured by
  tests/test_gpu_expr.py::test_function_accuracy, and 1 ulp for numpy's -- plus its conditioning term |f'(a)| err(a).
Test infrastructure, not part of the product."""
import numpy as np

OPS = ("CONST", "VAR", "PARAM", "NEG", "ADD", "SUB", "MUL", "DIV", "IPOW", "POWC", "EXP", "LOG", "SQRT", "SIN", "COS", "TANH", "ATAN", "ABS")
CONST, VAR, PARAM, NEG, ADD, SUB, MUL, DIV, IPOW, POWC, EXP, LOG, SQRT, SIN, COS, TANH, ATAN, ABS = range(18)
U = 2.0 ** -52

# Error of the device library's functions in ulp over the argument ranges of tests/expr_cases.py (ACCURACY_RANGES): the
# maximum test_function_accuracy measured against numpy.longdouble on an MI355X, rounded up to an integer
# (profiles/expr_rate.txt has the measured values: 0.849, 0.638, 0.741, 0.745, 0.833, 1.474, 1.326).
U_F = {"exp": 1, "log": 1, "sin": 1, "cos": 1, "tanh": 1, "atan": 2, "pow": 2}


class Num:
    """A float64 array with a first-order bound of its error beside it."""
    __array_priority__ = 100

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros(self.v.shape) if e is None else np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, Num) else Num(np.asarray(x, dtype=np.float64))

    @staticmethod
    def _exact(v, prop):
        """An exact operation's result: the propagated error, and a rounding of the result where there is any."""
        return Num(v, np.where(prop > 0.0, prop + U * np.abs(v), 0.0))

    def __add__(self, o):
        o = Num.of(o)
        return Num._exact(self.v + o.v, self.e + o.e)

    def __radd__(self, o):
        return Num.of(o) + self

    def __sub__(self, o):
        o = Num.of(o)
        return Num._exact(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Num.of(o) - self

    def __mul__(self, o):
        o = Num.of(o)
        return Num._exact(self.v * o.v, np.abs(o.v) * self.e + np.abs(self.v) * o.e)

    def __rmul__(self, o):
        return Num.of(o) * self

    def __truediv__(self, o):
        o = Num.of(o)
        v = self.v / o.v
        return Num._exact(v, self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v))

    def __rtruediv__(self, o):
        return Num.of(o) / self

    def __neg__(self):
        return Num(-self.v, self.e)


def _lib(name, f, dabs):
    """A library function on Num: (U_F + 1) ulp of the result, and the conditioning term."""
    def g(a, *rest):
        v = f(a.v, *rest)
        return Num(v, (U_F[name] + 1) * U * np.abs(v) + dabs(a.v, v, *rest) * a.e)
    return g


class _Plain:
    """The functions of the table on plain arrays (any dtype)."""
    exp, log, sqrt, sin, cos, tanh, atan = np.exp, np.log, np.sqrt, np.sin, np.cos, np.tanh, np.arctan

    @staticmethod
    def pow(a, c):
        return np.power(a, c)

    @staticmethod
    def abs(a):
        return np.where(a.real < 0, -a, a) if np.iscomplexobj(a) else np.abs(a)

    @staticmethod
    def negative(a):                       # a < 0 of the ABS tangent
        return a.real < 0


class _Tracked:
    exp = staticmethod(_lib("exp", np.exp, lambda a, v: np.abs(v)))
    log = staticmethod(_lib("log", np.log, lambda a, v: 1.0 / np.abs(a)))
    sin = staticmethod(_lib("sin", np.sin, lambda a, v: np.abs(np.cos(a))))
    cos = staticmethod(_lib("cos", np.cos, lambda a, v: np.abs(np.sin(a))))
    tanh = staticmethod(_lib("tanh", np.tanh, lambda a, v: 1.0 - v * v))
    atan = staticmethod(_lib("atan", np.arctan, lambda a, v: 1.0 / (1.0 + a * a)))
    pow = staticmethod(_lib("pow", lambda a, c: np.power(a, c), lambda a, v, c: np.abs(c * v / a)))

    @staticmethod
    def sqrt(a):
        v = np.sqrt(a.v)
        return Num._exact(v, a.e / (2.0 * v))

    @staticmethod
    def abs(a):
        return Num(np.abs(a.v), a.e)

    @staticmethod
    def negative(a):
        return a.v < 0


def _where(c, a, b, F):
    if F is _Tracked:
        return Num(np.where(c, a.v, b.v), np.where(c, a.e, b.e))
    return np.where(c, a, b)


def run(prog, x, tv, j=None, F=_Plain):
    """One pass over the program (op, arg, consts, mask) for parameters x [n] and variables tv [nvar][rows]: (value, tangent
    for column j or None where it is absent -- always None with j = None)."""
    op, arg, consts, mask = prog
    shape = np.shape(tv[0].v if isinstance(tv[0], Num) else tv[0])
    lift = (lambda s: Num(np.full(shape, s))) if F is _Tracked else (lambda s: np.full(shape, s, dtype=np.result_type(x, np.float64)))
    vs, ds = [], []
    for pc in range(len(op)):
        o, k = int(op[pc]), int(arg[pc])
        if o == CONST:
            vs.append(lift(consts[k])); ds.append(None)
        elif o == VAR:
            vs.append(tv[k] if F is _Tracked else np.asarray(tv[k])); ds.append(None)
        elif o == PARAM:
            vs.append(lift(x[k])); ds.append(lift(1.0) if j is not None and k == j else None)
        elif o in (ADD, SUB, MUL, DIV):
            b, db = vs.pop(), ds.pop()
            a, da = vs.pop(), ds.pop()
            ha, hb = da is not None, db is not None
            d = None
            if o == ADD:
                v = a + b
                if ha or hb:
                    d = da + db if ha and hb else (da if ha else db)
            elif o == SUB:
                v = a - b
                if ha or hb:
                    d = da - db if ha and hb else (da if ha else -db)
            elif o == MUL:
                v = a * b
                if ha or hb:
                    d = da * b + a * db if ha and hb else (da * b if ha else a * db)
            else:
                v = q = a / b
                if ha or hb:
                    d = (da - q * db) / b if ha and hb else (da / b if ha else -((q * db) / b))
            vs.append(v); ds.append(d)
        else:
            a, da = vs.pop(), ds.pop()
            d = None
            if o == NEG:
                v = -a
                if da is not None:
                    d = -da
            elif o == IPOW:
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
            elif o == POWC:
                c = float(consts[k])
                v = F.pow(a, c)
                if da is not None:
                    d = (c * F.pow(a, c - 1.0)) * da
            elif o == EXP:
                v = F.exp(a)
                if da is not None:
                    d = v * da
            elif o == LOG:
                v = F.log(a)
                if da is not None:
                    d = da / a
            elif o == SQRT:
                v = F.sqrt(a)
                if da is not None:
                    d = da / (2.0 * v)
            elif o == SIN:
                v = F.sin(a)
                if da is not None:
                    d = F.cos(a) * da
            elif o == COS:
                v = F.cos(a)
                if da is not None:
                    d = -(F.sin(a) * da)
            elif o == TANH:
                v = F.tanh(a)
                if da is not None:
                    d = (1.0 - v * v) * da
            elif o == ATAN:
                v = F.atan(a)
                if da is not None:
                    d = da / (1.0 + a * a)
            elif o == ABS:
                v = F.abs(a)
                if da is not None:
                    d = _where(F.negative(a), -da, da, F)
            else:
                raise ValueError(f"opcode {o}")
            vs.append(v); ds.append(d)
        # "structural": a tangent exists exactly where the compiler's mask says so
        assert j is None or (ds[-1] is not None) == bool((int(mask[pc]) >> j) & 1), (pc, j)
    assert len(vs) == 1
    return vs[0], ds[0]


def value(prog, x, tv):
    """Model values at the rows of tv [nvar][rows]."""
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


def _tracked_vars(tv):
    return [Num(t) for t in tv]


def residual_bound(prog, x, tv, y, w=None):
    """(residual, bound of |device - numpy|) per row."""
    r = run(prog, x, _tracked_vars(tv), F=_Tracked)[0] - Num(y)
    if w is not None:
        r = Num(w) * r
    return r.v, r.e


def jacobian_bound(prog, x, tv, w=None):
    """(Jacobian, bound), both (rows, n)."""
    vals, errs = [], []
    for j in range(len(x)):
        d = run(prog, x, _tracked_vars(tv), j, F=_Tracked)[1]
        if d is None:
            d = Num(np.zeros(np.shape(tv[0])))
        if w is not None:
            d = Num(w) * d
        vals.append(d.v); errs.append(d.e)
    return np.stack(vals, axis=1), np.stack(errs, axis=1)
