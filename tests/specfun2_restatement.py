"""The formula models with the second set of special functions (include/nonlin_hip.h: NLH_EXPR_J0 .. NLH_EXPR_LOG1P)
restated in numpy: the whole instruction set -- the 28 instructions as tests/pwfun_restatement.py and
tests/defs_restatement.py have them (LOAD is run as it stands: a copy of slot k), then J0, J1, I0E, I1E, LGAMMA, EXPM1 and
LOG1P -- following the header's table literally, one IEEE operation per step.

i0e, i1e and digamma are the header's stated arithmetic, on the tables tests/golden/make_specfun2_tables.py printed (the
literals below are that run's, as the kernel header's are): i0e and i1e use + - * / and sqrt only, so a formula whose only
functions they are gives the device's bits.  expm1 and log1p are math's, j0, j1 and lgamma the C library's through ctypes.
No scipy, no mpmath: the GPU tests load this file.  Real dtypes only.

The running bound (expr_restatement.Num) gets, per call of a library function f, (U_F[f] + NUMPY_F[f]) 2^-52 times the scale
its error is measured against -- |v|, for j0 and j1 the envelope min(1, sqrt(2/(pi |a|))), for lgamma max(|v|, 1) -- plus
the conditioning term |g| err(a).  U_F: the device function's error in ulp of that scale, the maximum
tests/test_gpu_specfun2.py::test_function_accuracy measured on an MI355X against the 40-digit fixture, rounded up
(profiles/specfun2_accuracy.txt).  NUMPY_F: this file's own side, measured against the same fixture by
tests/test_specfun2_cpu.py::test_restatement_against_the_fixture.  i0e and i1e are exact arithmetic: of an exact operand they
carry no error; of an operand that carries one, the conditioning term and twice their own bound (specfun2_cases.BOUND: the
two evaluations round differently).  digamma is run on Num objects as it is written, so its log and its operations carry
their own terms.  Test infrastructure, not part of the product."""
import ctypes
import math

import numpy as np

import expr_restatement as R
import specfun_restatement as S
import pwfun_restatement as PW
import defs_restatement as D
from expr_restatement import Num, U

EXPR_SPECIAL2_OPS = ("J0", "J1", "I0E", "I1E", "LGAMMA", "EXPM1", "LOG1P")
OPS = D.OPS + EXPR_SPECIAL2_OPS
J0, J1, I0E, I1E, LGAMMA, EXPM1, LOG1P = range(28, 35)
LOAD = D.LOAD

# the device library's functions, in ulp of the scale above: measured 1.868, 1.859, 1.444, 0.993, 0.881 on an MI355X
# (profiles/specfun2_accuracy.txt)
U_F = dict(PW.U_F, j0=2, j1=2, lgamma=2, expm1=1, log1p=1)
# this file's side: the C library's j0, j1, lgamma and math's expm1, log1p, measured 1.576, 2.076, 1.863, 0.992, 0.984 ulp
NUMPY_F = dict(S.NUMPY_F, j0=2, j1=3, lgamma=2, expm1=1, log1p=1)
# i0e, i1e of an operand that carries an error: twice specfun2_cases.BOUND (4 x 7.78e-16 and 4 x 3.71e-16, relative)
EXACT_F = {"i0e": 2 * 4 * 7.78e-16, "i1e": 2 * 4 * 3.71e-16}

I0E_A = np.array([float.fromhex(h) for h in (
    "-0x1.45cb72134d0efp-58", "0x1.33362977da589p-55", "-0x1.184eb721ebbb4p-52", "0x1.ee6d893f65ebap-50",
    "-0x1.a5022c297fbebp-47", "0x1.59b464b262627p-44", "-0x1.1164c62ee1af0p-41", "0x1.9fe2fe19bd324p-39",
    "-0x1.2fc957a946abcp-36", "0x1.a98becc743c10p-34", "-0x1.1d4fe13ae9556p-31", "0x1.6d903a454cb34p-29",
    "-0x1.beaf68c0b30abp-27", "0x1.03b769d4d6435p-24", "-0x1.1ec638f227f8dp-22", "0x1.2bf24978cf4acp-20",
    "-0x1.2866fcba56427p-18", "0x1.13f58be9a2859p-16", "-0x1.e2b2659c41d5ap-15", "0x1.8b51b74107cabp-13",
    "-0x1.2e2fd1f15eb52p-11", "0x1.adc758a12100ep-10", "-0x1.1b65e201aa849p-8", "0x1.59961f3dde3ddp-7",
    "-0x1.84e9ef121b6f0p-6", "0x1.93e8acea8a32dp-5", "-0x1.84b70342d06eap-4", "0x1.5f7ac77ac88c0p-3",
    "-0x1.37febc057cd8dp-2", "0x1.5a84e9035a22ap-1",
)])
I0E_B = np.array([float.fromhex(h) for h in (
    "-0x1.0adb754ca8b19p-57", "-0x1.646da66119130p-58", "0x1.9be1812d98421p-55", "0x1.3f3dd076041cdp-55",
    "-0x1.4600babd21fe4p-52", "-0x1.8aee7d908de38p-52", "0x1.fee7da3eafb1fp-50", "0x1.12a919094e6d7p-48",
    "-0x1.583fe7e65629ap-47", "-0x1.75d99cf68bb32p-45", "0x1.156ff0d5fc545p-46", "0x1.b1c8c6b83c073p-42",
    "0x1.94347fa268cecp-41", "-0x1.f904303178d66p-40", "-0x1.d0fd7357e7bf2p-37", "-0x1.1511d08397425p-35",
    "0x1.a24feabe8004fp-37", "0x1.0f9ccc0f46f75p-31", "0x1.d2c64a9225b87p-29", "0x1.8569280d6d56dp-26",
    "0x1.b8007d9cd616ep-23", "0x1.8412bc101c586p-19", "0x1.20fa378999e52p-14", "0x1.b998ca2e59049p-9",
    "0x1.9be62aca809cbp-1",
)])
I1E_A = np.array([float.fromhex(h) for h in (
    "0x1.7cec2db187285p-57", "-0x1.7237f96834e46p-52", "0x1.50bb830d17b75p-47", "-0x1.1d48a49755aa2p-42",
    "0x1.bfd46f9bed1cbp-38", "-0x1.4396657ae9b3cp-33", "0x1.ab4d622e41c6cp-29", "-0x1.ff01fcb434e5fp-25",
    "0x1.11b468693d58cp-20", "-0x1.030dc18649cd8p-16", "0x1.a999415d3048fp-13", "-0x1.2822a9da1083dp-9",
    "0x1.50c931cd756efp-6", "-0x1.2670dd1fc00bfp-3", "0x1.553130fd36b0ap-1",
)])
I1E_M = np.array([float.fromhex(h) for h in (
    "0x1.341a9e4567edap-59", "-0x1.34cf57a7ba1e6p-56", "0x1.2ab592d3ef91ap-53", "-0x1.167fd6b18cb28p-50",
    "0x1.f3e0cb302fefdp-48", "-0x1.af342327635e9p-45", "0x1.64f94e52ff15ep-42", "-0x1.1b23d2c6aaf22p-39",
    "0x1.ad8f4c8a1c5d7p-37", "-0x1.370675b689ab6p-34", "0x1.acff924c92859p-32", "-0x1.19267d6a5c7e4p-29",
    "0x1.5d4e0bf7c4eafp-27", "-0x1.9a37889088869p-25", "0x1.c5f81ce8ff7f7p-23", "-0x1.d7ca694355559p-21",
    "0x1.caaab7dcaa367p-19", "-0x1.9f46b100f0dc5p-17", "0x1.5c5441866551ap-15", "-0x1.0cf0154c327d8p-13",
    "0x1.7b020071a581ep-12", "-0x1.e15a34ac81499p-11", "0x1.0d692b21c9c96p-9", "-0x1.f97b8a302d41fp-9",
    "0x1.4dbc7f3dfde8cp-8", "0x1.f998700f0c15ep-11", "-0x1.6c0a234c41eb2p-5", "0x1.665b03d233307p-2",
)])
I1E_B = np.array([float.fromhex(h) for h in (
    "0x1.1556db352e8e6p-57", "0x1.45b8aea87b950p-58", "-0x1.acea3b2532277p-55", "-0x1.2806c9c773320p-55",
    "0x1.55915fceb588ap-52", "0x1.7d68e5f04a2d1p-52", "-0x1.0efcd8bc4d22ap-49", "-0x1.12db5138afbc7p-48",
    "0x1.776e1762d31e8p-47", "0x1.80d3c26b3281ep-45", "-0x1.7a9482e6d22a0p-46", "-0x1.cbc458e73e255p-42",
    "-0x1.953e1076ab493p-41", "0x1.1e7d3f6439fa3p-39", "0x1.f101f653c457bp-37", "0x1.1e1a1f1587865p-35",
    "-0x1.4dcf9d4504c0cp-36", "-0x1.334ca5423dd80p-31", "-0x1.0790b9ad53528p-28", "-0x1.c415394bb46c1p-26",
    "-0x1.0dbfd2e9e5443p-22", "-0x1.048df49ca0373p-18", "-0x1.cfd7f804aa9a6p-14", "-0x1.3fda053fcdb4cp-7",
    "0x1.8ea18b55b1514p-1",
)])
DIGAMMA_B = np.array([float.fromhex(h) for h in (
    "0x1.5555555555555p-4", "-0x1.1111111111111p-7", "0x1.0410410410410p-8", "-0x1.1111111111111p-8",
    "0x1.f07c1f07c1f08p-8", "-0x1.5995995995996p-6", "0x1.5555555555555p-4",
)])
TABLES = {"I0E_A": I0E_A, "I0E_B": I0E_B, "I1E_A": I1E_A, "I1E_M": I1E_M, "I1E_B": I1E_B, "DIGAMMA_B": DIGAMMA_B}


# --------------------------------------------------------------------------------------------- the stated arithmetic
def chebyshev(y, c):
    """Clenshaw's recurrence over c, highest degree first: the header's steps."""
    b0, b1, b2 = c[0] + 0.0 * y, 0.0 * y, 0.0 * y
    for k in range(1, len(c)):
        b2 = b1
        b1 = b0
        b0 = (y * b1 - b2) + c[k]
    return 0.5 * (b0 - b2)


def i0e(a):
    """exp(-|a|) I0(a)."""
    x = np.abs(np.asarray(a, dtype=np.float64))
    with np.errstate(all="ignore"):
        low = chebyshev(x / 2.0 - 2.0, I0E_A)
        high = chebyshev(32.0 / x - 2.0, I0E_B) / np.sqrt(x)
    return np.where(x <= 8.0, low, high)


def i1e(a):
    """exp(-|a|) I1(a); odd, i1e(-0.0) = +0.0."""
    a = np.asarray(a, dtype=np.float64)
    x = np.abs(a)
    with np.errstate(all="ignore"):
        low = chebyshev(x * 4.0 - 2.0, I1E_A) * x
        middle = chebyshev((x - 4.5) / 1.75, I1E_M)
        high = chebyshev(32.0 / x - 2.0, I1E_B) / np.sqrt(x)
    v = np.where(x <= 1.0, low, np.where(x <= 8.0, middle, high))
    return np.where(a < 0.0, -v, v)


def _digamma(a, log, sel, lift, val):
    """The header's digamma on plain arrays or on Num objects (sel: a select by a plain mask; val: the plain values)."""
    dom = val(a) > 0.0
    a = sel(dom, a, lift(1.0))                                       # (outside the domain: NaN below; keep the loop finite)
    r = lift(0.0)
    for _ in range(10):                                              # while a < 10.0: ten steps at most for a > 0
        go = val(a) < 10.0
        r = sel(go, r + 1.0 / a, r)
        a = sel(go, a + 1.0, a)
    z = 1.0 / (a * a)
    p = lift(DIGAMMA_B[6])
    for k in range(5, -1, -1):
        p = p * z + DIGAMMA_B[k]
    p = p * z
    return sel(dom, ((log(a) - 0.5 / a) - p) - r, lift(np.nan))


def digamma(a):
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(all="ignore"):
        return _digamma(a, np.log, np.where, lambda s: np.full(a.shape, s), lambda v: v)


# --------------------------------------------------------------------------------------------- the library functions
_libm = ctypes.CDLL("libm.so.6")


def _c(name):
    f = getattr(_libm, name)
    f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
    return np.vectorize(lambda v: f(float(v)), otypes=[np.float64])


def _m(f):
    def g(v):
        try:
            return f(v)
        except (ValueError, OverflowError):                          # log1p(a <= -1), expm1 past the range: the C library's values
            return math.nan if v < -1.0 or v != v else (-math.inf if v == -1.0 else math.inf)
    return np.vectorize(g, otypes=[np.float64])


j0, j1, lgamma = _c("j0"), _c("j1"), _c("lgamma")
expm1, log1p = _m(math.expm1), _m(math.log1p)


def envelope(a):
    """The amplitude of j0 and j1, the scale their errors are measured against: min(1, sqrt(2/(pi |a|)))."""
    with np.errstate(divide="ignore"):
        return np.minimum(1.0, np.sqrt(2.0 / (np.pi * np.abs(a))))


def _lib(name, f, scale, dabs):
    def g(a):
        v = f(a.v)
        return Num(v, (U_F[name] + NUMPY_F[name]) * U * scale(a.v, v) + dabs(a.v, v) * a.e)
    return g


def _exact(name, f, dabs):
    def g(a):
        v = f(a.v)
        return Num(v, np.where(a.e > 0.0, dabs(a.v, v) * a.e + EXACT_F[name] * np.abs(v), 0.0))
    return g


def _di0e(a, v):
    return np.abs(i1e(a) - np.where(a < 0.0, -v, v))


def _di1e(a, v):
    with np.errstate(all="ignore"):
        return np.abs(np.where(a == 0.0, 0.5, (i0e(a) - np.where(a < 0.0, -v, v)) - v / a))


def _dj1(a, v):
    with np.errstate(all="ignore"):
        return np.abs(np.where(a == 0.0, 0.5, j0(a) - v / a))


class _Plain(PW._Plain):
    j0, j1, lgamma, expm1, log1p = staticmethod(j0), staticmethod(j1), staticmethod(lgamma), staticmethod(expm1), staticmethod(log1p)
    i0e, i1e, digamma = staticmethod(i0e), staticmethod(i1e), staticmethod(digamma)


class _Tracked(PW._Tracked):
    j0 = staticmethod(_lib("j0", j0, lambda a, v: envelope(a), lambda a, v: np.abs(j1(a))))
    j1 = staticmethod(_lib("j1", j1, lambda a, v: envelope(a), _dj1))
    lgamma = staticmethod(_lib("lgamma", lgamma, lambda a, v: np.maximum(np.abs(v), 1.0), lambda a, v: np.abs(digamma(a))))
    expm1 = staticmethod(_lib("expm1", expm1, lambda a, v: np.abs(v), lambda a, v: np.exp(a)))
    log1p = staticmethod(_lib("log1p", log1p, lambda a, v: np.abs(v), lambda a, v: 1.0 / np.abs(1.0 + a)))
    i0e = staticmethod(_exact("i0e", i0e, _di0e))
    i1e = staticmethod(_exact("i1e", i1e, _di1e))

    @staticmethod
    def digamma(a):
        shape = a.v.shape
        return _digamma(a, PW._Tracked.log, lambda m, p, q: Num(np.where(m, Num.of(p).v, Num.of(q).v), np.where(m, Num.of(p).e, Num.of(q).e)),
                        lambda s: Num(np.full(shape, s)), lambda x: x.v)


# --------------------------------------------------------------------------------------------- the interpreter
_UNARY_OLD = (R.NEG, R.IPOW, R.POWC, R.EXP, R.LOG, R.SQRT, R.SIN, R.COS, R.TANH, R.ATAN, R.ABS, S.ERF, S.ERFC, S.ERFCX)


def _special2(F, o, a, da, lift, plain):
    """(v, d) of J0 .. LOG1P: the header's rows.  g is computed only where the operand has a tangent."""
    neg, zero = plain(a) < 0.0, plain(a) == 0.0
    d = None
    if o == J0:
        v = F.j0(a)
        if da is not None:
            d = -(F.j1(a) * da)
    elif o == J1:
        v = F.j1(a)
        if da is not None:
            d = F.select(zero, lift(0.5), F.j0(a) - v / a) * da
    elif o == I0E:
        v = F.i0e(a)
        if da is not None:
            d = (F.i1e(a) - F.select(neg, -v, v)) * da
    elif o == I1E:
        v = F.i1e(a)
        if da is not None:
            d = F.select(zero, lift(0.5), (F.i0e(a) - F.select(neg, -v, v)) - v / a) * da
    elif o == LGAMMA:
        v = F.lgamma(a)
        if da is not None:
            d = F.digamma(a) * da
    elif o == EXPM1:
        v = F.expm1(a)
        if da is not None:
            d = F.exp(a) * da
    elif o == LOG1P:
        v = F.log1p(a)
        if da is not None:
            d = da / (1.0 + a)
    else:
        raise ValueError(f"opcode {o}")
    return v, d


@PW._quiet
def run(prog, x, tv, j=None, F=_Plain):
    """One pass over the program (op, arg, consts, mask) for parameters x [n] and variables tv [nvar][rows]: (value, tangent
    for column j or None where it is absent -- always None with j = None).  A stack machine over all 35 opcodes: LOAD k
    pushes slot k again (definitions stay at the bottom, so the model value ends on top of them), J0 .. LOG1P are
    _special2, the older rows _pw_instruction."""
    op, arg, consts, mask = prog
    tracked = F is _Tracked
    shape = np.shape(tv[0].v if isinstance(tv[0], Num) else tv[0])
    lift = (lambda s: Num(np.full(shape, s))) if tracked else (lambda s: np.full(shape, s, dtype=np.float64))
    plain = (lambda a: a.v) if tracked else (lambda a: a)
    vs, ds = [], []
    for pc in range(len(op)):
        o, k = int(op[pc]), int(arg[pc])
        if o == R.CONST:
            vs.append(lift(consts[k])); ds.append(None)
        elif o == R.VAR:
            vs.append(tv[k] if tracked else np.asarray(tv[k], dtype=np.float64)); ds.append(None)
        elif o == R.PARAM:
            vs.append(lift(x[k])); ds.append(lift(1.0) if j is not None and k == j else None)
        elif o == LOAD:
            vs.append(vs[k]); ds.append(ds[k])
        elif o >= J0:
            a, da = vs.pop(), ds.pop()
            v, d = _special2(F, o, a, da, lift, plain)
            vs.append(v); ds.append(d)
        else:
            nops = 1 if o in _UNARY_OLD else (3 if o in (S.VOIGT, PW.WHERE) else 2)
            operands, tangents = vs[len(vs) - nops:], ds[len(ds) - nops:]
            del vs[len(vs) - nops:], ds[len(ds) - nops:]
            v, d = _pw_instruction(o, k, consts, operands, tangents, F, lift, tracked)
            vs.append(v); ds.append(d)
        assert j is None or (ds[-1] is not None) == bool((int(mask[pc]) >> j) & 1), (pc, j)
    assert len(vs) == 1 + len(D.definition_roots(op))
    return vs[-1], ds[-1]


def _pw_instruction(o, k, consts, ops, tans, F, lift, tracked):
    """The rows of the older instructions, as pwfun_restatement.run states them (the same text, one instruction at a time)."""
    eq0 = (lambda a: a.v == 0.0) if tracked else (lambda a: a == 0.0)
    wrap = (lambda v: Num(v)) if tracked else (lambda v: v)
    d = None
    if o in (R.ADD, R.SUB, R.MUL, R.DIV, PW.POW, PW.ATAN2, PW.MIN, PW.MAX):
        (a, b), (da, db) = ops, tans
        ha, hb = da is not None, db is not None
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
        elif o == PW.POW:
            v = F.pow2(a, b)
            if ha:
                ta = F.select(eq0(da), lift(0.0), (b * F.pow2(a, b - 1.0)) * da)
            if hb:
                tb = F.select(eq0(v), lift(0.0), v * F.log(a)) * db
            if ha or hb:
                d = ta + tb if ha and hb else (ta if ha else tb)
        elif o == PW.ATAN2:
            v = F.atan2(a, b)
            den = a * a + b * b
            if ha or hb:
                d = (b * da - a * db) / den if ha and hb else ((b * da) / den if ha else -((a * db) / den))
        else:
            s = F.val(b) > F.val(a) if o == PW.MAX else F.val(b) < F.val(a)
            v = F.select(s, b, a)
            if ha or hb:
                d = F.select(s, db if hb else lift(0.0), da if ha else lift(0.0))
        return v, d
    if o == PW.WHERE:
        (c, a, b), (dc, da, db) = ops, tans
        s = F.val(c) >= 0.0
        v = F.select(s, a, b)
        if da is not None or db is not None or dc is not None:
            d = F.select(s, da if da is not None else lift(0.0), db if db is not None else lift(0.0))
        return v, d
    if o == S.VOIGT:
        (a, b, c), (da, db, dc) = ops, tans
        v, gx, gs, gg = (wrap(r) for r in S.voigt(S._exact_operand(a), S._exact_operand(b), S._exact_operand(c)))
        for g, t in ((gx, da), (gs, db), (gg, dc)):
            if t is not None:
                d = g * t if d is None else d + g * t
        return v, d
    (a,), (da,) = ops, tans
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
    return v, d


def value(prog, x, tv, F=_Plain):
    return run(prog, x, tv, F=F)[0]


def residual(prog, x, tv, y, w=None, F=_Plain):
    """F: the function table (specfun2_cases.shifted makes one whose library functions are moved by a few ulp)."""
    r = value(prog, x, tv, F) - y
    if w is not None:
        r = w * r
    return r


def jacobian(prog, x, tv, w=None, F=_Plain):
    """The analytic Jacobian as a (rows, n) array; a column the formula does not depend on is +0.0 (times w)."""
    cols = []
    for j in range(len(x)):
        d = run(prog, x, tv, j, F=F)[1]
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
