"""The single solves with a HOST callback -- nlh_lm_solve, nlh_newton_solve, nlh_quasi_newton_solve, nlh_cls_solve and
nlh_bfgs_solve -- as a list of cases, and what one run of a case leaves behind: the return code, x and fvec / fout as
hex, the seven fields of ib, how often each callback was called, a SHA-256 over the sequence of (kind, bytes of the x
argument) of every callback call, and the text printed when print_status is set.  The user's function is the observable
of these entry points: the order and the arguments of its calls are part of what they promise.

tests/golden/make_host_solves.py records every case on the GPU (tests/golden/host_solves_parent.json, written on the
commit BEFORE these entry points were put on the lock-step drivers); tests/test_gpu_host_solves.py holds every later
commit to that file; tests/test_host_solve_cases_cpu.py runs the same cases through the CPU oracle and checks that each
one still does what its label says (it backtracks, it ends at a bound, it runs out of evaluations).

Every callback is deterministic across machines: the compiled dense-quadratic family of tests/host_callback, the
reference's small problems of tests/problems_ref.py, and objectives summed with math.fsum (exactly rounded)."""
import ctypes as C
import hashlib
import json
import math
import os
import subprocess
import tempfile

import numpy as np

import problems_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "host_callback", "libdq_callback.so")
GOLDEN = os.path.join(HERE, "golden", "host_solves_parent.json")
dp = C.POINTER(C.c_double)

CONVERGENCE_ERROR, INVALID_INPUT, UNDEFINED_FUNCTION, UNDERDEFINED, BAD_HANDLE = 106, 201, 211, 212, -3
IB_FIELDS = ("iter_count", "fcn_count", "jacobian_count", "gradient_count", "converge_on_fcn", "converge_on_chng",
             "converge_on_zero_diff")


class DqCtx(C.Structure):
    _fields_ = [("m", C.c_int32), ("n", C.c_int32), ("A", dp), ("b", dp), ("gamma", C.c_double), ("ncalls", C.c_int64), ("u", dp)]


_cb = None


def _dq_lib():
    global _cb
    if _cb is None:
        if not os.path.exists(SO):
            subprocess.check_call(["make", "-C", os.path.dirname(SO), "-s"])
        _cb = C.CDLL(SO)
        for f in (_cb.dq_user_fcn, _cb.dq_user_jac):
            f.restype = None
            f.argtypes = [C.c_void_p, C.c_int32, dp, C.c_int32, dp]
    return _cb


# ---------------------------------------------------------------------------
# problems: f_raw(n, xp, m, fp) / j_raw(n, xp, m, jp) on the callbacks' own pointers; scalar: s_raw(n, xp) -> float,
# g_raw(n, xp, gp)
# ---------------------------------------------------------------------------
class Problem:
    def __init__(self, m, n, x0, f_raw=None, j_raw=None, s_raw=None, g_raw=None, keep=()):
        self.m, self.n, self.x0 = m, n, np.array(x0, dtype=np.float64)
        self.f_raw, self.j_raw, self.s_raw, self.g_raw, self.keep = f_raw, j_raw, s_raw, g_raw, keep


def dq(oracle, m, n, seed=12345, square=False, **kw):
    """The compiled dense-quadratic family (tests/host_callback/dq_callback.c) on the generator's problem `seed`."""
    cb = _dq_lib()
    if square:
        kw = dict(dict(sigma=0.0, square_shift=True), **kw)
    A, b, xt, x0 = oracle.dq_generate(seed, m, n, **kw)
    u = np.zeros(m)
    ctx = DqCtx(m, n, A.ctypes.data_as(dp), b.ctypes.data_as(dp), kw.get("gamma", 0.5), 0, u.ctypes.data_as(dp))
    ref = C.addressof(ctx)
    return Problem(m, n, x0, lambda n_, xp, m_, fp: cb.dq_user_fcn(ref, n_, xp, m_, fp), lambda n_, xp, m_, jp: cb.dq_user_jac(ref, n_, xp, m_, jp),
                   keep=(A, b, u, ctx))


def py(m, n, x0, fcn, jac=None, args=None):
    """A problem of tests/problems_ref.py: fcn(x, f, args), jac(x, J, args) with J an m x n Fortran-order view."""
    def f_raw(n_, xp, m_, fp):
        fcn(np.ctypeslib.as_array(xp, shape=(n_,)), np.ctypeslib.as_array(fp, shape=(m_,)), args)

    def j_raw(n_, xp, m_, jp):
        jac(np.ctypeslib.as_array(xp, shape=(n_,)), np.ctypeslib.as_array(jp, shape=(n_, m_)).T, args)
    return Problem(m, n, x0, f_raw, j_raw if jac else None)


def _cube(x, f, args=None):                                      # n = 1: x^3 - 2 x - 5 = 0 (Wallis), root 2.0945...
    f[0] = x[0] * x[0] * x[0] - 2.0 * x[0] - 5.0


def _cube_jac(x, J, args=None):
    J[0, 0] = 3.0 * (x[0] * x[0]) - 2.0


_T3 = np.array([1.0, 2.0, 4.0])
_Y3 = np.array([2.1, 3.9, 8.2])


def _line3(x, f, args=None):                                     # 3 x 1: y = x t through three points
    f[:] = x[0] * _T3 - _Y3


def _line3_jac(x, J, args=None):
    J[:, 0] = _T3


def _zero_at(x0):
    """F(x) = x - x0 and its Jacobian: the solve converges at its starting point."""
    c = np.array(x0, dtype=np.float64)

    def f(x, out, args=None):
        out[:] = x - c

    def j(x, J, args=None):
        J[:, :] = 0.0
        for i in range(len(c)):
            J[i, i] = 1.0
    return f, j


def rosen(n, x0, scale=100.0):
    """Chained Rosenbrock as a fcnnvar, summed exactly (math.fsum), with its gradient."""
    def terms(x):
        a = x[1:] - x[:-1] * x[:-1]
        b = 1.0 - x[:-1]
        return a, b

    def s_raw(n_, xp):
        x = np.ctypeslib.as_array(xp, shape=(n_,))
        if n_ == 1:
            return float((x[0] - 1.0) * (x[0] - 1.0) * (1.0 + x[0] * x[0]))
        a, b = terms(x)
        return math.fsum(scale * (a * a)) + math.fsum(b * b)

    def g_raw(n_, xp, gp):
        x = np.ctypeslib.as_array(xp, shape=(n_,))
        g = np.ctypeslib.as_array(gp, shape=(n_,))
        if n_ == 1:
            d = x[0] - 1.0
            g[0] = 2.0 * d * (1.0 + x[0] * x[0]) + d * d * (2.0 * x[0])
            return
        a, b = terms(x)
        g[:] = 0.0
        g[:-1] += -4.0 * scale * (a * x[:-1]) - 2.0 * b
        g[1:] += 2.0 * scale * a
    return Problem(1, n, x0, s_raw=s_raw, g_raw=g_raw)


def quad(n, x0):
    """A convex quadratic bowl with unequal axes: f = sum (i + 1) (x_i - 1)^2, and its gradient."""
    w = np.arange(1.0, n + 1.0)

    def s_raw(n_, xp):
        d = np.ctypeslib.as_array(xp, shape=(n_,)) - 1.0
        return math.fsum(w * (d * d))

    def g_raw(n_, xp, gp):
        d = np.ctypeslib.as_array(xp, shape=(n_,)) - 1.0
        np.ctypeslib.as_array(gp, shape=(n_,))[:] = 2.0 * (w * d)
    return Problem(1, n, x0, s_raw=s_raw, g_raw=g_raw)


# ---------------------------------------------------------------------------
# the cases.  solver, a problem factory (oracle) -> Problem, analytic (the user's Jacobian / gradient is handed in),
# options, solver arguments (jdelta; lower, upper, delta, stepscale), and the labels tests/test_host_solve_cases_cpu.py
# checks against the oracle's run of the case.
# ---------------------------------------------------------------------------
def case(name, solver, problem, analytic=False, opts=None, labels=(), **extra):
    return dict(name=name, solver=solver, problem=problem, analytic=analytic, opts=dict(opts or {}), labels=tuple(labels), extra=extra)


def _square_cases(solver, **extra):
    tag = {"newton": "nt", "qn": "qn"}[solver]
    out = []
    for n in (1, 2, 3, 65, 257):
        for analytic in (False, True):
            for ls in (1, 0):
                if n == 1:
                    prob = (lambda o: py(1, 1, [2.5], _cube, _cube_jac))
                elif n == 2:
                    prob = (lambda o: py(2, 2, [1.0, 1.0], PR.fcn1, PR.jac1))
                else:
                    prob = (lambda o, n=n: dq(o, n, n, square=True))
                out.append(case(f"{tag}_n{n}_{'jac' if analytic else 'fd'}_ls{ls}", solver, prob, analytic,
                                dict(max_evals=500, use_line_search=ls), **extra))
    return out


def _lm_shapes():
    return [("3x1", lambda o: py(3, 1, [0.5], _line3, _line3_jac)),
            ("16x3", lambda o: dq(o, 16, 3, seed=7)),
            ("66x65", lambda o: dq(o, 66, 65, seed=11)),
            ("300x37", lambda o: dq(o, 300, 37, gamma=2.0, sigma=0.1, spread=5.0))]


def build_cases():
    cs = []
    # ---- newton_solver
    cs += _square_cases("newton")
    cs.append(case("nt_backtracks", "newton", lambda o: dq(o, 5, 5, seed=BACKTRACK_SEED["newton"], square=True, spread=1.0), True, dict(max_evals=300),
                   labels=("backtracks2",)))
    cs.append(case("nt_backtracks_fd", "newton", lambda o: dq(o, 5, 5, seed=BACKTRACK_SEED["newton"], square=True, spread=1.0), False, dict(max_evals=300)))
    cs.append(case("nt_max_evals", "newton", lambda o: py(2, 2, [0.0, 1.0], PR.powell, PR.powell_jac), True, dict(max_evals=6), labels=("max_evals",)))
    cs.append(case("nt_at_start", "newton", lambda o: py(3, 3, [1.0, -2.0, 0.5], *_zero_at([1.0, -2.0, 0.5])), True, labels=("at_start",)))
    cs.append(case("nt_print", "newton", lambda o: py(2, 2, [1.0, 1.0], PR.fcn1, PR.jac1), True, dict(print_status=1), labels=("print",)))
    cs.append(case("nt_powell", "newton", lambda o: py(2, 2, [0.0, 1.0], PR.powell, PR.powell_jac), True, dict(max_evals=500)))
    cs.append(case("nt_misc01_fd", "newton", lambda o: py(2, 2, [-5.0, 5.0], PR.misc01), False))
    # ---- quasi_newton_solver
    cs += _square_cases("qn", jdelta=5)
    cs.append(case("qn_jdelta1", "qn", lambda o: dq(o, 65, 65, square=True), False, dict(max_evals=500), labels=("jdelta",), jdelta=1))
    cs.append(case("qn_jdelta1_n2", "qn", lambda o: py(2, 2, [1.0, 1.0], PR.fcn1, PR.jac1), True, jdelta=1))
    cs.append(case("qn_backtracks", "qn", lambda o: dq(o, 5, 5, seed=BACKTRACK_SEED["qn"], square=True, spread=1.0), True, dict(max_evals=300),
                   labels=("qn_backtracks",), jdelta=5))
    cs.append(case("qn_max_evals", "qn", lambda o: py(2, 2, [1.0, 1.0], PR.fcn1, PR.jac1), True, dict(max_evals=8), labels=("max_evals",), jdelta=5))
    cs.append(case("qn_at_start", "qn", lambda o: py(3, 3, [1.0, -2.0, 0.5], *_zero_at([1.0, -2.0, 0.5])), True, labels=("at_start",), jdelta=5))
    cs.append(case("qn_print", "qn", lambda o: py(2, 2, [1.0, 1.0], PR.fcn1, PR.jac1), True, dict(print_status=1), labels=("print",), jdelta=5))
    # ---- least_squares_solver
    for tag, prob in _lm_shapes():
        for analytic in (False, True):
            cs.append(case(f"lm_{tag}_{'jac' if analytic else 'fd'}", "lm", prob, analytic, dict(max_evals=500)))
    for policy in (0, 1, 2):
        cs.append(case(f"lm_16x3_policy{policy}", "lm", lambda o: dq(o, 16, 3, seed=7), False, dict(max_evals=500, factor_policy=policy)))
        cs.append(case(f"lm_300x37_policy{policy}", "lm", lambda o: dq(o, 300, 37, gamma=2.0, sigma=0.1, spread=5.0), False,
                       dict(max_evals=500, factor_policy=policy, factor=0.1)))
    cs.append(case("lm_cubic_fit", "lm", lambda o: py(21, 4, [1.0, 1.0, 1.0, 1.0], PR.lsfcn1), False))
    cs.append(case("lm_max_evals", "lm", lambda o: dq(o, 300, 37, gamma=2.0, sigma=0.1, spread=5.0), False, dict(max_evals=3, factor=0.1),
                   labels=("max_evals",)))
    cs.append(case("lm_at_start", "lm", lambda o: py(3, 3, [1.0, -2.0, 0.5], *_zero_at([1.0, -2.0, 0.5])), True, labels=("at_start",)))
    cs.append(case("lm_print", "lm", lambda o: py(21, 4, [1.0, 1.0, 1.0, 1.0], PR.lsfcn1), False, dict(print_status=1), labels=("print",)))
    # ---- constrained_least_squares_solver
    for tag, prob in _lm_shapes():
        for analytic in (False, True):
            cs.append(case(f"cls_{tag}_{'jac' if analytic else 'fd'}", "cls", prob, analytic, dict(max_evals=500)))
    cs.append(case("cls_lower_active", "cls", lambda o: py(21, 4, [1.0, 1.0, 1.0, 2.0], PR.lsfcn1), False, dict(max_evals=500),
                   labels=("lower_active",), lower=[-10.0, 0.0, -10.0, -10.0], upper=[10.0, 10.0, 10.0, 10.0]))
    cs.append(case("cls_x0_outside", "cls", lambda o: py(21, 4, [1.0, 1.0, 1.0, 5.0], PR.lsfcn1), False, dict(max_evals=500),
                   labels=("x0_outside",), lower=[-10.0, -10.0, -10.0, -10.0], upper=[10.0, 10.0, 10.0, 3.0]))
    cs.append(case("cls_bounds_jac", "cls", lambda o: dq(o, 16, 3, seed=7), True, dict(max_evals=500), lower=[-0.05, -1.0, -1.0], upper=[1.0, 1.0, 0.05]))
    cs.append(case("cls_backtracks", "cls", lambda o: py(2, 2, [0.0, 1.0], PR.powell, PR.powell_jac), True, dict(max_evals=200), labels=("cls_backtracks",),
                   delta=10.0))
    cs.append(case("cls_stepscale", "cls", lambda o: py(2, 2, [0.0, 1.0], PR.powell, PR.powell_jac), True, dict(max_evals=200), delta=10.0, stepscale=0.5))
    cs.append(case("cls_max_evals", "cls", lambda o: dq(o, 300, 37, gamma=2.0, sigma=0.1, spread=5.0), False, dict(max_evals=3), labels=("max_evals",)))
    cs.append(case("cls_at_start", "cls", lambda o: py(3, 3, [1.0, -2.0, 0.5], *_zero_at([1.0, -2.0, 0.5])), True, labels=("at_start",)))
    cs.append(case("cls_print", "cls", lambda o: py(21, 4, [1.0, 1.0, 1.0, 1.0], PR.lsfcn1), False, dict(print_status=1, max_evals=500), labels=("print",)))
    # ---- bfgs
    bf = dict(max_evals=500)
    for n, x0 in ((1, [3.0]), (2, [-1.2, 1.0]), (3, [-1.2, 1.0, -1.2])):
        for analytic in (False, True):
            for ls in (1, 0):
                cs.append(case(f"bfgs_rosen_n{n}_{'grad' if analytic else 'fd'}_ls{ls}", "bfgs", lambda o, n=n, x0=x0, ls=ls: rosen(n, x0, 100.0 if ls else 1.0),
                               analytic, dict(bf, use_line_search=ls)))
    cs.append(case("bfgs_quad_n65_grad", "bfgs", lambda o: quad(65, np.zeros(65)), True, bf))
    cs.append(case("bfgs_quad_n257_grad", "bfgs", lambda o: quad(257, np.zeros(257)), True, dict(max_evals=80), labels=("max_evals",)))
    cs.append(case("bfgs_quad_n65_fd", "bfgs", lambda o: quad(65, np.zeros(65)), False, bf))
    cs.append(case("bfgs_update", "bfgs", lambda o: quad(5, np.zeros(5)), True, bf, labels=("update_branch",)))
    cs.append(case("bfgs_refactor", "bfgs", lambda o: rosen(2, [-1.2, 1.0]), True, bf, labels=("refactor_branch",)))
    cs.append(case("bfgs_backtracks", "bfgs", lambda o: rosen(3, [-1.2, 1.0, -1.2]), True, bf, labels=("backtracks2",)))
    cs.append(case("bfgs_max_evals", "bfgs", lambda o: rosen(3, [-1.2, 1.0, -1.2]), True, dict(max_evals=8), labels=("max_evals",)))
    cs.append(case("bfgs_at_start", "bfgs", lambda o: quad(3, np.ones(3)), True, bf, labels=("at_start",)))
    cs.append(case("bfgs_print", "bfgs", lambda o: quad(3, np.zeros(3)), True, dict(bf, print_status=1), labels=("print",)))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


# Generator problems whose first Newton / quasi-Newton steps overshoot, so that a line search backtracks twice or more
# (found by scanning seeds with the CPU oracle; tests/test_host_solve_cases_cpu.py holds them to it).
BACKTRACK_SEED = {"newton": 65, "qn": 36}


# ---------------------------------------------------------------------------
# backends: how a case reaches a library
# ---------------------------------------------------------------------------
class OracleBackend:
    """The CPU oracle (oracle/pyoracle.py): the reference's algorithms, the same callback interface."""
    name = "oracle"

    def __init__(self, O):
        self.O, self.L = O, O.lib()
        self.VECFCN, self.JACFCN, self.FCNNVAR, self.GRADFCN, self.IB = O.VECFCN, O.JACFCN, O.FCNNVAR, O.GRADFCN, O.IterationBehavior

    def options(self, kw):
        return self.O.default_options(**{k: v for k, v in kw.items() if k != "factor_policy"})

    def call(self, solver, o, m, n, f, j, x, out, ib, jdelta, lo, hi, delta, stepscale):
        L, po, pib = self.L, (C.byref(o) if o is not None else None), C.byref(ib)
        if solver == "lm":
            return L.nlo_lm_solve(po, f, j, None, m, n, x, out, pib)
        if solver == "newton":
            return L.nlo_newton_solve(po, f, j, None, n, x, out, pib)
        if solver == "qn":
            return L.nlo_quasi_newton_solve(po, jdelta, f, j, None, n, x, out, pib)
        if solver == "cls":
            return L.nlo_cls_solve(po, delta, stepscale, lo, hi, f, j, None, m, n, x, out, pib)
        return L.nlo_bfgs_solve(po, f, j, None, n, x, out, pib)


class DeviceBackend:
    """The library's C ABI on the handle of a DeviceSolver (the `ds` fixture)."""
    name = "device"

    def __init__(self, ds):
        from nonlin_amd import _lib
        self._lib, self.L, self.h = _lib, ds.lib, ds.h.ptr
        self.VECFCN, self.JACFCN, self.FCNNVAR, self.GRADFCN, self.IB = _lib.VECFCN, _lib.JACFCN, _lib.FCNNVAR, _lib.GRADFCN, _lib.IterationBehavior

    def options(self, kw):
        o = self._lib.default_options()
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(self, solver, o, m, n, f, j, x, out, ib, jdelta, lo, hi, delta, stepscale, h="own"):
        L, po, pib = self.L, (C.byref(o) if o is not None else None), (C.byref(ib) if ib is not None else None)
        h = self.h if h == "own" else h
        if solver == "lm":
            return L.nlh_lm_solve(h, po, m, n, f, j, None, x, out, pib)
        if solver == "newton":
            return L.nlh_newton_solve(h, po, n, f, j, None, x, out, pib)
        if solver == "qn":
            return L.nlh_quasi_newton_solve(h, po, jdelta, n, f, j, None, x, out, pib)
        if solver == "cls":
            return L.nlh_cls_solve(h, po, delta, stepscale, lo, hi, m, n, f, j, None, x, out, pib)
        return L.nlh_bfgs_solve(h, po, n, f, j, None, x, out, pib)


class _Capture:
    """What the process writes to file descriptor 1 (the C library's printf included) while the block runs."""

    def __enter__(self):
        self.libc = C.CDLL(None)
        self.libc.fflush(None)
        self.saved = os.dup(1)
        self.tmp = tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 1)
        return self

    def __exit__(self, *exc):
        self.libc.fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode()
        self.tmp.close()


def _hex(a):
    """The bytes of a float64 array, little-endian, as one hex string (16 digits per value)."""
    return np.atleast_1d(a).astype("<f8").tobytes().hex()


def unhex(s):
    return np.frombuffer(bytes.fromhex(s), dtype="<f8")


def run_case(c, be, oracle, capture=True, points=None):
    """One case through a backend.  Returns the record (plain JSON types) and `kinds`, the callback kinds in call order
    ('f' residual / objective, 'j' Jacobian / gradient).  points: a list that receives (kind, x) of every call."""
    pr = c["problem"](oracle)
    m, n, scalar = pr.m, pr.n, c["solver"] == "bfgs"
    sha, kinds = hashlib.sha256(), []

    def seen(kind, xp, n_):
        kinds.append(kind)
        if points is not None:
            points.append((kind, np.ctypeslib.as_array(xp, shape=(n_,)).copy()))
        sha.update(kind.encode())
        sha.update(C.string_at(xp, 8 * n_))

    if scalar:
        def _f(ctx, n_, xp):
            seen("f", xp, n_)
            return pr.s_raw(n_, xp)

        def _j(ctx, n_, xp, gp):
            seen("j", xp, n_)
            pr.g_raw(n_, xp, gp)
        f = be.FCNNVAR(_f)
        j = be.GRADFCN(_j) if c["analytic"] else C.cast(None, be.GRADFCN)
    else:
        def _f(ctx, n_, xp, m_, fp):
            seen("f", xp, n_)
            pr.f_raw(n_, xp, m_, fp)

        def _j(ctx, n_, xp, m_, jp):
            seen("j", xp, n_)
            pr.j_raw(n_, xp, m_, jp)
        f = be.VECFCN(_f)
        j = be.JACFCN(_j) if c["analytic"] else C.cast(None, be.JACFCN)
    ex = c["extra"]
    lo = np.array(ex["lower"], dtype=np.float64) if ex.get("lower") is not None else None
    hi = np.array(ex["upper"], dtype=np.float64) if ex.get("upper") is not None else None
    x, out, ib = pr.x0.copy(), np.zeros(1 if scalar else m), be.IB()
    o = be.options(c["opts"])
    args = (c["solver"], o, m, n, f, j, x.ctypes.data_as(dp), out.ctypes.data_as(dp), ib, int(ex.get("jdelta", 5)),
            lo.ctypes.data_as(dp) if lo is not None else None, hi.ctypes.data_as(dp) if hi is not None else None,
            float(ex.get("delta", 1.0)), float(ex.get("stepscale", 1.0)))
    text = ""
    if capture:
        with _Capture() as cap:
            rc = be.call(*args)
        text = cap.text
    else:
        rc = be.call(*args)
    rec = {"rc": int(rc), "x": _hex(x), "out": _hex(out), "ib": [int(getattr(ib, k)) for k in IB_FIELDS],
           "calls": {"f": kinds.count("f"), "j": kinds.count("j")}, "sha256": sha.hexdigest(), "stdout": text}
    return rec, "".join(kinds)


# ---------------------------------------------------------------------------
# refusals: the ladder of each entry point, one fault at a time, in the order the entry checks them
# ---------------------------------------------------------------------------
REFUSALS = ("null_handle", "null_fcn", "null_options", "n_zero", "m_zero", "n_above_m", "lds_bound", "qn_max_n")
LM_LDS_MAX_N, QN_MAX_N, ARRAY_SIZE = 3000, 8192, 202             # nlh_lm.hip, nlh_internal.h; NLH_ARRAY_SIZE_ERROR


def run_refusals(be, oracle):
    """Every entry point with one bad argument at a time (and, last, all of them at once: the first rung answers).
    Returns {solver: {fault: [rc, the ib fields after the call (sevens before it)]}}."""
    out = {}
    for solver in ("lm", "newton", "qn", "cls", "bfgs"):
        scalar, rect = solver == "bfgs", solver in ("lm", "cls")
        res = {}
        for fault in REFUSALS + ("all",):
            if fault in ("m_zero", "n_above_m") and not rect:
                continue
            if (fault == "lds_bound" and solver != "lm") or (fault == "qn_max_n" and solver not in ("qn", "bfgs")):
                continue
            on = (lambda k: fault in (k, "all"))
            calls = []
            if scalar:
                f = be.FCNNVAR(lambda ctx, n_, xp: calls.append(1) or 0.0)
                nof, noj = C.cast(None, be.FCNNVAR), C.cast(None, be.GRADFCN)
            else:
                f = be.VECFCN(lambda ctx, n_, xp, m_, fp: calls.append(1))
                nof, noj = C.cast(None, be.VECFCN), C.cast(None, be.JACFCN)
            m, n = (3, 2) if rect else (2, 2)
            if on("n_zero"):
                n = 0
            if on("m_zero") and rect:
                m = 0
            if fault == "n_above_m":
                m, n = 2, 3
            opts = {}
            if fault == "lds_bound":                             # a non-exact policy keeps its n-vectors in LDS: n <= 3000
                m = n = LM_LDS_MAX_N + 1
                opts = dict(factor_policy=0)
            if fault == "qn_max_n":                              # k_qn_retri / k_bf_chol_*: eight columns per thread at most
                m = n = QN_MAX_N + 1
            size = max(4, m, n)
            x, o_, ib = np.ones(size), np.zeros(size), be.IB()
            for k in IB_FIELDS:
                setattr(ib, k, 7)
            o = None if on("null_options") else be.options(opts)
            rc = be.call(solver, o, m, n, nof if on("null_fcn") else f, noj, x.ctypes.data_as(dp), o_.ctypes.data_as(dp), ib, 5, None, None,
                         1.0, 1.0, h=None if on("null_handle") else "own")
            assert not calls and np.array_equal(x, np.ones(size)) and not o_.any(), (solver, fault)
            res[fault] = [int(rc), [int(getattr(ib, k)) for k in IB_FIELDS]]
        out[solver] = res
    return out


def record_all(ds, oracle):
    be = DeviceBackend(ds)
    return {"cases": {c["name"]: run_case(c, be, oracle)[0] for c in build_cases()}, "refusals": run_refusals(be, oracle)}


def dump(rec, path):
    """One line per case, so that the file stays a few hundred lines."""
    with open(path, "w") as fh:
        fh.write('{"cases": {\n')
        fh.write(",\n".join(json.dumps(k) + ": " + json.dumps(v, sort_keys=True) for k, v in sorted(rec["cases"].items())))
        fh.write('\n},\n"refusals": {\n')
        fh.write(",\n".join(json.dumps(k) + ": " + json.dumps(v, sort_keys=True) for k, v in sorted(rec["refusals"].items())))
        fh.write("\n}}\n")


def load(path=GOLDEN):
    with open(path) as fh:
        return json.load(fh)
