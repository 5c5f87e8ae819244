"""CPU tests of the formulas' j0, j1, i0e, i1e, lgamma, expm1 and log1p (include/nonlin_hip.h: NLH_EXPR_J0 ..
NLH_EXPR_LOG1P): what the compiler makes of them and what it refuses, the numpy restatement
(tests/specfun2_restatement.py) against the 40-digit fixture, the Chebyshev tables against mpmath off their nodes, every
tangent rule against the fixture's own values and against central differences, and Airy and gamma-pdf fits on the CPU
oracle with the restatement as callback.  Every test here fails on a library without the seven names."""
import ctypes as C
import math

import numpy as np
import pytest

import defs_restatement as D
import pwfun_restatement as PW
import specfun2_cases as SC
import specfun2_restatement as S2

U = 2.0 ** -52
NL_INVALID_INPUT_ERROR = 201
NAMES = ("j0", "j1", "i0e", "i1e", "lgamma", "expm1", "log1p")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _expr(formula, vars, params):
    import nonlin_amd as nl
    return nl.Expr(formula, vars, params)


@pytest.fixture(scope="module", autouse=True)
def _the_library_knows_the_names():
    """Every test below is about a library that compiles the seven names (the restatement alone proves nothing about it)."""
    for f in NAMES:
        _expr(f"{f}(t)+c", "t", "c").close()


def _listing(e):
    op, arg, consts, mask = e.program()
    return [(S2.OPS[o], int(a)) for o, a in zip(op, arg)]


# ------------------------------------------------------------------------------------------------ 1. the compiler
def test_the_new_tuple_and_the_numbers():
    import nonlin_amd as nl
    assert nl.EXPR_SPECIAL2_OPS == ("J0", "J1", "I0E", "I1E", "LGAMMA", "EXPM1", "LOG1P") == S2.EXPR_SPECIAL2_OPS and "EXPR_SPECIAL2_OPS" in nl.__all__
    assert (S2.J0, S2.J1, S2.I0E, S2.I1E, S2.LGAMMA, S2.EXPM1, S2.LOG1P) == (28, 29, 30, 31, 32, 33, 34) and S2.OPS[28:] == nl.EXPR_SPECIAL2_OPS
    # the older tuples are what they were
    assert nl.EXPR_OPS == PW.OPS[:18] and nl.EXPR_SPECIAL_OPS == ("ERF", "ERFC", "ERFCX", "VOIGT")
    assert nl.EXPR_EXTENDED_OPS == ("POW", "ATAN2", "MIN", "MAX", "WHERE") and nl.EXPR_DEF_OPS == ("LOAD",)
    assert S2.OPS[:28] == nl.EXPR_OPS + nl.EXPR_SPECIAL_OPS + nl.EXPR_EXTENDED_OPS + nl.EXPR_DEF_OPS == D.OPS
    for k, f in enumerate(NAMES):
        e = _expr(f"{f}(a*t)", "t", "a")
        assert _listing(e) == [("PARAM", 0), ("VAR", 0), ("MUL", 0), (f.upper(), 0)] and int(e.program()[0][3]) == 28 + k
        assert [int(v) for v in e.program()[3]] == [1, 0, 1, 1] and e.depth == 2 and not e.roots()[0][3] and not e.roots()[1].any()


def test_listings_masks_and_depth():
    e = _expr("a*(2*j1(k*r)/(k*r))^2+b", "r", "a,k,b")
    assert _listing(e) == [("PARAM", 0), ("CONST", 0), ("PARAM", 1), ("VAR", 0), ("MUL", 0), ("J1", 0), ("MUL", 0), ("PARAM", 1), ("VAR", 0),
                           ("MUL", 0), ("DIV", 0), ("IPOW", 2), ("MUL", 0), ("PARAM", 2), ("ADD", 0)]
    assert [int(v) for v in e.program()[3]] == [1, 0, 2, 0, 2, 2, 2, 2, 0, 2, 2, 2, 3, 4, 7] and e.depth == 4 and e.nconst == 1 and e.defs == ()
    e = SC.compile_formula("vonmises")
    assert _listing(e) == [("PARAM", 0), ("PARAM", 1), ("VAR", 0), ("PARAM", 2), ("SUB", 0), ("COS", 0), ("CONST", 0), ("SUB", 0), ("MUL", 0),
                           ("EXP", 0), ("MUL", 0), ("CONST", 1), ("CONST", 2), ("MUL", 0), ("PARAM", 1), ("I0E", 0), ("MUL", 0), ("DIV", 0)]
    masks = [int(v) for v in e.program()[3]]
    assert masks[15] == 2 and masks[16] == 2 and masks[9] == 6 and masks[17] == 7 and e.depth == 4 and e.nconst == 3
    # a new function inside a definition: LOAD reads it, the frame counts its slot
    e = SC.compile_formula("airy_def")
    assert e.defs == ("u",) and _listing(e) == [("PARAM", 1), ("VAR", 0), ("MUL", 0), ("PARAM", 0), ("CONST", 0), ("LOAD", 0), ("J1", 0), ("MUL", 0),
                                                ("LOAD", 0), ("DIV", 0), ("IPOW", 2), ("MUL", 0), ("PARAM", 2), ("ADD", 0)]
    assert [int(v) for v in e.program()[3]] == [2, 0, 2, 1, 0, 2, 2, 2, 2, 2, 2, 3, 4, 7] and e.depth == 4
    e = _expr("v = j1(k*r); a*v*v+b", "r", "a,k,b")
    assert _listing(e)[:4] == [("PARAM", 1), ("VAR", 0), ("MUL", 0), ("J1", 0)] and e.roots()[0][5] == 3 and e.depth == 3
    # the expanded program is the substituted formula's
    for name in ("airy_def",):
        e = SC.compile_formula(name)
        sub = _expr(D.substituted(SC.FORMULAS[name][0]), "r", "a,k,b")
        assert D.same_program(D.expand(e.program(), e.roots()[0]), sub.program())
        x, r = np.array([3.0, 1.2, 0.1]), np.linspace(0.05, 10.0, 67)
        assert np.array_equal(_bits(S2.value(e.program(), x, [r])), _bits(S2.value(sub.program(), x, [r])))
        assert np.array_equal(_bits(S2.jacobian(e.program(), x, [r])), _bits(S2.jacobian(sub.program(), x, [r])))


def test_older_formulas_run_through_this_restatement_as_before():
    """The older formulas of tests/pwfun_cases.py hold no new opcode, and this restatement gives the older restatement's bits
    for them: values, columns and running bounds.  (That they compile to the words they compiled to is held by the listings
    the older test files pin.)"""
    import pwfun_cases as PC
    for name in PC.EXACT + PC.WITH_FUNCTIONS:
        prog, t, y, xt, x0 = PC.problems(name, 64, nprob=1, zero=name != "phase")
        assert not (prog[0] >= 28).any()
        assert np.array_equal(_bits(S2.residual(prog, x0[0], t[:, 0], y[0])), _bits(PW.residual(prog, x0[0], t[:, 0], y[0])))
        assert np.array_equal(_bits(S2.jacobian(prog, x0[0], t[:, 0])), _bits(PW.jacobian(prog, x0[0], t[:, 0])))
        for got, want in zip(S2.residual_bound(prog, x0[0], t[:, 0], y[0]) + S2.jacobian_bound(prog, x0[0], t[:, 0]),
                             PW.residual_bound(prog, x0[0], t[:, 0], y[0]) + PW.jacobian_bound(prog, x0[0], t[:, 0])):
            assert np.array_equal(_bits(got), _bits(want)), name


REFUSALS = [(f"{f}(t,s)", "t", "s", f"col {len(f) + 2}: '{f}' takes one argument") for f in NAMES]
REFUSALS += [(f"1+{f}(t,s,s)", "t", "s", f"col {len(f) + 4}: '{f}' takes one argument") for f in NAMES]
REFUSALS += [("j0 t", "t", "s", "col 3: '(' expected"), ("lgamma s", "t", "s", "col 7: '(' expected"), ("j0()", "t", "s", "col 3: unexpected ')'")]
REFUSALS += [("t", f, "s", f"vars col 0: '{f}' is a function") for f in NAMES]
REFUSALS += [("t", "t", f"s,{f}", f"params col 2: '{f}' is a function") for f in NAMES]
REFUSALS += [(f"{f} = t; s", "t", "s", f"col 0: '{f}' is a function") for f in NAMES]
REFUSALS += [("s+sinh(t)", "t", "s", "col 2: unknown name 'sinh'"), ("s+cosh(t)", "t", "s", "col 2: unknown name 'cosh'"),
             ("s+y1(t)", "t", "s", "col 2: unknown name 'y1'"), ("s+digamma(t)", "t", "s", "col 2: unknown name 'digamma'")]


@pytest.mark.parametrize("formula,vars,params,message", REFUSALS)
def test_refusals_name_the_column(formula, vars, params, message):
    from nonlin_amd import _lib
    import nonlin_amd as nl
    L = _lib.load()
    e = C.c_void_p(7)
    assert L.nlh_expr_compile(formula.encode(), vars.encode(), params.encode(), C.byref(e)) == NL_INVALID_INPUT_ERROR
    got = L.nlh_expr_error().decode()
    assert not e.value and got.startswith(message), got
    with pytest.raises(ValueError, match="col [0-9]+: "):
        nl.Expr(formula, vars, params)


def test_y0_is_still_a_parameter():
    assert _listing(_expr("y0+j0(t)", "t", "y0")) == [("PARAM", 0), ("VAR", 0), ("J0", 0), ("ADD", 0)]


# ------------------------------------------------------------------------------------------------ 2. the restatement, the fixture
def test_restatement_against_the_fixture():
    """NUMPY_F, this side of the running bound, is the measured error of the restatement's library functions rounded up to an
    integer ulp; MEASURED is the stated arithmetic's, rounded up in the third digit, and i0e and i1e stay within 8 ulp."""
    got = {f: SC.error(f, getattr(S2, f)(SC.fixture()[SC.MEASURES[f][0]])) for f in SC.MEASURES}
    for f, (err, at) in got.items():
        print(f"{f}: {err / U:.3f} ulp of its scale ({err:.3e}) at a = {at!r}")
    for f in ("j0", "j1", "lgamma", "expm1", "log1p"):
        assert math.ceil(got[f][0] / U) == S2.NUMPY_F[f], (f, got[f])
    for f in ("i0e", "i1e", "digamma"):
        assert 0.99 * SC.MEASURED[f] <= got[f][0] <= SC.MEASURED[f], (f, got[f], SC.MEASURED[f])
        assert SC.BOUND[f] == 4.0 * SC.MEASURED[f]
    assert got["i0e"][0] <= SC.CONDITION and got["i1e"][0] <= SC.CONDITION
    assert S2.EXACT_F == {"i0e": 2 * SC.BOUND["i0e"], "i1e": 2 * SC.BOUND["i1e"]}


def test_edges_of_the_stated_arithmetic():
    z = np.array([0.0, -0.0])
    assert np.array_equal(_bits(S2.i1e(z)), _bits([0.0, 0.0])) and (np.abs(S2.i0e(z) - 1.0) <= SC.CONDITION).all()
    big = np.array([1e6, -1e6, 1e300, np.inf])
    assert np.isfinite(S2.i0e(big)).all() and (S2.i0e(big[:2]) > 0).all() and S2.i0e(big)[3] == 0.0
    assert np.array_equal(_bits(S2.i1e(big[:2])), _bits([S2.i1e(1e6), -S2.i1e(1e6)])) and np.isnan(S2.i0e(np.array([np.nan]))).all()
    for f, at in ((S2.i0e, 8.0), (S2.i1e, 8.0), (S2.i1e, 1.0)):       # the ranges meet within the condition
        v = f(np.array([np.nextafter(at, 0.0), at, np.nextafter(at, 9.0)]))
        assert (np.abs(np.diff(v)) <= 2 * SC.CONDITION * v[1]).all()
    d = S2.digamma(np.array([0.0, -0.0, -1.5, np.nan, np.inf, 1.0, 1e-300]))
    assert np.isnan(d[:4]).all() and d[4] == np.inf and abs(d[5] + 0.5772156649015329) <= SC.BOUND["digamma"] and abs(d[6] + 1e300) <= 4 * U * 1e300


def test_tables_against_mpmath_off_the_nodes():
    """The five Chebyshev series against mpmath at points that are no interpolation node (the generator fits at
    Chebyshev-Gauss points of y), and the digamma terms against the Bernoulli numbers.  The rounding error of a series peaks
    at the ends of its range and the peaks are narrow (the first arrangement of i1e passed 8 ulp at one argument in 700 of
    [6, 8] only), so the ranges below 8 are sampled densely and their ends more densely: every value within the condition."""
    import mpmath as mp
    mp.mp.dps = 40
    rng = np.random.default_rng(5)
    low = np.concatenate([rng.uniform(0.0, 8.0, 3000), rng.uniform(6.0, 8.0, 1500), rng.uniform(0.0, 1.0, 500), rng.uniform(1.0, 1.5, 500)])
    high = 8.0 / rng.uniform(1e-6, 1.0, 500)
    for nu, f, parity in ((0, S2.i0e, 1.0), (1, S2.i1e, -1.0)):
        for a in (low, high):
            ref = np.array([float(mp.exp(-mp.mpf(float(v))) * mp.besseli(nu, mp.mpf(float(v)))) for v in a])
            err = np.abs(f(a) - ref) / ref
            print(f"i{nu}e on [{a.min():.3g}, {a.max():.3g}], {len(a)} points: {err.max() / U:.3f} ulp at {a[err.argmax()]!r}")
            assert (err <= SC.CONDITION).all(), (nu, float(err.max() / U), float(a[err.argmax()]))
            assert np.array_equal(_bits(f(-a)), _bits(parity * f(a)))
    assert [len(S2.TABLES[k]) for k in ("I0E_A", "I0E_B", "I1E_A", "I1E_M", "I1E_B", "DIGAMMA_B")] == [30, 25, 15, 28, 25, 7]
    for k in range(1, 8):
        assert S2.DIGAMMA_B[k - 1] == float(mp.bernoulli(2 * k) / (2 * k))
    # the series' truncation: the first omitted terms are below half an ulp of the value
    a = np.array([10.0, 10.5, 12.0])
    assert (np.abs(float(mp.bernoulli(16)) / 16.0 / a ** 16) <= 0.5 * U * np.abs(S2.digamma(a))).all()


# ------------------------------------------------------------------------------------------------ 3. the tangent rules
def _vj(formula, params, x, t):
    e = _expr(formula, "t", params)
    t = np.asarray(t, dtype=np.float64)
    return S2.value(e.program(), np.asarray(x, dtype=np.float64), [t]), S2.jacobian(e.program(), np.asarray(x, dtype=np.float64), [t])


def test_tangents_are_the_fixtures_own_functions():
    """d/da of each function written with the 40-digit values of its neighbours in the table: J0' = -J1, J1' = J0 - J1/a,
    i0e' = i1e - sign(a) i0e, i1e' = i0e - sign(a) i1e - i1e/a, lgamma' = digamma, expm1' = expm1 + 1, log1p' = 1/(1 + a)."""
    fx = SC.fixture()
    a = fx["j_a"]
    nz = a != 0.0
    env = S2.envelope(a)
    v, J = _vj("j0(p+t)", "p", [0.0], a)
    assert (np.abs(J[:, 0] + fx["j1"]) <= 8 * U * env).all()
    v, J = _vj("j1(p+t)", "p", [0.0], a)
    want = np.where(nz, fx["j0"] - fx["j1"] / np.where(nz, a, 1.0), 0.5)
    assert (np.abs(J[:, 0] - want)[nz] <= 16 * U * env[nz] * np.maximum(1.0, 1.0 / np.abs(a[nz]))).all() and (J[~nz, 0] == 0.5).all()
    a = fx["ie_a"]
    nz = a != 0.0
    sg = np.where(a < 0.0, -1.0, 1.0)
    v, J = _vj("i0e(p+t)", "p", [0.0], a)
    want = fx["i1e"] - sg * fx["i0e"]
    assert (np.abs(J[:, 0] - want) <= 4 * SC.BOUND["i0e"] * fx["i0e"]).all()
    v, J = _vj("i1e(p+t)", "p", [0.0], a)
    want = np.where(nz, (fx["i0e"] - sg * fx["i1e"]) - fx["i1e"] / np.where(nz, a, 1.0), 0.5)
    assert (np.abs(J[:, 0] - want)[nz] <= 4 * SC.BOUND["i1e"] * fx["i0e"][nz]).all() and (J[~nz, 0] == 0.5).all()
    a = fx["lg_a"]
    v, J = _vj("lgamma(p+t)", "p", [0.0], a)
    assert (np.abs(J[:, 0] - fx["digamma"]) <= SC.BOUND["digamma"] * np.maximum(np.abs(fx["digamma"]), 1.0)).all()
    a = fx["em_a"]
    v, J = _vj("expm1(p+t)", "p", [0.0], a)
    assert (np.abs(J[:, 0] - np.exp(a)) == 0.0).all() and (np.abs(J[:, 0] - (fx["expm1"] + 1.0)) <= 4 * U * J[:, 0] + U).all()   # (+ U: v + 1.0 cancels for a << 0, the header's remark)
    a = fx["lp_a"]
    v, J = _vj("log1p(p+t)", "p", [0.0], a)
    assert np.array_equal(_bits(J[:, 0]), _bits(1.0 / (1.0 + a)))


@pytest.mark.parametrize("name", SC.EXACT + SC.WITH_FUNCTIONS)
def test_columns_against_central_differences(name):
    """Every analytic column of the case formulas against central differences of the restated value, arguments of both
    signs among them (bessel10, mixed).  h = 1e-6 max(1, |x_j|): truncation and rounding both stay below 1e-8 of the column."""
    prog, t, y, xt, x0 = SC.problems(name, 64, nprob=2)
    for p in range(2):
        J = S2.jacobian(prog, x0[p], t[:, p])
        assert np.isfinite(J).all()
        for j in range(x0.shape[1]):
            xp, xm = x0[p].copy(), x0[p].copy()
            h = 1e-6 * max(1.0, abs(xp[j]))
            xp[j] += h
            xm[j] -= h
            fd = (S2.value(prog, xp, t[:, p]) - S2.value(prog, xm, t[:, p])) / (xp[j] - xm[j])
            assert np.abs(fd - J[:, j]).max() <= 1e-8 * max(1.0, np.abs(J[:, j]).max()), (name, p, j)
    r, eb = S2.residual_bound(prog, x0[0], t[:, 0], y[0])
    Jb, ej = S2.jacobian_bound(prog, x0[0], t[:, 0])
    assert np.array_equal(_bits(r), _bits(S2.residual(prog, x0[0], t[:, 0], y[0]))) and np.array_equal(_bits(Jb), _bits(S2.jacobian(prog, x0[0], t[:, 0])))
    if name in SC.EXACT:
        assert (eb == 0.0).all() and (ej == 0.0).all()                 # the bit-exact class: i0e and i1e only
    else:
        assert (eb > 0.0).all() and (eb <= 1e-9 * np.abs(y[0]).max()).all() and np.isfinite(ej).all()


def test_tangent_edge_rows():
    """The a == 0 rows of J1 and I1E, a < 0 for the even and the odd function, lgamma outside digamma's domain."""
    t = np.array([0.0, -0.0])
    for f in ("j1", "i1e"):
        v, J = _vj(f"{f}(p+t)", "p", [0.0], t)
        assert (v == 0.0).all() and np.array_equal(_bits(J[:, 0]), _bits([0.5, 0.5]))
    t = np.array([0.7, 3.0, 9.5])
    for f, parity in (("j0", 1.0), ("i0e", 1.0), ("j1", -1.0), ("i1e", -1.0)):
        vp, Jp = _vj(f"{f}(p+t)", "p", [0.0], t)
        vm, Jm = _vj(f"{f}(p+t)", "p", [0.0], -t)
        assert np.array_equal(_bits(vm), _bits(parity * vp)) and np.array_equal(_bits(Jm[:, 0]), _bits(-parity * Jp[:, 0])), f
    v, J = _vj("lgamma(p+t)", "p", [0.0], [-1.5, 0.0, 0.5])
    assert np.isnan(J[:2, 0]).all() and np.isfinite(J[2, 0]) and abs(v[0] - math.lgamma(-1.5)) <= 4 * U and v[1] == np.inf
    v, J = _vj("expm1(p*t)+log1p(-(q*t))", "p,q", [1.0, 1.0], [1e-18])
    assert v[0] == 0.0 and np.array_equal(_bits(J[0]), _bits([1e-18, -1e-18]))
    # a tangent that is absent is not computed: no NaN reaches a column that does not name the operand
    v, J = _vj("a+lgamma(t)", "a", [1.0], [-1.5])
    assert J[0, 0] == 1.0


# ------------------------------------------------------------------------------------------------ 4. fits on the oracle
def test_fit_tolerance(oracle):
    """FIT_SHIFT is the measurement: how far the oracle's x moves when the restated library functions are moved by
    U_F + NUMPY_F ulp, rounded up, or SHIFT_FLOOR where the measurement is below it -- at least what is measured here and
    not ten times more (the margin tests/test_pois_cpu.py::test_perturbation_study gives its record: another C library moves
    the last digits).  FIT_TOL is 4 x that, plus, for the Poisson case, what the wrapper's own log and log1p may move."""
    import pois_cases
    for case, recorded in SC.FIT_SHIFT.items():
        got = max(SC.fit_shift(oracle, case), SC.SHIFT_FLOOR)
        print(f"{case}: measured {got:.3e}, recorded {recorded:.3e}")
        assert got <= recorded * (1 + 1e-9) and recorded <= 10.0 * got, (case, got, recorded)
        assert SC.FIT_TOL[case] == 4.0 * recorded + (pois_cases.recorded_tolerance(True) if case.endswith("/pois") else 0.0)


def test_recovery_seed_on_the_oracle(oracle):
    """The seeds of the GPU recovery test: on the CPU oracle alone every solve returns 0, and in RECOVERY_N of the 64 noisy
    Airy patterns and gamma-pdf curves every parameter is within 3 standard errors of its generating value (at most 4 may
    miss: 64 problems x 3 parameters at 0.27 % each would miss about 0.5).  tests/test_gpu_specfun2.py::test_recovery holds
    the device to 4 fewer."""
    for name in SC.RECOVERY:
        prog, t, y, xt, x0 = SC.recovery_problems(name)
        good = 0
        for p in range(len(y)):
            rc, x, f, ib = SC.oracle_fit(oracle, prog, t[:, p], y[p], x0[p], True)
            assert rc == 0, (name, p, rc, ib)
            good += bool((np.abs(x - xt[p]) <= 3.0 * SC.standard_errors(prog, x, t[:, p], y[p])).all())
        print(f"{name} recovery on the oracle: {good} of {len(y)}")
        assert good == SC.RECOVERY_N[name] >= len(y) - 4
