"""CPU tests of the formulas' pow, atan2, min, max and where (include/nonlin_hip.h: NLH_EXPR_POW .. NLH_EXPR_WHERE): what
the compiler makes of them and what it refuses, the selections against Python's own eval bit for bit, the edge rules of the
header's table by bits (ties, signed zeros, NaN, the branch not taken, POW's two guards at a = 0), the presence patterns of
every tangent, the analytic POW and ATAN2 columns against central differences, and the hinge, the power law and the
stretched exponential -- t = 0 in the grid -- on the CPU oracle with the numpy restatement (tests/pwfun_restatement.py) as
callback."""
import ctypes as C

import numpy as np
import pytest

import expr_restatement as R
import pwfun_cases as PC
import pwfun_restatement as W
import specfun_restatement as S

EPS = 2.0 ** -52
NL_INVALID_INPUT_ERROR = 201
NAN, INF = float("nan"), float("inf")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _listing(e):
    op, arg, consts, mask = e.program()
    return [(W.OPS[o], int(a)) for o, a in zip(op, arg)]


def _expr(formula, vars, params):
    import nonlin_amd as nl
    return nl.Expr(formula, vars, params)


# ------------------------------------------------------------------------------------------------ 1. the compiler
def test_compile_and_read_back():
    import nonlin_amd as nl
    assert nl.EXPR_EXTENDED_OPS == ("POW", "ATAN2", "MIN", "MAX", "WHERE") == W.EXPR_EXTENDED_OPS == W.OPS[22:]
    assert "EXPR_EXTENDED_OPS" in nl.__all__
    assert W.OPS[:22] == nl.EXPR_OPS + nl.EXPR_SPECIAL_OPS and (W.POW, W.ATAN2, W.MIN, W.MAX, W.WHERE) == (22, 23, 24, 25, 26)
    e = _expr("a*pow(t,b)+c", "t", "a,b,c")
    assert _listing(e) == [("PARAM", 0), ("VAR", 0), ("PARAM", 1), ("POW", 0), ("MUL", 0), ("PARAM", 2), ("ADD", 0)]
    assert [int(k) for k in e.program()[3]] == [1, 0, 2, 2, 3, 4, 7] and e.depth == 3 and e.nconst == 0
    aroot, broot = e.roots()
    assert list(aroot) == [0, 0, 0, 1, 0, 0, 4] and not broot.any()
    for k, f in enumerate(("pow", "atan2", "min", "max")):
        e = _expr(f"{f}(a*t,b)", "t", "a,b")
        assert _listing(e) == [("PARAM", 0), ("VAR", 0), ("MUL", 0), ("PARAM", 1), (f.upper(), 0)]
        assert int(e.program()[0][4]) == 22 + k and e.roots()[0][4] == 2 and e.depth == 2
    # where with operands that are subtrees of their own: c's producer in aroot, a's in broot, b's is the instruction before
    e = _expr("where(t-t0, a*(t-t0), b+1)*s", "t", "t0,a,b,s")
    assert _listing(e) == [("VAR", 0), ("PARAM", 0), ("SUB", 0), ("PARAM", 1), ("VAR", 0), ("PARAM", 0), ("SUB", 0), ("MUL", 0),
                           ("PARAM", 2), ("CONST", 0), ("ADD", 0), ("WHERE", 0), ("PARAM", 3), ("MUL", 0)]
    assert int(e.program()[0][11]) == 26
    aroot, broot = e.roots()
    assert (aroot[11], broot[11]) == (2, 7) and aroot[13] == 11
    masks = [int(k) for k in e.program()[3]]
    assert masks[11] == 1 | 3 | 4 == 7 and masks[2] == 1 and masks[7] == 3 and masks[10] == 4 and masks[13] == 15 and e.depth == 4
    # the condition's parameters are in the mask even where no branch names them
    e = _expr("where(t-p,1+t,2)", "t", "p")
    assert [int(k) for k in e.program()[3]][-1] == 1
    # nesting; the depth: a, where's c and a, and pow's two operands on top of them
    assert _expr("a+where(min(t,a),max(t,1),pow(t,2))", "t", "a").depth == 5
    assert _listing(_expr("a^2.5", "t", "a")) == [("PARAM", 0), ("POWC", 0)]              # '^' is what it was


REFUSALS = [("pow(t)", "t", "s", "col 5: 'pow' takes two arguments"), ("pow(t,s,s)", "t", "s", "col 7: 'pow' takes two arguments"),
            ("atan2(t)", "t", "s", "col 7: 'atan2' takes two arguments"), ("atan2(t,s,1)", "t", "s", "col 9: 'atan2' takes two arguments"),
            ("min(t)", "t", "s", "col 5: 'min' takes two arguments"), ("min(t,s,s)", "t", "s", "col 7: 'min' takes two arguments"),
            ("max(t)", "t", "s", "col 5: 'max' takes two arguments"), ("1+max(t,s,s)", "t", "s", "col 9: 'max' takes two arguments"),
            ("where(t,s)", "t", "s", "col 9: 'where' takes three arguments"), ("where(t)", "t", "s", "col 7: 'where' takes three arguments"),
            ("where(t,s,1,2)", "t", "s", "col 11: 'where' takes three arguments"), ("max t", "t", "s", "col 4: '(' expected"),
            ("t", "t", "s,pow", "params col 2: 'pow' is a function"), ("t", "t", "atan2", "params col 0: 'atan2' is a function"),
            ("t", "t", "min", "params col 0: 'min' is a function"), ("t", "t", "a,b,max", "params col 4: 'max' is a function"),
            ("t", "t", "where", "params col 0: 'where' is a function"), ("t", "pow", "s", "vars col 0: 'pow' is a function"),
            ("t", "t,atan2", "s", "vars col 2: 'atan2' is a function"), ("t", "min", "s", "vars col 0: 'min' is a function"),
            ("t", "max", "s", "vars col 0: 'max' is a function"), ("t", "t, where", "s", "vars col 3: 'where' is a function"),
            ("a^b", "t", "a,b", "col 2: a number expected at 'b'"), ("a^(2)", "t", "a", "col 2: a number expected at '('"),
            ("a*t^b+c", "t", "a,b,c", "col 4: a number expected at 'b'"),
            ("s+sinh(t)", "t", "s", "col 2: unknown name 'sinh'"), ("s+foo", "t", "s", "col 2: unknown name 'foo'")]


@pytest.mark.parametrize("formula,vars,params,message", REFUSALS)
def test_refusals_name_the_column(formula, vars, params, message):
    from nonlin_amd import _lib
    import nonlin_amd as nl
    L = _lib.load()
    e = C.c_void_p(7)
    assert L.nlh_expr_compile(formula.encode(), vars.encode(), params.encode(), C.byref(e)) == NL_INVALID_INPUT_ERROR
    got = L.nlh_expr_error().decode()
    assert not e.value and got.startswith(message), got
    if "^" in formula:
        assert got.endswith("pow(a, b)"), got                          # the pointer to the function that takes the exponent
    with pytest.raises(ValueError, match="col [0-9]+: "):
        nl.Expr(formula, vars, params)


# ------------------------------------------------------------------------------------------------ 3. the exact class
PY_FORMULAS = ["max(a*t,b)", "min(a*t,b)-c", "max(t-a,0)*b+c", "where(t-a,b*t,c)", "where(a-t,b/t,c*t)+min(t,a)", "min(max(t-a,b),c)/(1+t)",
               "a+b*max(t-c,0)-b*max(t-2*c,0)", "where(max(t-a,0),t*t,-t)*min(b,c)", "where(t-a,where(t-c,1,2),3)*b"]


@pytest.mark.parametrize("formula", PY_FORMULAS)
def test_exact_class_against_python(formula):
    """Over + - * /, min, max and where the stated order and selections are Python's: eval of the same string on float64
    arrays, min / max / where as the header's selects, gives the interpreter's bits, values and every column's support."""
    e = _expr(formula, "t", "a,b,c")
    rng = np.random.default_rng(len(formula))
    t = np.sort(rng.uniform(0.1, 4.0, 257))
    t[::16] = 1.5                                                       # ties: t - a == 0 exactly, a*t == b
    env = {"max": lambda a, b: np.where(b > a, b, a), "min": lambda a, b: np.where(b < a, b, a),
           "where": lambda c, a, b: np.where(np.asarray(c) >= 0.0, a, b), "t": t}
    for x in (np.array([1.5, 2.25, 3.0]), np.array([1.5, 0.5, 0.75]), rng.uniform(0.5, 3.0, 3)):
        env.update(a=np.full(257, x[0]), b=np.full(257, x[1]), c=np.full(257, x[2]))
        want = eval(formula, {"__builtins__": {}}, env) + np.zeros(257)
        assert np.array_equal(_bits(W.value(e.program(), x, [t])), _bits(want)), formula
        r, eb = W.residual_bound(e.program(), x, [t], np.zeros(257))
        assert np.array_equal(_bits(r), _bits(want)) and (eb == 0.0).all()       # bound 0: the bit-exact class


# ------------------------------------------------------------------------------------------------ 4. edge rules, by bits
def _vj(formula, params, x, t):
    e = _expr(formula, "t", params)
    t = np.asarray(t, dtype=np.float64)
    return W.value(e.program(), np.asarray(x, dtype=np.float64), [t]), W.jacobian(e.program(), np.asarray(x, dtype=np.float64), [t])


def test_min_max_ties_zeros_and_nan():
    """A tie keeps a; a NaN b is dropped, a NaN a stays; the tangent is the selected operand's."""
    t = np.array([0.0, -0.0, 1.0, NAN, 2.0])
    # max(t, p) at p = 0.0: rows (0, 0) tie -> a = +0.0; (-0, 0) tie -> a = -0.0; (1, 0) -> a; (NaN, 0) -> a = NaN; then p = 2: tie
    for f in ("max", "min"):
        v, J = _vj(f"{f}(t,p)", "p", [0.0], t[:4])
        assert np.array_equal(_bits(v[:2]), _bits([0.0, -0.0])) and np.isnan(v[3])
        assert np.array_equal(_bits(J[:2, 0]), _bits([0.0, 0.0])) and np.array_equal(_bits(J[3, 0]), _bits(0.0))   # a selected: a is Z, +0.0
        v, J = _vj(f"{f}(p,t)", "p", [0.0], t[:4])                      # a = p, b = t
        assert np.array_equal(_bits(v[:2]), _bits([0.0, 0.0])) and np.array_equal(_bits(J[:2, 0]), _bits([1.0, 1.0]))
        assert v[3] == 0.0 and J[3, 0] == 1.0                          # a NaN b is dropped
        v, J = _vj(f"{f}(p,-t)", "p", [-0.0], t[:2])                    # a = -0.0 against b = -0.0, +0.0: a stays
        assert np.array_equal(_bits(v), _bits([-0.0, -0.0]))
    v, J = _vj("max(t,p)", "p", [1.0], t)
    assert np.array_equal(_bits(v[[0, 1, 2, 4]]), _bits([1.0, 1.0, 1.0, 2.0])) and np.array_equal(_bits(J[:, 0]), _bits([1.0, 1.0, 0.0, 0.0, 0.0]))
    v, J = _vj("min(t,p)", "p", [1.0], t)
    assert np.array_equal(_bits(v[[0, 1, 2, 4]]), _bits([0.0, -0.0, 1.0, 1.0])) and np.array_equal(_bits(J[:, 0]), _bits([0.0, 0.0, 0.0, 0.0, 1.0]))
    # a NaN parameter as a: stays
    v, J = _vj("max(p,t)", "p", [NAN], [1.0])
    assert np.isnan(v[0]) and J[0, 0] == 1.0


def test_where_edges():
    """-0.0 selects a, NaN selects b; the branch not taken reaches neither the value nor the tangent."""
    t = np.array([-0.0, 0.0, NAN, -1e-300, 1e-300])
    v, J = _vj("where(t,p,q)", "p,q", [2.0, 3.0], t)
    assert np.array_equal(_bits(v), _bits([2.0, 2.0, 3.0, 3.0, 2.0]))
    assert np.array_equal(_bits(J), _bits([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.0, 1.0], [1.0, 0.0]]))
    # sqrt of a negative number in the branch not taken: exact +0.0 in value and tangent, no NaN
    t = np.array([-4.0, -1.0, -1e-9, 0.0, 1.0, 4.0])
    v, J = _vj("where(t,p*sqrt(t),0)", "p", [3.0], t)
    assert np.array_equal(_bits(v), _bits([0.0, 0.0, 0.0, 0.0, 3.0, 6.0])) and np.array_equal(_bits(J[:, 0]), _bits([0.0, 0.0, 0.0, 0.0, 1.0, 2.0]))
    v, J = _vj("where(t-p,sqrt(t-p),0)", "p", [0.5], t)               # the tangent of sqrt at 0 and below: inf and NaN, not taken
    assert np.array_equal(_bits(v[:4]), _bits(np.zeros(4))) and np.array_equal(_bits(J[:4, 0]), _bits(np.zeros(4)))
    assert np.isfinite(v).all() and np.isfinite(J).all() and J[5, 0] == -1.0 / (2.0 * np.sqrt(3.5))
    v, J = _vj("where(t,1/t,p)", "p", [7.0], [0.0, -0.0])              # c >= 0 at both zeros: a = 1/t, +inf and -inf
    assert np.array_equal(_bits(v), _bits([INF, -INF])) and np.array_equal(_bits(J[:, 0]), _bits([0.0, 0.0]))


def test_pow_guards_at_zero():
    """At a = 0 (b > 0): gb is +0.0, not 0 * -inf; with beta < 1 the infinite ga against da = -0.0 gives 0, not NaN."""
    t = np.array([0.0, 0.5, 2.0])
    v, J = _vj("a*pow(t,b)+c", "a,b,c", [1.3, 0.7, 0.2], t)
    assert np.isfinite(J).all() and np.array_equal(_bits(J[0]), _bits([0.0, 0.0, 1.0])) and v[0] == 0.2
    assert J[1, 1] == 1.3 * (np.power(0.5, 0.7) * np.log(0.5))
    v, J = _vj("a*exp(-pow(t/tau,beta))+c", "a,tau,beta,c", [1.3, 1.1, 0.6, 0.1], t)
    assert np.isfinite(J).all() and np.array_equal(_bits(J[0]), _bits([1.0, -0.0, -0.0, 1.0])) and v[0] == 1.3 + 0.1
    # without the guards the same row is NaN: the workaround's analytic column
    v, J = _vj("a*exp(b*log(t))+c", "a,b,c", [1.3, 0.7, 0.2], t)
    assert v[0] == 0.2 and np.isnan(J[0, 1]) and np.isfinite(J[1:]).all()
    # a negative base with a fitted exponent is outside the domain: NaN in b's column only
    v, J = _vj("pow(t-p,b)", "p,b", [3.0, 2.0], t)
    assert np.array_equal(_bits(v), _bits([9.0, 6.25, 1.0])) and np.isnan(J[:, 1]).all() and np.array_equal(_bits(J[:, 0]), _bits([6.0, 5.0, 2.0]))


# ------------------------------------------------------------------------------------------------ 5. presence patterns
@pytest.mark.parametrize("formula,params", PC.PATTERNS)
def test_presence_patterns(formula, params):
    """Each pattern's Jacobian is the table's form for the operands that carry a tangent, an absent one dropped; a column
    that only the condition of a where names is present and +0.0."""
    e = _expr(formula, "t", params)
    names = params.split(",")
    x = np.array([PC.PATTERN_X[k] for k in names])
    t = np.linspace(0.0, 3.0, 49)                                      # t = 1.25 is in it: where's c = 0
    env = dict(zip(names, x))
    f, rest = formula.split("(", 1)
    args = rest[:-1].split(",")
    masks = [int(k) for k in e.program()[3]]
    assert masks[-1] == (1 << len(names)) - 1
    J = W.jacobian(e.program(), x, [t])
    v = W.value(e.program(), x, [t])

    def operand(text):
        """(value, {name: tangent}) of an operand: these are affine in every parameter or q*q, so eval and a hand rule do."""
        val = eval(text, {"__builtins__": {}}, dict(env, t=t)) + np.zeros(49)
        tan = {}
        for k in names:
            if k in text:
                if text == "q*q":
                    tan[k] = 1.0 * env["q"] + env["q"] * 1.0 + np.zeros(49)
                elif text.startswith(k + "*t"):
                    tan[k] = 1.0 * t
                elif "-" + k in text:
                    tan[k] = -np.ones(49)
                else:
                    tan[k] = np.ones(49)
        return val, tan

    ops = [operand(a) for a in args]
    for j, k in enumerate(names):
        if f == "where":
            (c, _), (a, da), (b, db) = ops
            want = np.where(c >= 0.0, da.get(k, np.zeros(49)), db.get(k, np.zeros(49)))
            assert np.array_equal(_bits(v), _bits(np.where(c >= 0.0, a, b)))
        else:
            (a, da), (b, db) = ops
            ha, hb = k in da, k in db
            with np.errstate(all="ignore"):
                if f in ("min", "max"):
                    s = b > a if f == "max" else b < a
                    want = np.where(s, db.get(k, np.zeros(49)), da.get(k, np.zeros(49)))
                    assert np.array_equal(_bits(v), _bits(np.where(s, b, a)))
                elif f == "atan2":
                    den = a * a + b * b
                    want = (b * da[k] - a * db[k]) / den if ha and hb else ((b * da[k]) / den if ha else -((a * db[k]) / den))
                else:
                    pv = np.power(a, b)
                    ta = np.where(da[k] == 0.0, 0.0, (b * np.power(a, b - 1.0)) * da[k]) if ha else None
                    tb = np.where(pv == 0.0, 0.0, pv * np.log(a)) * db[k] if hb else None
                    want = ta + tb if ha and hb else (ta if ha else tb)
        assert np.array_equal(_bits(J[:, j]), _bits(want)), (formula, k)
    if formula == "where(t-p,1+t,2)":
        assert np.array_equal(_bits(J[:, 0]), _bits(np.zeros(49)))


# ------------------------------------------------------------------------------------------------ 6. central differences
@pytest.mark.parametrize("name", PC.WITH_FUNCTIONS)
def test_pow_and_atan2_jacobian_against_central_differences(name):
    """Central differences with h = 2^-20 |x_j| of the restated value, as tests/test_specfun_cpu.py has them for the erf
    family: truncation h^2/6 |f'''| and rounding eps |f|/h both stay under 1e-7 of the column's largest entry on these
    formulas away from t = 0, where pow(t, b) has no third derivative in b to speak of (the abscissae are the jittered grid,
    t >= 0.01); the running bound of the analytic column is added."""
    m = 64
    prog, t, y, xt, x0 = PC.problems(name, m, nprob=3)
    for p in range(3):
        tv = t[:, p]
        J, eJ = W.jacobian_bound(prog, x0[p], tv)
        assert np.array_equal(_bits(J), _bits(W.jacobian(prog, x0[p], tv)))
        for j in range(J.shape[1]):
            h = 2.0 ** -20 * abs(x0[p][j])
            xp, xm = x0[p].copy(), x0[p].copy()
            xp[j] += h
            xm[j] -= h
            col = (W.value(prog, xp, tv) - W.value(prog, xm, tv)) / (xp[j] - xm[j])
            bound = 1e-7 * np.abs(col).max() + eJ[:, j]
            assert (np.abs(J[:, j] - col) <= bound).all(), (name, p, j, (np.abs(J[:, j] - col) / bound).max())


def test_running_bound_and_old_instructions():
    """On the 22 old instructions this restatement is the existing ones': the same bits on their own formulas, plain and
    tracked; the exact formulas here have bound 0, the library-function ones a small positive one."""
    import expr_cases as EC
    import specfun_cases as SC
    for name in EC.FORMULAS:
        prog, t, y, xt, x0 = EC.expr_problems(name, 225 if name == "gauss2d" else 64, nprob=1)
        assert np.array_equal(_bits(W.residual(prog, x0[0], t[:, 0], y[0])), _bits(R.residual(prog, x0[0], t[:, 0], y[0])))
        assert np.array_equal(_bits(W.jacobian(prog, x0[0], t[:, 0])), _bits(R.jacobian(prog, x0[0], t[:, 0])))
        for got, want in zip(W.residual_bound(prog, x0[0], t[:, 0], y[0]) + W.jacobian_bound(prog, x0[0], t[:, 0]),
                             R.residual_bound(prog, x0[0], t[:, 0], y[0]) + R.jacobian_bound(prog, x0[0], t[:, 0])):
            assert np.array_equal(_bits(got), _bits(want)), name
    for name in SC.FORMULAS:
        prog, t, y, xt, x0 = SC.problems(name, 64, nprob=1)
        assert np.array_equal(_bits(W.residual(prog, x0[0], t[:, 0], y[0])), _bits(S.residual(prog, x0[0], t[:, 0], y[0])))
        assert np.array_equal(_bits(W.jacobian(prog, x0[0], t[:, 0])), _bits(S.jacobian(prog, x0[0], t[:, 0])))
        for got, want in zip(W.residual_bound(prog, x0[0], t[:, 0], y[0]) + W.jacobian_bound(prog, x0[0], t[:, 0]),
                             S.residual_bound(prog, x0[0], t[:, 0], y[0]) + S.jacobian_bound(prog, x0[0], t[:, 0])):
            assert np.array_equal(_bits(got), _bits(want)), name
    for name in PC.EXACT + PC.WITH_FUNCTIONS:
        prog, t, y, xt, x0 = PC.problems(name, 64, nprob=1, zero=name != "phase")
        r, e = W.residual_bound(prog, x0[0], t[:, 0], y[0])
        J, eJ = W.jacobian_bound(prog, x0[0], t[:, 0])
        assert np.array_equal(_bits(r), _bits(W.residual(prog, x0[0], t[:, 0], y[0])))
        assert np.array_equal(_bits(J), _bits(W.jacobian(prog, x0[0], t[:, 0])))
        assert np.isfinite(e).all() and np.isfinite(eJ).all() and np.isfinite(J).all()
        if name in PC.EXACT:
            assert (e == 0.0).all() and (eJ == 0.0).all(), name
        else:
            assert (e[1:] > 0.0).all() and (e <= 1e-9 * np.abs(y[0]).max()).all(), name


# ------------------------------------------------------------------------------------------------ 7. fits on the oracle
@pytest.fixture(scope="module")
def fits():
    return PC.fit_problems()


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("name", [c[0] for c in PC.FIT_CASES])
def test_fits_on_the_oracle(oracle, fits, name, analytic):
    """64 problems of each form, t = 0 in the grid of the power law and the stretched exponential: every solve returns 0, with
    forward differences and with the analytic Jacobian."""
    prog, t, y, xt, x0 = fits[name]
    assert t[0] == 0.0 and len(t) == dict(PC.FIT_CASES)[name] and y.shape[0] == 64
    rcs, worst = [], 0.0
    for p in range(len(y)):
        rc, x, f, ib = PC.oracle_fit(oracle, prog, t, y[p], x0[p], analytic)
        rcs.append(rc)
        if rc == 0:
            worst = max(worst, float(np.abs(x / xt[p] - 1.0).max()))
    print(f"{name} analytic={analytic}: rc = 0 in {rcs.count(0)} of {len(rcs)}, worst |x/x_true - 1| {worst:.3e}")
    assert rcs.count(0) == len(rcs), (name, analytic, rcs)


# ------------------------------------------------------------------------------------------------ 8. the recorded study
def test_recorded_study(oracle):
    """pow(t,b) against exp(b*log(t)) on the same data, analytic Jacobian, with and without the t = 0 row
    (tests/golden/pwfun_study.json, made by tests/golden/make_pwfun_study.py): the counts are the recording's, the
    statistics of b within 1e-9 (another C library's pow and log move the last bits of a fit, not its eighth digit).  With
    the t = 0 row no pow fit fails and every workaround fit does; without it the two forms agree."""
    got, want = PC.study(oracle), PC.recorded_study()
    print(got)
    assert set(got) == set(want)
    for k in want:
        assert got[k]["failed"] == want[k]["failed"] and got[k]["fitted"] == want[k]["fitted"], (k, got[k], want[k])
        for s in ("b_bias", "b_scatter"):
            assert (got[k][s] is None) == (want[k][s] is None) and (want[k][s] is None or abs(got[k][s] - want[k][s]) <= 1e-9), (k, s, got[k], want[k])
    assert want["powerlaw/with_t0"]["failed"] == 0 and want["powerlaw_explog/with_t0"]["failed"] == 64
    assert want["powerlaw/without_t0"]["failed"] == 0 and want["powerlaw_explog/without_t0"]["failed"] == 0


def _standard_errors(prog, x, tv, y):
    m, n = len(y), len(x)
    f, J = W.residual(prog, x, tv, y), W.jacobian(prog, x, tv)
    return np.sqrt(np.diag(np.linalg.inv(J.T @ J)) * (f @ f) / (m - n))


def test_recovery_seed_on_the_oracle(oracle):
    """The seed of the GPU recovery test: on the CPU oracle alone, in how many of the 64 noisy power laws every parameter is
    within 3 standard errors of its generating value.  tests/test_gpu_pwfun.py::test_recovery holds the device to 4 fewer."""
    prog, t, y, xt, x0 = PC.recovery_problems()
    good = 0
    for p in range(len(y)):
        rc, x, f, ib = PC.oracle_fit(oracle, prog, t, y[p], x0[p], True)
        assert rc == 0, (p, rc, ib)
        good += bool((np.abs(x - xt[p]) <= 3.0 * _standard_errors(prog, x, [t], y[p])).all())
    print("power-law recovery on the oracle:", good, "of", len(y))
    assert good == PC.RECOVERY_N
