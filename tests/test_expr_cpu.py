"""CPU tests of the formula models: what nlh_expr_compile makes of a formula (shapes, dependency masks, the exact postfix),
its refusals and limits, the error codes that need no device, and the numpy restatement the GPU tests compare the kernels
with (tests/expr_restatement.py) held to Python's own evaluation of the formula, to the curve models' restatement, to a
complex-step derivative of its own values and to the CPU oracle's solver on the generator's cases."""
import ctypes as C

import numpy as np
import pytest

import curve_cases as CC
import curve_restatement as CR
import expr_cases as EC
import expr_restatement as R

EPS = 2.0 ** -52
NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3
LORENTZ_HEADER = "0+a/(1.0+((t-mu)/w)*((t-mu)/w))+(c1*t+c0)"            # K = 1, B = 1 in the header's operation order
GAUSS_HEADER = "0+a*exp(-0.5*(((t-mu)/s)*((t-mu)/s)))+(c1*t+c0)"
HEADER_PARAMS = {"lorentz": "a,mu,w,c0,c1", "gauss": "a,mu,s,c0,c1"}


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _listing(e):
    op, arg, consts, mask = e.program()
    return [(R.OPS[o], int(a)) for o, a in zip(op, arg)]


def test_compile_shapes_and_masks():
    import nonlin_amd as nl
    assert nl.EXPR_OPS == R.OPS
    want = {"mm": (1, 2, 7, 0, 3), "hill": (1, 2, 10, 0, 3), "lorentz2": (1, 6, 33, 3, 6), "rational": (1, 5, 21, 1, 4),
            "gauss2d": (2, 5, 20, 1, 5), "dsine": (1, 5, 20, 2, 3)}
    for name, shape in want.items():
        e = EC.compile_formula(name)
        assert (e.nvar, e.nparams, e.ninstr, e.nconst, e.depth) == shape, (name, e.ninstr, e.nconst, e.depth)
        op, arg, consts, mask = e.program()
        assert len(op) == len(arg) == len(mask) == e.ninstr and len(consts) == e.nconst
        assert int(mask[-1]) == (1 << e.nparams) - 1                 # the root names every parameter
        for o, a, k in zip(op, arg, mask):                           # leaves: a parameter names itself, nothing else names any
            if o == R.PARAM:
                assert int(k) == 1 << int(a)
            elif o in (R.CONST, R.VAR):
                assert int(k) == 0
        e.close()
        e.close()                                                    # (closing twice is harmless)
    # a parameter the formula never names: its bit is in no mask; every literal and every pi is a constant of its own
    e = nl.Expr("a*t+2+2+pi+pi", "t", "a,unused")
    op, arg, consts, mask = e.program()
    assert int(mask[-1]) == 1 and e.nparams == 2 and list(consts) == [2.0, 2.0, np.pi, np.pi]


def test_exact_postfix_of_two_formulas():
    import nonlin_amd as nl
    e = nl.Expr("-a^2 + b*(t - 1.5e0)/ +c ^-3", ("t",), ("a", "b", "c"))
    assert _listing(e) == [("PARAM", 0), ("IPOW", 2), ("NEG", 0), ("PARAM", 1), ("VAR", 0), ("CONST", 0), ("SUB", 0), ("MUL", 0),
                           ("PARAM", 2), ("IPOW", -3), ("DIV", 0), ("ADD", 0)]
    op, arg, consts, mask = e.program()
    assert list(consts) == [1.5] and [int(k) for k in mask] == [1, 1, 1, 2, 0, 0, 0, 2, 4, 4, 6, 7] and e.depth == 4
    e = nl.Expr("sqrt(x^0.5) - y^17 * exp(-k*x) / abs(q^-1)", "x, y", "k, q")
    assert _listing(e) == [("VAR", 0), ("POWC", 0), ("SQRT", 0), ("VAR", 1), ("POWC", 1), ("PARAM", 0), ("NEG", 0), ("VAR", 0), ("MUL", 0),
                           ("EXP", 0), ("MUL", 0), ("PARAM", 1), ("POWC", 2), ("ABS", 0), ("DIV", 0), ("SUB", 0)]
    assert list(e.program()[2]) == [0.5, 17.0, -1.0] and (e.nvar, e.nparams) == (2, 2)


PY_FORMULAS = ["a*t+b", "a-b-c-t", "a/b/c*t", "-a^2+t", "(a+b)*(c-t)/(a*t+1)", "sqrt(a*a+t^2)-abs(b-t)", "-(-a)*-t+ +b",
               "a/(1+((t-b)/c)^2)", "abs(-sqrt(abs(a-t)))/3+0.1*t", "a-(b-(c-(t-1)))", "1/3*a+2/7*t-b*1e-3"]


@pytest.mark.parametrize("formula", PY_FORMULAS)
def test_values_are_pythons_own_evaluation(formula):
    """Over + - * /, unary minus, parentheses, sqrt, abs and ^2 the stated order is Python's: eval of the same string on
    float64 arrays (^ as **) gives the interpreter's bits."""
    import nonlin_amd as nl
    rng = np.random.default_rng(len(formula))
    e = nl.Expr(formula, "t", "a,b,c")
    t = rng.uniform(-2.0, 2.0, 500)
    for _ in range(3):
        x = rng.uniform(-2.0, 2.0, 3)
        env = {"t": t, "a": np.float64(x[0]), "b": np.float64(x[1]), "c": np.float64(x[2]), "sqrt": np.sqrt, "abs": np.abs}
        with np.errstate(invalid="ignore"):
            want = eval(formula.replace("^", "**"), {"__builtins__": {}}, env)
            got = R.value(e.program(), x, [t])
        assert np.array_equal(_bits(got), _bits(want)), formula


@pytest.mark.parametrize("kind,formula", [("lorentz", LORENTZ_HEADER), ("gauss", GAUSS_HEADER)])
def test_header_order_formulas_are_the_curve_models(kind, formula):
    import nonlin_amd as nl
    e = nl.Expr(formula, "t", HEADER_PARAMS[kind])
    t, y, xt, x0 = CC.curve_problems(kind, 1, 1, 301, nprob=4)
    w = np.random.default_rng(3).uniform(0.5, 2.0, t.shape)
    for p in range(4):
        for wp in (None, w[p]):
            a = R.residual(e.program(), x0[p], [t[p]], y[p], wp)
            b = CR.residual(CR.KINDS[kind], 1, 1, x0[p], t[p], y[p], wp)
            assert np.array_equal(_bits(a), _bits(b)), (kind, p)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", list(EC.FORMULAS))
def test_analytic_jacobian_against_complex_step(name, weighted):
    """Every operation of the table is analytic in x where the generator puts it (abs stays away from 0): Im value(x + i h e_j)
    / h is the derivative to rounding.  The bound is test_curve_cpu.py's: 64 eps |entry| + 64 eps times the column's largest."""
    m = 225 if name == "gauss2d" else 200
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=3)
    rng = np.random.default_rng(5)
    h = 1e-30
    for p in range(3):
        tv = t[:, p]
        w = rng.uniform(0.5, 2.0, m) if weighted else None
        J = R.jacobian(prog, x0[p], tv, w)
        assert J.shape == (m, x0.shape[1])
        for j in range(J.shape[1]):
            xc = x0[p].astype(np.complex128)
            xc[j] += 1j * h
            col = R.residual(prog, xc, tv, y[p], w).imag / h
            bound = 64 * EPS * np.abs(col) + 64 * EPS * np.abs(col).max()
            assert (np.abs(J[:, j] - col) <= bound).all(), (name, p, j, (np.abs(J[:, j] - col) / bound).max())


def test_exact_programs_have_bound_zero():
    """The running bound of a formula without library functions is 0 (bit equality is what it claims); with one it is not."""
    for name in EC.FORMULAS:
        prog, t, y, xt, x0 = EC.expr_problems(name, 225 if name == "gauss2d" else 64, nprob=1)
        r, e = R.residual_bound(prog, x0[0], t[:, 0], y[0])
        J, eJ = R.jacobian_bound(prog, x0[0], t[:, 0])
        assert np.array_equal(_bits(r), _bits(R.residual(prog, x0[0], t[:, 0], y[0]))) and np.array_equal(_bits(J), _bits(R.jacobian(prog, x0[0], t[:, 0])))
        if name in EC.EXP_FREE:
            assert (e == 0.0).all() and (eJ == 0.0).all(), name
        else:
            assert (e > 0.0).all() and (e <= 1e-9 * np.abs(y[0]).max()).all(), name


REFUSALS = [("a+foo", "t", "a", "col 2: unknown name 'foo'"), ("a^2^3", "t", "a", "col 3"), ("a+", "t", "a", "col 2"), ("(a+t", "t", "a", "col 4"),
            ("a t", "t", "a", "col 2"), ("a+*t", "t", "a", "col 2"), ("exp a", "t", "a", "col 4"), ("a^b", "t", "a,b", "col 2"),
            ("a^(2)", "t", "a", "col 2"), ("a$t", "t", "a", "col 1"), ("", "t", "a", "col 0"), ("a+sinh(t)", "t", "a", "col 2: unknown name 'sinh'"),
            ("a", "", "a", "vars col 0"), ("a", "t", "", "params col 0"), ("a", "t,t", "a", "vars col 2"), ("a", "t", "a,b,a", "params col 4"),
            ("a", "t", "a,t", "params col 2"), ("a", "t", "a,,b", "params col 2"), ("a", "t,", "a", "vars col 2"), ("a", "t", "pi", "params col 0"),
            ("a", "exp", "a", "vars col 0"), ("a", "t,u,v,w,z", "a", "vars col 8"), ("a", "t", "2a", "params col 0")]


@pytest.mark.parametrize("formula,vars,params,message", REFUSALS)
def test_refusals_name_the_column(formula, vars, params, message):
    from nonlin_amd import _lib
    import nonlin_amd as nl
    L = _lib.load()
    e = C.c_void_p(7)
    assert L.nlh_expr_compile(formula.encode(), vars.encode(), params.encode(), C.byref(e)) == NL_INVALID_INPUT_ERROR
    assert not e.value and L.nlh_expr_error().decode().startswith(message), L.nlh_expr_error()
    with pytest.raises(ValueError, match="col [0-9]+: "):
        nl.Expr(formula, vars, params)


def test_limits_at_their_edges():
    import nonlin_amd as nl
    plist = ",".join("p%d" % k for k in range(33))
    e = nl.Expr("-a" + "+a" * 127, "t", "a")                        # 128 PARAM, 127 ADD, 1 NEG
    assert e.ninstr == 256
    with pytest.raises(ValueError, match="col 257: more than 256 instructions"):
        nl.Expr("-a" + "+a" * 127 + "+t", "t", "a")
    deep = lambda d: "a+(" * (d - 1) + "a" + ")" * (d - 1)
    assert nl.Expr(deep(16), "t", "a").depth == 16
    with pytest.raises(ValueError, match="deeper than 16"):
        nl.Expr(deep(17), "t", "a")
    assert nl.Expr("a" + "+1" * 64, "t", "a").nconst == 64
    with pytest.raises(ValueError, match="more than 64 constants"):
        nl.Expr("a" + "+1" * 65, "t", "a")
    e = nl.Expr("p31-p0", "t", plist[:plist.rindex(",")])
    assert e.nparams == 32 and int(e.program()[3][-1]) == (1 << 31) | 1
    with pytest.raises(ValueError, match="params col [0-9]+: more than 32 names"):
        nl.Expr("p0", "t", plist)
    assert nl.Expr("a*x*y*z*u", "x,y,z,u", "a").nvar == 4
    # exponents: integers 2 .. 16 of either sign are products, every other literal is pow
    for text, ins in (("a^2", ("IPOW", 2)), ("a^16", ("IPOW", 16)), ("a^-16", ("IPOW", -16)), ("a^2.0", ("IPOW", 2)), ("a^1", ("POWC", 0)),
                      ("a^17", ("POWC", 0)), ("a^-1", ("POWC", 0)), ("a^0", ("POWC", 0)), ("a^2.5", ("POWC", 0))):
        assert _listing(nl.Expr(text, "t", "a"))[-1] == ins, text


def test_error_codes_without_a_device():
    from nonlin_amd import _lib
    import nonlin_amd as nl
    L = _lib.load()
    e = nl.Expr("a*exp(-k*t)+c", "t", "a,k,c")
    md = C.c_void_p(7)
    one = np.ones(8)
    p = one.ctypes.data_as(_lib.c_double_p)
    o = _lib.default_options()
    assert L.nlh_expr_model_create(None, e.ptr, 1, 8, p, 0, p, None, 1, C.byref(md)) == NLH_ERR_BAD_HANDLE
    assert not md.value                                              # nothing is handed out
    assert L.nlh_expr_eval_batch(None, e.ptr, 1, 8, None, 0, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_fit_batch(None, C.byref(o), e.ptr, 1, 8, None, 0, None, None, 1, None, None, None, None, None, None, None, None, None,
                                None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_fit_batch_h(None, C.byref(o), e.ptr, 1, 8, p, 0, p, None, 1, None, None, p, p, None, None, None, None, None,
                                  None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_program(None, None, None, None) == NL_INVALID_INPUT_ERROR and L.nlh_expr_masks(e.ptr, None) == NL_INVALID_INPUT_ERROR
    L.nlh_expr_destroy(None)
    # a malformed context is refused by the launchers before any launch (no device is touched: this runs without one)
    two = nl.Expr("a*x+k*y+c", "x,y", "a,k,c")
    for fn in (L.nlh_expr_device_fcn, L.nlh_expr_device_jac):
        assert fn(None, None, 1, None, 3, None, 8, None) == NL_INVALID_INPUT_ERROR
        for ex, n, m, dt, dy, stride in ((None, 3, 8, 1, 1, 0), (e.ptr, 4, 8, 1, 1, 0), (e.ptr, 2, 8, 1, 1, 0), (e.ptr, 3, 9, 1, 1, 0),
                                         (e.ptr, 3, 8, None, 1, 0), (e.ptr, 3, 8, 1, None, 0), (two.ptr, 3, 8, 1, 1, 0), (two.ptr, 3, 8, 1, 1, 7)):
            ctx = _lib.ExprCtx(ex, 0, 8, dt, dy, None, stride)        # (non-NULL addresses that are never read)
            assert fn(C.byref(ctx), None, 1, 1, n, 1, m, 1) == NL_INVALID_INPUT_ERROR, (n, m, dt, dy, stride)
        ctx = _lib.ExprCtx(e.ptr, 0, 8, 1, 1, None, 0)
        assert fn(C.byref(ctx), None, 1, None, 3, 1, 8, 1) == NL_INVALID_INPUT_ERROR      # no problem list
        assert fn(C.byref(ctx), None, 0, 1, 3, 1, 8, 1) == 0                              # nothing to do is not an error


@pytest.mark.parametrize("analytic", [False, True])
def test_reference_solver_fits_the_generated_cases(oracle, analytic):
    """The generator's exp-free problems are ones the reference's lss_solve solves with the restatement as callback: every
    problem counted, nothing masked, 1 <= jacobian_count <= 30."""
    solved = 0
    for name, m in EC.SOLVE_CASES:
        prog, t, y, xt, x0 = EC.expr_problems(name, m)
        n = x0.shape[1]
        o = oracle.default_options(max_evals=EC.MAX_EVALS)
        for p in range(EC.NPROB):
            tv = t[:, p]
            fcn = lambda x, f: f.__setitem__(slice(None), R.residual(prog, x, tv, y[p]))
            jac = (lambda x, J: J.__setitem__((slice(None), slice(None)), R.jacobian(prog, x, tv))) if analytic else None
            rc, x, f, ib = oracle.lm_solve(fcn, m, n, x0[p], jac=jac, opts=o)
            assert rc == 0 and 1 <= ib["jacobian_count"] <= 30, (name, p, rc, ib)
            assert np.abs(f).max() <= 2e-3 * np.abs(y[p]).max(), (name, p)       # the noise level: a fit, not a stall
            solved += 1
    assert solved == len(EC.SOLVE_CASES) * EC.NPROB
