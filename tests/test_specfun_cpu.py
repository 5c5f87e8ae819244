"""CPU tests of the formulas' special functions (erf, erfc, erfcx, voigt; nlh_faddeeva): what the compiler makes of them and
what it refuses, the Faddeeva constants against their FFT derivation, the host entry bit for bit against the numpy
restatement (tests/specfun_restatement.py), the restatement against the 40-digit fixture
(tests/golden/specfun_reference.npz), its tangents against complex-step and central-difference columns, the seven presence
patterns of VOIGT's tangent, the ABS rule for negative sigma and gamma, and the recovery seed on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import expr_restatement as R
import specfun_cases as SC
import specfun_restatement as S

EPS = 2.0 ** -52
NL_INVALID_INPUT_ERROR = 201
MEASURED, BOUND = SC.MEASURED, SC.BOUND


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _listing(e):
    op, arg, consts, mask = e.program()
    return [(S.OPS[o], int(a)) for o, a in zip(op, arg)]


# ------------------------------------------------------------------------------------------------ the compiler
def test_compile_and_read_back():
    import nonlin_amd as nl
    assert nl.EXPR_OPS == R.OPS and len(nl.EXPR_OPS) == 18                       # the existing tuple stays what it is
    assert nl.EXPR_SPECIAL_OPS == ("ERF", "ERFC", "ERFCX", "VOIGT") == S.OPS[18:]
    assert (S.ERF, S.ERFC, S.ERFCX, S.VOIGT) == (18, 19, 20, 21)
    e = nl.Expr("a*voigt(t-mu,s,g)+c", "t", "a,mu,s,g,c")
    assert _listing(e) == [("PARAM", 0), ("VAR", 0), ("PARAM", 1), ("SUB", 0), ("PARAM", 2), ("PARAM", 3), ("VOIGT", 0), ("MUL", 0),
                           ("PARAM", 4), ("ADD", 0)]
    op, arg, consts, mask = e.program()
    assert [int(k) for k in mask] == [1, 0, 2, 2, 4, 8, 14, 15, 16, 31] and e.depth == 4 and e.nconst == 0
    aroot, broot = e.roots()
    assert (aroot[6], broot[6]) == (3, 4)                              # x's producer: the SUB; sigma's: PARAM s; gamma's is pc - 1
    assert aroot[7] == 0 and aroot[9] == 7 and not broot[[0, 1, 2, 3, 4, 5, 7, 8, 9]].any()
    # operands that are subtrees of their own: the roots are the subtrees' last instructions
    e = nl.Expr("voigt(t, s*2, (g+1)*s)", "t", "s,g")
    assert _listing(e) == [("VAR", 0), ("PARAM", 0), ("CONST", 0), ("MUL", 0), ("PARAM", 1), ("CONST", 1), ("ADD", 0), ("PARAM", 0),
                           ("MUL", 0), ("VOIGT", 0)]
    aroot, broot = e.roots()
    assert (aroot[9], broot[9]) == (0, 3) and [int(k) for k in e.program()[3]] == [0, 1, 0, 1, 2, 0, 2, 1, 3, 3] and e.depth == 4
    for k, f in enumerate(("erf", "erfc", "erfcx")):
        e = nl.Expr(f"a*{f}(k*t)", "t", "a,k")
        assert _listing(e) == [("PARAM", 0), ("PARAM", 1), ("VAR", 0), ("MUL", 0), (f.upper(), 0), ("MUL", 0)]
        assert int(e.program()[0][4]) == 18 + k and e.depth == 3
    # nesting, and the depth a VOIGT leaves behind: three operands on top of a
    assert nl.Expr("a+voigt(erf(t),erfc(s),erfcx(s))", "t", "a,s").depth == 4


REFUSALS = [("voigt(t,s)", "t", "s,g", "col 9: 'voigt' takes three arguments"), ("voigt(t,s,g,g)", "t", "s,g", "col 11: 'voigt' takes three"),
            ("erf(t,s)", "t", "s", "col 5: 'erf' takes one argument"), ("erf t", "t", "s", "col 4: '(' expected"),
            ("voigt(t)", "t", "s", "col 7: 'voigt' takes three"), ("s+erfcx(t,)", "t", "s", "col 9"),
            ("t", "t", "s,erfc", "params col 2: 'erfc' is a function"), ("t", "voigt", "s", "vars col 0: 'voigt' is a function"),
            ("t", "t", "erf", "params col 0: 'erf' is a function"), ("t", "t,erfcx", "s", "vars col 2: 'erfcx' is a function"),
            ("s+sinh(t)", "t", "s", "col 2: unknown name 'sinh'"), ("(t,s)", "t", "s", "col 2")]


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


# ------------------------------------------------------------------------------------------------ the Faddeeva function
def test_coefficient_table_is_weidemans():
    """The library's literals against the FFT derivation: 1e-15 relative per coefficient, plus 1e-15 of the largest one for the
    coefficients that are themselves at the rounding level of the transform (the first ones, about 1e-15)."""
    L, a = S.table()
    L2, a2 = S.weideman_table()
    assert a.shape == (40,) and L == L2 == np.sqrt(40 / np.sqrt(2.0))
    assert (np.abs(a - a2) <= 1e-15 * np.abs(a2) + 1e-15 * np.abs(a2).max()).all()
    assert a[-1] == np.abs(a).max() and 2.8 < a[-1] < 3.0


def test_host_entry_bits_and_domain():
    import nonlin_amd as nl
    from nonlin_amd import _lib
    F = SC.fixture()
    wr, wi = S.faddeeva_w(F["w_re"], F["w_im"])
    got = nl.wofz(F["w_re"] + 1j * F["w_im"])
    assert np.array_equal(_bits(got.real), _bits(wr)) and np.array_equal(_bits(got.imag), _bits(wi))
    assert nl.wofz(0j) == complex(*S.faddeeva_w(np.float64(0.0), np.float64(0.0))) and abs(nl.wofz(0j) - 1.0) < 4 * EPS
    L = _lib.load()
    a, b = C.c_double(7.0), C.c_double(7.0)
    for re, im in ((0.0, -1e-300), (1.0, -2.0), (0.0, float("nan"))):
        assert L.nlh_faddeeva(re, im, C.byref(a), C.byref(b)) == NL_INVALID_INPUT_ERROR and (a.value, b.value) == (7.0, 7.0)
    assert L.nlh_faddeeva(1.0, 1.0, None, C.byref(b)) == NL_INVALID_INPUT_ERROR
    assert L.nlh_faddeeva_batch(None, 1, None, None, None, None) == -3        # NLH_ERR_BAD_HANDLE: no device needed to say so
    with pytest.raises(ValueError):
        nl.wofz(1.0 - 1.0j)


def test_accuracy_against_the_fixture():
    F = SC.fixture()
    wr, wi = S.faddeeva_w(F["w_re"], F["w_im"])
    ref = F["w_wr"] + 1j * F["w_wi"]
    got = {"w": float((np.abs(wr + 1j * wi - ref) / np.abs(ref)).max())}
    v, gx, gs, gg = S.voigt(F["v_x"], F["v_s"], F["v_g"])
    peak, slope = F["v_peak"], F["v_peak"] / F["v_s"]
    got["v"] = float((np.abs(v - F["v"]) / peak).max())
    for k, g in (("gx", gx), ("gs", gs), ("gg", gg)):
        got[k] = float((np.abs(g - F["v_" + k]) / slope).max())
    print("specfun accuracy against the fixture:", {k: f"{v:.3e}" for k, v in got.items()})
    for k in BOUND:
        assert got[k] <= BOUND[k], (k, got[k], BOUND[k])
    assert (F["v_x"] == 0.0).sum() >= 50 and (F["w_re"] == 0.0).sum() >= 30       # the fixture holds x = 0


def test_numpy_side_of_the_erf_family():
    """What the running bound charges to this side: math.erf, math.erfc and the restatement's erfcx against the fixture."""
    F = SC.fixture()
    a = F["erf_a"]
    assert np.abs(a).max() == 26.0 and (np.abs(a) < 1.5).sum() > 1500
    for name, f in (("erf", S._erf), ("erfc", S._erfc), ("erfcx", S.erfcx)):
        ulp = float((np.abs(f(a) - F[name]) / np.spacing(np.abs(F[name]))).max())
        print(f"numpy-side {name}: {ulp:.1f} ulp")
        assert ulp <= S.NUMPY_F[name], (name, ulp)


# ------------------------------------------------------------------------------------------------ tangents
@pytest.mark.parametrize("name", SC.VOIGT_ONLY)
def test_voigt_jacobian_against_complex_step(name):
    """VOIGT is + - * / all the way down, so the restatement runs on complex numbers and Im value(x + i h e_j)/h is the
    derivative of the value the fixture checks.  The analytic column carries the error of the stated partials: the sigma
    partial's, 4 x 2.57e-11 of V(0)/sigma times the amplitude, dominates; a column's largest entry is of that size
    (|dV/dsigma| at the peak is about V(0)/sigma), hence BOUND["gs"] times twice the column's largest entry, beside the
    64 eps of tests/test_expr_cpu.py."""
    m = 129
    prog, t, y, xt, x0 = SC.problems(name, m, nprob=3)
    h = 1e-30
    for p in range(3):
        tv = t[:, p]
        J = S.jacobian(prog, x0[p], tv)
        for j in range(J.shape[1]):
            xc = x0[p].astype(np.complex128)
            xc[j] += 1j * h
            col = S.residual(prog, xc, tv, y[p]).imag / h
            bound = 64 * EPS * np.abs(col) + (64 * EPS + 2 * BOUND["gs"]) * np.abs(col).max()
            assert (np.abs(J[:, j] - col) <= bound).all(), (name, p, j, (np.abs(J[:, j] - col) / bound).max())


@pytest.mark.parametrize("name", SC.WITH_FUNCTIONS)
def test_erf_family_jacobian_against_central_differences(name):
    """math.erf takes no complex number: central differences with h = 2^-20 |x_j| of the restated value.  Truncation is
    h^2/6 |f'''| and rounding eps |f|/h: with the third derivatives of these formulas within 1e3 of the column's largest
    entry and |f| within 1e2 of it, both stay under 1e-7 of that entry; the running bound of the analytic column is far
    smaller and is added."""
    m = 64
    prog, t, y, xt, x0 = SC.problems(name, m, nprob=3)
    for p in range(3):
        tv = t[:, p]
        J, eJ = S.jacobian_bound(prog, x0[p], tv)
        assert np.array_equal(_bits(J), _bits(S.jacobian(prog, x0[p], tv)))
        for j in range(J.shape[1]):
            h = 2.0 ** -20 * abs(x0[p][j])
            xp, xm = x0[p].copy(), x0[p].copy()
            xp[j] += h
            xm[j] -= h
            col = (S.value(prog, xp, tv) - S.value(prog, xm, tv)) / (xp[j] - xm[j])
            bound = 1e-7 * np.abs(col).max() + eJ[:, j]
            assert (np.abs(J[:, j] - col) <= bound).all(), (name, p, j, (np.abs(J[:, j] - col) / bound).max())


def test_running_bound_is_zero_exactly_for_voigt_only_formulas():
    for name in SC.VOIGT_ONLY + SC.WITH_FUNCTIONS:
        prog, t, y, xt, x0 = SC.problems(name, 64, nprob=1)
        r, e = S.residual_bound(prog, x0[0], t[:, 0], y[0])
        J, eJ = S.jacobian_bound(prog, x0[0], t[:, 0])
        assert np.array_equal(_bits(r), _bits(S.residual(prog, x0[0], t[:, 0], y[0])))
        assert np.array_equal(_bits(J), _bits(S.jacobian(prog, x0[0], t[:, 0])))
        if name in SC.VOIGT_ONLY:
            assert (e == 0.0).all() and (eJ == 0.0).all(), name
        else:
            assert (e > 0.0).all() and (e <= 1e-9 * np.abs(y[0]).max()).all(), name


def test_old_instructions_are_the_existing_restatement():
    """The 18 old instructions here are the existing restatement's: the same bits on its own formulas."""
    import expr_cases as EC
    for name in EC.FORMULAS:
        prog, t, y, xt, x0 = EC.expr_problems(name, 225 if name == "gauss2d" else 64, nprob=1)
        assert np.array_equal(_bits(S.residual(prog, x0[0], t[:, 0], y[0])), _bits(R.residual(prog, x0[0], t[:, 0], y[0])))
        assert np.array_equal(_bits(S.jacobian(prog, x0[0], t[:, 0])), _bits(R.jacobian(prog, x0[0], t[:, 0])))


@pytest.mark.parametrize("formula,params", SC.PATTERNS)
def test_presence_patterns(formula, params):
    """Each pattern's Jacobian is the table's partials in the stated summation order: gx*dx, then + gs*dsigma, then + gg*dgamma,
    an absent operand dropped.  Here dx = -1 for mu (t - mu: SUB's -db), dsigma = 1 for s, dgamma = 1 for g or 0.5*1.0."""
    import nonlin_amd as nl
    e = nl.Expr(formula, "t", params)
    names = params.split(",")
    x = np.array([SC.PATTERN_X[k] for k in names])
    t = np.linspace(0.0, 10.0, 64)
    val = dict(zip(names, x))
    args = formula[len("voigt("):-1].split(",")
    xv = t - val["mu"] if "mu" in args[0] else t
    sv = np.full(64, val["s"]) if args[1] == "s" else np.full(64, 0.5)
    gv = np.full(64, val["g"]) if args[2] == "g" else (0.5 * sv if args[2] == "0.5*s" else np.full(64, 0.1))
    v, gx, gs, gg = S.voigt(xv, sv, gv)
    assert np.array_equal(_bits(S.value(e.program(), x, [t])), _bits(v))
    J = S.jacobian(e.program(), x, [t])
    for j, k in enumerate(names):
        if k == "mu":
            want = gx * -np.ones(64)
        elif k == "g":
            want = gg * np.ones(64)
        elif args[2] == "0.5*s":                                        # s reaches sigma and gamma: a * db of the MUL is 0.5 * 1.0
            want = gs * np.ones(64) + gg * (0.5 * np.ones(64))
        else:
            want = gs * np.ones(64)
        assert np.array_equal(_bits(J[:, j]), _bits(want)), (formula, k)
    masks = [int(k) for k in e.program()[3]]
    assert masks[-1] == (1 << len(names)) - 1


def test_negative_sigma_and_gamma():
    """The ABS rule: the value at the absolute values, the partial's sign flipped with its operand's."""
    import nonlin_amd as nl
    e = nl.Expr("voigt(t-mu,s,g)", "t", "mu,s,g")
    t = np.linspace(0.0, 10.0, 65)
    base = np.array([4.7, 0.45, 0.35])
    v0, J0 = S.value(e.program(), base, [t]), S.jacobian(e.program(), base, [t])
    for ss, sg in ((-1, 1), (1, -1), (-1, -1)):
        x = base * np.array([1.0, ss, sg])
        assert np.array_equal(_bits(S.value(e.program(), x, [t])), _bits(v0))
        J = S.jacobian(e.program(), x, [t])
        assert np.array_equal(_bits(J), _bits(J0 * np.array([1.0, ss, sg])))
    assert (v0 > 0).all() and abs(S.value(e.program(), base, [np.linspace(-400, 400, 400001)]).sum() * 0.002 - 1.0) < 2e-3      # unit area (the tails beyond 400: 6e-4)


# ------------------------------------------------------------------------------------------------ the solver's cases
def _standard_errors(prog, x, tv, y):
    m, n = len(y), len(x)
    f, J = S.residual(prog, x, tv, y), S.jacobian(prog, x, tv)
    return np.sqrt(np.diag(np.linalg.inv(J.T @ J)) * (f @ f) / (m - n))


def test_recovery_seed_on_the_oracle(oracle):
    """The seed of the GPU recovery test: on the CPU oracle alone, every parameter within 3 standard errors of its generating
    value in at least 60 of the 64 problems."""
    m, nprob = SC.RECOVERY_M, SC.RECOVERY_NPROB
    prog, t, y, xt, x0 = SC.problems("voigt1", m, nprob=nprob, seed=SC.RECOVERY_SEED, gaussian=SC.RECOVERY_NOISE)
    n = x0.shape[1]
    o = oracle.default_options(max_evals=SC.MAX_EVALS)
    good = 0
    for p in range(nprob):
        tv = t[:, p]
        fcn = lambda x, f: f.__setitem__(slice(None), S.residual(prog, x, tv, y[p]))
        jac = lambda x, J: J.__setitem__((slice(None), slice(None)), S.jacobian(prog, x, tv))
        rc, x, f, ib = oracle.lm_solve(fcn, m, n, x0[p], jac=jac, opts=o)
        assert rc == 0, (p, rc, ib)
        good += bool((np.abs(x - xt[p]) <= 3.0 * _standard_errors(prog, x, tv, y[p])).all())
    print("recovery on the oracle:", good, "of", nprob)
    assert good >= 60
