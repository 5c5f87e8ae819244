"""CPU tests of the robust losses (include/nonlin_hip.h: nlh_loss_*): the properties of the numpy restatement
(tests/loss_restatement.py) the header promises, the validation of the Python Loss, the error codes that need no device, and
the outlier family of tests/loss_cases.py on the CPU oracle's solver with the restated transform as a host callback."""
import ctypes as C

import numpy as np
import pytest

import curve_restatement as R
import loss_cases as LC
import loss_restatement as LR

EPS = 2.0 ** -52
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NLH_ERR_BAD_HANDLE = 201, 211, -3
dp = C.POINTER(C.c_double)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _residuals(rng, n, c):
    """Residuals on both sides of the scale, some exactly at it, zeros of both signs, tiny and large ones."""
    r = np.concatenate([c * rng.uniform(-1, 1, n), c * rng.uniform(-50, 50, n), c * np.exp(rng.uniform(-30, 30, n)) * rng.choice([-1, 1], n),
                        [c, -c, 0.0, -0.0, np.nextafter(c, 2 * c), -np.nextafter(c, 2 * c), np.nextafter(c, 0), 1e-200, -1e-200]])
    return r


def test_huber_is_the_identity_inside_the_scale():
    rng = np.random.default_rng(1)
    for c in (0.06, 1.0, 3.7e-5, 1e300):
        r = _residuals(rng, 500, min(c, 1e10))
        out, g, wgt = LR.apply(LR.HUBER, c, r)
        inside = np.fabs(r / c) <= 1.0
        assert inside.any()
        assert np.array_equal(_bits(out[inside]), _bits(r[inside]))
        assert (g[inside] == 1.0).all() and (wgt[inside] == 1.0).all()
        assert (np.fabs(out[~inside]) <= np.fabs(r[~inside]) * (1.0 + 2 * EPS)).all() and (g[~inside] <= 1.0).all() and (wgt[~inside] < 1.0).all()
    out, g, wgt = LR.apply(LR.HUBER, 1e300, r)
    assert np.array_equal(_bits(out), _bits(r))                         # a scale nothing reaches: the plain fit


@pytest.mark.parametrize("kind", ["linear", "huber", "soft_l1", "cauchy"])
def test_every_kind_is_odd_and_keeps_zero_rows(kind):
    rng = np.random.default_rng(2)
    k = LR.KINDS[kind]
    for c in (0.06, 2.5):
        r = _residuals(rng, 400, c)
        out, g, wgt = LR.apply(k, c, r)
        mo, mg, mw = LR.apply(k, c, -r)
        assert np.array_equal(_bits(mo), _bits(-out)) and np.array_equal(_bits(mg), _bits(g)) and np.array_equal(_bits(mw), _bits(wgt))
        assert (np.sign(out) == np.sign(r)).all() and (g > 0).all() and (wgt > 0).all() and (wgt <= 1.0).all()
    z = np.array([0.0, -0.0])
    for c in (0.06, 1.0, 1e300, np.array([0.5, 2.0])):
        out, g, wgt = LR.apply(k, c, z)
        assert np.array_equal(_bits(out), _bits(z)) and (g == 1.0).all() and (wgt == 1.0).all()   # zero-weight padding stays +-0


@pytest.mark.parametrize("kind", ["linear", "huber", "soft_l1", "cauchy"])
def test_sum_of_squares_is_the_robust_cost(kind):
    """sum out^2 = c^2 sum rho((r / c)^2), entry by entry against rho in extended precision.  out is sqrt(rho) after at most
    four roundings (u, the argument of the root, the root or log1p, the product with c), each within half an ulp -- one ulp
    for numpy's log1p --, so out^2 lies within 2 (4 + 1) eps of c^2 rho to first order, one more eps for the square."""
    rng = np.random.default_rng(3)
    k = LR.KINDS[kind]
    for c in (0.06, 1.0, 41.0):
        r = c * np.concatenate([rng.uniform(-1, 1, 300), rng.uniform(-60, 60, 300), np.exp(rng.uniform(-8, 8, 300))])
        out = LR.residual(k, c, r)
        cl, rl = np.longdouble(c), r.astype(np.longdouble)
        want = cl * cl * LR.rho(k, (rl / cl) ** 2)
        got = out.astype(np.longdouble) ** 2
        assert (np.abs(got - want) <= 11 * EPS * want).all(), (kind, c, float(np.max(np.abs(got - want) / want)) / EPS)
        assert abs(float(got.sum() - want.sum())) <= 11 * EPS * float(want.sum())


@pytest.mark.parametrize("kind", ["huber", "soft_l1", "cauchy"])
def test_g_is_the_derivative_of_out(kind):
    """g against a central difference of out with step h = 1e-5 c, away from Huber's kink: the difference's truncation error
    is h^2 |out'''| / 6 <= (1e-5)^2 / c^2 * c relative to a g of order 1 / 50 or more here, its rounding error eps |out| / h;
    both are below 1e-8 of g over these residuals (|r| <= 50 c), and 1e-7 is asserted."""
    rng = np.random.default_rng(4)
    k = LR.KINDS[kind]
    for c in (0.06, 1.0):
        r = c * np.concatenate([rng.uniform(-0.95, 0.95, 200), rng.uniform(1.05, 50, 200), -rng.uniform(1.05, 50, 200)])
        h = 1e-5 * c
        g = LR.apply(k, c, r)[1]
        fd = (LR.residual(k, c, r + h).astype(np.longdouble) - LR.residual(k, c, r - h).astype(np.longdouble)) / (2 * np.longdouble(h))
        assert (np.abs(fd - g) <= 1e-7 * g).all(), (kind, c, float(np.max(np.abs(fd - g) / g)))
    # the Jacobian rule: a row of J times its g
    J = rng.standard_normal((7, 3))
    r7 = rng.uniform(-3, 3, 7)
    assert np.array_equal(LR.jacobian(k, 1.0, r7, J), LR.apply(k, 1.0, r7)[1][:, None] * J)
    # wgt = rho'(z), against a central difference of rho in extended precision
    z = (np.concatenate([rng.uniform(0.01, 0.9, 100), rng.uniform(1.1, 400, 100)])).astype(np.longdouble)
    dz = np.longdouble(1e-6) * z
    wfd = (LR.rho(k, z + dz) - LR.rho(k, z - dz)) / (2 * dz)
    wgt = LR.apply(k, 1.0, np.sqrt(z).astype(np.float64))[2]
    assert (np.abs(wfd - wgt) <= 1e-9 * wgt + 4 * EPS).all()


def test_a_bad_scale_is_nan():
    r = np.array([0.5, -2.0, 0.0])
    for k in (LR.HUBER, LR.SOFT_L1, LR.CAUCHY):
        for c in (0.0, -1.0, np.inf, np.nan):
            for v in LR.apply(k, c, r):
                assert np.isnan(v).all(), (k, c)
        out, g, wgt = LR.apply(k, np.array([1.0, -1.0, 1.0]), r)
        assert np.isnan(out[1]) and not np.isnan(out[[0, 2]]).any()
    out, g, wgt = LR.apply(LR.LINEAR, np.nan, r)
    assert np.array_equal(out, r)


def test_loss_validation():
    import nonlin_amd as nl
    assert (nl.LOSS_LINEAR, nl.LOSS_HUBER, nl.LOSS_SOFT_L1, nl.LOSS_CAUCHY) == (LR.LINEAR, LR.HUBER, LR.SOFT_L1, LR.CAUCHY) == (0, 1, 2, 3)
    assert nl.LOSS_KINDS == LR.KINDS
    a = nl.Loss("huber", 0.06)
    assert (a.kind, a.shared, list(a.scale)) == (1, True, [0.06])
    assert a.scale_for(5)[1] == 1 and a.scale_for(1)[0].shape == (1,)
    b = nl.Loss(nl.LOSS_CAUCHY, [0.1, 0.2, 0.3])
    assert (b.kind, b.shared) == (3, False) and b.scale.dtype == np.float64 and b.scale_for(3)[1] == 0
    with pytest.raises(ValueError):
        b.scale_for(4)
    assert nl.Loss("Soft_L1", np.float32(2.0)).kind == 2 and nl.Loss("linear").kind == 0
    for bad in (("hubert", 1.0), (4, 1.0), (-1, 1.0), (1.5, 1.0), (None, 1.0), (True, 1.0), ("huber", 0.0), ("huber", -1.0),
                ("huber", float("inf")), ("huber", float("nan")), ("cauchy", [1.0, 0.0]), ("cauchy", [1.0, float("nan")]), ("soft_l1", []),
                ("soft_l1", [[1.0, 2.0]]), ("huber", "wide"), ("huber", None)):
        with pytest.raises(ValueError):
            nl.Loss(*bad)


def test_library_loads_and_refuses_device_work_without_a_handle():
    from nonlin_amd import _lib
    L = _lib.load()
    one = np.ones(16)
    p = one.ctypes.data_as(dp)
    o = _lib.default_options()
    out = C.c_void_p(7)
    fcn = C.cast(L.nlh_curve_device_fcn, _lib.DEVFCN)
    none = C.cast(None, _lib.DEVFCN)
    assert L.nlh_loss_wrap(None, 1, None, 0, fcn, none, None, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    assert L.nlh_loss_apply_batch(None, 1, 1, 1, None, 0, None, None, None, None) == NLH_ERR_BAD_HANDLE
    out = C.c_void_p(7)
    assert L.nlh_loss_model_create(None, None, 1, p, 1, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    for loss in (1, 0):                                                 # LINEAR is the _pmap entry point: its answer
        assert L.nlh_curve_fit_batch_loss(None, C.byref(o), 1, 1, -1, 1, 8, None, 0, None, None, 1, None, None, None, loss, None, 0, None, None,
                                          None, None, None, None, None, None) == NLH_ERR_BAD_HANDLE
        assert L.nlh_curve_fit_batch_loss_h(None, C.byref(o), 1, 1, -1, 1, 8, p, 0, p, None, 1, None, None, None, loss, p, 1, p, p, None, None,
                                            None, None, None, None) == NLH_ERR_BAD_HANDLE
        assert L.nlh_expr_fit_batch_loss(None, C.byref(o), None, 1, 8, None, 0, None, None, 1, None, None, None, loss, None, 0, None, None, None,
                                         None, None, None, None, None) == NLH_ERR_BAD_HANDLE
        assert L.nlh_expr_fit_batch_loss_h(None, C.byref(o), None, 1, 8, p, 0, p, None, 1, None, None, None, loss, p, 1, p, p, None, None, None,
                                           None, None, None) == NLH_ERR_BAD_HANDLE
    # a malformed context is refused by the launchers before any launch (no device is touched: this runs without one)
    for fn in (L.nlh_loss_device_fcn, L.nlh_loss_device_jac):
        assert fn(None, None, 1, None, 2, None, 8, None) == NL_INVALID_INPUT_ERROR
        junk = (C.c_uint32 * 64)()
        assert fn(C.byref(junk), None, 1, None, 2, 1, 8, 1) == NL_INVALID_INPUT_ERROR
    L.nlh_loss_unwrap(None)


def _solve(oracle, kind, t, y, x0, analytic=False, opts=None):
    k = LR.KINDS[kind]
    raw = lambda x: R.residual(R.LORENTZ, LC.K, LC.B, x, t, y)
    f = lambda x, out: out.__setitem__(slice(None), LR.residual(k, LC.SCALE, raw(x)))
    j = (lambda x, J: J.__setitem__((slice(None), slice(None)), LR.jacobian(k, LC.SCALE, raw(x), R.jacobian(R.LORENTZ, LC.K, LC.B, x, t)))) \
        if analytic else None
    rec = []
    rc, xo, fo, ib = oracle.lm_solve(f, len(t), 4, x0, jac=j, opts=opts, record=rec)
    return rc, xo, fo, ib, len(rec)


@pytest.mark.parametrize("m,nout", LC.FAMILIES)
def test_outlier_recovery_on_the_reference_path(oracle, m, nout):
    """The outlier family on the oracle's lm_solve under DEFAULT options, the restated transform as the callback, forward
    differences: for every problem, every robust kind solves with status 0 and its worst parameter error is below the plain
    fit's.  A condition, not a measurement: the family's seed is one for which it holds."""
    t, y, xt, x0 = LC.outlier_problems(m, nout)
    worst = {k: 0.0 for k in ("linear",) + LR.ROBUST}
    evals = 0
    for p in range(LC.NPROB):
        rc, xo, fo, ib, ne = _solve(oracle, "linear", t[p], y[p], x0[p])
        assert rc == 0, (p, rc)
        plain = float(np.abs(xo - xt[p]).max())
        worst["linear"] = max(worst["linear"], plain)
        for kind in LR.ROBUST:
            rc, xo, fo, ib, ne = _solve(oracle, kind, t[p], y[p], x0[p])
            err = float(np.abs(xo - xt[p]).max())
            assert rc == 0, (kind, p, rc)
            assert err < plain, (kind, p, err, plain)
            worst[kind] = max(worst[kind], err)
            evals = max(evals, ne)
    print(f"outliers m = {m}, {nout} per spectrum: worst parameter error " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items())
          + f"; at most {evals} residual evaluations per robust fit")
    assert all(worst[k] < worst["linear"] for k in LR.ROBUST)


def test_analytic_jacobian_reaches_the_same_fit(oracle):
    """The Jacobian rule (rows of J times g) in the oracle's solver: the same minimum as forward differences of the wrapped
    residual, to the solver's tolerance."""
    m, nout = LC.FAMILIES[0]
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=8)
    for kind in LR.ROBUST:
        for p in range(8):
            a = _solve(oracle, kind, t[p], y[p], x0[p], analytic=False)
            b = _solve(oracle, kind, t[p], y[p], x0[p], analytic=True)
            assert a[0] == b[0] == 0
            assert np.abs(a[1] - b[1]).max() < 1e-5, (kind, p, a[1], b[1])
