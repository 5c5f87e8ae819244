"""CPU tests of the built-in curve models: what nlh_curve_nparams answers, the error codes that need no device, and the
numpy restatement the GPU tests compare the kernels with (tests/curve_restatement.py) held to a complex-step derivative of
its own model and to the CPU oracle's solver on the generator's cases."""
import ctypes as C

import numpy as np
import pytest

import curve_cases as CC
import curve_restatement as R

EPS = 2.0 ** -52
NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3


def test_nparams_values_and_refusals():
    from nonlin_amd import _lib
    import nonlin_amd as nl
    L = _lib.load()
    assert (nl.CURVE_GAUSS, nl.CURVE_LORENTZ, nl.CURVE_EXPDECAY) == (R.GAUSS, R.LORENTZ, R.EXPDECAY) == (0, 1, 2)
    assert nl.CURVE_KINDS == R.KINDS
    for kind in (0, 1, 2):
        for K in (1, 2, 7, 100):
            for B in range(-1, 9):
                assert L.nlh_curve_nparams(kind, K, B) == R.nparams(kind, K, B) == (2 if kind == 2 else 3) * K + B + 1
    assert L.nlh_curve_nparams(R.GAUSS, 1, -1) == 3 and L.nlh_curve_nparams(R.EXPDECAY, 3, 8) == 15
    for bad in ((3, 1, 0), (-1, 1, 0), (0, 0, 0), (1, -2, 0), (2, 1, -2), (2, 1, 9), (0, 2731, -1), (0, 2 ** 30, 0)):
        assert L.nlh_curve_nparams(*bad) == -1, bad
    assert L.nlh_curve_nparams(0, 2730, 1) == 8192                 # the largest n a point's x is staged for
    for name, (kind, K, B, _) in zip(("gauss", "lorentz", "expdecay"), (CC.CASES[1], CC.CASES[4], CC.CASES[6])):
        assert nl.curve_nparams(name, K, B) == R.nparams(R.KINDS[name], K, B)
    with pytest.raises(ValueError):
        nl.curve_nparams("voigt", 1, -1)
    with pytest.raises(ValueError):
        nl.curve_nparams("gauss", 0, -1)


def test_error_codes_without_a_device():
    from nonlin_amd import _lib
    L = _lib.load()
    md = C.c_void_p(7)
    one = np.ones(8)
    p = one.ctypes.data_as(_lib.c_double_p)
    o = _lib.default_options()
    assert L.nlh_curve_model_create(None, 0, 1, -1, 1, 8, p, 0, p, None, 1, C.byref(md)) == NLH_ERR_BAD_HANDLE
    assert not md.value                                              # nothing is handed out
    assert L.nlh_curve_eval_batch(None, 0, 1, -1, 1, 8, None, 0, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_curve_fit_batch(None, C.byref(o), 0, 1, -1, 1, 8, None, 0, None, None, 1, None, None, None, None, None, None, None,
                                 None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_curve_fit_batch_h(None, C.byref(o), 0, 1, -1, 1, 8, p, 0, p, None, 1, None, None, p, p, None, None, None, None,
                                   None, None) == NLH_ERR_BAD_HANDLE
    # a malformed context is refused by the launchers before any launch (no device is touched: this runs without one)
    for fn in (L.nlh_curve_device_fcn, L.nlh_curve_device_jac):
        assert fn(None, None, 1, None, 3, None, 8, None) == NL_INVALID_INPUT_ERROR
        for kind, K, B, n, m in ((5, 1, -1, 3, 8), (0, 0, -1, 3, 8), (0, 1, 9, 13, 16), (0, 1, -2, 3, 8), (0, 1, -1, 4, 8), (2, 1, -1, 3, 8),
                                 (0, 1, -1, 3, 9)):
            ctx = _lib.CurveCtx(kind, K, B, 0, 8, 1, 1, None)        # (non-NULL addresses that are never read)
            assert fn(C.byref(ctx), None, 1, 1, n, 1, m, 1) == NL_INVALID_INPUT_ERROR, (kind, K, B, n, m)


@pytest.mark.parametrize("kind,K,B,m", CC.CASES)
@pytest.mark.parametrize("weighted", [False, True])
def test_analytic_jacobian_against_complex_step(kind, K, B, m, weighted):
    """The terms are analytic in x: Im model(x + i h e_j) / h is the derivative to rounding.  Bound: 64 eps |entry| + 64 eps
    times the largest entry of the column."""
    kd = R.KINDS[kind]
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=3)
    rng = np.random.default_rng(5)
    h = 1e-30
    for p in range(3):
        w = rng.uniform(0.5, 2.0, m) if weighted else None
        J = R.jacobian(kd, K, B, x0[p], t[p], w)
        assert J.shape == (m, R.nparams(kd, K, B))
        for j in range(J.shape[1]):
            xc = x0[p].astype(np.complex128)
            xc[j] += 1j * h
            col = R.residual(kd, K, B, xc, t[p], y[p], w).imag / h
            bound = 64 * EPS * np.abs(col) + 64 * EPS * np.abs(col).max()
            assert (np.abs(J[:, j] - col) <= bound).all(), (kind, p, j, (np.abs(J[:, j] - col) / bound).max())


def test_lorentz_restatement_is_the_user_family():
    """Without baseline and weights the Lorentzian is tests/user_models.py's lorentz_row_numpy, bit for bit."""
    import user_models as UM
    t, y, xt, x0 = CC.curve_problems("lorentz", 4, -1, 512, nprob=4)
    for p in range(4):
        a, b = R.residual(R.LORENTZ, 4, -1, x0[p], t[p], y[p]), UM.lorentz_row_numpy(x0[p], t[p], y[p])
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("analytic", [False, True])
def test_reference_solver_fits_the_generated_cases(oracle, analytic):
    """The generator's problems are ones the reference's lss_solve solves (every problem, nothing masked)."""
    for kind, K, B, m in (CC.CASES[0], CC.CASES[4], CC.CASES[5]):
        kd, n = R.KINDS[kind], R.nparams(R.KINDS[kind], K, B)
        t, y, xt, x0 = CC.curve_problems(kind, K, B, m)
        o = oracle.default_options(max_evals=CC.MAX_EVALS)
        for p in range(CC.NPROB):
            fcn = lambda x, f: f.__setitem__(slice(None), R.residual(kd, K, B, x, t[p], y[p]))
            jac = (lambda x, J: J.__setitem__((slice(None), slice(None)), R.jacobian(kd, K, B, x, t[p]))) if analytic else None
            rc, x, f, ib = oracle.lm_solve(fcn, m, n, x0[p], jac=jac, opts=o)
            assert rc == 0 and 1 <= ib["jacobian_count"] <= 30, (kind, p, rc, ib)
            assert np.abs(x - xt[p]).max() <= 0.05 * np.abs(xt[p]).max(), (kind, p)
