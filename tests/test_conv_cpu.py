"""CPU tests of the instrument-response fits (include/nonlin_hip.h: nlh_conv_*): the numpy restatement
(tests/conv_restatement.py) against a per-row scalar loop, numpy.convolve and an explicit Toeplitz product; the identities the
header promises; the validation of the Python Convolve; the error codes that need no device; and, on the CPU oracle's solver
with the restated transform as a host callback, the study of reconvolution against tail fitting and the perturbation study
recorded under tests/golden/."""
import ctypes as C
import json

import numpy as np
import pytest

import conv_cases as CV
import conv_restatement as CR
import curve_restatement as R

NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NLH_ERR_BAD_HANDLE = 201, 211, -3
dp = C.POINTER(C.c_double)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _toeplitz(m, k, origin, ext):
    """The m-by-m matrix of the transform: row i holds tap j at column s = i + origin - j (clamped under HOLD, where taps that
    meet on an edge column add up; dropped outside under ZERO)."""
    A = np.zeros((m, m))
    for i in range(m):
        for j in range(len(k)):
            s = i + origin - j
            if 0 <= s < m:
                A[i, s] += k[j]
            elif ext == CR.HOLD:
                A[i, min(max(s, 0), m - 1)] += k[j]
    return A


SHAPES = [(1, 1, 0), (1, 5, 2), (2, 3, 0), (5, 9, 4), (5, 9, 8), (17, 4, 1), (64, 64, 0), (64, 64, 63), (65, 33, 16), (130, 1, 0), (40, 32, 31)]


@pytest.mark.parametrize("ext", [CR.ZERO, CR.HOLD])
@pytest.mark.parametrize("m,L,origin", SHAPES)
def test_restatement_is_the_definition(m, L, origin, ext):
    """The loop over taps of whole-array operations gives the bits of the per-row scalar loop, and lies within the derived
    first-order bound 2 L 2^-53 sum |k_j v_s| per row of numpy.convolve (ZERO) and of the explicit Toeplitz product (both)."""
    rng = np.random.default_rng(100 * m + L)
    v, k = rng.standard_normal(m), rng.standard_normal(L)
    got = CR.convolve(v, k, origin, ext)
    assert np.array_equal(_bits(got), _bits(CR.scalar(v, k, origin, ext)))
    bd = CR.bound(v, k, origin, ext)
    assert (np.abs(got - _toeplitz(m, k, origin, ext) @ v) <= bd).all()
    if ext == CR.ZERO:
        assert (np.abs(got - np.convolve(v, k)[origin:origin + m]) <= bd).all()
    # a stack of columns and a kernel per problem: each column alone
    V, Kp = rng.standard_normal((3, 2, m)), rng.standard_normal((3, L))
    both = CR.jacobian(V, None, Kp, origin, ext)
    for p in range(3):
        for c in range(2):
            assert np.array_equal(_bits(both[p, c]), _bits(CR.scalar(V[p, c], Kp[p], origin, ext)))


def test_residual_jacobian_and_weights():
    """residual: mu = r + y (one add), c over mu, c - y, times w; Jacobian: c over each column, times w; a zero-weight row is
    +0.0 by bit pattern whatever the row holds."""
    rng = np.random.default_rng(5)
    m, n, L, o = 33, 4, 7, 2
    r, y, J, k = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal((n, m)), rng.standard_normal(L)
    w = rng.uniform(0.5, 2.0, m)
    w[[0, 7, m - 1]] = 0.0
    w[3] = -0.0
    for ext in (CR.ZERO, CR.HOLD):
        c = CR.convolve(r + y, k, o, ext)
        out, outw = CR.residual(r, y, None, k, o, ext), CR.residual(r, y, w, k, o, ext)
        assert np.array_equal(_bits(out), _bits(c - y))
        z = w == 0.0
        assert z.sum() == 4 and not _bits(outw[z]).any() and np.array_equal(_bits(outw[~z]), _bits((w * (c - y))[~z]))
        Jw = CR.jacobian(J, w, k, o, ext)
        for j in range(n):
            cj = CR.convolve(J[j], k, o, ext)
            assert not _bits(Jw[j][z]).any() and np.array_equal(_bits(Jw[j][~z]), _bits((w * cj)[~z]))
        Jn = J.copy()
        Jn[:, 7] = np.nan                                            # the row is still convolved: its neighbours see it
        assert not _bits(CR.jacobian(Jn, w, k, o, ext)[:, 7]).any() and np.isnan(CR.jacobian(Jn, w, k, o, ext)[:, 8]).all()


def test_identities():
    rng = np.random.default_rng(2)
    m = 50
    J = rng.standard_normal((3, m))
    J[0, 4], J[1, 9] = 0.0, -0.0
    # L = 1, k = [1.0]: unchanged up to the sign of zero (+0.0 + (-0.0) = +0.0)
    for ext in (CR.ZERO, CR.HOLD):
        c = CR.jacobian(J, None, [1.0], 0, ext)
        assert np.array_equal(c, J) and np.array_equal(_bits(c[J != 0]), _bits(J[J != 0])) and _bits(c[1, 9:10])[0] == 0
    # origin + 1 shifts the output by one row in the interior (the rows whose taps all lie inside under both origins)
    k = rng.standard_normal(6)
    for ext in (CR.ZERO, CR.HOLD):
        for o in range(5):
            a, b = CR.convolve(J, k, o, ext), CR.convolve(J, k, o + 1, ext)
            lo, hi = 5 - o, m - 1 - (o + 1)                          # row i of a: i + o - 5 >= 0; row i - 1 of b the same rows
            assert hi - lo > 30 and np.array_equal(_bits(b[:, lo - 1:hi]), _bits(a[:, lo:hi + 1]))
    # HOLD, a unit-sum kernel of powers of two: a constant passes exactly -- any constant when every partial sum is a power
    # of two, a constant of few bits for any such kernel
    for taps, consts in (([0.5, 0.5], [3.7, -1e-300, 1.1e300]), ([0.25, 0.25, 0.5], [3.7, np.pi]), ([0.125, 0.125, 0.25, 0.5], [np.e]),
                         ([0.5, 0.25, 0.125, 0.125], [3.0, -80.5])):
        for cst in consts:
            for o in range(len(taps)):
                v = np.full(9, cst)
                assert np.array_equal(_bits(CR.convolve(v, taps, o, CR.HOLD)), _bits(v)), (taps, cst, o)
    # ZERO: the same constant ramps up over the first taps of a causal kernel
    ramp = CR.convolve(np.full(9, 3.0), [0.5, 0.25, 0.125, 0.125], 0, CR.ZERO)
    assert list(ramp[:4]) == [1.5, 2.25, 2.625, 3.0] and (ramp[3:] == 3.0).all()


def test_convolve_validation():
    import nonlin_amd as nl
    c = nl.Convolve([0.25, 0.5, 0.25])
    assert (c.L, c.origin, c.ext, c.shared) == (3, 0, CR.ZERO, True) and c.kernel.shape == (1, 3)
    c = nl.Convolve(np.ones((4, 5)), origin=2, extend="hold")
    assert (c.L, c.origin, c.ext, c.shared) == (5, 2, CR.HOLD, False) and c.kernel_for(4)[0].shape == (4, 5) and c.kernel_for(4)[1] == 0
    with pytest.raises(ValueError):
        c.kernel_for(3)
    assert nl.Convolve([1.0], extend="ZERO").ext == nl.CONV_ZERO == 0 and nl.Convolve([1.0], extend=nl.CONV_HOLD).ext == nl.CONV_HOLD == 1
    assert nl.Convolve(np.ones(CR.MAX_L)).L == CR.MAX_L and nl.Convolve([1, 2, 3], origin=np.int64(2)).origin == 2
    k = np.array([0.1, 0.7, 0.3, 1e-3])
    tot = 0.0
    for v in k:
        tot = tot + v
    assert np.array_equal(_bits(nl.Convolve(k, normalize=True).kernel[0]), _bits(k / tot))
    two = nl.Convolve(np.stack([k, 2 * k]), normalize=True).kernel
    assert np.array_equal(_bits(two[0]), _bits(k / tot)) and np.array_equal(_bits(nl.Convolve(k).kernel[0]), _bits(k))
    s = nl.Convolve(k, origin=1, extend="hold").struct(1234)
    assert (s.L, s.origin, s.ext, s.shared_k, s.k) == (4, 1, 1, 1, 1234)
    for bad in ([], [[]], np.ones((2, 2, 2)), np.ones(CR.MAX_L + 1), [1.0, np.nan], [np.inf], "abc", None, [1.0, "x"], 2.0):
        with pytest.raises(ValueError):
            nl.Convolve(bad)
    for origin in (-1, 3, 1.0, "0", None, True):
        with pytest.raises(ValueError):
            nl.Convolve([1.0, 2.0, 3.0], origin=origin)
    for ext in ("wrap", 2, -1, None, True, 0.0):
        with pytest.raises(ValueError):
            nl.Convolve([1.0, 2.0], extend=ext)
    for k0 in ([1.0, -1.0], [0.0, 0.0], [1e308, 1e308]):
        with pytest.raises(ValueError):
            nl.Convolve(k0, normalize=True)


def test_library_loads_and_refuses_device_work_without_a_handle():
    from nonlin_amd import _lib
    L = _lib.load()
    one = np.ones(16)
    cv = _lib.ConvStruct(3, 1, 0, 1, one.ctypes.data)
    out = C.c_void_p(7)
    fcn = C.cast(L.nlh_curve_device_fcn, _lib.DEVFCN)
    none = C.cast(None, _lib.DEVFCN)
    assert L.nlh_conv_wrap(None, C.byref(cv), one.ctypes.data, None, fcn, none, None, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    assert L.nlh_conv_apply_batch(None, C.byref(cv), 1, 1, 1, None, None) == NLH_ERR_BAD_HANDLE
    # a malformed context is refused by the launchers before any launch (no device is touched: this runs without one)
    for fn in (L.nlh_conv_device_fcn, L.nlh_conv_device_jac):
        assert fn(None, None, 1, None, 2, None, 8, None) == NL_INVALID_INPUT_ERROR
        junk = (C.c_uint32 * 256)()
        assert fn(C.byref(junk), None, 1, None, 2, 1, 8, 1) == NL_INVALID_INPUT_ERROR
    L.nlh_conv_unwrap(None)


def test_decay_model_is_the_curve_restatement():
    rng = np.random.default_rng(1)
    t = CV.BIN * np.arange(CV.M)
    for _ in range(5):
        x = np.array([rng.uniform(100, 3000), rng.uniform(0.5, 5.0), rng.uniform(0.1, 2.0)])
        assert np.array_equal(_bits(CV.decay_model(x, t)), _bits(R.model(R.EXPDECAY, 1, 0, x, t)))
        assert np.array_equal(_bits(CV.decay_jacobian(x, t).T), _bits(R.jacobian(R.EXPDECAY, 1, 0, x, t)))
    k = CV.irf()
    tot = 0.0
    for v in k:
        tot = tot + v
    assert len(k) == CV.IRF_L and abs(tot - 1.0) <= 4 * CR.U * CV.IRF_L and int(np.argmax(k)) == CV.IRF_CENTRE


def test_study(oracle):
    """The README's table, re-measured on the oracle with the restated operation order.  Asserted is the ordering only:
    reconvolution never fails and its rate is within three standard errors of the truth; the fit of the tail from bin 20 is
    off by more than three; and tests/golden/conv_study.json records what is measured here."""
    got = CV.study(oracle)
    fits = got["fits"]
    for name, v in fits.items():
        print(f"conv study {name}: truth k {v['truth'][1]:g}, failed {v['failed']}, k {v['k_mean']:.4f} +- {v['k_stderr']:.4f}, scatter {v['k_scatter']:.4f}")
    for name in ("truth0_reconvolution", "truth1_reconvolution"):
        v = fits[name]
        assert v["failed"] == 0 and abs(v["k_mean"] - v["truth"][1]) <= 3 * v["k_stderr"], name
    v = fits["truth0_tail20"]
    assert abs(v["k_mean"] - v["truth"][1]) > 3 * v["k_stderr"]
    with open(CV.STUDY_GOLDEN) as fh:
        rec = json.load(fh)
    assert set(rec["fits"]) == set(fits)
    for name, v in fits.items():
        for key, val in v.items():
            if key == "truth":
                assert rec["fits"][name][key] == val
            else:
                assert rec["fits"][name][key] == pytest.approx(val, rel=1e-6, abs=1e-9), (name, key)


def test_perturbation_study(oracle):
    """What a last-bit change of exp does to a reconvolution fit, re-measured: tests/golden/conv_perturbation.json records at
    least what is measured here (it is what the GPU comparisons take their tolerance from), and not ten times more."""
    got = CV.perturbation_study(oracle)
    print("conv perturbation study, worst relative change of x: " + ", ".join(f"{k} {got[k]:.3g}" for k in ("analytic", "fd")))
    with open(CV.PERT_GOLDEN) as fh:
        rec = json.load(fh)
    for key in ("analytic", "fd"):
        assert got[key] <= rec[key] * (1 + 1e-9) and rec[key] <= 10 * got[key], (key, got[key], rec[key])
    assert CV.recorded_tolerance(True) == 4 * rec["analytic"] and CV.recorded_tolerance(False) == 4 * rec["fd"]
