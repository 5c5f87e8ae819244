"""CPU tests of the bands: the new entry points are declared, exported and bound and refuse a NULL handle without a device;
tests/band_restatement.py -- the numpy statement of nlh_propagate's arithmetic the GPU tests compare with bit for bit --
held to the properties the header promises and to a numpy.longdouble evaluation of J C J^T; and a coverage study of the
band on the CPU oracle's solver, recorded in tests/golden/band_study.json.

The rounding bound is derived from the operation count, not tuned.  A product C[j][k] J_k J_j goes through one multiply,
at most j adds of the inner sum, the exact doubling, one more add, the multiply by J_j and at most n adds of the outer
sum: at most 2 n + 3 roundings, so |v^ - v| <= gamma(2 n + 3) * A with gamma(k) = k u / (1 - k u), u = 2^-53 and
A = sum_jk |C[j][k]| |J_j| |J_k| (Higham, Accuracy and Stability, lemma 3.1).  The square root adds one rounding:
|sd^ - sqrt(v)| <= gamma A / sqrt(v) + u sd^ for v > 0 (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b))."""
import ctypes as C
import json
import os

import numpy as np

import band_restatement as B
import covar_restatement as cr
import curve_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3
NEW = ("nlh_propagate", "nlh_propagate_batch_device", "nlh_propagate_batch_device_h", "nlh_curve_band_batch", "nlh_expr_band_batch",
       "nlh_dq_model_propagate")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _spd(rng, npoints, n):
    a = rng.standard_normal((npoints, n, n + 2))
    return a @ np.transpose(a, (0, 2, 1)) / (n + 2)


def test_symbols_declared_exported_and_bound():
    from nonlin_amd import _lib
    L = _lib.load()
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "nonlin_hip.h")).read()
    for name in NEW:
        assert name + "(" in hdr, name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    from nonlin_amd.device import DeviceSolver
    for name in ("propagate", "propagate_batch_device", "curve_band", "expr_band"):
        assert callable(getattr(DeviceSolver, name)), name
    shim = open(os.path.join(os.path.dirname(HERE), "nonlin_amd", "fortran", "nonlin_hip_c.f90")).read()
    assert 'name="nlh_dq_model_propagate"' in shim
    lsq = open(os.path.join(os.path.dirname(HERE), "nonlin_amd", "fortran", "nonlin_least_squares.f90")).read()
    assert "propagate_batch =>" in lsq


def test_null_handle_without_a_device():
    from nonlin_amd import _lib
    L = _lib.load()
    one = np.ones(8)
    p = one.ctypes.data_as(_lib.c_double_p)
    null = C.cast(None, _lib.DEVFCN)
    assert L.nlh_propagate(None, 1, 2, 2, None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_propagate_batch_device(None, 1, 2, 2, null, null, None, None, None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_propagate_batch_device_h(None, 1, 2, 2, null, null, None, p, p, None, None, p) == NLH_ERR_BAD_HANDLE
    assert L.nlh_curve_band_batch(None, 1, 1, -1, 1, 8, None, 0, None, None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_band_batch(None, None, 1, 8, None, 0, None, None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_dq_model_propagate(None, None, p, p, None, None, p) == NLH_ERR_BAD_HANDLE


def test_upper_triangle_is_never_read():
    rng = np.random.default_rng(1)
    for n in (1, 2, 5, 17):
        J = rng.standard_normal((4, n, 7))
        cov = _spd(rng, 4, n)
        noise = rng.uniform(0.0, 1.0, 4)
        bad = cov.copy()
        bad[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]] = np.nan
        for nz in (None, noise):
            assert np.array_equal(_bits(B.propagate(J, cov, nz)), _bits(B.propagate(J, bad, nz)))
            assert not np.isnan(B.propagate(J, bad, nz)).any()


def test_negative_definite_gives_exact_zero():
    rng = np.random.default_rng(2)
    for n in (1, 3, 9):
        J = rng.standard_normal((3, n, 5))
        cov = np.broadcast_to(-np.eye(n), (3, n, n)).copy()
        sd = B.propagate(J, cov)
        assert np.array_equal(_bits(sd), _bits(np.zeros((3, 5))))     # +0.0, not -0.0, not NaN


def test_nan_in_the_lower_triangle_gives_nan():
    rng = np.random.default_rng(3)
    n = 4
    J = rng.standard_normal((3, n, 5))
    cov = _spd(rng, 3, n)
    ref = B.propagate(J, cov)
    for j, k in ((0, 0), (2, 1), (3, 3)):
        bad = cov.copy()
        bad[1, j, k] = np.nan
        sd = B.propagate(J, bad)
        assert np.isnan(sd[1]).all()
        assert np.array_equal(_bits(sd[[0, 2]]), _bits(ref[[0, 2]]))  # the neighbours are untouched


def test_one_parameter():
    """n = 1: v = J*(C*J), two roundings, then the square root's: sd^ = |J| sqrt(C) (1 + d), |d| <= (1 + u)^2 - 1 (the square
    root halves the first two); the reference is formed in numpy.longdouble (2^-60 covers its own roundings)."""
    rng = np.random.default_rng(4)
    J = rng.standard_normal((50, 1, 6))
    cov = rng.uniform(0.1, 10.0, (50, 1, 1))
    sd = B.propagate(J, cov)
    ref = np.abs(J[:, 0, :].astype(np.longdouble)) * np.sqrt(cov[:, 0, 0].astype(np.longdouble))[:, None]
    assert (np.abs(sd - ref) <= (2.0 * U + U * U + 2.0 ** -60) * ref).all()      # ((1 + u)^2 - 1, written out: 1 + u rounds to 1)


def test_rounding_against_longdouble():
    """200 random symmetric positive-definite cases, n = 1 .. 40: the bound of the module docstring."""
    assert np.finfo(np.longdouble).nmant >= 63                        # an 80-bit (or wider) long double: u_ld <= 2^-64
    rng = np.random.default_rng(5)
    worst = 0.0
    for case in range(200):
        n = 1 + case % 40
        m = 5
        J = rng.standard_normal((1, n, m))
        cov = _spd(rng, 1, n)
        noise = rng.uniform(0.0, 0.5, 1) if case % 2 else None
        sd = B.propagate(J, cov, noise)[0]
        v = B.propagate_longdouble(J, cov, noise)[0]
        assert (v > 0).all()
        full = np.tril(cov[0]) + np.tril(cov[0], -1).T
        A = np.einsum("ji,jk,ki->i", np.abs(J[0]), np.abs(full), np.abs(J[0])) + (0.0 if noise is None else noise[0])
        k = 2 * n + 3 + (1 if noise is not None else 0)
        gamma = k * U / (1.0 - k * U)
        rt = np.sqrt(v)
        err = np.abs(sd - rt)
        bound = gamma * A / rt + U * sd + 2.0 ** -60 * rt
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (case, n)
    print(f"largest error / bound over 200 cases: {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# the coverage study
# ---------------------------------------------------------------------------------------------------------------------
STUDY_T = (0.3, 2.0, 4.5)
STUDY_N, STUDY_M, STUDY_NOISE = 300, 64, 0.02


def run_study(oracle):
    """300 decays a exp(-k t) + c on 64 points of [0, 5], Gaussian noise of 0.02, fitted by the oracle's
    least_squares_solver from (0.9, 1.1, 1) * truth; cov by the oracle's lmfactor and the covar restatement, scaled; the band
    from the restatement on the restated Jacobian at STUDY_T.  Returns the number of problems, per abscissa, whose true
    curve lies within 1.96 sd of the fitted one, and the number of fits that converged."""
    kind, K, Bd = R.EXPDECAY, 1, 0
    rng = np.random.default_rng(20261019)
    t = np.linspace(0.0, 5.0, STUDY_M)
    tg = np.array(STUDY_T)
    inside = np.zeros(len(STUDY_T), dtype=int)
    solved = 0
    for _ in range(STUDY_N):
        truth = np.array([rng.uniform(1.0, 2.0), rng.uniform(0.5, 1.5), rng.uniform(0.1, 0.5)])
        y = R.model(kind, K, Bd, truth, t) + STUDY_NOISE * rng.standard_normal(STUDY_M)

        def fcn(x, f):
            f[:] = R.residual(kind, K, Bd, x, t, y)

        def jac(x, J):
            J[:, :] = R.jacobian(kind, K, Bd, x, t)

        rc, x, fvec, _ = oracle.lm_solve(fcn, STUDY_M, 3, truth * np.array([0.9, 1.1, 1.0]), jac=jac)
        solved += rc == 0
        a, ipvt, rdiag, _ = oracle.lmfactor(np.asfortranarray(R.jacobian(kind, K, Bd, x, t)))
        cov, _, rank, _ = cr.lm_covariance(cr.r_of_lmfactor(a, rdiag), ipvt, fvec, scaled=True)
        assert rank == 3
        G = R.jacobian(kind, K, Bd, x, tg)                            # (3 abscissae, 3 parameters)
        sd = B.propagate(G.T[None], cov[None])[0]
        inside += np.abs(R.model(kind, K, Bd, x, tg) - R.model(kind, K, Bd, truth, tg)) <= 1.96 * sd
    return inside, solved


def test_coverage_study(oracle):
    """Each share within 0.95 +- 4 sqrt(0.95 * 0.05 / 300), the binomial spread; the counts are the recorded ones."""
    rec = json.load(open(os.path.join(HERE, "golden", "band_study.json")))
    inside, solved = run_study(oracle)
    print("inside:", inside.tolist(), "of", STUDY_N, "solved:", solved)
    half = 4.0 * np.sqrt(0.95 * 0.05 / STUDY_N)
    assert solved == STUDY_N
    for c in inside:
        assert abs(c / STUDY_N - 0.95) <= half, inside
    assert rec["abscissae"] == list(STUDY_T) and rec["problems"] == STUDY_N
    assert rec["inside"] == inside.tolist()
