"""CPU tests of the separable fits (include/nonlin_hip.h: nlh_sep_*): the object and its refusals (host code of the
library, no GPU), and the restated arithmetic (tests/sep_restatement.py) held to a least-squares solve in 80-digit arithmetic (the issue asks for 60; 80 costs nothing), to the
complex-step gradient, to the full fit's minimiser on the CPU oracle, and to the biexponential study the README quotes.  The
constants and the study are recorded under tests/golden/ (tests/sep_cases.py writes them)."""
import ctypes as C
import json

import numpy as np
import pytest

import sep_cases as SC
import sep_restatement as SR
import nonlin_amd as nl
from nonlin_amd import _lib

NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NLH_ERR_BAD_HANDLE = 201, 211, -3
ip = C.POINTER(C.c_int32)


def _create(N, lin):
    lib = _lib.load()
    ptr = C.c_void_p(0xdead)
    a = np.ascontiguousarray(lin, dtype=np.int32)
    rc = lib.nlh_sep_create(N, len(a), a.ctypes.data_as(ip) if lin is not None else None, C.byref(ptr))
    return rc, ptr


# ------------------------------------------------------------------------------------------------ 1. the object
def test_object_and_tables():
    sp = nl.Separable(7, linear=(6, 0, 3))
    assert (sp.nparams, sp.nlin, sp.nnonlin) == (7, 3, 4)
    lin, nln = sp.tables()
    assert lin.tolist() == [0, 3, 6] and nln.tolist() == [1, 2, 4, 5]
    want = SR.tables(7, (6, 0, 3))
    assert lin.tolist() == want[0].tolist() and nln.tolist() == want[1].tolist()
    sp.close()
    sp.close()                                                    # twice is harmless
    full = nl.Separable(33, linear=range(32))                     # L = NLH_SEP_MAX_L with one nonlinear parameter left
    assert (full.nlin, full.nnonlin) == (32, 1) and full.tables()[1].tolist() == [32]


def test_for_curve_and_for_expr():
    assert nl.Separable.for_curve("lorentz", 2, 1).tables()[0].tolist() == [0, 3, 6, 7]
    assert nl.Separable.for_curve("gauss", 1, -1).tables()[0].tolist() == [0]
    assert nl.Separable.for_curve("expdecay", 2, 0).tables()[0].tolist() == list(SC.STUDY_LINEAR)
    e = nl.Expr("vmax*s/(km+s) + b", ("s",), ("vmax", "km", "b"))
    sp = nl.Separable.for_expr(e, linear=("b", "vmax"))
    assert sp.tables()[0].tolist() == [0, 2] and sp.tables()[1].tolist() == [1]
    with pytest.raises(ValueError):
        nl.Separable.for_expr(e, linear=("nope",))


@pytest.mark.parametrize("N,lin", [(3, []),                       # L < 1
                                   (40, list(range(33))),         # L > NLH_SEP_MAX_L
                                   (3, [0, 1, 2]),                # n < 1
                                   (3, [0, 3]), (3, [-1, 1]),     # out of range
                                   (4, [1, 1]),                   # repeated
                                   (4, [2, 1]),                   # not ascending
                                   (8193, [0])])                  # beyond the models' parameter limit
def test_create_refusals(N, lin):
    rc, ptr = _create(N, lin)
    assert rc == NL_INVALID_INPUT_ERROR and not ptr.value
    if lin != [2, 1]:                                             # (the class sorts what it is given)
        with pytest.raises(ValueError):
            nl.Separable(N, linear=lin)


def test_null_arguments():
    lib = _lib.load()
    ptr = C.c_void_p(0xdead)
    assert lib.nlh_sep_create(3, 1, None, C.byref(ptr)) == NL_INVALID_INPUT_ERROR and not ptr.value
    assert lib.nlh_sep_create(3, 1, (C.c_int32 * 1)(0), None) == NL_INVALID_INPUT_ERROR
    assert lib.nlh_sep_tables(None, None, None) == NL_INVALID_INPUT_ERROR
    s = [C.c_int32(5) for _ in range(3)]
    lib.nlh_sep_shape(None, *[C.byref(v) for v in s])
    assert [v.value for v in s] == [0, 0, 0]
    lib.nlh_sep_destroy(None)
    lib.nlh_sep_unwrap(None)
    # what a wrap refuses before it needs a device: no handle
    sp = nl.Separable(3, linear=(0,))
    out = C.c_void_p(0xdead)
    assert lib.nlh_sep_wrap(None, sp.ptr, C.cast(None, _lib.DEVFCN), C.cast(None, _lib.DEVFCN), None, C.byref(out)) == NLH_ERR_BAD_HANDLE
    assert not out.value
    assert lib.nlh_sep_gather_batch(None, sp.ptr, 1, None, None) == NLH_ERR_BAD_HANDLE
    assert lib.nlh_sep_solve_batch(None, None, 1, 4, None, None, None) == NLH_ERR_BAD_HANDLE


# ------------------------------------------------------------------------------------------------ 2. the restated arithmetic
def test_rowsum_is_the_block_sum():
    """The order of tests/sep_restatement.rowsum, spelled out on a case where it matters."""
    rng = np.random.default_rng(1)
    a, b = rng.uniform(-1, 1, 600) * 10.0 ** rng.integers(-8, 8, 600), rng.uniform(-1, 1, 600)
    part = [0.0] * 256
    for i in range(5, 600):
        part[i % 256] = part[i % 256] + a[i] * b[i]
    waves = []
    for w in range(4):
        p = part[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            p = [p[l] + p[l + off] for l in range(off)] + p[off:]
        waves.append(p[0])
    want = 0.0
    for v in waves:
        want = want + v
    assert SR.rowsum(a, b, 4) == want


def test_solve_accuracy_against_80_digits():
    """The restatement's c against the least-squares solution of the same doubles in 80-digit arithmetic, in units of
    L 2^-52 cond2(Phi) |c|: below the recorded constant, which is 4 x the recorded measurement rounded up to a power of two."""
    got = SC.accuracy_ratios()
    worst = max(got.values())
    print("separable solve, |c - exact| / (L u cond |c|): " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    print(f"largest ratio {worst:.4g}")
    with open(SC.ACCURACY_GOLDEN) as fh:
        rec = json.load(fh)
    assert rec["solve_c"] == SC._pow2_above(4 * rec["solve_ratio_max"])
    assert worst <= rec["solve_c"] and rec["solve_ratio_max"] <= 4 * worst


def test_dead_column():
    """Two identical columns: the second is dead, its c is +0.0, the rank is L - 1, and the others solve the reduced problem."""
    rng = np.random.default_rng(3)
    t = np.linspace(0.0, 1.0, 301)
    a = 1.0 / (1.0 + ((t - 0.4) / 0.1) ** 2)
    Phi = np.stack([a, np.ones(301), a, t], axis=1)
    f0 = -(2.0 * a + 0.5 - 0.3 * t) + 1e-3 * rng.uniform(-1, 1, 301)
    c, rank, V, tau, rpos = SR.qr_solve(Phi, f0)
    assert rank == 3 and rpos.tolist() == [0, 1, -1, 2] and tau[2] == 0.0
    assert c[2] == 0.0 and not np.signbit(c[2])
    c3 = SR.qr_solve(Phi[:, [0, 1, 3]], f0)[0]
    assert np.allclose(c[[0, 1, 3]], c3, rtol=1e-12, atol=0)
    assert np.allclose(c[[0, 1, 3]], [2.0, 0.5, -0.3], atol=1e-3)
    # a projected column has no component along the live basis, the dead column included (it lies in their span)
    D = rng.uniform(-1, 1, (301, 2))
    P = SR.project(V, tau, rpos, D)
    assert np.abs(Phi.T @ P).max() <= 1e-12 * np.abs(Phi).max() * 301
    z = np.zeros((301, 1))
    assert np.array_equal(SR.project(V, tau, rpos, z), z)


def test_gradient_identity():
    """J_K^T r of the restatement is the gradient of 1/2 |r(alpha)|^2 (Kaufman's Jacobian is exact there, because r is
    orthogonal to span Phi): against the complex step, within the roundoff of the products, c m 2^-52 sum_i |J_ik r_i|."""
    got = SC.gradient_ratios()
    worst = max(got.values())
    print("separable gradient, |J^T r - g| / (m u sum |J r|): " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    print(f"largest ratio {worst:.4g}")
    with open(SC.ACCURACY_GOLDEN) as fh:
        rec = json.load(fh)
    assert rec["gradient_c"] == SC._pow2_above(4 * rec["gradient_ratio_max"])
    assert worst <= rec["gradient_c"] and rec["gradient_ratio_max"] <= 4 * worst


def test_projection_and_residual_identities():
    """The residual the restatement returns is the inner residual at the solved parameters, and it is orthogonal to Phi."""
    K, B, m = 2, 1, 200
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, 1, seed=9)
    fcn, jac = SC.lorentz_callbacks(K, B, t[0], y[0])
    N = 8
    lin, nln = SR.tables(N, SC.lorentz_linear(K, B))
    ph, rank, _ = SR.solve(fcn, jac, N, lin, x0[0][nln])
    assert rank == len(lin) and np.array_equal(ph[nln], x0[0][nln])
    r = SR.residual(fcn, jac, N, lin, x0[0][nln])
    assert np.array_equal(r, fcn(ph))
    Phi = jac(ph)[:, lin]
    assert np.abs(Phi.T @ r).max() <= 1e-12 * m * np.abs(Phi).max() * np.abs(r).max() * 10


# ------------------------------------------------------------------------------------------------ 3. on the oracle's solver
def test_minimiser_is_the_full_fit_s(oracle):
    """lm_solve over the restatement lands where lm_solve over the full model lands: the difference in units of the full
    fit's sigma is within 4 x the recorded one, and below 1e-2 in any case."""
    got = SC.minimiser_differences(oracle)
    worst = max(got.values())
    print("separable against full fit, |dx| / sigma: " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
    with open(SC.STUDY_GOLDEN) as fh:
        rec = json.load(fh)
    assert worst <= 4 * rec["minimiser_max_sigma"] and worst <= 1e-2


def test_study(oracle):
    """The README's table, re-measured on the oracle.  Conditions: the projected fit reaches cost <= 1.05 x the cost at the
    truth on every problem, and its mean evaluation count is below the informed full fit's; tests/golden/sep_study.json
    records what is measured here."""
    got = SC.study(oracle)
    arms = got["arms"]
    print("separable study: " + json.dumps(arms))
    assert arms["sep_kaufman"]["reached"] == got["nprob"] == 200
    assert arms["sep_kaufman"]["mean_evals"] < arms["full_informed"]["mean_evals"]
    with open(SC.STUDY_GOLDEN) as fh:
        rec = json.load(fh)
    assert rec["truth"] == list(SC.STUDY_TRUTH) and rec["seed"] == SC.STUDY_SEED and set(rec["arms"]) == set(arms)
    for name, v in arms.items():
        assert v["reached"] == rec["arms"][name]["reached"], name
        assert abs(v["mean_evals"] - rec["arms"][name]["mean_evals"]) <= 0.02 * rec["arms"][name]["mean_evals"], name
