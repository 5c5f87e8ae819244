"""CPU tests of nelder_mead: the plain-Python restatement of nm_solve (tests/nm_restatement.py) meets the reference's own
known answers (tests/nonlin_test_optimize.f90:54-181 of the reference), its counts are pinned as regression values, the
Python type carries the reference's defaults, and the three entry points are exported and bound -- with no host
fallback when no GPU is visible."""
import ctypes as C

import numpy as np
import pytest

import nm_restatement as R


def _near(x, xans, tol=1e-5):
    return all(abs(a - b) < tol for a, b in zip(x, xans))


def test_restatement_meets_reference_known_answers():
    """test_nelder_mead_1 / _2 / _3: Rosenbrock from 0, Beale from 1, Rosenbrock with args = 100, tolerance 1e-5."""
    r1 = R.nm_solve(R.rosenbrock, [0.0, 0.0])
    assert r1["status"] == 0 and r1["converge_on_fcn"] and _near(r1["x"], [1.0, 1.0])
    r2 = R.nm_solve(R.beale, [1.0, 1.0])
    assert r2["status"] == 0 and _near(r2["x"], [3.0, 0.5])

    def rosen2(x, a):
        t = x[1] - x[0] * x[0]
        u = x[0] - 1.0
        return a * (t * t) + u * u
    r3 = R.nm_solve(rosen2, [0.0, 0.0], args=100.0)
    assert r3["status"] == 0 and _near(r3["x"], [1.0, 1.0])
    assert r3["x"] == r1["x"] and r3["fout"] == r1["fout"]     # the same arithmetic with a = 100


def test_restatement_regression_counts():
    """Counts of the restatement on a few inputs (the reference's statements, re-derived): shrinks included."""
    cases = [
        (R.rosenbrock, [0.0, 0.0], {}, (85, 163, 0, 1)),
        (R.beale, [1.0, 1.0], {}, (55, 102, 0, 0)),
        (R.rosenbrock, [0.0, 0.0], {"max_evals": 40}, (19, 40, 106, 1)),
    ]
    for fcn, x0, kw, (it, ne, st, sh) in cases:
        r = R.nm_solve(fcn, x0, **kw)
        assert (r["iter_count"], r["fcn_count"], r["status"], r["shrinks"]) == (it, ne, st, sh), (x0, kw, r["iter_count"],
                                                                                               r["fcn_count"], r["shrinks"])
    r = R.nm_solve(R.rosenbrock, [0.0, 0.0])
    assert r["x"] == [1.000000120302314, 1.0000001665459648]


def test_restatement_max_evals_quirks():
    """A max-evaluations stop leaves x as it came in and reports the stale f(1) of the initial simplex (:220, :316-337);
    a shrink adds npts evaluations to the count (:299)."""
    r = R.nm_solve(R.rosenbrock, [0.0, 0.0], max_evals=40)
    assert r["status"] == 106 and not r["converge_on_fcn"]
    assert r["x"] == [0.0, 0.0] and r["fout"] == R.rosenbrock([0.0, 0.0])
    # a shrink counts n + 1 evaluations for the n it makes
    calls = [0]

    def counted(x, a):
        calls[0] += 1
        return R.rosenbrock(x)
    r = R.nm_solve(counted, [0.0, 0.0])
    assert r["shrinks"] == 1 and r["fcn_count"] == calls[0] + r["shrinks"]


def test_restatement_continues_from_simplex():
    """The object's simplex: a second solve from the final simplex of the first starts where it stopped (x ignored)."""
    r1 = R.nm_solve(R.rosenbrock, [0.0, 0.0], max_evals=60)
    r2 = R.nm_solve(R.rosenbrock, [5.0, 5.0], simplex=r1["simplex"])
    assert r2["status"] == 0 and _near(r2["x"], [1.0, 1.0])


def test_python_nelder_mead_defaults_and_copies():
    import nonlin_amd as nl
    s = nl.nelder_mead()
    assert isinstance(s, nl.equation_optimizer)
    assert (s.get_max_fcn_evals(), s.get_tolerance(), s.get_initial_size(), s.get_print_status()) == (500, 1e-12, 1.0, False)
    assert s.get_simplex() is None
    p = np.arange(6.0).reshape(2, 3)
    s.set_simplex(p)
    q = s.get_simplex()
    assert q.shape == (2, 3) and np.array_equal(q, p)
    q[0, 0] = 99.0
    p[1, 1] = -7.0
    assert s.get_simplex()[0, 0] == 0.0 and s.get_simplex()[1, 1] == 4.0
    s.set_initial_size(0.25)
    assert s.get_initial_size() == 0.25


def test_nelder_mead_symbols_bound():
    from nonlin_amd import _lib
    lib = _lib.load()
    for name in ("nlh_nelder_mead_solve", "nlh_nelder_mead_solve_batch_device", "nlh_dq_model_nelder_mead_solve"):
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
    assert "nelder_mead" in __import__("nonlin_amd").__all__


def test_nelder_mead_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import nonlin_amd as nl
    obj = nl.fcnnvar_helper()
    obj.set_fcn(lambda x, a: float(x[0] * x[0] + x[1] * x[1]), 2)
    x = np.ones(2)
    with pytest.raises(nl.NonlinHipUnavailable):
        nl.nelder_mead().solve(obj, x)
    assert x[0] == 1.0 and x[1] == 1.0
    from nonlin_amd import _lib
    assert _lib.load().nlh_nelder_mead_solve(None, None, 1.0, 2, _lib.FCNNVAR(lambda c, n, p: 0.0), None,
                                             x.ctypes.data_as(_lib.c_double_p), None, 0, None, None) == -3   # no handle
