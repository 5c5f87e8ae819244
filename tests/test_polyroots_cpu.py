"""CPU tests of the polynomial root finder's restatement (tests/polyroots_restatement.py, which the GPU kernels are held to
bit for bit in tests/test_gpu_polyroots.py) against the reference's own solver and against the truth, and of the
polynomial arithmetic against numpy.polynomial.

The reference's polynomial%roots builds the companion matrix (src/nonlin_polynomials.f90:346-353) and calls LAPACK DGEEV
through linalg's eigen (:380); numpy.linalg.eigvals on that matrix IS that call, so it is the reference here.  The truth is
mpmath at 60 digits.  Families a-f: tests/polyroots_cases.py.

The accuracy statistic is r(z) = |p(z)| / sum_k |a_k| |z|^k (mpmath, 60 digits), r = 0 where z == 0 and a_0 == 0.  Per
family max r(ours) <= M max(max r(LAPACK), eps), eps = 2.22e-16.  M comes from tests/golden/poly_roots_study.json
(tests/golden/make_poly_roots_study.py): the smallest power of two that is at least twice the largest measured family
ratio, never above 16.  Two orderings of the same backward-stable iteration differ by small factors; a missing balancing
step or a wrong deflation test shows as 10^2 and more (test_the_bound_separates_right_from_wrong).  The LAPACK side is
recomputed live; the file supplies M only.  Measured when the file was written: ratios 0.50 (a), 0.81 (b), 0.29 (c),
0.11 (d), 1.31 (e): M = 4."""
import json
import math
import os

import numpy as np
import numpy.polynomial.polynomial as npoly
import pytest

import polyroots_cases as cases
import polyroots_measure as pm
import polyroots_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUDY = json.load(open(os.path.join(ROOT, "tests", "golden", "poly_roots_study.json")))


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_bound_is_derived_from_the_study():
    m = pm.bound_from_study(STUDY)
    assert m == STUDY["M"] and m <= 16 and m & (m - 1) == 0
    worst = max(v["ratio"] for v in STUDY["families"].values())
    assert m >= 2.0 * worst and (m == 1 or m / 2 < 2.0 * worst)
    assert set(STUDY["families"]) == {"a", "b", "c", "d", "e"}


def _pairing_ok(z):
    """(i): every complex root's conjugate is the next entry: bitwise equal real parts, negated imaginary parts."""
    i = 0
    while i < len(z):
        re, im = z[i]
        if im != 0.0:
            assert im > 0.0 and i + 1 < len(z), (i, z)
            re2, im2 = z[i + 1]
            assert _bits(re) == _bits(re2) and _bits(im2) == _bits(-im), (i, z)
            i += 2
        else:
            i += 1


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_family_against_lapack_and_truth(name):
    m_bound = STUDY["M"]
    forward = name in ("a", "c")
    mo = ml = fo = fl = 0.0
    ncases = 0
    for c in cases.FAMILIES[name]():
        n = len(c) - 1
        st = {}
        pairs, info = rs.poly_roots([float(v) for v in c], stats=st)
        assert info == 0 and len(pairs) == n                                   # (i) count
        assert st["sweeps"] < st["itmax"]                                      # (v) the iteration limit is not reached
        _pairing_ok(pairs)
        z = np.array([complex(re, im) for re, im in pairs])
        w = pm.lapack(c)                                                       # raises if DGEEV fails: it does not
        p = pm.match(z, w)                                                     # (ii) one to one, nothing left over
        assert sorted(p) == list(range(n))
        mo = max(mo, max(pm.ratio_r(c, v) for v in z))
        ml = max(ml, max(pm.ratio_r(c, v) for v in w))
        if forward:
            t = pm.true_roots(c)
            fo = max(fo, pm.forward_error(z, t))
            fl = max(fl, pm.forward_error(w, t))
        ncases += 1
    print(f"family {name}: {ncases} cases, max r(LAPACK) {ml:.3e}, max r(ours) {mo:.3e}, ratio {mo / max(ml, pm.EPS):.3f}, M {m_bound}")
    assert mo <= m_bound * max(ml, pm.EPS)                                     # (iii)
    if forward:
        print(f"family {name}: max fwd(LAPACK) {fl:.3e}, max fwd(ours) {fo:.3e}")
        assert fo <= m_bound * max(fl, pm.EPS)                                 # (iv)


def test_family_a_reference_checks():
    """tests/nonlin_test_poly.f90:53-84: |p(z)| <= 1e-6 at every root of x^3 - 4x^2 + x + 6 (roots 2, 3, -1); the roots
    example's x^3 - 2x - 1 has roots -1, (1 +- sqrt 5) / 2."""
    c = [6.0, 1.0, -4.0, 1.0]
    z, info = rs.poly_roots(c)
    assert info == 0
    for re, im in z:
        yr, yi = rs.poly_eval_complex(c, re, im)
        assert math.hypot(yr, yi) <= 1e-6
    assert sorted(round(re, 9) for re, _ in z) == [-1.0, 2.0, 3.0] and all(im == 0.0 for _, im in z)
    z, info = rs.poly_roots([-1.0, -2.0, 0.0, 1.0])
    assert info == 0 and all(im == 0.0 for _, im in z)
    want = sorted([-1.0, (1.0 - math.sqrt(5.0)) / 2.0, (1.0 + math.sqrt(5.0)) / 2.0])
    assert np.allclose(sorted(re for re, _ in z), want, rtol=0, atol=1e-14)
    assert sorted(f"{re:9.6f}" for re, _ in z) == sorted(["-1.000000", " 1.618034", "-0.618034"])


@pytest.mark.parametrize("c, nzero", cases.ZERO_CASES)
def test_exact_zero_roots(c, nzero):
    """(vi): LAPACK returns nzero roots that are exactly 0.0 (DGEBAL's permutation isolates them); so must we, and in the
    same place (last)."""
    w = pm.lapack(np.array(c))
    assert int(np.sum(w == 0)) == nzero
    z, info = rs.poly_roots(c)
    assert info == 0
    assert sum(1 for re, im in z if re == 0.0 and im == 0.0) == nzero
    assert all(re == 0.0 and im == 0.0 for re, im in z[len(z) - nzero:])
    assert all(bool(v == 0) for v in w[len(w) - nzero:])


def test_failure_rows():
    """f: leading coefficient 0 -> NL_DIVIDE_BY_ZERO_ERROR; a non-finite coefficient -> NL_INVALID_INPUT_ERROR; roots NaN."""
    for c, want in cases.family_f():
        z, info = rs.poly_roots([float(v) for v in c])
        assert info == want and len(z) == len(c) - 1
        assert all(math.isnan(re) and math.isnan(im) for re, im in z)
    z, info = rs.poly_roots([1e300, 1.0, 1e-300])               # finite coefficients, infinite companion entry
    assert info == rs.NL_INVALID_INPUT_ERROR
    assert rs.poly_roots([3.0]) == ([], 0)                      # order 0: nothing (:373)


def test_the_bound_separates_right_from_wrong():
    """The same restatement WITHOUT the balancing step misses the bound on the badly scaled family by orders of magnitude:
    the inputs and the bound do tell a missing step from a different rounding."""
    mo = ml = 0.0
    for c in cases.family_d():
        pairs, info = rs.poly_roots([float(v) for v in c], balance=False)
        z = np.array([complex(re, im) for re, im in pairs])
        finite = np.isfinite(z)
        mo = max(mo, max([pm.ratio_r(c, v) for v in z[finite]] + ([1.0] if not finite.all() else [])))
        ml = max(ml, max(pm.ratio_r(c, v) for v in pm.lapack(c)))
    print(f"family d without balancing: max r {mo:.3e} against LAPACK's {ml:.3e}")
    assert mo > 16 * max(ml, pm.EPS)


def test_horner_restatement():
    rng = np.random.default_rng(7)
    for order in (0, 1, 2, 5, 11):
        c = rng.standard_normal(order + 1)
        for x in rng.standard_normal(5):
            assert abs(rs.poly_eval(list(c), float(x)) - npoly.polyval(x, c)) <= 1e-12 * max(1.0, abs(npoly.polyval(x, c)))
        for x in rng.standard_normal(5) + 1j * rng.standard_normal(5):
            yr, yi = rs.poly_eval_complex(list(c), x.real, x.imag)
            want = npoly.polyval(x, c)
            assert abs(complex(yr, yi) - want) <= 1e-12 * max(1.0, abs(want))
    assert rs.poly_eval([], 2.0) == 0.0 and rs.poly_eval_complex([], 1.0, 1.0) == (0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# arithmetic: the restatement and the product's host code (nonlin_amd.polynomial), both against numpy.polynomial
# ---------------------------------------------------------------------------------------------------------------------
def _poly(c):
    import nonlin_amd as nl
    p = nl.polynomial()
    p.initialize(c)
    return p


def test_add_subtract_where_the_reference_loops_are_right():
    """x_ord <= y_ord (what tests/nonlin_test_poly.f90:87-202 exercises: orders 10 and 20): bitwise equal to numpy's
    polyadd / polysub (the operation order is forced), and within the reference's tol = 1e-8."""
    rng = np.random.default_rng(11)
    for ox, oy in ((10, 20), (3, 3), (0, 5), (7, 8)):
        x, y = rng.random(ox + 1), rng.random(oy + 1)
        for sub, ref in ((False, npoly.polyadd), (True, npoly.polysub)):
            want = ref(x, y)
            got_r = rs.poly_add_sub(list(x), list(y), sub)
            got_p = (_poly(x) - _poly(y)) if sub else (_poly(x) + _poly(y))
            assert np.array_equal(_bits(got_r), _bits(want)) and np.array_equal(_bits(got_p.get_all()), _bits(want))
            assert np.max(np.abs(np.array(got_r) - want)) <= 1e-8


def test_add_subtract_kept_oddities():
    """Reference behaviour kept.  src/nonlin_polynomials.f90:538 and :593: for x_ord > y_ord the copy loop runs
    do i = y_ord + 2, x_ord, so the LEADING coefficient of x + y and x - y stays 0.  :576-580: x - y with x uninitialised
    returns +y."""
    import nonlin_amd as nl
    x, y = [1.0, 2.0, 3.0, 4.0, 5.0], [10.0, 20.0]
    for sub in (False, True):
        want = [1.0 - 10.0, 2.0 - 20.0, 3.0, 4.0, 0.0] if sub else [11.0, 22.0, 3.0, 4.0, 0.0]
        assert rs.poly_add_sub(x, y, sub) == want
        got = (_poly(x) - _poly(y)) if sub else (_poly(x) + _poly(y))
        assert got.order() == 4 and list(got.get_all()) == want
    assert rs.poly_add_sub(None, y, True) == y                                 # +y, not -y
    got = nl.polynomial() - _poly(y)
    assert list(got.get_all()) == y
    assert list((nl.polynomial() + _poly(y)).get_all()) == y and list((_poly(x) - nl.polynomial()).get_all()) == x
    assert (nl.polynomial() + nl.polynomial()).order() == -1


def test_multiply_and_scale():
    p1, p2 = [5.0, 0.0, 10.0, 6.0], [1.0, 2.0, 4.0]                            # tests/nonlin_test_poly.f90:206-250
    want = [5.0, 10.0, 30.0, 26.0, 52.0, 24.0]
    assert rs.poly_mult(p1, p2) == want and list((_poly(p1) * _poly(p2)).get_all()) == want
    rng = np.random.default_rng(12)
    for ox, oy in ((4, 9), (9, 4), (0, 3), (6, 6)):
        x, y = rng.standard_normal(ox + 1), rng.standard_normal(oy + 1)
        ref = npoly.polymul(x, y)
        got = rs.poly_mult(list(x), list(y))
        assert np.max(np.abs(np.array(got) - ref)) <= 1e-8
        assert np.array_equal(_bits((_poly(x) * _poly(y)).get_all()), _bits(got))
        for got_s in ((_poly(x) * 2.5).get_all(), (2.5 * _poly(x)).get_all(), rs.poly_scale(list(x), 2.5)):
            assert np.array_equal(_bits(got_s), _bits(x * 2.5))


def test_divide():
    import nonlin_amd as nl
    q, r = rs.poly_divide([0.0, 1.0, 0.0, 1.0], [1.0, 1.0])                    # tests/nonlin_test_poly.f90:254-297
    assert np.allclose(q, [2.0, -1.0, 1.0], rtol=0, atol=1e-8) and np.allclose(r, [-2.0], rtol=0, atol=1e-8)
    pq, pr = _poly([0.0, 1.0, 0.0, 1.0]).divide(_poly([1.0, 1.0]))
    assert list(pq.get_all()) == q and list(pr.get_all()) == r
    rng = np.random.default_rng(13)
    for on, od in ((7, 3), (5, 5), (9, 1), (2, 4)):
        num, den = rng.standard_normal(on + 1), rng.standard_normal(od + 1)
        qn, rn = npoly.polydiv(num, den)
        q, r = rs.poly_divide(list(num), list(den))
        pq, pr = _poly(num).divide(_poly(den))
        assert np.array_equal(_bits(pq.get_all()), _bits(q)) and np.array_equal(_bits(pr.get_all()), _bits(r))
        assert len(q) == len(qn) and np.max(np.abs(np.array(q) - qn)) <= 1e-8
        rpad = np.zeros(max(len(r), len(rn)))
        rpad[:len(r)] = r
        rnp = np.zeros_like(rpad)
        rnp[:len(rn)] = rn
        assert np.max(np.abs(rpad - rnp)) <= 1e-8
    with pytest.raises(ZeroDivisionError):
        rs.poly_divide([1.0, 2.0, 3.0], [1.0, 1e-17])                          # |lead| <= epsilon, :717
    with pytest.raises(nl.NonlinError) as e:
        _poly([1.0, 2.0, 3.0]).divide(_poly([1.0, 1e-17]))
    assert e.value.code == nl.NL_DIVIDE_BY_ZERO_ERROR
    q, r = rs.poly_divide([1.0, 2.0, 1.0], [1.0, 1.0])                         # exact: the remainder trims to order 0
    assert q == [1.0, 1.0] and r == [0.0]


def test_assignment_companion_and_complex_evaluate_host_side():
    import nonlin_amd as nl
    p = _poly([6.0, 1.0, -4.0, 1.0])
    assert np.array_equal(p.companion_mtx(), cases.companion(np.array([6.0, 1.0, -4.0, 1.0])))
    q = p.copy()
    q.set(1, 0.0)
    assert p.get(1) == 6.0 and q.get(1) == 0.0
    assert list(nl.polynomial(2).assign(3.0).get_all()) == [3.0, 3.0, 3.0]     # :473-488
    assert list(nl.polynomial().assign([1.0, 2.0]).get_all()) == [1.0, 2.0]    # :491-498
    assert list(nl.polynomial(5).assign(p).get_all()) == [6.0, 1.0, -4.0, 1.0]  # :454-470
    x = np.array([0.5 + 0.25j, -1.0 + 2.0j, 3.0 + 0.0j])
    y = p.evaluate(x)
    for k in range(3):
        yr, yi = rs.poly_eval_complex([6.0, 1.0, -4.0, 1.0], x[k].real, x[k].imag)
        assert _bits(y[k].real) == _bits(yr) and _bits(y[k].imag) == _bits(yi)
    xr = np.array([0.5, -1.0, 3.0])
    assert np.array_equal(_bits(p.evaluate(xr)), _bits([rs.poly_eval([6.0, 1.0, -4.0, 1.0], float(v)) for v in xr]))
