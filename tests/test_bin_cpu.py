"""CPU tests of the bin-integrated fits (include/nonlin_hip_bin.h: nlh_bin_*): the new entry points are declared, exported and
bound; the numpy restatement (tests/bin_restatement.py) against a per-bin scalar loop; nlh_bin_rule -- host code -- against
numpy's leggauss and against its own definition; the identities the header promises; the validation of the Python Binned, its
node layout and its pixels; the error codes that need no device; and, on the CPU oracle's solver with the restated transform
as a host callback, the study of the bias of a fitted width recorded in tests/golden/bin_study.json."""
import ctypes as C
import json
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import bin_cases as BC
import bin_restatement as BR
from nonlin_amd import Binned
from nonlin_amd._lib import BIN_SYMBOLS  # noqa: F401  (the feature: without it nothing here runs)

HERE = os.path.dirname(os.path.abspath(__file__))
NL_INVALID_INPUT_ERROR, NL_ARRAY_SIZE_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NLH_ERR_BAD_HANDLE = 201, 202, 211, -3
NEW = ("nlh_bin_rule", "nlh_bin_wrap", "nlh_bin_unwrap", "nlh_bin_device_fcn", "nlh_bin_device_jac", "nlh_bin_apply_batch")
dp = C.POINTER(C.c_double)
ORDERS = list(range(1, 9))


def _read(name):
    return open(os.path.join(os.path.dirname(HERE), "include", name)).read()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _rule(Q):
    from nonlin_amd import _lib
    xi, c = np.full(Q, 7.0), np.full(Q, 7.0)
    assert _lib.load().nlh_bin_rule(Q, xi.ctypes.data_as(dp), c.ctypes.data_as(dp)) == 0
    return xi, c


def test_symbols_declared_exported_and_bound():
    from nonlin_amd import _lib
    import nonlin_amd
    L = _lib.load()
    assert '#include "nonlin_hip_bin.h"' in _read("nonlin_hip.h")             # who includes nonlin_hip.h has the entry points
    text = _read("nonlin_hip_bin.h")
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(nlh_[a-z0-9_]+)\s*\(", hdr))) == sorted(NEW) == sorted(_lib.BIN_SYMBOLS)      # table and header agree
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == _lib.BIN_SYMBOLS[name][1], name
        assert all(name not in tab for tab in (_lib.SYMBOLS, _lib.GUESS_SYMBOLS, _lib.STARTS_SYMBOLS, _lib.BOOT_SYMBOLS))
    assert int(re.search(r"#define\s+NLH_BIN_MAX_Q\s+(\d+)", text).group(1)) == _lib.BIN_MAX_Q == BR.MAX_Q == 16
    assert not any("bin" in v for v in _lib.FIT_VARIANT)                      # no new one-call entry points in C
    assert nonlin_amd.Binned is _lib.Binned
    # nlh_bin as C lays it out: Q, eight-byte aligned c [16], s, shared_s
    assert (_lib.BinStruct.c.offset, _lib.BinStruct.s.offset, _lib.BinStruct.shared_s.offset, C.sizeof(_lib.BinStruct)) == (8, 136, 144, 152)
    from nonlin_amd.device import DeviceSolver
    for name in ("bin_launchers", "bin_apply", "bin_nodes"):
        assert callable(getattr(DeviceSolver, name))
    import inspect
    for name in ("curve_fit_batch", "expr_fit_batch"):
        assert list(inspect.signature(getattr(DeviceSolver, name)).parameters)[-1] == "bins"


# ---------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,Q", [(1, 1), (1, 16), (2, 3), (7, 2), (33, 5), (64, 4), (65, 16), (130, 1)])
def test_restatement_is_the_definition(m, Q):
    """The loop over nodes of whole-array operations gives the bits of the per-bin scalar loop: one column, a stack of columns,
    a scale for every problem and one per problem, and none."""
    rng = np.random.default_rng(100 * m + Q)
    v, c, s = rng.standard_normal(Q * m), rng.standard_normal(Q), rng.uniform(0.1, 2.0, m)
    assert np.array_equal(_bits(BR.reduce(v, c, s)), _bits(BR.scalar(v, c, s)))
    assert np.array_equal(_bits(BR.reduce(v, c)), _bits(BR.scalar(v, c)))
    V, S = rng.standard_normal((3, 2, Q * m)), rng.uniform(0.1, 2.0, (3, m))
    for scale in (None, s, S):
        both = BR.jacobian(V, None, c, scale)
        assert both.shape == (3, 2, m)
        for p in range(3):
            for k in range(2):
                sp = None if scale is None else scale if scale.ndim == 1 else scale[p]
                assert np.array_equal(_bits(both[p, k]), _bits(BR.scalar(V[p, k], c, sp)))


def test_residual_jacobian_and_weights():
    """residual: g - y, times w; Jacobian: g over each column, times w; a zero-weight bin is +0.0 by bit pattern whatever the
    bin holds."""
    rng = np.random.default_rng(5)
    m, n, Q = 33, 4, 3
    v, y, J, c, s = rng.standard_normal(Q * m), rng.standard_normal(m), rng.standard_normal((n, Q * m)), rng.standard_normal(Q), rng.uniform(0.5, 2, m)
    w = rng.uniform(0.5, 2.0, m)
    w[[0, 7, m - 1]] = 0.0
    w[3] = -0.0
    z = w == 0.0
    g = BR.reduce(v, c, s)
    out, outw = BR.residual(v, y, None, c, s), BR.residual(v, y, w, c, s)
    assert np.array_equal(_bits(out), _bits(g - y))
    assert z.sum() == 4 and not _bits(outw[z]).any() and np.array_equal(_bits(outw[~z]), _bits((w * (g - y))[~z]))
    Jn = J.copy()
    Jn[:, 7], Jn[:, m + 8] = np.nan, np.inf                          # node 0 of bin 7 (zero weight) and node 1 of bin 8
    Jw = BR.jacobian(Jn, w, c, s)
    for j in range(n):
        gj = BR.reduce(J[j], c, s)
        keep = ~z
        keep[8] = False
        assert not _bits(Jw[j][z]).any() and np.array_equal(_bits(Jw[j][keep]), _bits((w * gj)[keep])) and not np.isfinite(Jw[j][8])


def test_identities():
    rng = np.random.default_rng(2)
    m = 50
    J = rng.standard_normal((3, m))
    J[0, 4], J[1, 9] = 0.0, -0.0
    # Q = 1, c = [1.0], no scale: unchanged up to the sign of zero (+0.0 + (-0.0) = +0.0)
    g = BR.jacobian(J, None, [1.0])
    assert np.array_equal(g, J) and np.array_equal(_bits(g[J != 0]), _bits(J[J != 0])) and _bits(g[1, 9:10])[0] == 0 and _bits(g[0, 4:5])[0] == 0
    # "mean" of a constant whose partial sums are exact returns the constant: the halved weights of the orders 1 and 2 are 1
    # and (1/2, 1/2) -- any constant --, and a constant of few bits under every order survives the rounding of c v
    for order in ORDERS:
        b = Binned(np.arange(m), np.arange(m) + 1.0, order=order, mode="mean")
        assert b.scale is None and np.array_equal(_bits(b.c), _bits(0.5 * _rule(order)[1]))
        for cst in ([3.7, -1e-300, 1.1e300, np.pi] if order <= 2 else []):
            assert np.array_equal(_bits(BR.reduce(np.full(order * m, cst), b.c)), _bits(np.full(m, cst))), (order, cst)
    for c, consts in (([0.25, 0.25, 0.5], [3.7, np.pi]), ([0.125, 0.125, 0.25, 0.5], [np.e]), ([0.5, 0.25, 0.125, 0.125], [3.0, -80.5])):
        for cst in consts:
            b = Binned(np.arange(m), np.arange(m) + 2.0, mode="mean", rule=(np.linspace(-1, 1, len(c)), 2.0 * np.array(c)))
            assert np.array_equal(_bits(b.c), _bits(np.array(c)))
            assert np.array_equal(_bits(BR.reduce(np.full(len(c) * m, cst), b.c)), _bits(np.full(m, cst))), (c, cst)
    # "integral" of a constant density over bins of width 2^k is the constant times the width, exactly, under orders 1 and 2
    for order in (1, 2):
        b = Binned(np.arange(m) * 0.25, np.arange(m) * 0.25 + 0.25, order=order)
        assert np.array_equal(_bits(BR.reduce(np.full(order * m, 3.7), b.c, b.scale[0])), _bits(np.full(m, 3.7 * 0.25)))


# ---------------------------------------------------------------------------------------------------------------------
# nlh_bin_rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", ORDERS)
def test_rule_nodes_against_leggauss(Q):
    """The nodes of nlh_bin_rule within 2^-52 absolute of numpy.polynomial.legendre.leggauss, ascending and symmetric."""
    xi, c = _rule(Q)
    x0, c0 = BC.leggauss(Q)
    print(f"bin rule Q={Q}: nodes differ from leggauss by at most {np.abs(xi - x0).max():.3g} (allowed {2.0 ** -52:.3g})")
    assert (np.abs(xi - x0) <= 2.0 ** -52).all()
    assert (np.diff(xi) > 0).all() and np.array_equal(xi, -xi[::-1]) and np.array_equal(c, c[::-1])


@pytest.mark.parametrize("Q", ORDERS)
def test_rule_weights_against_leggauss(Q):
    """The weights of nlh_bin_rule within 2^-52 absolute of numpy.polynomial.legendre.leggauss."""
    xi, c = _rule(Q)
    x0, c0 = BC.leggauss(Q)
    print(f"bin rule Q={Q}: weights differ from leggauss by at most {np.abs(c - c0).max():.3g} (allowed {2.0 ** -52:.3g})")
    assert (np.abs(c - c0) <= 2.0 ** -52).all()


def _legendre(Q, x):
    """(P_Q(x), P_Q'(x)) in rational arithmetic."""
    p0, p1 = Fraction(1), x
    if Q == 0:
        return p0, Fraction(0)
    for k in range(2, Q + 1):
        p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
    return p1, Q * (x * p1 - p0) / (x * x - 1)


def _exact_rule(Q, start):
    """The exact nodes and weights of the rule, as rationals good to 200 bits: the roots of P_Q by Newton's iteration in
    rational arithmetic from the doubles `start` (truncated to 200 bits per step; quadratic convergence from 1e-16 reaches
    1e-60 in two steps), and c = 2 / ((1 - x^2) P_Q'(x)^2) there."""
    xs, ws = [], []
    for v in start:
        x = Fraction(float(v))
        if x != 0:
            for _ in range(3):
                p, d = _legendre(Q, x)
                x = x - p / d
                x = Fraction(int(x * 2 ** 200), 2 ** 200)
        d = _legendre(Q, x if x != 0 else Fraction(1, 2 ** 300))[1]
        xs.append(x)
        ws.append(2 / ((1 - x * x) * d * d))
    return xs, ws


@pytest.mark.parametrize("Q", ORDERS)
def test_rule_against_the_exact_rule(Q):
    """Every node is the double nearest the exact value.  Every weight lies within 2^-52 of the reference's, so it is held to
    the exact weight by the reference's own error, measured here in rational arithmetic, plus 2^-52."""
    xi, c = _rule(Q)
    xs, ws = _exact_rule(Q, xi)
    c0 = BC.leggauss(Q)[1]
    ref = max(abs(Fraction(float(c0[q])) - ws[q]) for q in range(Q))
    print(f"bin rule Q={Q}: leggauss's weights are off the exact ones by at most {float(ref):.3g}")
    for q in range(Q):
        assert float(xs[q]) == xi[q], (Q, q, float(xs[q]), xi[q])
        err = abs(Fraction(float(c[q])) - ws[q])
        assert err <= ref + Fraction(1, 2 ** 52), (Q, q, float(err))


@pytest.mark.parametrize("Q", ORDERS)
def test_rule_sum_and_monomials(Q):
    """The sequential sum of the weights within 4 ulp of 2; and monomials up to degree 2 Q - 1 integrated over a bin, through
    Binned and the restated transform, to 1e-14 relative."""
    xi, c = _rule(Q)
    tot = 0.0
    for v in c:
        tot = tot + v
    assert abs(tot - 2.0) <= 4 * 2.0 ** -52 * 2.0, tot
    lo, hi = np.array([0.5, 1.0, -0.25]), np.array([1.75, 1.5, 2.0])      # (a bin across 0 has odd monomials that cancel: skipped below)
    b = Binned(lo, hi, order=Q)
    tq = b.nodes()
    for deg in range(2 * Q):
        got = BR.reduce(tq ** deg, b.c, b.scale[0])
        want = (hi ** (deg + 1) - lo ** (deg + 1)) / (deg + 1)
        rel = np.abs(got - want)[:2] / np.abs(want)[:2]
        assert (rel <= 1e-14).all(), (Q, deg, rel)
        mean = BR.reduce(tq ** deg, Binned(lo, hi, order=Q, mode="mean").c)
        assert (np.abs(mean * (hi - lo) - want)[:2] <= 1e-14 * np.abs(want)[:2]).all()
    if Q < 8:                                                        # and degree 2 Q is NOT exact: the rule has the order it claims
        got = BR.reduce(tq ** (2 * Q), b.c, b.scale[0])
        want = (hi ** (2 * Q + 1) - lo ** (2 * Q + 1)) / (2 * Q + 1)
        assert (np.abs(got - want)[:1] > 1e-13 * np.abs(want)[:1]).all()


def test_rule_refusals():
    from nonlin_amd import _lib
    L = _lib.load()
    xi, c = np.full(8, 7.0), np.full(8, 7.0)
    for Q in (0, -1, 9, 16):
        assert L.nlh_bin_rule(Q, xi.ctypes.data_as(dp), c.ctypes.data_as(dp)) == NL_INVALID_INPUT_ERROR
    assert L.nlh_bin_rule(3, None, c.ctypes.data_as(dp)) == NL_INVALID_INPUT_ERROR
    assert L.nlh_bin_rule(3, xi.ctypes.data_as(dp), None) == NL_INVALID_INPUT_ERROR
    assert (xi == 7.0).all() and (c == 7.0).all()
    for bad in (0, 9, True, 2.0, "3", None):
        with pytest.raises(ValueError):
            _lib.bin_rule(bad)


# ---------------------------------------------------------------------------------------------------------------------
# Binned
# ---------------------------------------------------------------------------------------------------------------------
def test_binned_validation():
    from nonlin_amd import _lib
    b = Binned([0.0, 1.0, 3.0], [1.0, 3.0, 3.5])
    assert (b.m, b.Q, b.shared, b.nvar, b.mode) == (3, 3, True, 1, "integral") and b.scale.shape == (1, 3)
    assert np.array_equal(b.scale[0], [0.5, 1.0, 0.25]) and np.array_equal(_bits(b.c), _bits(_rule(3)[1]))
    assert b.scale_for(5)[0].shape == (3,) and b.scale_for(5)[1] == 1 and b.nodes_for(5).shape == (9,)
    b = Binned(np.zeros((4, 6)), np.ones((4, 6)), order=np.int64(2), mode="MEAN")
    assert (b.m, b.Q, b.shared, b.mode) == (6, 2, False, "mean") and b.scale is None and b.scale_for(4) == (None, 1)
    assert b.nodes().shape == (4, 12)
    with pytest.raises(ValueError):
        b.scale_for(3)
    with pytest.raises(ValueError):
        b.nodes_for(5)
    b = Binned(np.zeros((4, 6)), np.ones((4, 6)), order=8)
    assert b.scale_for(4)[0].shape == (4, 6) and b.scale_for(4)[1] == 0 and b.Q == 8
    e = Binned.edges([0.0, 1.0, 3.0, 3.5], order=2)
    assert np.array_equal(e.nodes(), Binned([0.0, 1.0, 3.0], [1.0, 3.0, 3.5], order=2).nodes()) and e.shared
    r = Binned([0.0], [2.0], rule=([-1.0, 0.0, 1.0], [1 / 3, 4 / 3, 1 / 3]), order="ignored")          # Simpson's rule
    assert r.Q == 3 and np.array_equal(r.nodes(), [0.0, 1.0, 2.0]) and np.array_equal(r.scale[0], [1.0])
    assert Binned([0.0], [1.0], rule=(np.zeros(16), np.ones(16))).Q == 16
    s = b.struct(1234, 0)
    assert (s.Q, s.s, s.shared_s) == (8, 1234, 0) and np.array_equal(_bits(list(s.c)[:8]), _bits(b.c)) and list(s.c)[8:] == [0.0] * 8
    assert Binned([0.0], [1.0], mode="mean").struct(None, 1).s is None
    for lo, hi in (([], []), ([[]], [[]]), (np.zeros((2, 2, 2)), np.ones((2, 2, 2))), ([0.0, 1.0], [1.0]), ([0.0], [np.nan]), ([-np.inf], [0.0]),
                   ([0.0], [0.0]), ([1.0], [0.0]), ("ab", "cd"), (None, None), ([0.0, "x"], [1.0, 2.0]), (0.0, 1.0)):
        with pytest.raises(ValueError):
            Binned(lo, hi)
    for order in (0, 9, -1, 1.0, "3", None, True):
        with pytest.raises(ValueError):
            Binned([0.0], [1.0], order=order)
    for mode in ("sum", 1, None, True):
        with pytest.raises(ValueError):
            Binned([0.0], [1.0], mode=mode)
    for rule in (([], []), ([0.0], [1.0, 1.0]), (np.zeros(17), np.ones(17)), ([np.nan], [1.0]), ([0.0], [np.inf]), "ab", 3, ([[0.0]], [[1.0]]),
                 ([0.0],), (["x"], [1.0])):
        with pytest.raises(ValueError):
            Binned([0.0], [1.0], rule=rule)
    for e in ([0.0], [], [[0.0, 1.0]], "abc", [0.0, 0.0], [1.0, 0.0]):
        with pytest.raises(ValueError):
            Binned.edges(e)
    assert _lib.BIN_MAX_ORDER == 8


@pytest.mark.parametrize("per_problem", [False, True])
def test_nodes_layout(per_problem):
    """nodes(): node-major, entry q m + i = mid_i + half_i * xi_q with mid = 0.5 (lo + hi) and half = 0.5 (hi - lo), bit for
    bit -- shared and per problem."""
    rng = np.random.default_rng(3)
    nprob, m, Q = 3, 7, 5
    lo = np.sort(rng.uniform(0, 10, (nprob, m)), axis=1)
    hi = lo + rng.uniform(0.1, 1.0, (nprob, m))
    if not per_problem:
        lo, hi = lo[0], hi[0]
    b = Binned(lo, hi, order=Q)
    tq = b.nodes()
    assert tq.shape == ((nprob, Q * m) if per_problem else (Q * m,))
    xi = _rule(Q)[0]
    lo2, hi2, tq2 = np.atleast_2d(lo), np.atleast_2d(hi), np.atleast_2d(tq)
    for p in range(len(lo2)):
        for q in range(Q):
            for i in range(m):
                mid, half = 0.5 * (lo2[p, i] + hi2[p, i]), 0.5 * (hi2[p, i] - lo2[p, i])
                assert tq2[p, q * m + i] == mid + half * xi[q]
                assert b.scale[p, i] == half
    assert np.array_equal(_bits(tq), _bits(BR.nodes(lo, hi, xi)))
    tq[...] = 0.0                                                    # a copy: the object keeps its own
    assert (b.nodes() != 0.0).any()


@pytest.mark.parametrize("mode", ["integral", "mean"])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_pixels_against_a_double_loop(order, mode):
    """Binned.pixels: node q = a order + b at (x node a, y node b), weight c_a c_b (a quarter of it under "mean"), scale
    half_x half_y under "integral" -- and the rule integrates x^i y^j up to degree 2 order - 1 in each variable."""
    rng = np.random.default_rng(order)
    nprob, m = 2, 5
    xlo, ylo = rng.uniform(0, 3, (nprob, m)), rng.uniform(-1, 1, (nprob, m))
    xhi, yhi = xlo + rng.uniform(0.2, 1.0, (nprob, m)), ylo + rng.uniform(0.2, 1.0, (nprob, m))
    px = Binned.pixels((xlo, xhi), (ylo, yhi), order=order, mode=mode)
    xi, c = _rule(order)
    Q = order * order
    assert (px.Q, px.m, px.nvar, px.shared) == (Q, m, 2, False)
    tq = px.nodes()
    assert tq.shape == (2, nprob, Q * m)
    for p in range(nprob):
        for i in range(m):
            hx, hy = 0.5 * (xhi[p, i] - xlo[p, i]), 0.5 * (yhi[p, i] - ylo[p, i])
            for a in range(order):
                for b in range(order):
                    q = a * order + b
                    assert tq[0, p, q * m + i] == 0.5 * (xlo[p, i] + xhi[p, i]) + hx * xi[a]
                    assert tq[1, p, q * m + i] == 0.5 * (ylo[p, i] + yhi[p, i]) + hy * xi[b]
                    assert px.c[q] == (c[a] * c[b] if mode == "integral" else 0.25 * (c[a] * c[b]))
            if mode == "integral":
                assert px.scale[p, i] == hx * hy
    assert (px.scale is None) == (mode == "mean")
    for i in range(2 * order):
        for j in range(2 * order):
            got = BR.reduce(tq[0] ** i * tq[1] ** j, px.c, px.scale)
            want = (xhi ** (i + 1) - xlo ** (i + 1)) / (i + 1) * (yhi ** (j + 1) - ylo ** (j + 1)) / (j + 1)
            if mode == "mean":
                want = want / ((xhi - xlo) * (yhi - ylo))
            assert (np.abs(got - want) <= 1e-13 * np.abs(want) + 1e-15).all(), (i, j)
    sh = Binned.pixels((xlo[0], xhi[0]), (ylo[0], yhi[0]), order=order, mode=mode)
    assert sh.shared and sh.nodes().shape == (2, Q * m) and np.array_equal(sh.nodes(), tq[:, 0])
    for bad in (0, 5, True, 2.0, None):
        with pytest.raises(ValueError):
            Binned.pixels((xlo, xhi), (ylo, yhi), order=bad)
    for x, y in (((xlo, xhi), (ylo[0], yhi[0])), ((xlo,), (ylo, yhi)), (xlo, ylo[:1]), ((xhi, xlo), (ylo, yhi)), ((xlo, xhi), (ylo, ylo))):
        with pytest.raises(ValueError):
            Binned.pixels(x, y, order=order)
    with pytest.raises(ValueError):
        Binned.pixels((xlo, xhi), (ylo, yhi), mode="sum")


# ---------------------------------------------------------------------------------------------------------------------
# the error codes that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_library_refuses_device_work_without_a_handle():
    from nonlin_amd import _lib
    L = _lib.load()
    one = np.ones(16)
    bn = Binned([0.0], [1.0]).struct(one.ctypes.data, 1)
    out = C.c_void_p(7)
    fcn = C.cast(L.nlh_curve_device_fcn, _lib.DEVFCN)
    none = C.cast(None, _lib.DEVFCN)
    assert L.nlh_bin_wrap(None, C.byref(bn), one.ctypes.data, None, fcn, none, None, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    assert L.nlh_bin_apply_batch(None, C.byref(bn), 1, 1, 1, None, None) == NLH_ERR_BAD_HANDLE
    # a malformed context is refused by the launchers before any launch (no device is touched: this runs without one)
    for fn in (L.nlh_bin_device_fcn, L.nlh_bin_device_jac):
        assert fn(None, None, 1, None, 2, None, 8, None) == NL_INVALID_INPUT_ERROR
        junk = (C.c_uint32 * 256)()
        assert fn(C.byref(junk), None, 1, None, 2, 1, 8, 1) == NL_INVALID_INPUT_ERROR
    L.nlh_bin_unwrap(None)


# ---------------------------------------------------------------------------------------------------------------------
# the study
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_counts_and_the_restated_integral():
    """The histogram of the study: its exact counts sum to the events inside the window, and the order-8 rule reproduces them
    to rounding."""
    for h in BC.HS:
        y = BC.exact_counts(h)
        assert abs(y.sum() - BC.COUNTS) <= 1e-9 * BC.COUNTS
        e = BC.edges(h)
        b = Binned.edges(e, order=8)
        import curve_restatement as R
        got = BR.reduce(R.model(R.GAUSS, 1, -1, BC.truth(h), b.nodes()), b.c, b.scale[0])
        assert (np.abs(got - y) <= 1e-9 * y.max()).all(), h


def test_study(oracle):
    """The README's table, re-measured on the oracle with the restated operation order.  Asserted: noise-free, the bias of the
    width under the centre value times the bin width is within 10 % of Sheppard's sqrt(1 + h^2 / 12 sigma^2) - 1 at every h,
    and under the rule of 3 nodes it is below 1e-3 in magnitude at every h.  The noisy rows are recorded as they fall; and
    tests/golden/bin_study.json records what is measured here."""
    got = BC.study(oracle)
    for h in BC.HS:
        row = got["noise_free"][f"h{h:g}"]
        print(f"bin study h/sigma {h:g}: Sheppard {row['sheppard']:+.3e}, " + ", ".join(f"order {o} {row[f'order{o}']:+.3e}" for o in BC.ORDERS))
        assert abs(row["order1"] - row["sheppard"]) <= 0.1 * row["sheppard"], (h, row)
        assert abs(row["order3"]) < 1e-3, (h, row)
    for o in (1, 3):
        v = got["noisy"][f"order{o}"]
        print(f"bin study noisy h/sigma {BC.NOISY_H:g} order {o}: failed {v['failed']}, sigma {v['sigma_mean']:.5f} +- {v['sigma_stderr']:.5f}, "
              f"scatter {v['sigma_scatter']:.5f}")
    with open(BC.STUDY_GOLDEN) as fh:
        rec = json.load(fh)

    def same(a, b, path):
        if isinstance(a, dict):
            assert isinstance(b, dict) and set(a) == set(b), path
            for k in a:
                same(a[k], b[k], path + (k,))
        elif isinstance(a, float) and path[-1] not in ("failed",):
            # (the noise-free biases of the higher orders are differences of 1: absolute 1e-9 is 1e-9 of sigma)
            assert b == pytest.approx(a, rel=1e-6, abs=1e-9), path
        else:
            assert a == b, path
    same(got, rec, ())
