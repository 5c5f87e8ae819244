"""CPU tests of the global fits (include/nonlin_hip.h: nlh_group_*): the group object's order, shapes, index and refusals, the
Python Group by index and by name, the numpy restatement (tests/group_restatement.py) on the CPU oracle's solver, the error
codes that need no device, and the study that motivates the feature -- a shared decay rate from 8 data sets at once against
the 8 separate fits -- redone with the oracle and held to tests/golden/group_study.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import curve_restatement as R
import group_cases as GC
import group_restatement as GR

NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3
ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
HERE = os.path.dirname(os.path.abspath(__file__))


def _create(nfull, shared, nsets, nshared=None):
    from nonlin_amd import _lib
    L = _lib.load()
    sh = None if shared is None else np.ascontiguousarray(shared, dtype=np.int32)
    g = C.c_void_p(7)
    rc = L.nlh_group_create(nfull, len(sh) if nshared is None else nshared, None if sh is None else sh.ctypes.data_as(ip), nsets, C.byref(g))
    return rc, g


def test_create_refusals():
    from nonlin_amd import _lib
    L = _lib.load()
    rc, g = _create(3, [1], 8)
    assert rc == 0 and g.value
    L.nlh_group_destroy(g)
    bad = [("nfull < 1", 0, [], 2, None), ("nfull > NLH_PMAP_MAX_N", 8193, [], 2, None), ("nsets < 1", 3, [1], 0, None),
           ("nsets negative", 3, [1], -4, None), ("an index below range", 3, [-1], 2, None), ("an index above range", 3, [3], 2, None),
           ("an index repeated", 3, [1, 1], 2, None), ("nshared negative", 3, [1], 2, -1), ("nshared > nfull", 3, [0, 1, 2, 0], 2, None),
           ("shared NULL with nshared > 0", 3, None, 2, 1), ("n beyond int32", 8192, [], 1 << 20, None)]
    for what, nfull, shared, nsets, ns in bad:
        rc, g = _create(nfull, shared, nsets, ns)
        assert rc == NL_INVALID_INPUT_ERROR and not g.value, what
    assert L.nlh_group_create(3, 0, None, 2, None) == NL_INVALID_INPUT_ERROR
    for nfull, shared, nsets, ns in ((3, None, 2, 0), (3, [0, 1, 2], 1, None), (3, [2, 0, 1], 9, None), (1, [], 1, None)):
        rc, g = _create(nfull, shared, nsets, ns)                       # nothing shared (NULL will do), everything shared, G = 1
        assert rc == 0 and g.value
        L.nlh_group_destroy(g)
    L.nlh_group_destroy(None)
    s = [C.c_int32(5) for _ in range(4)]
    L.nlh_group_shape(None, *[C.byref(v) for v in s])
    assert [v.value for v in s] == [0, 0, 0, 0]
    assert L.nlh_group_index(None, 0, 0) == -1


def test_order_shape_and_index():
    """The order of the outer unknowns is part of the interface: shared first, ascending; then per data set its local ones,
    ascending -- whatever the order `shared` is given in."""
    import nonlin_amd as nl
    specs = [(7, (1, 4), 3), (7, (4, 1), 3), (7, (), 2), (7, tuple(range(7)), 5), (3, (1,), 8), (9, (8, 0, 3), 1), (1, (), 4), (33, (32, 5), 6)]
    for nfull, shared, G in specs:
        g = nl.Group(nfull, shared=shared, nsets=G)
        T = GR.tables(nfull, shared, G)
        S, L = len(shared), nfull - len(shared)
        assert (g.nparams, g.nshared, g.nsets, g.nouter) == (nfull, S, G, S + G * L) and g.nouter == GR.nouter(T)
        got = np.array([[g.index(s, k) for k in range(nfull)] for s in range(G)])
        assert np.array_equal(got, GR.outer_index(T)), (nfull, shared, G)
        # written out: shared parameter number s is outer unknown s; local number l of data set s is S + s L + l
        for j, k in enumerate(sorted(shared)):
            assert all(g.index(s, k) == j for s in range(G))
        for l, k in enumerate(k for k in range(nfull) if k not in shared):
            assert all(g.index(s, k) == S + s * L + l for s in range(G))
        assert sorted(set(got.ravel())) == list(range(g.nouter))       # every outer unknown is somebody's parameter
        for s, k in ((-1, 0), (G, 0), (0, -1), (0, nfull)):
            assert g.lib.nlh_group_index(g.ptr, s, k) == -1
            with pytest.raises(IndexError):
                g.index(s, k)
        g.close()
    for bad in (dict(nparams=0), dict(nparams=3, shared=(3,)), dict(nparams=3, shared=(-1,)), dict(nparams=3, shared=(1, 1)),
                dict(nparams=3, shared=(1,), nsets=0)):
        with pytest.raises(ValueError):
            nl.Group(**bad)
    e = nl.Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
    by_name, by_index = nl.Group.for_expr(e, shared=("k",), nsets=8), nl.Group(3, shared=(1,), nsets=8)
    assert by_name.nouter == by_index.nouter == 17
    assert [by_name.index(s, k) for s in range(8) for k in range(3)] == [by_index.index(s, k) for s in range(8) for k in range(3)]
    with pytest.raises(ValueError):
        nl.Group.for_expr(e, shared=("b",), nsets=2)


def test_restatement_gather_expand_scatter():
    rng = np.random.default_rng(5)
    for nfull, shared, G in ((7, (1, 4), 3), (7, (), 2), (4, (0, 1, 2, 3), 5), (3, (1,), 8), (5, (4,), 1)):
        T = GR.tables(nfull, shared, G)
        n, S = GR.nouter(T), len(shared)
        x = rng.standard_normal((4, n))
        P = GR.expand(T, x)
        assert P.shape == (4 * G, nfull) and np.array_equal(GR.gather(T, P), x)     # expand then gather: the identity
        assert np.array_equal(GR.expand(T, x[2]), P[2 * G:3 * G])                   # one group alone
        for k in shared:
            assert all(np.array_equal(P[g::G, k], P[0::G, k]) for g in range(G))   # a shared parameter is equal across the group
        full = rng.standard_normal((4 * G, nfull))
        xg = GR.gather(T, full)
        back = GR.expand(T, xg)
        loc = [k for k in range(nfull) if k not in shared]
        assert np.array_equal(back[:, loc], full[:, loc])
        for k in shared:                                                            # a shared parameter: data set 0's value
            assert np.array_equal(back[:, k], np.repeat(full[0::G, k], G))
        m = 6
        Jf = [rng.standard_normal((m, nfull)) for g in range(G)]
        J = GR.scatter(T, Jf)
        assert J.shape == (G * m, n)
        # J is d(stacked residual) / d(outer unknowns): Jf of the block-diagonal problem times the 0 / 1 matrix of expand
        E = np.zeros((G * nfull, n))
        for g in range(G):
            for k in range(nfull):
                E[g * nfull + k, GR.index(T, g, k)] = 1.0
        B = np.zeros((G * m, G * nfull))
        for g in range(G):
            B[g * m:(g + 1) * m, g * nfull:(g + 1) * nfull] = Jf[g]
        assert np.array_equal(J, B @ E)                                             # (one non-zero term per sum: exact)
        assert not np.signbit(J[J == 0.0]).any()
        for g in range(G):                                                          # a local column is +0.0 outside its own rows
            for l in range(nfull - S):
                col = J[:, S + g * (nfull - S) + l].copy()
                col[g * m:(g + 1) * m] = 0.0
                assert (col == 0.0).all()


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("case", GC.CASES)
def test_stacked_problem_recovers_the_truth(oracle, case, analytic):
    """oracle.lm_solve on the restated stacked problem of a noise-free group returns 0 and the truth: the restatement is a
    correct statement of a global fit.  With forward differences the callback is entered fcn_count + n * jacobian_count times:
    n outer unknowns, so (n + 1) G inner evaluations per Jacobian (the reference's fcn_count does not count them)."""
    kind, K, B, m, G, shared = case
    kd, N = R.KINDS[kind], R.nparams(R.KINDS[kind], K, B)
    t, y, xt, x0 = GC.problems(kind, K, B, m, G, shared, ngroup=2, sigma=0.0)
    T = GR.tables(N, shared, G)
    n = GR.nouter(T)
    oo = oracle.default_options(max_evals=GC.MAX_EVALS)
    for p in range(2):
        d = slice(p * G, (p + 1) * G)
        f, j = GR.stacked(T, lambda g, q: R.residual(kd, K, B, q, t[d][g], y[d][g]), lambda g, q: R.jacobian(kd, K, B, q, t[d][g]))
        rec = []
        rc, xo, fo, ib = oracle.lm_solve(f, G * m, n, GR.gather(T, x0[d])[0], jac=j if analytic else None, opts=oo, record=rec)
        assert rc == 0, (case, p, rc)
        assert len(rec) == ib["fcn_count"] + (0 if analytic else n * ib["jacobian_count"])
        got = GR.expand(T, xo)
        assert np.abs(got - xt[d]).max() < 1e-7, np.abs(got - xt[d]).max()
        assert np.abs(fo).max() < 1e-9


def test_library_refuses_device_work_without_a_handle():
    from nonlin_amd import _lib
    L = _lib.load()
    rc, g = _create(3, [1], 2)
    assert rc == 0
    one = np.ones(64)
    p = one.ctypes.data_as(dp)
    o = _lib.default_options()
    out = C.c_void_p(7)
    fcn = C.cast(L.nlh_curve_device_fcn, _lib.DEVFCN)
    none = C.cast(None, _lib.DEVFCN)
    assert L.nlh_group_wrap(None, g, fcn, none, None, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    assert L.nlh_group_gather_batch(None, g, 1, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_group_expand_batch(None, g, 1, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_group_sigma_batch(None, g, 1, None, None, None) == NLH_ERR_BAD_HANDLE
    out = C.c_void_p(7)
    assert L.nlh_group_model_create(None, None, g, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    tail = (0, None, 0, 0, 0.0)
    assert L.nlh_curve_fit_batch_group(None, C.byref(o), 2, 1, 0, 2, 8, None, 0, None, None, 1, None, None, g, *tail, None, None, None, None,
                                       None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_curve_fit_batch_group_h(None, C.byref(o), 2, 1, 0, 2, 8, p, 0, p, None, 1, None, None, g, *tail, p, p, None, None, None,
                                         None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_fit_batch_group(None, C.byref(o), None, 2, 8, None, 0, None, None, 1, None, None, g, *tail, None, None, None, None,
                                      None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_fit_batch_group_h(None, C.byref(o), None, 2, 8, p, 0, p, None, 1, None, None, g, *tail, p, p, None, None, None, None,
                                        None, None) == NLH_ERR_BAD_HANDLE
    # a malformed context is refused by the launchers before any launch (no device is touched: this runs without one)
    for fn in (L.nlh_group_device_fcn, L.nlh_group_device_jac):
        assert fn(None, None, 1, None, 2, None, 8, None) == NL_INVALID_INPUT_ERROR
        junk = (C.c_uint32 * 64)()
        assert fn(C.byref(junk), None, 1, None, 2, 1, 8, 1) == NL_INVALID_INPUT_ERROR
    L.nlh_group_destroy(g)


def _decay_res(t, y):
    return lambda g, q: (q[0] * np.exp(-(q[1] * t)) + q[2]) - y[g]


def _decay_jac(t):
    def jac(g, q):
        e = np.exp(-(q[1] * t))
        return np.stack([e, -((q[0] * t) * e), np.ones_like(t)], axis=1)
    return jac


def study(oracle):
    """The scatter of the decay rate k from the 1,200 separate fits and from the 150 global fits of the same data."""
    S = GC.STUDY
    ngroup, G, m = S["ngroup"], S["G"], S["m"]
    t, y, xt = GC.study_data(**S)
    oo = oracle.default_options(max_evals=GC.MAX_EVALS)
    one, T = GR.tables(3, (), 1), GR.tables(3, (1,), G)
    x0 = np.array([50.0, 1.2, 0.0])
    ksep, kglob = np.empty(ngroup * G), np.empty(ngroup)
    for p in range(ngroup * G):
        f, j = GR.stacked(one, _decay_res(t, y[p:p + 1]), _decay_jac(t))
        rc, xo, fo, ib = oracle.lm_solve(f, m, 3, x0, jac=j, opts=oo)
        assert rc == 0, p
        ksep[p] = xo[1]
    for p in range(ngroup):
        f, j = GR.stacked(T, _decay_res(t, y[p * G:(p + 1) * G]), _decay_jac(t))
        rc, xo, fo, ib = oracle.lm_solve(f, G * m, GR.nouter(T), GR.gather(T, np.tile(x0, (G, 1)))[0], jac=j, opts=oo)
        assert rc == 0, p
        kglob[p] = xo[GR.index(T, 0, 1)]
    sep, glob = float(np.std(ksep - 1.0)), float(np.std(kglob - 1.0))
    return {"scatter_k_separate": sep, "scatter_k_global": glob, "ratio": sep / glob}


def test_study_global_fit_gains_sqrt_G(oracle):
    """150 groups of G = 8 decays a exp(-k t) + c with one k: adding Fisher information predicts that the global fit's k
    scatters sqrt(8) = 2.83 times less than a separate fit's, and plain numpy measured 2.82.  2.0 leaves room for the 5 %
    sampling error of 150 groups.  The values are recorded in tests/golden/group_study.json, which this test reproduces."""
    got = study(oracle)
    print("group study:", got)
    assert got["ratio"] > 2.0
    with open(os.path.join(HERE, "golden", "group_study.json")) as fh:
        want = json.load(fh)
    for k in ("scatter_k_separate", "scatter_k_global", "ratio"):
        assert abs(got[k] - want[k]) <= 1e-6 * want[k], (k, got[k], want[k])
