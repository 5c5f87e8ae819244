"""CPU tests of the parameter maps (include/nonlin_hip.h: nlh_pmap_*): every refusal of nlh_pmap_create, the read-back, the
Python ParamMap by index and by name, the numpy restatement (tests/pmap_restatement.py) held to the dense matrix of the
map, the error codes that need no device, and the cases of tests/pmap_cases.py on the CPU oracle's solver."""
import ctypes as C

import numpy as np
import pytest

import curve_restatement as R
import pmap_cases as PC
import pmap_restatement as PR

EPS = 2.0 ** -52
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NLH_ERR_BAD_HANDLE = 201, 211, -3
ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def _create(nfull, kind, src=None, scale=None, offset=None):
    from nonlin_amd import _lib
    L = _lib.load()
    a = lambda v, t: None if v is None else np.ascontiguousarray(v, dtype=t)
    kind, src, scale, offset = a(kind, np.int32), a(src, np.int32), a(scale, np.float64), a(offset, np.float64)
    p = lambda v, t: None if v is None else v.ctypes.data_as(t)
    pm = C.c_void_p(7)
    rc = L.nlh_pmap_create(nfull, p(kind, ip), p(src, ip), p(scale, dp), p(offset, dp), C.byref(pm))
    return rc, pm


def test_create_refusals():
    from nonlin_amd import _lib
    L = _lib.load()
    ok = dict(kind=[0, 2, 1], src=[0, 0, 0], scale=[1.0, 2.0, 1.0], offset=[0.0, 0.5, 0.0])
    rc, pm = _create(3, **ok)
    assert rc == 0 and pm.value
    L.nlh_pmap_destroy(pm)
    bad = [
        ("nfull < 1", 0, ok),
        ("nfull > NLH_PMAP_MAX_N", 8193, dict(kind=[0] * 8193)),
        ("a kind outside 0 .. 2", 3, dict(ok, kind=[0, 3, 1])),
        ("a negative kind", 3, dict(ok, kind=[0, -1, 1])),
        ("source below range", 3, dict(ok, src=[0, -1, 0])),
        ("source above range", 3, dict(ok, src=[0, 3, 0])),
        ("source is itself", 3, dict(ok, src=[0, 1, 0])),
        ("source is tied (a chain)", 3, dict(kind=[0, 2, 2], src=[0, 0, 1], scale=[1.0, 2.0, 2.0], offset=[0.0, 0.0, 0.0])),
        ("scale inf", 3, dict(ok, scale=[1.0, np.inf, 1.0])),
        ("scale nan", 3, dict(ok, scale=[1.0, np.nan, 1.0])),
        ("offset inf", 3, dict(ok, offset=[0.0, -np.inf, 0.0])),
        ("offset nan", 3, dict(ok, offset=[0.0, np.nan, 0.0])),
        ("scale 0.0", 3, dict(ok, scale=[1.0, 0.0, 1.0])),
        ("scale -0.0", 3, dict(ok, scale=[1.0, -0.0, 1.0])),
        ("no free parameter", 3, dict(kind=[1, 2, 1], src=[0, 0, 0], scale=[1.0, 2.0, 1.0], offset=[0.0, 0.0, 0.0])),
        ("all fixed", 2, dict(kind=[1, 1])),
        ("a tie without tables", 3, dict(kind=[0, 2, 1])),
    ]
    for what, nfull, kw in bad:
        rc, pm = _create(nfull, **kw)
        assert rc == NL_INVALID_INPUT_ERROR and not pm.value, what
    # what is read only at tied positions may hold anything elsewhere; nothing tied: all three may be NULL
    rc, pm = _create(3, kind=[0, 2, 1], src=[99, 0, -5], scale=[np.nan, 2.0, 0.0], offset=[np.inf, 0.5, np.nan])
    assert rc == 0
    L.nlh_pmap_destroy(pm)
    rc, pm = _create(8192, kind=[0] * 8192)
    assert rc == 0
    L.nlh_pmap_destroy(pm)
    rc, pm = _create(2, kind=[1, 0])
    assert rc == 0
    L.nlh_pmap_destroy(pm)
    # a tie to a FIXED source is allowed: a derived constant
    rc, pm = _create(3, kind=[0, 2, 1], src=[0, 2, 0], scale=[1.0, 2.0, 1.0], offset=[0.0, 0.5, 0.0])
    assert rc == 0
    L.nlh_pmap_destroy(pm)
    assert L.nlh_pmap_create(3, None, None, None, None, C.byref(pm)) == NL_INVALID_INPUT_ERROR
    assert L.nlh_pmap_tables(None, None, None, None, None, None) == NL_INVALID_INPUT_ERROR
    L.nlh_pmap_destroy(None)


def test_shape_and_tables_read_back():
    import nonlin_amd as nl
    assert (nl.PMAP_FREE, nl.PMAP_FIXED, nl.PMAP_TIED) == (PR.FREE, PR.FIXED, PR.TIED) == (0, 1, 2)
    specs = [(7, [6], {5: (2, 1.25, 0.0)}), (9, [0, 4], {8: (4, -2.0, 0.5), 2: (3, 0.5, -1.0), 7: (3, 3.0, 0.0)}), (4, [], {}),
             (5, [1, 2, 3, 4], {})]
    for (kind, K, B, m), mp in PC.PAIRS:
        specs.append((R.nparams(R.KINDS[kind], K, B),) + PC.map_spec(mp, K, B))
    for nfull, fixed, tied in specs:
        pm = nl.ParamMap(nfull, fixed=fixed, tied=tied)
        want = PR.tables(nfull, fixed, tied)
        assert (pm.nfull, pm.nfree, pm.ntied) == (nfull, len(want[4]), len(tied))
        for g, w in zip(pm.tables(), want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (nfull, fixed, tied)
        assert list(want[4]) == sorted(want[4]) and all(want[1][k] == j for j, k in enumerate(want[4]))
        assert all(want[1][k] == -1 for k in fixed)
        pm.close()
    s = [C.c_int32(5) for _ in range(3)]
    nl._lib.load().nlh_pmap_shape(None, *[C.byref(v) for v in s])
    assert [v.value for v in s] == [0, 0, 0]


def test_param_map_by_index_and_by_name():
    import nonlin_amd as nl
    for bad in (dict(nfull=0), dict(nfull=3, fixed=(3,)), dict(nfull=3, fixed=(-1,)), dict(nfull=3, tied={1: (3, 1.0, 0.0)}),
                dict(nfull=3, tied={1: (1, 1.0, 0.0)}), dict(nfull=3, tied={1: (2, 1.0, 0.0), 2: (0, 1.0, 0.0)}),
                dict(nfull=3, tied={1: (0, 0.0, 0.0)}), dict(nfull=3, tied={1: (0, float("nan"), 0.0)}),
                dict(nfull=3, tied={1: (0, 1.0, float("inf"))}), dict(nfull=2, fixed=(0, 1)), dict(nfull=3, fixed=(1,), tied={1: (0, 1.0, 0.0)}),
                dict(nfull=8193)):
        with pytest.raises(ValueError):
            nl.ParamMap(**bad)
    e = nl.Expr("a1/(1+((t-m1)/w1)^2) + a2/(1+((t-m2)/w2)^2) + c", ("t",), ("a1", "m1", "w1", "a2", "m2", "w2", "c"))
    by_name = nl.ParamMap.for_expr(e, fixed=("c",), tied={"w2": ("w1", 1.25, 0.0)})
    by_index = nl.ParamMap(7, fixed=(6,), tied={5: (2, 1.25, 0.0)})
    for g, w in zip(by_name.tables(), by_index.tables()):
        assert np.array_equal(g, w)
    assert (by_name.nfull, by_name.nfree, by_name.ntied) == (7, 5, 1)
    with pytest.raises(ValueError):
        nl.ParamMap.for_expr(e, fixed=("b",))
    with pytest.raises(ValueError):
        nl.ParamMap.for_expr(e, tied={"w2": ("w3", 1.0, 0.0)})


def _random_map(rng, N):
    """A random valid map: sources are free or fixed, never tied."""
    while True:
        kind = rng.integers(0, 3, N)
        roots = np.flatnonzero(kind != PR.TIED)
        if (kind == PR.FREE).any():
            break
    fixed = [int(k) for k in np.flatnonzero(kind == PR.FIXED)]
    tied = {int(k): (int(rng.choice(roots)), float(rng.choice([-1, 1]) * rng.uniform(0.2, 3.0)), float(rng.uniform(-1, 1)))
            for k in np.flatnonzero(kind == PR.TIED)}
    return fixed, tied


def test_contraction_equals_dense_product():
    """contract(Jf) against Jf @ S, S the dense N x n matrix of the map.  Column j of the contraction is a sequential sum
    of L = (ties of the column + 1) terms: every term but the first is rounded once as a product and every term takes part
    in at most L - 1 additions, each within the unit roundoff eps / 2, so the sum lies within L (eps / 2) sum|terms| of the
    exact value to first order.  The bound L eps sum|terms| -- derived from the sum length, not measured -- is held against
    the exact product, formed in extended precision so that the reference's own rounding needs no allowance."""
    rng = np.random.default_rng(7)
    for trial in range(40):
        N, m = int(rng.integers(2, 14)), int(rng.integers(1, 40))
        fixed, tied = _random_map(rng, N)
        T = PR.tables(N, fixed, tied)
        Jf = rng.standard_normal((m, N))
        got = PR.contract(T, Jf)
        S = PR.dense(T)
        exact = Jf.astype(np.longdouble) @ S.astype(np.longdouble)
        terms = np.abs(Jf) @ np.abs(S)
        for j in range(len(T[4])):
            L = len(PR.ties_of(T, j)) + 1
            if L == 1:
                assert np.array_equal(got[:, j], Jf[:, T[4][j]])        # an untied column is a copy
            bound = L * EPS * terms[:, j]
            assert (np.abs(got[:, j].astype(np.longdouble) - exact[:, j]) <= bound).all(), (trial, j, L)
        # columns of fixed parameters, and of parameters tied to fixed ones, are not read
        jk, g = PR.factors(T)
        Jn = Jf.copy()
        Jn[:, jk < 0] = np.nan
        assert np.array_equal(PR.contract(T, Jn), got)


def test_expand_gather_and_the_linear_part():
    rng = np.random.default_rng(9)
    for trial in range(40):
        N = int(rng.integers(2, 14))
        fixed, tied = _random_map(rng, N)
        T = PR.tables(N, fixed, tied)
        kind, index, scale, offset, f2f = T
        full = rng.standard_normal((5, N))
        x = rng.standard_normal((5, len(f2f)))
        p = PR.expand(T, x, full)
        assert np.array_equal(PR.gather(T, p), x)                       # expand then gather: the identity on free positions
        assert np.array_equal(p[:, kind == PR.FIXED], full[:, kind == PR.FIXED])
        for k in np.flatnonzero(kind == PR.TIED):
            assert np.array_equal(p[:, k], scale[k] * p[:, index[k]] + offset[k])
        assert np.array_equal(PR.expand(T, PR.gather(T, full), full)[:, kind != PR.TIED], full[:, kind != PR.TIED])
        assert np.array_equal(PR.expand(T, x[2], full[2]), p[2])        # one problem alone
        # cov_expand is S cov S^T entry by entry, exactly where |g| = 1, and symmetric; no factor: +0.0
        A = rng.standard_normal((len(f2f), len(f2f)))
        cov = A @ A.T
        sigma = np.sqrt(np.diag(cov))
        cf, sf = PR.cov_expand(T, cov, sigma)
        S = PR.dense(T)
        assert np.allclose(cf, S @ cov @ S.T, rtol=4 * EPS, atol=0.0)
        jk, g = PR.factors(T)
        assert (cf[jk < 0] == 0.0).all() and (cf[:, jk < 0] == 0.0).all() and (sf[jk < 0] == 0.0).all() and (sf >= 0.0).all()
        assert not np.signbit(cf[jk < 0]).any()
        cn, sn = PR.cov_expand(T, cov, sigma, failed=True)
        assert np.isnan(cn).all() and np.isnan(sn).all()


def test_library_loads_and_refuses_device_work_without_a_handle():
    from nonlin_amd import _lib
    L = _lib.load()
    rc, pm = _create(3, kind=[0, 2, 1], src=[0, 0, 0], scale=[1.0, 2.0, 1.0], offset=[0.0, 0.5, 0.0])
    assert rc == 0
    one = np.ones(16)
    p = one.ctypes.data_as(dp)
    o = _lib.default_options()
    out = C.c_void_p(7)
    fcn = C.cast(L.nlh_curve_device_fcn, _lib.DEVFCN)
    none = C.cast(None, _lib.DEVFCN)
    assert L.nlh_pmap_wrap(None, pm, fcn, none, None, None, 0, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    assert L.nlh_pmap_gather_batch(None, pm, 1, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_pmap_expand_batch(None, pm, 1, None, None, 0, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_pmap_cov_batch(None, pm, 1, None, None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_pmap_model_create(None, None, pm, p, 0, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    assert L.nlh_curve_fit_batch_pmap(None, C.byref(o), 1, 1, -1, 1, 8, None, 0, None, None, 1, None, None, pm, None, None, None, None,
                                      None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_curve_fit_batch_pmap_h(None, C.byref(o), 1, 1, -1, 1, 8, p, 0, p, None, 1, None, None, pm, p, p, None, None, None,
                                        None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_fit_batch_pmap(None, C.byref(o), None, 1, 8, None, 0, None, None, 1, None, None, pm, None, None, None, None, None,
                                     None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_fit_batch_pmap_h(None, C.byref(o), None, 1, 8, p, 0, p, None, 1, None, None, pm, p, p, None, None, None, None,
                                       None, None) == NLH_ERR_BAD_HANDLE
    # with no map the new entry points are the old ones: the old ones' answer
    assert L.nlh_curve_fit_batch_pmap(None, C.byref(o), 1, 1, -1, 1, 8, None, 0, None, None, 1, None, None, None, None, None, None, None,
                                      None, None, None, None) == NLH_ERR_BAD_HANDLE
    # a malformed context is refused by the launchers before any launch (no device is touched: this runs without one)
    for fn in (L.nlh_pmap_device_fcn, L.nlh_pmap_device_jac):
        assert fn(None, None, 1, None, 2, None, 8, None) == NL_INVALID_INPUT_ERROR
        junk = (C.c_uint32 * 64)()
        assert fn(C.byref(junk), None, 1, None, 2, 1, 8, 1) == NL_INVALID_INPUT_ERROR
    L.nlh_pmap_destroy(pm)
    import torch
    if not torch.cuda.is_available():
        import nonlin_amd as nl
        from nonlin_amd.device import DeviceSolver
        with pytest.raises(nl.NonlinHipUnavailable):
            DeviceSolver(0)


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("case,mp", PC.PAIRS)
def test_cases_solve_on_the_reference_path(oracle, case, mp, analytic):
    """The condition the GPU tests assert -- status 0 for the whole batch -- is one these inputs meet on the reference path
    alone: the oracle on the reduced problem with the restatement's expand and contract as callbacks.  With forward
    differences the callback is entered fcn_count + nfree * jacobian_count times: nfree, not N, evaluations per Jacobian
    (the reference's fcn_count itself does not count them)."""
    kind, K, B, m = case
    kd, N = R.KINDS[kind], R.nparams(R.KINDS[kind], K, B)
    t, y, xt, x0 = PC.problems(kind, K, B, m)
    T = PR.tables(N, *PC.map_spec(mp, K, B))
    n = len(T[4])
    assert n < N
    full = PC.full_start(T, xt, x0)
    oo = oracle.default_options(max_evals=PC.MAX_EVALS)
    worst = 0.0
    for p in range(PC.NPROB):
        f = lambda x, out: out.__setitem__(slice(None), R.residual(kd, K, B, PR.expand(T, x, full[p]), t[p], y[p]))
        j = (lambda x, J: J.__setitem__((slice(None), slice(None)), PR.contract(T, R.jacobian(kd, K, B, PR.expand(T, x, full[p]), t[p])))) \
            if analytic else None
        rec = []
        rc, xo, fo, ib = oracle.lm_solve(f, m, n, PR.gather(T, full[p]), jac=j, opts=oo, record=rec)
        assert rc == 0, (case, mp, p, rc)
        assert 3 <= ib["jacobian_count"] <= 8
        assert len(rec) == ib["fcn_count"] + (0 if analytic else n * ib["jacobian_count"])
        worst = max(worst, float(np.abs(PR.expand(T, xo, full[p]) - xt[p]).max()))
    assert worst < 6.1e-3, worst
