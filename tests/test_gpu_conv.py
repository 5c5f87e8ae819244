"""GPU tests of the instrument-response fits (include/nonlin_hip.h: nlh_conv_*): the kernels through the wrapping launchers
against the numpy restatement (tests/conv_restatement.py), bit for bit, over a chosen list of sizes, taps, origins, extensions,
parameter counts, forms, column splits and slicings; zero-weight rows; how a NaN row and a tap that is not finite spread;
nlh_conv_apply_batch; LM and bounded solves through the wrappers against the CPU oracle, alone, inside a parameter map and
inside a group; the error returns."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import conv_cases as CV
import conv_restatement as CR
import curve_cases as CC
import curve_restatement as R
import group_restatement as GR
import pmap_restatement as PM
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

FORMS = [None, "row", "flat"]               # None: the form m selects; a forced form that cannot hold m falls back to it
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR, NLH_ERR_BAD_HANDLE = 201, 211, 212, -3
T = CV.ROW_TILE
LMAX = CR.MAX_L
HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    """Bit for bit, the sign of zero included; NaN against NaN (its payload is the hardware's own)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


class _env:
    """Environment variables for the calls inside (the library reads NLH_CONV_* at every call); None: unset."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.kw}
        for k, v in self.kw.items():
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _dev(ds, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ds.device)


def _launch(ds, fcn, ctx, plist, X, m, jac=False, rc_want=0):
    """One call of a launcher on the points X (numpy [npoints, n]) of the problems plist (None: no dprob, point q is problem
    q): F [npoints, m] or J [npoints, n, m]."""
    npts, n = X.shape
    dX = _dev(ds, X)
    dprob = _dev(ds, plist, np.int32) if plist is not None else None
    out = torch.full((npts, n, m) if jac else (npts, m), np.nan, dtype=torch.float64, device=ds.device)
    stream = torch.cuda.current_stream(ds.device).cuda_stream
    rc = fcn(ds._ctxp(ctx), C.c_void_p(stream), npts, C.c_void_p(dprob.data_ptr()) if dprob is not None else None, n,
             C.c_void_p(dX.data_ptr()), m, C.c_void_p(out.data_ptr()))
    assert rc == rc_want
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _inner(ds, n, m, nprob, seed):
    """An exp-free inner model of n parameters on m rows, bound without weights: the formula a*t (n = 1) or a Lorentzian
    model (n = 3, 4, 5, 9).  Returns (launchers, keep, t, y, x0)."""
    rng = np.random.default_rng(seed)
    if n == 1:
        t = np.tile(np.linspace(-1.0, 1.0, m) if m > 1 else np.array([0.7]), (nprob, 1)) + rng.uniform(-0.1, 0.1, (nprob, m)) / m
        x0 = rng.uniform(0.5, 1.5, (nprob, 1))
        y = x0 * t + 0.01 * rng.standard_normal((nprob, m))
        dt, dy = _dev(ds, t), _dev(ds, y)
        ex = nl.Expr("a*t", ("t",), ("a",))
        return ds.expr_launchers(ex, dt, dy), (ex, dt, dy), t, y, x0
    KK, BB = {3: (1, -1), 4: (1, 0), 5: (1, 1), 9: (2, 2)}[n]
    t, y, xt, x0 = CC.curve_problems("lorentz", KK, BB, m, nprob=nprob, seed=seed, sigma=0.02)
    dt, dy = _dev(ds, t), _dev(ds, y)
    return ds.curve_launchers("lorentz", KK, BB, dt, dy), (dt, dy), t, y, x0


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("case", CV.LAUNCH_CASES, ids=CV.case_id)
def test_launchers_against_restatement(ds, case):
    """k_conv_row and k_conv_flat through the wrapping launchers: F and J of the restatement applied to what the inner
    launchers give for the same points, bit for bit (the sign of zero included) -- with and without dprob, a point list with
    repeated problems, the form m selects and both forced forms, the column split forced, sliced (three slices or more) and
    unsliced, with weights (zeros among them) and without, one kernel for all and one per problem."""
    m, L, origin, ext, n, shared = case
    nprob = 5
    (fcn, jac, ctx), keep, t, y, x0 = _inner(ds, n, m, nprob, seed=1000 * n + m + L)
    rng = np.random.default_rng(m * 31 + L)
    k = rng.standard_normal(L) if shared else rng.standard_normal((nprob, L))
    w = rng.uniform(0.5, 2.0, (nprob, m))
    w[rng.uniform(size=(nprob, m)) < 0.25] = 0.0
    w[:, -1] = 0.0
    w[0, 0] = -0.0
    conv = nl.Convolve(k, origin=origin, extend=ext)
    dy, dw = keep[-1], _dev(ds, w)
    wrapped = {True: ds.conv_launchers(conv, fcn, jac, ctx, dy, dw), False: ds.conv_launchers(conv, fcn, jac, ctx, dy)}
    shapes = [None, list(np.random.default_rng(3).integers(0, nprob, 9)) + [0, 0, nprob - 1]]
    for kk, plist in enumerate(shapes):
        rows = list(range(nprob)) if plist is None else [int(p) for p in plist]
        X = x0[rows] * (1.0 + (0.002 if kk else 0.0) * np.random.default_rng(kk).uniform(-1, 1, (len(rows), n)))
        rawF = _launch(ds, fcn, ctx, rows, X, m)
        rawJ = _launch(ds, jac, ctx, rows, X, m, jac=True)
        kq = k if shared else k[rows]
        plainF = CR.residual(rawF, y[rows], None, kq, origin, CV.EXT[ext])
        plainJ = CR.jacobian(rawJ, None, kq, origin, CV.EXT[ext])
        for weighted in (True, False):
            wq = w[rows] if weighted else None
            wantF = CR.weigh(plainF, wq)
            wantJ = CR.weigh(plainJ, wq[:, None, :] if weighted else None)
            wf, wj, wctx = wrapped[weighted]
            for form in FORMS:
                for split, sliced in ((None, False), (2, False), (n, True)):
                    with _env(NLH_CONV_FORM=form, NLH_CONV_SPLIT=split, NLH_CONV_SCRATCH=2 * (8 * m + 4) if sliced else None):
                        Fg = _launch(ds, wf, wctx, plist, X, m)
                    with _env(NLH_CONV_FORM=form, NLH_CONV_SPLIT=split, NLH_CONV_SCRATCH=2 * (8 * m * n + 4) if sliced else None):
                        Jg = _launch(ds, wj, wctx, plist, X, m, jac=True)
                    what = (case, kk, weighted, form, split, sliced)
                    assert _same(Fg, wantF), what
                    assert _same(Jg, wantJ), what
            if weighted:                                             # zero-weight rows: +0.0 by bit pattern
                assert not _bits(Fg[wq == 0.0]).any() and not _bits(np.moveaxis(Jg, 1, 2)[wq == 0.0]).any()
    for v in wrapped.values():
        v[2].close()


@pytest.mark.parametrize("m,L,origin", [(129, 9, 0), (300, 33, 16), (T + 40, 64, 0), (T + 40, 64, 63), (64, 9, 0)])
def test_nan_rows_spread_as_far_as_the_taps(ds, m, L, origin):
    """conv_apply under ZERO on columns with one NaN row: the rows whose taps do not reach it are bit-equal to the run without
    the NaN, the rows that reach it are NaN -- a NaN in the middle, in the halo of the second row tile, and at row m - 1 with
    a causal kernel (which only row m - 1 itself reads)."""
    rng = np.random.default_rng(m + L)
    nprob, ncol = 3, 2
    k = rng.uniform(0.1, 1.0, L)
    conv = nl.Convolve(k, origin=origin, extend="zero")
    v = rng.standard_normal((nprob, ncol, m))
    clean = ds.conv_apply(conv, _dev(ds, v)).cpu().numpy()
    assert _same(clean, CR.convolve(v, k, origin, CR.ZERO))
    spots = [m // 2, m - 1] + ([T - 3, T + 2] if m > T else [])
    for form in FORMS:
        for s in spots:
            vn = v.copy()
            vn[1, 0, s] = np.nan
            with _env(NLH_CONV_FORM=form):
                got = ds.conv_apply(conv, _dev(ds, vn)).cpu().numpy()
            i = np.arange(m)
            reach = (i + origin - (L - 1) <= s) & (s <= i + origin)      # row i reads s = i + origin - j for some j
            assert reach.any() and (origin != 0 or s != m - 1 or reach.sum() == 1)
            assert np.isnan(got[1, 0, reach]).all(), (form, s)
            keep = np.ones((nprob, ncol, m), dtype=bool)
            keep[1, 0, reach] = False
            assert np.array_equal(_bits(got[keep]), _bits(clean[keep])), (form, s)


@pytest.mark.parametrize("m", [5, 129, T + 9])
def test_a_tap_that_is_not_finite_is_skipped_outside_the_rows(ds, m):
    """ZERO skips a tap outside the rows: nothing is multiplied, so an infinite tap reaches only the rows that read a row with
    it -- the restatement's bits, under every form; and HOLD reads the edge row."""
    rng = np.random.default_rng(m)
    L, origin = 9, 4
    k = rng.standard_normal(L)
    k[0], k[8] = np.inf, -np.inf
    v = rng.uniform(0.5, 1.5, (2, 3, m))
    for ext, e in (("zero", CR.ZERO), ("hold", CR.HOLD)):
        conv = nl.Convolve.__new__(nl.Convolve)                      # (the constructor refuses such a kernel: the device takes it)
        conv.kernel, conv.shared, conv.L, conv.origin, conv.ext = k[None, :], True, L, origin, e
        want = CR.convolve(v, k, origin, e)
        for form in FORMS:
            with _env(NLH_CONV_FORM=form):
                got = ds.conv_apply(conv, _dev(ds, v)).cpu().numpy()
            assert _same(got, want), (ext, form)
    assert np.isfinite(CR.convolve(v, np.where(np.isfinite(k), k, 0.0), origin, CR.ZERO)).all()


def test_apply_batch_shapes_and_kernels(ds):
    """nlh_conv_apply_batch: [nprob, m] and [nprob, ncol, m], a kernel per problem, L > m, both extensions; dout == dv and a
    bad transform are refused."""
    rng = np.random.default_rng(8)
    nprob, ncol, m = 4, 5, 77
    v = rng.standard_normal((nprob, ncol, m))
    for L, origin in ((1, 0), (6, 2), (200, 150), (LMAX, LMAX - 1)):
        k = rng.standard_normal((nprob, L))
        for ext, e in (("zero", CR.ZERO), ("hold", CR.HOLD)):
            conv = nl.Convolve(k, origin=origin, extend=ext)
            assert _same(ds.conv_apply(conv, _dev(ds, v)).cpu().numpy(), CR.convolve(v, k[:, None, :], origin, e))
            assert _same(ds.conv_apply(conv, _dev(ds, v[:, 0])).cpu().numpy(), CR.convolve(v[:, 0], k, origin, e))
    dv, dk = _dev(ds, v), _dev(ds, np.ones(3))
    out = torch.empty_like(dv)
    L_ = ds.lib

    def call(cv, nprob_=nprob, m_=m, ncol_=ncol, src=dv, dst=out, h=ds.h.ptr):
        return L_.nlh_conv_apply_batch(h, C.byref(cv) if cv is not None else None, nprob_, m_, ncol_, src.data_ptr() if src is not None else None,
                                       dst.data_ptr() if dst is not None else None)
    good = _lib.ConvStruct(3, 1, 0, 1, dk.data_ptr())
    assert call(good) == 0
    assert call(good, h=None) == NLH_ERR_BAD_HANDLE
    for bad in (None, _lib.ConvStruct(0, 0, 0, 1, dk.data_ptr()), _lib.ConvStruct(LMAX + 1, 0, 0, 1, dk.data_ptr()),
                _lib.ConvStruct(3, 3, 0, 1, dk.data_ptr()), _lib.ConvStruct(3, -1, 0, 1, dk.data_ptr()),
                _lib.ConvStruct(3, 1, 2, 1, dk.data_ptr()), _lib.ConvStruct(3, 1, -1, 1, dk.data_ptr()), _lib.ConvStruct(3, 1, 0, 1, None)):
        assert call(bad) == NL_INVALID_INPUT_ERROR
    assert call(good, m_=0) == NL_INVALID_INPUT_ERROR and call(good, ncol_=0) == NL_INVALID_INPUT_ERROR and call(good, nprob_=-1) == NL_INVALID_INPUT_ERROR
    assert call(good, dst=dv) == NL_INVALID_INPUT_ERROR and call(good, src=None) == NL_INVALID_INPUT_ERROR and call(good, dst=None) == NL_INVALID_INPUT_ERROR
    assert call(good, nprob_=0, src=None, dst=None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the oracle
KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
LK, LB, LM_, LN = 1, 0, 64, 4                    # the spectrum: one Lorentzian on a constant, 64 rows


def _same_counts(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _line(ds, nprob, weighted, **kw):
    t, y, xt, x0 = CV.line_problems(LK, LB, LM_, nprob, **kw)
    w = None
    if weighted:
        w = np.random.default_rng(6).uniform(0.5, 2.0, (nprob, LM_))
        w[:, [3, 40]] = 0.0
    dt, dy = _dev(ds, t), _dev(ds, y)
    dw = _dev(ds, w) if weighted else None
    inner = ds.curve_launchers("lorentz", LK, LB, dt, dy)
    conv = nl.Convolve(CV.line_shape(), origin=CV.LINE_ORIGIN, extend=CV.LINE_EXTEND)
    return t, y, w, xt, x0, inner, ds.conv_launchers(conv, inner[0], inner[1], inner[2], dy, dw), (dt, dy, dw)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
def test_solves_against_oracle(ds, oracle, analytic, bounded, weighted):
    """lm_solve / cls_solve of the oracle with the restated callbacks (the Lorentzian restatement, then the restated transform)
    under default options, 24 spectra behind a centred 9-tap line shape: status, x, fvec and every count identical."""
    nprob = 24
    t, y, w, xt, x0, inner, (wf, wj, wctx), keep = _line(ds, nprob, weighted)
    lower = upper = None
    if bounded:                                                         # a box some true values lie outside of: bounds that bind
        lower, upper = np.minimum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) - 0.02, np.maximum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) + 0.02
        x0 = np.clip(x0, lower, upper)
    x = _dev(ds, x0)
    if bounded:
        fvec, ibs, status = ds.cls_solve_batch_device(wf, wctx, LM_, x, jac=wj if analytic else None, opts=ds.options(), lower=lower, upper=upper)
    else:
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, LM_, x, jac=wj if analytic else None, opts=ds.options())
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options()
    for p in range(nprob):
        f, j = CV.line_callbacks(LK, LB, t[p], y[p], w[p] if weighted else None, analytic)
        if bounded:
            rc, xo, fo, ibo = oracle.cls_solve(f, LM_, LN, x0[p], jac=j, opts=oo, lower=lower, upper=upper)
        else:
            rc, xo, fo, ibo = oracle.lm_solve(f, LM_, LN, x0[p], jac=j, opts=oo)
        what = (analytic, bounded, weighted, p)
        assert status[p] == rc, (what, status[p], rc)
        assert _same_counts(ibs[p], ibo), (what, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), what
    if not bounded:
        assert set(status) == {0}
    wctx.close()


@pytest.mark.parametrize("analytic", [False, True])
def test_solve_through_a_map_and_through_a_group_against_oracle(ds, oracle, analytic):
    """The convolving pair inside a parameter map (the baseline fixed at its true value) and inside a group (G = 4, the width
    shared): status, x, fvec and every count identical to the oracle's on the restated stacks."""
    nprob, G = 24, 4
    t, y, w, xt, x0, inner, (cf, cj, cctx), keep = _line(ds, nprob, False, shared=(2,), G=G)
    oo = oracle.default_options()
    # the map
    T = PM.tables(LN, (3,), None)
    pm = nl.ParamMap(LN, fixed=(3,))
    full = x0.copy()
    full[:, 3] = xt[:, 3]
    dfull = _dev(ds, full)
    wf, wj, wctx = ds.pmap_launchers(pm, cf, cj, cctx, dfull)
    x = ds.pmap_gather(pm, dfull)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, LM_, x, jac=wj if analytic else None, opts=ds.options())
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    for p in range(nprob):
        f0, j0 = CV.line_callbacks(LK, LB, t[p], y[p], None, True)

        def f(xx, out, f0=f0, p=p):
            f0(PM.expand(T, np.array(xx), full[p]), out)

        def j(xx, J, j0=j0, p=p):
            Jf = np.empty((LM_, LN))
            j0(PM.expand(T, np.array(xx), full[p]), Jf)
            J[:, :] = PM.contract(T, Jf)
        rc, xo, fo, ibo = oracle.lm_solve(f, LM_, 3, PM.gather(T, full[p]), jac=j if analytic else None, opts=oo)
        assert status[p] == rc == 0 and _same_counts(ibs[p], ibo), (p, status[p], rc, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)) and np.array_equal(_bits(fg[p]), _bits(fo)), p
    wctx.close()
    # the group
    TG = GR.tables(LN, (2,), G)
    grp = nl.Group(LN, shared=(2,), nsets=G)
    n, M, ngroup = GR.nouter(TG), G * LM_, nprob // G
    wf, wj, wctx = ds.group_launchers(grp, cf, cj, cctx)
    x = ds.group_gather(grp, _dev(ds, x0))
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, M, x, jac=wj if analytic else None, opts=ds.options())
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    xs = GR.gather(TG, x0)
    for p in range(ngroup):
        d = slice(p * G, (p + 1) * G)
        cbs = [CV.line_callbacks(LK, LB, t[q], y[q], None, True) for q in range(p * G, (p + 1) * G)]

        def res(g, q, cbs=cbs):
            out = np.empty(LM_)
            cbs[g][0](q, out)
            return out

        def jcb(g, q, cbs=cbs):
            J = np.empty((LM_, LN))
            cbs[g][1](q, J)
            return J
        f, j = GR.stacked(TG, res, jcb)
        rc, xo, fo, ibo = oracle.lm_solve(f, M, n, xs[p], jac=j if analytic else None, opts=oo)
        assert status[p] == rc == 0 and _same_counts(ibs[p], ibo), (p, status[p], rc, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)) and np.array_equal(_bits(fg[p]), _bits(fo)), p
    wctx.close()
    cctx.close()


def _decay_inner(ds, model, dt, dy):
    e = nl.Expr(CV.FORMULA, ("t",), CV.PARAMS)
    return (ds.curve_launchers(CV.KIND, CV.K, CV.B, dt, dy) if model == "curve" else ds.expr_launchers(e, dt, dy)), e


def _irf():
    return nl.Convolve(CV.irf(), origin=CV.ORIGIN, extend=CV.EXTEND)


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("model", ["curve", "formula"])
def test_decays_against_oracle(ds, oracle, model, analytic):
    """The decay family by reconvolution, expdecay and a formula with exp: the oracle's lm_solve with the restated transform on
    the DEVICE's own inner residual and Jacobian (a round trip per callback), so that the two solves differ by the exponential
    alone: statuses equal, x within the recorded tolerance (4 x what a last-bit change of exp did to the oracle's own fit)."""
    nprob, m = CV.PERT_NPROB, CV.M
    t, y, xt, x0 = CV.family(nprob)
    dt, dy = _dev(ds, t), _dev(ds, y)
    inner, e = _decay_inner(ds, model, dt, dy)
    wf, wj, wctx = ds.conv_launchers(_irf(), inner[0], inner[1], inner[2], dy)
    x = _dev(ds, x0)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options())
    xg = x.cpu().numpy()
    tol = CV.recorded_tolerance(analytic)
    k, ext = CV.irf(), CV.EXT[CV.EXTEND]
    oo = oracle.default_options()
    worst = 0.0
    for p in range(nprob):
        raw = lambda xx, p=p: _launch(ds, inner[0], inner[2], [p], np.array(xx)[None, :], m)[0]
        rawJ = lambda xx, p=p: _launch(ds, inner[1], inner[2], [p], np.array(xx)[None, :], m, jac=True)[0]
        f = lambda xx, out, p=p, raw=raw: out.__setitem__(slice(None), CR.residual(raw(xx), y[p], None, k, CV.ORIGIN, ext))
        j = (lambda xx, J, rawJ=rawJ: J.__setitem__((slice(None), slice(None)), CR.jacobian(rawJ(xx), None, k, CV.ORIGIN, ext).T)) if analytic else None
        rc, xo, fo, ibo = oracle.lm_solve(f, m, 3, x0[p], jac=j, opts=oo)
        assert status[p] == rc == 0, (model, analytic, p, status[p], rc)
        rel = float(np.max(np.abs(xg[p] - xo) / np.abs(xo)))
        worst = max(worst, rel)
        assert rel <= tol, (model, analytic, p, rel, tol)
    print(f"conv decays against oracle {model} analytic={analytic}: worst relative difference of x {worst:.3g} (allowed {tol:.3g})")
    wctx.close()


# ------------------------------------------------------------------------------------------------ 3. the composition
def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


def _by_hand(ds, inner, conv, dy, dw, dx0, m, analytic, o, loss=None, stat=None, pm=None, grp=None):
    """The one-call fit composed by hand from the launchers: the convolving pair around the model's (made without weights),
    then the loss or the Poisson pair (which then keeps the weights as its mask), then the map or the group; gather, solve,
    covariance (unscaled under the Poisson pair), expand."""
    nprob = dy.shape[0]
    stack = [ds.conv_launchers(conv, inner[0], inner[1], inner[2], dy, None if stat is not None else dw)]
    if loss is not None:
        stack.append(ds.loss_launchers(loss, *stack[-1], nprob=nprob))
    if stat is not None:
        stack.append(ds.pois_launchers(stat, stack[-1][0], stack[-1][1], stack[-1][2], dy, dw))
    M = m
    if pm is not None:
        stack.append(ds.pmap_launchers(pm, *stack[-1], dx0))
        xs = ds.pmap_gather(pm, dx0)
    elif grp is not None:
        stack.append(ds.group_launchers(grp, *stack[-1]))
        xs, M = ds.group_gather(grp, dx0), grp.nsets * m
    else:
        xs = dx0.clone()
    top = stack[-1]
    j = top[1] if analytic else None
    fvec, ibs, st = ds.lm_solve_batch_device(top[0], top[2], M, xs, jac=j, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(top[0], top[2], M, xs, jac=j, scaled=stat is None)
    x = xs
    if pm is not None:
        x = ds.pmap_expand(pm, xs, dx0)
        T = PM.tables(*pm_spec(pm))
        ce = [PM.cov_expand(T, c, s) for c, s in zip(cov.cpu().numpy(), sigma.cpu().numpy())]
        cov, sigma = _dev(ds, np.stack([c for c, s in ce])), _dev(ds, np.stack([s for c, s in ce]))
    elif grp is not None:
        x = ds.group_expand(grp, xs)
        sigma = ds.group_sigma(grp, sigma, _dev(ds, np.array(st, dtype=np.int32)))
    for s_ in reversed(stack):
        s_[2].close()
    return x, fvec.reshape(nprob, m), sigma, cov, chi2, rank, ibs, st


def pm_spec(pm):
    """(nfull, fixed, tied) of the one map the tests here use: the baseline of the decay fixed."""
    assert pm.nfull == 3 and pm.nfree == 2
    return 3, (2,), None


def _check(got, want, what):
    assert set(want[7]) == {0}, (what, want[7])
    assert got[7] == want[7] and got[6] == want[6], (what, got[6], want[6])
    for g, w_, name in zip(got[:6], want[:6], ("x", "fvec", "sigma", "cov", "chi2", "rank")):
        assert _eq(g, w_), (what, name)


def _deviance_chi2(ds, fvec, w, per, n):
    """chi2 of a Poisson fit: (sum of f_i^2, ascending) / (unmasked rows - n), per problem of `per` rows."""
    fh = fvec.cpu().numpy().reshape(-1, per)
    wm = np.ones_like(fh) if w is None else w.reshape(-1, per)
    q = []
    for p in range(len(fh)):
        s = 0.0
        for v in fh[p]:
            s = s + v * v
        q.append(s / float(int((wm[p] != 0).sum()) - n))
    return _dev(ds, np.array(q))


COMBOS = ["plain", "weights", "loss", "loss+map", "pois", "pois+mask", "pois+map", "map", "group", "group+loss", "group+pois"]


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("model", ["curve", "formula"])
def test_one_call_fit_is_the_composition(ds, model, analytic, combo):
    """curve_fit_batch / expr_fit_batch with conv= (nlh_curve_fit_batch_conv, nlh_expr_fit_batch_conv) = the launchers composed
    by hand, GPU against GPU and bit for bit: x, fvec, sigma, cov, chi2, rank, counts and status -- alone, with weights, with a
    loss, with the Poisson deviance (the mask stays with the Poisson pair: masked rows of fvec are +0.0), inside a map and
    inside a group."""
    nprob, m, G = 16, CV.M, 4
    t, y, xt, x0 = CV.family(nprob)
    parts = combo.split("+")
    rng = np.random.default_rng(3)
    w = None
    if "weights" in parts or "loss" in parts:
        w = 1.0 / np.sqrt(np.maximum(y, 1.0))
    if "mask" in parts:
        w = (rng.uniform(size=y.shape) < 0.9).astype(np.float64)
        w[:, :6] = 0.0                                                  # the bins before the pulse
    loss = nl.Loss("soft_l1", 3.0) if "loss" in parts else None
    stat = nl.Poisson() if "pois" in parts else None
    pm = nl.ParamMap(3, fixed=(2,)) if "map" in parts else None
    grp = nl.Group(3, shared=(1,), nsets=G) if "group" in parts else None
    start = x0.copy()
    if pm is not None:
        start[:, 2] = xt[:, 2]
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, start)
    dw = _dev(ds, w) if w is not None else None
    o = ds.options()
    conv = _irf()
    inner, e = _decay_inner(ds, model, dt, dy)
    if not analytic:
        inner = (inner[0], None, inner[2])
    kw = dict(weights=dw, analytic=analytic, opts=o, pmap=pm, loss=loss, stat=stat, group=grp, conv=conv)
    got = (ds.curve_fit_batch(CV.KIND, dt, dy, dx0, ncomp=CV.K, baseline=CV.B, **kw) if model == "curve"
           else ds.expr_fit_batch(e, dt, dy, dx0, **kw))
    want = list(_by_hand(ds, inner, conv, dy, dw, dx0, m, analytic, o, loss=loss, stat=stat, pm=pm, grp=grp))
    if stat is not None or w is not None:                              # chi2 with weights or a mask: the sequential sum over the dof
        n = 2 if pm is not None else grp.nouter if grp is not None else 3
        want[4] = _deviance_chi2(ds, want[1], w, (G if grp is not None else 1) * m, n)
    _check(got, want, (model, analytic, combo))
    if "mask" in parts:
        fg = got[1].cpu().numpy()
        assert not _bits(fg[w == 0.0]).any() and (fg[w != 0.0] != 0.0).all()


def test_alone_inside_a_batch_of_300_and_host_forms(ds):
    """300 problems reach the sub-batches (concurrent calls of the wrapping launchers on different streams): a problem alone
    equals the same problem inside the batch; the host-array twins give the same bits; and what the feature is for: the rate
    of the reconvolution fit is within three standard errors of the truth."""
    nprob, m = 300, CV.M
    t, y, xt, x0 = CV.decay_problems(CV.TRUTHS[0], nprob, start=CV.START)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    stat, conv = nl.Poisson(), _irf()
    big = None
    for analytic in (False, True):
        big = ds.curve_fit_batch(CV.KIND, dt, dy, dx0, ncomp=CV.K, baseline=CV.B, analytic=analytic, opts=o, stat=stat, conv=conv)
        for p in (0, 137, nprob - 1):
            one = ds.curve_fit_batch(CV.KIND, dt[p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dx0[p:p + 1].contiguous(), ncomp=CV.K,
                                     baseline=CV.B, analytic=analytic, opts=o, stat=stat, conv=conv)
            for g, w_ in zip(one[:6], big[:6]):
                assert _eq(g, w_[p:p + 1]), (analytic, p)
            assert one[6][0] == big[6][p]
    assert set(big[7]) == {0}
    kk = xt[:, 1]
    rel = (big[0].cpu().numpy()[:, 1] - kk) / kk
    bias, se = float(rel.mean()), float(rel.std(ddof=1) / np.sqrt(nprob))
    print(f"device reconvolution, Poisson deviance: k {100 * bias:+.2f} % +- {100 * se:.2f} %")
    assert abs(bias) <= 3 * se
    # per-problem kernels that are all the same kernel: the same bits
    per = ds.curve_fit_batch(CV.KIND, dt, dy, dx0, ncomp=CV.K, baseline=CV.B, analytic=True, opts=o, stat=stat,
                             conv=nl.Convolve(np.tile(CV.irf(), (nprob, 1)), origin=CV.ORIGIN, extend=CV.EXTEND))
    for g, w_ in zip(per[:6], big[:6]):
        assert _eq(g, w_)
    # the host forms
    k = CV.irf()
    cv = _lib.ConvStruct(len(k), CV.ORIGIN, CV.EXT[CV.EXTEND], 1, k.ctypes.data)
    xh, fh = x0.copy(), np.zeros((nprob, m))
    sh, ch, qh, rh = np.zeros((nprob, 3)), np.zeros((nprob, 3, 3)), np.zeros(nprob), np.zeros(nprob, dtype=np.int32)
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    dp = C.POINTER(C.c_double)
    rc = ds.lib.nlh_curve_fit_batch_conv_h(ds.h.ptr, C.byref(o), R.EXPDECAY, CV.K, CV.B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp),
                                           None, 1, None, None, None, None, C.byref(cv), 0, None, 0, 1, stat.mu_floor, xh.ctypes.data_as(dp),
                                           fh.ctypes.data_as(dp), sh.ctypes.data_as(dp), ch.ctypes.data_as(dp), qh.ctypes.data_as(dp),
                                           rh.ctypes.data_as(_lib.c_int32_p), ib, st)
    assert rc == 0
    for g, w_ in zip((xh, fh, sh, ch, qh), big[:5]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    assert np.array_equal(rh, big[5].cpu().numpy()) and [ib[p].as_dict() for p in range(nprob)] == big[6] and list(st) == big[7]
    e = nl.Expr(CV.FORMULA, ("t",), CV.PARAMS)
    w = 1.0 / np.sqrt(np.maximum(y, 1.0))
    bige = ds.expr_fit_batch(e, dt, dy, dx0, weights=_dev(ds, w), analytic=True, opts=o, conv=conv)
    xh2, fh2, sh2 = x0.copy(), np.zeros((nprob, m)), np.zeros((nprob, 3))
    rc = ds.lib.nlh_expr_fit_batch_conv_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                          1, None, None, None, None, C.byref(cv), 0, None, 0, 0, 0.0, xh2.ctypes.data_as(dp), fh2.ctypes.data_as(dp),
                                          sh2.ctypes.data_as(dp), None, None, None, None, None)
    assert rc == 0
    for g, w_ in zip((xh2, fh2, sh2), bige[:3]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    # the convolved model for plotting: curve_eval, then conv_apply -- fvec of an unweighted fit is that minus y
    plain = ds.curve_fit_batch(CV.KIND, dt, dy, dx0, ncomp=CV.K, baseline=CV.B, opts=o, covariance=False, conv=conv)
    shown = ds.conv_apply(conv, ds.curve_eval(CV.KIND, plain[0], dt, ncomp=CV.K, baseline=CV.B))
    diff = (shown - dy - plain[1]).abs().max().item()
    assert diff <= 8 * 2.0 ** -52 * max(float(y.max()), shown.max().item()), diff     # (mu = r + y re-rounds the model: a few ulp of the counts)


# ------------------------------------------------------------------------------------------------ 4. the model object
@pytest.mark.parametrize("analytic", [0, 1])
@pytest.mark.parametrize("weighted", [False, True])
def test_model_object(ds, analytic, weighted):
    """nlh_conv_model_create over a curve model made without weights, through _eval, _lm_solve, _lm_covariance = the launcher
    forms, with a kernel per problem."""
    nprob, m = 12, CV.M
    t, y, xt, x0 = CV.family(nprob)
    w = 1.0 / np.sqrt(np.maximum(y, 1.0)) if weighted else None
    k = np.tile(CV.irf(), (nprob, 1)) * (1.0 + 0.01 * np.arange(nprob))[:, None]
    dt, dy = _dev(ds, t), _dev(ds, y)
    dw = _dev(ds, w) if weighted else None
    fcn, jac, ctx = ds.curve_launchers(CV.KIND, CV.K, CV.B, dt, dy)
    wf, wj, wctx = ds.conv_launchers(nl.Convolve(k, origin=CV.ORIGIN, extend=CV.EXTEND), fcn, jac, ctx, dy, dw)
    j = wj if analytic else None
    o = ds.options()
    dp = C.POINTER(C.c_double)
    inner, md = C.c_void_p(), C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.EXPDECAY, CV.K, CV.B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, analytic,
                                         C.byref(inner)) == 0
    cv = _lib.ConvStruct(k.shape[1], CV.ORIGIN, CV.EXT[CV.EXTEND], 0, k.ctypes.data)
    assert ds.lib.nlh_conv_model_create(ds.h.ptr, inner, C.byref(cv), y.ctypes.data_as(dp), w.ctypes.data_as(dp) if weighted else None,
                                        C.byref(md)) == 0
    try:
        sp, sm, sn = C.c_int32(), C.c_int32(), C.c_int32()
        ds.lib.nlh_dq_model_shape(md, C.byref(sp), C.byref(sm), C.byref(sn))
        assert (sp.value, sm.value, sn.value) == (nprob, m, 3)
        f0 = np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_eval(ds.h.ptr, md, x0.ctypes.data_as(dp), f0.ctypes.data_as(dp)) == 0
        assert np.array_equal(_bits(f0), _bits(_launch(ds, wf, wctx, list(range(nprob)), x0, m)))
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        xh, fh = x0.copy(), np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_lm_solve(ds.h.ptr, C.byref(o), md, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, x0)
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=j, opts=o)
        assert np.array_equal(_bits(xh), _bits(x.cpu().numpy())) and np.array_equal(_bits(fh), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(nprob)] == ibs and list(st) == status and set(status) == {0}
        ch, sh, rh, qh = np.zeros((nprob, 3, 3)), np.zeros((nprob, 3)), np.zeros(nprob, dtype=np.int32), np.zeros(nprob)
        assert ds.lib.nlh_dq_model_lm_covariance(ds.h.ptr, md, xh.ctypes.data_as(dp), 1, 0.0, ch.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                                 rh.ctypes.data_as(_lib.c_int32_p), qh.ctypes.data_as(dp)) == 0
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=j, scaled=True)
        assert np.array_equal(_bits(ch), _bits(cov.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sigma.cpu().numpy()))
        assert np.array_equal(rh, rank.cpu().numpy()) and np.array_equal(_bits(qh), _bits(chi2.cpu().numpy()))
        # refusals: a bad transform, a tap or a y that is not finite, a dense-quadratic inner model
        out = C.c_void_p(7)
        bad = _lib.ConvStruct(k.shape[1], k.shape[1], 0, 0, k.ctypes.data)
        assert ds.lib.nlh_conv_model_create(ds.h.ptr, inner, C.byref(bad), y.ctypes.data_as(dp), None, C.byref(out)) == NL_INVALID_INPUT_ERROR and not out.value
        assert ds.lib.nlh_conv_model_create(None, inner, C.byref(cv), y.ctypes.data_as(dp), None, C.byref(out)) == NLH_ERR_BAD_HANDLE
        kb, yb = k.copy(), y.copy()
        kb[3, 2], yb[2, 5] = np.inf, np.nan
        badk = _lib.ConvStruct(k.shape[1], 0, 0, 0, kb.ctypes.data)
        assert ds.lib.nlh_conv_model_create(ds.h.ptr, inner, C.byref(badk), y.ctypes.data_as(dp), None, C.byref(out)) == NL_INVALID_INPUT_ERROR
        assert ds.lib.nlh_conv_model_create(ds.h.ptr, inner, C.byref(cv), yb.ctypes.data_as(dp), None, C.byref(out)) == NL_INVALID_INPUT_ERROR
        assert ds.lib.nlh_conv_model_create(ds.h.ptr, None, C.byref(cv), y.ctypes.data_as(dp), None, C.byref(out)) == NL_INVALID_INPUT_ERROR
    finally:
        ds.lib.nlh_dq_model_destroy(md)
        ds.lib.nlh_dq_model_destroy(inner)
        wctx.close()


@pytest.fixture(scope="module")
def fortran_conv_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_conv")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "conv_fit")


def test_fortran_conv_fit(ds, fortran_conv_exe, tmp_path):
    """The Fortran user program (create_curve -> create_convolved -> create_poisson -> solve_batch -> covariance_batch with
    scaled = .false.: one masked batch of decays behind the response) prints the x, sigma and counts of the Python path, digit
    for digit (ES24.16)."""
    nprob, m = 6, CV.M
    t, y, xt, x0 = CV.family(nprob)
    w = np.ones((nprob, m))
    w[:, :6] = 0.0
    w[2, 100:] = 0.0
    k = CV.irf()
    path = str(tmp_path / "decays.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m, len(k), CV.ORIGIN, CV.EXT[CV.EXTEND]], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(w.tobytes()); fh.write(k.tobytes()); fh.write(x0.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_conv_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    o = ds.options(max_evals=500)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    fcn, jac, ctx = ds.curve_launchers(CV.KIND, CV.K, CV.B, dt, dy)
    cf, cj, cctx = ds.conv_launchers(_irf(), fcn, jac, ctx, dy)
    wf, wj, wctx = ds.pois_launchers(nl.Poisson(), cf, cj, cctx, dy, dw)
    x = _dev(ds, x0)
    fvec, ibs, st = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=wj, scaled=False)
    xh, sh = x.cpu().numpy(), sigma.cpu().numpy()
    want = []
    for p in range(nprob):
        want.append("x %d" % (p + 1) + "".join("%24.16E" % v for v in xh[p]))
        want.append("sigma %d" % (p + 1) + "".join("%24.16E" % v for v in sh[p]))
        want.append("counts %d %d %d %d %d" % (p + 1, ibs[p]["iter_count"], ibs[p]["fcn_count"], ibs[p]["jacobian_count"], int(rank[p])))
    lines = [" ".join(ln.split()) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1] == "done"
    assert lines[:-1] == [" ".join(w_.split()) for w_ in want], out.stdout
    wctx.close()
    cctx.close()


# ------------------------------------------------------------------------------------------------ 5. error returns
def test_error_returns(ds):
    """In the documented order; nothing is written where a call is refused."""
    m, nprob = 6, 2
    t, y, xt, x0 = CC.curve_problems("lorentz", 2, 0, m, nprob=nprob)          # N = 7 > m = 6
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    pm = nl.ParamMap(7, fixed=(6,), tied={5: (2, 1.25, 0.0)})           # nfree 5
    pm4 = nl.ParamMap(4)
    g2 = nl.Group(7, shared=(1, 2, 4, 5), nsets=2)                      # n = 4 + 2 * 3 = 10 < M = 12
    g3 = nl.Group(7, shared=(1, 4), nsets=3)                            # nprob = 2 is no multiple of 3
    f = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)
    sg = torch.full((nprob, 7), 7.0, dtype=torch.float64, device=ds.device)
    dk = _dev(ds, np.array([0.25, 0.5, 0.25]))
    good = _lib.ConvStruct(3, 1, 1, 1, dk.data_ptr())
    ptr = lambda a: a.ptr if a is not None else None

    def fit(kd=1, mm=m, p=pm, g=None, cv=good, loss=0, stat=0, floor=0.0, x=dx, h=ds.h.ptr, sigma=None, np_=nprob):
        return ds.lib.nlh_curve_fit_batch_conv(h, C.byref(o), kd, 2, 0, np_, mm, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None, ptr(g), ptr(p),
                                               C.byref(cv) if cv is not None else None, loss, None, 1, stat, floor,
                                               x.data_ptr() if x is not None else None, f.data_ptr(),
                                               sigma.data_ptr() if sigma is not None else None, None, None, None, None, None)
    bad_cvs = [None, _lib.ConvStruct(3, 1, 1, 1, None), _lib.ConvStruct(0, 0, 0, 1, dk.data_ptr()), _lib.ConvStruct(LMAX + 1, 0, 0, 1, dk.data_ptr()),
               _lib.ConvStruct(3, 3, 0, 1, dk.data_ptr()), _lib.ConvStruct(3, -1, 0, 1, dk.data_ptr()), _lib.ConvStruct(3, 1, 2, 1, dk.data_ptr()),
               _lib.ConvStruct(3, 1, -1, 1, dk.data_ptr())]
    assert fit(h=None, cv=None) == NLH_ERR_BAD_HANDLE                    # NLH_ERR_BAD_HANDLE first
    assert fit(kd=7, cv=None) == NL_INVALID_INPUT_ERROR                  # the model
    assert fit(p=pm4) == NL_INVALID_INPUT_ERROR                          # a map of another model
    assert fit(p=pm, g=g2) == NL_INVALID_INPUT_ERROR                     # a map and a group together
    assert fit(p=None, g=g3) == NL_INVALID_INPUT_ERROR                   # nprob no multiple of G
    assert fit(mm=4, cv=None) == NL_UNDERDEFINED_PROBLEM_ERROR           # m < nfree, before the transform is looked at
    assert fit(p=None, cv=None) == NL_UNDERDEFINED_PROBLEM_ERROR         # m < N without a map
    assert fit(loss=4, cv=None) == NL_INVALID_INPUT_ERROR and fit(stat=2, cv=None) == NL_INVALID_INPUT_ERROR
    assert fit(loss=1, stat=1, floor=1e-6) == NL_INVALID_INPUT_ERROR     # Poisson with a loss
    assert fit(x=None) == NL_INVALID_INPUT_ERROR
    assert fit(p=nl.ParamMap(7, fixed=(6,)), sigma=sg) == NL_INVALID_INPUT_ERROR    # nfree 6 = m: no degree of freedom for errors
    assert fit(stat=1, floor=0.0) == NL_INVALID_INPUT_ERROR              # a bad floor
    for bad in bad_cvs:                                                  # then the transform
        assert fit(cv=bad) == NL_INVALID_INPUT_ERROR
        assert fit(p=None, g=g2, cv=bad) == NL_INVALID_INPUT_ERROR
    assert fit(cv=None, np_=0) == 0                                      # (no problems: nothing further is looked at)
    torch.cuda.synchronize()
    assert (f == 7.0).all() and torch.equal(dx, _dev(ds, x0))
    assert fit() == 0 and fit(p=None, g=g2) == 0
    # the formula entry point takes the same ladder
    e = nl.Expr("a1/(1+((t-m1)/w1)^2) + a2/(1+((t-m2)/w2)^2) + c", ("t",), ("a1", "m1", "w1", "a2", "m2", "w2", "c"))

    def efit(mm=m, p=pm, g=None, cv=good, h=ds.h.ptr):
        return ds.lib.nlh_expr_fit_batch_conv(h, C.byref(o), e.ptr, nprob, mm, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None, ptr(g), ptr(p),
                                              C.byref(cv) if cv is not None else None, 0, None, 1, 0, 0.0, dx.data_ptr(), f.data_ptr(), None, None,
                                              None, None, None, None)
    assert efit(h=None) == NLH_ERR_BAD_HANDLE and efit(p=pm4) == NL_INVALID_INPUT_ERROR and efit(g=g2) == NL_INVALID_INPUT_ERROR
    assert efit(mm=4, cv=None) == NL_UNDERDEFINED_PROBLEM_ERROR
    for bad in bad_cvs:
        assert efit(cv=bad) == NL_INVALID_INPUT_ERROR
    assert efit() == 0
    # host taps and data are checked: every tap finite, y finite on EVERY row, whatever its weight
    dp = C.POINTER(C.c_double)
    xh, fh = x0.copy(), np.zeros((nprob, m))
    kh = np.array([0.25, 0.5, 0.25])
    zw = np.ones((nprob, m))
    zw[1, 2] = 0.0

    def fit_h(yy, kk, ww=None, expr=False):
        cvh = _lib.ConvStruct(3, 1, 1, 1, kk.ctypes.data)
        wp = ww.ctypes.data_as(dp) if ww is not None else None
        if expr:
            return ds.lib.nlh_expr_fit_batch_conv_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, yy.ctypes.data_as(dp), wp, 1, None,
                                                    None, None, pm.ptr, C.byref(cvh), 0, None, 1, 0, 0.0, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp),
                                                    None, None, None, None, None, None)
        return ds.lib.nlh_curve_fit_batch_conv_h(ds.h.ptr, C.byref(o), 1, 2, 0, nprob, m, t.ctypes.data_as(dp), 0, yy.ctypes.data_as(dp), wp, 1, None,
                                                 None, None, pm.ptr, C.byref(cvh), 0, None, 1, 0, 0.0, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp),
                                                 None, None, None, None, None, None)
    for expr in (False, True):
        for bad in (np.nan, np.inf, -np.inf):
            yb, kb = y.copy(), kh.copy()
            yb[1, 2], kb[2] = bad, bad
            assert fit_h(yb, kh, expr=expr) == NL_INVALID_INPUT_ERROR
            assert fit_h(yb, kh, zw, expr=expr) == NL_INVALID_INPUT_ERROR      # a zero-weight row is convolved too
            assert fit_h(y, kb, expr=expr) == NL_INVALID_INPUT_ERROR
    assert np.array_equal(xh, x0) and (fh == 0.0).all()
    assert fit_h(y, kh) == 0 and (fh != 0.0).all()
    # the wrap and the launchers' own refusals, and an inner refusal handed back as it is with nothing written
    fcn, jac, ctx = ds.curve_launchers("lorentz", 2, 0, dt, dy)
    out = C.c_void_p(7)
    none = C.cast(None, _lib.DEVFCN)
    wrap = lambda h, cv, yy, ff: ds.lib.nlh_conv_wrap(h, C.byref(cv) if cv is not None else None, yy, None, ff, jac, ds._ctxp(ctx), C.byref(out))
    assert wrap(None, good, dy.data_ptr(), fcn) == NLH_ERR_BAD_HANDLE and not out.value
    assert wrap(ds.h.ptr, good, None, fcn) == NL_INVALID_INPUT_ERROR and not out.value
    for bad in bad_cvs:
        assert wrap(ds.h.ptr, bad, dy.data_ptr(), fcn) == NL_INVALID_INPUT_ERROR and not out.value
    assert wrap(ds.h.ptr, good, dy.data_ptr(), none) == NL_UNDEFINED_FUNCTION_ERROR and not out.value
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    J = torch.full((nprob, 7, m), 7.0, dtype=torch.float64, device=ds.device)
    lst = _dev(ds, [0, 1], np.int32)
    wf, wj, wctx = ds.conv_launchers(nl.Convolve(kh, origin=1, extend="hold"), fcn, None, ctx, dy)
    assert wj is None
    args = lambda n_, m_: (wctx.ptr, stream, nprob, lst.data_ptr(), n_, dx.data_ptr(), m_, J.data_ptr())
    assert ds.lib.nlh_conv_device_fcn(*args(0, m)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_conv_device_fcn(*args(7, 0)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_conv_device_jac(*args(7, m)) == NL_UNDEFINED_FUNCTION_ERROR   # no inner Jacobian launcher
    assert ds.lib.nlh_conv_device_fcn(*args(7, m + 1)) == NL_INVALID_INPUT_ERROR    # the inner launcher's refusal (m != ctx.m)
    torch.cuda.synchronize()
    assert (J == 7.0).all()
    wctx.close()
    with pytest.raises(ValueError):
        ds.curve_fit_batch("lorentz", dt, dy, dx, ncomp=2, baseline=0, pmap=pm, group=g2, conv=nl.Convolve(kh, origin=1))
    with pytest.raises(ValueError):
        ds.curve_fit_batch("lorentz", dt, dy, dx, ncomp=2, baseline=0, conv=nl.Convolve(np.ones((3, 3))))     # kernels for 3 problems, 2 data sets
