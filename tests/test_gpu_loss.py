"""GPU tests of the robust losses (include/nonlin_hip.h: nlh_loss_*), bit for bit unless said: the kernels through the
wrapping launchers against the numpy restatement (tests/loss_restatement.py) for every launch shape, form, column split
and slicing; Huber with a scale nothing reaches against the unwrapped launcher and solve; the LINEAR entry points against
the _pmap ones; zero-weight rows; LM and bounded solves through the wrappers against the CPU oracle, alone and inside a
parameter map; a problem alone against the same problem inside a batch of 300; the one-call fits as the composition they
stand for; the model object; the Fortran program; the error returns; Cauchy within the bound built from the measured error
of the device library's log1p."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import curve_restatement as R
import expr_restatement as XR
import loss_cases as LC
import loss_restatement as LR
import pmap_restatement as PR
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
FORMS = [None, "row", "flat"]               # None: the form m selects; a forced form that cannot hold m falls back to it
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR = 201, 211, 212
FORMULA = "a/(1+((t-mu)/w)^2) + c"          # the Lorentzian on a constant, exp-free: the curve model's operations in its order
PARAMS = ("a", "mu", "w", "c")
KIND, K, B = LC.KIND, LC.K, LC.B
# the map of the mapped tests over (a, mu, w, c): the baseline fixed, the amplitude tied to the width (a = 3.3 w + 0.05, about
# what the family's truth has): free unknowns mu, w, and the free column of w carries a tie
MAP_FIXED, MAP_TIED = (3,), {0: (2, 3.3, 0.05)}


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


class _env:
    """Environment variables for the calls inside (the library reads NLH_LOSS_* at every call); None: unset."""

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


def _inner(ds, n, m, nprob, seed, weights=None):
    """An inner launcher pair of n parameters on m rows: the formula a*t (n = 1) or a Lorentzian model (n = 3, 4, 5, 9).
    Returns (launchers, x0 [nprob, n], keep-alive)."""
    rng = np.random.default_rng(seed)
    if n == 1:
        e = nl.Expr("a*t", ("t",), ("a",))
        t = np.tile(np.linspace(-1.0, 1.0, m) if m > 1 else np.array([0.7]), (nprob, 1)) + rng.uniform(-0.1, 0.1, (nprob, m)) / m
        xt = rng.uniform(0.5, 1.5, (nprob, 1))
        y = xt * t + 0.02 * rng.standard_normal((nprob, m))
        x0 = xt * (1.0 + 0.1 * rng.uniform(-1, 1, (nprob, 1)))
        dt, dy = _dev(ds, t), _dev(ds, y)
        dw = _dev(ds, weights) if weights is not None else None
        return ds.expr_launchers(e, dt, dy, dw), x0, (e, dt, dy, dw)
    KK, BB = {3: (1, -1), 4: (1, 0), 5: (1, 1), 9: (2, 2)}[n]
    import curve_cases as CC
    t, y, xt, x0 = CC.curve_problems("lorentz", KK, BB, m, nprob=nprob, seed=seed, sigma=0.02)
    dt, dy = _dev(ds, t), _dev(ds, y)
    dw = _dev(ds, weights) if weights is not None else None
    return ds.curve_launchers("lorentz", KK, BB, dt, dy, dw), x0, (dt, dy, dw)


def _scales(rawF, nprob):
    """Per-problem scales that put residuals on both sides: half or twice the median |r| of the problem's first point."""
    c = np.empty(nprob)
    for p in range(nprob):
        med = float(np.median(np.abs(rawF[p])))
        c[p] = (med if med > 0 else 1.0) * (0.5 if p % 2 == 0 else 2.0)
    return c


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("m", [1, 64, 128, 129, 256, 257, 301])
def test_launchers_bitwise(ds, m, n):
    """k_loss_fcn and k_loss_jac through the wrapping launchers: F = out(inner F) and J = g * inner J of the restatement,
    applied to what the inner launchers give for the same points -- Huber, soft-L1 and LINEAR, per-problem and shared scale,
    with and without dprob, a point list with repeated problems, both forms, the column split forced, sliced and unsliced."""
    nprob = 5
    (fcn, jac, ctx), x0, keep = _inner(ds, n, m, nprob, seed=100 * n + m)
    rawF0 = _launch(ds, fcn, ctx, list(range(nprob)), x0, m)
    cper = _scales(rawF0, nprob)
    shapes = [None, list(np.random.default_rng(3).integers(0, nprob, 23)) + [0, 0, nprob - 1], [nprob - 2]]
    seen_inside = seen_outside = False
    for k, plist in enumerate(shapes):
        rows = list(range(nprob)) if plist is None else [int(p) for p in plist]
        X = x0[rows] * (1.0 + 0.02 * np.random.default_rng(k).uniform(-1, 1, (len(rows), n)))
        rawF = _launch(ds, fcn, ctx, rows, X, m)
        rawJ = _launch(ds, jac, ctx, rows, X, m, jac=True)
        for kind in ("huber", "soft_l1", "linear"):
            for shared in (False, True):
                loss = nl.Loss(kind, float(cper[1]) if shared else cper)
                wf, wj, wctx = ds.loss_launchers(loss, fcn, jac, ctx)
                cq = [float(cper[1]) if shared else cper[p] for p in rows]
                want = [LR.apply(LR.KINDS[kind], cq[q], rawF[q]) for q in range(len(rows))]
                if kind == "huber":
                    a = np.abs(np.concatenate([rawF[q] / cq[q] for q in range(len(rows))]))
                    seen_inside |= bool((a <= 1.0).any())
                    seen_outside |= bool((a > 1.0).any())
                # (split: column groups; scratch: a cap that cuts a call into slices of two points)
                for form in FORMS:
                    for split, sliced in ((None, False), (2, False), (n, True), (None, True)):
                        with _env(NLH_LOSS_FORM=form, NLH_LOSS_SPLIT=split, NLH_LOSS_SCRATCH=8 if sliced else None):
                            F = _launch(ds, wf, wctx, plist, X, m)      # (without dprob: its problem list comes in slices of two)
                        with _env(NLH_LOSS_FORM=form, NLH_LOSS_SPLIT=split, NLH_LOSS_SCRATCH=2 * (8 * m + 4) if sliced else None):
                            J = _launch(ds, wj, wctx, plist, X, m, jac=True)
                        for q in range(len(rows)):
                            what = (kind, shared, k, q, form, split, sliced)
                            assert np.array_equal(_bits(F[q]), _bits(want[q][0])), what
                            assert np.array_equal(_bits(J[q]), _bits(want[q][1][None, :] * rawJ[q])), what
                wctx.close()
    assert (seen_inside and seen_outside) or m == 1


def test_apply_batch_bitwise(ds):
    """nlh_loss_apply_batch: out, g and wgt of the table for Huber, soft-L1 and LINEAR, per-problem and shared scale; a scale
    that is not finite or not positive makes that problem NaN, it alone; any output may be NULL; out may be r itself."""
    rng = np.random.default_rng(5)
    nprob, m = 7, 301
    c = np.exp(rng.uniform(-3, 3, nprob))
    r = c[:, None] * np.concatenate([rng.uniform(-1, 1, (nprob, 150)), rng.uniform(-40, 40, (nprob, 150)), np.zeros((nprob, 1))], axis=1)
    r[:, 7] = c
    r[:, 8] = -c
    r[:, 9] = -0.0
    dr = _dev(ds, r)
    for kind in ("huber", "soft_l1", "linear"):
        for scale in (c, 0.37):
            got = [v.cpu().numpy() for v in ds.loss_apply(nl.Loss(kind, scale), dr)]
            want = LR.apply(LR.KINDS[kind], c[:, None] if scale is c else scale, r)
            for g_, w_ in zip(got, want):
                assert np.array_equal(_bits(g_), _bits(w_)), kind
    bad = c.copy()
    bad[[1, 3, 4, 6]] = [0.0, -1.0, np.inf, np.nan]
    dbad = _dev(ds, bad)
    out, wgt = torch.full_like(dr, 7.0), torch.full_like(dr, 7.0)
    assert ds.lib.nlh_loss_apply_batch(ds.h.ptr, LR.SOFT_L1, nprob, m, dbad.data_ptr(), 0, dr.data_ptr(), out.data_ptr(), None, wgt.data_ptr()) == 0
    torch.cuda.synchronize()
    wo, wg, ww = LR.apply(LR.SOFT_L1, bad[:, None], r)
    oh, wh = out.cpu().numpy(), wgt.cpu().numpy()
    for p in range(nprob):
        if p in (1, 3, 4, 6):
            assert np.isnan(oh[p]).all() and np.isnan(wh[p]).all()
        else:
            assert np.array_equal(_bits(oh[p]), _bits(wo[p])) and np.array_equal(_bits(wh[p]), _bits(ww[p]))
    inplace = dr.clone()
    dc = _dev(ds, c)
    assert ds.lib.nlh_loss_apply_batch(ds.h.ptr, LR.HUBER, nprob, m, dc.data_ptr(), 0, inplace.data_ptr(), inplace.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(inplace.cpu().numpy()), _bits(LR.residual(LR.HUBER, c[:, None], r)))


# ------------------------------------------------------------------------------------------------ 2. the plain fit inside
@pytest.mark.parametrize("analytic", [False, True])
def test_huber_with_a_scale_nothing_reaches_is_the_unwrapped_call(ds, analytic):
    m, nout, nprob = 64, 4, 16
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob)
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, dy)
    wf, wj, wctx = ds.loss_launchers(nl.Loss("huber", 1e300), fcn, jac, ctx)
    rows = list(range(nprob))
    assert np.array_equal(_bits(_launch(ds, wf, wctx, rows, x0, m)), _bits(_launch(ds, fcn, ctx, rows, x0, m)))
    assert np.array_equal(_bits(_launch(ds, wj, wctx, rows, x0, m, jac=True)), _bits(_launch(ds, jac, ctx, rows, x0, m, jac=True)))
    o = ds.options()
    xa, xb = _dev(ds, x0), _dev(ds, x0)
    fa, iba, sta = ds.lm_solve_batch_device(fcn, ctx, m, xa, jac=jac if analytic else None, opts=o)
    fb, ibb, stb = ds.lm_solve_batch_device(wf, wctx, m, xb, jac=wj if analytic else None, opts=o)
    assert _eq(xa, xb) and _eq(fa, fb) and iba == ibb and sta == stb
    wctx.close()


def test_linear_loss_entry_points_are_the_pmap_ones(ds):
    m, nout, nprob = 64, 4, 12
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    lin = nl.Loss("linear")
    for pm in (None, nl.ParamMap(4, fixed=MAP_FIXED, tied=MAP_TIED)):
        for old, new in ((ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, opts=o, pmap=pm),
                          ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, opts=o, pmap=pm, loss=lin)),
                         (ds.expr_fit_batch(e, dt, dy, dx0, opts=o, pmap=pm), ds.expr_fit_batch(e, dt, dy, dx0, opts=o, pmap=pm, loss=lin))):
            for g, w_ in zip(new[:6], old[:6]):
                assert _eq(g, w_)
            assert new[6] == old[6] and new[7] == old[7]
    # the host-array twins, scale NULL
    xh, fh = x0.copy(), np.zeros((nprob, m))
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    assert ds.lib.nlh_curve_fit_batch_loss_h(ds.h.ptr, C.byref(o), R.LORENTZ, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None,
                                             1, None, None, None, 0, None, 0, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), None, None, None,
                                             None, ib, st) == 0
    old = ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, opts=o, covariance=False)
    assert np.array_equal(_bits(xh), _bits(old[0].cpu().numpy())) and np.array_equal(_bits(fh), _bits(old[1].cpu().numpy()))
    xh2, fh2 = x0.copy(), np.zeros((nprob, m))
    assert ds.lib.nlh_expr_fit_batch_loss_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1, None,
                                            None, None, 0, None, 0, xh2.ctypes.data_as(dp), fh2.ctypes.data_as(dp), None, None, None, None,
                                            None, None) == 0
    olde = ds.expr_fit_batch(e, dt, dy, dx0, opts=o, covariance=False)
    assert np.array_equal(_bits(xh2), _bits(olde[0].cpu().numpy())) and np.array_equal(_bits(fh2), _bits(olde[1].cpu().numpy()))


@pytest.mark.parametrize("kind", ["huber", "soft_l1", "cauchy"])
def test_zero_weight_rows_stay_exactly_zero(ds, kind):
    m, n, nprob = 129, 4, 5
    rng = np.random.default_rng(2)
    w = rng.uniform(0.5, 2.0, (nprob, m))
    w[rng.uniform(size=(nprob, m)) < 0.3] = 0.0
    w[:, -1] = 0.0
    (fcn, jac, ctx), x0, keep = _inner(ds, n, m, nprob, seed=9, weights=w)
    rows = list(range(nprob))
    rawF = _launch(ds, fcn, ctx, rows, x0, m)
    rawJ = _launch(ds, jac, ctx, rows, x0, m, jac=True)
    wf, wj, wctx = ds.loss_launchers(nl.Loss(kind, _scales(rawF, nprob)), fcn, jac, ctx)
    for form in ("row", "flat"):
        with _env(NLH_LOSS_FORM=form):
            F = _launch(ds, wf, wctx, rows, x0, m)
            J = _launch(ds, wj, wctx, rows, x0, m, jac=True)
        z = w == 0.0
        assert z.any() and (rawF[z] == 0.0).all()
        assert np.array_equal(_bits(F[z]), _bits(rawF[z]))              # +-0 stays +-0
        for q in rows:
            assert np.array_equal(_bits(J[q][:, z[q]]), _bits(rawJ[q][:, z[q]]))   # g = 1.0 there: the inner rows (zeros) as they are
    wctx.close()


# ------------------------------------------------------------------------------------------------ 3. the oracle
def _raw(model, prog, x, t, y):
    return R.residual(R.LORENTZ, K, B, x, t, y) if model == "curve" else XR.residual(prog, x, t[None], y)


def _rawjac(model, prog, x, t):
    return R.jacobian(R.LORENTZ, K, B, x, t) if model == "curve" else XR.jacobian(prog, x, t[None])


def _callbacks(model, prog, k, c, t, y, analytic, T=None, full=None):
    ex = (lambda x: x) if T is None else (lambda x: PR.expand(T, x, full))
    con = (lambda J: J) if T is None else (lambda J: PR.contract(T, J))
    f = lambda x, out: out.__setitem__(slice(None), LR.residual(k, c, _raw(model, prog, ex(x), t, y)))
    j = (lambda x, J: J.__setitem__((slice(None), slice(None)),
                                    con(LR.jacobian(k, c, _raw(model, prog, ex(x), t, y), _rawjac(model, prog, ex(x), t))))) if analytic else None
    return f, j


def _problem_scales(nprob):
    return LC.SCALE * (1.0 + 0.5 * np.arange(nprob) / nprob)            # a scale per problem


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("kind", ["huber", "soft_l1"])
@pytest.mark.parametrize("model", ["curve", "formula"])
def test_solves_against_oracle(ds, oracle, model, kind, analytic, bounded):
    """lm_solve / cls_solve of the oracle with the restated transform as callbacks, under default options, every problem of
    the outlier family's first 24: status, x, fvec and every count identical; forward differences without bounds solve with
    status 0 (tests/test_loss_cpu.py holds the family to that on the reference path alone)."""
    m, nout, nprob = 64, 4, 24
    k = LR.KINDS[kind]
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob)
    c = _problem_scales(nprob)
    dt, dy = _dev(ds, t), _dev(ds, y)
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    prog = e.program()
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, dy) if model == "curve" else ds.expr_launchers(e, dt, dy)
    wf, wj, wctx = ds.loss_launchers(nl.Loss(kind, c), fcn, jac, ctx)
    lower = upper = None
    if bounded:
        lower, upper = xt.mean(0) - np.array([0.1, 0.2, 0.05, 0.01]), xt.mean(0) + np.array([0.1, 0.2, 0.05, 0.01])   # bounds that bind
        x0 = np.clip(x0, lower, upper)
    x = _dev(ds, x0)
    o = ds.options()
    if bounded:
        fvec, ibs, status = ds.cls_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=o, lower=lower, upper=upper)
    else:
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=o)
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options()
    for p in range(nprob):
        f, j = _callbacks(model, prog, k, c[p], t[p], y[p], analytic)
        if bounded:
            rc, xo, fo, ibo = oracle.cls_solve(f, m, 4, x0[p], jac=j, opts=oo, lower=lower, upper=upper)
        else:
            rc, xo, fo, ibo = oracle.lm_solve(f, m, 4, x0[p], jac=j, opts=oo)
        what = (model, kind, analytic, bounded, p)
        assert status[p] == rc, (what, status[p], rc)
        assert _same(ibs[p], ibo), (what, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), what
    if not bounded and not analytic:
        assert set(status) == {0}
    wctx.close()


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("kind", ["huber", "soft_l1"])
def test_solve_through_a_map_against_oracle(ds, oracle, kind, analytic):
    """The loss inside the map: the map's launchers around the loss's around the curve model's, the baseline fixed and the
    amplitude tied to the width (MAP_FIXED, MAP_TIED), so that the contraction sums two columns whose rows the loss has already
    scaled -- against the oracle on expand -> model -> loss -> contract.  Equality only: the tie is no property of the data."""
    m, nout, nprob = 64, 4, 16
    k = LR.KINDS[kind]
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob)
    c = _problem_scales(nprob)
    T = PR.tables(4, MAP_FIXED, MAP_TIED)
    pm = nl.ParamMap(4, fixed=MAP_FIXED, tied=MAP_TIED)
    assert pm.nfree == 2 and len(PR.ties_of(T, 1)) == 1
    full = x0.copy()
    full[:, 3] = xt[:, 3]
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, dy)
    lf, lj, lctx = ds.loss_launchers(nl.Loss(kind, c), fcn, jac, ctx)
    wf, wj, wctx = ds.pmap_launchers(pm, lf, lj, lctx, dfull)
    x = ds.pmap_gather(pm, dfull)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options())
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options()
    for p in range(nprob):
        f, j = _callbacks("curve", None, k, c[p], t[p], y[p], analytic, T, full[p])
        rc, xo, fo, ibo = oracle.lm_solve(f, m, 2, PR.gather(T, full[p]), jac=j, opts=oo)
        assert status[p] == rc and _same(ibs[p], ibo), (p, status[p], rc, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)) and np.array_equal(_bits(fg[p]), _bits(fo)), p
    wctx.close()
    lctx.close()


# ------------------------------------------------------------------------------------------------ 4. the composition
def _fit_by_hand(ds, loss, pm, launchers, dstart, m, analytic, o, lower=None, upper=None):
    """loss_launchers, then (with a map) pmap_launchers around them; gather, solve, covariance, expand, cov_expand."""
    fcn, jac, ctx = launchers
    lf, lj, lctx = ds.loss_launchers(loss, fcn, jac, ctx)
    if pm is not None:
        T = pm.tables()
        wf, wj, wctx = ds.pmap_launchers(pm, lf, lj, lctx, dstart)
        x = ds.pmap_gather(pm, dstart)
        f2f = T[4]
    else:
        wf, wj, wctx, x, f2f = lf, lj, lctx, dstart.clone(), slice(None)
    j = wj if analytic else None
    if lower is not None:
        fvec, ibs, st = ds.cls_solve_batch_device(wf, wctx, m, x, jac=j, opts=o, lower=lower[f2f], upper=upper[f2f])
    else:
        fvec, ibs, st = ds.lm_solve_batch_device(wf, wctx, m, x, jac=j, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=j, scaled=True)
    cov, sigma = cov.cpu().numpy(), sigma.cpu().numpy()
    if pm is not None:
        x = ds.pmap_expand(pm, x, dstart)
        full = [PR.cov_expand(T, cov[p], sigma[p]) for p in range(len(st))]
        cov, sigma = np.stack([v[0] for v in full]), np.stack([v[1] for v in full])
        wctx.close()
    lctx.close()
    return x, fvec, sigma, cov, chi2, rank, ibs, st


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("model", ["curve", "formula"])
def test_one_call_fit_is_the_composition(ds, model, mapped, analytic, bounded):
    """nlh_curve_fit_batch_loss / nlh_expr_fit_batch_loss = the launchers composed by hand, the loss inside the map: x, fvec
    (the transformed residual), sigma, cov, chi2 (sum fvec^2 / dof), rank, counts and status."""
    m, nout, nprob = 64, 4, 16
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob)
    loss = nl.Loss("soft_l1" if analytic else "huber", _problem_scales(nprob))
    pm = nl.ParamMap(4, fixed=MAP_FIXED, tied=MAP_TIED) if mapped else None
    start = x0.copy()
    if mapped:
        start[:, 3] = xt[:, 3]
        start[:, 0] = 1e300                                             # tied positions are ignored on entry
    lower = upper = None
    if bounded:
        lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
    dt, dy, dstart = _dev(ds, t), _dev(ds, y), _dev(ds, start)
    o = ds.options()
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    if model == "curve":
        got = ds.curve_fit_batch(KIND, dt, dy, dstart, ncomp=K, baseline=B, lower=lower, upper=upper, analytic=analytic, opts=o, pmap=pm, loss=loss)
        launchers = ds.curve_launchers(KIND, K, B, dt, dy)
    else:
        got = ds.expr_fit_batch(e, dt, dy, dstart, lower=lower, upper=upper, analytic=analytic, opts=o, pmap=pm, loss=loss)
        launchers = ds.expr_launchers(e, dt, dy)
    want = _fit_by_hand(ds, loss, pm, launchers, dstart, m, analytic, o, lower, upper)
    assert _eq(got[0], want[0]) and _eq(got[1], want[1]) and got[6] == want[6] and got[7] == want[7]
    assert bounded or mapped or set(got[7]) == {0}
    sg, cg, qg, rg = (v.cpu().numpy() for v in got[2:6])
    fh = got[1].cpu().numpy()
    nfree = 2 if mapped else 4
    for p, st in enumerate(got[7]):
        if st != 0:
            assert np.isnan(sg[p]).all() and np.isnan(cg[p]).all() and np.isnan(qg[p]) and rg[p] == -1
            continue
        assert np.array_equal(_bits(sg[p]), _bits(want[2][p])) and np.array_equal(_bits(cg[p]), _bits(want[3][p])), p
        assert _bits(qg[p]) == _bits(want[4][p].cpu().numpy()) and rg[p] == int(want[5][p]) == nfree
        s = 0.0
        for v in fh[p]:
            s = s + v * v
        assert _bits(qg[p]) == _bits(s / float(m - nfree)), p             # chi2 is that of the transformed residual


def test_alone_and_inside_a_batch_of_300(ds):
    """300 problems reach the sub-batches (concurrent calls of the wrapping launchers on different streams); the host-array
    twin gives the same bits."""
    m, nout, nprob = 64, 4, 300
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob, seed=77)
    c = _problem_scales(nprob)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    big = None
    for analytic in (True, False):
        for form in (None, "row"):
            with _env(NLH_LOSS_FORM=form):
                big = ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, analytic=analytic, opts=o, loss=nl.Loss("huber", c))
                for p in (0, 137, nprob - 1):
                    one = ds.curve_fit_batch(KIND, dt[p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dx0[p:p + 1].contiguous(), ncomp=K,
                                             baseline=B, analytic=analytic, opts=o, loss=nl.Loss("huber", [c[p]]))
                    for g, w_ in zip(one[:6], big[:6]):
                        assert _eq(g, w_[p:p + 1]), (analytic, form, p)
                    assert one[6][0] == big[6][p]
    assert set(big[7]) == {0}
    xh, fh = x0.copy(), np.zeros((nprob, m))
    sh, ch, qh, rh = np.zeros((nprob, 4)), np.zeros((nprob, 4, 4)), np.zeros(nprob), np.zeros(nprob, dtype=np.int32)
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    rc = ds.lib.nlh_curve_fit_batch_loss_h(ds.h.ptr, C.byref(o), R.LORENTZ, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 0,
                                           None, None, None, LR.HUBER, c.ctypes.data_as(dp), 0, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp),
                                           sh.ctypes.data_as(dp), ch.ctypes.data_as(dp), qh.ctypes.data_as(dp),
                                           rh.ctypes.data_as(_lib.c_int32_p), ib, st)
    assert rc == 0
    for g, w_ in zip((xh, fh, sh, ch, qh), big[:5]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    assert np.array_equal(rh, big[5].cpu().numpy()) and [ib[p].as_dict() for p in range(nprob)] == big[6]
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    xh2, fh2 = x0.copy(), np.zeros((nprob, m))
    rc = ds.lib.nlh_expr_fit_batch_loss_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 0, None, None,
                                          None, LR.HUBER, c.ctypes.data_as(dp), 0, xh2.ctypes.data_as(dp), fh2.ctypes.data_as(dp), None, None,
                                          None, None, None, None)
    assert rc == 0                                                      # (the formula's residual bits are the curve model's)
    assert np.array_equal(_bits(xh2), _bits(xh)) and np.array_equal(_bits(fh2), _bits(fh))


def test_robust_fit_recovers_what_the_plain_fit_loses(ds):
    """What the feature is for, on the device: on the outlier family every robust one-call fit ends closer to the truth than
    the plain one, problem by problem (the condition tests/test_loss_cpu.py holds the reference path to), and the weights of
    loss_apply on the raw residuals flag the planted outliers."""
    m, nout = LC.FAMILIES[0]
    t, y, xt, x0 = LC.outlier_problems(m, nout)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    plain = ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, analytic=False, opts=o, covariance=False)
    perr = np.abs(plain[0].cpu().numpy() - xt).max(1)
    for kind in LR.ROBUST:
        got = ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, analytic=False, opts=o, covariance=False, loss=nl.Loss(kind, LC.SCALE))
        assert set(got[7]) == {0}
        err = np.abs(got[0].cpu().numpy() - xt).max(1)
        assert (err < perr).all(), (kind, float(err.max()), float(perr.max()))
    raw = ds.curve_eval(KIND, got[0], dt, ncomp=K, baseline=B) - dy
    wgt = ds.loss_apply(nl.Loss("cauchy", LC.SCALE), raw.contiguous())[2].cpu().numpy()
    clean = np.stack([R.model(R.LORENTZ, K, B, xt[p], t[p]) for p in range(len(xt))])
    planted = (y - clean) > 0.4                                         # the spikes are 0.5 .. 1.5 on a noise of sigma 0.02
    assert planted.sum() == nout * len(xt) and (wgt[planted] < 0.05).all() and np.median(wgt[~planted]) > 0.5


# ------------------------------------------------------------------------------------------------ 5. the model object
@pytest.mark.parametrize("analytic", [0, 1])
@pytest.mark.parametrize("shared", [False, True])
def test_model_object(ds, analytic, shared):
    """nlh_loss_model_create over a curve model, through _eval, _lm_solve, _lm_covariance = the launcher forms."""
    m, nout, nprob = 64, 4, 12
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob)
    c = np.array([LC.SCALE]) if shared else _problem_scales(nprob)
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, dy)
    wf, wj, wctx = ds.loss_launchers(nl.Loss("soft_l1", float(c[0]) if shared else c), fcn, jac, ctx)
    j = wj if analytic else None
    o = ds.options()
    inner, md = C.c_void_p(), C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.LORENTZ, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, analytic,
                                         C.byref(inner)) == 0
    assert ds.lib.nlh_loss_model_create(ds.h.ptr, inner, LR.SOFT_L1, c.ctypes.data_as(dp), int(shared), C.byref(md)) == 0
    try:
        sp, sm, sn = C.c_int32(), C.c_int32(), C.c_int32()
        ds.lib.nlh_dq_model_shape(md, C.byref(sp), C.byref(sm), C.byref(sn))
        assert (sp.value, sm.value, sn.value) == (nprob, m, 4)
        f0 = np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_eval(ds.h.ptr, md, x0.ctypes.data_as(dp), f0.ctypes.data_as(dp)) == 0
        assert np.array_equal(_bits(f0), _bits(_launch(ds, wf, wctx, list(range(nprob)), x0, m)))
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        xh, fh = x0.copy(), np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_lm_solve(ds.h.ptr, C.byref(o), md, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, x0)
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=j, opts=o)
        assert np.array_equal(_bits(xh), _bits(x.cpu().numpy())) and np.array_equal(_bits(fh), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(nprob)] == ibs and list(st) == status
        ch, sh, rh, qh = np.zeros((nprob, 4, 4)), np.zeros((nprob, 4)), np.zeros(nprob, dtype=np.int32), np.zeros(nprob)
        assert ds.lib.nlh_dq_model_lm_covariance(ds.h.ptr, md, xh.ctypes.data_as(dp), 1, 0.0, ch.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                                 rh.ctypes.data_as(_lib.c_int32_p), qh.ctypes.data_as(dp)) == 0
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=j)
        assert np.array_equal(_bits(ch), _bits(cov.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sigma.cpu().numpy()))
        assert np.array_equal(rh, rank.cpu().numpy()) and np.array_equal(_bits(qh), _bits(chi2.cpu().numpy()))
    finally:
        ds.lib.nlh_dq_model_destroy(md)
        ds.lib.nlh_dq_model_destroy(inner)
        wctx.close()


@pytest.fixture(scope="module")
def fortran_loss_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_loss")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "loss_fit")


def test_fortran_loss_fit(ds, fortran_loss_exe, tmp_path):
    """The Fortran user program (create_curve -> create_robust -> solve_batch -> covariance_batch: spiked Lorentzians under a
    Huber loss with a scale per spectrum) prints the x, sigma and counts of the Python path, digit for digit (ES24.16)."""
    m, nout, nprob = 64, 4, 6
    t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob, seed=31)
    c = _problem_scales(nprob)
    path = str(tmp_path / "spikes.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(x0.tobytes()); fh.write(c.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_loss_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    o = ds.options(max_evals=500)
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, dy)
    wf, wj, wctx = ds.loss_launchers(nl.Loss("huber", c), fcn, jac, ctx)
    x = _dev(ds, x0)
    fvec, ibs, st = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=wj)
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


# ------------------------------------------------------------------------------------------------ 6. error returns
def test_error_returns(ds):
    """In the documented order; nothing is written where a call is refused."""
    m, nprob = 6, 2
    import curve_cases as CC
    t, y, xt, x0 = CC.curve_problems(KIND, 2, 0, m, nprob=nprob)           # N = 7 > m = 6
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    pm = nl.ParamMap(7, fixed=(6,), tied={5: (2, 1.25, 0.0)})           # nfree 5
    pm4 = nl.ParamMap(4)
    dc = _dev(ds, np.full(nprob, 0.1))
    f = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)

    def fit(kd, mm, p, loss, scale=dc, x=dx, h=ds.h.ptr):
        return ds.lib.nlh_curve_fit_batch_loss(h, C.byref(o), kd, 2, 0, nprob, mm, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                               p.ptr if p is not None else None, loss, scale.data_ptr() if scale is not None else None, 0,
                                               x.data_ptr() if x is not None else None, f.data_ptr(), None, None, None, None, None, None)
    assert fit(1, m, pm, 1, h=None) == -3                               # NLH_ERR_BAD_HANDLE first
    assert fit(7, m, pm, 1) == NL_INVALID_INPUT_ERROR                   # the model
    assert fit(1, m, pm4, 1) == NL_INVALID_INPUT_ERROR                  # a map of another model
    assert fit(1, 4, pm, 1) == NL_UNDERDEFINED_PROBLEM_ERROR            # m < nfree
    assert fit(1, m, None, 1) == NL_UNDERDEFINED_PROBLEM_ERROR          # m < N without a map
    assert fit(1, m, pm, 4) == NL_INVALID_INPUT_ERROR and fit(1, m, pm, -1) == NL_INVALID_INPUT_ERROR   # the kind of loss
    assert fit(1, m, pm, 1, scale=None) == NL_INVALID_INPUT_ERROR and fit(1, m, pm, 1, x=None) == NL_INVALID_INPUT_ERROR
    torch.cuda.synchronize()
    assert (f == 7.0).all() and torch.equal(dx, _dev(ds, x0))
    assert fit(1, m, pm, 1) == 0
    # host scales are checked: not finite, not positive
    xh, fh = x0.copy(), np.zeros((nprob, m))
    e = nl.Expr("a1/(1+((t-m1)/w1)^2) + a2/(1+((t-m2)/w2)^2) + c", ("t",), ("a1", "m1", "w1", "a2", "m2", "w2", "c"))
    for bad in ([0.1, 0.0], [0.1, -2.0], [np.inf, 0.1], [0.1, np.nan]):
        sc = np.array(bad)
        assert ds.lib.nlh_curve_fit_batch_loss_h(ds.h.ptr, C.byref(o), 1, 2, 0, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1,
                                                 None, None, pm.ptr, 2, sc.ctypes.data_as(dp), 0, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp),
                                                 None, None, None, None, None, None) == NL_INVALID_INPUT_ERROR
        assert ds.lib.nlh_expr_fit_batch_loss_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1,
                                                None, None, pm.ptr, 3, sc.ctypes.data_as(dp), 0, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp),
                                                None, None, None, None, None, None) == NL_INVALID_INPUT_ERROR
    assert np.array_equal(xh, x0) and (fh == 0.0).all()
    assert ds.lib.nlh_curve_fit_batch_loss_h(ds.h.ptr, C.byref(o), 1, 2, 0, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1, None,
                                             None, pm.ptr, 2, None, 0, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), None, None, None, None,
                                             None, None) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_expr_fit_batch_loss(ds.h.ptr, C.byref(o), e.ptr, nprob, m, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None, pm4.ptr, 1,
                                          dc.data_ptr(), 0, dx.data_ptr(), f.data_ptr(), None, None, None, None, None, None) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_expr_fit_batch_loss(ds.h.ptr, C.byref(o), e.ptr, nprob, 4, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None, pm.ptr, 1,
                                          dc.data_ptr(), 0, dx.data_ptr(), f.data_ptr(), None, None, None, None, None, None) == NL_UNDERDEFINED_PROBLEM_ERROR
    # a bad scale on the device: that problem's residuals are NaN, the other's are not
    fcn, jac, ctx = ds.curve_launchers(KIND, 2, 0, dt, dy)
    dbad = _dev(ds, np.array([0.1, -1.0]))
    out = C.c_void_p(7)
    none = C.cast(None, _lib.DEVFCN)
    assert ds.lib.nlh_loss_wrap(ds.h.ptr, 9, dbad.data_ptr(), 0, fcn, jac, ds._ctxp(ctx), C.byref(out)) == NL_INVALID_INPUT_ERROR and not out.value
    assert ds.lib.nlh_loss_wrap(ds.h.ptr, 1, dbad.data_ptr(), 0, none, jac, ds._ctxp(ctx), C.byref(out)) == NL_UNDEFINED_FUNCTION_ERROR
    assert ds.lib.nlh_loss_wrap(ds.h.ptr, 1, None, 0, fcn, jac, ds._ctxp(ctx), C.byref(out)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_loss_wrap(ds.h.ptr, 1, dbad.data_ptr(), 0, fcn, jac, ds._ctxp(ctx), C.byref(out)) == 0 and out.value
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    F = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)
    J = torch.full((nprob, 7, m), 7.0, dtype=torch.float64, device=ds.device)
    lst = _dev(ds, [0, 1], np.int32)
    assert ds.lib.nlh_loss_device_fcn(out, stream, nprob, lst.data_ptr(), 7, dx.data_ptr(), m, F.data_ptr()) == 0
    assert ds.lib.nlh_loss_device_jac(out, stream, nprob, lst.data_ptr(), 7, dx.data_ptr(), m, J.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(F[0]).any() and torch.isnan(F[1]).all() and not torch.isnan(J[0]).any() and torch.isnan(J[1]).all()
    ds.lib.nlh_loss_unwrap(out)
    # the launchers' own refusals, and an inner refusal handed back as it is with nothing written
    wf, wj, wctx = ds.loss_launchers(nl.Loss("huber", 0.1), fcn, None, ctx)
    assert wj is None
    J.fill_(7.0)
    args = lambda n_, m_: (wctx.ptr, stream, nprob, lst.data_ptr(), n_, dx.data_ptr(), m_, J.data_ptr())
    assert ds.lib.nlh_loss_device_fcn(*args(0, m)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_loss_device_fcn(*args(7, 0)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_loss_device_jac(*args(7, m)) == NL_UNDEFINED_FUNCTION_ERROR   # no inner Jacobian launcher
    assert ds.lib.nlh_loss_device_fcn(*args(7, m + 1)) == NL_INVALID_INPUT_ERROR    # the inner launcher's refusal (m != ctx.m)
    torch.cuda.synchronize()
    assert (J == 7.0).all()
    wctx.close()
    # the model object
    md, inner = C.c_void_p(7), C.c_void_p()
    A, b = np.ones((1, 2, 2)), np.ones((1, 2))
    one = np.ones(8)
    assert ds.lib.nlh_dq_model_create(ds.h.ptr, 1, 2, 2, A.ctypes.data_as(dp), b.ctypes.data_as(dp), 0.5, C.byref(inner)) == 0
    assert ds.lib.nlh_loss_model_create(ds.h.ptr, inner, 1, one.ctypes.data_as(dp), 1, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    ds.lib.nlh_dq_model_destroy(inner)                                  # (a dense-quadratic model has no launchers to wrap)
    inner = C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, 1, 2, 0, nprob, 7, np.ones((nprob, 7)).ctypes.data_as(dp), 0,
                                         np.ones((nprob, 7)).ctypes.data_as(dp), None, 1, C.byref(inner)) == 0
    zero = np.array([1.0, 0.0])
    assert ds.lib.nlh_loss_model_create(ds.h.ptr, inner, 5, one.ctypes.data_as(dp), 1, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    assert ds.lib.nlh_loss_model_create(ds.h.ptr, inner, 1, None, 1, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    assert ds.lib.nlh_loss_model_create(ds.h.ptr, inner, 1, zero.ctypes.data_as(dp), 0, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    assert ds.lib.nlh_loss_model_create(ds.h.ptr, inner, 1, zero.ctypes.data_as(dp), 1, C.byref(md)) == 0 and md.value   # shared: [1] is read
    ds.lib.nlh_dq_model_destroy(md)
    assert ds.lib.nlh_loss_model_create(ds.h.ptr, inner, 0, None, 0, C.byref(md)) == 0 and md.value                      # LINEAR reads no scale
    ds.lib.nlh_dq_model_destroy(md)
    ds.lib.nlh_dq_model_destroy(inner)
    with pytest.raises(ValueError):                                     # Python: a scale per problem must match the batch
        ds.curve_fit_batch(KIND, dt, dy, dx, ncomp=2, baseline=0, loss=nl.Loss("huber", [0.1, 0.1, 0.1]))


# ------------------------------------------------------------------------------------------------ 7. Cauchy
def _ulps(got, ref):
    """|got - ref| in units of the float64 spacing at ref (ref: numpy.longdouble)."""
    r64 = np.abs(ref).astype(np.float64)
    return float((np.abs(got.astype(np.longdouble) - ref) / np.spacing(r64).astype(np.longdouble)).max())


@pytest.fixture(scope="module")
def log1p_probe():
    d = os.path.join(HERE, "device_loss")
    subprocess.check_call(["make", "-C", d, "-s"])
    probe = C.CDLL(os.path.join(d, "liblog1p_probe.so"))
    probe.probe_log1p.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return probe


def test_log1p_accuracy(ds, log1p_probe):
    """The error of the device library's log1p in ulp against numpy.longdouble at 2^18 arguments over [1e-12, 1e6], spread
    evenly in the logarithm (tests/device_loss/log1p_probe.hip: the function alone, compiled with the library's flags by the fixture).  The
    restatement's U_LOG1P is this maximum rounded up to an integer, no more and no less."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is no wider than float64 here: nothing to measure against"
    probe = log1p_probe
    npts = 1 << 18
    z = np.exp(np.random.default_rng(12).uniform(math.log(1e-12), math.log(1e6), npts))
    dz = _dev(ds, z)
    out = torch.empty_like(dz)
    assert probe.probe_log1p(torch.cuda.current_stream(ds.device).cuda_stream, npts, dz.data_ptr(), out.data_ptr()) == 0
    torch.cuda.synchronize()
    worst = _ulps(out.cpu().numpy(), np.log1p(z.astype(np.longdouble)))
    print(f"loss function accuracy log1p: {worst:.3f} ulp over [1e-12, 1e6] (table {LR.U_LOG1P})")
    assert math.ceil(worst) == LR.U_LOG1P, (worst, LR.U_LOG1P)


@pytest.mark.parametrize("m,n", [(64, 4), (129, 3), (301, 9)])
def test_cauchy_within_the_bound(ds, m, n):
    """Cauchy through the launchers and nlh_loss_apply_batch against the restatement: |device - numpy| within
    loss_restatement.cauchy_bounds -- out, g and the rows of J, whose entries add one rounding of the product g * J to g's
    bound --; wgt, which no library function reaches, and every row with r = 0, bit for bit."""
    nprob = 5
    (fcn, jac, ctx), x0, keep = _inner(ds, n, m, nprob, seed=7 * m + n)
    rows = [0, 3, 3, 1, 4, 2]
    X = x0[rows]
    rawF = _launch(ds, fcn, ctx, rows, X, m)
    rawJ = _launch(ds, jac, ctx, rows, X, m, jac=True)
    c = _scales(_launch(ds, fcn, ctx, list(range(nprob)), x0, m), nprob)
    wf, wj, wctx = ds.loss_launchers(nl.Loss("cauchy", c), fcn, jac, ctx)
    worst = 0.0
    for form in ("row", "flat"):
        with _env(NLH_LOSS_FORM=form):
            F = _launch(ds, wf, wctx, rows, X, m)
            J = _launch(ds, wj, wctx, rows, X, m, jac=True)
        for q, p in enumerate(rows):
            wo, wg, ww = LR.apply(LR.CAUCHY, c[p], rawF[q])
            bo, bg = LR.cauchy_bounds(wo, wg)
            assert (np.abs(F[q] - wo) <= bo).all(), (form, q)
            wJ = wg[None, :] * rawJ[q]
            assert (np.abs(J[q] - wJ) <= bg[None, :] * np.abs(rawJ[q]) + LR.U * np.abs(wJ)).all(), (form, q)
            worst = max(worst, float((np.abs(F[q] - wo) / np.spacing(np.abs(wo))).max()))
    print(f"cauchy m = {m} n = {n}: out differs from numpy by at most {worst:.1f} ulp")
    r = np.ascontiguousarray(rawF[:nprob])
    r[:, 0] = 0.0
    out, g, wgt = (v.cpu().numpy() for v in ds.loss_apply(nl.Loss("cauchy", c[rows[:nprob]]), _dev(ds, r)))
    wo, wg, ww = LR.apply(LR.CAUCHY, c[rows[:nprob]][:, None], r)
    bo, bg = LR.cauchy_bounds(wo, wg)
    assert (np.abs(out - wo) <= bo).all() and (np.abs(g - wg) <= bg).all()
    assert np.array_equal(_bits(wgt), _bits(ww))
    assert np.array_equal(_bits(out[:, 0]), _bits(r[:, 0])) and (g[:, 0] == 1.0).all()
    wctx.close()
