"""GPU tests of the Poisson likelihood fits (include/nonlin_hip.h: nlh_pois_*): the kernels through the wrapping launchers
against the numpy restatement (tests/pois_restatement.py) for every launch shape, form, column split and slicing -- bit for
bit on the rows that reach no library function, within the derived bound on the others --; masked rows; the NaN rules; LM and
bounded solves through the wrappers against the CPU oracle, alone and inside a parameter map, within the tolerance recorded
by the perturbation study; the one-call fits as the composition they stand for, bit for bit; a problem alone against the same
problem inside a batch of 300; the model object; the Fortran program; the error returns; the device library's log."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import curve_cases as CC
import curve_restatement as R
import pmap_restatement as PM
import pois_cases as PC
import pois_restatement as PR
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
FORMS = [None, "row", "flat"]               # None: the form m selects; a forced form that cannot hold m falls back to it
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR = 201, 211, 212
KIND, K, B = PC.KIND, PC.K, PC.B
F = PR.MU_FLOOR
AREA_BOUND = PC.AREA_BOUND


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


class _env:
    """Environment variables for the calls inside (the library reads NLH_POIS_* at every call); None: unset."""

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


def _branch_data(n, m, nprob, seed):
    """An inner model of n parameters on m rows -- the formula a*t (n = 1) or a Lorentzian model (n = 3, 4, 5, 9) -- with
    counts y, a mask w and a floor f chosen from the model's values at x0 so that every path of the table occurs: row i of
    problem p takes pattern (5 p + i) mod 6 -- masked; y = 0; y within 2^-8 of the model (the series); the model 2 % .. 300 %
    above or 2 % .. 45 % below y (log1p); the model at 1 % .. 45 % of y (log) -- and the floor lies inside the range of the
    model's values (m = 1: just above the second smallest), so that rows of every pattern fall below it.
    Returns (make(ds) -> (launchers, keep), t, y, w, f, x0)."""
    rng = np.random.default_rng(seed)
    if n == 1:
        t = np.tile(np.linspace(-1.0, 1.0, m) if m > 1 else np.array([0.7]), (nprob, 1)) + rng.uniform(-0.1, 0.1, (nprob, m)) / m
        x0 = rng.uniform(0.5, 1.5, (nprob, 1))
        model = x0 * t
        if m == 1:
            t[1] = -t[1]                                             # a negative model value: below any floor
            model = x0 * t
    else:
        KK, BB = {3: (1, -1), 4: (1, 0), 5: (1, 1), 9: (2, 2)}[n]
        t, _, xt, x0 = CC.curve_problems("lorentz", KK, BB, m, nprob=nprob, seed=seed, sigma=0.02)
        if m == 1:
            t[:, 0] = x0[:, 1]                                       # on the first peak: six positive model values
        model = np.stack([R.model(R.LORENTZ, KK, BB, x0[p], t[p]) for p in range(nprob)])
    mag = np.maximum(np.abs(model), 1e-3)
    pat = (5 * np.arange(nprob)[:, None] + np.arange(m)[None, :]) % 6
    sgn = rng.choice([-1.0, 1.0], (nprob, m))
    e = np.select([pat == 2, pat == 3, pat == 4, pat == 5],
                  [sgn * rng.uniform(0.0, 2.0 ** -8, (nprob, m)), np.where(sgn > 0, rng.uniform(0.02, 3.0, (nprob, m)), -rng.uniform(0.02, 0.45, (nprob, m))),
                   -rng.uniform(0.55, 0.99, (nprob, m)), -rng.uniform(0.55, 0.99, (nprob, m))], 0.0)
    y = np.where(pat <= 1, 0.0, mag / (1.0 + e))
    w = np.where(pat == 0, 0.0, 1.0)
    y[pat == 0] = rng.choice([3.0, 0.0, np.nan, -2.0, np.inf], int((pat == 0).sum()))      # a masked row may hold anything
    vals = np.sort(model.ravel())
    f = max(float(vals[1]) * 1.01, F) if m == 1 else max(0.5 * float(np.median(np.abs(model))), F)

    def make(ds):
        dt, dy = _dev(ds, t), _dev(ds, y)
        if n == 1:
            ex = nl.Expr("a*t", ("t",), ("a",))
            return ds.expr_launchers(ex, dt, dy), (ex, dt, dy)
        return ds.curve_launchers("lorentz", KK, BB, dt, dy), (dt, dy)
    return make, t, y, w, f, x0


def _check_rows(F_, J_, rawF, rawJ, y, w, f, what, seen):
    """One point's F [m] and J [n, m] against the restatement on the device's own inner rawF, rawJ."""
    wo, wg, wD, br = PR.apply(y, w, f, rawF)
    low = PR.branches(y, w, f, rawF)[1]
    bo, bg = PR.device_bounds(y, w, f, rawF)
    exact = ~PR.uses_library(br)
    assert np.array_equal(_bits(F_[exact]), _bits(wo[exact])), what
    assert (np.abs(F_ - wo)[~exact] <= bo[~exact]).all(), what
    wJ = PR.jacobian(y, w, f, rawF, rawJ.T).T
    assert np.array_equal(_bits(J_[:, exact]), _bits(wJ[:, exact])), what
    assert (np.abs(J_ - wJ)[:, ~exact] <= (bg[None, :] * np.abs(rawJ) + PR.U * np.abs(wJ))[:, ~exact]).all(), what
    for b in range(5):
        seen[b] |= bool((br == b).any())
    seen[5] |= bool(low.any())
    seen[6] |= bool((low & PR.uses_library(br)).any())


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("m", [1, 64, 128, 129, 256, 257, 301])
def test_launchers_against_restatement(ds, m, n):
    """k_pois_fcn and k_pois_jac through the wrapping launchers: F = out(inner F) and J = g * inner J of the restatement,
    applied to what the inner launchers give for the same points -- with and without dprob, a point list with repeated
    problems, both forms, the column split forced, sliced and unsliced.  Every path of the table occurs and is seen: masked,
    y = 0, series, log1p, log, floor.  Rows that use no library function are bit for bit, the others within the bound."""
    nprob = 6 if m == 1 else 5
    make, t, y, w, f, x0 = _branch_data(n, m, nprob, seed=100 * n + m)
    (fcn, jac, ctx), keep = make(ds)
    dy, dw = _dev(ds, y), _dev(ds, w)
    stat = nl.Poisson(f)
    wf, wj, wctx = ds.pois_launchers(stat, fcn, jac, ctx, dy, dw)
    shapes = [None, list(np.random.default_rng(3).integers(0, nprob, 23)) + [0, 0, nprob - 1], [nprob - 2]]
    seen = [False] * 7
    for k, plist in enumerate(shapes):
        rows = list(range(nprob)) if plist is None else [int(p) for p in plist]
        X = x0[rows] * (1.0 + (0.002 if k else 0.0) * np.random.default_rng(k).uniform(-1, 1, (len(rows), n)))
        rawF = _launch(ds, fcn, ctx, rows, X, m)
        rawJ = _launch(ds, jac, ctx, rows, X, m, jac=True)
        # (split: column groups; scratch: a cap that cuts a call into slices of two points)
        for form in FORMS:
            for split, sliced in ((None, False), (2, False), (n, True), (None, True)):
                with _env(NLH_POIS_FORM=form, NLH_POIS_SPLIT=split, NLH_POIS_SCRATCH=8 if sliced else None):
                    Fg = _launch(ds, wf, wctx, plist, X, m)          # (without dprob: its problem list comes in slices of two)
                with _env(NLH_POIS_FORM=form, NLH_POIS_SPLIT=split, NLH_POIS_SCRATCH=2 * (8 * m + 4) if sliced else None):
                    Jg = _launch(ds, wj, wctx, plist, X, m, jac=True)
                for q, p in enumerate(rows):
                    _check_rows(Fg[q], Jg[q], rawF[q], rawJ[q], y[p], w[p], f, (k, q, form, split, sliced), seen)
    wctx.close()
    want = 6 if m == 1 else 7                                           # (m = 1: six rows; a floor row on a library path needs more)
    assert all(seen[:want]), seen
    # without a mask: the rows the mask keeps as they were, with and without dprob
    wf, wj, wctx = ds.pois_launchers(stat, fcn, jac, ctx, dy, dw)
    nf, nj, nctx = ds.pois_launchers(stat, fcn, jac, ctx, dy)
    rows, keepr = list(range(nprob)), w == 1.0
    Fm, Jm = _launch(ds, wf, wctx, rows, x0, m), _launch(ds, wj, wctx, rows, x0, m, jac=True)
    for plist in (rows, None):
        Fn, Jn = _launch(ds, nf, nctx, plist, x0, m), _launch(ds, nj, nctx, plist, x0, m, jac=True)
        assert np.array_equal(_bits(Fn[keepr]), _bits(Fm[keepr]))
        for q in rows:
            assert np.array_equal(_bits(Jn[q][:, keepr[q]]), _bits(Jm[q][:, keepr[q]]))
    nctx.close()
    wctx.close()


def test_apply_batch(ds):
    """nlh_pois_apply_batch: out, g and the row deviances of the table; any output may be NULL; out may be r itself."""
    rng = np.random.default_rng(5)
    nprob, m = 7, 301
    mu = np.exp(rng.uniform(np.log(0.02), np.log(300.0), (nprob, m)))
    y = rng.poisson(mu).astype(np.float64)
    mu[:, :9] = y[:, :9] * (1.0 + rng.uniform(-2.0 ** -7, 2.0 ** -7, (nprob, 9)))          # the series, e = 0 among them
    mu[:, 9] = y[:, 9]
    mu[:, 10:14] = rng.uniform(-2.0, 1e-7, (nprob, 4))                                      # below the floor
    w = (rng.uniform(size=(nprob, m)) > 0.2).astype(np.float64)
    r = mu - y
    dr, dy, dw = _dev(ds, r), _dev(ds, y), _dev(ds, w)
    stat = nl.Poisson()
    for mask, dmask in ((w, dw), (None, None)):
        got = [v.cpu().numpy() for v in ds.pois_apply(stat, dr, dy, dmask)]
        wo, wg, wD, br = PR.apply(y, mask, F, r)
        low = PR.branches(y, mask, F, r)[1]
        bo, bg = PR.device_bounds(y, mask, F, r)
        exact = ~PR.uses_library(br)
        assert {0, 1, 2, 3, 4} - set(np.unique(br)) == ({0} if mask is None else set()) and low.any()
        for g_, w_ in zip(got, (wo, wg, wD)):
            assert np.array_equal(_bits(g_[exact]), _bits(w_[exact]))
        assert (np.abs(got[0] - wo) <= bo).all() and (np.abs(got[1] - wg) <= bg).all()
        relD = 2 * PR.device_bounds(y, mask, F, r)[0] / np.where(np.abs(wo) > 0, np.abs(wo), 1.0)
        assert (np.abs(got[2] - wD)[~exact & ~low] <= ((relD + 2 * PR.U) * np.abs(wD))[~exact & ~low]).all()
    inplace = dr.clone()
    assert ds.lib.nlh_pois_apply_batch(ds.h.ptr, nprob, m, dy.data_ptr(), dw.data_ptr(), F, inplace.data_ptr(), inplace.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert _eq(inplace, ds.pois_apply(stat, dr, dy, dw)[0])


@pytest.mark.parametrize("m,n", [(129, 4), (64, 3), (257, 5)])
def test_masked_rows_are_exactly_zero(ds, m, n):
    """Masked rows are +0.0 in F and in every column of J under both forms, whatever y and the inner rows hold."""
    nprob = 5
    make, t, y, w, f, x0 = _branch_data(n, m, nprob, seed=9)
    rng = np.random.default_rng(2)
    w = (rng.uniform(size=(nprob, m)) > 0.3).astype(np.float64)
    w[:, -1] = 0.0
    y = np.where(w == 0.0, rng.choice([np.nan, -1.0, np.inf, 2.0], (nprob, m)), np.where(np.isfinite(y) & (y >= 0), y, 1.0))
    dt = _dev(ds, t)
    dy, dw = _dev(ds, y), _dev(ds, w)
    KK, BB = {3: (1, -1), 4: (1, 0), 5: (1, 1)}[n]
    fcn, jac, ctx = ds.curve_launchers("lorentz", KK, BB, dt, dy)
    wf, wj, wctx = ds.pois_launchers(nl.Poisson(f), fcn, jac, ctx, dy, dw)
    rows = list(range(nprob))
    z = w == 0.0
    for form in ("row", "flat"):
        for split in (None, n):
            with _env(NLH_POIS_FORM=form, NLH_POIS_SPLIT=split):
                Fg = _launch(ds, wf, wctx, rows, x0, m)
                Jg = _launch(ds, wj, wctx, rows, x0, m, jac=True)
            assert z.any() and (_bits(Fg[z]) == 0).all()
            for q in rows:
                assert (_bits(Jg[q][:, z[q]]) == 0).all()
                assert np.isfinite(Fg[q][~z[q]]).all() and np.isfinite(Jg[q][:, ~z[q]]).all()
    wctx.close()


def test_nan_rules(ds):
    """w neither 0 nor 1, y < 0 or y not finite: that row NaN, it alone; a floor that is not finite or not positive: every
    row NaN, masked ones included, through apply and through the launchers."""
    nprob, m = 3, 64
    t, yc, xt, x0 = PC.decay_problems(50.0, nprob)
    y, w = yc.copy(), np.ones((nprob, m))
    y[0, 3], y[1, 5], y[2, 7], y[2, 8] = -1.0, np.nan, np.inf, -1e-300
    w[0, 10], w[1, 11], w[2, 12], w[0, 13], w[1, 20] = 0.5, 2.0, np.nan, -1.0, 0.0
    bad = np.zeros((nprob, m), bool)
    for p, i in ((0, 3), (1, 5), (2, 7), (2, 8), (0, 10), (1, 11), (2, 12), (0, 13)):
        bad[p, i] = True
    model = np.stack([R.model(R.EXPDECAY, K, B, x0[p], t[p]) for p in range(nprob)])
    r = model - yc
    dr, dy, dw = _dev(ds, r), _dev(ds, y), _dev(ds, w)
    out, g, dev = (v.cpu().numpy() for v in ds.pois_apply(nl.Poisson(), dr, dy, dw))
    for v in (out, g, dev):
        assert np.isnan(v[bad]).all() and not np.isnan(v[~bad]).any()
    assert _bits(out[1, 20:21])[0] == 0 and _bits(g[1, 20:21])[0] == 0
    wo, wg, wD, br = PR.apply(y, w, F, r)
    assert np.array_equal(np.isnan(wo), bad)
    dt = _dev(ds, t)
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, _dev(ds, yc))
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    lst = _dev(ds, list(range(nprob)), np.int32)
    dx = _dev(ds, x0)
    for bad_f in (0.0, -1.0, float("inf"), float("nan")):
        o2 = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)
        assert ds.lib.nlh_pois_apply_batch(ds.h.ptr, nprob, m, dy.data_ptr(), dw.data_ptr(), bad_f, dr.data_ptr(), o2.data_ptr(), None, None) == 0
        c = C.c_void_p()
        assert ds.lib.nlh_pois_wrap(ds.h.ptr, dy.data_ptr(), dw.data_ptr(), bad_f, fcn, jac, ds._ctxp(ctx), C.byref(c)) == 0
        Fg = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)
        Jg = torch.full((nprob, 3, m), 7.0, dtype=torch.float64, device=ds.device)
        assert ds.lib.nlh_pois_device_fcn(c, stream, nprob, lst.data_ptr(), 3, dx.data_ptr(), m, Fg.data_ptr()) == 0
        assert ds.lib.nlh_pois_device_jac(c, stream, nprob, lst.data_ptr(), 3, dx.data_ptr(), m, Jg.data_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.isnan(o2).all() and torch.isnan(Fg).all() and torch.isnan(Jg).all()
        ds.lib.nlh_pois_unwrap(c)


# ------------------------------------------------------------------------------------------------ 2. the oracle
def _family(nprob=24):
    """The decay family's first nprob / 2 problems at each amplitude."""
    parts = [PC.decay_problems(a, nprob // 2) for a in PC.AMPLITUDES]
    return tuple(np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in range(4))


def _oracle_callbacks(ds, inner, p, y, w, f, m, analytic, T=None, full=None):
    """(fcn, jac) of problem p for the oracle: the restated transform (numpy's log1p and log) on the DEVICE's own inner
    residual and Jacobian (a round trip per callback, as tests/test_gpu_curve.py does for the exp kinds), so that the two
    solves differ by the library functions of the transform alone -- what the perturbation study measures."""
    fi, ji, ci = inner
    ex = (lambda x: np.array(x)) if T is None else (lambda x: PM.expand(T, np.array(x), full))
    con = (lambda J: J) if T is None else (lambda J: PM.contract(T, J))
    raw = lambda x: _launch(ds, fi, ci, [p], ex(x)[None, :], m)[0]
    rawJ = lambda x: _launch(ds, ji, ci, [p], ex(x)[None, :], m, jac=True)[0].T
    fcn = lambda x, out: out.__setitem__(slice(None), PR.residual(y, w, f, raw(x)))
    jac = (lambda x, J: J.__setitem__((slice(None), slice(None)), con(PR.jacobian(y, w, f, raw(x), rawJ(x))))) if analytic else None
    return fcn, jac


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("model", ["curve", "formula"])
def test_solves_against_oracle(ds, oracle, model, analytic, bounded):
    """lm_solve / cls_solve of the oracle with the restated transform as callbacks, under default options, 24 problems of the
    decay family: statuses equal, x within the recorded tolerance (4 x what a last-bit change of log1p / log did to the
    oracle's own fit), and the area rule on the device's unbounded fits."""
    nprob, m = 24, PC.M
    t, y, xt, x0 = _family(nprob)
    dt, dy = _dev(ds, t), _dev(ds, y)
    e = nl.Expr(PC.FORMULA, ("t",), PC.PARAMS)
    inner = ds.curve_launchers(KIND, K, B, dt, dy) if model == "curve" else ds.expr_launchers(e, dt, dy)
    wf, wj, wctx = ds.pois_launchers(nl.Poisson(), inner[0], inner[1], inner[2], dy)
    lower = upper = None
    if bounded:                                                         # bounds that bind: the rate from below, the baseline from above
        lower, upper = np.array([1.0, 1.02, 0.0]), np.array([5000.0, 3.0, 0.45])
        x0 = np.clip(x0, lower, upper)
    x = _dev(ds, x0)
    o = ds.options()
    if bounded:
        fvec, ibs, status = ds.cls_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=o, lower=lower, upper=upper)
    else:
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=o)
    xg = x.cpu().numpy()
    tol = PC.recorded_tolerance(analytic)
    oo = oracle.default_options()
    worst = 0.0
    for p in range(nprob):
        f, j = _oracle_callbacks(ds, inner, p, y[p], None, F, m, analytic)
        if bounded:
            rc, xo, fo, ibo = oracle.cls_solve(f, m, 3, x0[p], jac=j, opts=oo, lower=lower, upper=upper)
        else:
            rc, xo, fo, ibo = oracle.lm_solve(f, m, 3, x0[p], jac=j, opts=oo)
        what = (model, analytic, bounded, p)
        assert status[p] == rc, (what, status[p], rc)
        assert (np.abs(xg[p] - xo) <= tol * np.abs(xo)).all(), (what, xg[p], xo, tol)     # (a component on a bound at 0: equal)
        worst = max(worst, float(np.max(np.abs(xg[p] - xo)[xo != 0] / np.abs(xo[xo != 0]))))
        if not bounded:
            a = PC.AMPLITUDES[0] if p < nprob // 2 else PC.AMPLITUDES[1]
            area = abs(R.model(R.EXPDECAY, K, B, xg[p], t[p]).sum() - y[p].sum()) / y[p].sum()
            assert area <= AREA_BOUND[a], (what, area)
    print(f"poisson solves against oracle {model} analytic={analytic} bounded={bounded}: worst relative difference of x {worst:.3g} (allowed {tol:.3g})")
    if not bounded:
        assert set(status) == {0}
    wctx.close()


@pytest.mark.parametrize("analytic", [False, True])
def test_solve_through_a_map_against_oracle(ds, oracle, analytic):
    """The Poisson pair inside a parameter map, the baseline fixed at its true value: the map's launchers around the Poisson
    launchers around the curve model's, against the oracle on expand -> model -> transform -> contract."""
    nprob, m = 24, PC.M
    t, y, xt, x0 = _family(nprob)
    T = PM.tables(3, (2,), None)
    pm = nl.ParamMap(3, fixed=(2,))
    assert pm.nfree == 2
    full = x0.copy()
    full[:, 2] = xt[:, 2]
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    inner = ds.curve_launchers(KIND, K, B, dt, dy)
    qf, qj, qctx = ds.pois_launchers(nl.Poisson(), inner[0], inner[1], inner[2], dy)
    wf, wj, wctx = ds.pmap_launchers(pm, qf, qj, qctx, dfull)
    x = ds.pmap_gather(pm, dfull)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options())
    xg = x.cpu().numpy()
    tol = PC.recorded_tolerance(analytic)
    oo = oracle.default_options()
    for p in range(nprob):
        f, j = _oracle_callbacks(ds, inner, p, y[p], None, F, m, analytic, T, full[p])
        rc, xo, fo, ibo = oracle.lm_solve(f, m, 2, PM.gather(T, full[p]), jac=j, opts=oo)
        assert status[p] == rc == 0, (p, status[p], rc)
        rel = float(np.max(np.abs(xg[p] - xo) / np.abs(xo)))
        assert rel <= tol, (analytic, p, rel, tol)
    wctx.close()
    qctx.close()


# ------------------------------------------------------------------------------------------------ 3. the composition
def _mask(nprob, m, seed=4):
    """A 0 / 1 mask: ragged tails and a few holes; problem 1 keeps two rows only (no degree of freedom for two unknowns or three)."""
    rng = np.random.default_rng(seed)
    w = np.ones((nprob, m))
    for p in range(nprob):
        w[p, m - int(rng.integers(0, 12)):] = 0.0
        w[p, rng.choice(m - 12, 3, replace=False)] = 0.0
    w[1, 2:] = 0.0
    return w


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("model", ["curve", "formula"])
def test_one_call_fit_is_the_composition(ds, model, mapped, analytic, masked):
    """nlh_curve_fit_batch_pois / nlh_expr_fit_batch_pois = the launchers composed by hand, GPU against GPU and bit for bit:
    x, fvec (the deviance residual), sigma and cov (unscaled), chi2 (the deviance / dof), rank, counts and status; the
    unmasked form also bounded."""
    nprob, m = 16, PC.M
    t, y, xt, x0 = _family(nprob)
    stat = nl.Poisson()
    pm = nl.ParamMap(3, fixed=(2,)) if mapped else None
    n = 2 if mapped else 3
    start = x0.copy()
    if mapped:
        start[:, 2] = xt[:, 2]
    w = _mask(nprob, m) if masked else None
    dt, dy, dstart = _dev(ds, t), _dev(ds, y), _dev(ds, start)
    dw = _dev(ds, w) if masked else None
    o = ds.options()
    e = nl.Expr(PC.FORMULA, ("t",), PC.PARAMS)
    for lower, upper in ((None, None),) if masked else ((None, None), (np.array([1.0, 1.02, 0.0]), np.array([5000.0, 3.0, 0.45]))):
        s0 = dstart if lower is None else _dev(ds, np.clip(start, lower, upper))
        if model == "curve":
            got = ds.curve_fit_batch(KIND, dt, dy, s0, ncomp=K, baseline=B, weights=dw, lower=lower, upper=upper, analytic=analytic, opts=o,
                                     pmap=pm, stat=stat)
        else:
            got = ds.expr_fit_batch(e, dt, dy, s0, weights=dw, lower=lower, upper=upper, analytic=analytic, opts=o, pmap=pm, stat=stat)
        # by hand: every run of consecutive problems that have degrees of freedom is a call of its own -- pois_launchers,
        # then (with a map) pmap_launchers around them; gather, solve, covariance with scaled=False, expand, cov_expand --
        # and the dof rule: chi2 = (sum of f_i^2, ascending) / (unmasked rows - n), cov and sigma as they are; a problem
        # without a degree of freedom is refused before anything is evaluated and keeps its x
        nz = (w != 0).sum(1) if masked else np.full(nprob, m)
        live = [p for p in range(nprob) if nz[p] - n > 0]
        assert (len(live) == nprob - 1) if masked else (len(live) == nprob)
        f2f = pm.tables()[4] if mapped else slice(None)
        xs = ds.pmap_gather(pm, s0) if mapped else s0.clone()
        fv = torch.zeros((nprob, m), dtype=torch.float64, device=ds.device)
        status = [NL_INVALID_INPUT_ERROR] * nprob
        ibs = [None] * nprob
        cov_h, sig_h, chi_h, rank_h = np.full((nprob, n, n), np.nan), np.full((nprob, n), np.nan), np.full(nprob, np.nan), np.full(nprob, -1)
        runs, p = [], 0
        while p < nprob:
            if p not in live:
                p += 1
                continue
            q = p
            while q < nprob and q in live:
                q += 1
            runs.append((p, q))
            p = q
        for p0, p1 in runs:
            # a run of problems is a call of its own on launchers whose data start at p0
            sub = (ds.curve_launchers(KIND, K, B, dt[p0:p1].contiguous(), dy[p0:p1].contiguous()) if model == "curve"
                   else ds.expr_launchers(e, dt[p0:p1].contiguous(), dy[p0:p1].contiguous()))
            sy = dy[p0:p1].contiguous()
            sw = dw[p0:p1].contiguous() if masked else None
            sq = ds.pois_launchers(stat, sub[0], sub[1], sub[2], sy, sw)
            if pm is not None:
                sfull = s0[p0:p1].contiguous()
                sm = ds.pmap_launchers(pm, sq[0], sq[1], sq[2], sfull)
            else:
                sm = sq
            xr = xs[p0:p1].contiguous()
            jj = sm[1] if analytic else None
            if lower is not None:
                fr, ibr, sr = ds.cls_solve_batch_device(sm[0], sm[2], m, xr, jac=jj, opts=o, lower=lower[f2f], upper=upper[f2f])
            else:
                fr, ibr, sr = ds.lm_solve_batch_device(sm[0], sm[2], m, xr, jac=jj, opts=o)
            cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(sm[0], sm[2], m, xr, jac=jj, scaled=False)
            xs[p0:p1] = xr
            fv[p0:p1] = fr
            status[p0:p1] = sr
            ibs[p0:p1] = ibr
            cov_h[p0:p1], sig_h[p0:p1], rank_h[p0:p1], chi_h[p0:p1] = cov.cpu().numpy(), sigma.cpu().numpy(), rank.cpu().numpy(), chi2.cpu().numpy()
            if pm is not None:
                sm[2].close()
            sq[2].close()
        xfull = ds.pmap_expand(pm, xs, s0) if mapped else xs
        assert _eq(got[0], xfull)
        fh, fg = fv.cpu().numpy(), got[1].cpu().numpy()
        sg, cg, qg, rg = (v.cpu().numpy() for v in got[2:6])
        for p in range(nprob):
            if p not in live:
                assert got[7][p] == NL_INVALID_INPUT_ERROR and np.isnan(sg[p]).all() and np.isnan(cg[p]).all() and np.isnan(qg[p]) and rg[p] == -1
                continue
            assert got[7][p] == status[p] and got[6][p] == ibs[p], (p, got[7][p], status[p])
            assert np.array_equal(_bits(fg[p]), _bits(fh[p])), p
            if status[p] != 0:
                assert np.isnan(sg[p]).all() and np.isnan(cg[p]).all() and np.isnan(qg[p]) and rg[p] == -1
                continue
            cw, sw_ = (cov_h[p], sig_h[p]) if not mapped else PM.cov_expand(PM.tables(3, (2,), None), cov_h[p], sig_h[p])
            assert np.array_equal(_bits(sg[p]), _bits(sw_)) and np.array_equal(_bits(cg[p]), _bits(cw)), p
            assert rg[p] == rank_h[p] == n
            s = 0.0
            for v in fh[p]:
                s = s + v * v
            assert _bits(qg[p]) == _bits(s / float(nz[p] - n)), p         # the deviance over the degrees of freedom
            if not masked:
                assert _bits(qg[p]) == _bits(chi_h[p])
        if lower is None and not masked:
            assert set(got[7]) == {0}


def test_alone_inside_a_batch_of_300_host_forms_and_all_ones_mask(ds):
    """300 problems reach the sub-batches (concurrent calls of the wrapping launchers on different streams): a problem alone
    equals the same problem inside the batch; the host-array twins give the same bits; an all-ones mask equals no mask; and
    what the feature is for: on 300 decays at 50 counts the rate bias of weighted least squares exceeds three of its
    standard errors, the Poisson fit's is within three."""
    nprob, m = 300, PC.M
    t, y, xt, x0 = PC.decay_problems(50.0, nprob, spread=0.0)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    stat = nl.Poisson()
    big = None
    for analytic in (False, True):
        for form in (None, "row"):
            with _env(NLH_POIS_FORM=form):
                big = ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, analytic=analytic, opts=o, stat=stat)
                for p in (0, 137, nprob - 1):
                    one = ds.curve_fit_batch(KIND, dt[p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dx0[p:p + 1].contiguous(), ncomp=K,
                                             baseline=B, analytic=analytic, opts=o, stat=stat)
                    for g, w_ in zip(one[:6], big[:6]):
                        assert _eq(g, w_[p:p + 1]), (analytic, form, p)
                    assert one[6][0] == big[6][p]
    assert set(big[7]) == {0}
    ones = ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, weights=torch.ones_like(dy), analytic=True, opts=o, stat=stat)
    for g, w_ in zip(ones[:6], big[:6]):
        assert _eq(g, w_)
    assert ones[6] == big[6] and ones[7] == big[7]
    xh, fh = x0.copy(), np.zeros((nprob, m))
    sh, ch, qh, rh = np.zeros((nprob, 3)), np.zeros((nprob, 3, 3)), np.zeros(nprob), np.zeros(nprob, dtype=np.int32)
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    rc = ds.lib.nlh_curve_fit_batch_pois_h(ds.h.ptr, C.byref(o), R.EXPDECAY, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1,
                                           None, None, None, F, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                           ch.ctypes.data_as(dp), qh.ctypes.data_as(dp), rh.ctypes.data_as(_lib.c_int32_p), ib, st)
    assert rc == 0
    for g, w_ in zip((xh, fh, sh, ch, qh), big[:5]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    assert np.array_equal(rh, big[5].cpu().numpy()) and [ib[p].as_dict() for p in range(nprob)] == big[6]
    e = nl.Expr(PC.FORMULA, ("t",), PC.PARAMS)
    bige = ds.expr_fit_batch(e, dt, dy, dx0, analytic=True, opts=o, stat=stat)
    xh2, fh2, sh2 = x0.copy(), np.zeros((nprob, m)), np.zeros((nprob, 3))
    rc = ds.lib.nlh_expr_fit_batch_pois_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1, None, None,
                                          None, F, xh2.ctypes.data_as(dp), fh2.ctypes.data_as(dp), sh2.ctypes.data_as(dp), None, None, None,
                                          None, None)
    assert rc == 0
    for g, w_ in zip((xh2, fh2, sh2), bige[:3]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    # the bias: the condition tests/test_pois_cpu.py::test_bias_study holds the reference path to, on the device
    wls = ds.curve_fit_batch(KIND, dt, dy, dx0, ncomp=K, baseline=B, weights=_dev(ds, PC.ls_weights(y)), analytic=True, opts=o, covariance=False)
    assert set(wls[7]) == {0}
    for name, fit, inside in (("weighted least squares", wls, False), ("poisson", big, True)):
        rel = (fit[0].cpu().numpy()[:, 1] - xt[:, 1]) / xt[:, 1]
        bias, se = float(rel.mean()), float(rel.std(ddof=1) / math.sqrt(nprob))
        print(f"device bias study {name}: k {100 * bias:+.2f} % +- {100 * se:.2f} %")
        assert (abs(bias) <= 3 * se) == inside, (name, bias, se)
    # sigma is the unscaled one: the inverse Fisher information predicts the scatter of the fits (within 20 % at 300 fits)
    sig_k = big[2].cpu().numpy()[:, 1]
    scatter = float((big[0].cpu().numpy()[:, 1]).std(ddof=1))
    assert 0.8 * scatter <= float(np.median(sig_k)) <= 1.25 * scatter, (scatter, float(np.median(sig_k)))


# ------------------------------------------------------------------------------------------------ 4. the model object
@pytest.mark.parametrize("analytic", [0, 1])
@pytest.mark.parametrize("masked", [False, True])
def test_model_object(ds, analytic, masked):
    """nlh_pois_model_create over a curve model made without weights, through _eval, _lm_solve, _lm_covariance = the launcher
    forms; under the mask the host counts are NaN padding."""
    nprob, m = 12, PC.M
    t, y, xt, x0 = _family(nprob)
    w = _mask(nprob, m) if masked else None
    if masked:
        w[1] = 1.0
        y[w == 0.0] = np.nan                                            # a masked row may hold anything, in host arrays too
    dt, dy = _dev(ds, t), _dev(ds, y)
    dw = _dev(ds, w) if masked else None
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, dy)
    wf, wj, wctx = ds.pois_launchers(nl.Poisson(), fcn, jac, ctx, dy, dw)
    j = wj if analytic else None
    o = ds.options()
    inner, md = C.c_void_p(), C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.EXPDECAY, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, analytic,
                                         C.byref(inner)) == 0
    assert ds.lib.nlh_pois_model_create(ds.h.ptr, inner, y.ctypes.data_as(dp), w.ctypes.data_as(dp) if masked else None, F, C.byref(md)) == 0
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
        assert ds.lib.nlh_dq_model_lm_covariance(ds.h.ptr, md, xh.ctypes.data_as(dp), 0, 0.0, ch.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                                 rh.ctypes.data_as(_lib.c_int32_p), qh.ctypes.data_as(dp)) == 0
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=j, scaled=False)
        assert np.array_equal(_bits(ch), _bits(cov.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sigma.cpu().numpy()))
        assert np.array_equal(rh, rank.cpu().numpy()) and np.array_equal(_bits(qh), _bits(chi2.cpu().numpy()))
    finally:
        ds.lib.nlh_dq_model_destroy(md)
        ds.lib.nlh_dq_model_destroy(inner)
        wctx.close()


@pytest.fixture(scope="module")
def fortran_pois_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_pois")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "pois_fit")


def test_fortran_pois_fit(ds, fortran_pois_exe, tmp_path):
    """The Fortran user program (create_curve -> create_poisson -> solve_batch -> covariance_batch with scaled = .false.:
    one masked batch of decays) prints the x, sigma and counts of the Python path, digit for digit (ES24.16)."""
    nprob, m = 6, PC.M
    t, y, xt, x0 = _family(nprob)
    w = _mask(nprob, m, seed=8)
    w[1] = 1.0
    path = str(tmp_path / "decays.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(w.tobytes()); fh.write(x0.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_pois_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    o = ds.options(max_evals=500)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, dy)
    wf, wj, wctx = ds.pois_launchers(nl.Poisson(), fcn, jac, ctx, dy, dw)
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


# ------------------------------------------------------------------------------------------------ 5. error returns
def test_error_returns(ds):
    """In the documented order; nothing is written where a call is refused."""
    m, nprob = 6, 2
    t, y, xt, x0 = CC.curve_problems("lorentz", 2, 0, m, nprob=nprob)          # N = 7 > m = 6
    y = np.abs(np.round(50 * y))
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    pm = nl.ParamMap(7, fixed=(6,), tied={5: (2, 1.25, 0.0)})           # nfree 5
    pm4 = nl.ParamMap(4)
    f = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)
    sg = torch.full((nprob, 7), 7.0, dtype=torch.float64, device=ds.device)

    def fit(kd, mm, p, floor=F, x=dx, h=ds.h.ptr, sigma=None):
        return ds.lib.nlh_curve_fit_batch_pois(h, C.byref(o), kd, 2, 0, nprob, mm, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                               p.ptr if p is not None else None, floor, x.data_ptr() if x is not None else None, f.data_ptr(),
                                               sigma.data_ptr() if sigma is not None else None, None, None, None, None, None)
    assert fit(1, m, pm, h=None) == -3                                  # NLH_ERR_BAD_HANDLE first
    assert fit(7, m, pm) == NL_INVALID_INPUT_ERROR                      # the model
    assert fit(1, m, pm4) == NL_INVALID_INPUT_ERROR                     # a map of another model
    assert fit(1, 4, pm) == NL_UNDERDEFINED_PROBLEM_ERROR               # m < nfree
    assert fit(1, m, None) == NL_UNDERDEFINED_PROBLEM_ERROR             # m < N without a map
    assert fit(1, 4, pm, floor=0.0) == NL_UNDERDEFINED_PROBLEM_ERROR    # ... before the floor is looked at
    assert fit(1, m, pm, x=None) == NL_INVALID_INPUT_ERROR
    pm6 = nl.ParamMap(7, fixed=(6,))                                    # nfree 6 = m: no degree of freedom for errors
    assert fit(1, m, pm6, floor=0.0, sigma=sg) == NL_INVALID_INPUT_ERROR
    for bad in (0.0, -1.0, float("inf"), float("nan")):                 # then the floor
        assert fit(1, m, pm, floor=bad) == NL_INVALID_INPUT_ERROR
    torch.cuda.synchronize()
    assert (f == 7.0).all() and torch.equal(dx, _dev(ds, x0))
    assert fit(1, m, pm) == 0
    # host counts and masks are checked: negative, not finite; a mask outside {0, 1}
    xh, fh = x0.copy(), np.zeros((nprob, m))
    e = nl.Expr("a1/(1+((t-m1)/w1)^2) + a2/(1+((t-m2)/w2)^2) + c", ("t",), ("a1", "m1", "w1", "a2", "m2", "w2", "c"))
    ones = np.ones((nprob, m))

    def fit_h(yy, ww, floor=F, expr=False):
        wp = ww.ctypes.data_as(dp) if ww is not None else None
        if expr:
            return ds.lib.nlh_expr_fit_batch_pois_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, yy.ctypes.data_as(dp), wp, 1,
                                                    None, None, pm.ptr, floor, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), None, None, None,
                                                    None, None, None)
        return ds.lib.nlh_curve_fit_batch_pois_h(ds.h.ptr, C.byref(o), 1, 2, 0, nprob, m, t.ctypes.data_as(dp), 0, yy.ctypes.data_as(dp), wp, 1,
                                                 None, None, pm.ptr, floor, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), None, None, None,
                                                 None, None, None)
    for expr in (False, True):
        for bad in (-1.0, np.nan, np.inf):
            yb = y.copy()
            yb[1, 2] = bad
            assert fit_h(yb, None, expr=expr) == NL_INVALID_INPUT_ERROR
        for bad in (0.5, 2.0, -1.0, np.nan):
            wb = ones.copy()
            wb[0, 4] = bad
            assert fit_h(y, wb, expr=expr) == NL_INVALID_INPUT_ERROR
        assert fit_h(y, ones, floor=0.0, expr=expr) == NL_INVALID_INPUT_ERROR
    assert np.array_equal(xh, x0) and (fh == 0.0).all()
    assert fit_h(y, ones) == 0
    for expr in (False, True):                                          # a masked row may hold anything, on host arrays too
        xh[:] = x0
        ypad, wpad = y.copy(), ones.copy()
        ypad[0, 5], wpad[0, 5] = np.nan, 0.0
        assert fit_h(ypad, wpad, expr=expr) == 0
        xpad = xh.copy()
        xh[:] = x0
        ypad[0, 5] = 3.0
        assert fit_h(ypad, wpad, expr=expr) == 0 and np.array_equal(_bits(xpad), _bits(xh))
    assert ds.lib.nlh_expr_fit_batch_pois(ds.h.ptr, C.byref(o), e.ptr, nprob, m, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None, pm4.ptr, F,
                                          dx.data_ptr(), f.data_ptr(), None, None, None, None, None, None) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_expr_fit_batch_pois(ds.h.ptr, C.byref(o), e.ptr, nprob, 4, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None, pm.ptr, F,
                                          dx.data_ptr(), f.data_ptr(), None, None, None, None, None, None) == NL_UNDERDEFINED_PROBLEM_ERROR
    # the wrap and the launchers' own refusals, and an inner refusal handed back as it is with nothing written
    fcn, jac, ctx = ds.curve_launchers("lorentz", 2, 0, dt, dy)
    out = C.c_void_p(7)
    none = C.cast(None, _lib.DEVFCN)
    assert ds.lib.nlh_pois_wrap(ds.h.ptr, dy.data_ptr(), None, F, none, jac, ds._ctxp(ctx), C.byref(out)) == NL_UNDEFINED_FUNCTION_ERROR and not out.value
    assert ds.lib.nlh_pois_wrap(ds.h.ptr, None, None, F, fcn, jac, ds._ctxp(ctx), C.byref(out)) == NL_INVALID_INPUT_ERROR and not out.value
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    J = torch.full((nprob, 7, m), 7.0, dtype=torch.float64, device=ds.device)
    lst = _dev(ds, [0, 1], np.int32)
    wf, wj, wctx = ds.pois_launchers(nl.Poisson(), fcn, None, ctx, dy)
    assert wj is None
    args = lambda n_, m_: (wctx.ptr, stream, nprob, lst.data_ptr(), n_, dx.data_ptr(), m_, J.data_ptr())
    assert ds.lib.nlh_pois_device_fcn(*args(0, m)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_pois_device_fcn(*args(7, 0)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_pois_device_jac(*args(7, m)) == NL_UNDEFINED_FUNCTION_ERROR   # no inner Jacobian launcher
    assert ds.lib.nlh_pois_device_fcn(*args(7, m + 1)) == NL_INVALID_INPUT_ERROR    # the inner launcher's refusal (m != ctx.m)
    torch.cuda.synchronize()
    assert (J == 7.0).all()
    # ... and forward differences of the wrapped residual solve without the Jacobian launcher
    t2, y2, xt2, x02 = _family(4)
    dt2, dy2 = _dev(ds, t2), _dev(ds, y2)
    f2, j2, c2 = ds.curve_launchers(KIND, K, B, dt2, dy2)
    q2 = ds.pois_launchers(nl.Poisson(), f2, None, c2, dy2)
    x2 = _dev(ds, x02)
    assert set(ds.lm_solve_batch_device(q2[0], q2[2], PC.M, x2, jac=None, opts=o)[2]) == {0}
    q2[2].close()
    wctx.close()
    # the model object
    md, inner = C.c_void_p(7), C.c_void_p()
    A, b = np.ones((1, 2, 2)), np.ones((1, 2))
    one = np.ones(8)
    assert ds.lib.nlh_dq_model_create(ds.h.ptr, 1, 2, 2, A.ctypes.data_as(dp), b.ctypes.data_as(dp), 0.5, C.byref(inner)) == 0
    assert ds.lib.nlh_pois_model_create(ds.h.ptr, inner, one.ctypes.data_as(dp), None, F, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    ds.lib.nlh_dq_model_destroy(inner)                                  # (a dense-quadratic model has no launchers to wrap)
    inner = C.c_void_p()
    y7 = np.ones((nprob, 7))
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, 1, 2, 0, nprob, 7, np.ones((nprob, 7)).ctypes.data_as(dp), 0, y7.ctypes.data_as(dp), None, 1,
                                         C.byref(inner)) == 0
    mc = lambda yy, ww, fl: ds.lib.nlh_pois_model_create(ds.h.ptr, inner, yy.ctypes.data_as(dp) if yy is not None else None,
                                                         ww.ctypes.data_as(dp) if ww is not None else None, fl, C.byref(md))
    neg, half = y7.copy(), y7.copy()
    neg[1, 3], half[0, 0] = -1.0, 0.5
    assert mc(None, None, F) == NL_INVALID_INPUT_ERROR and not md.value
    assert mc(y7, None, 0.0) == NL_INVALID_INPUT_ERROR and not md.value
    assert mc(y7, None, float("nan")) == NL_INVALID_INPUT_ERROR and not md.value
    assert mc(neg, None, F) == NL_INVALID_INPUT_ERROR and not md.value
    assert mc(y7, half, F) == NL_INVALID_INPUT_ERROR and not md.value
    wneg = y7.copy()
    wneg[1, 3] = 0.0
    assert mc(neg, wneg, F) == 0 and md.value                           # ... but not on a row the mask zeroes
    ds.lib.nlh_dq_model_destroy(md)
    assert mc(y7, y7, F) == 0 and md.value
    ds.lib.nlh_dq_model_destroy(md)
    ds.lib.nlh_dq_model_destroy(inner)
    with pytest.raises(ValueError):                                     # Python: a Poisson fit has no robust loss
        ds.curve_fit_batch("lorentz", dt, dy, dx, ncomp=2, baseline=0, loss=nl.Loss("huber", 0.1), stat=nl.Poisson())
    with pytest.raises(ValueError):
        ds.expr_fit_batch(e, dt, dy, dx, loss=nl.Loss("huber", 0.1), stat=nl.Poisson())


# ------------------------------------------------------------------------------------------------ 6. the library's log
def _ulps(got, ref):
    """|got - ref| in units of the float64 spacing at ref (ref: numpy.longdouble)."""
    r64 = np.abs(ref).astype(np.float64)
    return float((np.abs(got.astype(np.longdouble) - ref) / np.spacing(r64).astype(np.longdouble)).max())


@pytest.fixture(scope="module")
def log_probe():
    d = os.path.join(HERE, "device_pois")
    subprocess.check_call(["make", "-C", d, "-s"])
    probe = C.CDLL(os.path.join(d, "liblog_probe.so"))
    probe.probe_log.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return probe


def test_log_accuracy(ds, log_probe):
    """The error of the device library's log in ulp against numpy.longdouble at 2^18 arguments over [1e-12, 0.5] -- the
    arguments u of the e < -0.5 path --, spread evenly in the logarithm (tests/device_pois/log_probe.hip: the function alone,
    compiled with the library's flags by the fixture).  The restatement's U_LOG is this maximum rounded up to an integer, no
    more and no less."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is no wider than float64 here: nothing to measure against"
    npts = 1 << 18
    u = np.exp(np.random.default_rng(12).uniform(math.log(1e-12), math.log(0.5), npts))
    du = _dev(ds, u)
    out = torch.empty_like(du)
    assert log_probe.probe_log(torch.cuda.current_stream(ds.device).cuda_stream, npts, du.data_ptr(), out.data_ptr()) == 0
    torch.cuda.synchronize()
    worst = _ulps(out.cpu().numpy(), np.log(u.astype(np.longdouble)))
    print(f"poisson function accuracy log: {worst:.3f} ulp over [1e-12, 0.5] (table {PR.U_LOG})")
    assert math.ceil(worst) == PR.U_LOG, (worst, PR.U_LOG)
