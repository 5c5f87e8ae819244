"""GPU tests of the bin-integrated fits (include/nonlin_hip_bin.h: nlh_bin_*): the kernel through the wrapping launchers against
the numpy restatement (tests/bin_restatement.py), bit for bit, over a chosen list of bins, nodes, parameter counts, forms,
column splits, slicings and scales; zero-weight bins; how a NaN node spreads; nlh_bin_apply_batch; LM and bounded solves through
the wrappers against the CPU oracle, alone, inside a parameter map and inside a group; the one-call fits with bins= against the
launchers composed by hand; what the feature is for, end to end; the error returns."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bin_cases as BC
import bin_restatement as BR
import curve_cases as CC
import group_restatement as GR
import pmap_restatement as PM
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

FORMS = [None, "row", "flat"]               # None: the form m selects; a forced form that cannot hold m falls back to it
SCALES = ["shared", "per", None]
NL_INVALID_INPUT_ERROR, NL_ARRAY_SIZE_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NLH_ERR_BAD_HANDLE = 201, 202, 211, -3


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    """Bit for bit, the sign of zero included; NaN against NaN (its payload is the hardware's own)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


class _env:
    """Environment variables for the calls inside (the library reads NLH_BIN_* at every call); None: unset."""

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


def _inner(ds, n, rows, nprob, seed):
    """An exp-free inner model of n parameters on `rows` rows that returns model values -- bound with y = 0 and without
    weights --: the formula a*t (n = 1) or a Lorentzian model (n = 3, 9).  Returns (launchers, keep, x0)."""
    rng = np.random.default_rng(seed)
    dzero = torch.zeros((nprob, rows), dtype=torch.float64, device=ds.device)
    if n == 1:
        t = np.tile(np.linspace(-1.0, 1.0, rows) if rows > 1 else np.array([0.7]), (nprob, 1)) + rng.uniform(-0.1, 0.1, (nprob, rows)) / rows
        x0 = rng.uniform(0.5, 1.5, (nprob, 1))
        dt = _dev(ds, t)
        ex = nl.Expr("a*t", ("t",), ("a",))
        return ds.expr_launchers(ex, dt, dzero), (ex, dt, dzero), x0
    KK, BB = {3: (1, -1), 9: (2, 2)}[n]
    t, y, xt, x0 = CC.curve_problems("lorentz", KK, BB, rows, nprob=nprob, seed=seed, sigma=0.02)
    dt = _dev(ds, t)
    return ds.curve_launchers("lorentz", KK, BB, dt, dzero), (dt, dzero), x0


def _binned(m, Q, nprob, scale, seed):
    """(Binned, c, s): a transform of Q nodes on m bins whose device scale is s -- [m], [nprob, m] or None ("mean": the
    weights halved) -- made through the public constructor: bins 0 .. 2 s have half = s exactly."""
    rng = np.random.default_rng(seed)
    kw = dict(order=Q) if Q <= 8 else dict(rule=(np.linspace(-1.0, 1.0, Q), BC.rule(Q, seed)))
    if scale is None:
        b = nl.Binned(np.zeros(m), np.ones(m), mode="mean", **kw)
        return b, b.c, None
    s = rng.uniform(0.25, 4.0, m if scale == "shared" else (nprob, m))
    b = nl.Binned(np.zeros(s.shape), 2.0 * s, **kw)
    assert np.array_equal(_bits(b.scale.reshape(s.shape)), _bits(s)) and b.shared == (scale == "shared")
    return b, b.c, s


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("case", BC.LAUNCH_CASES, ids=BC.case_id)
def test_launchers_against_restatement(ds, case):
    """k_bin through the wrapping launchers: F and J of the restatement applied to what the inner launchers give for the same
    points, bit for bit (the sign of zero included) -- with and without dprob, a point list with repeated problems, the form m
    selects and both forced forms, the column split forced to 2 and to n, sliced (three slices or more) and unsliced, with
    weights (zeros and a -0.0 among them) and without, the scale shared, per problem and NULL."""
    m, Q, n = case
    nprob, qm = 5, Q * m
    (fcn, jac, ctx), keep, x0 = _inner(ds, n, qm, nprob, seed=1000 * n + m + Q)
    rng = np.random.default_rng(m * 31 + Q)
    y = rng.standard_normal((nprob, m))
    w = rng.uniform(0.5, 2.0, (nprob, m))
    w[rng.uniform(size=(nprob, m)) < 0.25] = 0.0
    w[:, -1] = 0.0
    w[0, 0] = -0.0
    dy, dw = _dev(ds, y), _dev(ds, w)
    shapes = [None, list(np.random.default_rng(3).integers(0, nprob, 9)) + [0, 0, nprob - 1]]
    raw = []
    for kk, plist in enumerate(shapes):
        rows = list(range(nprob)) if plist is None else [int(p) for p in plist]
        X = x0[rows] * (1.0 + (0.002 if kk else 0.0) * np.random.default_rng(kk).uniform(-1, 1, (len(rows), n)))
        raw.append((rows, X, _launch(ds, fcn, ctx, rows, X, qm), _launch(ds, jac, ctx, rows, X, qm, jac=True)))
    for scale in SCALES:
        bins, c, s = _binned(m, Q, nprob, scale, seed=m + 7 * Q)
        wrapped = {True: ds.bin_launchers(bins, fcn, jac, ctx, dy, dw), False: ds.bin_launchers(bins, fcn, jac, ctx, dy)}
        for kk, plist in enumerate(shapes):
            rows, X, rawF, rawJ = raw[kk]
            sq = s if scale != "per" else s[rows]
            plainF = BR.residual(rawF, y[rows], None, c, sq)
            plainJ = BR.jacobian(rawJ, None, c, sq)
            for weighted in (True, False):
                wq = w[rows] if weighted else None
                wantF = BR.weigh(plainF, wq)
                wantJ = BR.weigh(plainJ, wq[:, None, :] if weighted else None)
                wf, wj, wctx = wrapped[weighted]
                for form in FORMS:
                    for split, sliced in ((None, False), (2, False), (n, True)):
                        with _env(NLH_BIN_FORM=form, NLH_BIN_SPLIT=split, NLH_BIN_SCRATCH=2 * (8 * qm + 4) if sliced else None):
                            Fg = _launch(ds, wf, wctx, plist, X, m)
                        with _env(NLH_BIN_FORM=form, NLH_BIN_SPLIT=split, NLH_BIN_SCRATCH=2 * (8 * qm * n + 4) if sliced else None):
                            Jg = _launch(ds, wj, wctx, plist, X, m, jac=True)
                        what = (case, scale, kk, weighted, form, split, sliced)
                        assert _same(Fg, wantF), what
                        assert _same(Jg, wantJ), what
                if weighted:                                         # zero-weight bins: +0.0 by bit pattern
                    assert not _bits(Fg[wq == 0.0]).any() and not _bits(np.moveaxis(Jg, 1, 2)[wq == 0.0]).any()
        for v in wrapped.values():
            v[2].close()


@pytest.mark.parametrize("m,Q", [(1, 1), (64, 3), (129, 5), (300, 16), (1000, 2)])
def test_apply_against_reduce(ds, m, Q):
    """nlh_bin_apply_batch against the restatement's reduce: [nprob, Q m] and [nprob, ncol, Q m], every scale, every form, the
    split forced."""
    rng = np.random.default_rng(m + Q)
    nprob, ncol = 4, 5
    v = rng.standard_normal((nprob, ncol, Q * m))
    v[0, 0, 0], v[1, 2, Q * m - 1] = -0.0, 0.0
    for scale in SCALES:
        bins, c, s = _binned(m, Q, nprob, scale, seed=m)
        want3 = BR.jacobian(v, None, c, s)
        want2 = BR.reduce(v[:, 0], c, s)
        for form in FORMS:
            for split in (None, 2, ncol):
                with _env(NLH_BIN_FORM=form, NLH_BIN_SPLIT=split):
                    got3 = ds.bin_apply(bins, _dev(ds, v)).cpu().numpy()
                    got2 = ds.bin_apply(bins, _dev(ds, v[:, 0])).cpu().numpy()
                assert got3.shape == (nprob, ncol, m) and got2.shape == (nprob, m)
                assert _same(got3, want3) and _same(got2, want2), (scale, form, split)


def test_apply_refusals(ds):
    """nlh_bin_apply_batch: dout == dv, NULL arrays, bad shapes and a bad transform are refused, in the documented order."""
    nprob, ncol, m, Q = 3, 2, 10, 3
    bins, c, s = _binned(m, Q, nprob, "shared", 1)
    dv = _dev(ds, np.ones((nprob, ncol, Q * m)))
    out = torch.full((nprob, ncol, m), 7.0, dtype=torch.float64, device=ds.device)
    bn, dsc = ds._bin_struct(bins, nprob)

    def call(b=bn, nprob_=nprob, m_=m, ncol_=ncol, src=dv, dst=out, h=ds.h.ptr):
        return ds.lib.nlh_bin_apply_batch(h, C.byref(b) if b is not None else None, nprob_, m_, ncol_, src.data_ptr() if src is not None else None,
                                          dst.data_ptr() if dst is not None else None)
    bad0, bad17 = bins.struct(dsc.data_ptr(), 1), bins.struct(dsc.data_ptr(), 1)
    bad0.Q, bad17.Q = 0, 17
    assert call(h=None) == NLH_ERR_BAD_HANDLE
    for bad in (None, bad0, bad17):
        assert call(b=bad) == NL_INVALID_INPUT_ERROR
    assert call(m_=0) == NL_INVALID_INPUT_ERROR and call(ncol_=0) == NL_INVALID_INPUT_ERROR and call(nprob_=-1) == NL_INVALID_INPUT_ERROR
    assert call(m_=2 ** 30, src=None, dst=None) == NL_ARRAY_SIZE_ERROR               # Q m beyond 2^31 - 1, before the arrays are looked at
    assert call(dst=dv) == NL_INVALID_INPUT_ERROR and call(src=None) == NL_INVALID_INPUT_ERROR and call(dst=None) == NL_INVALID_INPUT_ERROR
    assert call(nprob_=0, src=None, dst=None) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert _same(out.cpu().numpy(), BR.jacobian(np.ones((nprob, ncol, Q * m)), None, c, s))
    with pytest.raises(ValueError):
        ds.bin_apply(bins, _dev(ds, np.ones((nprob, Q * m + 1))))


@pytest.mark.parametrize("m,Q", [(64, 3), (129, 5), (300, 2)])
def test_a_nan_node_reaches_its_bin_and_no_other(ds, m, Q):
    """bin_apply on columns with one NaN node: the bin that owns the node is NaN, every other output is bit-equal to the run
    without the NaN -- the first and the last node plane, the first, a middle and the last bin, every form."""
    rng = np.random.default_rng(m + Q)
    nprob, ncol = 3, 2
    bins, c, s = _binned(m, Q, nprob, "per", m)
    v = rng.standard_normal((nprob, ncol, Q * m))
    clean = ds.bin_apply(bins, _dev(ds, v)).cpu().numpy()
    assert _same(clean, BR.jacobian(v, None, c, s)) and np.isfinite(clean).all()
    for form in FORMS:
        for q in (0, Q - 1):
            for i in (0, m // 2, m - 1):
                vn = v.copy()
                vn[1, 0, q * m + i] = np.nan
                with _env(NLH_BIN_FORM=form):
                    got = ds.bin_apply(bins, _dev(ds, vn)).cpu().numpy()
                keep = np.ones((nprob, ncol, m), dtype=bool)
                keep[1, 0, i] = False
                assert np.isnan(got[1, 0, i]) and np.array_equal(_bits(got[keep]), _bits(clean[keep])), (form, q, i)


# ------------------------------------------------------------------------------------------------ 2. the oracle
KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
LK, LB, LM_, LN, ORDER = 1, 0, 64, 4, 3          # the spectrum: one Lorentzian on a constant, 64 bins, three nodes each


def _same_counts(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _line(ds, nprob, weighted, **kw):
    lo, hi, y, xt, x0 = BC.line_problems(LK, LB, LM_, nprob, order=ORDER, **kw)
    w = None
    if weighted:
        w = np.random.default_rng(6).uniform(0.5, 2.0, (nprob, LM_))
        w[:, [3, 40]] = 0.0
    bins = nl.Binned(lo, hi, order=ORDER)
    dtq, dy = ds.bin_nodes(bins, nprob), _dev(ds, y)
    dzero = torch.zeros_like(dtq)
    dw = _dev(ds, w) if weighted else None
    inner = ds.curve_launchers("lorentz", LK, LB, dtq, dzero)
    return lo, hi, y, w, xt, x0, inner, ds.bin_launchers(bins, inner[0], inner[1], inner[2], dy, dw), (bins, dtq, dzero, dy, dw)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
def test_solves_against_oracle(ds, oracle, analytic, bounded, weighted):
    """lm_solve / cls_solve of the oracle with the restated callbacks (the Lorentzian restatement at the nodes, then the
    restated transform) under default options, 24 binned spectra: status, x, fvec and every count identical."""
    nprob = 24
    lo, hi, y, w, xt, x0, inner, (wf, wj, wctx), keep = _line(ds, nprob, weighted)
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
        f, j = BC.line_callbacks(LK, LB, lo[p], hi[p], y[p], w[p] if weighted else None, analytic, order=ORDER)
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
    """The bin pair inside a parameter map (the baseline fixed at its true value) and inside a group (G = 4, the width
    shared): status, x, fvec and every count identical to the oracle's on the restated stacks."""
    nprob, G = 24, 4
    lo, hi, y, w, xt, x0, inner, (cf, cj, cctx), keep = _line(ds, nprob, False, shared=(2,), G=G)
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
        f0, j0 = BC.line_callbacks(LK, LB, lo[p], hi[p], y[p], None, True, order=ORDER)

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
        cbs = [BC.line_callbacks(LK, LB, lo[q], hi[q], y[q], None, True, order=ORDER) for q in range(p * G, (p + 1) * G)]

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


# ------------------------------------------------------------------------------------------------ 3. the one call
GAUSS = "a*exp(-0.5*((t-mu)/s)^2)"
H = BC.NOISY_H


def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


def _histograms(nprob):
    """nprob Poisson histograms of the study's Gaussian at h = 1.5 sigma, their bins and a start."""
    y = BC.noisy_histograms(H, nprob)
    x0 = np.tile(BC.truth(H) * BC.START + np.array([0.0, 0.1, 0.0]), (nprob, 1))
    return BC.edges(H), y, x0


def _by_hand(ds, model, bins, dy, dw, dx0, analytic, o, loss=None, stat=None, conv=None, lower=None, upper=None):
    """The one-call fit composed by hand from the launchers: the model on the nodes with a zero y, the bin pair with y (and
    the weights, unless conv or stat take them), conv, then the Poisson pair or the loss; solve, covariance (unscaled under the
    Poisson pair)."""
    nprob, m = dy.shape
    dtq = ds.bin_nodes(bins, nprob)
    dzero = torch.zeros((nprob, bins.Q * m), dtype=torch.float64, device=ds.device)
    inner = model(dtq, dzero)
    plain = conv is None and stat is None
    stack = [ds.bin_launchers(bins, inner[0], inner[1], inner[2], dy, dw if plain else None)]
    if conv is not None:
        stack.append(ds.conv_launchers(conv, *stack[-1], dy, None if stat is not None else dw))
    if stat is not None:
        stack.append(ds.pois_launchers(stat, *stack[-1], dy, dw))
    if loss is not None:
        stack.append(ds.loss_launchers(loss, *stack[-1], nprob=nprob))
    top = stack[-1]
    j = top[1] if analytic else None
    x = dx0.clone()
    if lower is not None:
        fvec, ibs, st = ds.cls_solve_batch_device(top[0], top[2], m, x, jac=j, opts=o, lower=lower, upper=upper)
    else:
        fvec, ibs, st = ds.lm_solve_batch_device(top[0], top[2], m, x, jac=j, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(top[0], top[2], m, x, jac=j, scaled=stat is None)
    for s_ in reversed(stack):
        s_[2].close()
    return x, fvec, sigma, cov, chi2, rank, ibs, st


COMBOS = ["plain", "weights", "loss", "pois", "pois+mask", "conv", "conv+weights", "conv+pois", "bounds", "bounds+pois"]


@pytest.mark.parametrize("combo", COMBOS)
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("model", ["curve", "formula"])
def test_one_call_fit_is_the_composition(ds, model, analytic, combo):
    """curve_fit_batch / expr_fit_batch with bins= = the launchers composed by hand, GPU against GPU and bit for bit in x and
    fvec, with counts and status -- alone, with weights, with a loss, with the Poisson deviance (masked bins of fvec are +0.0),
    behind a response, inside bounds.  Without weights sigma, cov, chi2 and rank are lm_covariance_batch_device's bits; with
    weights they follow the zero-weight rule (torch arithmetic: compared to 1e-12)."""
    nprob, m, n = 16, BC.M, 3
    e, y, x0 = _histograms(nprob)
    parts = combo.split("+")
    rng = np.random.default_rng(3)
    w = None
    if "weights" in parts or "loss" in parts:
        w = 1.0 / np.sqrt(np.maximum(y, 1.0))
        w[:, [0, m - 1]] = 0.0
    if "mask" in parts:
        w = (rng.uniform(size=y.shape) < 0.9).astype(np.float64)
        w[:, :2] = 0.0
    loss = nl.Loss("soft_l1", 3.0) if "loss" in parts else None
    stat = nl.Poisson() if "pois" in parts else None
    conv = nl.Convolve([0.25, 0.5, 0.25], origin=1, extend="hold") if "conv" in parts else None
    lower = upper = None
    if "bounds" in parts:                                               # the width held below its estimate: a bound that binds
        lower, upper = np.array([0.0, -5.0, 0.1]), np.array([1e6, 5.0, 1.0])
        x0 = np.clip(x0, lower, upper)
    bins = nl.Binned.edges(e, order=3)
    dy, dx0 = _dev(ds, y), _dev(ds, x0)
    dw = _dev(ds, w) if w is not None else None
    o = ds.options()
    ex = nl.Expr(GAUSS, ("t",), ("a", "mu", "s"))
    launchers = (lambda tq, z: ds.curve_launchers("gauss", 1, -1, tq, z)) if model == "curve" else (lambda tq, z: ds.expr_launchers(ex, tq, z))
    kw = dict(weights=dw, lower=lower, upper=upper, analytic=analytic, opts=o, loss=loss, stat=stat, conv=conv, bins=bins)
    got = ds.curve_fit_batch("gauss", None, dy, dx0, **kw) if model == "curve" else ds.expr_fit_batch(ex, None, dy, dx0, **kw)
    want = _by_hand(ds, launchers, bins, dy, dw, dx0, analytic, o, loss=loss, stat=stat, conv=conv, lower=lower, upper=upper)
    what = (model, analytic, combo)
    assert got[7] == want[7] and got[6] == want[6], what
    assert _eq(got[0], want[0]) and _eq(got[1], want[1]), what
    assert torch.equal(dx0, _dev(ds, x0))                               # x0 is not modified
    if "bounds" in parts:                                               # (a bounded solve may end with a status of its own: its
        bad = _dev(ds, np.array(want[7]) != 0)                          # errors are then NaN and its rank -1, as from _fit)
        assert torch.isnan(got[2][bad]).all() and torch.isnan(got[3][bad]).all() and torch.isnan(got[4][bad]).all() and (got[5][bad] == -1).all()
        for k in (2, 3, 4, 5):
            assert _eq(got[k][~bad], want[k][~bad]), (what, k)
        return
    assert set(want[7]) == {0}, (what, want[7])
    if w is None:
        for k in (2, 3, 4, 5):
            assert _eq(got[k], want[k]), (what, k)
    else:
        dof = (w != 0).sum(1) - n
        f = _dev(ds, (m - n) / dof)
        assert torch.allclose(got[4], want[4] * f, rtol=1e-12, atol=0) and torch.equal(got[5], want[5])
        cov = want[3] if stat is not None else want[3] * f[:, None, None]
        assert torch.allclose(got[3], cov, rtol=1e-12, atol=0)
        assert torch.allclose(got[2], torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2)), rtol=1e-12, atol=0)
    if "mask" in parts:
        fg = got[1].cpu().numpy()
        assert not _bits(fg[w == 0.0]).any() and (fg[w != 0.0] != 0.0).all()
    none = ds.curve_fit_batch("gauss", None, dy, dx0, covariance=False, opts=o, bins=bins)
    assert none[2] is None and none[3] is None and none[4] is None and none[5] is None


def test_one_call_refusals(ds):
    """bins= refuses pmap, group, sep, starts, x0=None and a t, with a ValueError that names the launcher route; bins of
    another size, of another number of variables and a problem without a degree of freedom."""
    nprob, m = 4, BC.M
    e, y, x0 = _histograms(nprob)
    dy, dx0 = _dev(ds, y), _dev(ds, x0)
    bins = nl.Binned.edges(e, order=2)
    ex = nl.Expr(GAUSS, ("t",), ("a", "mu", "s"))
    dt = _dev(ds, 0.5 * (e[1:] + e[:-1]))
    st = nl.Starts([1.0, -1.0, 0.5], [1e5, 1.0, 2.0])
    for kw in (dict(pmap=nl.ParamMap(3, fixed=(1,))), dict(group=nl.Group(3, shared=(2,), nsets=2)), dict(sep=nl.Separable(3, linear=(0,))),
               dict(starts=st, x0=None), dict(x0=None)):
        x0_ = kw.pop("x0", dx0)
        for call in (lambda: ds.curve_fit_batch("gauss", None, dy, x0_, bins=bins, **kw), lambda: ds.expr_fit_batch(ex, None, dy, x0_, bins=bins, **kw)):
            with pytest.raises(ValueError, match="bin_launchers"):
                call()
    for call in (lambda: ds.curve_fit_batch("gauss", dt, dy, dx0, bins=bins), lambda: ds.expr_fit_batch(ex, dt, dy, dx0, bins=bins)):
        with pytest.raises(ValueError, match="t=None"):
            call()
    with pytest.raises(ValueError):
        ds.curve_fit_batch("gauss", None, dy, dx0, bins=nl.Binned.edges(e[:-1]))                  # 23 bins, 24 columns
    with pytest.raises(ValueError):
        ds.curve_fit_batch("gauss", None, dy, dx0, bins=nl.Binned(np.zeros((3, m)), np.ones((3, m))))     # bins for 3 problems, 4 data sets
    with pytest.raises(ValueError):
        ds.curve_fit_batch("gauss", None, dy, dx0, bins=nl.Binned.pixels((e[:-1], e[1:]), (e[:-1], e[1:])))   # two variables
    with pytest.raises(ValueError):
        ds.expr_fit_batch(nl.Expr("a*x+b*y", ("x", "y"), ("a", "b")), None, dy, dx0[:, :2].contiguous(), bins=bins)
    w = np.ones((nprob, m))
    w[2, 3:] = 0.0                                                       # three bins left for three parameters
    with pytest.raises(ValueError, match="degree of freedom"):
        ds.curve_fit_batch("gauss", None, dy, dx0, weights=_dev(ds, w), bins=bins)
    with pytest.raises(ValueError):
        ds.curve_fit_batch("gauss", None, dy, dx0, loss=nl.Loss("huber", 1.0), stat=nl.Poisson(), bins=bins)
    with pytest.raises(ValueError):
        ds.bin_launchers(bins, None, None, None, _dev(ds, y[:, :5]))


# ------------------------------------------------------------------------------------------------ 4. end to end
def test_end_to_end_width_of_a_histogrammed_gaussian(ds):
    """What the feature is for, under the conditions of the study's table: 64 Gaussian histograms of 24 bins, h = 1.5 sigma,
    20,000 counts, Poisson deviance.  With bins=Binned(order=3) the mean of sigma-hat / sigma is within 0.01 of 1 (expected:
    about 1e-4 bias plus 6e-4 scatter of the mean); with the centre value times the bin width it is above 1.05 (expected:
    1.09)."""
    nprob = 64
    e, y, x0 = _histograms(nprob)
    dy, dx0 = _dev(ds, y), _dev(ds, x0)
    stat = nl.Poisson()
    binned = ds.curve_fit_batch("gauss", None, dy, dx0, stat=stat, bins=nl.Binned.edges(e, order=3))
    centre = ds.expr_fit_batch(nl.Expr(f"{H!r}*a*exp(-0.5*((t-mu)/s)^2)", ("t",), ("a", "mu", "s")), _dev(ds, 0.5 * (e[:-1] + e[1:])), dy, dx0, stat=stat)
    assert set(binned[7]) == {0} and set(centre[7]) == {0}
    sb, sc = binned[0][:, 2].cpu().numpy(), centre[0][:, 2].cpu().numpy()
    print(f"binned Gaussians, h = {H} sigma: order 3 sigma-hat/sigma {sb.mean():.5f} +- {sb.std(ddof=1) / np.sqrt(nprob):.5f}, "
          f"centre x width {sc.mean():.5f} +- {sc.std(ddof=1) / np.sqrt(nprob):.5f}")
    assert abs(sb.mean() - 1.0) <= 0.01
    assert sc.mean() > 1.05
    # the area comes back too: a sigma sqrt(2 pi) within 3 % of the counts
    area = (binned[0][:, 0] * binned[0][:, 2]).cpu().numpy() * np.sqrt(2 * np.pi)
    assert abs(area.mean() / BC.COUNTS - 1.0) <= 0.03
    # the centre fit is order 1 of the binned path -- the same function up to rounding --: the same width to what the solver's
    # stop leaves, a relative cost change below ftol = 1e-8, so sqrt(1e-8) of the width's statistical error 6e-3 per fit, twice
    # 6e-7; a decade above that
    one = ds.curve_fit_batch("gauss", None, dy, dx0, stat=stat, bins=nl.Binned.edges(e, order=1))
    assert set(one[7]) == {0} and np.abs(one[0][:, 2].cpu().numpy() - sc).max() <= 1e-5


def test_pixels_end_to_end(ds):
    """A formula of two variables averaged over the pixels of an image: a round Gaussian spot of width 0.8 pixels on 9 x 9
    pixels, noise-free data from the 4 x 4 rule in numpy; the 3 x 3 rule on the device recovers the width to 1e-3, the centre
    value does not (it is wider by more than 3 %)."""
    K = 9
    gx, gy = np.meshgrid(np.arange(K, dtype=np.float64), np.arange(K, dtype=np.float64), indexing="ij")
    xlo, ylo = gx.reshape(-1), gy.reshape(-1)
    truth = np.array([100.0, 4.3, 3.8, 0.8, 2.0])
    ref = nl.Binned.pixels((xlo, xlo + 1), (ylo, ylo + 1), order=4, mode="mean")
    tx, ty = ref.nodes()
    spot = lambda a, x0, y0, s, b, X, Y: b + a * np.exp(-((X - x0) ** 2 + (Y - y0) ** 2) / (2 * s * s))
    y = BR.reduce(spot(*truth, tx, ty), ref.c)[None, :]
    ex = nl.Expr("b + a*exp(-((x-x0)^2+(y-y0)^2)/(2*s^2))", ("x", "y"), ("a", "x0", "y0", "s", "b"))
    dy, dx0 = _dev(ds, y), _dev(ds, (truth * np.array([0.9, 1.02, 0.98, 1.2, 1.1]))[None, :])
    px = nl.Binned.pixels((xlo, xlo + 1), (ylo, ylo + 1), order=3, mode="mean")
    fit = ds.expr_fit_batch(ex, None, dy, dx0, bins=px)
    centre = ds.expr_fit_batch(ex, _dev(ds, np.stack([xlo + 0.5, ylo + 0.5])), dy, dx0)
    assert fit[7] == [0] and centre[7] == [0]
    sb, sc = float(fit[0][0, 3]), float(centre[0][0, 3])
    print(f"pixels: width {sb:.6f} with the 3 x 3 rule, {sc:.6f} with the centre value, truth {truth[3]}")
    assert abs(sb / truth[3] - 1.0) <= 1e-3 and sc / truth[3] > 1.03
    # the binned model for plotting: expr_eval at the nodes, then bin_apply -- fvec of an unweighted fit is that minus y
    shown = ds.bin_apply(px, ds.expr_eval(ex, fit[0], ds.bin_nodes(px, 1)))
    assert _eq(shown - dy, fit[1])


# ------------------------------------------------------------------------------------------------ 5. error returns
def test_error_returns(ds):
    """nlh_bin_wrap and the launchers, in the documented order; nothing is written where a call is refused."""
    m, nprob, Q = 6, 2, 3
    bins, c, s = _binned(m, Q, nprob, "shared", 5)
    (fcn, jac, ctx), keep, x0 = _inner(ds, 3, Q * m, nprob, seed=9)
    dy, dx = _dev(ds, np.zeros((nprob, m))), _dev(ds, x0)
    bn, dsc = ds._bin_struct(bins, nprob)
    bad0, bad17 = bins.struct(dsc.data_ptr(), 1), bins.struct(dsc.data_ptr(), 1)
    bad0.Q, bad17.Q = 0, 17
    out = C.c_void_p(7)
    none = C.cast(None, _lib.DEVFCN)
    wrap = lambda h, b, yy, ff: ds.lib.nlh_bin_wrap(h, C.byref(b) if b is not None else None, yy, None, ff, jac, ds._ctxp(ctx), C.byref(out))
    assert wrap(None, bn, dy.data_ptr(), fcn) == NLH_ERR_BAD_HANDLE and not out.value
    assert wrap(ds.h.ptr, bn, None, fcn) == NL_INVALID_INPUT_ERROR and not out.value
    for bad in (None, bad0, bad17):
        assert wrap(ds.h.ptr, bad, dy.data_ptr(), fcn) == NL_INVALID_INPUT_ERROR and not out.value
    assert ds.lib.nlh_bin_wrap(ds.h.ptr, C.byref(bn), dy.data_ptr(), None, fcn, jac, ds._ctxp(ctx), None) == NL_INVALID_INPUT_ERROR
    assert wrap(ds.h.ptr, bn, dy.data_ptr(), none) == NL_UNDEFINED_FUNCTION_ERROR and not out.value
    nos = bins.struct(None, 1)                                           # a NULL scale is a transform without one
    assert wrap(ds.h.ptr, nos, dy.data_ptr(), fcn) == 0 and out.value
    ds.lib.nlh_bin_unwrap(out)
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    J = torch.full((nprob, 3, m), 7.0, dtype=torch.float64, device=ds.device)
    lst = _dev(ds, [0, 1], np.int32)
    wf, wj, wctx = ds.bin_launchers(bins, fcn, None, ctx, dy)
    assert wj is None
    args = lambda n_, m_, np_=nprob, x=dx, o=J: (wctx.ptr, stream, np_, lst.data_ptr(), n_, x.data_ptr() if x is not None else None, m_,
                                                 o.data_ptr() if o is not None else None)
    assert ds.lib.nlh_bin_device_fcn(*args(0, m)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_bin_device_fcn(*args(3, 0)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_bin_device_fcn(*args(3, m, x=None)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_bin_device_fcn(*args(3, m, o=None)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_bin_device_jac(*args(3, m)) == NL_UNDEFINED_FUNCTION_ERROR    # no inner Jacobian launcher
    assert ds.lib.nlh_bin_device_fcn(*args(3, m, np_=0)) == 0                       # no points
    assert ds.lib.nlh_bin_device_fcn(*args(3, 2 ** 30)) == NL_ARRAY_SIZE_ERROR       # Q m beyond 2^31 - 1
    assert ds.lib.nlh_bin_device_fcn(*args(3, m + 1)) == NL_INVALID_INPUT_ERROR     # the inner launcher's refusal (Q (m + 1) != ctx.m)
    torch.cuda.synchronize()
    assert (J == 7.0).all()
    assert ds.lib.nlh_bin_device_fcn(*args(3, m)) == 0
    torch.cuda.synchronize()
    assert (J.reshape(-1)[:nprob * m] != 7.0).all()
    wctx.close()
