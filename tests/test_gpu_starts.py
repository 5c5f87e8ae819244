"""GPU tests of starts (include/nonlin_hip_starts.h: nlh_starts_*).  Everything is bit for bit against tests/starts_restatement.py:
the scan's cost and selection are restated from the residuals the device's own launcher gives at the same points, so the file
uses no tolerance."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import starts_cases as SC
import starts_restatement as S
from nonlin_amd import _lib, Starts, Expr, Loss, Poisson, Convolve, Separable

pytestmark = pytest.mark.gpu

NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3
FORMULA = ("a*exp(-k*t)+c*sin(w*t)", ("t",), ("a", "k", "c", "w"))
BOX4 = dict(lower=(0.5, 0.05, -2.0, 0.5), upper=(5.0, 3.0, 2.0, 9.0), log=(1,))


def _dev(ds, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ds.device)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what=""):
    assert np.array_equal(_bits(got), _bits(want)), what


def _data(nprob, m, shared, weighted, seed):
    """t on (0, 4] ([m] or per problem), y of the formula's family with noise, weights with zeros among them or None."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.1, 4.0, m) if shared else np.sort(rng.uniform(0.1, 4.0, (nprob, m)), axis=1)
    x = np.stack([rng.uniform(1, 4, nprob), rng.uniform(0.2, 2, nprob), rng.uniform(-1, 1, nprob), rng.uniform(1, 8, nprob)], axis=1)
    tt = np.broadcast_to(t, (nprob, m))
    y = x[:, 0:1] * np.exp(-x[:, 1:2] * tt) + x[:, 2:3] * np.sin(x[:, 3:4] * tt) + 0.05 * rng.standard_normal((nprob, m))
    w = np.where(rng.random((nprob, m)) < 0.1, 0.0, rng.uniform(0.5, 2.0, (nprob, m))) if weighted else None
    return t, y, w


def _launchers(ds, model, t, y, w):
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w) if w is not None else None
    if model == "expr":
        return ds.expr_launchers(Expr(*FORMULA), dt, dy, dw)
    return ds.curve_launchers("gauss", 1, 0, dt, dy, dw)


def _evaluate(ds, fcn, ctx, nprob, m, table):
    """F [nprob * ncand, m] of every candidate of every problem through the launcher itself, problem-major."""
    ncand, n = table.shape
    X = _dev(ds, np.tile(table, (nprob, 1)))
    prob = _dev(ds, np.repeat(np.arange(nprob), ncand), np.int32)
    F = torch.empty((nprob * ncand, m), dtype=torch.float64, device=ds.device)
    stream = torch.cuda.current_stream(ds.device).cuda_stream
    rc = ds._devfcn(fcn)(ds._ctxp(ctx), C.c_void_p(stream) if stream else None, nprob * ncand, prob.data_ptr(), n, X.data_ptr(), m, F.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return F.cpu().numpy()


def _expected(ds, fcn, ctx, nprob, m, starts, positions=None):
    table = starts.candidates(positions=positions)
    F = _evaluate(ds, fcn, ctx, nprob, m, table)
    return S.search(S.cost(F).reshape(nprob, starts.ncand), table, starts.keep)


def _check_search(ds, fcn, ctx, nprob, m, starts, positions=None):
    x0, cost, index = ds.starts_search(fcn, ctx, nprob, m, starts, positions)
    torch.cuda.synchronize()
    wx, wc, wi = _expected(ds, fcn, ctx, nprob, m, starts, positions)
    assert np.array_equal(index.cpu().numpy(), wi)
    _same(cost, wc, "cost")
    _same(x0, wx, "x0")
    return x0.cpu().numpy(), cost.cpu().numpy(), index.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# the cost kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 127, 128, 129, 4097])
def test_cost_at_the_size_edges(ds, m):
    """Every row count at which a lane gains or loses a row or the unrolled loop gains a step, with 1 .. 5 points (the last
    workgroup partial) and 1025; rows holding NaN, +-Inf and -0.0 among them."""
    rng = np.random.default_rng(m)
    for npoints in (1, 3, 4, 5, 1025):
        F = rng.standard_normal((npoints, m)) * 10.0 ** rng.integers(-4, 4, (npoints, m))
        F[0, 0] = -0.0
        if npoints >= 3:
            F[1, rng.integers(0, m)] = np.nan
            F[2, rng.integers(0, m)] = np.inf
        if npoints >= 5:
            F[4, rng.integers(0, m)] = -np.inf
            F[3, :] = -0.0
        got = ds.starts_cost(_dev(ds, F))
        torch.cuda.synchronize()
        _same(got, S.cost(F), (m, npoints))


# ---------------------------------------------------------------------------------------------------------------------
# the scan
# ---------------------------------------------------------------------------------------------------------------------
SEARCH_CASES = [  # model, nprob, m, ncand, keep, shared t, weights
    ("expr", 1, 4, 1, 1, True, False), ("expr", 3, 4, 8, 2, False, True), ("expr", 3, 513, 9, 8, True, True),
    ("expr", 1, 513, 63, 8, False, False), ("expr", 3, 4, 64, 1, True, False), ("expr", 700, 4, 65, 2, False, True),
    ("expr", 3, 513, 257, 8, False, True), ("curve", 1, 513, 8, 8, True, True), ("curve", 3, 4, 9, 1, False, False),
    ("curve", 700, 4, 63, 8, True, False), ("curve", 3, 4, 64, 2, False, True), ("curve", 1, 4, 65, 1, True, True),
    ("curve", 3, 513, 257, 2, True, False), ("curve", 3, 4, 1, 1, False, True),
]


@pytest.mark.parametrize("model,nprob,m,ncand,keep,shared,weighted", SEARCH_CASES)
def test_search_against_the_restatement(ds, model, nprob, m, ncand, keep, shared, weighted):
    t, y, w = _data(nprob, m, shared, weighted, seed=nprob + m + ncand)
    fcn, _, ctx = _launchers(ds, model, t, y, w)
    _, cost, index = _check_search(ds, fcn, ctx, nprob, m, Starts(**BOX4, ncand=ncand, keep=keep))
    assert (index >= 0).all() and np.isfinite(cost).all() and (np.diff(cost, axis=1) >= 0).all()


def test_search_of_a_subset_of_the_box(ds):
    """positions: the scan runs over the launcher's unknowns alone -- here the nonlinear ones of a separable formula."""
    nprob, m = 3, 65
    t, y, w = _data(nprob, m, True, True, seed=9)
    e = Expr(*FORMULA)
    sep = Separable.for_expr(e, linear=("a", "c"))
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y), _dev(ds, w))
    sf, _, sc = ds.sep_launchers(sep, fcn, jac, ctx)
    pos = [int(k) for k in sep.tables()[1]]
    assert pos == [1, 3]
    x0, _, _ = _check_search(ds, sf, sc, nprob, m, Starts(**BOX4, ncand=65, keep=2), positions=pos)
    assert x0.shape == (nprob, 2, 2)


@pytest.mark.parametrize("nprob,ncand,keep", [(5, 65, 2), (3, 9, 8)])
def test_chunks_and_slices_do_not_change_the_bits(ds, monkeypatch, nprob, ncand, keep):
    """NLH_STARTS_POINTS: one point per launcher call, `keep` points, a chunk that does not divide the candidates, one problem's
    worth + 1 (slices of one problem), and a value that puts two problems in a slice and leaves a last slice of one."""
    m = 33
    t, y, w = _data(nprob, m, False, True, seed=ncand)
    fcn, _, ctx = _launchers(ds, "expr", t, y, w)
    st = Starts(**BOX4, ncand=ncand, keep=keep)
    monkeypatch.delenv("NLH_STARTS_POINTS", raising=False)
    ref = _check_search(ds, fcn, ctx, nprob, m, st)
    for points in (1, keep, 7, ncand + 1, 2 * ncand + 3):
        monkeypatch.setenv("NLH_STARTS_POINTS", str(points))
        got = ds.starts_search(fcn, ctx, nprob, m, st)
        torch.cuda.synchronize()
        for g, r, name in zip(got, ref, ("x0", "cost", "index")):
            _same(g.to(torch.float64), r.astype(np.float64), (points, name))


@pytest.mark.parametrize("model", ["expr", "curve"])
def test_a_problem_does_not_depend_on_its_batch(ds, model):
    nprob, m = 700, 19
    t, y, w = _data(nprob, m, False, True, seed=77)
    st = Starts(**BOX4, ncand=65, keep=8)
    fcn, _, ctx = _launchers(ds, model, t, y, w)
    x0, cost, index = (a.cpu().numpy() for a in ds.starts_search(fcn, ctx, nprob, m, st))
    for p in (0, 350, 699):
        f1, _, c1 = _launchers(ds, model, t[p:p + 1], y[p:p + 1], w[p:p + 1])
        a, b, c = ds.starts_search(f1, c1, 1, m, st)
        _same(a[0], x0[p]); _same(b[0], cost[p])
        assert np.array_equal(c[0].cpu().numpy(), index[p])


def test_ties_keep_the_lowest_indices(ds):
    e = Expr("0*a+1", ("t",), ("a",))
    nprob, m = 3, 70
    t, y, _ = _data(nprob, m, True, False, seed=1)
    fcn, _, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    for ncand, keep in ((8, 8), (300, 5), (65, 1)):
        _, cost, index = _check_search(ds, fcn, ctx, nprob, m, Starts((0.0,), (1.0,), ncand=ncand, keep=keep))
        assert (index == np.arange(keep)[None, :]).all() and (cost == cost[:, :1]).all()


def test_costs_that_are_not_finite_are_never_kept(ds):
    """log(a*t) with per-problem t = +1 or -1.  A box across 0: problem 0 sees NaN at every a < 0 and -Inf at a = 0 (candidate
    0, the centre), problem 1 the mirror image; only finite costs come back.  A box wholly below 0: problem 0 has nothing
    finite -- index -1, cost +Inf, rows of NaN -- and its neighbour, for whom every a*t is positive, is what it is alone."""
    e = Expr("log(a*t)", ("t",), ("a",))
    m = 5
    t = np.stack([np.ones(m), -np.ones(m), np.ones(m)])
    y = np.zeros((3, m))
    fcn, _, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    across = Starts((-2.0,), (2.0,), ncand=64, keep=8)
    x0, cost, index = _check_search(ds, fcn, ctx, 3, m, across)
    assert np.isfinite(cost).all() and (index > 0).all()
    assert (x0[0] > 0).all() and (x0[1] < 0).all() and (x0[2] > 0).all()
    few = Starts((-2.0,), (2.0,), ncand=9, keep=8)                              # fewer finite costs than keep: the rest is empty
    x0, cost, index = _check_search(ds, fcn, ctx, 3, m, few)
    nfin = (few.candidates()[:, 0] > 0).sum()
    assert 0 < nfin < 8 and (index[0, nfin:] == -1).all() and np.isposinf(cost[0, nfin:]).all() and np.isnan(x0[0, nfin:]).all()
    below = Starts((-3.0,), (-1.0,), ncand=65, keep=2)
    x0, cost, index = _check_search(ds, fcn, ctx, 3, m, below)
    for p in (0, 2):
        assert (index[p] == -1).all() and np.isposinf(cost[p]).all() and np.isnan(x0[p]).all()
    assert (index[1] >= 0).all() and np.isfinite(cost[1]).all()
    f1, _, c1 = ds.expr_launchers(e, _dev(ds, t[1:2]), _dev(ds, y[1:2]))
    a, b, c = ds.starts_search(f1, c1, 1, m, below)
    _same(a[0], x0[1]); _same(b[0], cost[1])
    assert np.array_equal(c[0].cpu().numpy(), index[1])


def test_the_host_array_twin(ds):
    nprob, m, st = 3, 33, Starts(**BOX4, ncand=65, keep=2)
    t, y, w = _data(nprob, m, True, False, seed=4)
    fcn, _, ctx = _launchers(ds, "expr", t, y, w)
    want = _check_search(ds, fcn, ctx, nprob, m, st)
    x0, cost, index = np.empty((nprob, 2, 4)), np.empty((nprob, 2)), np.empty((nprob, 2), dtype=np.int32)
    lo, hi, lg = st.box()
    rc = ds.lib.nlh_starts_search_batch_device_h(ds.h.ptr, nprob, m, 4, ds._devfcn(fcn), ds._ctxp(ctx), lo.ctypes.data_as(_lib.c_double_p),
                                                 hi.ctypes.data_as(_lib.c_double_p), lg.ctypes.data_as(_lib.c_int32_p), 65, 2,
                                                 x0.ctypes.data_as(_lib.c_double_p), cost.ctypes.data_as(_lib.c_double_p),
                                                 index.ctypes.data_as(_lib.c_int32_p))
    assert rc == 0
    _same(x0, want[0]); _same(cost, want[1])
    assert np.array_equal(index, want[2])


# ---------------------------------------------------------------------------------------------------------------------
# pick and take
# ---------------------------------------------------------------------------------------------------------------------
def test_pick_and_take(ds):
    rng = np.random.default_rng(6)
    for keep, nprob, n in ((1, 5, 3), (2, 300, 4), (8, 1025, 5)):
        c = rng.integers(0, 4, (keep, nprob)).astype(np.float64)                # ties
        c[rng.random((keep, nprob)) < 0.3] = np.nan
        c[rng.random((keep, nprob)) < 0.1] = np.inf
        c[:, 1] = np.nan                                                        # a column with nothing finite
        c[:, 2] = 1.0                                                           # a column that is one tie
        which = ds.starts_pick(_dev(ds, c))
        want = S.pick(c)
        assert np.array_equal(which.cpu().numpy(), want) and want[1] == -1 and want[2] == 0
        for shape in ((), (1,), (n, n)):                                        # widths 1 and n*n
            src = rng.standard_normal((keep, nprob) + shape)
            got = ds.starts_take(_dev(ds, src), which)
            _same(got, S.take(src, want), (keep, shape))
            assert got.shape == (nprob,) + shape and np.isnan(got[1].cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------
# the one-call fits
# ---------------------------------------------------------------------------------------------------------------------
DECAY = ("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
DECAY_BOX = dict(lower=(1.0, 0.05, 0.0), upper=(200.0, 5.0, 20.0), log=(0, 1))


def _decay_data(seed, counts=False):
    rng = np.random.default_rng(seed)
    nprob, m = 8, 64
    t = np.arange(m) * 0.125
    x = np.stack([rng.uniform(40, 80, nprob), rng.uniform(0.5, 2.0, nprob), rng.uniform(2, 6, nprob)], axis=1)
    mu = x[:, 0:1] * np.exp(-x[:, 1:2] * t[None, :]) + x[:, 2:3]
    y = rng.poisson(mu).astype(np.float64) if counts else mu + rng.standard_normal((nprob, m))
    w = np.where(rng.random((nprob, m)) < 0.1, 0.0, 1.0)
    return t, y, w


def _by_hand(ds, model_launchers, fit, n, m, y, w, st, loss=None, stat=None, conv=None, sep=None):
    """The composition the one-call form documents, through the public pieces."""
    nprob = y.shape[0]
    layers = [model_launchers(None if conv is not None or stat is not None else w)]
    if conv is not None:
        layers.append(ds.conv_launchers(conv, *layers[-1], y, None if stat is not None else w))
    if stat is not None:
        layers.append(ds.pois_launchers(stat, *layers[-1], y, w))
    if loss is not None:
        layers.append(ds.loss_launchers(loss, *layers[-1], nprob))
    pos = None
    if sep is not None:
        layers.append(ds.sep_launchers(sep, *layers[-1]))
        pos = [int(k) for k in sep.tables()[1]]
    x0s, cost, index = ds.starts_search(layers[-1][0], layers[-1][2], nprob, m, st, pos)
    runs = []
    for k in range(st.keep):
        x0 = x0s[:, k].contiguous()
        if pos is not None:
            x0 = torch.zeros((nprob, n), dtype=torch.float64, device=ds.device)
            x0[:, pos] = x0s[:, k]
        runs.append(fit(x0))
    which = ds.starts_pick(torch.stack([ds.starts_cost(r[1]) for r in runs]))
    out = [ds.starts_take(torch.stack([r[j] for r in runs]), which) for j in range(5)]
    rank = torch.stack([r[5] for r in runs]).cpu().numpy()
    wh = which.cpu().numpy()
    out.append(np.where(wh < 0, -1, rank[np.maximum(wh, 0), np.arange(nprob)]))
    out.append([runs[max(k, 0)][6][p] for p, k in enumerate(wh)])
    out.append([runs[max(k, 0)][7][p] for p, k in enumerate(wh)])
    return out, which, index, cost


def _compare(got, st, hand):
    want, which, index, cost = hand
    for j, name in enumerate(("x", "fvec", "sigma", "cov", "chi2")):
        _same(got[j], want[j], name)
    assert np.array_equal(got[5].cpu().numpy(), want[5]) and got[5].dtype == torch.int32
    assert got[6] == want[6] and got[7] == want[7]
    assert np.array_equal(st.which.cpu().numpy(), which.cpu().numpy())
    assert np.array_equal(st.index.cpu().numpy(), index.cpu().numpy())
    _same(st.cost, cost)
    assert np.isfinite(got[0].cpu().numpy()).all()


@pytest.mark.parametrize("variant", ["plain", "loss", "stat", "conv", "sep"])
def test_expr_fit_with_starts_is_the_composition(ds, variant):
    e = Expr(*DECAY)
    t, y, w = _decay_data(31, counts=variant == "stat")
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    kw = {"plain": {}, "loss": dict(loss=Loss("huber", 2.0)), "stat": dict(stat=Poisson()),
          "conv": dict(conv=Convolve([0.2, 0.5, 0.3], origin=0, extend="hold")),
          "sep": dict(sep=Separable.for_expr(e, linear=("a", "c")))}[variant]
    st = Starts.for_expr(e, lower=dict(zip(e.params.split(","), DECAY_BOX["lower"])), upper=dict(zip(e.params.split(","), DECAY_BOX["upper"])),
                         ncand=64, keep=2, log=("a", "k"))
    got = ds.expr_fit_batch(e, dt, dy, None, weights=dw, starts=st, **kw)
    hand = _by_hand(ds, lambda ww: ds.expr_launchers(e, dt, dy, ww), lambda x0: ds.expr_fit_batch(e, dt, dy, x0, weights=dw, **kw), 3, len(t), dy, dw,
                    Starts(**DECAY_BOX, ncand=64, keep=2), **kw)
    _compare(got, st, hand)
    assert all(s == 0 for s in got[7])


@pytest.mark.parametrize("variant", ["plain", "sep"])
def test_curve_fit_with_starts_is_the_composition(ds, variant):
    t, y, w = _decay_data(32)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    kw = dict(sep=Separable.for_curve("expdecay", 1, 0)) if variant == "sep" else {}
    st = Starts(**DECAY_BOX, ncand=64, keep=2)
    got = ds.curve_fit_batch("expdecay", dt, dy, None, ncomp=1, baseline=0, weights=dw, starts=st, **kw)
    hand = _by_hand(ds, lambda ww: ds.curve_launchers("expdecay", 1, 0, dt, dy, ww),
                    lambda x0: ds.curve_fit_batch("expdecay", dt, dy, x0, ncomp=1, baseline=0, weights=dw, **kw), 3, len(t), dy, dw,
                    Starts(**DECAY_BOX, ncand=64, keep=2), **kw)
    _compare(got, st, hand)
    nocov = ds.curve_fit_batch("expdecay", dt, dy, None, ncomp=1, baseline=0, weights=dw, starts=st, covariance=False, **kw)
    _same(nocov[0], got[0]); _same(nocov[1], got[1])
    assert nocov[2] is nocov[3] is nocov[4] is nocov[5] is None


def test_fit_refusals(ds):
    from nonlin_amd import ParamMap
    e = Expr(*DECAY)
    t, y, w = _decay_data(33)
    dt, dy = _dev(ds, t), _dev(ds, y)
    st = Starts(**DECAY_BOX)
    x0 = torch.ones((8, 3), dtype=torch.float64, device=ds.device)
    with pytest.raises(ValueError, match="starts excludes x0"):
        ds.expr_fit_batch(e, dt, dy, x0, starts=st)
    with pytest.raises(ValueError, match="starts excludes x0"):
        ds.curve_fit_batch("expdecay", dt, dy, x0, baseline=0, starts=st)
    with pytest.raises(ValueError, match="starts excludes pmap and group"):
        ds.expr_fit_batch(e, dt, dy, None, pmap=ParamMap(3, fixed=[2]), starts=st)
    with pytest.raises(ValueError, match="a box over 2 parameters, the model has 3"):
        ds.curve_fit_batch("expdecay", dt, dy, None, baseline=0, starts=Starts((0.0, 0.0), (1.0, 1.0)))


def test_the_study_s_first_problems_on_the_device(ds):
    """The first 8 problems of the sinusoid study, a, b, c projected out and 64 candidates of w scanned, at full size: the
    problems that end within 1.05 x the cost at the truth are the ones tests/golden/starts_study.json records for these 8."""
    rec = json.load(open(SC.STUDY_GOLDEN))
    t, y, xt = SC.problems(8)
    e = Expr(SC.SEP_FORMULA, ("t",), SC.SEP_PARAMS)
    st = Starts.for_expr(e, lower=dict(a=-10.0, w=SC.SEP_LOWER[0], b=-10.0, c=-10.0), upper=dict(a=10.0, w=SC.SEP_UPPER[0], b=10.0, c=10.0),
                         ncand=64, keep=1)
    x, fvec, *_ = ds.expr_fit_batch(e, _dev(ds, t), _dev(ds, y), None, sep=Separable.for_expr(e, linear=("a", "b", "c")), starts=st,
                                    opts=ds.options(max_evals=SC.MAX_EVALS))
    fv = fvec.cpu().numpy()
    cost = np.sum(fv ** 2, axis=1)
    cap = 1.05 * SC.truth_cost(t, y, xt)
    print("cost / cost at the truth:", cost / (cap / 1.05))
    reached = "".join(str(int(np.isfinite(fv[p]).all() and cost[p] <= cap[p])) for p in range(8))
    assert reached == rec["problems"]["sep_64"][:8]


# ---------------------------------------------------------------------------------------------------------------------
# error returns
# ---------------------------------------------------------------------------------------------------------------------
def test_error_returns_with_a_real_handle(ds):
    """In the header's order, writing nothing: canary-filled outputs stay what they were."""
    nprob, m, n = 2, 16, 4
    t, y, w = _data(nprob, m, True, False, seed=2)
    fcn, _, ctx = _launchers(ds, "expr", t, y, w)
    x0 = torch.full((nprob, 8, n), 7.0, dtype=torch.float64, device=ds.device)
    cost = torch.full((nprob, 8), 7.0, dtype=torch.float64, device=ds.device)
    index = torch.full((nprob, 8), 7, dtype=torch.int32, device=ds.device)
    lo, hi, lg = (np.array(BOX4["lower"]), np.array(BOX4["upper"]), np.array([0, 1, 0, 0], dtype=np.int32))
    dp, ip = lambda a: a.ctypes.data_as(_lib.c_double_p) if a is not None else None, lambda a: a.ctypes.data_as(_lib.c_int32_p)
    none = C.cast(None, _lib.DEVFCN)

    def call(h=ds.h.ptr, nprob=nprob, m=m, n=n, f=ds._devfcn(fcn), xl=lo, xu=hi, ls=lg, ncand=16, keep=2, out=(x0, cost, index)):
        return ds.lib.nlh_starts_search_batch_device(h, nprob, m, n, f, ds._ctxp(ctx), dp(xl), dp(xu), ip(ls), ncand, keep,
                                                     *[o.data_ptr() if o is not None else None for o in out])
    assert call(h=None) == NLH_ERR_BAD_HANDLE
    assert call(h=None, f=none, keep=0) == NLH_ERR_BAD_HANDLE
    bad_lo, log_lo = lo.copy(), lo.copy()
    bad_lo[2] = 3.0                                                             # lo > hi
    log_lo[1] = 0.0                                                             # a log dimension from 0
    for bad in (dict(f=none), dict(xl=None), dict(xu=None), dict(nprob=-1), dict(m=0), dict(n=0), dict(n=33), dict(ncand=0),
                dict(ncand=S.MAX_CAND + 1), dict(keep=0), dict(keep=9), dict(ncand=4, keep=5), dict(xl=bad_lo), dict(xl=log_lo),
                dict(xu=np.array([5.0, 3.0, np.inf, 9.0])), dict(out=(None, cost, index)), dict(out=(x0, None, index)),
                dict(out=(x0, cost, None))):
        assert call(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert call(nprob=0) == 0
    F = torch.full((4, 8), 2.0, dtype=torch.float64, device=ds.device)
    wh = torch.full((4,), 7, dtype=torch.int32, device=ds.device)
    L, h = ds.lib, ds.h.ptr
    for rc in (L.nlh_starts_cost_batch(h, -1, 8, F.data_ptr(), cost.data_ptr()), L.nlh_starts_cost_batch(h, 4, 0, F.data_ptr(), cost.data_ptr()),
               L.nlh_starts_cost_batch(h, 4, 8, None, cost.data_ptr()), L.nlh_starts_pick_batch(h, 4, 0, F.data_ptr(), wh.data_ptr()),
               L.nlh_starts_pick_batch(h, 4, 9, F.data_ptr(), wh.data_ptr()), L.nlh_starts_pick_batch(h, 4, 2, F.data_ptr(), None),
               L.nlh_starts_take_batch(h, 4, 2, 0, F.data_ptr(), wh.data_ptr(), cost.data_ptr()),
               L.nlh_starts_take_batch(h, 4, 9, 1, F.data_ptr(), wh.data_ptr(), cost.data_ptr()),
               L.nlh_starts_take_batch(h, -1, 2, 1, F.data_ptr(), wh.data_ptr(), cost.data_ptr())):
        assert rc == NL_INVALID_INPUT_ERROR
    assert L.nlh_starts_cost_batch(None, 4, 8, F.data_ptr(), cost.data_ptr()) == NLH_ERR_BAD_HANDLE
    torch.cuda.synchronize()
    assert (x0 == 7.0).all() and (cost == 7.0).all() and (index == 7).all() and (wh == 7).all() and (F == 2.0).all()
    assert call() == 0                                                          # and the same call, let through, writes
    torch.cuda.synchronize()
    got =ds.starts_search(fcn, ctx, nprob, m, Starts(**BOX4, ncand=16, keep=2))
    _same(x0.reshape(-1)[:nprob * 2 * n], got[0].reshape(-1)); _same(cost.reshape(-1)[:nprob * 2], got[1].reshape(-1))
