"""GPU tests of the bootstrap: nlh_boot_resample_batch and nlh_boot_summary_batch bit for bit against tests/boot_restatement.py at
every size edge of their kernels -- a wave's 64 rows, the workgroup's 256, the most rows and replicas there are --, under every
launch shape and slicing; and the one-call forms against the composition they document.  No tolerance anywhere."""
import functools

import numpy as np
import pytest
import torch

import boot_restatement as B
from nonlin_amd import Bootstrap, Expr, Loss, Convolve, Separable

pytestmark = pytest.mark.gpu

SEED = 20261027
NPROB, NREP = 3, 65                                                   # the largest of each: smaller calls are slices of this one
SENTINEL = -7.25


def _dev(ds, a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(ds.device)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what=""):
    assert np.array_equal(_bits(got), _bits(want)), what


def _same_or_nan(got, want, what=""):
    """Bit for bit where the restatement holds a number; a NaN where it holds a NaN."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan])), what


@functools.lru_cache(maxsize=None)
def _data(m, weighted):
    """mu, y [3, m] and weights: None, or problem 0 with about 10 % zero weights, problem 1 with a single active row and
    problem 2 with none."""
    rng = np.random.default_rng(1000 + m)
    mu = rng.uniform(-2.0, 2.0, (NPROB, m))
    y = mu + 0.3 * rng.standard_normal((NPROB, m)) * 10.0 ** rng.integers(-2, 2, (NPROB, m))
    w = None
    if weighted:
        w = np.where(rng.random((NPROB, m)) < 0.1, 0.0, rng.uniform(0.5, 2.0, (NPROB, m)))
        w[0, m // 2] = 1.5                                                     # (problem 0 keeps an active row at m = 1, too)
        w[1] = 0.0
        w[1, (2 * m) // 3] = 0.75
        w[2] = 0.0
        w[2, 0] = -0.0                                                         # a zero of the other sign is a zero
    for a in (mu, y, w):
        if a is not None:
            a.setflags(write=False)
    return mu, y, w


@functools.lru_cache(maxsize=None)
def _reference(kind, m, weighted, centre):
    """The restatement's replicas of the whole: [NREP, NPROB, m], computed once and shared."""
    mu, y, w = _data(m, weighted)
    ys, ws = B.resample(B.KINDS[kind], SEED, mu, y, w, centre, NREP)
    ys.setflags(write=False)
    if ws is not None:
        ws.setflags(write=False)
    return ys, ws


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 16384])
@pytest.mark.parametrize("kind", ["residual", "wild", "pairs"])
def test_resample_bit_for_bit(ds, kind, m):
    for weighted in (False, True):
        mu, y, w = _data(m, weighted)
        for centre in ((True, False) if kind == "residual" else (True,)):
            want_y, want_w = _reference(kind, m, weighted, centre)
            boot = Bootstrap(nrep=NREP, kind=kind, seed=SEED, centre=centre)
            for nprob in (1, 3):
                dmu, dy, dw = _dev(ds, mu[:nprob]), _dev(ds, y[:nprob]), _dev(ds, None if w is None else w[:nprob])
                for nrep in (1, 2, 3, 65):
                    ys, ws = ds.boot_resample(boot, dmu, dy, dw, nrep=nrep)
                    what = (kind, m, weighted, centre, nprob, nrep)
                    assert tuple(ys.shape) == (nrep, nprob, m)
                    _same(ys, want_y[:nrep, :nprob], what)
                    if kind == "pairs":
                        _same(ws, want_w[:nrep, :nprob], what)
                    else:
                        assert ws is None
            if weighted:                                                       # rows of weight 0 are the data's; no active row: a copy
                got = ys.cpu().numpy()
                assert np.array_equal(_bits(got[:, w == 0.0]), _bits(np.broadcast_to(y[w == 0.0], (NREP, int((w == 0.0).sum())))))
                _same(got[:, 2], np.broadcast_to(y[2], (NREP, m)))


@pytest.mark.parametrize("kind", ["residual", "wild", "pairs"])
def test_resample_odd_alignment(ds, kind):
    """Outputs that do not start on 16 bytes take the 8-byte stores: the same bits."""
    m = 64
    mu, y, w = _data(m, True)
    want_y, want_w = _reference(kind, m, True, True)
    L = ds.lib
    dmu, dy, dw = _dev(ds, mu), _dev(ds, y), _dev(ds, w)
    yo = torch.full((5 * NPROB * m + 1,), SENTINEL, dtype=torch.float64, device=ds.device)
    wo = torch.full((5 * NPROB * m + 1,), SENTINEL, dtype=torch.float64, device=ds.device)
    assert yo.data_ptr() % 16 == 0
    rc = L.nlh_boot_resample_batch(ds.h.ptr, B.KINDS[kind], SEED, NPROB, 0, m, 0, 5, dmu.data_ptr(), dy.data_ptr(), dw.data_ptr(), 1,
                                   yo.data_ptr() + 8, wo.data_ptr() + 8)
    assert rc == 0
    torch.cuda.synchronize()
    _same(yo[1:].reshape(5, NPROB, m), want_y[:5])
    assert float(yo[0]) == SENTINEL
    if kind == "pairs":
        _same(wo[1:].reshape(5, NPROB, m), want_w[:5])
    else:
        assert (wo == SENTINEL).all()                                          # the other kinds do not look at dwout


@pytest.mark.parametrize("kind", ["residual", "wild", "pairs"])
def test_resample_slices(ds, kind):
    """A slice of the problems from prob0 and of the replicas from rep0 is the matching rows of the whole."""
    m = 257
    mu, y, w = _data(m, True)
    want_y, want_w = _reference(kind, m, True, True)
    boot = Bootstrap(nrep=NREP, kind=kind, seed=SEED)
    for prob0, nprob, rep0, nrep in ((1, 2, 0, 65), (0, 3, 60, 5), (2, 1, 7, 3), (1, 1, 64, 1)):
        sl = slice(prob0, prob0 + nprob)
        ys, ws = ds.boot_resample(boot, _dev(ds, mu[sl]), _dev(ds, y[sl]), _dev(ds, w[sl]), prob0=prob0, rep0=rep0, nrep=nrep)
        _same(ys, want_y[rep0:rep0 + nrep, sl], (prob0, nprob, rep0, nrep))
        if kind == "pairs":
            _same(ws, want_w[rep0:rep0 + nrep, sl], (prob0, nprob, rep0, nrep))
    big = 2 ** 40 + 5                                                           # a problem far into a large data set
    ys, _ = ds.boot_resample(boot, _dev(ds, mu[:1]), _dev(ds, y[:1]), _dev(ds, w[:1]), prob0=big, rep0=2 ** 31 - 3, nrep=2)
    for r in range(2):
        _same(ys[r, 0], B.resample_one(B.KINDS[kind], SEED, big, 2 ** 31 - 3 + r, mu[0], y[0], w[0], True)[0])


def test_resample_many_problems_and_replicas(ds):
    """More problems than one replica group's grid and the most replicas there are: every (problem, replica) by its own key."""
    m, nprob = 6, 700
    rng = np.random.default_rng(3)
    mu = rng.standard_normal((nprob, m))
    y = mu + rng.standard_normal((nprob, m))
    boot = Bootstrap(nrep=B.MAX_REP, kind="residual", seed=1)
    ys, _ = ds.boot_resample(boot, _dev(ds, mu), _dev(ds, y))
    got = ys.cpu().numpy()
    for p, b in ((0, 0), (699, 4095), (350, 64), (1, 63), (698, 2048)):
        _same(got[b, p], B.resample_one(B.RESIDUAL, 1, p, b, mu[p], y[p], None, True)[0], (p, b))
    ys2, _ = ds.boot_resample(boot, _dev(ds, mu[:2]), _dev(ds, y[:2]))         # the same replicas from another launch shape
    _same(ys2, got[:, :2])


def test_resample_refused_writes_nothing(ds):
    m = 16
    mu, y, w = (_dev(ds, a) for a in _data(64, True))
    L = ds.lib
    yo = torch.full((4, NPROB, m), SENTINEL, dtype=torch.float64, device=ds.device)
    wo = torch.full((4, NPROB, m), SENTINEL, dtype=torch.float64, device=ds.device)

    def call(kind=0, nprob=NPROB, prob0=0, mm=m, rep0=0, nrep=4, pmu=mu.data_ptr(), py=y.data_ptr(), pyo=yo.data_ptr(), pwo=wo.data_ptr()):
        return L.nlh_boot_resample_batch(ds.h.ptr, kind, SEED, nprob, prob0, mm, rep0, nrep, pmu, py, w.data_ptr(), 1, pyo, pwo)
    for bad in (dict(kind=3), dict(kind=-1), dict(nprob=-1), dict(nrep=-1), dict(nrep=B.MAX_REP + 1), dict(mm=0), dict(mm=B.MAX_ROWS + 1),
                dict(prob0=-1), dict(rep0=-1), dict(rep0=2 ** 31 - 2), dict(py=None), dict(pmu=None), dict(kind=1, pmu=None),
                dict(kind=2, pwo=None)):
        assert call(**bad) == 201, bad
    assert call(nprob=0) == 0 and call(nrep=0) == 0
    torch.cuda.synchronize()
    assert (yo == SENTINEL).all() and (wo == SENTINEL).all()
    assert call(kind=2, pmu=None) == 0                                          # pairs does not read the fitted values
    torch.cuda.synchronize()
    assert not (yo == SENTINEL).any() and not (wo == SENTINEL).any()


# ---------------------------------------------------------------------------------------------------------------------
# summary
# ---------------------------------------------------------------------------------------------------------------------
def _refits(nrep, n, seed):
    """xs [nrep, 6, n]: clean; about 20 % of the replicas with a NaN or an infinity somewhere; all NaN; one valid replica;
    ties and zeros of both signs; values of one sign and large."""
    rng = np.random.default_rng(seed)
    xs = rng.standard_normal((nrep, 6, n)) * 10.0 ** rng.integers(-3, 4, (1, 6, n))
    for b in np.flatnonzero(rng.random(nrep) < 0.2):
        xs[b, 1, rng.integers(n)] = rng.choice([np.nan, np.inf, -np.inf])
    xs[:, 2, :] = np.nan
    xs[:, 3, 0] = np.nan
    xs[nrep // 2, 3, 0] = 1.25
    xs[:, 4, :] = rng.integers(-2, 3, (nrep, n))
    xs[:, 4, :][rng.random((nrep, n)) < 0.3] = -0.0
    xs[:, 5, :] = 1e300 + 1e299 * rng.random((nrep, n))
    return xs


@pytest.mark.parametrize("n", [1, 3, 32])
@pytest.mark.parametrize("nrep", [1, 2, 3, 63, 64, 65, 4096])
def test_summary_bit_for_bit(ds, nrep, n):
    xs = _refits(nrep, n, 100 * nrep + n)
    for level in (0.95, 0.5):
        want = B.summary(xs, level)
        got = ds.boot_summary(_dev(ds, xs), level)
        for g, w_, name in zip(got[:4], want[:4], ("lo", "hi", "mean", "sd")):
            assert tuple(g.shape) == (6, n)
            _same_or_nan(g, w_, (name, nrep, n, level))
        assert got[4].dtype == torch.int32 and np.array_equal(got[4].cpu().numpy(), want[4])
    nv = want[4]
    assert nv[0] == nrep and nv[2] == 0 and nv[3] == 1 and nv[4] == nrep
    assert np.isnan(got[0][2].cpu().numpy()).all() and np.isnan(got[3][3].cpu().numpy()).all()
    assert float(got[2][3, 0]) == 1.25
    one = ds.boot_summary(_dev(ds, xs[:, 1:2]), 0.5)                            # a problem's summary does not depend on its batch
    for g, w_ in zip(one[:4], want[:4]):
        _same_or_nan(g, w_[1:2])


def test_summary_refused_writes_nothing(ds):
    xs = _dev(ds, _refits(8, 2, 5))
    outs = [torch.full((6, 2), SENTINEL, dtype=torch.float64, device=ds.device) for _ in range(4)]
    nv = torch.full((6,), -9, dtype=torch.int32, device=ds.device)
    L = ds.lib

    def call(nrep=8, nprob=6, n=2, level=0.95, pxs=xs.data_ptr()):
        return L.nlh_boot_summary_batch(ds.h.ptr, nrep, nprob, n, pxs, level, *[o.data_ptr() for o in outs], nv.data_ptr())
    for bad in (dict(nrep=0), dict(nrep=B.MAX_REP + 1), dict(nprob=-1), dict(n=0), dict(level=0.0), dict(level=1.0), dict(level=float("nan")),
                dict(pxs=None)):
        assert call(**bad) == 201, bad
    assert call(nprob=0) == 0
    torch.cuda.synchronize()
    assert all((o == SENTINEL).all() for o in outs) and (nv == -9).all()


# ---------------------------------------------------------------------------------------------------------------------
# the one-call forms
# ---------------------------------------------------------------------------------------------------------------------
DECAY = ("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))


def _decay_data(seed):
    rng = np.random.default_rng(seed)
    nprob, m = 3, 64
    t = np.arange(m) * 0.125
    x = np.stack([rng.uniform(40, 80, nprob), rng.uniform(0.5, 2.0, nprob), rng.uniform(2, 6, nprob)], axis=1)
    y = x[:, 0:1] * np.exp(-x[:, 1:2] * t[None, :]) + x[:, 2:3] + rng.standard_normal((nprob, m))
    y[1, 20] += 25.0                                                           # an outlier for the robust fit
    w = np.where(rng.random((nprob, m)) < 0.1, 0.0, rng.uniform(0.5, 2.0, (nprob, m)))
    return t, y, w, x


def _by_hand(ds, boot, fit, evaluate, x, y, w):
    """The composition the one-call form documents: the restatement's replicas of the device's fitted values, the one-call
    fit of every replica on its own, the restatement's summary."""
    mu = None if boot.kind == B.PAIRS else evaluate(x).cpu().numpy()
    ys, ws = B.resample(boot.kind, boot.seed, mu, y, w, boot.centre, boot.nrep)
    xs = np.empty((boot.nrep,) + tuple(x.shape))
    for r in range(boot.nrep):
        out = fit(_dev(ds, ys[r]), _dev(ds, w if ws is None else ws[r]))
        xr = out[0].cpu().numpy()
        xr[[s != 0 for s in out[7]]] = np.nan
        xs[r] = xr
    return B.summary(xs, boot.level) + (xs,)


def _compare(got, want):
    for g, w_, name in zip(got[:4] + got[5:], want[:4] + want[5:], ("lo", "hi", "mean", "sd", "xs")):
        _same_or_nan(g, w_, name)
    assert np.array_equal(got[4].cpu().numpy(), want[4])


@pytest.mark.parametrize("kind", ["residual", "wild", "pairs"])
@pytest.mark.parametrize("variant", ["plain", "loss", "sep", "bounds"])
def test_expr_boot_is_the_composition(ds, monkeypatch, variant, kind):
    e = Expr(*DECAY)
    t, y, w, xt = _decay_data(41)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    kw = {"plain": {}, "loss": dict(loss=Loss("huber", [2.0, 3.0, 2.5])), "sep": dict(sep=Separable.for_expr(e, linear=("a", "c"))),
          "bounds": dict(lower=(0.0, 0.0, 3.5), upper=(100.0, 1.2, 10.0))}[variant]
    x = ds.expr_fit_batch(e, dt, dy, _dev(ds, xt), weights=dw, covariance=False, **kw)[0]
    boot = Bootstrap(nrep=5, kind=kind, seed=77, level=0.8)
    want = _by_hand(ds, boot, lambda ys, ws: ds.expr_fit_batch(e, dt, ys, x, weights=ws, covariance=False, **kw),
                    lambda v: ds.expr_eval(e, v, dt), x, y, w)
    got = ds.expr_boot_batch(e, dt, dy, x, boot, weights=dw, **kw)
    _compare(got, want)
    assert tuple(got[5].shape) == (5, 3, 3) and got[4].dtype == torch.int32
    for reps in ("1", "2", "4", "64"):                                         # however the replicas are chunked
        monkeypatch.setenv("NLH_BOOT_REPS", reps)
        again = ds.expr_boot_batch(e, dt, dy, x, boot, weights=dw, **kw)
        for a, b in zip(again, got):
            _same_or_nan(a.to(torch.float64), b.to(torch.float64).cpu().numpy(), reps)


@pytest.mark.parametrize("kind", ["residual", "wild"])
def test_curve_boot_with_conv_is_the_composition(ds, monkeypatch, kind):
    t, y, w, xt = _decay_data(42)
    tt = np.broadcast_to(t, y.shape).copy()                                    # a per-problem t: repeated per chunk
    dt, dy, dw = _dev(ds, tt), _dev(ds, y), _dev(ds, w)
    conv = Convolve([0.2, 0.5, 0.3], origin=0, extend="hold")
    kw = dict(ncomp=1, baseline=0, conv=conv)
    x = ds.curve_fit_batch("expdecay", dt, dy, _dev(ds, xt), weights=dw, covariance=False, **kw)[0]
    boot = Bootstrap(nrep=5, kind=kind, seed=78)
    want = _by_hand(ds, boot, lambda ys, ws: ds.curve_fit_batch("expdecay", dt, ys, x, weights=ws, covariance=False, **kw),
                    lambda v: ds.conv_apply(conv, ds.curve_eval("expdecay", v, dt, 1, 0)), x, y, w)
    got = ds.curve_boot_batch("expdecay", dt, dy, x, boot, weights=dw, **kw)
    _compare(got, want)
    monkeypatch.setenv("NLH_BOOT_REPS", "2")
    again = ds.curve_boot_batch("expdecay", dt, dy, x, boot, weights=dw, **kw)
    for a, b in zip(again, got):
        _same_or_nan(a.to(torch.float64), b.to(torch.float64).cpu().numpy())


def test_one_call_spread_is_the_noise(ds):
    """Not a check of bits: the interval of a well-posed fit holds the fit, and sd is of the size of the fit's own sigma."""
    e = Expr(*DECAY)
    t, y, w, xt = _decay_data(43)
    y[1, 20] -= 25.0
    dt, dy = _dev(ds, t), _dev(ds, y)
    x, _, sigma, *_ = ds.expr_fit_batch(e, dt, dy, _dev(ds, xt))
    lo, hi, mean, sd, nvalid, xs = ds.expr_boot_batch(e, dt, dy, x, Bootstrap(nrep=200, seed=3))
    assert (nvalid == 200).all() and (lo < x).all() and (x < hi).all()
    ratio = (sd / sigma).cpu().numpy()
    assert (ratio > 0.5).all() and (ratio < 2.0).all(), ratio


def test_one_call_refusals(ds):
    from nonlin_amd import Poisson
    e = Expr(*DECAY)
    t, y, w, xt = _decay_data(44)
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, xt)
    with pytest.raises(ValueError, match="excludes stat and group"):
        ds.expr_boot_batch(e, dt, dy, dx, Bootstrap(5), stat=Poisson())
    with pytest.raises(ValueError, match="excludes stat and group"):
        ds.curve_boot_batch("expdecay", dt, dy, dx, Bootstrap(5), baseline=0, group=object())
    with pytest.raises(ValueError, match='"pairs" excludes conv'):
        ds.curve_boot_batch("expdecay", dt, dy, dx, Bootstrap(5, "pairs"), baseline=0, conv=Convolve([0.5, 0.5]))
