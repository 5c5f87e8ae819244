"""GPU tests of the Poisson bootstrap: nlh_boot_poisson_batch bit for bit against tests/boot_pois_restatement.py, `bad` included,
at the shapes where its kernel can go wrong -- one row, both store widths, the crossing of a ballot word, the staged and the
per-thread setup, a block of replicas and one more --; the one-call forms against the composition they document; and the spread
of the replicas' fits against the CPU study.  No tolerance on any bit."""
import functools
import json

import numpy as np
import pytest
import torch

import boot_pois_cases as BC
import boot_pois_restatement as BP
import boot_restatement as B
import pois_cases as PC
from nonlin_amd import PoissonBootstrap, Poisson, Expr, Convolve

pytestmark = pytest.mark.gpu

SEED = 20261103
NPROB, NREP = 3, 65                                                   # the largest of each: smaller calls are slices of this one
SENTINEL = -7.25
MEANS = (2.0 ** -20, 0.3, 1.0, 4.7, 50.5, 1000.25)                   # along the rows: the lanes of a wave walk different lengths


def _dev(ds, a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(ds.device)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want, what=""):
    assert np.array_equal(_bits(got), _bits(want)), what


def _same_or_nan(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan])), what


@functools.lru_cache(maxsize=None)
def _data(m, weighted):
    """mu, y [3, m] and weights.  mu: MEANS along the rows, shifted per problem; problem 1 holds the row classes as far as it has
    rows for them: a zero row (1), a bad one (2: negative), an inactive one (0, with weights), -0.0 (4), NaN (5), above 2^24 (6).
    Weights: None, or problem 0 with zero rows at the first, a middle and the last row, problem 1 as said, problem 2 all zero."""
    rng = np.random.default_rng(2000 + m)
    mu = np.array([[MEANS[(i + 2 * p) % len(MEANS)] for i in range(m)] for p in range(NPROB)])
    y = rng.poisson(mu).astype(np.float64) + 1.0                               # (never 0: a copied row shows)
    for i, v in ((1, 0.0), (2, -1.0), (4, -0.0), (5, np.nan), (6, 2.0 ** 24 + 2)):
        if i < m:
            mu[1, i] = v
    w = None
    if weighted:
        w = np.ones((NPROB, m))
        w[0, [0, m // 2, m - 1]] = 0.0
        if m >= 4:
            w[1, 0] = 0.0
        if m >= 130:
            w[1, 70] = -0.0                                                    # a zero of the other sign is a zero
            mu[1, 70] = np.nan                                                 # and a bad mean on an inactive row is not bad
        w[2] = 0.0
    for a in (mu, y, w):
        if a is not None:
            a.setflags(write=False)
    return mu, y, w


@functools.lru_cache(maxsize=None)
def _reference(m, weighted):
    """The restatement's replicas of the whole: [NREP, NPROB, m] and bad [NPROB], computed once and shared."""
    mu, y, w = _data(m, weighted)
    ys, bad = BP.poisson(SEED, mu, y, w, NREP)
    ys.setflags(write=False)
    return ys, bad


@pytest.mark.parametrize("m", [1, 2, 7, 64, 65, 130])
def test_poisson_bit_for_bit(ds, m):
    boot = PoissonBootstrap(nrep=NREP, seed=SEED)
    for weighted in (False, True):
        mu, y, w = _data(m, weighted)
        want, want_bad = _reference(m, weighted)
        for nprob in (1, 3):
            dmu, dy, dw = _dev(ds, mu[:nprob]), _dev(ds, y[:nprob]), _dev(ds, None if w is None else w[:nprob])
            for nrep in (1, 64, 65):
                ys, bad = ds.boot_poisson(boot, dmu, dy, dw, nrep=nrep)
                what = (m, weighted, nprob, nrep)
                assert tuple(ys.shape) == (nrep, nprob, m) and bad.dtype == torch.int32
                _same(ys, want[:nrep, :nprob], what)
                assert np.array_equal(bad.cpu().numpy(), want_bad[:nprob]), what
        got = ys.cpu().numpy()
        assert (got[~np.isnan(got)] >= 0.0).all() and (got[:, 0] == np.floor(got[:, 0])).all()
        if m >= 7:
            assert list(want_bad) == [0, 3, 0]                                 # negative, NaN, above 2^24; -0.0 and 0.0 are zero rows
            assert (got[:, 1, [1, 4]] == 0.0).all() and not np.signbit(got[:, 1, [1, 4]]).any()
            _same(got[:, 1, [2, 5, 6]], np.broadcast_to(y[1, [2, 5, 6]], (NREP, 3)))
        if weighted:                                                           # rows of weight 0 are the data's; no active row: a copy
            assert np.array_equal(_bits(got[:, w == 0.0]), _bits(np.broadcast_to(y[w == 0.0], (NREP, int((w == 0.0).sum())))))
            _same(got[:, 2], np.broadcast_to(y[2], (NREP, m)))


def test_poisson_most_rows(ds):
    """m = 16384: every thread owns 32 units of two rows and makes their setup itself."""
    m = B.MAX_ROWS
    rng = np.random.default_rng(6)
    mu = (rng.choice([2.0 ** -20, 0.3, 1.0, 4.7, 50.0], m) * rng.uniform(0.5, 1.0, m))[None]
    y = rng.poisson(mu).astype(np.float64)
    w = np.where(rng.random((1, m)) < 0.1, 0.0, 1.0)
    mu[0, 9000] = -3.0
    w[0, 9000] = 1.0
    want, want_bad = BP.poisson(SEED, mu, y, w, 2)
    ys, bad = ds.boot_poisson(PoissonBootstrap(nrep=2, seed=SEED), _dev(ds, mu), _dev(ds, y), _dev(ds, w))
    _same(ys, want)
    assert bad.cpu().tolist() == [1] == list(want_bad)


def test_poisson_largest_mean(ds):
    """A single row at mu = 2^24: the longest setup and the longest walks there are."""
    mu, y = np.array([[2.0 ** 24]]), np.array([[5.0]])
    want, _ = BP.poisson(SEED, mu, y, None, 2)
    ys, bad = ds.boot_poisson(PoissonBootstrap(nrep=2, seed=SEED), _dev(ds, mu), _dev(ds, y))
    _same(ys, want)
    assert bad.cpu().tolist() == [0] and abs(float(ys[0, 0, 0]) - 2.0 ** 24) < 6 * 4096


def test_poisson_odd_alignment(ds):
    """An output that does not start on 16 bytes takes the 8-byte stores with an even m: the same bits."""
    m = 64
    mu, y, w = _data(m, True)
    want, want_bad = _reference(m, True)
    dmu, dy, dw = _dev(ds, mu), _dev(ds, y), _dev(ds, w)
    yo = torch.full((5 * NPROB * m + 1,), SENTINEL, dtype=torch.float64, device=ds.device)
    bad = torch.full((NPROB,), -9, dtype=torch.int32, device=ds.device)
    assert yo.data_ptr() % 16 == 0
    rc = ds.lib.nlh_boot_poisson_batch(ds.h.ptr, SEED, NPROB, 0, m, 0, 5, dmu.data_ptr(), dy.data_ptr(), dw.data_ptr(), yo.data_ptr() + 8,
                                       bad.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    _same(yo[1:].reshape(5, NPROB, m), want[:5])
    assert float(yo[0]) == SENTINEL and np.array_equal(bad.cpu().numpy(), want_bad)


def test_poisson_slices(ds):
    """A slice of the problems from prob0 and of the replicas from rep0 is the matching rows of the whole."""
    m = 65
    mu, y, w = _data(m, True)
    want, want_bad = _reference(m, True)
    boot = PoissonBootstrap(nrep=NREP, seed=SEED)
    for prob0, nprob, rep0, nrep in ((1, 2, 0, 65), (0, 3, 60, 5), (2, 1, 7, 3), (1, 1, 64, 1)):
        sl = slice(prob0, prob0 + nprob)
        ys, bad = ds.boot_poisson(boot, _dev(ds, mu[sl]), _dev(ds, y[sl]), _dev(ds, w[sl]), prob0=prob0, rep0=rep0, nrep=nrep)
        _same(ys, want[rep0:rep0 + nrep, sl], (prob0, nprob, rep0, nrep))
        assert np.array_equal(bad.cpu().numpy(), want_bad[sl])
    prob0, nrep = 2 ** 31 - 3, 3                                                # problems and replicas at the end of 32 bits
    rep0 = 2 ** 31 - 1 - nrep
    ys, bad = ds.boot_poisson(boot, _dev(ds, mu), _dev(ds, y), _dev(ds, w), prob0=prob0, rep0=rep0, nrep=nrep)
    far, far_bad = BP.poisson(SEED, mu, y, w, nrep, prob0=prob0, rep0=rep0)
    _same(ys, far)
    assert np.array_equal(bad.cpu().numpy(), far_bad) and not np.array_equal(_bits(far), _bits(want[:nrep]))


def test_poisson_refused_writes_nothing(ds):
    m = 16
    mu, y, w = (_dev(ds, a) for a in _data(64, True))
    yo = torch.full((4, NPROB, m), SENTINEL, dtype=torch.float64, device=ds.device)
    bad = torch.full((NPROB,), -9, dtype=torch.int32, device=ds.device)

    def call(nprob=NPROB, prob0=0, mm=m, rep0=0, nrep=4, pmu=mu.data_ptr(), py=y.data_ptr(), pyo=yo.data_ptr(), pbad=bad.data_ptr()):
        return ds.lib.nlh_boot_poisson_batch(ds.h.ptr, SEED, nprob, prob0, mm, rep0, nrep, pmu, py, w.data_ptr(), pyo, pbad)
    for kw in (dict(nprob=-1), dict(nrep=-1), dict(nrep=B.MAX_REP + 1), dict(mm=0), dict(mm=B.MAX_ROWS + 1), dict(prob0=-1), dict(rep0=-1),
               dict(rep0=2 ** 31 - 2), dict(pmu=None), dict(py=None), dict(pyo=None), dict(pbad=None)):
        assert call(**kw) == 201, kw
    assert call(nprob=0) == 0 and call(nrep=0) == 0
    torch.cuda.synchronize()
    assert (yo == SENTINEL).all() and (bad == -9).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (yo == SENTINEL).any() and not (bad == -9).any()


# ---------------------------------------------------------------------------------------------------------------------
# the one-call forms
# ---------------------------------------------------------------------------------------------------------------------
DECAY = ("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))


def _decays(nprob, m, seed):
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 4.0, m)
    xt = np.stack([rng.uniform(30, 70, nprob), rng.uniform(0.7, 1.4, nprob), rng.uniform(0.5, 3.0, nprob)], axis=1)
    y = rng.poisson(xt[:, 0:1] * np.exp(-xt[:, 1:2] * t[None, :]) + xt[:, 2:3]).astype(np.float64)
    return t, y, xt


def _by_hand(ds, boot, fit, evaluate, x, y, w):
    """The composition the one-call form documents: the restatement's replicas of the device's fitted values, the one-call
    deviance fit of every replica on its own, the restatement's summary."""
    mu = evaluate(x).cpu().numpy()
    ys, bad = BP.poisson(boot.seed, mu, y, w, boot.nrep)
    xs = np.empty((boot.nrep,) + tuple(x.shape))
    for r in range(boot.nrep):
        out = fit(_dev(ds, ys[r]))
        xr = out[0].cpu().numpy()
        xr[[s != 0 for s in out[7]]] = np.nan
        xr[bad > 0] = np.nan
        xs[r] = xr
    return B.summary(xs, boot.level) + (xs,)


def _compare(got, want):
    for g, w_, name in zip(got[:4] + got[5:], want[:4] + want[5:], ("lo", "hi", "mean", "sd", "xs")):
        _same_or_nan(g, w_, name)
    assert np.array_equal(got[4].cpu().numpy(), want[4])


@pytest.mark.parametrize("variant", ["plain", "conv", "mask"])
def test_expr_boot_is_the_composition(ds, monkeypatch, variant):
    e = Expr(*DECAY)
    t, y, xt = _decays(4, 32, 51)
    w = None
    kw = {}
    if variant == "mask":
        w = np.where(np.random.default_rng(52).random(y.shape) < 0.15, 0.0, 1.0)
    if variant == "conv":
        kw = dict(conv=Convolve([0.2, 0.5, 0.3], origin=0, extend="hold"))
    stat = Poisson()
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    x = ds.expr_fit_batch(e, dt, dy, _dev(ds, xt), weights=dw, covariance=False, stat=stat, **kw)[0]
    boot = PoissonBootstrap(8, seed=77, level=0.8)
    evaluate = (lambda v: ds.conv_apply(kw["conv"], ds.expr_eval(e, v, dt))) if variant == "conv" else (lambda v: ds.expr_eval(e, v, dt))
    want = _by_hand(ds, boot, lambda ys: ds.expr_fit_batch(e, dt, ys, x, weights=dw, covariance=False, stat=stat, **kw), evaluate, x, y, w)
    got = ds.expr_boot_batch(e, dt, dy, x, boot, weights=dw, stat=stat, **kw)
    _compare(got, want)
    assert tuple(got[5].shape) == (8, 4, 3) and got[4].dtype == torch.int32 and (got[4] > 0).all()
    monkeypatch.setenv("NLH_BOOT_REPS", "3")                                   # however the replicas are chunked
    again = ds.expr_boot_batch(e, dt, dy, x, boot, weights=dw, stat=stat, **kw)
    for a, b in zip(again, got):
        _same_or_nan(a.to(torch.float64), b.to(torch.float64).cpu().numpy())


def test_a_negative_fitted_value_invalidates_its_problem_alone(ds):
    e = Expr(*DECAY)
    t, y, xt = _decays(4, 32, 53)
    stat = Poisson()
    dt, dy = _dev(ds, t), _dev(ds, y)
    x = ds.expr_fit_batch(e, dt, dy, _dev(ds, xt), covariance=False, stat=stat)[0]
    boot = PoissonBootstrap(8, seed=78)
    good = ds.expr_boot_batch(e, dt, dy, x, boot, stat=stat)
    xb = x.clone()
    xb[1, 2] = -5.0                                                            # a*exp(-k*t) + c falls below 0 at the late bins
    assert (ds.expr_eval(e, xb, dt)[1] < 0.0).any()
    lo, hi, mean, sd, nvalid, xs = ds.expr_boot_batch(e, dt, dy, xb, boot, stat=stat)
    assert nvalid.cpu().tolist()[1] == 0 and all(torch.isnan(a[1]).all() for a in (lo, hi, mean, sd)) and torch.isnan(xs[:, 1]).all()
    keep = [0, 2, 3]
    for a, b in zip((lo, hi, mean, sd, xs.transpose(0, 1)), good[:4] + (good[5].transpose(0, 1),)):
        _same_or_nan(a[keep], b[keep].cpu().numpy())
    assert nvalid.cpu().tolist()[0::2] == good[4].cpu().tolist()[0::2] and nvalid.cpu().tolist()[3] == good[4].cpu().tolist()[3]


def test_spread_against_the_cpu_study(ds):
    """The first 64 decays of the study's first truth, fitted and bootstrapped on the device: the median of sd_boot / sigma over
    them lies within four of the standard errors recorded in boot_pois_study.json of the value recorded there for the same 64
    data sets on the CPU oracle."""
    s = json.load(open(BC.STUDY_GOLDEN))["study"][0]["median_ratio_first%d" % BC.NGPU]
    t, y, xt, x0 = BC.problems(0)
    n = BC.NGPU
    dt, dy = _dev(ds, t[:n]), _dev(ds, y[:n])
    stat = Poisson()
    kw = dict(ncomp=PC.K, baseline=PC.B, stat=stat)
    x, _, sigma, *_ = ds.curve_fit_batch(PC.KIND, dt, dy, _dev(ds, x0[:n]), **kw)
    lo, hi, mean, sd, nvalid, xs = ds.curve_boot_batch(PC.KIND, dt, dy, x, PoissonBootstrap(BC.NREP, seed=BC.BOOT_SEED, level=BC.LEVEL), **kw)
    assert int(nvalid.min()) >= BC.NREP - 2
    ratio = (sd / sigma).cpu().numpy()
    for j, q in enumerate(BC.PARAMS):
        med = float(np.median(ratio[:, j]))
        print(q, med, s[q])
        assert abs(med - s[q]["median"]) <= 4.0 * s[q]["stderr"], (q, med, s[q])
