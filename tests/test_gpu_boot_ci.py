"""GPU tests of the studentised and the BCa interval of the bootstrap: nlh_boot_student_batch, nlh_boot_accel_batch and
nlh_boot_jackknife_batch bit for bit against tests/boot_ci_restatement.py at every size edge of their kernels -- a wave's 64,
the workgroup's 256, the most replicas and rows there are --; nlh_boot_bca_batch exact in everything that reaches no library
function, within the header's 2^-44 in alpha, and bit for bit in lo and hi given the alphas it returns; and the one-call forms
against the composition of the public pieces."""
import functools

import numpy as np
import pytest
import torch

import boot_restatement as B
import boot_ci_restatement as R
from nonlin_amd import Bootstrap, PoissonBootstrap, Expr, Loss, Convolve, Poisson

pytestmark = pytest.mark.gpu

NPROB = 3
SENTINEL = -7.25
ALPHA_TOL = 2.0 ** -44                                                          # the header's bound between two libraries' alphas
# ppnd16's tails: an 8-ulp log is 2^-50 relative, enters r = sqrt(-log p) halved, and z(r) -- close to linear in r over the tails,
# |z'(r) r / z| < 2 -- passes it on at most doubled: 2^-50 relative and a few roundings.  2^-44 relative leaves room for both.
Z0_TAIL_TOL = 2.0 ** -44
SEEN = {"alpha": 0.0, "z0_tail": 0.0}                                           # the largest differences met (printed by the tests)


def _dev(ds, a, dtype=None):
    return None if a is None else torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(ds.device)


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=np.float64).view(np.uint64)


def _same(got, want, what=""):
    assert np.array_equal(_bits(got), _bits(want)), what


def _same_or_nan(got, want, what=""):
    """Bit for bit where the restatement holds a number; a NaN where it holds a NaN."""
    got, want = _np(got), _np(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan])), what


@functools.lru_cache(maxsize=None)
def _case(nrep, n):
    """xs, sigs [nrep, 3, n], x, sigma, a [3, n].  Problem 0: small integers -- ties -- and zeros of both signs; problem 1: about
    20 % of the replicas with a NaN or an infinity somewhere; problem 2: large values of one sign.  sigs: about a quarter 0,
    negative, NaN or Inf.  xhat by parameter in turn: a value the replicas take (ties with xhat), below all of them, above all of
    them, their median.  With n >= 3 also an xhat that is a NaN, sigmas that will not do, an acceleration that is a NaN and one
    that makes the upper end's denominator negative."""
    rng = np.random.default_rng(7000 + 37 * nrep + n)
    xs = rng.standard_normal((nrep, NPROB, n))
    xs[:, 0, :] = rng.integers(-2, 3, (nrep, n))
    xs[:, 0, :][rng.random((nrep, n)) < 0.3] = -0.0
    for b in np.flatnonzero(rng.random(nrep) < 0.2):
        xs[b, 1, rng.integers(n)] = rng.choice([np.nan, np.inf, -np.inf])
    xs[:, 2, :] = 1e6 + 1e5 * rng.random((nrep, n))
    sigs = rng.uniform(0.5, 2.0, (nrep, NPROB, n))
    bad = rng.random((nrep, NPROB, n)) < 0.25
    sigs[bad] = rng.choice([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf], int(bad.sum()))
    valid = np.isfinite(xs).all(axis=2)
    x = np.empty((NPROB, n))
    for p in range(NPROB):
        v = xs[valid[:, p], p, :] if valid[:, p].any() else np.zeros((1, n))
        for j in range(n):
            kind = (j + p) % 4
            x[p, j] = (v[0, j], v[:, j].min() - 1.0, v[:, j].max() + 1.0, np.median(v[:, j]))[kind]
    sigma = rng.uniform(0.5, 2.0, (NPROB, n))
    a = rng.uniform(-0.05, 0.05, (NPROB, n))
    if n >= 3:
        x[1, 0] = np.nan
        sigma[0, 1], sigma[1, 1], sigma[2, 1] = 0.0, -1.0, np.inf
        a[0, 0] = np.nan
        x[2, 2], a[2, 2] = np.median(xs[:, 2, 2]), 50.0                         # z0 near 0: den = 1 - 50 (z0 + z_hi) < 0
    for arr in (xs, sigs, x, sigma, a):
        arr.setflags(write=False)
    return xs, sigs, x, sigma, a


@pytest.mark.parametrize("n", [1, 3, 32])
@pytest.mark.parametrize("nrep", [1, 2, 3, 63, 64, 65, 255, 256, 257, 4096])
def test_student_bit_for_bit(ds, nrep, n):
    xs, sigs, x, sigma, _ = _case(nrep, n)
    dxs, dsigs, dx, dsigma = (_dev(ds, v) for v in (xs, sigs, x, sigma))
    for level in (0.95, 0.5):
        want = R.student(xs, sigs, x, sigma, level)
        got = ds.boot_student(dxs, dsigs, dx, dsigma, level)
        assert tuple(got[0].shape) == (NPROB, n) and got[2].dtype == torch.int32
        _same_or_nan(got[0], want[0], ("lo", nrep, n, level))
        _same_or_nan(got[1], want[1], ("hi", nrep, n, level))
        assert np.array_equal(_np(got[2]), want[2])
    if n >= 3:
        assert np.isnan(_np(got[0])[:, 1]).all() and np.isnan(_np(got[0])[1, 0])
    if nrep >= 63:
        assert np.isfinite(_np(got[0])[0, 0]) and (want[2] < nrep).any() and (want[2] > 0).all()
    one = ds.boot_student(_dev(ds, xs[:, 1:2]), _dev(ds, sigs[:, 1:2]), _dev(ds, x[1:2]), _dev(ds, sigma[1:2]), 0.5)
    for g, w_ in zip(one[:2], want[:2]):                                        # a problem's interval does not depend on its batch
        _same_or_nan(g, w_[1:2])


@pytest.mark.parametrize("n", [1, 3, 32])
@pytest.mark.parametrize("nrep", [1, 2, 3, 63, 64, 65, 255, 256, 257, 4096])
def test_bca(ds, nrep, n):
    xs, _, x, _, a = _case(nrep, n)
    dxs, dx, da = _dev(ds, xs), _dev(ds, x), _dev(ds, a)
    for level in (0.95, 0.5):
        lo, hi, z0, alo, ahi, flags, nvalid = (_np(v) for v in ds.boot_bca(dxs, dx, da, level))
        want = R.bca(xs, x, a, level)
        c2, cnt = R.bca_counts(xs, x)
        what = (nrep, n, level)
        assert np.array_equal(flags, want[5]) and flags.dtype == np.int32, what          # the integers
        assert np.array_equal(nvalid, want[6]) and nvalid.dtype == np.int32, what
        zq = [R.ppnd16(q) for q in R.levels(level)]
        for p in range(NPROB):
            for j in range(n):
                f = int(flags[p, j])
                if f & R.NO_REPLICA:
                    assert all(np.isnan(v[p, j]) for v in (lo, hi, z0, alo, ahi)), what
                    continue
                if f & R.DEGENERATE:
                    assert z0[p, j] == want[2][p, j] and np.isinf(z0[p, j]) and (alo[p, j], ahi[p, j]) == R.levels(level), what
                    continue
                u = float(c2[p, j]) / float(2 * cnt[p])
                if R.central(u):
                    assert _bits(z0[p, j]) == _bits(want[2][p, j]), what + (p, j)
                else:
                    d = abs(z0[p, j] - want[2][p, j]) / abs(want[2][p, j])
                    SEEN["z0_tail"] = max(SEEN["z0_tail"], d)
                    assert d <= Z0_TAIL_TOL, what + (p, j, z0[p, j], want[2][p, j])
                aeff = 0.0 if f & R.NO_ACCEL else a[p, j]
                for t, (g, w_) in enumerate(((alo[p, j], want[3][p, j]), (ahi[p, j], want[4][p, j]))):
                    den = 1.0 - aeff * (want[2][p, j] + zq[t])
                    if not den > 0.0:
                        assert den < -1e-6 and f & R.BAD_DENOM and g == R.levels(level)[t], what + (p, j)
                        continue
                    assert den >= 0.5, what + (p, j)                                 # the inputs stay where the bound is stated
                    SEEN["alpha"] = max(SEEN["alpha"], abs(g - w_))
                    assert abs(g - w_) <= ALPHA_TOL, what + (p, j, g, w_)
        given = R.bca(xs, x, a, level, alphas=(alo, ahi))                       # lo and hi: exact given the device's own alphas
        _same_or_nan(lo, given[0], ("lo",) + what)
        _same_or_nan(hi, given[1], ("hi",) + what)
    print("largest |alpha - restatement|", SEEN["alpha"], "largest relative z0 tail difference", SEEN["z0_tail"])
    if n >= 3:
        assert flags[1, 0] == R.NO_REPLICA and flags[0, 0] & R.NO_ACCEL and flags[2, 2] == R.BAD_DENOM
    deg = [(p, j) for p in range(NPROB) for j in range(n) if (j + p) % 4 in (1, 2) and not (n >= 3 and (p, j) in ((1, 0), (2, 2)))]
    assert all(flags[p, j] & R.DEGENERATE for p, j in deg if cnt[p] > 0), (nrep, n)         # xhat below all, above all


def test_bca_no_replica_and_single_problem(ds):
    xs, _, x, _, a = _case(65, 3)
    none = np.array(xs)
    none[:, 2, 1] = np.nan                                                      # every row of problem 2 holds a NaN
    got = [_np(v) for v in ds.boot_bca(_dev(ds, none), _dev(ds, x), _dev(ds, a), 0.9)]
    assert (got[5][2] == R.NO_REPLICA).all() and got[6][2] == 0 and all(np.isnan(v[2]).all() for v in got[:5])
    whole = [_np(v) for v in ds.boot_bca(_dev(ds, xs), _dev(ds, x), _dev(ds, a), 0.9)]
    one = [_np(v) for v in ds.boot_bca(_dev(ds, xs[:, 1:2]), _dev(ds, x[1:2]), _dev(ds, a[1:2]), 0.9)]
    for g, w_ in zip(one[:5], whole[:5]):                                       # a problem's interval does not depend on its batch
        _same_or_nan(g, w_[1:2])
    assert np.array_equal(one[5], whole[5][1:2]) and one[6][0] == whole[6][1]
    for g, w_ in zip(got[:5], whole[:5]):
        _same_or_nan(g[:2], w_[:2])


@functools.lru_cache(maxsize=None)
def _jack_case(m):
    rng = np.random.default_rng(9000 + m)
    n = 3
    xj = rng.standard_normal((m, NPROB, n)) * 10.0 ** rng.integers(-2, 3, (1, NPROB, n))
    xj[:, 1, :] = np.round(xj[:, 1, :])                                         # ties; with few rows: no spread at all
    for i in np.flatnonzero(rng.random(m) < 0.15):
        xj[i, 2, rng.integers(n)] = rng.choice([np.nan, np.inf, -np.inf])
    w = np.where(rng.random((NPROB, m)) < 0.2, 0.0, rng.uniform(0.5, 2.0, (NPROB, m)))
    w[0, 0] = -0.0
    for arr in (xj, w):
        arr.setflags(write=False)
    return xj, w


@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 256, 257, 16384])
def test_accel_bit_for_bit(ds, m):
    xj, w = _jack_case(m)
    for weights in (None, w):
        want_a, want_n = R.accel(xj, weights)
        a, nj = ds.boot_accel(_dev(ds, xj), _dev(ds, weights))
        assert nj.dtype == torch.int32 and np.array_equal(_np(nj), want_n), (m, weights is None)
        _same(a, want_a, (m, weights is None))
    if m >= 63:
        assert want_a[[0, 2]].all() and (want_n < m).all() and (want_n > 1).all()   # (a small scale rounds problem 1 to no spread)
    if m == 1:
        assert not _np(a).any() and not np.signbit(_np(a)).any()                # fewer than two deletions: +0.0
    one, nj1 = ds.boot_accel(_dev(ds, xj[:, 2:3]), _dev(ds, w[2:3]))            # a problem's value does not depend on its batch
    _same(one, want_a[2:3])
    assert _np(nj1)[0] == want_n[2]


@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 256, 257, 16384])
def test_jackknife_bit_for_bit(ds, m):
    _, w = _jack_case(m)
    slices = [(0, m)] if m <= 257 else [(0, 3), (m - 3, 3), (8191, 2)]
    for weights in (None, w):
        dw = _dev(ds, weights)
        for row0, nrows in slices:
            want = R.jackknife(weights, NPROB, m, row0, nrows)
            got = ds.boot_jackknife(dw, NPROB, m, row0, nrows)
            assert tuple(got.shape) == (nrows, NPROB, m)
            _same(got, want, (m, weights is None, row0, nrows))
        if m <= 257:
            whole = _np(ds.boot_jackknife(dw, NPROB, m))                        # nrows=None: every row
            _same(whole, want)
            for row0, nrows in ((0, 1), (m - 1, 1), (m // 2, m - m // 2)):
                _same(ds.boot_jackknife(dw, NPROB, m, row0, nrows), whole[row0:row0 + nrows], (m, row0, nrows))
            # an output that does not start on 16 bytes takes the 8-byte stores: the same bits, and nothing outside them
            buf = torch.full((m * NPROB * m + 2,), SENTINEL, dtype=torch.float64, device=ds.device)
            assert buf.data_ptr() % 16 == 0
            rc = ds.lib.nlh_boot_jackknife_batch(ds.h.ptr, NPROB, m, 0, m, dw.data_ptr() if dw is not None else None, buf.data_ptr() + 8)
            assert rc == 0
            torch.cuda.synchronize()
            _same(buf[1:-1].reshape(m, NPROB, m), whole)
            assert float(buf[0]) == SENTINEL and float(buf[-1]) == SENTINEL


def test_refused_calls_write_nothing(ds):
    xs, sigs, x, sigma, a = (_dev(ds, v) for v in _case(65, 3))
    L, h = ds.lib, ds.h.ptr
    outs = [torch.full((NPROB, 3), SENTINEL, dtype=torch.float64, device=ds.device) for _ in range(5)]
    ints = [torch.full(shape, -9, dtype=torch.int32, device=ds.device) for shape in ((NPROB, 3), (NPROB,))]
    big = torch.full((8, NPROB, 8), SENTINEL, dtype=torch.float64, device=ds.device)
    P = lambda t_: t_.data_ptr()

    def stud(nrep=65, nprob=NPROB, n=3, level=0.95, pxs=P(xs), psg=P(sigs)):
        return L.nlh_boot_student_batch(h, nrep, nprob, n, pxs, psg, P(x), P(sigma), level, P(outs[0]), P(outs[1]), P(ints[0]))

    def bca(nrep=65, nprob=NPROB, n=3, level=0.95, pxs=P(xs), pa=P(a)):
        return L.nlh_boot_bca_batch(h, nrep, nprob, n, pxs, P(x), pa, level, *[P(o) for o in outs], P(ints[0]), P(ints[1]))
    for call in (stud, bca):
        for bad in (dict(nrep=0), dict(nrep=B.MAX_REP + 1), dict(nprob=-1), dict(n=0), dict(level=0.0), dict(level=1.0),
                    dict(level=float("nan")), dict(pxs=None)):
            assert call(**bad) == 201, (call.__name__, bad)
        assert call(nprob=0) == 0
    assert stud(psg=None) == 201 and bca(pa=None) == 201

    def jack(nprob=NPROB, m=8, row0=0, nrows=8, pout=P(big)):
        return L.nlh_boot_jackknife_batch(h, nprob, m, row0, nrows, None, pout)
    for bad in (dict(nprob=-1), dict(m=0), dict(m=B.MAX_ROWS + 1), dict(row0=-1), dict(nrows=-1), dict(row0=1), dict(nrows=9), dict(pout=None)):
        assert jack(**bad) == 201, bad
    assert jack(nprob=0) == 0 and jack(nrows=0) == 0

    def acc(m=8, nprob=NPROB, n=3, pxj=P(xs)):
        return L.nlh_boot_accel_batch(h, m, nprob, n, pxj, None, P(outs[0]), P(ints[1]))
    for bad in (dict(m=0), dict(m=B.MAX_ROWS + 1), dict(nprob=-1), dict(n=0), dict(pxj=None)):
        assert acc(**bad) == 201, bad
    assert acc(nprob=0) == 0
    torch.cuda.synchronize()
    assert all((o == SENTINEL).all() for o in outs) and all((i == -9).all() for i in ints) and (big == SENTINEL).all()
    assert stud() == 0 and bca() == 0 and jack() == 0 and acc() == 0            # the same calls, accepted, do write
    torch.cuda.synchronize()
    assert not any((o == SENTINEL).any() for o in outs) and not (big == SENTINEL).any() and not any((i == -9).any() for i in ints)


# ---------------------------------------------------------------------------------------------------------------------
# the one-call forms
# ---------------------------------------------------------------------------------------------------------------------
DECAY = ("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
NDEC, MDEC = 8, 16


def _decays(seed, counts=False):
    rng = np.random.default_rng(seed)
    t = np.arange(MDEC) * 0.25
    xt = np.stack([rng.uniform(40, 80, NDEC), rng.uniform(0.5, 1.5, NDEC), rng.uniform(2, 6, NDEC)], axis=1)
    mu = xt[:, 0:1] * np.exp(-xt[:, 1:2] * t[None, :]) + xt[:, 2:3]
    y = rng.poisson(mu).astype(np.float64) if counts else mu + rng.standard_normal((NDEC, MDEC))
    w = np.where(rng.random((NDEC, MDEC)) < 0.1, 0.0, 1.0 if counts else rng.uniform(0.5, 2.0, (NDEC, MDEC)))
    return t, y, w, xt


def _masked(out, j):
    """Entry j of a one-call fit's result, NaN where the status is not 0."""
    bad = torch.tensor([s != 0 for s in out[7]], dtype=torch.bool, device=out[0].device)
    return out[j].masked_fill(bad[:, None], float("nan"))


def _by_hand(ds, boot, fit, mu, x, sigma, y, w):
    """The composition of the public pieces that the one-call form documents: the replicas, a fit of every replica on its own
    -- with covariance for "student" --, the summary; then boot_student, or the delete-one weights, a fit per deleted row,
    boot_accel and boot_bca."""
    pois = isinstance(boot, PoissonBootstrap)
    pairs = not pois and boot.kind == B.PAIRS
    if pois:
        ystar, nbad = ds.boot_poisson(boot, mu, y, w)
        assert not nbad.any()
        wstar = None
    else:
        ystar, wstar = ds.boot_resample(boot, mu, y, w)
    outs = [fit(ystar[r], wstar[r] if pairs else w, boot.interval == "student") for r in range(boot.nrep)]
    xs = torch.stack([_masked(o, 0) for o in outs])
    lo, hi, mean, sd, nvalid = ds.boot_summary(xs, boot.level)
    if boot.interval == "student":
        sigs = torch.stack([_masked(o, 2) for o in outs])
        lo, hi, nvalid_t = ds.boot_student(xs, sigs, x, sigma, boot.level)
        return (lo, hi, mean, sd, nvalid, xs), dict(sigs=sigs, nvalid_t=nvalid_t)
    wj = ds.boot_jackknife(w, NDEC, MDEC)
    xjack = torch.stack([_masked(fit(y, wj[i], False), 0) for i in range(MDEC)])
    accel, njack = ds.boot_accel(xjack, w)
    lo, hi, z0, alo, ahi, flags, nv = ds.boot_bca(xs, x, accel, boot.level)
    assert torch.equal(nv, nvalid)
    return (lo, hi, mean, sd, nvalid, xs), dict(xjack=xjack, njack=njack, accel=accel, z0=z0, alpha_lo=alo, alpha_hi=ahi, flags=flags)


def _compare(got, want):
    assert len(got) == 7 and sorted(got[6]) == sorted(want[1])
    for g, w_, name in zip(got[:6], want[0], ("lo", "hi", "mean", "sd", "nvalid", "xs")):
        assert g.dtype == w_.dtype
        _same_or_nan(g.to(torch.float64), w_.to(torch.float64), name)
    for k, v in want[1].items():
        assert got[6][k].dtype == v.dtype and tuple(got[6][k].shape) == tuple(v.shape), k
        _same_or_nan(got[6][k].to(torch.float64), v.to(torch.float64), k)


@pytest.mark.parametrize("interval", ["student", "bca"])
@pytest.mark.parametrize("variant", ["plain", "bounds", "loss", "conv", "pairs"])
def test_one_call_is_the_composition(ds, monkeypatch, variant, interval):
    e = Expr(*DECAY)
    t, y, w, xt = _decays(61)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    conv = Convolve([0.2, 0.5, 0.3], origin=0, extend="hold")
    kw = {"plain": {}, "pairs": {}, "bounds": dict(lower=(0.0, 0.0, 3.0), upper=(100.0, 1.2, 10.0)),
          "loss": dict(loss=Loss("huber", list(np.linspace(2.0, 3.0, NDEC)))), "conv": dict(conv=conv)}[variant]
    x, _, sigma, *_ = ds.expr_fit_batch(e, dt, dy, _dev(ds, xt), weights=dw, **kw)
    boot = Bootstrap(nrep=5, kind="pairs" if variant == "pairs" else "residual", seed=81, level=0.8, interval=interval)
    mu = ds.expr_eval(e, x, dt)
    if variant == "conv":
        mu = ds.conv_apply(conv, mu)
    want = _by_hand(ds, boot, lambda ys, ws, cov: ds.expr_fit_batch(e, dt, ys, x, weights=ws, covariance=cov, **kw), mu, x, sigma, dy, dw)
    got = ds.expr_boot_batch(e, dt, dy, x, boot, weights=dw, sigma=sigma, **kw)
    _compare(got, want)
    assert tuple(got[5].shape) == (5, NDEC, 3) and int(got[4].max()) > 0
    if interval == "student":
        assert tuple(got[6]["sigs"].shape) == (5, NDEC, 3) and int(got[6]["nvalid_t"].max()) > 0
    else:
        assert tuple(got[6]["xjack"].shape) == (MDEC, NDEC, 3) and int(got[6]["njack"].max()) >= 2
        assert bool((got[6]["accel"] != 0).any())
    for reps in ("1", "3"):                                                     # however the replicas and the deletions are chunked
        monkeypatch.setenv("NLH_BOOT_REPS", reps)
        _compare(ds.expr_boot_batch(e, dt, dy, x, boot, weights=dw, sigma=sigma, **kw), want)


@pytest.mark.parametrize("interval", ["student", "bca"])
def test_poisson_one_call_is_the_composition(ds, monkeypatch, interval):
    t, y, w, xt = _decays(62, counts=True)
    tt = np.broadcast_to(t, y.shape).copy()                                     # a per-problem t: repeated per chunk
    dt, dy, dw = _dev(ds, tt), _dev(ds, y), _dev(ds, w)
    stat = Poisson()
    kw = dict(ncomp=1, baseline=0, stat=stat)
    x, _, sigma, *_ = ds.curve_fit_batch("expdecay", dt, dy, _dev(ds, xt), weights=dw, **kw)
    boot = PoissonBootstrap(5, seed=82, level=0.8, interval=interval)
    mu = ds.curve_eval("expdecay", x, dt, 1, 0)
    want = _by_hand(ds, boot, lambda ys, ws, cov: ds.curve_fit_batch("expdecay", dt, ys, x, weights=ws, covariance=cov, **kw), mu, x, sigma,
                    dy, dw)
    for reps in (None, "2"):
        if reps:
            monkeypatch.setenv("NLH_BOOT_REPS", reps)
        _compare(ds.curve_boot_batch("expdecay", dt, dy, x, boot, weights=dw, sigma=sigma, **kw), want)


def test_percentile_is_what_it_was(ds):
    """interval="percentile" -- the default -- returns the 6-tuple of before: the replicas, every replica's fit, the summary."""
    e = Expr(*DECAY)
    t, y, w, xt = _decays(63)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    x = ds.expr_fit_batch(e, dt, dy, _dev(ds, xt), weights=dw, covariance=False)[0]
    boot = Bootstrap(nrep=5, seed=83, level=0.8)
    got = ds.expr_boot_batch(e, dt, dy, x, boot, weights=dw)
    again = ds.expr_boot_batch(e, dt, dy, x, Bootstrap(nrep=5, seed=83, level=0.8, interval="percentile"), weights=dw, sigma=None)
    assert len(got) == len(again) == 6
    ystar, _ = ds.boot_resample(boot, ds.expr_eval(e, x, dt), dy, dw)
    xs = torch.stack([_masked(ds.expr_fit_batch(e, dt, ystar[r], x, weights=dw, covariance=False), 0) for r in range(5)])
    want = ds.boot_summary(xs, 0.8) + (xs,)
    for a, b, c in zip(got, again, want):
        _same_or_nan(a.to(torch.float64), c.to(torch.float64))
        _same_or_nan(b.to(torch.float64), c.to(torch.float64))
    bca = ds.expr_boot_batch(e, dt, dy, x, Bootstrap(nrep=5, seed=83, level=0.8, interval="bca"), weights=dw)
    for a, b in zip(bca[2:6], got[2:6]):                                        # mean, sd, nvalid and xs are the summary's under every interval
        _same_or_nan(a.to(torch.float64), b.to(torch.float64))


def test_bca_tails_of_ppnd16(ds):
    """xhat at the ranks 1, 5, 50 and 300 of 4096 replicas from either end: u down to 3/8192, where z0 goes through the device
    library's log and sqrt (ppnd16's branch r <= 5; the branch beyond needs u < 1.4e-11, which 4096 replicas cannot give)."""
    rng = np.random.default_rng(77)
    nrep, ranks = 4096, (1, 5, 50, 300, 4096 - 301, 4096 - 51, 4096 - 6, 4096 - 2)
    xs = rng.standard_normal((nrep, NPROB, len(ranks)))
    x = np.stack([np.sort(xs[:, p, :], axis=0)[ranks, np.arange(len(ranks))] for p in range(NPROB)])
    a = rng.uniform(-0.05, 0.05, x.shape)
    lo, hi, z0, alo, ahi, flags, nvalid = (_np(v) for v in ds.boot_bca(_dev(ds, xs), _dev(ds, x), _dev(ds, a), 0.95))
    want = R.bca(xs, x, a, 0.95)
    c2, cnt = R.bca_counts(xs, x)
    assert not flags.any() and (nvalid == nrep).all() and np.array_equal(c2, np.broadcast_to(2 * np.array(ranks) + 1, c2.shape))
    assert not any(R.central(u) for u in (c2 / (2.0 * nrep)).ravel())
    d = np.abs(z0 - want[2]) / np.abs(want[2])
    SEEN["z0_tail"] = max(SEEN["z0_tail"], float(d.max()))
    SEEN["alpha"] = max(SEEN["alpha"], float(np.abs(alo - want[3]).max()), float(np.abs(ahi - want[4]).max()))
    print("largest |alpha - restatement|", SEEN["alpha"], "largest relative z0 tail difference", SEEN["z0_tail"])
    assert (d <= Z0_TAIL_TOL).all() and (np.abs(alo - want[3]) <= ALPHA_TOL).all() and (np.abs(ahi - want[4]) <= ALPHA_TOL).all()
    given = R.bca(xs, x, a, 0.95, alphas=(alo, ahi))
    _same(lo, given[0])
    _same(hi, given[1])
