"""CPU tests of the Poisson bootstrap: the new entry points are declared, exported and bound; nlh_boot_poisson_draws -- host code
-- against tests/boot_pois_restatement.py exactly; every refusal that needs no device; the sampler's distribution against the
exact Poisson pmf; that a replica depends on (seed, problem, replica, mu) alone; and the coverage study on the CPU oracle's
solver, recorded in tests/golden/boot_pois_study.json."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import boot_pois_cases as BC
import boot_pois_restatement as BP
import boot_restatement as B
from nonlin_amd import PoissonBootstrap, Bootstrap
from nonlin_amd._lib import BOOT_POIS_SYMBOLS  # noqa: F401  (the feature: without it nothing here runs)

HERE = os.path.dirname(os.path.abspath(__file__))
NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3
NEW = ("nlh_boot_poisson_draws", "nlh_boot_poisson_batch")
TABLE_MU = (0.3, 1.0, 4.7, 50.5, 1000.25)                                     # the means of the issue's table up to 1000.25
GOOD_MU = (0.0, -0.0, 2.0 ** -20, 0.3, 1.0, 4.7, 50.5, 1000.25, 2.0 ** 24)
BAD_MU = (-1.0, math.nan, math.inf, 2.0 ** 24 + 2)
DIST_SEED, DIST_N = 20261103, 100000


def _read(name):
    return open(os.path.join(os.path.dirname(HERE), "include", name)).read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_declared_exported_and_bound():
    from nonlin_amd import _lib
    import nonlin_amd
    L = _lib.load()
    assert '#include "nonlin_hip_boot_pois.h"' in _read("nonlin_hip.h")       # who includes nonlin_hip.h has the entry points
    text = _read("nonlin_hip_boot_pois.h")
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(nlh_[a-z0-9_]+)\s*\(", hdr))) == sorted(NEW) == sorted(_lib.BOOT_POIS_SYMBOLS)
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == _lib.BOOT_POIS_SYMBOLS[name][1], name
        assert all(name not in tab for tab in (_lib.SYMBOLS, _lib.GUESS_SYMBOLS, _lib.STARTS_SYMBOLS, _lib.BOOT_SYMBOLS, _lib.BIN_SYMBOLS))
    assert int(re.search(r"#define\s+NLH_BOOT_POIS_MAX_MEAN\s+(\d+)", text).group(1)) == _lib.BOOT_POIS_MAX_MEAN == BP.MAX_MEAN == 2 ** 24
    assert nonlin_amd.PoissonBootstrap is _lib.PoissonBootstrap
    from nonlin_amd.device import DeviceSolver
    assert callable(DeviceSolver.boot_poisson)


# ---------------------------------------------------------------------------------------------------------------------
# the host function
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", GOOD_MU)
def test_draws_equal_the_restatement(mu):
    count = 40 if mu > 2.0 ** 20 else 300
    a = np.full(count, mu)
    streams = ((0, 0, 0, 0), (20261103, 2 ** 40 + 5, 2 ** 31 - 1, 37), ((1 << 64) - 1, 3, 4095, B.MAX_ROWS - count))
    for seed, p, b, first in streams[1:2] if mu > 2.0 ** 20 else streams:      # (the restatement's setup of 2^24 takes a second)
        got = PoissonBootstrap(seed=seed).draws(p, b, first, a)
        want = BP.draws(seed, p, b, first, a)
        assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(want)), (mu, seed, p, b, first)
        assert (got >= 0.0).all() and (got == np.floor(got)).all() and not np.signbit(got).any()
        if mu == 0.0 or mu == 2.0 ** -20:
            assert (got == 0.0).all()                                          # (2^-20: one draw in a million is not 0)
    whole = PoissonBootstrap(seed=5).draws(7, 3, 0, np.full(count, mu))
    part = PoissonBootstrap(seed=5).draws(7, 3, 11, np.full(count - 11, mu))  # first != 0: the matching draws of the whole
    assert np.array_equal(_bits(part), _bits(whole[11:]))


def test_draws_of_mixed_and_bad_means():
    mu = np.array(GOOD_MU[:-1] + BAD_MU + (3.0, 17.5, 255.999, 2.0 ** -1074, 1e-300))
    got = PoissonBootstrap(seed=9).draws(4, 2, 100, mu)
    want = BP.draws(9, 4, 2, 100, mu)
    assert np.array_equal(np.isnan(got), BP.bad_mean(mu)) and np.isnan(got).sum() == len(BAD_MU)
    ok = ~np.isnan(got)
    assert np.array_equal(_bits(got[ok]), _bits(want[ok])) and np.isnan(want[~ok]).all()
    # a row's draw is its own: the same mean at the same row of the same stream, whatever the other rows hold
    alone = PoissonBootstrap(seed=9).draws(4, 2, 100 + 7, mu[7:8])
    assert _bits(alone)[0] == _bits(got)[7]


def test_every_refusal_of_draws():
    from nonlin_amd import _lib
    L = _lib.load()
    dp = _lib.c_double_p
    mu, out = np.full(64, 4.7), np.full(64, -7.25)

    def call(seed=1, p=0, b=0, first=0, count=4, null_mu=False, null_out=False):
        return L.nlh_boot_poisson_draws(seed, p, b, first, count, None if null_mu else mu.ctypes.data_as(dp),
                                        None if null_out else out.ctypes.data_as(dp))
    assert call() == 0 and (out[:4] != -7.25).all() and (out[4:] == -7.25).all()
    out[:] = -7.25
    for bad in (dict(p=-1), dict(b=-1), dict(first=-1), dict(count=-1), dict(first=B.MAX_ROWS - 3), dict(first=2 ** 31 - 1, count=2 ** 31 - 1),
                dict(null_mu=True), dict(null_out=True)):
        assert call(**bad) == NL_INVALID_INPUT_ERROR, bad
        assert (out == -7.25).all(), bad                                       # a refused call writes nothing
    assert call(first=B.MAX_ROWS - 4) == 0
    assert call(count=0, null_mu=True, null_out=True) == 0
    bt = PoissonBootstrap()
    assert bt.draws(-1, 0, 0, [1.0]) is None and bt.draws(0, -1, 0, [1.0]) is None and bt.draws(2 ** 63, 0, 0, [1.0]) is None
    assert bt.draws(0, 0, B.MAX_ROWS, [1.0]) is None and bt.draws(0, 0, 0, [[1.0]]) is None and bt.draws(0, 0, 0, "a") is None


def test_poisson_bootstrap_value_errors():
    bt = PoissonBootstrap()
    assert (bt.nrep, bt.seed, bt.level) == (200, 0, 0.95)
    assert PoissonBootstrap(nrep=B.MAX_REP).nrep == 4096 and PoissonBootstrap(seed=-1).seed == (1 << 64) - 1
    for bad in (dict(nrep=0), dict(nrep=B.MAX_REP + 1), dict(nrep=2.5), dict(nrep=True), dict(seed=1.5), dict(seed="a"), dict(level=0.0),
                dict(level=1.0), dict(level=math.nan), dict(level="0.9"), dict(level=None)):
        with pytest.raises(ValueError, match="PoissonBootstrap"):
            PoissonBootstrap(**bad)
    with pytest.raises(TypeError):
        PoissonBootstrap(kind="wild")                                          # a class of its own: it has no kinds
    for bad in (dict(kind=3), dict(kind="poisson")):                           # and Bootstrap has no fourth
        with pytest.raises(ValueError):
            Bootstrap(**bad)


def test_device_entry_point_refuses_without_a_device():
    """The refusals look at the arguments only: a block of zero bytes stands in for a handle, and nothing reads it."""
    from nonlin_amd import _lib
    L = _lib.load()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    buf = np.ones(4096)
    v = C.c_void_p(buf.ctypes.data)

    def res(h=fake, nprob=1, prob0=0, m=8, rep0=0, nrep=2, mu=v, y=v, w=v, yout=v, bad=v):
        return L.nlh_boot_poisson_batch(h, 1, nprob, prob0, m, rep0, nrep, mu, y, w, yout, bad)
    assert res(h=None) == NLH_ERR_BAD_HANDLE
    assert res(h=None, m=0, y=None) == NLH_ERR_BAD_HANDLE                      # the handle comes first
    for bad in (dict(nprob=-1), dict(nrep=-1), dict(nrep=B.MAX_REP + 1), dict(m=0), dict(m=B.MAX_ROWS + 1), dict(prob0=-1), dict(rep0=-1),
                dict(rep0=2 ** 31 - 2), dict(mu=None), dict(y=None), dict(yout=None), dict(bad=None)):
        assert res(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert res(nprob=0) == res(nrep=0) == res(nrep=0, w=None) == 0              # nothing to do: no device
    assert (buf == 1.0).all()
    # the resampling entry point keeps refusing a fourth kind
    assert L.nlh_boot_resample_batch(fake, 3, 1, 1, 0, 8, 0, 2, v, v, v, 1, v, v) == NL_INVALID_INPUT_ERROR


def test_one_call_refusals_without_a_device():
    """A PoissonBootstrap without stat= or with group=, and a plain Bootstrap with stat=: refused before anything touches a
    device."""
    import torch
    from nonlin_amd import device, Expr
    from nonlin_amd._lib import Poisson
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(device, "_chk", lambda *a, **k: None)
        ds = object.__new__(device.DeviceSolver)
        t, y = torch.zeros(16, dtype=torch.float64), torch.zeros((2, 16), dtype=torch.float64)
        x = torch.zeros((2, 3), dtype=torch.float64)
        e = Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
        for call in (lambda **kw: ds.expr_boot_batch(e, t, y, x, **kw), lambda **kw: ds.curve_boot_batch("expdecay", t, y, x, baseline=0, **kw)):
            with pytest.raises(ValueError, match="PoissonBootstrap needs stat"):
                call(boot=PoissonBootstrap(5))
            with pytest.raises(ValueError, match="PoissonBootstrap excludes group"):
                call(boot=PoissonBootstrap(5), stat=Poisson(), group=object())
            with pytest.raises(ValueError, match="excludes stat and group: counts need a parametric sampler, a group its own resampling"):
                call(boot=Bootstrap(5), stat=Poisson())
            with pytest.raises(ValueError, match="excludes stat and group"):
                call(boot=Bootstrap(5, "wild"), group=object())


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _sample(mu):
    """DIST_N draws of the mean mu from the restatement: the rows 0 .. 16383 of the replicas 0, 1, .. of problem 0."""
    nrep = -(-DIST_N // B.MAX_ROWS)
    ys, bad = BP.poisson(DIST_SEED, np.full((1, B.MAX_ROWS), mu), np.zeros((1, B.MAX_ROWS)), None, nrep)
    assert bad[0] == 0
    return ys.reshape(-1)[:DIST_N]


@pytest.mark.parametrize("mu", TABLE_MU)
def test_distribution(mu):
    """Chi-square of 100,000 draws against scipy's exact pmf over bins of expectation >= 10 -- the k whose own expectation is
    at least 10, the lowest and the highest of them taking their tail (the pmf is unimodal, so every bin between has it, too).
    Deterministic: the seed is fixed; p >= 1e-3 is asked."""
    from scipy import stats
    d = _sample(mu)
    assert (d >= 0.0).all() and (d == np.floor(d)).all()                       # every drawn value is a non-negative integer
    ks = np.arange(0, int(max(d.max(), mu + 20 * math.sqrt(mu) + 20)) + 1)
    e = stats.poisson.pmf(ks, mu) * DIST_N
    big = np.flatnonzero(e >= 10.0)
    lo, hi = big[0], big[-1]
    assert (e[lo:hi + 1] >= 10.0).all()
    obs = np.bincount(d.astype(np.int64), minlength=len(ks)).astype(np.float64)
    O = np.concatenate([[obs[:lo + 1].sum()], obs[lo + 1:hi], [obs[hi:].sum()]])
    E = np.concatenate([[stats.poisson.cdf(lo, mu) * DIST_N], e[lo + 1:hi], [stats.poisson.sf(hi - 1, mu) * DIST_N]])
    assert O.sum() == DIST_N and abs(E.sum() - DIST_N) < 1e-6 * DIST_N and (E >= 10.0).all()
    chi2, df = float(((O - E) ** 2 / E).sum()), len(O) - 1
    pval = float(stats.chi2.sf(chi2, df))
    print(f"mu = {mu}: chi-square {chi2:.1f} / {df}, p = {pval:.4f}, mean {d.mean():.4f}")
    assert pval >= 1e-3, (mu, chi2, df, pval)
    assert abs(d.mean() - mu) < 5.0 * math.sqrt(mu / DIST_N)


def test_tiny_mean():
    d = _sample(2.0 ** -20)
    assert set(np.unique(d)) <= {0.0, 1.0} and d.sum() <= 3                    # 0.095 expected in 100,000 draws


def test_setup_against_the_exact_weights():
    """T q_k-sums are the pmf's: L / T = P(X < M) and 1 / T = P(X = M) to rounding, and the walks' ends hold the tails above
    EPS."""
    from scipy import stats
    mu = np.array([0.3, 1.0, 4.7, 50.5, 1000.25, 30000.5])
    M, L, T, kmin, kmax, r = BP.setup(mu)
    assert np.array_equal(M, np.floor(mu)) and (kmin >= 0.0).all() and (kmin <= M).all() and (kmax >= M).all()
    np.testing.assert_allclose(1.0 / T, stats.poisson.pmf(M, mu), rtol=1e-9)
    np.testing.assert_allclose(L / T, stats.poisson.cdf(M - 1, mu), rtol=1e-9, atol=1e-15)
    assert (stats.poisson.sf(kmax, mu) < 1e-15).all() and (stats.poisson.cdf(kmin - 1, mu) < 1e-15).all()


def test_a_replica_depends_on_its_own_key_and_mean_alone():
    """Not on the batch, the slice (prob0, rep0) or the chunking: the whole against its parts, and against the host function."""
    rng = np.random.default_rng(5)
    nprob, m, nrep = 4, 37, 9
    mu = rng.choice([2.0 ** -20, 0.3, 1.0, 4.7, 50.5, 1000.25], (nprob, m)) * rng.uniform(0.9, 1.1, (nprob, m))
    y = rng.poisson(mu).astype(np.float64)
    w = np.where(rng.random((nprob, m)) < 0.2, 0.0, 1.0)
    mu[1, 3], mu[1, 4], mu[2, 5] = 0.0, -0.0, -1.0
    w[1, 3], w[1, 4], y[1, 3], y[1, 4] = 1.0, 1.0, 2.0, 2.0                    # zero rows: active, and their data is not 0
    w[2, 5], w[3, 6], mu[3, 6] = 1.0, 0.0, math.nan                            # a bad row, and a bad mean on an inactive one
    whole, bad = BP.poisson(7, mu, y, w, nrep)
    assert list(bad) == [0, 0, 1, 0]
    assert (whole[:, w == 0.0] == y[w == 0.0]).all() and (whole[:, 2, 5] == y[2, 5]).all()
    assert (whole[:, 1, 3:5] == 0.0).all() and not np.signbit(whole[:, 1, 3:5]).any()
    for prob0, np_, rep0, nr in ((1, 2, 0, 9), (0, 4, 5, 4), (3, 1, 8, 1), (2, 2, 2, 3)):
        sl = slice(prob0, prob0 + np_)
        part, pbad = BP.poisson(7, mu[sl], y[sl], w[sl], nr, prob0=prob0, rep0=rep0)
        assert np.array_equal(_bits(part), _bits(whole[rep0:rep0 + nr, sl])) and np.array_equal(pbad, bad[sl])
    chunks = np.concatenate([BP.poisson(7, mu, y, w, r, rep0=r0)[0] for r0, r in ((0, 2), (2, 3), (5, 4))])
    assert np.array_equal(_bits(chunks), _bits(whole))
    one, b1 = BP.poisson_one(7, 2, 6, mu[2], y[2], w[2])
    assert np.array_equal(_bits(one), _bits(whole[6, 2])) and b1 == 1
    host = PoissonBootstrap(seed=7).draws(0, 4, 0, mu[0])                      # the host function: every row as if active
    act = w[0] != 0.0
    assert np.array_equal(_bits(host[act]), _bits(whole[4, 0, act]))
    nw, _ = BP.poisson(7, mu[:1], y[:1], None, 5)                              # without weights every row is active
    assert np.array_equal(_bits(nw[4, 0]), _bits(host))


# ---------------------------------------------------------------------------------------------------------------------
# the study
# ---------------------------------------------------------------------------------------------------------------------
def test_study(oracle):
    """The golden file is consistent with itself, and a subset of its data sets, recomputed, gives the recorded bits.  No
    coverage is a condition: the file records what the intervals do on the oracle's solver, whatever it is."""
    rec = json.load(open(BC.STUDY_GOLDEN))
    assert (rec["seed"], rec["ndata"], rec["m"], rec["nrep"], rec["level"], rec["boot_seed"]) == \
        (BC.PC.SEED, BC.NDATA, BC.M, BC.NREP, BC.LEVEL, BC.BOOT_SEED)
    assert [tuple(v) for v in rec["truths"]] == list(BC.TRUTHS) and len(rec["study"]) == 2
    for ti, s in enumerate(rec["study"]):
        for row in BC.ROWS:
            for q in BC.PARAMS:
                bits = s["covered"][row][q]
                assert len(bits) == BC.NDATA and set(bits) <= {"0", "1"}, (ti, row, q)
                c = bits.count("1") / BC.NDATA
                assert s["coverage"][row][q] == c and s["stderr"][row][q] == math.sqrt(c * (1.0 - c) / BC.NDATA), (ti, row, q)
        for q in BC.PARAMS:
            v = [float.fromhex(h) for h in s["ratio"][q]]
            for name, k in (("median_ratio", BC.NDATA), ("median_ratio_first%d" % BC.NGPU, BC.NGPU)):
                med, se = BC.median_stderr(v[:k])
                assert (s[name][q]["median"], s[name][q]["stderr"]) == (med, se), (ti, q, name)
        assert len(s["nvalid"]) == BC.NDATA and s["min_valid"] == min(s["nvalid"])
        data = BC.problems(ti)
        for p in (0, 1, 150, 299):
            got = BC.one(oracle, ti, p, data)
            for j, q in enumerate(BC.PARAMS):
                for row in BC.ROWS:
                    assert str(got[row][j]) == s["covered"][row][q][p], (ti, p, row, q)
                assert float(got["ratio"][j]).hex() == s["ratio"][q][p], (ti, p, q)
            assert got["nvalid"] == s["nvalid"][p]
