"""CPU tests of the bootstrap: the new entry points are declared, exported and bound; nlh_boot_draws -- host code -- against
tests/boot_restatement.py exactly; every refusal that needs no device; the restatement's quantile against numpy's and its sort
against a brute-force one; and the coverage study of the short-window decay on the CPU oracle's solver, recorded in
tests/golden/boot_study.json."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import boot_cases as BC
import boot_restatement as B
from nonlin_amd import Bootstrap
from nonlin_amd._lib import BOOT_SYMBOLS  # noqa: F401  (the feature: without it nothing here runs)

HERE = os.path.dirname(os.path.abspath(__file__))
NL_INVALID_INPUT_ERROR, NL_ARRAY_SIZE_ERROR, NLH_ERR_BAD_HANDLE = 201, 202, -3
NEW = ("nlh_boot_draws", "nlh_boot_resample_batch", "nlh_boot_summary_batch")


def _read(name):
    return open(os.path.join(os.path.dirname(HERE), "include", name)).read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_declared_exported_and_bound():
    from nonlin_amd import _lib
    import nonlin_amd
    L = _lib.load()
    assert '#include "nonlin_hip_boot.h"' in _read("nonlin_hip.h")            # who includes nonlin_hip.h has the entry points
    text = _read("nonlin_hip_boot.h")
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(nlh_[a-z0-9_]+)\s*\(", hdr))) == sorted(NEW) == sorted(_lib.BOOT_SYMBOLS)     # table and header agree
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == _lib.BOOT_SYMBOLS[name][1], name
        assert name not in _lib.SYMBOLS and name not in _lib.GUESS_SYMBOLS and name not in _lib.STARTS_SYMBOLS
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert (define("NLH_BOOT_MAX_ROWS"), define("NLH_BOOT_MAX_REP")) == (_lib.BOOT_MAX_ROWS, _lib.BOOT_MAX_REP) == \
        (B.MAX_ROWS, B.MAX_REP) == (16384, 4096)
    assert (define("NLH_BOOT_RESIDUAL"), define("NLH_BOOT_WILD"), define("NLH_BOOT_PAIRS")) == \
        (_lib.BOOT_RESIDUAL, _lib.BOOT_WILD, _lib.BOOT_PAIRS) == (B.RESIDUAL, B.WILD, B.PAIRS) == (0, 1, 2)
    assert _lib.BOOT_KINDS == B.KINDS
    assert nonlin_amd.Bootstrap is _lib.Bootstrap
    from nonlin_amd.device import DeviceSolver
    for name in ("boot_resample", "boot_summary", "curve_boot_batch", "expr_boot_batch"):
        assert callable(getattr(DeviceSolver, name))


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
def test_mix_spelled_out():
    """The restatement's uint64 arithmetic against Python integers mod 2^64."""
    M64 = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    g = 0x9E3779B97F4A7C15
    for seed, p, b, k in ((0, 0, 0, 0), (M64, 2 ** 40, 2 ** 31 - 1, 16383), (12345, 7, 3, 100)):
        key = mix((mix((seed + g * (p + 1)) & M64) + g * (b + 1)) & M64)
        z = mix((key + g * (k + 1)) & M64)
        assert int(B.key(seed, p, b)) == key and int(B.raw(seed, p, b, [k])[0]) == z
        assert int(B.index(B.raw(seed, p, b, [k]), 1000)[0]) == ((z >> 32) * 1000) >> 32


@pytest.mark.parametrize("cnt", [0, 1, 2, 3, 16384])
def test_draws_equal_the_restatement(cnt):
    for seed in (0, 20261027, (1 << 64) - 1):
        bt = Bootstrap(seed=seed)
        for p in (0, 1, 2 ** 31, 2 ** 62):
            for b in (0, 1, 4095, 2 ** 31 - 1):
                got = bt.draws(p, b, 0, 300, cnt)
                assert got.dtype == np.int32 and np.array_equal(got, B.draws(seed, p, b, 0, 300, cnt)), (seed, p, b)
                assert (got >= 0).all() and (got < max(cnt, 2)).all()
                part = bt.draws(p, b, 37, 101, cnt)                            # first != 0: the matching draws of the whole
                assert np.array_equal(part, got[37:138])
        last = bt.draws(3, 5, B.MAX_ROWS - 200, 200, cnt)                      # the last draws there are
        assert np.array_equal(last, B.draws(seed, 3, 5, B.MAX_ROWS - 200, 200, cnt))


def test_draws_fill_their_range():
    bt = Bootstrap(seed=5)
    whole = bt.draws(0, 0, 0, 16384, 16384)
    assert whole.min() < 10 and whole.max() > 16373
    frac = len(np.unique(whole)) / 16384.0                                      # with replacement: 1 - 1/e of the rows are drawn
    assert abs(frac - (1.0 - math.exp(-1.0))) < 0.02
    signs = bt.draws(0, 0, 0, 16384, 0)
    assert set(signs) == {0, 1} and abs(signs.mean() - 0.5) < 0.02
    assert sorted(set(bt.draws(0, 0, 0, 4000, 3))) == [0, 1, 2]
    assert Bootstrap(seed=-1).seed == (1 << 64) - 1                             # a seed is taken mod 2^64


def test_neighbouring_streams_differ():
    bt = Bootstrap(seed=0)
    base = bt.draws(10, 10, 0, 256, 16384)
    for p, b in ((11, 10), (10, 11), (9, 10), (10, 9), (11, 9), (9, 11)):      # (p + 1, b) is no shift of (p, b + 1) either
        other = bt.draws(p, b, 0, 256, 16384)
        assert (other == base).mean() < 0.05, (p, b)
    assert (Bootstrap(seed=1).draws(10, 10, 0, 256, 16384) == base).mean() < 0.05
    assert (bt.draws(10, 10, 1, 256, 16384)[:-1] == base[1:]).all()


def test_every_refusal_of_draws():
    from nonlin_amd import _lib
    L = _lib.load()
    out = np.full(64, 7, dtype=np.int32)

    def call(seed=1, p=0, b=0, first=0, count=4, cnt=10, null=False):
        return L.nlh_boot_draws(seed, p, b, first, count, cnt, None if null else out.ctypes.data_as(_lib.c_int32_p))
    assert call() == 0 and (out[:4] != 7).all() and (out[4:] == 7).all()
    out[:] = 7
    for bad in (dict(p=-1), dict(b=-1), dict(first=-1), dict(count=-1), dict(first=B.MAX_ROWS - 3), dict(first=2 ** 31 - 1, count=2 ** 31 - 1),
                dict(cnt=-1), dict(cnt=B.MAX_ROWS + 1), dict(null=True)):
        assert call(**bad) == NL_INVALID_INPUT_ERROR, bad
        assert (out == 7).all(), bad                                           # a refused call writes nothing
    assert call(first=B.MAX_ROWS - 4) == 0
    assert call(count=0, null=True) == 0
    bt = Bootstrap()
    assert bt.draws(-1, 0, 0, 1, 1) is None and bt.draws(0, 0, 0, 1, B.MAX_ROWS + 1) is None and bt.draws(2 ** 63, 0, 0, 1, 1) is None


def test_bootstrap_value_errors():
    bt = Bootstrap()
    assert (bt.nrep, bt.kind, bt.seed, bt.level, bt.centre, bt.name) == (200, B.RESIDUAL, 0, 0.95, True, "residual")
    assert Bootstrap(kind="WILD").kind == B.WILD and Bootstrap(kind=2).name == "pairs" and Bootstrap(nrep=B.MAX_REP).nrep == 4096
    for bad in (dict(kind="jackknife"), dict(kind=3), dict(kind=-1), dict(kind=True), dict(kind=1.0), dict(nrep=0), dict(nrep=B.MAX_REP + 1),
                dict(nrep=2.5), dict(nrep=True), dict(seed=1.5), dict(seed="a"), dict(level=0.0), dict(level=1.0), dict(level=math.nan),
                dict(level="0.9"), dict(level=None)):
        with pytest.raises(ValueError):
            Bootstrap(**bad)


def test_device_entry_points_refuse_without_a_device():
    """The refusals look at the arguments only: a block of zero bytes stands in for a handle, and nothing reads it."""
    from nonlin_amd import _lib
    L = _lib.load()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    buf = np.ones(4096)
    v = C.c_void_p(buf.ctypes.data)

    def res(h=fake, kind=0, nprob=1, prob0=0, m=8, rep0=0, nrep=2, mu=v, y=v, w=v, yout=v, wout=v):
        return L.nlh_boot_resample_batch(h, kind, 1, nprob, prob0, m, rep0, nrep, mu, y, w, 1, yout, wout)
    assert res(h=None) == NLH_ERR_BAD_HANDLE
    assert res(h=None, kind=9, m=0, y=None) == NLH_ERR_BAD_HANDLE              # the handle comes first
    for bad in (dict(kind=-1), dict(kind=3), dict(nprob=-1), dict(nrep=-1), dict(nrep=B.MAX_REP + 1), dict(m=0), dict(m=B.MAX_ROWS + 1),
                dict(prob0=-1), dict(rep0=-1), dict(rep0=2 ** 31 - 2), dict(y=None), dict(yout=None), dict(mu=None), dict(kind=1, mu=None),
                dict(kind=2, wout=None)):
        assert res(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert res(nprob=0) == res(nrep=0) == res(kind=2, mu=None, nprob=0) == res(wout=None, nrep=0) == 0     # nothing to do: no device

    def summ(h=fake, nrep=4, nprob=1, n=2, xs=v, level=0.95, outs=(v, v, v, v, v)):
        return L.nlh_boot_summary_batch(h, nrep, nprob, n, xs, level, *outs)
    assert summ(h=None) == summ(h=None, nrep=0, xs=None) == NLH_ERR_BAD_HANDLE
    for bad in (dict(nrep=0), dict(nrep=B.MAX_REP + 1), dict(nprob=-1), dict(n=0), dict(level=0.0), dict(level=1.0), dict(level=math.nan),
                dict(level=-0.5), dict(xs=None)) + tuple(dict(outs=tuple(None if i == k else v for i in range(5))) for k in range(5)):
        assert summ(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert summ(nprob=2 ** 30, n=2) == summ(nprob=2 ** 20, nrep=2048) == NL_ARRAY_SIZE_ERROR
    assert summ(nprob=0) == 0
    assert (buf == 1.0).all()


def test_one_call_refusals_without_a_device():
    """stat=, group= and pairs with conv=: refused before anything touches a device."""
    import torch
    from nonlin_amd import device, Expr
    from nonlin_amd._lib import Poisson, Convolve
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(device, "_chk", lambda *a, **k: None)
        ds = object.__new__(device.DeviceSolver)
        t, y = torch.zeros(16, dtype=torch.float64), torch.zeros((2, 16), dtype=torch.float64)
        x = torch.zeros((2, 3), dtype=torch.float64)
        e = Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
        cv = Convolve([0.25, 0.5, 0.25], origin=1)
        for call in (lambda **kw: ds.expr_boot_batch(e, t, y, x, **kw), lambda **kw: ds.curve_boot_batch("expdecay", t, y, x, baseline=0, **kw)):
            with pytest.raises(ValueError, match="excludes stat and group"):
                call(boot=Bootstrap(5), stat=Poisson())
            with pytest.raises(ValueError, match="excludes stat and group"):
                call(boot=Bootstrap(5, "wild"), group=object())
            with pytest.raises(ValueError, match='"pairs" excludes conv'):
                call(boot=Bootstrap(5, "pairs"), conv=cv)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_sort_against_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(200):
        cnt = int(rng.integers(1, 60))
        v = rng.integers(-3, 4, cnt).astype(np.float64)                         # many ties
        v[rng.random(cnt) < 0.3] = -0.0                                         # and zeros of both signs among them
        brute = sorted(range(cnt), key=lambda i: (v[i], i))                     # -0.0 == 0.0: the replica index decides
        assert np.array_equal(_bits(B.stable_sort(v)), _bits(v[brute]))


def test_quantile_against_numpy():
    rng = np.random.default_rng(12)
    for cnt in (1, 2, 3, 63, 64, 65, 200, 4096):
        v = np.sort(rng.standard_normal(cnt) * 10.0 ** rng.integers(-2, 3))
        for q in (0.0, 0.025, 0.05, 0.5, 0.95, 0.975, 1.0, float(rng.random())):
            got, want = B.quantile(v, q), np.percentile(v, 100.0 * q, method="linear")
            # the interpolation's terms are at most `scale`: a few roundings of that size; and numpy's position, q*100/100*(cnt-1),
            # carries two roundings more than q*(cnt-1): a few ulp of the position, times the slope there (at most `gap`)
            scale = max(abs(v[0]), abs(v[-1]))
            gap = np.diff(v).max() if cnt > 1 else 0.0
            assert abs(got - want) <= 4 * np.spacing(scale) + 4 * np.spacing(float(cnt)) * gap, (cnt, q)
            assert v[0] <= got <= v[-1]


def test_summary_spelled_out():
    xs = np.array([[[1.0, 5.0]], [[3.0, np.nan]], [[2.0, 4.0]], [[np.inf, 0.0]], [[0.0, 6.0]]])
    lo, hi, mean, sd, nvalid = B.summary(xs, 0.5)
    assert list(nvalid) == [3]                                                  # replicas 0, 2, 4: a row counts whole or not at all
    assert (mean[0, 0], mean[0, 1]) == (1.0, 5.0) and (sd[0, 0], sd[0, 1]) == (1.0, 1.0)
    assert (lo[0, 0], hi[0, 0], lo[0, 1], hi[0, 1]) == (0.5, 1.5, 4.5, 5.5)
    one = B.summary(xs[:2], 0.9)
    assert list(one[4]) == [1] and one[0][0, 0] == one[1][0, 0] == one[2][0, 0] == 1.0 and np.isnan(one[3]).all()
    none = B.summary(xs[1:2], 0.9)
    assert list(none[4]) == [0] and all(np.isnan(a).all() for a in none[:4])


def test_resample_spelled_out():
    """Each kind on a problem small enough to follow by hand from the draws."""
    seed, p, b = 9, 4, 2
    mu, y = np.array([1.0, 2.0, 3.0, 4.0, 5.0]), np.array([1.5, 1.0, 3.25, 4.0, 7.0])
    w = np.array([2.0, 0.0, 1.0, 4.0, 0.5])
    rows = [0, 2, 3, 4]
    j = B.draws(seed, p, b, 0, 4, 4)
    e = [w[i] * (y[i] - mu[i]) for i in rows]
    ys, ws = B.resample_one(B.RESIDUAL, seed, p, b, mu, y, w, False)
    assert ws is not None and np.array_equal(ws, w) and ys[1] == y[1]
    assert [ys[i] for i in rows] == [mu[i] + e[j[a]] / w[i] for a, i in enumerate(rows)]
    ys, _ = B.resample_one(B.RESIDUAL, seed, p, b, mu, y, w, True)
    part = np.zeros(64)
    for i, v in zip(rows, e):
        part[i % 64] = part[i % 64] + v
    off = 32
    while off:
        part[:off] = part[:off] + part[off:2 * off]
        off //= 2
    ebar = part[0] / 4.0
    assert [ys[i] for i in rows] == [mu[i] + (e[j[a]] - ebar) / w[i] for a, i in enumerate(rows)]
    sign = B.draws(seed, p, b, 0, 5, 0)
    ys, _ = B.resample_one(B.WILD, seed, p, b, mu, y, w, True)
    assert list(ys) == [y[i] if w[i] == 0.0 else (mu[i] - (y[i] - mu[i]) if sign[i] else mu[i] + (y[i] - mu[i])) for i in range(5)]
    ys, ws = B.resample_one(B.PAIRS, seed, p, b, None, y, w, True)
    c = np.bincount(j, minlength=4)
    assert np.array_equal(ys, y) and ws[1] == 0.0 and [ws[i] for i in rows] == [w[i] * np.sqrt(float(c[a])) for a, i in enumerate(rows)]
    ys, ws = B.resample_one(B.PAIRS, seed, p, b, None, y, None, True)
    j5 = B.draws(seed, p, b, 0, 5, 5)
    assert np.array_equal(ws, np.sqrt(np.bincount(j5, minlength=5).astype(np.float64))) and ws.sum() > 0
    for kind in (B.RESIDUAL, B.WILD, B.PAIRS):                                  # no active row: a copy of the data
        ys, ws = B.resample_one(kind, seed, p, b, mu, y, np.zeros(5), True)
        assert np.array_equal(_bits(ys), _bits(y)) and np.array_equal(ws, np.zeros(5))


# ---------------------------------------------------------------------------------------------------------------------
# the study
# ---------------------------------------------------------------------------------------------------------------------
def test_study(oracle):
    """Every data set of the study recomputed and compared with the golden file exactly.  No coverage is a condition: the file
    records what the intervals do on the oracle's solver, whatever it is."""
    rec = json.load(open(BC.STUDY_GOLDEN))
    assert (rec["seed"], rec["ndata"], rec["m"], rec["noise"], rec["nrep"], rec["level"], rec["boot_seed"], rec["max_evals"]) == \
        (BC.SEED, BC.NDATA, BC.M, BC.NOISE, BC.NREP, BC.LEVEL, BC.BOOT_SEED, BC.MAX_EVALS)
    assert sorted(rec["covered"]) == sorted(BC.ROWS)
    for row in BC.ROWS:
        for q in BC.PARAMS:
            s = rec["covered"][row][q]
            assert len(s) == BC.NDATA and set(s) <= {"0", "1"}, (row, q)
            c = s.count("1") / BC.NDATA
            assert rec["coverage"][row][q] == c and rec["stderr"][row][q] == math.sqrt(c * (1.0 - c) / BC.NDATA), (row, q)
    got, nvalid = BC.run_study(oracle)
    print({r: {q: sum(v) / BC.NDATA for q, v in got[r].items()} for r in BC.ROWS})
    for row in BC.ROWS:
        for q in BC.PARAMS:
            assert "".join(str(b) for b in got[row][q]) == rec["covered"][row][q], (row, q)
    assert {r: int(min(v)) for r, v in nvalid.items()} == rec["min_valid"]
