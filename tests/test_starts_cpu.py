"""CPU tests of starts: the new entry points are declared, exported and bound; nlh_starts_candidates -- host code -- against
tests/starts_restatement.py (linear dimensions bit for bit, log dimensions within 4 ulp of numpy's expression: the host's libm
and numpy's exp / log are each within an ulp or so of the true value, and one multiplication follows); every refusal without a
device; the restatement's selection against a brute-force sort; and the study of the sinusoid family on the CPU oracle's
solver, recorded in tests/golden/starts_study.json."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import starts_cases as SC
import starts_restatement as S
from nonlin_amd import Starts, Expr
from nonlin_amd._lib import STARTS_SYMBOLS  # noqa: F401  (the feature: without it nothing here runs)

HERE = os.path.dirname(os.path.abspath(__file__))
NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3
NEW = ("nlh_starts_candidates", "nlh_starts_search_batch_device", "nlh_starts_search_batch_device_h", "nlh_starts_cost_batch",
       "nlh_starts_pick_batch", "nlh_starts_take_batch")


def _read(name):
    return open(os.path.join(os.path.dirname(HERE), "include", name)).read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_declared_exported_and_bound():
    from nonlin_amd import _lib
    import nonlin_amd
    L = _lib.load()
    assert '#include "nonlin_hip_starts.h"' in _read("nonlin_hip.h")          # who includes nonlin_hip.h has the entry points
    text = _read("nonlin_hip_starts.h")
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(nlh_[a-z0-9_]+)\s*\(", hdr))) == sorted(NEW) == sorted(_lib.STARTS_SYMBOLS)   # table and header agree
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == _lib.STARTS_SYMBOLS[name][1], name
        assert name not in _lib.SYMBOLS and name not in _lib.GUESS_SYMBOLS
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert (define("NLH_STARTS_MAX_N"), define("NLH_STARTS_MAX_KEEP"), define("NLH_STARTS_MAX_CAND")) == \
        (_lib.STARTS_MAX_N, _lib.STARTS_MAX_KEEP, _lib.STARTS_MAX_CAND) == (S.MAX_N, S.MAX_KEEP, S.MAX_CAND) == (32, 8, 1 << 20)
    assert nonlin_amd.Starts is _lib.Starts
    from nonlin_amd.device import DeviceSolver
    for name in ("starts_search", "starts_cost", "starts_pick", "starts_take"):
        assert callable(getattr(DeviceSolver, name))


# ---------------------------------------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------------------------------------
def _box(n, seed=0):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-5.0, 5.0, n)
    return lo, lo + rng.uniform(0.5, 20.0, n)


def test_candidate_zero():
    from nonlin_amd import Starts
    got = Starts(np.zeros(32), np.ones(32), ncand=1).candidates()
    assert np.array_equal(_bits(got[0]), _bits([np.float64(1.0) / np.float64(p) for p in S.PRIMES]))


@pytest.mark.parametrize("n", [1, 2, 32])
def test_linear_dimensions_bit_for_bit(n):
    from nonlin_amd import Starts
    lo, hi = _box(n, n)
    st = Starts(lo, hi, ncand=300)
    want = S.candidates(lo, hi, (), 0, 300)
    assert np.array_equal(_bits(st.candidates()), _bits(want))
    assert ((want >= lo) & (want <= hi)).all()
    part = st.candidates(first=37, count=101)                                 # first != 0: the matching rows of the whole
    assert np.array_equal(_bits(part), _bits(want[37:138]))


def test_crossing_a_power_of_each_base():
    """i = c + 1 around p^k gains a digit: the candidates c = p^k - 3 .. p^k + 1 of dimension d, for every base."""
    from nonlin_amd import Starts
    lo, hi = _box(32, 5)
    st = Starts(lo, hi)
    for d, p in enumerate(S.PRIMES):
        k = 1
        while p ** (k + 1) + 2 <= S.MAX_CAND:
            k += 1
        for e in sorted({1, 2, k}):
            if p ** e + 2 > S.MAX_CAND:
                continue
            first = max(p ** e - 3, 0)
            got = st.candidates(first=first, count=5)[:, d]
            want = np.array([lo[d] + S.radical_inverse(c + 1, p) * (hi[d] - lo[d]) for c in range(first, first + 5)])
            assert np.array_equal(_bits(got), _bits(want)), (p, e)
    last = st.candidates(first=S.MAX_CAND - 2, count=2)                        # the last candidates there are
    assert np.array_equal(_bits(last), _bits(S.candidates(lo, hi, (), S.MAX_CAND - 2, 2)))


def test_log_dimensions():
    from nonlin_amd import Starts
    lo, hi = np.array([0.1, 1e-6, 3.0, 2.0]), np.array([10.0, 1e6, 3.5, 7.0])
    st = Starts(lo, hi, ncand=2000, log=(0, 1, 2))
    got = st.candidates()
    want = S.candidates(lo, hi, (0, 1, 2), 0, 2000)
    assert ((got >= lo) & (got <= hi)).all()
    assert np.array_equal(_bits(got[:, 3]), _bits(want[:, 3]))                # the linear one among them: bits
    u = S.unit(0, 2000, 3)
    for d in range(3):
        order = np.argsort(u[:, d], kind="stable")
        assert (np.diff(u[order, d]) > 0).all() and (np.diff(got[order, d]) > 0).all(), d     # strictly monotone in u
        ulp = np.spacing(np.abs(want[:, d]))
        assert (np.abs(got[:, d] - want[:, d]) <= 4 * ulp).all(), d
    assert np.array_equal(_bits(st.candidates(first=500, count=7)), _bits(got[500:507]))


def test_degenerate_dimension_and_positions():
    from nonlin_amd import Starts
    st = Starts((1.0, 2.5, -1.0), (3.0, 2.5, 4.0), ncand=50, log=(0,))
    got = st.candidates()
    assert (got[:, 1] == 2.5).all()
    sub = st.candidates(positions=(2, 0))                                      # dimension d of a subset scan is positions[d]
    assert np.array_equal(_bits(sub), _bits(Starts((-1.0, 1.0), (4.0, 3.0), ncand=50, log=(1,)).candidates()))
    with pytest.raises(ValueError):
        st.box(positions=(0, 0))
    with pytest.raises(ValueError):
        st.box(positions=(3,))


def test_every_refusal_of_candidates():
    from nonlin_amd import _lib
    L = _lib.load()
    out = np.full(64 * 33, 7.0)

    def call(n=2, first=0, count=4, lo=(0.5, 1.0), hi=(2.0, 3.0), lg=(0, 0), null=()):
        lo, hi, lg = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64), np.array(lg, dtype=np.int32)
        ptr = lambda a, t, name: None if name in null else a.ctypes.data_as(t)
        return L.nlh_starts_candidates(n, first, count, ptr(lo, _lib.c_double_p, "lo"), ptr(hi, _lib.c_double_p, "hi"),
                                       ptr(lg, _lib.c_int32_p, "lg"), ptr(out, _lib.c_double_p, "out"))
    assert call() == 0 and (out[:8] != 7.0).all() and (out[8:] == 7.0).all()
    out[:] = 7.0
    big = np.ones(33)
    for bad in (dict(n=0), dict(n=-1), dict(n=33, lo=big, hi=big, lg=np.zeros(33)), dict(lo=(math.nan, 1.0)), dict(hi=(2.0, math.inf)),
                dict(lo=(-math.inf, 1.0)), dict(lo=(2.5, 1.0)), dict(lg=(0, 1), lo=(0.5, 0.0)), dict(lg=(1, 0), lo=(-1.0, 1.0)),
                dict(count=-1), dict(first=-1), dict(first=S.MAX_CAND - 3), dict(first=2 ** 31 - 1, count=2 ** 31 - 1),
                dict(null=("lo",)), dict(null=("hi",)), dict(null=("out",))):
        assert call(**bad) == NL_INVALID_INPUT_ERROR, bad
        assert (out == 7.0).all(), bad                                         # a refused call writes nothing
    assert call(null=("lg",)) == 0                                             # no logscale: every dimension linear
    assert call(first=S.MAX_CAND - 4) == 0
    assert call(count=0, null=("out",)) == 0
    assert call(n=2, lo=(1.0, 1.0), hi=(1.0, 3.0)) == 0                        # lo == hi is allowed


def test_starts_value_errors():
    from nonlin_amd import Starts, Expr
    ok = dict(lower=(0.5, 1.0), upper=(2.0, 3.0))
    Starts(**ok, ncand=S.MAX_CAND, keep=8, log=(0, 1))
    for bad in (dict(lower=(0.5,)), dict(lower=(), upper=()), dict(lower=np.ones(33), upper=np.ones(33)), dict(lower=(math.nan, 1.0)),
                dict(upper=(math.inf, 3.0)), dict(lower=(2.5, 1.0)), dict(lower=(0.0, 1.0), log=(0,)), dict(log=(2,)), dict(log=(-1,)),
                dict(log=("a",)), dict(ncand=0), dict(ncand=S.MAX_CAND + 1), dict(ncand=2.5), dict(keep=0), dict(keep=9),
                dict(ncand=4, keep=5), dict(keep=True), dict(lower="ab")):
        with pytest.raises(ValueError):
            Starts(**dict(ok, **bad))
    st = Starts(**ok, ncand=10)
    for bad in (dict(first=-1), dict(count=-1), dict(first=S.MAX_CAND, count=1)):
        with pytest.raises(ValueError):
            st.candidates(**bad)
    e = Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
    se = Starts.for_expr(e, lower={"a": 1.0, "k": 0.01, "c": -1.0}, upper={"c": 1.0, "a": 5.0, "k": 100.0}, ncand=32, keep=2, log=("k",))
    assert se.n == 3 and list(se.lower) == [1.0, 0.01, -1.0] and list(se.upper) == [5.0, 100.0, 1.0] and list(se.logscale) == [0, 1, 0]
    assert np.array_equal(_bits(se.candidates()), _bits(Starts((1.0, 0.01, -1.0), (5.0, 100.0, 1.0), 32, 2, log=(1,)).candidates()))
    for bad in (dict(lower={"a": 1.0, "k": 0.01}), dict(upper={"a": 5.0, "k": 1.0, "c": 1.0, "z": 2.0}), dict(log=("q",))):
        with pytest.raises(ValueError):
            Starts.for_expr(e, **dict(dict(lower={"a": 1.0, "k": 0.01, "c": -1.0}, upper={"c": 1.0, "a": 5.0, "k": 100.0}), **bad))


def test_device_entry_points_refuse_without_a_device():
    """The refusals look at the arguments only: a block of zero bytes stands in for a handle, and nothing reads it."""
    from nonlin_amd import _lib
    L = _lib.load()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    lo, hi, lg = np.array([0.5, 1.0]), np.array([2.0, 3.0]), np.zeros(2, dtype=np.int32)
    buf = np.ones(4096)
    v = C.c_void_p(buf.ctypes.data)
    fcn = C.cast(L.nlh_curve_device_fcn, _lib.DEVFCN)
    none = C.cast(None, _lib.DEVFCN)
    dp, ip = lambda a: a.ctypes.data_as(_lib.c_double_p), lambda a: a.ctypes.data_as(_lib.c_int32_p)
    for fn, outs in ((L.nlh_starts_search_batch_device, (v, v, v)),
                     (L.nlh_starts_search_batch_device_h, (dp(buf), dp(buf), ip(np.zeros(64, dtype=np.int32))))):
        def call(h=fake, nprob=1, m=8, n=2, f=fcn, xl=lo, xu=hi, ls=lg, ncand=16, keep=2, out=outs):
            return fn(h, nprob, m, n, f, None, dp(xl) if xl is not None else None, dp(xu) if xu is not None else None,
                      ip(ls) if ls is not None else None, ncand, keep, *out)
        assert call(h=None) == NLH_ERR_BAD_HANDLE
        assert call(h=None, n=0, f=none, keep=0) == NLH_ERR_BAD_HANDLE          # the handle comes first
        for bad in (dict(f=none), dict(xl=None), dict(xu=None), dict(nprob=-1), dict(m=0), dict(n=0), dict(n=33), dict(ncand=0),
                    dict(ncand=S.MAX_CAND + 1), dict(keep=0), dict(keep=9), dict(ncand=4, keep=5), dict(xl=np.array([0.5, math.nan])),
                    dict(xl=np.array([2.5, 1.0])), dict(xl=np.array([0.0, 1.0]), ls=np.array([1, 0], dtype=np.int32)),
                    dict(out=(None, outs[1], outs[2])), dict(out=(outs[0], None, outs[2])), dict(out=(outs[0], outs[1], None))):
            assert call(**bad) == NL_INVALID_INPUT_ERROR, bad
        assert call(nprob=0) == 0                                               # nothing to do: no device is touched
    assert (buf == 1.0).all()
    cost, pick, take = L.nlh_starts_cost_batch, L.nlh_starts_pick_batch, L.nlh_starts_take_batch
    assert cost(None, 1, 1, v, v) == pick(None, 1, 1, v, v) == take(None, 1, 1, 1, v, v, v) == NLH_ERR_BAD_HANDLE
    for rc in (cost(fake, -1, 1, v, v), cost(fake, 1, 0, v, v), cost(fake, 1, 1, None, v), cost(fake, 1, 1, v, None),
               pick(fake, -1, 1, v, v), pick(fake, 1, 0, v, v), pick(fake, 1, 9, v, v), pick(fake, 1, 1, None, v), pick(fake, 1, 1, v, None),
               take(fake, -1, 1, 1, v, v, v), take(fake, 1, 0, 1, v, v, v), take(fake, 1, 9, 1, v, v, v), take(fake, 1, 1, 0, v, v, v),
               take(fake, 1, 1, 1, None, v, v), take(fake, 1, 1, 1, v, None, v), take(fake, 1, 1, 1, v, v, None)):
        assert rc == NL_INVALID_INPUT_ERROR
    assert cost(fake, 0, 1, v, v) == pick(fake, 0, 1, v, v) == take(fake, 0, 1, 1, v, v, v) == 0


def test_fit_refusals_without_a_device():
    """starts with an x0, with pmap or group, or with a box of another length: refused before anything touches a device."""
    import torch
    from nonlin_amd import device, Starts, Expr
    from nonlin_amd._lib import ParamMap
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(device, "_chk", lambda *a, **k: None)
        ds = object.__new__(device.DeviceSolver)
        t, y = torch.zeros(16, dtype=torch.float64), torch.zeros((2, 16), dtype=torch.float64)
        s4, s3 = Starts(np.zeros(4), np.ones(4)), Starts(np.zeros(3), np.ones(3))
        e = Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
        with pytest.raises(ValueError, match="starts excludes x0"):
            ds.curve_fit_batch("gauss", t, y, torch.zeros((2, 4), dtype=torch.float64), baseline=0, starts=s4)
        with pytest.raises(ValueError, match="starts excludes x0"):
            ds.expr_fit_batch(e, t, y, torch.zeros((2, 3), dtype=torch.float64), starts=s3)
        with pytest.raises(ValueError, match="starts excludes pmap and group"):
            ds.curve_fit_batch("gauss", t, y, None, baseline=0, pmap=ParamMap(4, fixed=[3]), starts=s4)
        with pytest.raises(ValueError, match="starts excludes pmap and group"):
            ds.expr_fit_batch(e, t, y, None, group=object(), starts=s3)
        with pytest.raises(ValueError, match="a box over 3 parameters, the model has 4"):
            ds.curve_fit_batch("gauss", t, y, None, baseline=0, starts=s3)
        with pytest.raises(ValueError, match="a box over 4 parameters, the model has 3"):
            ds.expr_fit_batch(e, t, y, None, starts=s4)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_cost_order_spelled_out():
    rng = np.random.default_rng(3)
    for m in (1, 63, 64, 65, 200):
        F = rng.standard_normal((3, m)) * 10.0 ** rng.integers(-3, 3, (3, m))
        for q in range(3):
            part = [0.0] * 64
            for i in range(m):
                part[i % 64] = part[i % 64] + F[q, i] * F[q, i]
            off = 32
            while off:
                for j in range(off):
                    part[j] = part[j] + part[j + off]
                off //= 2
            assert _bits(S.cost(F)[q]) == _bits(part[0])
            assert abs(part[0] - math.fsum(F[q] ** 2)) <= (m // 64 + 8) * 2.0 ** -52 * math.fsum(F[q] ** 2)


def test_selection_against_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(200):
        ncand = int(rng.integers(1, 40))
        c = rng.integers(0, 6, ncand).astype(np.float64)                        # many ties
        c[rng.random(ncand) < 0.3] = rng.choice([np.nan, np.inf, -np.inf])
        keep = int(rng.integers(1, min(8, ncand) + 1))
        brute = sorted((c[i], i) for i in range(ncand) if math.isfinite(c[i]))[:keep]
        oc, oi = S.select(c, keep)
        assert [(oc[k], oi[k]) for k in range(len(brute))] == brute
        assert (oi[len(brute):] == -1).all() and np.isposinf(oc[len(brute):]).all()


def test_pick_and_take():
    c = np.array([[3.0, np.nan, 1.0, np.inf], [1.0, np.nan, 1.0, 2.0], [0.5, np.inf, 4.0, -np.inf]])
    w = S.pick(c)
    assert list(w) == [2, -1, 0, 1]
    src = np.arange(3 * 4 * 2, dtype=np.float64).reshape(3, 4, 2)
    out = S.take(src, w)
    assert np.array_equal(out[0], src[2, 0]) and np.isnan(out[1]).all() and np.array_equal(out[2], src[0, 2]) and np.array_equal(out[3], src[1, 3])


# ---------------------------------------------------------------------------------------------------------------------
# the study
# ---------------------------------------------------------------------------------------------------------------------
STUDY_SUBSET = 6


def test_study(oracle):
    """The first STUDY_SUBSET problems, every row up to 256 candidates of the full model and 64 of the projected one,
    recomputed and compared with the golden file exactly.  No count is a condition: the file records what the oracle's solver
    does, whatever it is."""
    rec = json.load(open(SC.STUDY_GOLDEN))
    assert (rec["seed"], rec["nprob"], rec["m"], rec["noise"], rec["max_evals"]) == (SC.SEED, SC.NPROB, SC.M, SC.NOISE, SC.MAX_EVALS)
    want_rows = ["full_centre", "sep_centre"] + [f"full_{nc}_keep{k}" for nc in SC.FULL_NCAND for k in SC.FULL_KEEP] + \
        [f"sep_{nc}" for nc in SC.SEP_NCAND]
    assert sorted(rec["problems"]) == sorted(want_rows)
    for row, s in rec["problems"].items():
        assert len(s) == SC.NPROB and set(s) <= {"0", "1"} and rec["reached"][row] == s.count("1"), row
    got = SC.run_study(oracle, STUDY_SUBSET, full_ncand=(64, 256), sep_ncand=(16, 64))
    print({k: sum(v) for k, v in got.items()})
    for row, v in got.items():
        assert "".join(str(b) for b in v) == rec["problems"][row][:STUDY_SUBSET], row
