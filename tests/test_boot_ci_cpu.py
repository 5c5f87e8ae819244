"""CPU tests of the studentised and the BCa interval of the bootstrap: the new entry points are declared, exported and bound;
every refusal that needs no device; tests/boot_ci_restatement.py spelled out on cases small enough to follow by hand;
nlh_boot_bca_levels -- host code -- against the restatement; ppnd16 against the standard library's; the acceleration of a
sample whose value is known in closed form."""
import ctypes as C
import math
import os
import re
import statistics

import numpy as np
import pytest

import boot_restatement as B
import boot_ci_restatement as R
from nonlin_amd import Bootstrap, PoissonBootstrap, bca_levels
from nonlin_amd._lib import BOOT_CI_SYMBOLS  # noqa: F401  (the feature: without it nothing here runs)

HERE = os.path.dirname(os.path.abspath(__file__))
NL_INVALID_INPUT_ERROR, NL_ARRAY_SIZE_ERROR, NLH_ERR_BAD_HANDLE = 201, 202, -3
NEW = ("nlh_boot_bca_levels", "nlh_boot_student_batch", "nlh_boot_jackknife_batch", "nlh_boot_accel_batch", "nlh_boot_bca_batch")
ALPHA_TOL = 2.0 ** -44                                                          # the header's bound between two libraries' alphas


def _read(name):
    return open(os.path.join(os.path.dirname(HERE), "include", name)).read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_symbols_declared_exported_and_bound():
    from nonlin_amd import _lib
    import nonlin_amd
    L = _lib.load()
    assert '#include "nonlin_hip_boot_ci.h"' in _read("nonlin_hip.h")          # who includes nonlin_hip.h has the entry points
    text = _read("nonlin_hip_boot_ci.h")
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(nlh_[a-z0-9_]+)\s*\(", hdr))) == sorted(NEW) == sorted(_lib.BOOT_CI_SYMBOLS)  # table and header agree
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == _lib.BOOT_CI_SYMBOLS[name][1], name
        assert all(name not in tab for tab in (_lib.SYMBOLS, _lib.GUESS_SYMBOLS, _lib.STARTS_SYMBOLS, _lib.BOOT_SYMBOLS, _lib.BIN_SYMBOLS,
                                               _lib.BOOT_POIS_SYMBOLS, _lib.PROFILE_SYMBOLS))
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))
    assert (define("NLH_BCA_DEGENERATE"), define("NLH_BCA_NO_ACCEL"), define("NLH_BCA_BAD_DENOM"), define("NLH_BCA_NO_REPLICA")) == \
        (_lib.BCA_DEGENERATE, _lib.BCA_NO_ACCEL, _lib.BCA_BAD_DENOM, _lib.BCA_NO_REPLICA) == \
        (R.DEGENERATE, R.NO_ACCEL, R.BAD_DENOM, R.NO_REPLICA) == (1, 2, 4, 8)
    assert nonlin_amd.bca_levels is _lib.bca_levels and nonlin_amd.BOOT_INTERVALS == ("percentile", "student", "bca")
    from nonlin_amd.device import DeviceSolver
    for name in ("boot_student", "boot_jackknife", "boot_accel", "boot_bca"):
        assert callable(getattr(DeviceSolver, name))
    # the coefficients of the header's statement of AS 241 are the restatement's, in order
    nums = [float(v) for v in re.findall(r"[-+]?\d\.\d+e[-+]\d+", text.split("ppnd16      Wichura")[1].split("bca         validity")[0])]
    want = [c for tab in (R._A, R._B, R._C, R._D, R._E, R._F) for c in tab if c != 1.0]
    assert nums == want


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_bca_levels():
    from nonlin_amd import _lib
    L = _lib.load()
    out = [C.c_double(7.0), C.c_double(7.0), C.c_double(7.0)]
    flag = C.c_int32(-9)

    def call(c2=5, cnt=5, a=0.0, level=0.95, null=None):
        ptrs = [C.byref(o) for o in out] + [C.byref(flag)]
        if null is not None:
            ptrs[null] = None
        return L.nlh_boot_bca_levels(c2, cnt, a, level, *ptrs)
    for bad in (dict(cnt=-1), dict(c2=-1), dict(c2=11), dict(c2=1, cnt=0), dict(level=0.0), dict(level=1.0), dict(level=math.nan),
                dict(level=-0.5), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(c2=1, cnt=B.MAX_REP + 1),
                dict(c2=2 ** 31 - 1, cnt=2 ** 30)):
        assert call(**bad) == NL_INVALID_INPUT_ERROR, bad
        assert [o.value for o in out] == [7.0] * 3 and flag.value == -9, bad    # a refused call writes nothing
    assert call() == 0 and out[0].value == 0.0 and flag.value == 0
    assert call(c2=0, cnt=0) == 0 and all(math.isnan(o.value) for o in out) and flag.value == R.NO_REPLICA
    assert bca_levels(11, 5, 0.0) is None and bca_levels(1, 2, 0.0, 1.0) is None and bca_levels(2 ** 31, 2 ** 31, 0.0) is None
    assert bca_levels(1, B.MAX_REP, 0.0) is not None
    assert bca_levels("a", 5, 0.0) is None


def test_device_entry_points_refuse_without_a_device():
    """The refusals look at the arguments only: a block of zero bytes stands in for a handle, and nothing reads it."""
    from nonlin_amd import _lib
    L = _lib.load()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    buf = np.ones(4096)
    v = C.c_void_p(buf.ctypes.data)
    levels = (dict(level=0.0), dict(level=1.0), dict(level=math.nan), dict(level=-0.5))
    shape = (dict(nrep=0), dict(nrep=B.MAX_REP + 1), dict(nprob=-1), dict(n=0))

    def stud(h=fake, nrep=4, nprob=1, n=2, level=0.95, ptrs=(v,) * 7):
        return L.nlh_boot_student_batch(h, nrep, nprob, n, *ptrs[:4], level, *ptrs[4:])
    assert stud(h=None) == stud(h=None, nrep=0, ptrs=(None,) * 7) == NLH_ERR_BAD_HANDLE                  # the handle comes first
    for bad in shape + levels + tuple(dict(ptrs=tuple(None if i == k else v for i in range(7))) for k in range(7)):
        assert stud(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert stud(nprob=2 ** 30, n=2) == stud(nprob=2 ** 20, nrep=2048) == NL_ARRAY_SIZE_ERROR
    assert stud(nprob=0) == 0

    def bca(h=fake, nrep=4, nprob=1, n=2, level=0.95, ptrs=(v,) * 10):
        return L.nlh_boot_bca_batch(h, nrep, nprob, n, *ptrs[:3], level, *ptrs[3:])
    assert bca(h=None) == bca(h=None, nrep=0, ptrs=(None,) * 10) == NLH_ERR_BAD_HANDLE
    for bad in shape + levels + tuple(dict(ptrs=tuple(None if i == k else v for i in range(10))) for k in range(10)):
        assert bca(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert bca(nprob=2 ** 30, n=2) == bca(nprob=2 ** 20, nrep=2048) == NL_ARRAY_SIZE_ERROR
    assert bca(nprob=0) == 0

    def jack(h=fake, nprob=1, m=8, row0=0, nrows=8, w=v, wout=v):
        return L.nlh_boot_jackknife_batch(h, nprob, m, row0, nrows, w, wout)
    assert jack(h=None) == jack(h=None, m=0, wout=None) == NLH_ERR_BAD_HANDLE
    for bad in (dict(nprob=-1), dict(m=0), dict(m=B.MAX_ROWS + 1), dict(row0=-1), dict(nrows=-1), dict(row0=1), dict(nrows=9),
                dict(row0=2 ** 31 - 1, nrows=2 ** 31 - 1, m=B.MAX_ROWS), dict(wout=None)):
        assert jack(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert jack(nprob=2 ** 20, m=4096, nrows=1) == NL_ARRAY_SIZE_ERROR
    assert jack(nprob=0) == jack(nrows=0) == jack(nrows=0, row0=8) == 0

    def acc(h=fake, m=8, nprob=1, n=2, xj=v, w=v, a=v, nj=v):
        return L.nlh_boot_accel_batch(h, m, nprob, n, xj, w, a, nj)
    assert acc(h=None) == acc(h=None, m=0, xj=None) == NLH_ERR_BAD_HANDLE
    for bad in (dict(m=0), dict(m=B.MAX_ROWS + 1), dict(nprob=-1), dict(n=0), dict(xj=None), dict(a=None), dict(nj=None)):
        assert acc(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert acc(nprob=2 ** 30, n=2) == acc(nprob=2 ** 20, m=4096) == NL_ARRAY_SIZE_ERROR
    assert acc(nprob=0) == acc(nprob=0, w=None) == 0
    assert (buf == 1.0).all()


def test_constructor_value_errors():
    assert Bootstrap().interval == PoissonBootstrap().interval == "percentile"
    for kind in ("percentile", "student", "bca"):
        assert Bootstrap(interval=kind).interval == PoissonBootstrap(interval=kind).interval == kind
    for bad in ("BCa", "t", "", None, 1, b"bca", ("bca",)):
        with pytest.raises(ValueError, match="unknown interval"):
            Bootstrap(interval=bad)
        with pytest.raises(ValueError, match="PoissonBootstrap: unknown interval"):
            PoissonBootstrap(interval=bad)
    b = Bootstrap(5, "wild", 3, 0.9, False)                                     # the positional order of before is kept
    assert (b.nrep, b.name, b.seed, b.level, b.centre, b.interval) == (5, "wild", 3, 0.9, False, "percentile")


def test_one_call_refusals_without_a_device():
    """"student" without sigma=, and what was refused before is still refused with the new intervals: before anything touches a
    device."""
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
            with pytest.raises(ValueError, match='"student" needs sigma='):
                call(boot=Bootstrap(5, interval="student"))
            with pytest.raises(ValueError, match='"student" needs sigma='):
                call(boot=PoissonBootstrap(5, interval="student"), stat=Poisson())
            for kind in ("student", "bca"):
                with pytest.raises(ValueError, match="excludes stat and group"):
                    call(boot=Bootstrap(5, interval=kind), group=object(), sigma=x)
                with pytest.raises(ValueError, match="excludes group"):
                    call(boot=PoissonBootstrap(5, interval=kind), stat=Poisson(), group=object(), sigma=x)
                with pytest.raises(ValueError, match='"pairs" excludes conv'):
                    call(boot=Bootstrap(5, "pairs", interval=kind), conv=cv, sigma=x)


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_ppnd16_against_the_standard_library():
    """statistics.NormalDist.inv_cdf is the same algorithm: equal where no library function is reached, a few ulp in the tails."""
    inv = statistics.NormalDist().inv_cdf
    rng = np.random.default_rng(21)
    ps = [0.5, 0.0751, 0.9249, 0.3, 0.7] + list(rng.uniform(0.0751, 0.9249, 2000))
    for p in ps:
        assert R.central(p) and R.ppnd16(p) == inv(p), p
    assert R.ppnd16(0.5) == 0.0 and R.ppnd16(0.975) == -R.ppnd16(0.025) or abs(R.ppnd16(0.975) + R.ppnd16(0.025)) < 1e-14
    for p in [0.025, 0.975, 0.074, 0.926, 1e-10, 1.0 - 1e-10, 1e-300, 5e-324] + list(rng.uniform(0.0, 0.074, 500)):
        if 0.0 < p < 1.0:
            assert not R.central(p) and abs(R.ppnd16(p) - inv(p)) <= 4 * np.spacing(abs(inv(p))), p
    assert abs(R.ppnd16(0.975) - 1.959963984540054) < 1e-15 and abs(R.ppnd16(1e-10) + 6.361340902404056) < 1e-14


def test_student_spelled_out():
    """Five replicas, two parameters: a NaN row leaves both, a sigma that is 0 leaves its own parameter only."""
    xs = np.array([[[11.0, 5.0]], [[9.0, np.nan]], [[12.0, 5.0]], [[10.5, 5.0]], [[8.0, 5.0]]])
    sigs = np.array([[[0.5, 1.0]], [[1.0, 1.0]], [[1.0, 1.0]], [[0.0, 1.0]], [[2.0, 1.0]]])
    x, sigma = np.array([[10.0, 4.0]]), np.array([[2.0, 0.5]])
    lo, hi, nvt = R.student(xs, sigs, x, sigma, 0.5)
    # parameter 0: t = 2, 2, -1 of the replicas 0, 2, 4 -> sorted -1, 2, 2; T_0.25 = 0.5, T_0.75 = 2; lo = 10 - 2*2, hi = 10 - 0.5*2
    assert list(nvt[0]) == [3, 4] and (lo[0, 0], hi[0, 0]) == (6.0, 9.0)
    assert (lo[0, 1], hi[0, 1]) == (3.5, 3.5)                                   # every t is 1
    for bad in (-1.0, np.nan, np.inf):                                          # sigs that will not do, each alone
        s2 = sigs.copy()
        s2[3, 0, 0] = bad
        again = R.student(xs, s2, x, sigma, 0.5)
        assert again[2][0, 0] == 3 and (again[0][0, 0], again[1][0, 0]) == (6.0, 9.0)
    for bx, bs in ((np.nan, 2.0), (np.inf, 2.0), (10.0, 0.0), (10.0, -1.0), (10.0, np.nan), (10.0, np.inf)):
        lo2, hi2, nvt2 = R.student(xs, sigs, np.array([[bx, 4.0]]), np.array([[bs, 0.5]]), 0.5)
        assert np.isnan(lo2[0, 0]) and np.isnan(hi2[0, 0]) and nvt2[0, 0] == 3 and lo2[0, 1] == 3.5
    none = R.student(xs[1:2], sigs[1:2], x, sigma, 0.5)
    assert (none[2] == 0).all() and np.isnan(none[0]).all() and np.isnan(none[1]).all()


def test_jackknife_spelled_out():
    w = np.array([[2.0, 0.0, 3.0], [1.0, 1.0, -0.0]])
    out = R.jackknife(w, 2, 3)
    assert out.shape == (3, 2, 3)
    assert out[0].tolist() == [[0.0, 0.0, 3.0], [0.0, 1.0, -0.0]] and out[1].tolist() == [[2.0, 0.0, 3.0], [1.0, 0.0, -0.0]]
    assert out[2].tolist() == [[2.0, 0.0, 0.0], [1.0, 1.0, 0.0]]
    assert not np.signbit(out[2, 1, 2]) and np.signbit(out[0, 1, 2])            # a deleted row is +0.0; the others keep their bits
    assert np.array_equal(_bits(R.jackknife(w, 2, 3, 1, 2)), _bits(out[1:3]))
    assert R.jackknife(None, 1, 3).tolist() == [[[0.0, 1.0, 1.0]], [[1.0, 0.0, 1.0]], [[1.0, 1.0, 0.0]]]


def test_accel_in_closed_form():
    """0, 0, 0, 4: mean 1, d = 1, 1, 1, -3, S2 = 12, S3 = -24 -- all exact --, so a = -24/(6*12*sqrt(12)) = -1/(3*sqrt(12));
    a sample symmetric about its mean has a = 0; rows of weight 0 and NaN rows leave."""
    xj = np.zeros((4, 1, 2))
    xj[3, 0, 0] = 4.0
    xj[:, 0, 1] = [1.0, 2.0, 4.0, 5.0]
    a, nj = R.accel(xj)
    assert list(nj) == [4] and a[0, 0] == -24.0 / (6.0 * (12.0 * math.sqrt(12.0))) and a[0, 1] == 0.0
    assert abs(a[0, 0] + 1.0 / (3.0 * math.sqrt(12.0))) < 1e-16
    big = np.zeros((7, 1, 2))                                                   # the same sample among rows that do not count
    big[[0, 2, 3, 6]] = xj
    big[1] = np.nan
    big[4, 0, 1] = np.inf
    big[5] = 100.0
    w = np.ones((1, 7))
    w[0, 5] = 0.0
    a2, nj2 = R.accel(big, w)
    assert list(nj2) == [4] and np.array_equal(_bits(a2), _bits(a))
    for m in (0, 1):                                                            # fewer than two valid deletions; no spread
        a3, nj3 = R.accel(xj[:1] if m else np.full((3, 1, 2), np.nan))
        assert list(nj3) == [m] and not a3.any() and not np.signbit(a3).any()
    a4, nj4 = R.accel(np.full((5, 1, 1), 2.5))
    assert list(nj4) == [5] and a4[0, 0] == 0.0
    a5, _ = R.accel(np.array([0.0, 0.0, 0.0, 1e200]).reshape(4, 1, 1))         # S3 overflows: Inf/Inf is not finite
    assert a5[0, 0] == 0.0


def test_bca_spelled_out():
    """1 .. 5 with xhat = 3: two below and one equal, c2 = 5 -- odd --, u = 5/10, z0 = 0 exactly; with a = 0 the levels are
    Phi(z_q) = q again up to the two libraries' roundings."""
    xs = np.arange(1.0, 6.0).reshape(5, 1, 1)
    x = np.array([[3.0]])
    c2, cnt = R.bca_counts(xs, x)
    assert (int(c2[0, 0]), int(cnt[0])) == (5, 5)
    z0, alo, ahi, flag, u = R.bca_levels(5, 5, 0.0, 0.5)
    assert (u, z0, flag) == (0.5, 0.0, 0) and abs(alo - 0.25) < 1e-15 and abs(ahi - 0.75) < 1e-15
    lo, hi, z0s, alos, ahis, flags, nvalid = R.bca(xs, x, np.zeros((1, 1)), 0.5)
    assert (z0s[0, 0], alos[0, 0], ahis[0, 0], flags[0, 0], nvalid[0]) == (z0, alo, ahi, 0, 5)
    assert abs(lo[0, 0] - 2.0) < 1e-14 and abs(hi[0, 0] - 4.0) < 1e-14        # the percentile interval's 2 and 4
    # a positive acceleration moves both levels up: den = 1 - a*s is below 1 at the upper end and above 1 at the lower
    z0, alo2, ahi2, flag, _ = R.bca_levels(5, 5, 0.1, 0.5)
    assert flag == 0 and alo2 > alo and ahi2 > ahi
    zq = R.ppnd16(0.75)
    assert ahi2 == 0.5 * math.erfc(-((0.0 + (0.0 + zq) / (1.0 - 0.1 * (0.0 + zq))) * 0.70710678118654752))
    # xhat between the values: c2 even; xhat above more of them: z0 > 0
    assert int(R.bca_counts(xs, np.array([[3.5]]))[0][0, 0]) == 6 and R.bca_levels(6, 5, 0.0, 0.5)[0] > 0.0


def test_every_flag():
    xs = np.arange(1.0, 6.0).reshape(5, 1, 1)
    pct = B.summary(xs, 0.5)
    for xhat, z0 in ((0.0, -math.inf), (9.0, math.inf)):                        # below all replicas, above all of them
        lo, hi, z0s, alo, ahi, flags, nvalid = R.bca(xs, np.array([[xhat]]), np.array([[0.3]]), 0.5)
        assert flags[0, 0] == R.DEGENERATE and z0s[0, 0] == z0 and (alo[0, 0], ahi[0, 0]) == R.levels(0.5)
        assert (lo[0, 0], hi[0, 0]) == (pct[0][0, 0], pct[1][0, 0])             # the percentile interval
    for a in (math.nan, math.inf, -math.inf):
        got = R.bca_levels(5, 5, a, 0.5)
        assert got[3] == R.NO_ACCEL and got[:3] == R.bca_levels(5, 5, 0.0, 0.5)[:3]
    assert R.bca_levels(0, 5, math.nan, 0.5)[3] == R.NO_ACCEL | R.DEGENERATE
    zq = R.ppnd16(0.75)
    z0, alo, ahi, flag, _ = R.bca_levels(5, 5, 10.0, 0.5)                       # z0 = 0: den = 1 - 10 z_hi < 0 at the upper end only
    assert flag == R.BAD_DENOM and ahi == 0.75 and alo == 0.5 * math.erfc(-((-zq / (1.0 + 10.0 * zq)) * 0.70710678118654752))
    z0, alo, ahi, flag, _ = R.bca_levels(5, 5, 1.0 / zq, 0.5)                   # den == 0 exactly is not > 0
    assert 1.0 - (1.0 / zq) * zq == 0.0 and flag == R.BAD_DENOM and ahi == 0.75
    assert R.bca_levels(5, 5, -10.0, 0.5)[3] == R.BAD_DENOM and R.bca_levels(5, 5, -10.0, 0.5)[1] == 0.25
    none = R.bca(np.full((3, 1, 2), np.nan), np.zeros((1, 2)), np.zeros((1, 2)), 0.5)
    assert (none[5] == R.NO_REPLICA).all() and none[6][0] == 0 and all(np.isnan(a).all() for a in none[:5])
    xs2 = np.arange(10.0).reshape(5, 1, 2)
    bad = R.bca(xs2, np.array([[np.nan, 5.0]]), np.zeros((1, 2)), 0.5)          # an xhat that is not finite: its pair only
    assert list(bad[5][0]) == [R.NO_REPLICA, 0] and np.isnan(bad[0][0, 0]) and np.isfinite(bad[0][0, 1]) and bad[6][0] == 5


# ---------------------------------------------------------------------------------------------------------------------
# the host call against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_bca_levels_equal_the_restatement():
    """flags and the central z0 (so u = c2/(2 cnt)) bit for bit; alpha within the header's 2^-44 on inputs with
    |a (z0 + z)| <= 1/2 and 0 < c2 < 2 cnt, where an error of z0 enters alpha with a factor of at most 0.4 (1 + 1/den^2) <= 2."""
    rng = np.random.default_rng(22)
    worst, ntail, ncentral = 0.0, 0, 0
    for level in (0.95, 0.9, 0.5, 0.999):
        zq = max(abs(R.ppnd16(q)) for q in R.levels(level))
        for cnt in (1, 2, 5, 64, 200, 4095, 4096):
            c2s = sorted(set([1, 2, cnt, cnt + 1, 2 * cnt - 1] + list(rng.integers(1, 2 * cnt, 40)))) if cnt > 1 else [1]
            for c2 in c2s:
                c2 = int(c2)
                if not 0 < c2 < 2 * cnt:
                    continue
                z0r = R.ppnd16(c2 / (2.0 * cnt))
                amax = 0.5 / (abs(z0r) + zq)
                for a in (0.0, amax, -amax, 0.3 * amax, float(rng.uniform(-amax, amax))):
                    want = R.bca_levels(c2, cnt, a, level)
                    got = bca_levels(c2, cnt, a, level)
                    assert got[3] == want[3] == 0, (c2, cnt, a, level)
                    if R.central(want[4]):
                        ncentral += 1
                        assert _bits(got[0]) == _bits(want[0]), (c2, cnt, level)
                    else:
                        ntail += 1
                        assert abs(got[0] - want[0]) <= 8 * np.spacing(abs(want[0])), (c2, cnt, level)
                    for g, w_ in zip(got[1:3], want[1:3]):
                        worst = max(worst, abs(g - w_))
                        assert abs(g - w_) <= ALPHA_TOL, (c2, cnt, a, level, g, w_)
                        assert 0.0 <= g <= 1.0
    print("alpha: largest difference", worst, "central", ncentral, "tail", ntail)
    assert ncentral > 500 and ntail > 50
    # every flag, and the values that go with it, bit for bit: no library function is behind them
    for args in ((0, 5, 0.3, 0.5), (10, 5, 0.3, 0.5), (0, 5, math.nan, 0.9), (5, 5, math.inf, 0.5), (0, 0, 0.0, 0.5)):
        got, want = bca_levels(*args), R.bca_levels(*args)
        assert got[3] == want[3] and np.array_equal(_bits(got[:3]), _bits(want[:3])) or \
            (got[3] == want[3] == R.NO_ACCEL and abs(got[1] - want[1]) <= ALPHA_TOL)
    for a in (10.0, -10.0):
        got, want = bca_levels(5, 5, a, 0.5), R.bca_levels(5, 5, a, 0.5)
        assert got[3] == want[3] == R.BAD_DENOM and got[0] == 0.0
        kept = 2 if a > 0 else 1
        assert got[kept] == want[kept] == R.levels(0.5)[kept - 1]


# ---------------------------------------------------------------------------------------------------------------------
# the study
# ---------------------------------------------------------------------------------------------------------------------
def test_study(oracle):
    """tests/golden/boot_ci_study.json: the whole of it takes minutes on the oracle's solver, so the first NFIRST data sets of
    each family are recomputed and compared exactly, and the rest is checked for consistency -- the table against the
    per-data-set records, and the rows that earlier studies also hold against those.  No coverage is a condition: the file
    records what the intervals do, whatever it is."""
    import json
    import boot_cases as BC
    import boot_ci_cases as S
    import boot_pois_cases as BPC
    rec = json.load(open(S.STUDY_GOLDEN))
    assert (rec["nrep"], rec["level"], tuple(rec["rows"]), sorted(rec["families"])) == (S.NREP, S.LEVEL, S.ROWS, sorted(S.FAMILIES))
    for f in S.FAMILIES:
        fam = rec["families"][f]
        n = S.NDATA[f]
        assert fam["ndata"] == n and all(len(fam[k]) == n for k in ("nvalid", "nvalid_t", "njack", "flags"))
        for r in S.ROWS:
            for q in S.PARAMS:
                assert len(fam["cover"][r][q]) == n and set(fam["cover"][r][q]) <= set("1abn"), (f, r, q)
                assert len(fam["half_first"][r][q]) == S.NFIRST, (f, r, q)
                assert math.isfinite(fam["median_half"][r][q]), (f, r, q)
        want = S.table(fam, n)
        for k, v in want.items():
            assert fam[k] == v, (f, k)
        for r in S.ROWS:
            for q in S.PARAMS:
                assert abs(fam["coverage"][r][q] + fam["above"][r][q] + fam["below"][r][q] + fam["cover"][r][q].count("n") / n - 1.0) < 1e-12
        dat = S.data(f)
        got = S.summarise([S.one(oracle, f, p, dat) for p in range(S.NFIRST)])
        print(f, {r: got["coverage"][r] for r in S.ROWS})
        for r in S.ROWS:
            for q in S.PARAMS:
                assert got["cover"][r][q] == fam["cover"][r][q][:S.NFIRST], (f, r, q)
                assert got["half_first"][r][q] == fam["half_first"][r][q], (f, r, q)
        for k in ("nvalid", "nvalid_t", "njack", "flags"):
            assert got[k] == fam[k][:S.NFIRST], (f, k)
    # the same fits and replicas as the earlier studies: their Gaussian and percentile rows are these
    hit = lambda s: s.replace("a", "0").replace("b", "0").replace("n", "0")
    old = json.load(open(BC.STUDY_GOLDEN))
    for q in S.PARAMS:
        assert hit(rec["families"]["decay"]["cover"]["gauss"][q]) == old["covered"]["gauss"][q]
        assert hit(rec["families"]["decay"]["cover"]["percentile"][q]) == old["covered"]["residual"][q]
    old = json.load(open(BPC.STUDY_GOLDEN))["study"][S.POIS_TRUTH]
    for q in S.PARAMS:
        assert hit(rec["families"]["poisson"]["cover"]["gauss"][q]) == old["covered"]["gauss"][q]
        assert hit(rec["families"]["poisson"]["cover"]["percentile"][q]) == old["covered"]["percentile"][q]
    assert rec["families"]["poisson"]["nvalid"] == old["nvalid"]
