"""CPU tests of curve_guess: the new entry points are declared, exported and bound and make every documented refusal without a
device; tests/guess_restatement.py -- the numpy statement of the nonlinear stage the GPU tests compare with bit for bit --
held to bounds that are derived below, not tuned; and the four studies of the issue on the CPU oracle's solver, recorded in
tests/golden/guess_study.json.

THE BOUNDS.  dt: the grid spacing, h = smooth, delta = (h + 1) dt.
  position  the smoothed samples of a symmetric unimodal peak are largest at the grid point nearest mu or at a neighbour of
            it (a moving mean of a unimodal sequence is unimodal): |mu^ - mu| <= dt.
  width     noise-free, no baseline, F0 the true FWHM, F0 / 2 > (h + 2) dt.  The window of i* lies within delta of mu, so
            g(mu + delta) <= a^ <= a.  Right of the window of the peak g falls, so g(t + h dt) <= s(t) <= g(t - h dt).  The
            crossing is interpolated between the rows j - 1 and j with s[j-1] >= half > s[j]:  s[j] < a / 2 puts t_j above
            mu + F0/2 - h dt, and s[j-1] >= g(mu + delta) / 2 puts t_{j-1} below mu + x_lo + h dt, x_lo the half width of g
            at the level g(mu + delta) / 2.  The same on the left, so  F0 - 2 delta < F^ < 2 x_lo + 2 delta,  with
            x_lo = sqrt(2 sigma^2 ln 2 + delta^2) (Gaussian), sqrt(w^2 + 2 delta^2) (Lorentzian).
  rate      on a uniform grid the trapezoid of e^(-k t) over a step is rho = (k dt / 2) coth(k dt / 2) times its integral,
            the same factor on every step, and the trapezoid of a polynomial of degree <= 1 is exact.  So the sampled data
            satisfy the integral equation EXACTLY with kappa = k / rho = (2 / dt) tanh(k dt / 2) in the place of k (K = 2:
            kappa_1, kappa_2 are the roots of the characteristic equation), the panel's system is consistent, and
            k^ = kappa up to the rounding of a Householder least squares of a consistent system, which is at most
            8 m n u cond(panel) relative (Higham, Accuracy and Stability, theorem 20.3, first order, zero residual).
            k - kappa = k (1 - tanh(x) / x) <= k x^2 / 3 with x = k dt / 2.
  prefix    S_i is formed by at most c - 1 additions inside its chunk, 255 of chunk totals and one more:
            |S_i - exact| <= gamma(c + 256) sum_{j <= i} |q_j|, gamma(k) = k u / (1 - k u)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import curve_restatement as R
import guess_cases as GC
import guess_restatement as G

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -53
NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3
NEW = ("nlh_curve_guess_batch", "nlh_curve_guess_batch_h")


def _read(name):
    return open(os.path.join(os.path.dirname(HERE), "include", name)).read()


def _header():
    """The C ABI: nonlin_hip.h and the part of it that file includes, nonlin_hip_guess.h."""
    return _read("nonlin_hip.h") + _read("nonlin_hip_guess.h")


def _define(name):
    import re
    return int(re.search(r"#define\s+%s\s+(-?\d+)" % name, _header()).group(1))


def test_symbols_declared_exported_and_bound():
    from nonlin_amd import _lib
    L = _lib.load()
    import re
    assert '#include "nonlin_hip_guess.h"' in _read("nonlin_hip.h")           # who includes nonlin_hip.h has the entry points
    hdr = re.sub(r"/\*.*?\*/", "", _read("nonlin_hip_guess.h"), flags=re.S)
    assert sorted(set(re.findall(r"\b(nlh_[a-z0-9_]+)\s*\(", hdr))) == sorted(NEW) == sorted(_lib.GUESS_SYMBOLS)   # table and header agree
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == _lib.GUESS_SYMBOLS[name][1], name
    assert (_define("NLH_GUESS_MAX_M"), _define("NLH_GUESS_FALLBACK"), _define("NLH_GUESS_RANKDEF"), _define("NLH_GUESS_NONE")) == \
        (_lib.GUESS_MAX_M, _lib.GUESS_FALLBACK, _lib.GUESS_RANKDEF, _lib.GUESS_NONE) == (G.MAX_M, G.FALLBACK, G.RANKDEF, G.NONE)
    from nonlin_amd.device import DeviceSolver
    assert callable(DeviceSolver.curve_guess)
    shim = open(os.path.join(os.path.dirname(HERE), "nonlin_amd", "fortran", "nonlin_hip_c.f90")).read()
    assert 'name="nlh_curve_guess_batch_h"' in shim
    lsq = open(os.path.join(os.path.dirname(HERE), "nonlin_amd", "fortran", "nonlin_least_squares.f90")).read()
    assert "curve_guess_batch" in lsq


def test_every_refusal_without_a_device():
    """The refusals look at the arguments only: a block of zero bytes stands in for a handle, and nothing reads it."""
    from nonlin_amd import _lib
    L = _lib.load()
    under = _define("NLH_UNDERDEFINED_PROBLEM_ERROR")
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    buf = np.ones(4096)
    p = buf.ctypes.data_as(_lib.c_double_p)
    v = C.c_void_p(buf.ctypes.data)
    ip = np.zeros(64, dtype=np.int32).ctypes.data_as(_lib.c_int32_p)
    for fn, a, fl in ((L.nlh_curve_guess_batch, v, None), (L.nlh_curve_guess_batch_h, p, ip)):
        def call(h=fake, kind=0, K=1, B=0, nprob=1, m=16, t=a, y=a, w=None, smooth=2, x=a):
            return fn(h, kind, K, B, nprob, m, t, 0, y, w, smooth, x, fl)
        assert call(h=None) == NLH_ERR_BAD_HANDLE
        assert call(h=None, kind=7, m=0, t=None) == NLH_ERR_BAD_HANDLE          # the handle comes first
        for bad in (dict(kind=3), dict(kind=-1), dict(K=0), dict(B=-2), dict(B=9), dict(nprob=-1), dict(m=0),
                    dict(t=None), dict(y=None), dict(x=None), dict(smooth=-1), dict(m=G.MAX_M + 1),
                    dict(kind=0, K=30, B=2, m=256), dict(kind=1, K=33, B=-1, m=256), dict(kind=2, K=3, m=64)):
            assert call(**bad) == NL_INVALID_INPUT_ERROR, bad
        assert call(kind=0, K=2, B=0, m=6) == under                             # n = 7
        assert call(kind=2, K=2, B=1, m=5) == under                             # n = 6
        assert call(kind=2, K=3, B=1, m=5) == NL_INVALID_INPUT_ERROR            # invalid input comes before m < n
        assert call(nprob=0) == 0                                               # nothing to do: no device is touched


def test_x0_none_excludes_pmap_and_group():
    """The refusal is made before anything touches a device (the data are checked first: host tensors are refused there)."""
    import torch
    from nonlin_amd import device
    from nonlin_amd._lib import ParamMap
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(device, "_chk", lambda *a, **k: None)
        ds = object.__new__(device.DeviceSolver)
        t, y = torch.zeros(16, dtype=torch.float64), torch.zeros((2, 16), dtype=torch.float64)
        with pytest.raises(ValueError, match="x0=None excludes pmap and group"):
            ds.curve_fit_batch("gauss", t, y, None, baseline=0, pmap=ParamMap(4, fixed=[3]))
        with pytest.raises(ValueError, match="x0=None excludes pmap and group"):
            ds.curve_fit_batch("gauss", t, y, None, baseline=0, group=object())


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the derived bounds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0, 2, 5])
@pytest.mark.parametrize("kind", [R.GAUSS, R.LORENTZ])
def test_single_peak_position_and_width(kind, h):
    t = np.linspace(-5.0, 5.0, 201)
    dt = t[1] - t[0]
    delta = (h + 1) * dt
    for mu, wd in ((0.0, 0.5), (0.513, 0.6), (-1.237, 0.45), (2.02, 0.8)):
        F0 = G.FWHM_PER_SIGMA * wd if kind == R.GAUSS else 2.0 * wd
        assert F0 / 2.0 > (h + 2) * dt
        y = R.model(kind, 1, -1, np.array([3.0, mu, wd]), t)
        alpha, flag = G.nonlinear(kind, 1, -1, t, y, None, h)
        assert flag == 0
        assert abs(alpha[0] - mu) <= dt * (1 + 4 * U)
        F = alpha[1] * G.FWHM_PER_SIGMA if kind == R.GAUSS else 2.0 * alpha[1]
        x_lo = math.sqrt(2.0 * wd * wd * math.log(2.0) + delta * delta) if kind == R.GAUSS else math.sqrt(wd * wd + 2.0 * delta * delta)
        assert F0 - 2.0 * delta < F < 2.0 * x_lo + 2.0 * delta, (kind, h, mu, wd, F, F0)


def _rate_bound(K, B, t, y, k_true):
    """(kappa, eps ||c||, k - kappa's bound): eps = 8 m n u cond(panel), c the panel's least-squares solution by numpy."""
    tv, yv = G.compact(t, y, None)
    Phi, f0 = G.decay_panel(K, B, tv, yv, len(t))
    m, n = Phi.shape
    dt = t[1] - t[0]
    x = k_true * dt / 2.0
    kappa = (2.0 / dt) * np.tanh(x)
    c = np.linalg.lstsq(Phi, -f0, rcond=None)[0]
    return kappa, 8.0 * m * n * U * np.linalg.cond(Phi) * np.linalg.norm(c), k_true * x * x / 3.0


def test_single_decay_rate():
    """k^ = -c_0: its rounding is at most that of c, eps ||c||."""
    t = np.arange(128) * 0.0625 + 0.25
    for a, k, c in ((50.0, 1.0, 0.5), (3.0, 0.4, -1.0), (10.0, 2.5, 0.0)):
        y = R.model(R.EXPDECAY, 1, 0, np.array([a, k, c]), t)
        alpha, flag = G.nonlinear(R.EXPDECAY, 1, 0, t, y)
        kappa, slack, gap = _rate_bound(1, 0, t, y, np.array([k]))
        print(f"decay k = {k}: k^ - kappa = {alpha[0] - kappa[0]:.3g} (bound {slack:.3g}), k^ - k = {alpha[0] - k:.3g} (bound {gap[0] + slack:.3g})")
        assert flag == 0
        assert abs(alpha[0] - kappa[0]) <= slack
        assert abs(alpha[0] - k) <= gap[0] + slack
        x0, _ = G.guess(R.EXPDECAY, 1, 0, t, y)
        assert abs(x0[1] - alpha[0]) == 0.0 and np.isfinite(x0).all()


def test_biexponential_rates():
    """kappa_i is a root of kappa^2 + A kappa - Bc = 0 with 2 kappa_i + A = +-(kappa_1 - kappa_2), so a change (dA, dBc) of the
    coefficients moves it by at most (kappa_i |dA| + |dBc|) / (kappa_1 - kappa_2) to first order: (kappa_i + 1) eps ||c|| over the
    gap of the roots."""
    t = np.linspace(0.0, 8.0, 257)
    for k1, k2 in ((1.5, 0.3), (2.0, 0.5)):
        y = R.model(R.EXPDECAY, 2, 0, np.array([600.0, k1, 400.0, k2, 20.0]), t)
        alpha, flag = G.nonlinear(R.EXPDECAY, 2, 0, t, y)
        kappa, slack, gap = _rate_bound(2, 0, t, y, np.array([k1, k2]))
        s = (kappa + 1.0) * slack / (kappa[0] - kappa[1])
        print(f"biexponential ({k1}, {k2}): k^ - kappa = {alpha - kappa} (bound {s}), k^ - k = {alpha - np.array([k1, k2])}")
        assert flag == 0 and alpha[0] > alpha[1]                            # the fast rate first
        assert (np.abs(alpha - kappa) <= s).all()
        assert (np.abs(alpha - np.array([k1, k2])) <= gap + s).all()


@pytest.mark.parametrize("mv", [1, 255, 256, 257, 513])
def test_blocked_prefix_sum(mv):
    rng = np.random.default_rng(mv)
    q = rng.standard_normal(mv) * 10.0 ** rng.integers(-6, 6, mv)
    S = G.blocked_prefix(q)
    c = (mv + 255) // 256
    k = c + 256
    gamma = k * U / (1.0 - k * U)
    for i in range(mv):
        exact = math.fsum(q[:i + 1])
        assert abs(S[i] - exact) <= gamma * math.fsum(np.abs(q[:i + 1])) + U * abs(exact), (mv, i)
    # the order itself, spelled out
    run, tot, want = 0.0, [], np.empty(mv)
    loc = np.empty(mv)
    for i in range(mv):
        if i % c == 0:
            if i:
                tot.append(run)
            run = 0.0
        run = run + q[i]
        loc[i] = run
    off = [0.0]
    for v in tot:
        off.append(off[-1] + v)
    for i in range(mv):
        want[i] = off[i // c] + loc[i]
    assert np.array_equal(S.view(np.uint64), want.view(np.uint64))


def test_not_guessed():
    t = np.linspace(0.0, 1.0, 16)
    y = np.exp(-t)
    w = np.ones(16)
    for tt, yy, ww in ((t, np.where(np.arange(16) == 5, np.nan, y), None), (np.where(np.arange(16) == 3, t[2], t), y, None),
                       (t, y, np.where(np.arange(16) < 2, 1.0, 0.0)), (np.where(np.arange(16) == 9, np.inf, t), y, w)):
        alpha, flag = G.nonlinear(R.EXPDECAY, 1, 0, tt, yy, ww)
        assert flag == G.NONE and np.isnan(alpha).all()
    bad = np.where(np.arange(16) == 5, np.nan, y)                           # a row that is not valid may hold anything
    alpha, flag = G.nonlinear(R.EXPDECAY, 1, 0, t, bad, np.where(np.arange(16) == 5, 0.0, 1.0))
    assert flag == 0 and np.isfinite(alpha).all()


def test_flat_data_fall_back():
    t = np.linspace(0.0, 4.0, 64)
    for kind in (R.GAUSS, R.LORENTZ):
        alpha, flag = G.nonlinear(kind, 1, 0, t, np.full(64, 3.0))
        assert flag == G.FALLBACK and alpha[1] > 0.0
    alpha, flag = G.nonlinear(R.EXPDECAY, 1, 0, t, np.full(64, 3.0))
    assert flag == G.FALLBACK and alpha[0] == 2.0 / 4.0


# ---------------------------------------------------------------------------------------------------------------------
# the studies
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GC.STUDIES))
def test_study(oracle, name):
    """At most 5 % of the problems end above 1.05 x the cost at the truth or carry FALLBACK -- a condition, not a measurement
    --, and tests/golden/guess_study.json records what is measured here."""
    got = GC.run_study(oracle, name)
    print(name, got)
    assert got["failed"] <= GC.CAP * got["nprob"], got
    rec = json.load(open(GC.STUDY_GOLDEN))
    assert rec["cap"] == GC.CAP and rec["max_evals_option"] == GC.MAX_EVALS
    want = rec["studies"][name]
    for key in ("nprob", "m", "reached", "fallback", "failed", "max_evals"):
        assert got[key] == want[key], (name, key)
    assert got["mean_evals"] == pytest.approx(want["mean_evals"], rel=1e-9)
