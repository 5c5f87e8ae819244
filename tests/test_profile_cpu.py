"""CPU tests of the profile-likelihood intervals: the new entry points are declared, exported and bound; every refusal that needs
no device; the restated root finder on a straight line (the first trial is the end, bit for bit) and on synthetic costs that
reach every flag and branch; and the coverage study on the CPU oracle's solver, recorded in tests/golden/profile_study.json."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import profile_cases as PC
import profile_restatement as PR
import starts_restatement as S
from nonlin_amd import Profile
from nonlin_amd._lib import PROFILE_SYMBOLS  # noqa: F401  (the feature: without it nothing here runs)

HERE = os.path.dirname(os.path.abspath(__file__))
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NLH_ERR_BAD_HANDLE = 201, 211, -3
NEW = ("nlh_pin_wrap", "nlh_pin_set", "nlh_pin_unwrap", "nlh_pin_device_fcn", "nlh_pin_device_jac", "nlh_profile_start_batch_device",
       "nlh_profile_step_batch")


def _read(name):
    return open(os.path.join(os.path.dirname(HERE), "include", name)).read()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. symbols
# ---------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    from nonlin_amd import _lib
    import nonlin_amd
    L = _lib.load()
    assert '#include "nonlin_hip_profile.h"' in _read("nonlin_hip.h")          # who includes nonlin_hip.h has the entry points
    text = _read("nonlin_hip_profile.h")
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(nlh_[a-z0-9_]+)\s*\(", hdr))) == sorted(NEW) == sorted(_lib.PROFILE_SYMBOLS)
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == _lib.PROFILE_SYMBOLS[name][1], name
        assert all(name not in tab for tab in (_lib.SYMBOLS, _lib.GUESS_SYMBOLS, _lib.STARTS_SYMBOLS, _lib.BOOT_SYMBOLS, _lib.BIN_SYMBOLS,
                                               _lib.BOOT_POIS_SYMBOLS))
    # the flags and phases of the header, of the Python constants and of the restatement are the same numbers
    for k, name in enumerate(_lib.PROFILE_FLAGS):
        assert int(re.search(r"#define\s+NLH_PROFILE_%s\s+(\d+)" % name, text).group(1)) == k == getattr(_lib, "PROFILE_" + name) == getattr(PR, name)
    assert int(re.search(r"#define\s+NLH_PROFILE_LOWER\s+(\d+)", text).group(1)) == _lib.PROFILE_LOWER == PR.LOWER == 16
    for k, name in enumerate(("EXPAND", "BRACKET", "DONE")):
        assert int(re.search(r"#define\s+NLH_PROFILE_%s\s+(\d+)" % name, text).group(1)) == k == getattr(_lib, "PROFILE_" + name) == getattr(PR, name)
    # the state struct: the header's fields, in its order
    body = re.search(r"typedef struct nlh_profile_state \{(.*?)\} nlh_profile_state;", hdr, flags=re.S).group(1)
    assert re.findall(r"\*\s*([A-Za-z0-9]+)", body) == [k for k, _ in _lib.ProfileState._fields_] == list(PR.NAMES)
    assert nonlin_amd.Profile is _lib.Profile
    from nonlin_amd.device import DeviceSolver
    for name in ("pin_launchers", "pin_set", "profile_start", "profile_step", "profile_batch_device", "curve_profile_batch", "expr_profile_batch"):
        assert callable(getattr(DeviceSolver, name)), name


# ---------------------------------------------------------------------------------------------------------------------
# 2. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_profile_object():
    p = Profile()
    z = 1.959963984540054
    assert (p.level, p.tol, p.xtol, p.max_expand, p.maxit) == (0.95, 0.01, 1e-3, 8, 30)
    assert abs(p.crit - z * z) < 1e-12 and p.crit == PR.crit_of(0.95) == PC.CRIT
    assert Profile(level=0.68, crit=1.0).crit == 1.0
    assert abs(Profile(level=0.6826894921370859).crit - 1.0) < 1e-9
    for bad in (dict(level=0.0), dict(level=1.0), dict(level="0.9"), dict(level=True), dict(level=math.nan), dict(crit=0.0), dict(crit=-1.0),
                dict(crit=math.inf), dict(crit="1"), dict(tol=0.0), dict(tol=1.0), dict(tol=math.nan), dict(xtol=0.0), dict(xtol=2.0),
                dict(max_expand=-1), dict(max_expand=1.5), dict(max_expand=True), dict(maxit=0), dict(maxit="3"), dict(maxit=1 << 31)):
        with pytest.raises(ValueError, match="Profile"):
            Profile(**bad)


def _state(buf_ptr, **null):
    from nonlin_amd import _lib
    return _lib.ProfileState(**{k: (None if k in null else buf_ptr) for k, _ in _lib.ProfileState._fields_})


def test_entry_points_refuse_without_a_device():
    """The refusals look at the arguments only: a block of zero bytes stands in for a handle, and nothing reads it."""
    from nonlin_amd import _lib
    L = _lib.load()
    fake = C.cast(C.create_string_buffer(1 << 16), C.c_void_p)
    buf = np.ones(4096)
    v = C.c_void_p(buf.ctypes.data)
    fcn = C.cast(L.nlh_pin_device_fcn, _lib.DEVFCN)
    none = C.cast(None, _lib.DEVFCN)
    out = C.c_void_p()

    def wrap(h=fake, N=3, f=fcn, nend=4, src=v, pos=v, theta=v, o=C.byref(out)):
        return L.nlh_pin_wrap(h, N, f, none, None, nend, src, pos, theta, o)
    assert wrap(h=None) == wrap(h=None, N=1) == NLH_ERR_BAD_HANDLE                  # the handle comes first
    for bad in (dict(N=1), dict(N=0), dict(nend=-1), dict(src=None), dict(pos=None), dict(theta=None), dict(o=None)):
        assert wrap(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert wrap(f=none) == NL_UNDEFINED_FUNCTION_ERROR and not out.value
    # no live context: set and both launchers refuse; unwrap of NULL does nothing
    assert L.nlh_pin_set(None, 4, v, v, v) == NL_INVALID_INPUT_ERROR
    assert L.nlh_pin_set(fake, 4, v, v, v) == NL_INVALID_INPUT_ERROR               # (zero bytes: not a pin context)
    for launcher in (L.nlh_pin_device_fcn, L.nlh_pin_device_jac):
        assert launcher(None, None, 1, None, 2, v, 8, v) == NL_INVALID_INPUT_ERROR
        assert launcher(fake, None, 1, None, 2, v, 8, v) == NL_INVALID_INPUT_ERROR
    L.nlh_pin_unwrap(None)

    def start(h=fake, f=fcn, nprob=1, m=8, n=2, x=v, sg=v, st=None, null=()):
        s = _state(v, **{k: 1 for k in null})
        return L.nlh_profile_start_batch_device(h, f, None, nprob, m, n, x, sg, None, 3.84, 1, None, None, C.byref(s) if st is None else st)
    assert start(h=None) == start(h=None, m=0) == NLH_ERR_BAD_HANDLE
    for bad in (dict(nprob=-1), dict(m=0), dict(n=0), dict(x=None), dict(sg=None), dict(st=C.POINTER(_lib.ProfileState)()), dict(null=("end",)),
                dict(null=("C0",)), dict(null=("nfail",)), dict(nprob=1 << 30, n=2)):
        assert start(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert start(f=none) == NL_UNDEFINED_FUNCTION_ERROR
    assert start(nprob=0) == 0                                                      # nothing to do: no device

    left = C.c_int32(7)

    def step(h=fake, nprob=1, n=2, nact=1, act=v, cost=v, tol=0.01, xtol=1e-3, mx=8, maxit=30, nl=C.byref(left), null=()):
        s = _state(v, **{k: 1 for k in null})
        return L.nlh_profile_step_batch(h, nprob, n, nact, act, cost, None, C.byref(s), tol, xtol, mx, maxit, nl)
    assert step(h=None) == NLH_ERR_BAD_HANDLE
    for bad in (dict(nprob=-1), dict(n=0), dict(nact=-1), dict(act=None), dict(cost=None), dict(tol=-1.0), dict(tol=math.nan), dict(xtol=-1.0),
                dict(xtol=math.inf), dict(mx=-1), dict(maxit=0), dict(nl=None), dict(null=("phase",)), dict(nprob=1 << 30, n=2)):
        assert step(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert left.value == 7
    assert step(nprob=0, nact=0, act=None, cost=None) == 0 and left.value == 0      # no ends: none left, no device
    assert (buf == 1.0).all()


def test_one_call_refusals_without_a_device():
    """What the one-call profiles refuse before anything touches a device."""
    import torch
    from nonlin_amd import device, Expr, ParamMap
    from nonlin_amd._lib import Poisson, Loss
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(device, "_chk", lambda *a, **k: None)
        ds = object.__new__(device.DeviceSolver)
        t, y = torch.zeros(16, dtype=torch.float64), torch.zeros((2, 16), dtype=torch.float64)
        x = torch.zeros((2, 3), dtype=torch.float64)
        e = Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
        prof = Profile()
        for call in (lambda **kw: ds.expr_profile_batch(e, t, y, x, x, prof, **kw),
                     lambda **kw: ds.curve_profile_batch("expdecay", t, y, x, x, prof, baseline=0, **kw)):
            for name in ("sep", "group"):
                with pytest.raises(ValueError, match=f"a profile excludes {name}"):
                    call(**{name: object()})
            with pytest.raises(ValueError, match="a profile excludes starts"):
                call(starts=object())
            with pytest.raises(ValueError, match="stat and loss exclude each other"):
                call(stat=Poisson(), loss=Loss("huber", 1.0))
            with pytest.raises(ValueError, match="bounds|entries"):
                call(lower=[0.0, 0.0])
            with pytest.raises(ValueError, match="one free parameter"):
                call(pmap=ParamMap(3, fixed=(0, 1)))
            with pytest.raises(ValueError, match="pmap maps 2 parameters"):
                call(pmap=ParamMap(2, fixed=(0,)))
        with pytest.raises(ValueError, match="expected a Profile"):
            ds.expr_profile_batch(e, t, y, x, x, 0.95)
        e1 = Expr("a*t", ("t",), ("a",))
        with pytest.raises(ValueError, match="n = 1 is not implemented"):
            ds.expr_profile_batch(e1, t, y, x[:, :1], x[:, :1], prof)
        with pytest.raises(ValueError, match="n = 1 is not implemented"):
            ds.profile_batch_device(None, None, None, 16, x[:, :1], x[:, :1], prof)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the straight line: the profile cost is exactly quadratic, so the first trial is the end
# ---------------------------------------------------------------------------------------------------------------------
def test_straight_line_first_trial_is_the_end(oracle):
    rng = np.random.default_rng(3)
    nprob, m = 6, 24
    t = np.linspace(0.0, 5.0, m)
    y = 1.5 + 0.7 * t[None, :] + 0.2 * rng.standard_normal((nprob, m))
    res = lambda p, full: (full[0] + full[1] * t) - y[p]
    jac = lambda p, full: np.stack([np.ones(m), t], axis=1)
    x, sg, C0 = np.empty((nprob, 2)), np.empty((nprob, 2)), np.empty(nprob)
    for p in range(nprob):
        xf, fv = PC.fit(oracle, m, 2, res, jac, p, [0.0, 0.0])
        x[p], sg[p], C0[p] = xf, PC.sigma_of(jac, p, xf, fv, m, 2, True), S.cost(fv[None])[0]
    for crit in (PC.CRIT, 1.0):
        lo, hi, flags, nev, st = PR.drive(x, sg, C0, m, PR.oracle_solve(oracle, m, 2, res, jac), crit)
        rc = np.sqrt(np.float64(crit))
        assert (flags == PR.OK).all() and (nev == 1).all()
        assert np.array_equal(_bits(lo), _bits(x - rc * sg)) and np.array_equal(_bits(hi), _bits(x + rc * sg))
        assert (st["phase"] == PR.DONE).all() and (st["nexp"] == 0).all() and (st["last"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the step logic on synthetic costs
# ---------------------------------------------------------------------------------------------------------------------
def run_synthetic(nend, tol=PC.TOL, xtol=PC.XTOL, max_expand=PC.MAX_EXPAND, maxit=PC.MAXIT, crit=PC.CRIT):
    x, sigma, C0, lower, upper, cost, wfac, kinds = PC.synthetic(nend)
    m = 10
    st = PR.start(C0, x, sigma, m, crit, True, None, lower, upper)
    rounds = 0
    while True:
        act = np.flatnonzero(st["phase"] != PR.DONE)
        if len(act) == 0:
            break
        got = [cost(int(e), st["theta"][e], st) for e in act]
        left = PR.step(st, act, np.array([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int32), tol, xtol, max_expand, maxit)
        assert left == int((st["phase"] != PR.DONE).sum())
        rounds += 1
        assert rounds <= maxit + 1
    return st, wfac, kinds, lower, upper


def beyond(v, bound, s):
    """v at or past the side's bound."""
    return v >= bound if s else v <= bound


def check_synthetic(st, wfac, kinds, tol, max_expand):
    """Every end against what its synthetic cost must give; returns the set of (code, lower bit) reached."""
    seen = set()
    nend = len(st["theta"])
    for e in range(nend):
        s, k = e & 1, kinds[e]
        flag, end, xh, w0, bound = int(st["flag"][e]), st["end"][e], st["xhat"][e], st["width"][e], st["bound"][e]
        code, low = flag & 15, bool(flag & PR.LOWER)
        seen.add((code, low))
        sign = 1.0 if s else -1.0
        if not (w0 > 0):
            assert code == PR.NO_START and np.isnan(end) and st["nev"][e] == 0
        elif xh == bound:
            assert code == PR.ON_BOUND and end == bound and st["nev"][e] == 0
        elif k == 5:
            assert code == PR.FIT_FAILED and np.isnan(end) and st["nev"][e] == 4 and st["nfail"][e] == 4
        elif k in (3, 7):                                       # never rises: open -- at the bound, if the doublings reach it
            assert low == (k == 7)
            if beyond(xh + sign * 2.0 ** max_expand * w0, bound, s):
                assert code == PR.OPEN_AT_BOUND and end == bound
            else:
                assert code == PR.OPEN and end == sign * np.inf and st["nexp"][e] == max_expand
        else:
            w = wfac[e] * w0
            target = xh + sign * w
            assert not low
            far = 2.0 ** max_expand * (0.25 if k == 6 else 1.0)    # how far the doublings go, in first steps (two failures: a quarter)
            if wfac[e] > far and not beyond(xh + sign * far * w0, bound, s):
                assert code == PR.OPEN and end == sign * np.inf
            elif beyond(target, bound, s):
                # (a well whose end lies within the tolerance band past the bound is found AT the bound)
                assert end == bound and (code == PR.OPEN_AT_BOUND or (code == PR.OK and abs(target - bound) <= tol * w)), (e, flag, end)
            else:
                # |g| <= tol*delta is |u^2 - 1| <= tol, so |u - 1| <= tol/2 to first order: the end within tol*w/2 of the well's;
                # twice that is asserted (the bracket's xtol*width is far inside it)
                assert code == PR.OK and abs(end - target) <= tol * w / 2 * 2, (e, flag, end, target)
                assert st["nfail"][e] == 0 and (k != 6 or st["nev"][e] >= 3)
    return seen


def test_step_logic_on_synthetic_costs():
    st, wfac, kinds, lower, upper = run_synthetic(257)
    seen = check_synthetic(st, wfac, kinds, PC.TOL, PC.MAX_EXPAND)
    assert {(PR.OK, False), (PR.OPEN, False), (PR.OPEN, True), (PR.OPEN_AT_BOUND, False), (PR.OPEN_AT_BOUND, True), (PR.ON_BOUND, False),
            (PR.FIT_FAILED, False), (PR.NO_START, False)} <= seen
    assert (st["phase"] == PR.DONE).all() and (st["nev"] <= PC.MAXIT).all()
    assert ((st["last"] != 0) & (st["flag"] == PR.OK)).any() and ((st["nexp"] > 0) & (st["flag"] == PR.OK)).any()     # bracket and doublings
    # a well beyond 2^max_expand first steps is declared open
    st2, wfac2, kinds2, _, _ = run_synthetic(257, max_expand=2)
    seen2 = check_synthetic(st2, wfac2, kinds2, PC.TOL, 2)
    assert (PR.OPEN, False) in seen2 and int((st2["flag"] == PR.OPEN).sum()) > int((st["flag"] == PR.OPEN).sum())
    # two evaluations at the most: whoever is not done by then is MAXIT, with a finite end between the fit and the bound
    st3, _, _, _, _ = run_synthetic(65, maxit=2)
    mx = (st3["flag"] & 15) == PR.MAXIT
    assert mx.any() and (st3["nev"][mx] == 2).all() and np.isfinite(st3["end"][mx]).all() and (st3["nev"] <= 2).all()
    # a crude tolerance is met sooner, and its ends are inside the wider band
    st4, wfac4, kinds4, _, _ = run_synthetic(65, tol=0.2)
    check_synthetic(st4, wfac4, kinds4, 0.2, PC.MAX_EXPAND)
    st5, _, _, _, _ = run_synthetic(65)
    assert st4["nev"].sum() < st5["nev"].sum()


def test_an_end_does_not_depend_on_the_others():
    """A batch's ends one by one: the same bits."""
    st, _, _, _, _ = run_synthetic(64)
    x, sigma, C0, lower, upper, cost, wfac, kinds = PC.synthetic(64)
    one = PR.start(C0, x, sigma, 10, PC.CRIT, True, None, lower, upper)
    for e in range(len(one["theta"])):
        while one["phase"][e] != PR.DONE:
            c, f = cost(e, one["theta"][e], one)
            PR.step(one, np.array([e]), np.array([c]), np.array([f], dtype=np.int32), PC.TOL, PC.XTOL, PC.MAX_EXPAND, PC.MAXIT)
    for k in PR.NAMES:
        assert np.array_equal(one[k].view(np.uint64 if k in PR.F64 else np.int32), st[k].view(np.uint64 if k in PR.F64 else np.int32)), k


# ---------------------------------------------------------------------------------------------------------------------
# 5. the study
# ---------------------------------------------------------------------------------------------------------------------
def test_study(oracle):
    """tests/golden/profile_study.json: its figures follow from its own per-data-set marks, and the data sets PC.CHECK of every
    family, recomputed here, give the recorded bits.  No coverage is a condition: the file is the study as it fell."""
    with open(PC.STUDY_GOLDEN) as fh:
        rec = json.load(fh)
    assert float.fromhex(rec["crit"]) == PC.CRIT and (rec["tol"], rec["xtol"], rec["max_expand"], rec["maxit"]) == (PC.TOL, PC.XTOL, PC.MAX_EXPAND, PC.MAXIT)
    assert len(rec["study"]) == len(PC.FAMILIES) == 4
    for fam, s in zip(PC.FAMILIES, rec["study"]):
        n = s["ndata"]
        assert tuple(s["family"]) == fam and n == PC.ndata_of(fam) == (2000 if fam[0] == "mm" else 300)
        for r in PC.ROWS:
            for q in s["params"]:
                marks = s[r]["marks"][q]
                assert len(marks) == n and set(marks) <= set("abc")
                tot = 0.0
                for key, ch in (("covers", "c"), ("truth_above", "a"), ("truth_below", "b")):
                    v = s[r][key][q]
                    assert v == marks.count(ch) / n and s[r][key + "_stderr"][q] == math.sqrt(v * (1.0 - v) / n)
                    tot += v
                assert abs(tot - 1.0) < 1e-12
        nends = n * len(s["params"]) * 2
        assert sum(s["flag_counts"].values()) == nends and 1.0 <= s["mean_refits_per_end"] <= PC.MAXIT
        data = PC.family(fam)
        for p in PC.CHECK:
            got, want = PC.one(oracle, fam, p, data), s["check"][str(p)]
            for k in ("x", "sigma", "lo", "hi"):
                assert [float(a).hex() for a in got[k]] == want[k], (fam, p, k)
            assert got["flags"] == want["flags"] and got["nev"] == want["nev"], (fam, p)
