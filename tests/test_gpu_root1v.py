"""GPU tests of brent_solver and newton_1var_solver (brent_solve / newt1var_solve, src/nonlin_solve.f90:643-1032): the
device state machine behind host callbacks (nlh_brent_solve, nlh_newton_1var_solve and the Python types), behind the
user's device launchers (the *_batch_device entry points), behind a model (the Fortran shim's solve_batch) and through
the Fortran shim, against the plain-Python restatement of tests/root1v_restatement.py.  Every comparison is bitwise: x,
f, all seven iteration_behavior fields and the status -- and, for the host callbacks, the points they were called at."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import root1v_restatement as R
import scalar_models as SM

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
IB_KEYS = ("iter_count", "fcn_count", "jacobian_count", "gradient_count", "converge_on_fcn", "converge_on_chng",
           "converge_on_zero_diff")
BATCH_OPTS = dict(max_evals=40, ftol=1e-12, xtol=1e-12, gtol=1e-10)
RKW = dict(max_evals=40, ftol=1e-12, xtol=1e-12)


def _bits(v):
    return struct.pack("<d", float(v))


def _restate(kind, f, x1, x2, diff=None, want_f=True, x_in=0.0, max_evals=100, ftol=1e-8, xtol=1e-12, gtol=1e-12, args=None):
    if kind == "brent":
        return R.brent_solve(f, x1, x2, max_evals=max_evals, ftol=ftol, xtol=xtol, args=args)
    return R.newt1var_solve(f, x1, x2, diff=diff, max_evals=max_evals, ftol=ftol, xtol=xtol, dtol=gtol, args=args,
                            want_f=want_f, x_in=x_in)


def _c_solve(kind, f, x1, x2, diff=None, want_f=True, x_in=0.0, args=None, **kw):
    """The C entry point with ctypes callbacks that record every point: returns (rc, x, f, ib dict, fcn points, diff
    points)."""
    from nonlin_amd import _lib, api
    h = api.default_handle()
    o = _lib.default_options()
    for k, v in kw.items():
        setattr(o, k, v)
    pts, dpts = [], []

    def cb(ctx, n, xp):
        pts.append(xp[0])
        return float(f(xp[0], args))

    def cbd(ctx, n, xp):
        dpts.append(xp[0])
        return float(diff(xp[0], args))
    cf = _lib.FCNNVAR(cb)
    cd = _lib.FCNNVAR(cbd) if diff is not None else C.cast(None, _lib.FCNNVAR)
    x = C.c_double(x_in)
    fo = C.c_double(-123.0)
    ib = _lib.IterationBehavior()
    fp = C.cast(C.byref(fo), _lib.c_double_p) if want_f else None
    xp = C.cast(C.byref(x), _lib.c_double_p)
    if kind == "brent":
        rc = h.lib.nlh_brent_solve(h.ptr, C.byref(o), cf, None, x1, x2, xp, fp, C.byref(ib))
    else:
        rc = h.lib.nlh_newton_1var_solve(h.ptr, C.byref(o), cf, cd, None, x1, x2, xp, fp, C.byref(ib))
    h.check(rc, kind)
    return rc, x.value, (fo.value if want_f else None), ib.as_dict(), pts, dpts


def _same(rc, x, fo, ib, r):
    assert rc == r["status"], (rc, r["status"])
    for k in IB_KEYS:
        assert int(ib[k]) == int(r[k]), (k, ib, r)
    assert _bits(x) == _bits(r["x"]), (x, r["x"])
    if r["f"] is not None:
        assert _bits(fo) == _bits(r["f"]), (fo, r["f"])


def _check_host(kind, f, x1, x2, diff=None, want_f=True, x_in=0.0, args=None, **kw):
    r = _restate(kind, f, x1, x2, diff=diff, want_f=want_f, x_in=x_in, args=args, **kw)
    rc, x, fo, ib, pts, dpts = _c_solve(kind, f, x1, x2, diff=diff, want_f=want_f, x_in=x_in, args=args, **kw)
    _same(rc, x, fo, ib, r)
    assert pts == r["points"] and dpts == r["dpoints"]          # every callback, in the reference's order
    return r


# ------------------------------------------------------------------------------------------------ host-callback form
@pytest.mark.parametrize("kind", ["brent", "newton"])
def test_host_form_reference_problems(kind):
    """test_brent_1 / _2, test_newton_1var_1 / _2 (math.sin, with and without args) and the newton1d example's cubic."""
    r1 = _check_host(kind, R.sinx_over_x, 1.5, 5.0)
    r2 = _check_host(kind, R.a_sinx_over_x, 1.5, 5.0, args=2.0)
    assert abs(r1["x"] - math.pi) < 1e-6 and abs(r2["x"] - math.pi) < 1e-6
    r3 = _check_host(kind, R.example_cubic, 2.0, -2.0)
    assert abs(r3["x"] - 1.618033988749895) < 1e-6
    # through the Python types: (x, f), NonlinError after ib is filled
    import nonlin_amd as nl
    s = nl.brent_solver() if kind == "brent" else nl.newton_1var_solver()
    obj = nl.fcn1var_helper()
    obj.set_fcn(R.a_sinx_over_x)
    ib = nl.iteration_behavior()
    x, fo = s.solve(obj, nl.value_pair(1.5, 5.0), ib=ib, args=2.0)
    _same(0, x, fo, ib.as_dict(), r2)
    s.set_max_fcn_evals(4)
    with pytest.raises(nl.NonlinError) as e:
        s.solve(obj, nl.value_pair(1.5, 5.0), ib=ib, args=2.0)
    assert e.value.code == 106 and ib.fcn_count == _restate(kind, R.a_sinx_over_x, 1.5, 5.0, max_evals=4, args=2.0)["fcn_count"]


@pytest.mark.parametrize("kind", ["brent", "newton"])
def test_host_form_exits(kind):
    f, df = R.cubic((-1.0, -2.0, 0.0, 1.0))
    r = _check_host(kind, f, 2.0, -2.0, max_evals=5)                       # a max-evaluations stop
    assert r["status"] == 106
    if kind == "brent":
        assert r["x"] == 0.0                                                # x written only on convergence
    r = _check_host(kind, lambda x, a: x - 2.0, 2.0, -3.0)                  # an endpoint root
    assert r["converge_on_fcn"] and r["fcn_count"] == (2 if kind == "newton" else r["fcn_count"])
    r = _check_host(kind, f, 1e-20, 3e-20, x_in=4.5)                       # an invalid bracket: no callback made
    assert r["status"] == 201 and r["points"] == []
    if kind == "newton":
        assert r["x"] == 4.5
        rd = _check_host(kind, f, 2.0, -2.0, gtol=1e3)                      # the derivative-tolerance exit
        assert rd["converge_on_zero_diff"]
        rb = _check_host(kind, f, 2.0, -2.0, ftol=0.0, xtol=1e-3)           # the Newton-step exit (:964)
        assert rb["exit"] == "newton_step" and rb["x"] not in rb["points"][:-1]
        step = lambda x, a: -1.0 if x < 0.3 else 1.0                          # noqa: E731
        for d in (None, lambda x, a: 0.0):                                  # the bisection exit (:953)
            for wf in (True, False):
                rs = _check_host(kind, step, -2.0, 2.0, diff=d, want_f=wf, gtol=0.0, xtol=1e-6)
                assert rs["exit"] == "bisection" and rs["iter_count"] == 22
                assert rs["x"] not in (rs["points"][:-1] if wf else rs["points"])     # nothing at the new x but the extra f
        for d in (None, df):                                                # f absent against f present
            ra = _check_host(kind, f, 2.0, -2.0, diff=d, want_f=False)
            rp = _check_host(kind, f, 2.0, -2.0, diff=d, want_f=True)
            assert rp["fcn_count"] == ra["fcn_count"] + 1
        _check_host(kind, f, 2.0, -2.0, diff=df, max_evals=5)
    else:
        rx = _check_host(kind, f, 2.0, -2.0, ftol=0.0)                      # converges on the change in x
        assert rx["converge_on_chng"]
        rn = _check_host(kind, lambda x, a: math.nan if x >= 1.0 else x - 0.5, 0.0, 1.0)   # c, d, e unset: f NaN at b
        assert rn["x"] == 0.5 and rn["points"] == [0.0, 1.0, 0.5]


def test_host_form_undefined_function():
    from nonlin_amd import _lib, api
    h = api.default_handle()
    o = _lib.default_options()
    x, fo, ib = C.c_double(3.0), C.c_double(3.0), _lib.IterationBehavior()
    ib.fcn_count = 5
    null = C.cast(None, _lib.FCNNVAR)
    xp, fp = C.cast(C.byref(x), _lib.c_double_p), C.cast(C.byref(fo), _lib.c_double_p)
    assert h.lib.nlh_brent_solve(h.ptr, C.byref(o), null, None, 0.0, 1.0, xp, fp, C.byref(ib)) == 211
    assert x.value == 0.0 and fo.value == 0.0 and ib.fcn_count == 0          # x = 0 precedes the check (:691)
    x.value = 3.0
    assert h.lib.nlh_newton_1var_solve(h.ptr, C.byref(o), null, null, None, 0.0, 1.0, xp, fp, C.byref(ib)) == 211
    assert x.value == 3.0 and fo.value == 0.0
    import nonlin_amd as nl
    with pytest.raises(nl.NonlinError) as e:
        nl.brent_solver().solve(nl.fcn1var_helper(), nl.value_pair(0.0, 1.0))
    assert e.value.code == 211


@pytest.mark.parametrize("kind", ["brent", "newton"])
def test_host_form_print_status(kind, capfd):
    import nonlin_amd as nl
    s = nl.brent_solver() if kind == "brent" else nl.newton_1var_solver()
    s.set_print_status(True)
    obj = nl.fcn1var_helper()
    obj.set_fcn(R.example_cubic)
    capfd.readouterr()
    s.solve(obj, nl.value_pair(2.0, -2.0))
    out = capfd.readouterr().out
    assert out == R.status_text(_restate(kind, R.example_cubic, 2.0, -2.0)) and out.count("Iteration:") > 3
    s.set_max_fcn_evals(6)
    with pytest.raises(nl.NonlinError):
        s.solve(obj, nl.value_pair(2.0, -2.0))
    assert capfd.readouterr().out == R.status_text(_restate(kind, R.example_cubic, 2.0, -2.0, max_evals=6))


# ------------------------------------------------------------------------------------------------ the user's device launchers
def _device_solve(ds, kind, c, lim, diff=False, count=False, want_f=True, x0=-7.0, opts=None):
    """Returns (x, fout, status, ib, batch) -- batch still open when count (the caller closes it)."""
    import torch
    from nonlin_amd import _lib
    from nonlin_amd.device import IB_DTYPE
    b = SM.CubicBatch(c, count=count)
    dlim = torch.tensor(lim, dtype=torch.float64, device="cuda")
    x = torch.full((len(c),), x0, dtype=torch.float64, device="cuda")
    o = opts or ds.options(**BATCH_OPTS)
    if want_f:
        if kind == "brent":
            fo, st, ib = ds.brent_solve_batch_device(b.launch, b.ctx, dlim, x, opts=o)
        else:
            fo, st, ib = ds.newton_1var_solve_batch_device(b.launch, b.ctx, dlim, x, diff=b.launch_diff if diff else None, opts=o)
    else:                                               # f absent: fout NULL
        nprob = len(c)
        ibc = (_lib.IterationBehavior * nprob)()
        stc = (C.c_int32 * nprob)()
        rc = ds.lib.nlh_newton_1var_solve_batch_device(ds.h.ptr, C.byref(o), nprob, ds._devfcn(b.launch),
                                                       ds._devfcn(b.launch_diff if diff else None), b.ctx, dlim.data_ptr(),
                                                       x.data_ptr(), None, ibc, stc)
        assert rc == 0
        fo, st, ib = None, np.array(stc, dtype=np.int32), np.frombuffer(ibc, dtype=IB_DTYPE)
    torch.cuda.synchronize()
    xs = x.cpu().numpy()
    if not count:
        b.close()
        b = None
    return xs, fo, st, ib, b


def _check_problem(kind, c, lim, p, xs, fo, st, ib, diff=False, want_f=True, x0=-7.0):
    f, df = R.cubic(c[p])
    r = _restate(kind, f, lim[p, 0], lim[p, 1], diff=df if diff else None, want_f=want_f, x_in=x0, **RKW, gtol=1e-10)
    _same(int(st[p]), xs[p], None if fo is None else fo[p], {k: int(ib[k][p]) for k in IB_KEYS}, r)
    return r


@pytest.mark.parametrize("kind,diff", [("brent", False), ("newton", False), ("newton", True)])
def test_device_form_mixed_outcomes(ds, kind, diff):
    """4096 cubics: every exit of the solver, invalid brackets inside the batch, each problem bitwise against the
    restatement; the counting launcher sees each round's points in ascending problem order, and per problem exactly
    the restatement's points (its counted evaluations plus its uncounted forward-difference points)."""
    c, lim = SM.cubic_problems(4096)
    xs, fo, st, ib, b = _device_solve(ds, kind, c, lim, diff=diff, count=True)
    try:
        pts, probs = b.points()
        sizes = b.call_sizes()
        dcalls = b.calls(deriv=True)
    finally:
        b.close()
    rs = [_check_problem(kind, c, lim, p, xs, fo, st, ib, diff=diff) for p in range(len(c))]
    seen = {r["exit"] for r in rs}                                            # the statement that ended each solve
    want = {"fcn", "max_evals", "invalid"} | ({"xm"} if kind == "brent" else {"endpoint", "bisection", "newton_step"})
    if kind == "newton" and not diff:
        want |= {"diff"}                                                      # derivative-tolerance exits
    assert want <= seen, seen
    # one list per round, each in ascending problem order
    at = 0
    for n in sizes:
        assert np.all(np.diff(probs[at:at + n]) >= 0)
        at += n
    assert at == len(pts) == sum(len(r["points"]) for r in rs)
    order = np.argsort(probs, kind="stable")
    bounds = np.searchsorted(probs[order], np.arange(len(c) + 1))
    for p in range(len(c)):
        got = pts[order[bounds[p]:bounds[p + 1]]]
        assert [_bits(v) for v in got] == [_bits(v) for v in rs[p]["points"]], p
    if kind == "newton" and diff:
        assert 0 < dcalls < len(sizes)                                        # once per round after round 0


def test_device_form_f_absent(ds):
    c, lim = SM.cubic_problems(512, seed=3)
    for diff in (False, True):
        xs, fo, st, ib, _ = _device_solve(ds, "newton", c, lim, diff=diff, want_f=False)
        for p in range(len(c)):
            _check_problem("newton", c, lim, p, xs, fo, st, ib, diff=diff, want_f=False)


def test_device_form_scale_and_batch_independence(ds):
    """2^20 problems; 2000 of them, sampled by seed, against the restatement, and solved again as their own batch: the
    same bits."""
    n = 1 << 20
    c, lim = SM.cubic_problems(n, seed=11)
    sample = np.sort(np.random.default_rng(5).choice(n, 2000, replace=False))
    for kind, diff in (("brent", False), ("newton", False), ("newton", True)):
        xs, fo, st, ib, _ = _device_solve(ds, kind, c, lim, diff=diff)
        for p in sample:
            _check_problem(kind, c, lim, p, xs, fo, st, ib, diff=diff)
        xs2, fo2, st2, ib2, _ = _device_solve(ds, kind, c[sample], lim[sample], diff=diff)
        assert [_bits(v) for v in xs2] == [_bits(v) for v in xs[sample]]
        assert [_bits(v) for v in fo2] == [_bits(v) for v in fo[sample]]
        assert np.array_equal(st2, st[sample]) and np.array_equal(ib2, ib[sample])


def test_host_twins_match_restatement():
    so = SM.lib()
    c, lim = SM.cubic_problems(64)
    for p in range(64):
        f, df = R.cubic(c[p])
        cp = c[p].ctypes.data_as(SM.dp)
        for xv in (lim[p, 0], lim[p, 1], 0.5 * (lim[p, 0] + lim[p, 1]), 1e-3):
            assert _bits(so.cubic_host_f(cp, xv)) == _bits(f(xv)) and _bits(so.cubic_host_df(cp, xv)) == _bits(df(xv))


def test_model_form_matches_device_form(ds):
    from nonlin_amd import _lib
    c, lim = SM.cubic_problems(1000, seed=9)
    for kind, diff in (("brent", False), ("newton", False), ("newton", True)):
        xs, fo, st, ib, _ = _device_solve(ds, kind, c, lim, diff=diff)
        b = SM.CubicBatch(c)
        md = C.c_void_p()
        try:
            assert ds.lib.nlh_device_fcn_model_create(len(c), 1, 1, ds._devfcn(b.launch),
                                                      ds._devfcn(b.launch_diff if diff else None), b.ctx, C.byref(md)) == 0
            x = np.full(len(c), -7.0)
            fout = np.zeros(len(c))
            ibm = (_lib.IterationBehavior * len(c))()
            stm = (C.c_int32 * len(c))()
            fn = ds.lib.nlh_dq_model_brent_solve if kind == "brent" else ds.lib.nlh_dq_model_newton_1var_solve
            rc = fn(ds.h.ptr, C.byref(ds.options(**BATCH_OPTS)), md, lim.ctypes.data_as(_lib.c_double_p),
                    x.ctypes.data_as(_lib.c_double_p), fout.ctypes.data_as(_lib.c_double_p), ibm, stm)
            assert rc == 0
            assert x.tobytes() == xs.tobytes() and fout.tobytes() == fo.tobytes()
            assert np.array_equal(np.array(stm), st) and [ibm[k].as_dict() for k in range(len(c))] == \
                [{k: int(ib[k][p]) for k in IB_KEYS} for p in range(len(c))]
        finally:
            ds.lib.nlh_dq_model_destroy(md)
            b.close()
    # a model of n = 2 unknowns, or of the dense-quadratic family, has no one-variable form
    b = SM.CubicBatch(c)
    md = C.c_void_p()
    try:
        assert ds.lib.nlh_device_fcn_model_create(len(c), 1, 2, ds._devfcn(b.launch), ds._devfcn(None), b.ctx, C.byref(md)) == 0
        x = np.zeros(len(c))
        for fn in (ds.lib.nlh_dq_model_brent_solve, ds.lib.nlh_dq_model_newton_1var_solve):
            assert fn(ds.h.ptr, C.byref(ds.options()), md, lim.ctypes.data_as(_lib.c_double_p),
                      x.ctypes.data_as(_lib.c_double_p), None, None, None) == 104
    finally:
        ds.lib.nlh_dq_model_destroy(md)
        b.close()
    m = ds.model(np.ones((2, 1, 1)), np.ones((2, 1)), 0.5)
    lim2 = np.array([[0.0, 1.0], [0.0, 1.0]])
    x2 = np.zeros(2)
    assert ds.lib.nlh_dq_model_brent_solve(ds.h.ptr, C.byref(ds.options()), m._md, lim2.ctypes.data_as(_lib.c_double_p),
                                           x2.ctypes.data_as(_lib.c_double_p), None, None, None) == 104


def test_error_paths(ds):
    import torch
    from nonlin_amd import _lib
    null = C.cast(None, _lib.DEVFCN)
    lim = torch.zeros((2, 2), dtype=torch.float64, device="cuda")
    x = torch.zeros(2, dtype=torch.float64, device="cuda")
    ib = (_lib.IterationBehavior * 2)()
    ib[1].fcn_count = 5
    o = ds.options()
    assert ds.lib.nlh_brent_solve_batch_device(ds.h.ptr, C.byref(o), 2, null, None, lim.data_ptr(), x.data_ptr(), None, ib,
                                               None) == 211
    assert ib[1].fcn_count == 0
    c, _ = SM.cubic_problems(2)
    b = SM.CubicBatch(c)
    try:
        f = ds._devfcn(b.launch)
        assert ds.lib.nlh_newton_1var_solve_batch_device(ds.h.ptr, C.byref(o), -1, f, null, b.ctx, lim.data_ptr(),
                                                         x.data_ptr(), None, None, None) == 201
        assert ds.lib.nlh_brent_solve_batch_device(ds.h.ptr, C.byref(o), 0, f, b.ctx, None, None, None, None, None) == 0
        # a launcher that fails: the library reports the user's return code and stops
        bad = _lib.DEVFCN(lambda ctx, stream, npoints, dprob, n, dx, m, df: 7)
        with pytest.raises(RuntimeError):
            ds.brent_solve_batch_device(bad, None, torch.tensor([[0.0, 1.0], [0.0, 1.0]], dtype=torch.float64, device="cuda"), x)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ Fortran
def _unhex(h):
    return struct.unpack(">d", bytes.fromhex(h))[0]


@pytest.fixture(scope="module")
def fortran_exe(tmp_path_factory):
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    shim = os.path.join(ROOT, "nonlin_amd", "fortran", "build")
    if fc is None:
        pytest.skip("no Fortran compiler")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "nonlin_amd", "fortran"), "-s"])
    SM.lib()                                                   # builds tests/device_1var/libscalar_models.so if needed
    d = tmp_path_factory.mktemp("fortran_root1v")
    exe = str(d / "root1v_suite")
    libdir, smdir = os.path.join(ROOT, "nonlin_amd"), os.path.join(HERE, "device_1var")
    subprocess.check_call([fc, "-O2", "-I" + shim, "-module-dir", str(d),
                           os.path.join(HERE, "fortran_root1v", "root1v_suite.f90"), "-o", exe,
                           os.path.join(shim, "libnonlin_shim.a"), "-L" + libdir, "-lnonlin_hip", "-L" + smdir,
                           "-lscalar_models", "-Wl,-rpath," + libdir, "-Wl,-rpath," + smdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_fortran_shim_bitwise(fortran_exe):
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    res = {}
    for line in out.stdout.splitlines():
        t = line.split()
        if not t or t[0].startswith("#"):
            continue
        res.setdefault(t[0], []).append(t[1:])

    def cmp(row, r):
        assert int(row[0]) == r["status"], (row, r["status"])
        assert [int(v) for v in row[1:5]] == [r["iter_count"], r["fcn_count"], r["jacobian_count"], 0], (row, r)
        assert row[5:8] == ["T" if r[k] else "F" for k in ("converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")]
        assert _bits(_unhex(row[8])) == _bits(r["x"]) and _bits(_unhex(row[9])) == _bits(r["f"]), (row, r["x"], r["f"])

    cub = R.cubic((-1.0, -2.0, 0.0, 1.0))
    cmp(res["brent_cubic"][0], R.brent_solve(cub[0], 2.0, -2.0))
    cmp(res["user_brent_cubic"][0], R.brent_solve(cub[0], 2.0, -2.0))      # a user type with the reference's interface
    cmp(res["newton_cubic"][0], R.newt1var_solve(cub[0], 2.0, -2.0))
    cmp(res["newton_cubic_diff"][0], R.newt1var_solve(cub[0], 2.0, -2.0, diff=cub[1]))
    cmp(res["newton_cubic_args"][0], R.newt1var_solve(R.cubic((-1.0, -2.0, 0.0, 3.0))[0], 2.0, -2.0))
    for key in ("brent_sin", "newton_sin"):
        assert abs(_unhex(res[key][0][8]) - math.pi) < 1e-6            # sin(x)/x with flang's sin: the reference's 1e-6
    # solve_batch on the device model of the cubic family: c(:,k) = (-1 - k/8, -2, 0, 1), lim = (2, -2) (1-based k)
    for key, kind, diff in (("brent_batch", "brent", False), ("newton_batch", "newton", False),
                            ("newton_batch_diff", "newton", True)):
        assert len(res[key]) == 5
        for k in range(5):
            f, df = R.cubic((-1.0 - (k + 1) / 8.0, -2.0, 0.0, 1.0))
            cmp(res[key][k], _restate(kind, f, 2.0, -2.0, diff=df if diff else None, x_in=0.0))


def test_fortran_error_stop_on_max_evals(fortran_exe):
    out = subprocess.run(["timeout", "-k", "10", "120", fortran_exe, "errstop"], capture_output=True, text=True)
    assert out.returncode == 106, (out.returncode, out.stderr)
    assert "not reached" not in out.stdout
