"""GPU tests of nelder_mead (nm_solve, src/nonlin_optimize.f90:104-340): the device state machine behind a host callback
(nelder_mead.solve), behind the user's device launcher (nlh_nelder_mead_solve_batch_device) and behind a model of one
function (nlh_dq_model_nelder_mead_solve, the Fortran shim's solve_batch) against the plain-Python restatement of
tests/nm_restatement.py.  Every comparison is bitwise: x, fout, every ib field, the status and the final simplex."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import nm_restatement as R
import user_models as UM

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)


def _helper(f, n):
    import nonlin_amd as nl
    h = nl.fcnnvar_helper()
    h.set_fcn(f, n)
    return h


def _host_solve(f, x0, args=None, simplex=None, solver=None, **kw):
    """nelder_mead().solve on numpy x; returns (x, fout, ib dict, status, final simplex, solver)."""
    import nonlin_amd as nl
    s = solver or nl.nelder_mead()
    for k, v in kw.items():
        getattr(s, "set_" + k)(v)
    if simplex is not None:
        s.set_simplex(simplex)
    x = np.array(x0, dtype=np.float64)
    ib = nl.iteration_behavior()
    try:
        fo = s.solve(_helper(lambda xx, a: f(list(xx), a), len(x)), x, ib=ib, args=args)
        st = 0
    except nl.NonlinError as e:
        st, fo = e.code, None
    return x, fo, ib.as_dict(), st, s.get_simplex(), s


def _same_as_restatement(x, fo, ib, st, sim, r, x0=None):
    assert st == r["status"], (st, r["status"])
    assert ib["iter_count"] == r["iter_count"] and ib["fcn_count"] == r["fcn_count"], (ib, r["iter_count"], r["fcn_count"])
    assert ib["jacobian_count"] == 0 and ib["gradient_count"] == 0
    assert ib["converge_on_fcn"] == r["converge_on_fcn"] and not ib["converge_on_chng"] and not ib["converge_on_zero_diff"]
    if st == 0:
        assert fo == r["fout"]
        assert np.array_equal(x, np.array(r["x"])), (x, r["x"])
    else:
        assert np.array_equal(x, np.array(x0, dtype=np.float64))        # x untouched (:316-319)
    assert np.array_equal(sim, np.array(r["simplex"]).T), (sim, r["simplex"])


def _quad1(x, a=None):
    d = x[0] - 2.0
    return d * d + 0.5


def _rosen2(x, a):
    t = x[1] - x[0] * x[0]
    u = x[0] - 1.0
    return a * (t * t) + u * u


# ------------------------------------------------------------------------------------------------ host-callback form
@pytest.mark.parametrize("name,f,x0,args", [
    ("rosenbrock", R.rosenbrock, [0.0, 0.0], None),
    ("beale", R.beale, [1.0, 1.0], None),
    ("rosenbrock_args", _rosen2, [0.0, 0.0], 100.0),
    ("one_d", _quad1, [-3.0], None),
])
def test_host_form_bitwise(name, f, x0, args):
    x, fo, ib, st, sim, _ = _host_solve(f, x0, args=args)
    r = R.nm_solve(f, x0, args=args)
    _same_as_restatement(x, fo, ib, st, sim, r, x0)
    if name == "rosenbrock":
        assert r["shrinks"] > 0                      # the shrink path ran
        assert _host_solve(f, x0)[0].tolist() == x.tolist()


def test_host_form_user_simplex_ignores_x():
    sim0 = np.array([[-1.0, 0.5, 2.0], [1.5, -0.25, 0.75]])          # n x (n+1), Fortran layout
    x0 = [100.0, 100.0]
    x, fo, ib, st, sim, _ = _host_solve(R.rosenbrock, x0, simplex=sim0)
    r = R.nm_solve(R.rosenbrock, x0, simplex=sim0.T.tolist())
    _same_as_restatement(x, fo, ib, st, sim, r, x0)
    # a simplex of the wrong shape is replaced by one built from x (:176-188)
    x, fo, ib, st, sim, _ = _host_solve(R.rosenbrock, [0.5, 0.5], simplex=np.ones((3, 3)), initial_size=0.5)
    _same_as_restatement(x, fo, ib, st, sim, R.nm_solve(R.rosenbrock, [0.5, 0.5], init_size=0.5), [0.5, 0.5])


def test_host_form_second_solve_continues():
    x, fo, ib, st, sim, s = _host_solve(R.rosenbrock, [0.0, 0.0])
    r1 = R.nm_solve(R.rosenbrock, [0.0, 0.0])
    _same_as_restatement(x, fo, ib, st, sim, r1, [0.0, 0.0])
    x2, fo2, ib2, st2, sim2, _ = _host_solve(R.beale, [7.0, -3.0], solver=s)
    r2 = R.nm_solve(R.beale, [7.0, -3.0], simplex=r1["simplex"])
    _same_as_restatement(x2, fo2, ib2, st2, sim2, r2, [7.0, -3.0])


def test_host_form_max_evals():
    """A max-evaluations stop: NonlinError(106) after ib and the simplex are stored, x untouched, fout the stale f(1) of the
    initial simplex -- including a stop where a shrink carried neval past the limit (:299, :316)."""
    import nonlin_amd as nl
    shrink_stop = None
    for me in range(4, 170):
        r = R.nm_solve(R.rosenbrock, [0.0, 0.0], max_evals=me)
        if r["status"] == 106 and r["fcn_count"] >= me + 2:
            shrink_stop = me
            break
    assert shrink_stop is not None
    for me in (40, shrink_stop):
        r = R.nm_solve(R.rosenbrock, [0.0, 0.0], max_evals=me)
        x, fo, ib, st, sim, s = _host_solve(R.rosenbrock, [0.0, 0.0], max_fcn_evals=me)
        assert st == 106
        _same_as_restatement(x, fo, ib, st, sim, r, [0.0, 0.0])
        # fout of a flag exit: the stale f(1) of the initial simplex, through the C ABI
        from nonlin_amd import _lib, api
        h = api.default_handle()
        o = _lib.default_options()
        o.max_evals, o.gtol = me, 1e-12
        xx, fout, cib = np.zeros(2), C.c_double(-1.0), _lib.IterationBehavior()
        cf = _lib.FCNNVAR(lambda ctx, n, p: R.rosenbrock([p[0], p[1]]))
        rc = h.lib.nlh_nelder_mead_solve(h.ptr, C.byref(o), 1.0, 2, cf, None, xx.ctypes.data_as(_lib.c_double_p), None, 0,
                                         C.cast(C.byref(fout), _lib.c_double_p), C.byref(cib))
        assert rc == 106 and fout.value == R.rosenbrock([0.0, 0.0]) == r["fout"] and xx.tolist() == [0.0, 0.0]
        assert cib.fcn_count == r["fcn_count"]
    s = nl.nelder_mead()
    s.set_max_fcn_evals(10)
    ib = nl.iteration_behavior()
    x = np.zeros(2)
    with pytest.raises(nl.NonlinError) as e:
        s.solve(_helper(lambda xx, a: R.rosenbrock(list(xx)), 2), x, ib=ib)
    assert e.value.code == 106
    r = R.nm_solve(R.rosenbrock, [0.0, 0.0], max_evals=10)
    assert ib.fcn_count == r["fcn_count"] and np.array_equal(s.get_simplex(), np.array(r["simplex"]).T)


def test_host_form_print_status(capfd):
    import nonlin_amd as nl
    s = nl.nelder_mead()
    s.set_print_status(True)
    s.set_max_fcn_evals(60)
    capfd.readouterr()
    with pytest.raises(nl.NonlinError):
        s.solve(_helper(lambda xx, a: R.rosenbrock(list(xx)), 2), np.zeros(2))
    out = capfd.readouterr().out
    r = R.nm_solve(R.rosenbrock, [0.0, 0.0], max_evals=60)
    assert out == R.status_text(r)
    assert "Function Value:  0.100E+01" in out                 # the stale f(1) of the initial simplex
    s = nl.nelder_mead()
    s.set_print_status(True)
    s.solve(_helper(lambda xx, a: R.beale(list(xx)), 2), np.ones(2))
    assert capfd.readouterr().out == R.status_text(R.nm_solve(R.beale, [1.0, 1.0]))


# ------------------------------------------------------------------------------------------------ the user's device launcher
def _crosen_restated(c, x0, max_evals=500, init_size=1.0, simplex=None):
    so = UM.lib()
    n = len(x0)

    def f(x, a):
        return so.crosen_host_f(float(c), n, (C.c_double * n)(*x))
    return R.nm_solve(f, list(x0), simplex=simplex, max_evals=max_evals, init_size=init_size)


def _device_solve(ds, c, x0, max_evals=500, init_size=1.0, simplex=None):
    import torch
    batch = UM.BtriBatch(c)
    try:
        x = torch.tensor(x0, dtype=torch.float64, device="cuda")
        nprob, n = x0.shape
        sim = torch.tensor(simplex, dtype=torch.float64, device="cuda") if simplex is not None else \
            torch.zeros((nprob, n + 1, n), dtype=torch.float64, device="cuda")
        if simplex is None:          # the final simplex through dsimplex: built from x (use_simplex = 0), written back
            from nonlin_amd import _lib
            ib = (_lib.IterationBehavior * nprob)()
            status = (C.c_int32 * nprob)()
            fout = (C.c_double * nprob)()
            o = ds.options(max_evals=max_evals)
            rc = ds.lib.nlh_nelder_mead_solve_batch_device(ds.h.ptr, C.byref(o), float(init_size), nprob, n,
                                                           ds._devfcn(batch.crosen_launch), batch.ctx, x.data_ptr(),
                                                           sim.data_ptr(), 0, fout, ib, status)
            ds.check(rc, "nlh_nelder_mead_solve_batch_device")
            assert rc == 0
            res = ([float(v) for v in fout], [ib[k].as_dict() for k in range(nprob)], [int(status[k]) for k in range(nprob)])
        else:
            res = ds.nelder_mead_solve_batch_device(batch.crosen_launch, batch.ctx, x, simplex=sim, init_size=init_size,
                                                    opts=ds.options(max_evals=max_evals))
        torch.cuda.synchronize()
        return x.cpu().numpy(), sim.cpu().numpy(), res
    finally:
        batch.close()


def _check_device(xg, simg, res, p, r, x0):
    fout, ibs, st = res
    _same_as_restatement(xg[p], fout[p], ibs[p], st[p], simg[p].T, r, x0)
    assert fout[p] == r["fout"]                                 # (also on a flag exit: the stale f(1))


@pytest.mark.parametrize("nprob,n,max_evals", [(1, 1, 500), (7, 2, 500), (300, 5, 500), (4096, 8, 500), (7, 16, 500),
                                               (300, 16, 300), (7, 70, 400)])
def test_device_form_bitwise(ds, nprob, n, max_evals):
    c, x0 = UM.crosen_problems(nprob, n, seed=100 + n)
    xg, simg, res = _device_solve(ds, c, x0, max_evals=max_evals)
    sample = range(nprob) if nprob <= 8 else sorted(set(np.linspace(0, nprob - 1, 12).astype(int).tolist()))
    for p in sample:
        _check_device(xg, simg, res, p, _crosen_restated(c[p], x0[p], max_evals), x0[p])


def test_device_form_mixed_outcomes_and_shrinks(ds):
    """Converged and 106 problems in one batch, shrinks included, a larger initial simplex."""
    nprob, n = 32, 5
    c, x0 = UM.crosen_problems(nprob, n, seed=7, spread=5.0)
    xg, simg, res = _device_solve(ds, c, x0, init_size=4.0)
    rs = [_crosen_restated(c[p], x0[p], init_size=4.0) for p in range(nprob)]
    assert sum(r["shrinks"] for r in rs) > 0
    assert {r["status"] for r in rs} == {0, 106}
    for p in range(nprob):
        _check_device(xg, simg, res, p, rs[p], x0[p])
    # shrinks in two dimensions as well
    c2, x2 = UM.crosen_problems(32, 2, seed=7, spread=2.0)
    xg, simg, res = _device_solve(ds, c2, x2, init_size=4.0)
    rs = [_crosen_restated(c2[p], x2[p], init_size=4.0) for p in range(32)]
    assert sum(r["shrinks"] > 0 for r in rs) > 0
    for p in range(32):
        _check_device(xg, simg, res, p, rs[p], x2[p])


def test_device_form_user_simplex(ds):
    nprob, n = 9, 3
    c, x0 = UM.crosen_problems(nprob, n, seed=5)
    rng = np.random.default_rng(3)
    sim = rng.uniform(-1.0, 1.0, (nprob, n + 1, n))
    xg, simg, res = _device_solve(ds, c, x0, simplex=sim)
    for p in range(nprob):
        _check_device(xg, simg, res, p, _crosen_restated(c[p], x0[p], simplex=sim[p].tolist()), x0[p])


def test_device_form_batch_invariance(ds):
    """One problem gives the same bits alone, at different positions of batches of different sizes, and in a batch of
    70,000 problems (more than the 65535 of a grid dimension)."""
    n = 2
    c, x0 = UM.crosen_problems(70000, n, seed=21)
    cp, xp = c[:1].copy(), x0[:1].copy()
    alone = _device_solve(ds, cp, xp)
    ref = _crosen_restated(cp[0], xp[0])
    _check_device(alone[0], alone[1], alone[2], 0, ref, xp[0])
    for size, pos in ((3, 2), (50, 17)):
        cc, xx = c[1:size + 1].copy(), x0[1:size + 1].copy()
        cc[pos], xx[pos] = cp[0], xp[0]
        xg, simg, res = _device_solve(ds, cc, xx)
        assert np.array_equal(xg[pos], alone[0][0]) and np.array_equal(simg[pos], alone[1][0])
        assert res[0][pos] == alone[2][0][0] and res[1][pos] == alone[2][1][0] and res[2][pos] == alone[2][2][0]
    c[69999], x0[69999] = cp[0], xp[0]
    xg, simg, res = _device_solve(ds, c, x0)
    assert np.array_equal(xg[69999], alone[0][0]) and res[1][69999] == alone[2][1][0]
    for p in sorted(set(np.linspace(0, 69998, 63).astype(int).tolist()) | {65535, 65536}):
        _check_device(xg, simg, res, p, _crosen_restated(c[p], x0[p]), x0[p])


def test_model_form_matches_device_form(ds):
    from nonlin_amd import _lib
    nprob, n = 40, 4
    c, x0 = UM.crosen_problems(nprob, n, seed=9)
    xg, _, (fo_d, ib_d, st_d) = _device_solve(ds, c, x0, max_evals=400)
    batch = UM.BtriBatch(c)
    md = C.c_void_p()
    try:
        assert ds.lib.nlh_device_fcn_model_create(nprob, 1, n, ds._devfcn(batch.crosen_launch), ds._devfcn(None), batch.ctx,
                                                  C.byref(md)) == 0
        x = np.ascontiguousarray(x0.copy())
        fout = np.zeros(nprob)
        ib = (_lib.IterationBehavior * nprob)()
        st = (C.c_int32 * nprob)()
        o = ds.options(max_evals=400)
        rc = ds.lib.nlh_dq_model_nelder_mead_solve(ds.h.ptr, C.byref(o), 1.0, md, x.ctypes.data_as(_lib.c_double_p),
                                                   fout.ctypes.data_as(_lib.c_double_p), ib, st)
        assert rc == 0
        assert np.array_equal(x, xg) and fout.tolist() == fo_d
        assert [ib[k].as_dict() for k in range(nprob)] == ib_d and list(st) == st_d
    finally:
        ds.lib.nlh_dq_model_destroy(md)
        batch.close()
    # a dense-quadratic model has no Nelder-Mead form
    m = ds.model(np.ones((2, 3, 4)), np.ones((2, 4)), 0.5)
    x = np.zeros((2, 3))
    rc = ds.lib.nlh_dq_model_nelder_mead_solve(ds.h.ptr, C.byref(ds.options()), 1.0, m._md, x.ctypes.data_as(_lib.c_double_p),
                                               None, None, None)
    assert rc == 104


def test_error_paths(ds):
    import torch
    from nonlin_amd import _lib
    null = C.cast(None, _lib.DEVFCN)
    x = torch.zeros((2, 3), dtype=torch.float64, device="cuda")
    ib = (_lib.IterationBehavior * 2)()
    ib[0].iter_count = 7
    ib[1].fcn_count = 5
    o = ds.options()
    assert ds.lib.nlh_nelder_mead_solve_batch_device(ds.h.ptr, C.byref(o), 1.0, 2, 3, null, None, x.data_ptr(), None, 0,
                                                     None, ib, None) == 211
    assert ib[0].iter_count == 0 and ib[1].fcn_count == 0
    c, x0 = UM.crosen_problems(2, 3)
    batch = UM.BtriBatch(c)
    try:
        f = ds._devfcn(batch.crosen_launch)
        assert ds.lib.nlh_nelder_mead_solve_batch_device(ds.h.ptr, C.byref(o), 1.0, 2, 0, f, batch.ctx, x.data_ptr(), None, 0,
                                                         None, None, None) == 201
        assert ds.lib.nlh_nelder_mead_solve_batch_device(ds.h.ptr, C.byref(o), 1.0, 2, 3, f, batch.ctx, x.data_ptr(), None, 1,
                                                         None, None, None) == 201     # use_simplex without a simplex
        # the btri residual launcher refuses m = 1 (it wants m == n): the library reports the user's failure
        with pytest.raises(RuntimeError):
            ds.nelder_mead_solve_batch_device(batch.launch, batch.ctx, torch.tensor(x0, dtype=torch.float64, device="cuda"))
    finally:
        batch.close()
    h = ds.h
    cib = _lib.IterationBehavior()
    cib.iter_count = 3
    xx = np.zeros(2)
    assert h.lib.nlh_nelder_mead_solve(h.ptr, C.byref(o), 1.0, 2, C.cast(None, _lib.FCNNVAR), None,
                                       xx.ctypes.data_as(_lib.c_double_p), None, 0, None, C.byref(cib)) == 211
    assert cib.iter_count == 0
    cf = _lib.FCNNVAR(lambda ctx, n, p: 0.0)
    assert h.lib.nlh_nelder_mead_solve(h.ptr, C.byref(o), 1.0, 0, cf, None, xx.ctypes.data_as(_lib.c_double_p), None, 0,
                                       None, None) == 201


# ------------------------------------------------------------------------------------------------ Fortran
def _unhex(h):
    return struct.unpack(">d", bytes.fromhex(h))[0]


@pytest.fixture(scope="module")
def fortran_exe(tmp_path_factory):
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    shim = os.path.join(ROOT, "nonlin_amd", "fortran", "build")
    if not os.path.exists(os.path.join(shim, "libnonlin_shim.a")):
        if fc is None:
            pytest.skip("no Fortran compiler and no Fortran shim")
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "nonlin_amd", "fortran"), "-s"])
    if fc is None:
        pytest.skip("no Fortran compiler")
    UM.lib()                                                   # builds tests/device_model/libuser_models.so if needed
    d = tmp_path_factory.mktemp("fortran_nm")
    exe = str(d / "nm_suite")
    libdir, umdir = os.path.join(ROOT, "nonlin_amd"), os.path.join(HERE, "device_model")
    subprocess.check_call([fc, "-O2", "-I" + shim, "-module-dir", str(d), os.path.join(HERE, "fortran_nm", "nm_suite.f90"),
                           "-o", exe, os.path.join(shim, "libnonlin_shim.a"), "-L" + libdir, "-lnonlin_hip", "-L" + umdir,
                           "-luser_models", "-Wl,-rpath," + libdir, "-Wl,-rpath," + umdir, "-Wl,-rpath,/opt/rocm/lib"])
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
    assert "# Minimum: (1.00000, 1.00000)" in out.stdout         # README Example 4

    def cmp(row, x, fo, ib, st):
        assert int(row[0]) == st
        assert [int(v) for v in row[1:5]] == [ib["iter_count"], ib["fcn_count"], ib["jacobian_count"], ib["gradient_count"]]
        assert row[5:8] == ["T" if ib["converge_on_fcn"] else "F", "F", "F"]
        assert _unhex(row[8]) == fo
        assert [_unhex(h) for h in row[9:]] == list(x)

    for key, f, x0, args in (("ex4", R.rosenbrock, [0.25, 0.75], None), ("nm1", R.rosenbrock, [0.0, 0.0], None),
                             ("nm2", R.beale, [1.0, 1.0], None), ("nm3", _rosen2, [0.0, 0.0], 100.0)):
        x, fo, ib, st, sim, s = _host_solve(f, x0, args=args)
        r = R.nm_solve(f, x0, args=args)
        _same_as_restatement(x, fo, ib, st, sim, r, x0)
        cmp(res[key][0], x, fo, ib, st)
        if key == "nm1":
            assert [_unhex(h) for h in res["nm1_simplex"][0]] == sim.ravel(order="F").tolist()
            x2, fo2, ib2, st2, _, _ = _host_solve(R.beale, [7.0, -3.0], solver=s)
            cmp(res["nm1_again"][0], x2, fo2, ib2, st2)
    # solve_batch on the device model of crosen: c(k) = 1 + k/8, x0(i,k) = -1/2 + (i+k)/16 (1-based i, k)
    nprob, n = 5, 3
    c = np.array([1.0 + 0.125 * k for k in range(1, nprob + 1)])
    x0 = np.array([[-0.5 + 0.0625 * (i + k) for i in range(1, n + 1)] for k in range(1, nprob + 1)])
    assert len(res["nm_batch"]) == nprob
    for p in range(nprob):
        r = _crosen_restated(c[p], x0[p])
        ib = {"iter_count": r["iter_count"], "fcn_count": r["fcn_count"], "jacobian_count": 0, "gradient_count": 0,
              "converge_on_fcn": r["converge_on_fcn"]}
        cmp(res["nm_batch"][p], r["x"] if r["status"] == 0 else x0[p], r["fout"], ib, r["status"])


def test_fortran_error_stop_on_max_evals(fortran_exe):
    out = subprocess.run(["timeout", "-k", "10", "120", fortran_exe, "errstop"], capture_output=True, text=True)
    assert out.returncode == 106, (out.returncode, out.stderr)
    assert "not reached" not in out.stdout
