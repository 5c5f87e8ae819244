"""GPU tests of polynomial%roots (src/nonlin_polynomials.f90:357-381) and the batched Horner evaluation: every form of the
root kernels (lane per polynomial, wave per polynomial on an LDS window, wave per polynomial on a global-memory window)
bit for bit against the plain-Python restatement (tests/polyroots_restatement.py): roots, their order, info.  The
restatement itself is held to LAPACK and to mpmath in tests/test_polyroots_cpu.py; here the yardsticks are the
restatement and numpy only."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import polyroots_cases as cases
import polyroots_restatement as rs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FORMS = [None, "wave", "global"]           # None: the form the order selects (lane up to 8, wave up to 128, then global)
LANE_MAX, WAVE_MAX, CAP = 8, 128, 256      # include/nonlin_hip.h


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


class _form:
    """NLH_POLYROOTS_FORM for the calls inside (the library reads it at every call)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = os.environ.pop("NLH_POLYROOTS_FORM", None)
        if self.form is not None:
            os.environ["NLH_POLYROOTS_FORM"] = self.form

    def __exit__(self, *a):
        os.environ.pop("NLH_POLYROOTS_FORM", None)
        if self.old is not None:
            os.environ["NLH_POLYROOTS_FORM"] = self.old


def gpu_roots(ds, coefs, form=None):
    """coefs: [nprob, order + 1] array.  Returns (z float64 [nprob, order, 2], info int32 [nprob])."""
    c = torch.from_numpy(np.ascontiguousarray(coefs, dtype=np.float64)).to(ds.device)
    with _form(form):
        z, info = ds.poly_roots_batch(c)
    torch.cuda.synchronize()
    return torch.view_as_real(z).cpu().numpy(), info.cpu().numpy()


_memo = {}


def restated(c):
    """(z float64 [order, 2], info) of the restatement, memoised on the coefficient bits."""
    key = np.asarray(c, dtype=np.float64).tobytes()
    if key not in _memo:
        z, info = rs.poly_roots([float(v) for v in c])
        _memo[key] = (np.array(z, dtype=np.float64).reshape(len(c) - 1, 2), info)
    return _memo[key]


def check_batch(ds, coefs, form):
    coefs = np.asarray(coefs, dtype=np.float64)
    z, info = gpu_roots(ds, coefs, form)
    for p in range(coefs.shape[0]):
        zr, ir = restated(coefs[p])
        assert info[p] == ir, (form, p, coefs[p], info[p], ir)
        assert np.array_equal(_bits(z[p]), _bits(zr)), (form, p, coefs[p], z[p], zr)
    return z, info


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_families_bitwise_every_form(ds, name, form):
    results = {}
    for order, cs in cases.by_order(cases.FAMILIES[name]()).items():
        z, info = check_batch(ds, np.stack(cs), form)
        assert (info == 0).all()
        results[order] = z
    if form is not None:                                           # and the forms with each other, on the same inputs
        for order, cs in cases.by_order(cases.FAMILIES[name]()).items():
            z0, _ = gpu_roots(ds, np.stack(cs), None)
            assert np.array_equal(_bits(z0), _bits(results[order]))


@pytest.mark.parametrize("form", FORMS)
def test_failure_rows_and_mixed_batches(ds, form):
    """Family f: info 210 / 201 and NaN roots; a failing row changes no other row's bits."""
    rng = np.random.default_rng(5)
    for order in (3, 5):
        bad = [(c, want) for c, want in cases.family_f() if len(c) - 1 == order]
        good = rng.standard_normal((70, order + 1))
        z_good, info_good = check_batch(ds, good, form)
        assert (info_good == 0).all()
        mixed = good.copy()
        where = [0, 17, 63, 64, 69][:len(bad)]
        rows = list(mixed)
        for k, (c, _) in zip(where, bad):
            rows[k] = c
        z, info = check_batch(ds, np.stack(rows), form)
        for k, (c, want) in zip(where, bad):
            assert info[k] == want and np.isnan(z[k]).all()
        keep = [k for k in range(70) if k not in where]
        assert np.array_equal(_bits(z[keep]), _bits(z_good[keep])) and (info[keep] == 0).all()
    z, info = check_batch(ds, np.array([[1e300, 1.0, 1e-300]]), form)   # finite coefficients, infinite companion entry
    assert info[0] == 201 and np.isnan(z).all()


@pytest.mark.parametrize("order", [LANE_MAX, LANE_MAX + 1, WAVE_MAX, WAVE_MAX + 1, CAP])
def test_size_edges_of_the_forms(ds, order):
    """The largest order of each form and the first of the next, in the form the order selects."""
    rng = np.random.default_rng(order)
    coefs = rng.standard_normal((3 if order <= WAVE_MAX + 1 else 2, order + 1))
    _, info = check_batch(ds, coefs, None)
    assert (info == 0).all()


def test_cap_plus_one_launches_nothing(ds):
    from nonlin_amd.api import NL_ARRAY_SIZE_ERROR, NL_INVALID_INPUT_ERROR
    order = CAP + 1
    c = torch.ones((2, order + 1), dtype=torch.float64, device=ds.device)
    z = torch.full((2, order, 2), 7.0, dtype=torch.float64, device=ds.device)
    info = torch.full((2,), 7, dtype=torch.int32, device=ds.device)
    for form in FORMS:
        with _form(form):
            assert ds.lib.nlh_poly_roots_batch(ds.h.ptr, 2, order, c.data_ptr(), z.data_ptr(), info.data_ptr()) == NL_ARRAY_SIZE_ERROR
    torch.cuda.synchronize()
    assert (z == 7.0).all() and (info == 7).all()
    assert ds.lib.nlh_poly_roots_batch(ds.h.ptr, 2, -1, c.data_ptr(), z.data_ptr(), info.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_poly_roots_batch(ds.h.ptr, 2, 0, c.data_ptr(), z.data_ptr(), info.data_ptr()) == 0      # :373
    assert ds.lib.nlh_poly_roots_batch(ds.h.ptr, 0, 3, c.data_ptr(), z.data_ptr(), info.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (z == 7.0).all() and (info == 7).all()
    with pytest.raises(RuntimeError):
        ds.poly_roots_batch(c)


@pytest.mark.parametrize("nprob", [1, 63, 64, 65])
@pytest.mark.parametrize("form", FORMS)
def test_batch_sizes_around_a_wave(ds, nprob, form):
    coefs = np.random.default_rng(nprob).standard_normal((nprob, 4))
    _, info = check_batch(ds, coefs, form)
    assert (info == 0).all()


def test_a_million_cubics(ds):
    """2^20 cubics in one call: a strided sample of 4096 bitwise against the restatement, every info 0, and the whole batch
    bitwise equal to the same rows solved in chunks of 65,536 (a row's result does not depend on its place)."""
    nprob = 1 << 20
    coefs = np.random.default_rng(20).standard_normal((nprob, 4))
    c = torch.from_numpy(coefs).to(ds.device)
    z, info = ds.poly_roots_batch(c)
    torch.cuda.synchronize()
    assert int((info != 0).sum()) == 0
    zh = torch.view_as_real(z).cpu().numpy()
    for p in range(0, nprob, nprob // 4096):
        zr, ir = restated(coefs[p])
        assert ir == 0 and np.array_equal(_bits(zh[p]), _bits(zr)), p
    for p0 in range(0, nprob, 65536):
        zc, ic = ds.poly_roots_batch(c[p0:p0 + 65536].contiguous())
        assert torch.equal(torch.view_as_real(zc).view(torch.int64), torch.view_as_real(z[p0:p0 + 65536]).view(torch.int64))
        assert int((ic != 0).sum()) == 0


def test_timing_group(ds):
    """The root kernels have a timing id of their own (NLH_K_POLYROOTS): one bracket per nlh_poly_roots_batch call."""
    c = torch.from_numpy(np.random.default_rng(3).standard_normal((100, 6))).to(ds.device)
    assert ds.lib.nlh_kernel_name(14) == b"k_polyroots"
    ds.h.timing_enable(kernels=["polyroots"])
    ds.h.timing_reset()
    try:
        ds.poly_roots_batch(c)
        ds.poly_roots_batch(c)
        ms, launches = ds.h.timing("polyroots")
    finally:
        ds.h.timing_enable(False)
    assert launches == 2 and ms > 0.0


def test_eval_batch_bitwise(ds):
    import nonlin_amd as nl
    rng = np.random.default_rng(31)
    for order, npts in ((0, 5), (1, 7), (3, 300), (8, 65), (16, 1)):
        nprob = 9
        coefs = rng.standard_normal((nprob, order + 1))
        x = rng.standard_normal((nprob, npts))
        xc = rng.standard_normal((nprob, npts)) + 1j * rng.standard_normal((nprob, npts))
        cd = torch.from_numpy(coefs).to(ds.device)
        y = ds.poly_eval_batch(cd, torch.from_numpy(x).to(ds.device)).cpu().numpy()
        yc = ds.poly_eval_batch(cd, torch.from_numpy(xc).to(ds.device)).cpu().numpy()
        assert y.dtype == np.float64 and yc.dtype == np.complex128
        for p in range(nprob):
            cl = [float(v) for v in coefs[p]]
            want = [rs.poly_eval(cl, float(v)) for v in x[p]]
            assert np.array_equal(_bits(y[p]), _bits(want))
            pol = nl.polynomial()
            pol.initialize(coefs[p])
            assert np.array_equal(_bits(y[p]), _bits(pol.evaluate(x[p])))          # today's polynomial.evaluate
            wc = [rs.poly_eval_complex(cl, v.real, v.imag) for v in xc[p]]
            assert np.array_equal(_bits(yc[p].real), _bits([w[0] for w in wc]))
            assert np.array_equal(_bits(yc[p].imag), _bits([w[1] for w in wc]))
            hc = pol.evaluate(xc[p])                                               # the host API's complex evaluate
            assert np.array_equal(_bits(hc.real), _bits(yc[p].real)) and np.array_equal(_bits(hc.imag), _bits(yc[p].imag))


def test_fit_then_roots_on_the_device(ds):
    """poly_fit_batch's output goes straight into poly_roots_batch (no host copy); the same through the host API."""
    import nonlin_amd as nl
    rng = np.random.default_rng(41)
    nprob, npts, order = 6, 40, 5
    xs = np.sort(rng.uniform(-1.0, 1.0, size=(nprob, npts)), axis=1)
    ys = np.cos(3.0 * xs) + 0.01 * rng.standard_normal((nprob, npts))
    coef = ds.poly_fit_batch(torch.from_numpy(xs).to(ds.device), torch.from_numpy(ys).to(ds.device), order)
    z, info = ds.poly_roots_batch(coef)
    assert z.dtype == torch.complex128 and tuple(z.shape) == (nprob, order) and int((info != 0).sum()) == 0
    z = z.cpu().numpy()
    for p in range(nprob):
        pol = nl.polynomial()
        pol.fit(xs[p], ys[p].copy(), order)
        assert np.array_equal(_bits(pol.get_all()), _bits(coef[p].cpu().numpy()))
        zh = pol.roots()
        assert np.array_equal(_bits(zh.real), _bits(z[p].real)) and np.array_equal(_bits(zh.imag), _bits(z[p].imag))
        zr, _ = restated(pol.get_all())
        assert np.array_equal(_bits(zh.real), _bits(zr[:, 0])) and np.array_equal(_bits(zh.imag), _bits(zr[:, 1]))


def test_public_api(ds):
    import nonlin_amd as nl
    p = nl.polynomial()
    p.initialize([6.0, 1.0, -4.0, 1.0])                            # tests/nonlin_test_poly.f90:53-84
    z = p.roots()
    assert z.dtype == np.complex128 and z.shape == (3,)
    assert np.abs(p.evaluate(z)).max() <= 1e-6
    assert sorted(np.round(z.real, 9)) == [-1.0, 2.0, 3.0] and (z.imag == 0.0).all()
    f = nl.polynomial().assign([-1.0, -2.0, 0.0, 1.0])             # the roots example
    z = f.roots()
    assert sorted(f"{v:9.6f}" for v in z.real) == sorted(["-1.000000", " 1.618034", "-0.618034"]) and (z.imag == 0.0).all()
    zr, _ = restated(np.array([-1.0, -2.0, 0.0, 1.0]))
    assert np.array_equal(_bits(z.real), _bits(zr[:, 0]))
    assert nl.polynomial(0).roots().shape == (0,) and nl.polynomial().roots().shape == (0,)
    z = nl.polynomial().assign([5.0, 2.0, 1.0]).roots()            # -1 +- 2i: the +im root first
    assert z[0].imag > 0 and z[1] == np.conj(z[0]) and abs(z[0] - (-1 + 2j)) < 1e-14
    z = nl.polynomial().assign([0.0, -6.0, 1.0, 4.0, 1.0]).roots()
    assert z[-1] == 0 and np.count_nonzero(z == 0) == 1
    for c, want in cases.family_f():
        with pytest.raises(nl.NonlinError) as e:
            nl.polynomial().assign(c).roots()
        assert e.value.code == want
    with pytest.raises(nl.NonlinError) as e:
        nl.polynomial(CAP + 1).assign(1.0).roots()
    assert e.value.code == nl.NL_ARRAY_SIZE_ERROR
    # operators and divide through the public type
    q, r = nl.polynomial().assign([0.0, 1.0, 0.0, 1.0]).divide(nl.polynomial().assign([1.0, 1.0]))
    assert list(q.get_all()) == [2.0, -1.0, 1.0] and list(r.get_all()) == [-2.0]
    prod = nl.polynomial().assign([5.0, 0.0, 10.0, 6.0]) * nl.polynomial().assign([1.0, 2.0, 4.0])
    assert list(prod.get_all()) == [5.0, 10.0, 30.0, 26.0, 52.0, 24.0]
    # the roots of a product are the roots of its factors
    a, b = nl.polynomial().assign([-2.0, 1.0]), nl.polynomial().assign([5.0, 2.0, 1.0])
    z = (a * b).roots()
    assert min(abs(z - 2.0)) < 1e-13 and min(abs(z - (-1 + 2j))) < 1e-13 and min(abs(z - (-1 - 2j))) < 1e-13


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
    d = tmp_path_factory.mktemp("fortran_poly")
    exe = str(d / "poly_suite")
    libdir = os.path.join(ROOT, "nonlin_amd")
    subprocess.check_call([fc, "-O2", "-I" + shim, "-module-dir", str(d), os.path.join(HERE, "fortran_poly", "poly_suite.f90"),
                           "-o", exe, os.path.join(shim, "libnonlin_shim.a"), "-L" + libdir, "-lnonlin_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_fortran_poly_suite(fortran_exe):
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    res, example = {}, []
    for line in out.stdout.splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "#":
            example.append(line[len("# example"):])
            continue
        res[t[0]] = np.array([_unhex(v) for v in t[1:]])
    assert "done" in res and not any(k == "FAIL" for k in res)

    def flat(c):
        return restated(np.array(c))[0].ravel()

    c_test = [6.0, 1.0, -4.0, 1.0]
    assert np.array_equal(_bits(res["roots_test"]), _bits(flat(c_test)))
    vals = [rs.poly_eval_complex(c_test, re, im) for re, im in restated(np.array(c_test))[0]]
    assert np.array_equal(_bits(res["roots_test_values"]), _bits(np.array(vals).ravel()))
    assert np.array_equal(_bits(res["roots_example"]), _bits(flat([-1.0, -2.0, 0.0, 1.0])))
    assert sorted(s[:10] for s in example) == sorted([" -1.000000", "  1.618034", " -0.618034"])
    assert np.array_equal(_bits(res["roots_zero"]), _bits(flat([0.0, -6.0, 1.0, 4.0, 1.0]))) and res["roots_zero"][-2] == 0.0
    assert np.array_equal(_bits(res["roots_pair"]), _bits(flat([5.0, 2.0, 1.0]))) and res["roots_pair"][1] > 0.0
    assert np.array_equal(res["companion"].reshape(3, 3).T, cases.companion(np.array(c_test)))   # printed column-major
    c1 = [1.0 / i + 0.125 * ((i * 7) % 5) for i in range(1, 12)]
    c2 = [0.3 * i - 1.0 / (i + 2) for i in range(1, 22)]
    assert np.array_equal(_bits(res["add_10_20"]), _bits(rs.poly_add_sub(c1, c2, False)))
    assert np.array_equal(_bits(res["sub_10_20"]), _bits(rs.poly_add_sub(c1, c2, True)))
    # reference behaviour kept (src/nonlin_polynomials.f90:538, :593): the leading coefficient stays 0
    assert np.array_equal(_bits(res["add_20_10"]), _bits(rs.poly_add_sub(c2, c1, False))) and res["add_20_10"][-1] == 0.0
    assert np.array_equal(_bits(res["sub_20_10"]), _bits(rs.poly_add_sub(c2, c1, True))) and res["sub_20_10"][-1] == 0.0
    assert np.array_equal(_bits(res["sub_blank_10"]), _bits(c1))                    # :576-580: +y
    p1 = [5.0, 0.0, 10.0, 6.0]
    assert np.array_equal(_bits(res["mult"]), _bits(rs.poly_mult(p1, [1.0, 2.0, 4.0])))
    assert np.array_equal(_bits(res["mult_right"]), _bits(rs.poly_scale(p1, 2.5)))
    assert np.array_equal(_bits(res["mult_left"]), _bits(rs.poly_scale(p1, 2.5)))
    q, r = rs.poly_divide([0.0, 1.0, 0.0, 1.0], [1.0, 1.0])
    assert np.array_equal(_bits(res["div_q"]), _bits(q)) and np.array_equal(_bits(res["div_r"]), _bits(r))
    assert math.isclose(res["div_r"][0], -2.0, abs_tol=1e-8)
