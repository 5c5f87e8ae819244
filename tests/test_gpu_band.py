"""GPU tests of the bands (include/nonlin_hip.h: nlh_propagate*, nlh_curve_band_batch, nlh_expr_band_batch,
nlh_dq_model_propagate): the kernel bit for bit against tests/band_restatement.py in both workgroup forms, at the edges of
the sixteen-column blocks and of the LDS cap, for every batch shape; the chain against the restatement on the restated
Jacobians of the exp-free models; the band after real fits -- plain, mapped, separable, grouped, one of them failed; the model
object; the error returns.  Everything is bit for bit: no tolerance in this file."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import band_restatement as BR
import curve_cases as CC
import curve_restatement as R
import expr_restatement as ER
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

dp = C.POINTER(C.c_double)
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NLH_ERR_BAD_HANDLE = 201, 211, -3
LDS_CAP = 160 * 1024 - 2048
MS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 301]
# 16 | 17 and 32 | 33: the edges of the sixteen-column blocks (one block, two, two and a first column of a third);
# 200 | 201: the last n whose packed triangle fits LDS and the first that is read from global memory
NS = [1, 2, 3, 9, 15, 16, 17, 24, 32, 33, 200, 201]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _dev(ds, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ds.device)


class _env:
    """An environment variable for the calls inside (the library reads these at every call)."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.pop(self.name, None)
        if self.value is not None:
            os.environ[self.name] = str(self.value)

    def __exit__(self, *a):
        os.environ.pop(self.name, None)
        if self.old is not None:
            os.environ[self.name] = self.old


def _flat_points(m, n):
    """Points of a flat workgroup: as many as 256 threads and the LDS cap hold; 0: flat cannot hold the size."""
    if m > 256 or 4 * n * (n + 1) > LDS_CAP:
        return 0
    return min(256 // m, LDS_CAP // (4 * n * (n + 1)))


def _spd(rng, npoints, n):
    a = rng.standard_normal((npoints, n, n + 2))
    return a @ np.transpose(a, (0, 2, 1)) / (n + 2)


def _poisoned(cov):
    n = cov.shape[-1]
    bad = cov.copy()
    iu = np.triu_indices(n, 1)
    bad[:, iu[0], iu[1]] = np.nan
    return bad


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("n", NS)
def test_kernel_bitwise_every_m_form_and_batch(ds, n):
    """Every m of MS, every form that can hold it (None: the one the library picks), batches of 1, 3 and more than two
    workgroups of either form, with and without noise, with the strict upper triangle poisoned.  The reference is computed
    once per m on the largest batch: a point's bits do not depend on its batch, so its prefixes are the smaller ones'."""
    rng = np.random.default_rng(1000 + n)
    for m in MS:
        big = 2 * max(_flat_points(m, n), 1) + 1
        J = rng.standard_normal((big, n, m))
        cov = _spd(rng, big, n)
        noise = rng.uniform(0.0, 1.0, big)
        v = BR.variance(J, cov)
        want = {False: BR.finish(v), True: BR.finish(v, noise)}
        dJ, dcov, dbad, dnoise = _dev(ds, J), _dev(ds, cov), _dev(ds, _poisoned(cov)), _dev(ds, noise)
        for form in (None, "row", "flat"):
            with _env("NLH_BAND_FORM", form):
                for b in (1, 3, big):
                    for nz in (False, True):
                        got = ds.propagate(dJ[:b], dcov[:b], dnoise[:b] if nz else None).cpu().numpy()
                        assert np.array_equal(_bits(got), _bits(want[nz][:b])), (m, form, b, nz)
                got = ds.propagate(dJ, dbad, dnoise).cpu().numpy()
                assert np.array_equal(_bits(got), _bits(want[True])), (m, form, "upper triangle poisoned")


@pytest.mark.parametrize("form", [None, "row", "flat"])
@pytest.mark.parametrize("m,n", [(1, 3), (64, 9), (129, 17), (301, 24), (65, 201)])
def test_negative_definite_and_nan_matrices(ds, m, n, form):
    """A negative-definite matrix gives exact (+0.0) zeros; a NaN matrix in the middle of a batch gives NaN rows and leaves
    its neighbours' bits alone."""
    rng = np.random.default_rng(7 * m + n)
    npoints = 2 * max(_flat_points(m, n), 1) + 3
    J = rng.standard_normal((npoints, n, m))
    cov = _spd(rng, npoints, n)
    want = BR.propagate(J, cov)
    mid = npoints // 2
    cov[1] = -cov[1]
    cov[mid] = np.nan
    with _env("NLH_BAND_FORM", form):
        got = ds.propagate(_dev(ds, J), _dev(ds, cov)).cpu().numpy()
    assert np.array_equal(_bits(got[1]), _bits(np.zeros(m)))
    assert np.isnan(got[mid]).all()
    keep = [p for p in range(npoints) if p not in (1, mid)]
    assert np.array_equal(_bits(got[keep]), _bits(want[keep]))
    assert np.array_equal(_bits(got), _bits(BR.propagate(J, cov)))


# ------------------------------------------------------------------------------------------------ 2. the chain
def _lorentz_grid(ds, K, B, nprob, npts, shared, seed=3):
    """Parameters near the generator's and a grid other than the data's: (x [nprob, n], tt [nprob, npts], device t)."""
    _, _, xt, _ = CC.curve_problems("lorentz", K, B, 64, nprob=nprob, seed=seed)
    rng = np.random.default_rng(seed)
    tt = np.tile(np.linspace(-0.1, 1.1, npts), (nprob, 1)) if shared else np.sort(rng.uniform(-0.1, 1.1, (nprob, npts)))
    return xt, tt, _dev(ds, tt[0] if shared else tt)


def _curve_want(K, B, x, tt, cov, noise=None):
    J = np.stack([R.jacobian(R.LORENTZ, K, B, x[p], tt[p]).T for p in range(len(x))])
    y = np.stack([R.model(R.LORENTZ, K, B, x[p], tt[p]) for p in range(len(x))])
    return y, BR.propagate(J, cov, noise)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("K,B,npts", [(1, -1, 50), (2, 1, 131), (3, 0, 300)])
def test_curve_band_equals_the_restatement(ds, K, B, npts, shared):
    nprob = 7
    x, tt, dt = _lorentz_grid(ds, K, B, nprob, npts, shared)
    n = x.shape[1]
    rng = np.random.default_rng(npts)
    cov, noise = _spd(rng, nprob, n) * 1e-4, rng.uniform(0.0, 1e-3, nprob)
    dx, dcov = _dev(ds, x), _dev(ds, cov)
    y0 = ds.curve_eval("lorentz", dx, dt, ncomp=K, baseline=B).cpu().numpy()
    for nz in (None, noise):
        wy, wsd = _curve_want(K, B, x, tt, cov, nz)
        y, sd = ds.curve_band("lorentz", dx, dcov, dt, ncomp=K, baseline=B, noise=None if nz is None else _dev(ds, nz))
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(y0)) and np.array_equal(_bits(y0), _bits(wy))
        assert np.array_equal(_bits(sd.cpu().numpy()), _bits(wsd))
    # dy may be NULL
    sd2 = torch.empty((nprob, npts), dtype=torch.float64, device=ds.device)
    assert ds.lib.nlh_curve_band_batch(ds.h.ptr, R.LORENTZ, K, B, nprob, npts, dt.data_ptr(), int(shared), dx.data_ptr(), dcov.data_ptr(),
                                       None, None, sd2.data_ptr()) == 0
    assert np.array_equal(_bits(sd2.cpu().numpy()), _bits(_curve_want(K, B, x, tt, cov)[1]))


@pytest.mark.parametrize("shared", [False, True])
def test_expr_band_equals_the_restatement(ds, shared):
    e = nl.Expr("vmax*s/(km+s)", "s", "vmax,km")
    prog = e.program()
    nprob, npts = 6, 77
    rng = np.random.default_rng(9)
    x = np.column_stack([rng.uniform(1.0, 3.0, nprob), rng.uniform(0.2, 2.0, nprob)])
    tt = np.tile(np.linspace(0.05, 10.0, npts), (nprob, 1)) if shared else np.sort(rng.uniform(0.05, 10.0, (nprob, npts)))
    cov, noise = _spd(rng, nprob, 2) * 1e-3, rng.uniform(0.0, 1e-2, nprob)
    J = np.stack([ER.jacobian(prog, x[p], [tt[p]]).T for p in range(nprob)])
    wy = np.stack([ER.value(prog, x[p], [tt[p]]) for p in range(nprob)])
    dt = _dev(ds, tt[0] if shared else tt)
    y0 = ds.expr_eval(e, _dev(ds, x), dt).cpu().numpy()
    for nz in (None, noise):
        y, sd = ds.expr_band(e, _dev(ds, x), _dev(ds, cov), dt, noise=None if nz is None else _dev(ds, nz))
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(y0)) and np.array_equal(_bits(y0), _bits(wy))
        assert np.array_equal(_bits(sd.cpu().numpy()), _bits(BR.propagate(J, cov, nz)))


def test_standard_error_of_a_derived_quantity(ds):
    """The lifetime 1/k of a decay as a one-row formula of the parameters: m = 1 < n = 3."""
    e = nl.Expr("1/k + 0*t", "t", "a,k,c")
    prog = e.program()
    nprob = 300                                                       # more than one flat workgroup of 256 one-row points
    rng = np.random.default_rng(10)
    x = np.column_stack([rng.uniform(1, 2, nprob), rng.uniform(0.5, 1.5, nprob), rng.uniform(0.1, 0.5, nprob)])
    cov = _spd(rng, nprob, 3) * 1e-4
    one = np.zeros((nprob, 1))
    tau, sd = ds.expr_band(e, _dev(ds, x), _dev(ds, cov), _dev(ds, one))
    J = np.stack([ER.jacobian(prog, x[p], [one[p]]).T for p in range(nprob)])
    assert np.array_equal(_bits(sd.cpu().numpy()), _bits(BR.propagate(J, cov)))
    assert np.array_equal(_bits(tau.cpu().numpy()[:, 0]), _bits(np.stack([ER.value(prog, x[p], [one[p]])[0] for p in range(nprob)])))
    # first order: sd(1/k) = sd(k) / k^2, to the rounding of either side
    assert np.allclose(sd.cpu().numpy()[:, 0], np.sqrt(cov[:, 1, 1]) / x[:, 1] ** 2, rtol=1e-12)


def test_forward_differences_equal_propagate_on_fd_jacobian(ds):
    K, B, nprob, npts = 2, 0, 5, 90
    x, tt, dt = _lorentz_grid(ds, K, B, nprob, npts, False)
    n = x.shape[1]
    cov = _spd(np.random.default_rng(2), nprob, n) * 1e-4
    zero = torch.zeros((nprob, npts), dtype=torch.float64, device=ds.device)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, dt, zero)
    dx, dcov = _dev(ds, x), _dev(ds, cov)
    val, sd = ds.propagate_batch_device(fcn, ctx, npts, dx, dcov)
    Jfd = ds.fd_jacobian_device(fcn, ctx, npts, dx)
    assert torch.equal(sd, ds.propagate(Jfd, dcov))
    assert np.array_equal(_bits(val.cpu().numpy()), _bits(ds.curve_eval("lorentz", dx, dt, ncomp=K, baseline=B).cpu().numpy()))
    # dval NULL with forward differences: F(x) goes to the chain's own scratch, the same bits
    sd2 = torch.empty_like(sd)
    assert ds.lib.nlh_propagate_batch_device(ds.h.ptr, nprob, npts, n, ds._devfcn(fcn), ds._devfcn(None), ds._ctxp(ctx), dx.data_ptr(),
                                             dcov.data_ptr(), None, None, sd2.data_ptr()) == 0
    assert torch.equal(sd2, sd)
    # and with the analytic Jacobian the chain is curve_band
    val3, sd3 = ds.propagate_batch_device(fcn, ctx, npts, dx, dcov, jac=jac)
    y4, sd4 = ds.curve_band("lorentz", dx, dcov, dt, ncomp=K, baseline=B)
    assert torch.equal(sd3, sd4) and torch.equal(val3, y4)


def test_slices_give_the_unsliced_bits(ds):
    K, B, nprob, npts = 2, 1, 7, 70
    x, tt, dt = _lorentz_grid(ds, K, B, nprob, npts, False)
    n = x.shape[1]
    rng = np.random.default_rng(4)
    cov, noise = _spd(rng, nprob, n) * 1e-4, rng.uniform(0.0, 1e-3, nprob)
    dx, dcov, dnoise = _dev(ds, x), _dev(ds, cov), _dev(ds, noise)
    zero = torch.zeros((nprob, npts), dtype=torch.float64, device=ds.device)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, dt, zero)
    whole = ds.curve_band("lorentz", dx, dcov, dt, ncomp=K, baseline=B, noise=dnoise)
    whole_fd = ds.propagate_batch_device(fcn, ctx, npts, dx, dcov, noise=dnoise)
    assert np.array_equal(_bits(whole[1].cpu().numpy()), _bits(_curve_want(K, B, x, tt, cov, noise)[1]))
    per = 8 * npts * n                                                # bytes of one problem's Jacobian
    for cap in (3 * per, 2 * per + 8, 1):                             # slices of 3 + 3 + 1, of 2 + 2 + 2 + 1, of one problem each
        with _env("NLH_BAND_SCRATCH", cap):
            got = ds.curve_band("lorentz", dx, dcov, dt, ncomp=K, baseline=B, noise=dnoise)
            got_fd = ds.propagate_batch_device(fcn, ctx, npts, dx, dcov, noise=dnoise)
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1]), cap
        assert torch.equal(got_fd[0], whole_fd[0]) and torch.equal(got_fd[1], whole_fd[1]), cap


# ------------------------------------------------------------------------------------------------ 3. after real fits
M_FIT, NPROB_FIT, NPTS_FIT = 64, 5, 97


def _fit_data(K, B, seed, nprob=NPROB_FIT, tweak=None):
    """Lorentzian data sets on 64 points whose truth may be adjusted (tweak) before the data are made."""
    t, _, xt, x0 = CC.curve_problems("lorentz", K, B, M_FIT, nprob=nprob, seed=seed)
    if tweak is not None:
        tweak(xt, x0)
    rng = np.random.default_rng(seed + 1)
    y = np.stack([R.model(R.LORENTZ, K, B, xt[p], t[p]) for p in range(nprob)]) + 1e-3 * rng.standard_normal((nprob, M_FIT))
    return t, y, xt, x0


def _grid(nprob):
    return np.tile(np.linspace(-0.05, 1.05, NPTS_FIT), (nprob, 1))


def _check_band_after_fit(ds, K, B, x, cov, chi2):
    """curve_band on a fit's x and cov (device) against the restatement on the same numbers: confidence and prediction."""
    nprob = x.shape[0]
    tt = _grid(nprob)
    xh, ch, qh = x.cpu().numpy(), cov.cpu().numpy(), chi2.cpu().numpy()
    for nz in (None, qh):
        y, sd = ds.curve_band("lorentz", x, cov, _dev(ds, tt), ncomp=K, baseline=B, noise=None if nz is None else chi2)
        wy, wsd = _curve_want(K, B, xh, tt, ch, nz)
        assert np.array_equal(_bits(y.cpu().numpy()), _bits(wy)) and np.array_equal(_bits(sd.cpu().numpy()), _bits(wsd))
    return sd.cpu().numpy()


def test_band_after_a_plain_fit_and_a_failed_problem(ds):
    """max_evals = 7 is enough for the generator's starts (5 evaluations each) and not for problem 2's, moved away from its
    truth (9): its cov is NaN, so are its rows of the band, and the other problems' bits are those of the batch without it."""
    K, B = 1, 0
    t, y, xt, x0 = _fit_data(K, B, 41)
    x0[2] = xt[2] * np.array([3.0, 1.0, 0.2, 1.0]) + np.array([0.0, 0.3, 0.0, 0.0])
    o = ds.options(max_evals=7)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch("lorentz", _dev(ds, t), _dev(ds, y), _dev(ds, x0), ncomp=K, baseline=B, opts=o)
    assert st[2] != 0 and [st[p] for p in (0, 1, 3, 4)] == [0] * 4
    assert torch.isnan(cov[2]).all()
    sd = _check_band_after_fit(ds, K, B, x, cov, chi2)
    assert np.isnan(sd[2]).all() and np.isfinite(sd[[0, 1, 3, 4]]).all() and (sd[[0, 1, 3, 4]] > 0).all()
    keep = torch.tensor([0, 1, 3, 4], device=ds.device)
    _, sdk = ds.curve_band("lorentz", x[keep].contiguous(), cov[keep].contiguous(), _dev(ds, _grid(4)), ncomp=K, baseline=B,
                           noise=chi2[keep].contiguous())
    assert np.array_equal(_bits(sdk.cpu().numpy()), _bits(sd[[0, 1, 3, 4]]))


def test_band_after_a_plain_two_peak_fit(ds):
    K, B = 2, -1
    t, y, xt, x0 = _fit_data(K, B, 42)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch("lorentz", _dev(ds, t), _dev(ds, y), _dev(ds, x0), ncomp=K, baseline=B,
                                                                  opts=ds.options(max_evals=CC.MAX_EVALS))
    assert st == [0] * NPROB_FIT
    sd = _check_band_after_fit(ds, K, B, x, cov, chi2)
    assert np.isfinite(sd).all() and (sd > 0).all()


def test_band_after_a_mapped_fit(ds):
    """Two Lorentzians, the second width tied to the first and the second position fixed: the full covariance has a zero row
    and column at the fixed parameter, and the band is finite."""
    K, B = 2, -1

    def tweak(xt, x0):
        xt[:, 5] = 1.25 * xt[:, 2]
        x0[:, 4] = xt[:, 4]
    t, y, xt, x0 = _fit_data(K, B, 43, tweak=tweak)
    pm = nl.ParamMap(6, fixed=(4,), tied={5: (2, 1.25, 0.0)})
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch("lorentz", _dev(ds, t), _dev(ds, y), _dev(ds, x0), ncomp=K, baseline=B,
                                                                  opts=ds.options(max_evals=CC.MAX_EVALS), pmap=pm)
    assert st == [0] * NPROB_FIT
    ch = cov.cpu().numpy()
    assert not ch[:, 4, :].any() and not ch[:, :, 4].any()
    sd = _check_band_after_fit(ds, K, B, x, cov, chi2)
    assert np.isfinite(sd).all() and (sd > 0).all()


def test_band_after_a_separable_fit(ds):
    K, B = 1, 0
    t, y, xt, x0 = _fit_data(K, B, 44)
    sp = nl.Separable.for_curve("lorentz", K, B)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch("lorentz", _dev(ds, t), _dev(ds, y), _dev(ds, x0), ncomp=K, baseline=B,
                                                                  opts=ds.options(max_evals=CC.MAX_EVALS), sep=sp)
    assert st == [0] * NPROB_FIT
    sd = _check_band_after_fit(ds, K, B, x, cov, chi2)
    assert np.isfinite(sd).all() and (sd > 0).all()


def test_band_after_a_group_fit_through_group_launchers(ds):
    """G = 3 data sets per group share the width: the band of a group is propagate_batch_device over group_launchers around
    the plotting grid's launchers (y = 0), with the per-group cov and the gathered x.  The restatement builds the group's
    Jacobian from the restated curve Jacobians: rows of data set s, column index(s, k), +0.0 elsewhere."""
    K, B, G, ngroup = 1, 0, 3, NPROB_FIT
    N, nprob = 4, G * NPROB_FIT

    def tweak(xt, x0):
        for g in range(ngroup):
            xt[g * G:(g + 1) * G, 2] = xt[g * G, 2]
    t, y, xt, x0 = _fit_data(K, B, 45, nprob=nprob, tweak=tweak)
    grp = nl.Group(N, shared=(2,), nsets=G)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch("lorentz", _dev(ds, t), _dev(ds, y), _dev(ds, x0), ncomp=K, baseline=B,
                                                                  opts=ds.options(max_evals=CC.MAX_EVALS), group=grp)
    assert st == [0] * ngroup and tuple(cov.shape) == (ngroup, grp.nouter, grp.nouter)
    tt = _grid(nprob)
    zero = torch.zeros((nprob, NPTS_FIT), dtype=torch.float64, device=ds.device)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, _dev(ds, tt), zero)
    gf, gj, gctx = ds.group_launchers(grp, fcn, jac, ctx)
    xg = ds.group_gather(grp, x)
    val, sd = ds.propagate_batch_device(gf, gctx, G * NPTS_FIT, xg, cov, jac=gj, noise=chi2)
    xh, ch, qh = x.cpu().numpy(), cov.cpu().numpy(), chi2.cpu().numpy()
    J = np.zeros((ngroup, grp.nouter, G * NPTS_FIT))
    wy = np.zeros((ngroup, G * NPTS_FIT))
    for g in range(ngroup):
        for s in range(G):
            p = g * G + s
            Jp = R.jacobian(R.LORENTZ, K, B, xh[p], tt[p])
            rows = slice(s * NPTS_FIT, (s + 1) * NPTS_FIT)
            for k in range(N):
                J[g, grp.index(s, k), rows] = Jp[:, k]
            wy[g, rows] = R.model(R.LORENTZ, K, B, xh[p], tt[p])
    assert np.array_equal(_bits(val.cpu().numpy()), _bits(wy))
    assert np.array_equal(_bits(sd.cpu().numpy()), _bits(BR.propagate(J, ch, qh)))
    assert np.isfinite(sd.cpu().numpy()).all()
    gctx.close()


# ------------------------------------------------------------------------------------------------ 4. the model object
def test_model_object(ds):
    K, B, nprob, npts = 2, 0, 6, 83
    x, tt, dt = _lorentz_grid(ds, K, B, nprob, npts, False)
    n = x.shape[1]
    rng = np.random.default_rng(6)
    cov, noise = _spd(rng, nprob, n) * 1e-4, rng.uniform(0.0, 1e-3, nprob)
    y, sd = ds.curve_band("lorentz", _dev(ds, x), _dev(ds, cov), dt, ncomp=K, baseline=B, noise=_dev(ds, noise))
    zero = np.zeros((nprob, npts))
    md = C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.LORENTZ, K, B, nprob, npts, tt.ctypes.data_as(dp), 0, zero.ctypes.data_as(dp), None, 1,
                                         C.byref(md)) == 0
    try:
        vh, sh = np.full((nprob, npts), 7.0), np.full((nprob, npts), 7.0)
        assert ds.lib.nlh_dq_model_propagate(ds.h.ptr, md, x.ctypes.data_as(dp), cov.ctypes.data_as(dp), noise.ctypes.data_as(dp),
                                             vh.ctypes.data_as(dp), sh.ctypes.data_as(dp)) == 0
        assert np.array_equal(_bits(vh), _bits(y.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sd.cpu().numpy()))
        # noise and val NULL
        sh2 = np.full((nprob, npts), 7.0)
        assert ds.lib.nlh_dq_model_propagate(ds.h.ptr, md, x.ctypes.data_as(dp), cov.ctypes.data_as(dp), None, None, sh2.ctypes.data_as(dp)) == 0
        _, sd0 = ds.curve_band("lorentz", _dev(ds, x), _dev(ds, cov), dt, ncomp=K, baseline=B)
        assert np.array_equal(_bits(sh2), _bits(sd0.cpu().numpy()))
        assert ds.lib.nlh_dq_model_propagate(ds.h.ptr, md, None, cov.ctypes.data_as(dp), None, None, sh2.ctypes.data_as(dp)) == NL_INVALID_INPUT_ERROR
        assert ds.lib.nlh_dq_model_propagate(None, md, x.ctypes.data_as(dp), cov.ctypes.data_as(dp), None, None, sh2.ctypes.data_as(dp)) == NLH_ERR_BAD_HANDLE
    finally:
        ds.lib.nlh_dq_model_destroy(md)
    # a dense-quadratic model has no launchers to propagate through
    inner = C.c_void_p()
    A, b = np.ones((1, 2, 2)), np.ones((1, 2))
    assert ds.lib.nlh_dq_model_create(ds.h.ptr, 1, 2, 2, A.ctypes.data_as(dp), b.ctypes.data_as(dp), 0.5, C.byref(inner)) == 0
    one, out = np.ones(8), np.full(2, 7.0)
    assert ds.lib.nlh_dq_model_propagate(ds.h.ptr, inner, one.ctypes.data_as(dp), one.ctypes.data_as(dp), None, None,
                                         out.ctypes.data_as(dp)) == NL_INVALID_INPUT_ERROR
    assert (out == 7.0).all()
    ds.lib.nlh_dq_model_destroy(inner)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_error_returns_before_any_launch(ds):
    K, B, nprob, npts = 1, 0, 2, 8
    x, tt, dt = _lorentz_grid(ds, K, B, nprob, npts, False)
    n = x.shape[1]
    dx, dcov = _dev(ds, x), _dev(ds, _spd(np.random.default_rng(1), nprob, n))
    dJ = torch.ones((nprob, n, npts), dtype=torch.float64, device=ds.device)
    y = torch.full((nprob, npts), 7.0, dtype=torch.float64, device=ds.device)
    sd = torch.full((nprob, npts), 7.0, dtype=torch.float64, device=ds.device)
    L, h = ds.lib, ds.h.ptr
    P = lambda a: a.data_ptr()
    # the kernel
    assert L.nlh_propagate(None, nprob, npts, n, P(dJ), P(dcov), None, P(sd)) == NLH_ERR_BAD_HANDLE
    for bad in ((-1, npts, n), (nprob, 0, n), (nprob, npts, 0)):
        assert L.nlh_propagate(h, *bad, P(dJ), P(dcov), None, P(sd)) == NL_INVALID_INPUT_ERROR, bad
    for args in ((None, P(dcov), None, P(sd)), (P(dJ), None, None, P(sd)), (P(dJ), P(dcov), None, None)):
        assert L.nlh_propagate(h, nprob, npts, n, *args) == NL_INVALID_INPUT_ERROR
    assert L.nlh_propagate(h, 0, npts, n, None, None, None, None) == 0
    # the curve and formula bands
    band = lambda hh, kind, KK, BB, np_, m_, t_, x_, c_, s_: L.nlh_curve_band_batch(hh, kind, KK, BB, np_, m_, t_, 0, x_, c_, None, P(y), s_)
    assert band(None, R.LORENTZ, K, B, nprob, npts, P(dt), P(dx), P(dcov), P(sd)) == NLH_ERR_BAD_HANDLE
    assert band(h, 7, K, B, nprob, npts, P(dt), P(dx), P(dcov), P(sd)) == NL_INVALID_INPUT_ERROR
    assert band(h, R.LORENTZ, K, B, nprob, 0, P(dt), P(dx), P(dcov), P(sd)) == NL_INVALID_INPUT_ERROR          # npts < 1
    assert band(h, R.LORENTZ, K, B, -1, npts, P(dt), P(dx), P(dcov), P(sd)) == NL_INVALID_INPUT_ERROR
    for args in ((None, P(dx), P(dcov), P(sd)), (P(dt), None, P(dcov), P(sd)), (P(dt), P(dx), None, P(sd)), (P(dt), P(dx), P(dcov), None)):
        assert band(h, R.LORENTZ, K, B, nprob, npts, *args) == NL_INVALID_INPUT_ERROR
    assert band(h, R.LORENTZ, K, B, 0, npts, None, None, None, None) == 0
    e = nl.Expr("a/(1+((t-mu)/w)^2)+c", "t", "a,mu,w,c")
    assert L.nlh_expr_band_batch(None, e.ptr, nprob, npts, P(dt), 0, P(dx), P(dcov), None, P(y), P(sd)) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_band_batch(h, None, nprob, npts, P(dt), 0, P(dx), P(dcov), None, P(y), P(sd)) == NL_INVALID_INPUT_ERROR
    assert L.nlh_expr_band_batch(h, e.ptr, nprob, 0, P(dt), 0, P(dx), P(dcov), None, P(y), P(sd)) == NL_INVALID_INPUT_ERROR
    assert L.nlh_expr_band_batch(h, e.ptr, nprob, npts, P(dt), 0, P(dx), None, None, P(y), P(sd)) == NL_INVALID_INPUT_ERROR
    assert L.nlh_expr_band_batch(h, e.ptr, nprob, npts, P(dt), 0, P(dx), P(dcov), None, P(y), None) == NL_INVALID_INPUT_ERROR
    # the chain
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, dt, y)
    f, j, c = ds._devfcn(fcn), ds._devfcn(jac), ds._ctxp(ctx)
    null = ds._devfcn(None)
    chain = lambda hh, ff, np_, m_, n_, x_, c_, s_: L.nlh_propagate_batch_device(hh, np_, m_, n_, ff, j, c, x_, c_, None, P(y), s_)
    assert chain(None, f, nprob, npts, n, P(dx), P(dcov), P(sd)) == NLH_ERR_BAD_HANDLE
    assert chain(h, null, nprob, npts, n, P(dx), P(dcov), P(sd)) == NL_UNDEFINED_FUNCTION_ERROR
    for bad in ((-1, npts, n), (nprob, 0, n), (nprob, npts, 0)):
        assert chain(h, f, *bad, P(dx), P(dcov), P(sd)) == NL_INVALID_INPUT_ERROR, bad
    for args in ((None, P(dcov), P(sd)), (P(dx), None, P(sd)), (P(dx), P(dcov), None)):
        assert chain(h, f, nprob, npts, n, *args) == NL_INVALID_INPUT_ERROR
    assert chain(h, f, 0, npts, n, None, None, None) == 0
    xh, chh, sh = x.copy(), np.ones((nprob, n, n)), np.full((nprob, npts), 7.0)
    assert L.nlh_propagate_batch_device_h(h, nprob, npts, n, f, j, c, xh.ctypes.data_as(dp), None, None, None,
                                          sh.ctypes.data_as(dp)) == NL_INVALID_INPUT_ERROR
    assert L.nlh_propagate_batch_device_h(None, nprob, npts, n, f, j, c, xh.ctypes.data_as(dp), chh.ctypes.data_as(dp), None, None,
                                          sh.ctypes.data_as(dp)) == NLH_ERR_BAD_HANDLE
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (sd == 7.0).all() and (sh == 7.0).all()          # nothing was launched
    # the host-array twin gives the device form's bits
    cov = _spd(np.random.default_rng(1), nprob, n)
    vh = np.zeros((nprob, npts))
    assert L.nlh_propagate_batch_device_h(h, nprob, npts, n, f, j, c, xh.ctypes.data_as(dp), cov.ctypes.data_as(dp), None,
                                          vh.ctypes.data_as(dp), sh.ctypes.data_as(dp)) == 0
    val, sdd = ds.propagate_batch_device(fcn, ctx, npts, dx, _dev(ds, cov), jac=jac)
    assert np.array_equal(_bits(vh), _bits(val.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sdd.cpu().numpy()))
    # the Python checks
    with pytest.raises(ValueError):
        ds.curve_band("lorentz", dx, dcov, dt, ncomp=2, baseline=B)
    with pytest.raises(ValueError):
        ds.curve_band("lorentz", dx, dcov[:, :2, :2].contiguous(), dt, ncomp=K, baseline=B)
    with pytest.raises(ValueError):
        ds.propagate(dJ, dcov, noise=torch.zeros(5, dtype=torch.float64, device=ds.device))
