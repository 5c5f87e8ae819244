"""GPU tests of the parameter covariance (nlh_covar, nlh_lm_covariance*): every form of the covar kernels (lane per problem,
workgroup per problem on an LDS window, the same on a global-memory window) and the whole chain F(x) -> Jacobian -> lmfactor
-> covar -> chi2 / sigma, bit for bit against the plain-Python restatement (tests/covar_restatement.py) on the factors of
the CPU oracle.  The restatement itself is held to mpmath, symmetry and the rank rule in tests/test_covar_cpu.py."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import covar_restatement as cr
import user_models as UM
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)
FORMS = [None, "lane", "lds", "global"]     # None: the form n selects; a forced form that cannot hold n falls back to it
LANE_MAX = 8                                # include/nonlin_hip.h
LDS_CAP = 160 * 1024 - 2048                 # the library's dynamic-LDS cap (include/nonlin_hip.h: 161,792 bytes)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


class _form:
    """NLH_COVAR_FORM for the calls inside (the library reads it at every call)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = os.environ.pop("NLH_COVAR_FORM", None)
        if self.form is not None:
            os.environ["NLH_COVAR_FORM"] = self.form

    def __exit__(self, *a):
        os.environ.pop("NLH_COVAR_FORM", None)
        if self.old is not None:
            os.environ["NLH_COVAR_FORM"] = self.old


def lds_max_n():
    """The largest n whose LDS window the host check lets through: from the byte count that check uses."""
    lib = _lib.load()
    n = 33                                   # (beyond the grouped sizes the count grows with n)
    assert lib.nlh_covar_lds_bytes(n) <= LDS_CAP
    while lib.nlh_covar_lds_bytes(n + 1) <= LDS_CAP:
        n += 1
    return n


def dq_factors(ds, nprob, m, n, seed):
    """R, ipvt of the exact lmfactor on the analytic Jacobians of seeded dense-quadratic problems."""
    A, b, xt, x0 = ds.generate(nprob, m, n, seed0=seed)
    J = ds.jacobian(A, 0.5, x0)
    f = ds.residual(A, b, 0.5, x0)
    R, ipvt = ds.lmfactor_exact(J, f)[:2]
    return R, ipvt


def lorentz_factors(ds, nprob, m, K, seed):
    t, y, xt, x0 = UM.lorentz_problems(nprob, m, K, seed=seed)
    lb = UM.LorentzBatch(t, y)
    try:
        x = torch.from_numpy(xt).to(ds.device)
        J = ds.fd_jacobian_device(lb.launch, lb.ctx, m, x)
        f = torch.zeros((nprob, m), dtype=torch.float64, device=ds.device)
        R, ipvt = ds.lmfactor_exact(J, f)[:2]
        torch.cuda.synchronize()
    finally:
        lb.close()
    return R, ipvt


def check_covar(ds, R, ipvt, form, tol=None, sample=None):
    """ds.covar against the restatement on the device's own R and ipvt: cov bitwise, rank exactly."""
    with _form(form):
        cov, rank = ds.covar(R, ipvt, tol)
    torch.cuda.synchronize()
    Rh, ih, ch, rh = R.cpu().numpy(), ipvt.cpu().numpy(), cov.cpu().numpy(), rank.cpu().numpy()
    n = Rh.shape[1]
    restate = cr.covar if n <= 24 else cr.covar_fast
    for p in (range(Rh.shape[0]) if sample is None else sample):
        want, l = restate(Rh[p].T, ih[p], tol)                  # R[p] is column-major: R[p].T[i, j] = R(i, j)
        assert rh[p] == l, (form, n, p, rh[p], l)
        assert np.array_equal(_bits(ch[p]), _bits(want)), (form, n, p, np.abs(ch[p] - want).max())
    return cov, rank


# ------------------------------------------------------------------------------------------------ stage
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 2, 3, LANE_MAX, LANE_MAX + 1, 24, 33, 63, 64, 65])
def test_covar_bitwise_every_form(ds, n, form):
    R, ipvt = dq_factors(ds, 5, n + 7, n, seed=100 + n)
    cov, rank = check_covar(ds, R, ipvt, form)
    assert (rank.cpu().numpy() == n).all()
    cov0, rank0 = check_covar(ds, R, ipvt, None, sample=[])      # and the forms with each other
    assert torch.equal(cov.view(torch.int64), cov0.view(torch.int64)) and torch.equal(rank, rank0)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", [1, 2, 4, 8])
def test_covar_lorentzian_jacobians(ds, K, form):
    m = {1: 64, 2: 256, 4: 512, 8: 1024}[K]
    R, ipvt = lorentz_factors(ds, 4, m, K, seed=40 + K)
    _, rank = check_covar(ds, R, ipvt, form)
    assert (rank.cpu().numpy() == 3 * K).all()


def test_covar_lds_edge_and_global(ds):
    """The largest n of the LDS form and the first of the global form (from the byte count the host check uses), and one n
    well into the global form; the LDS-edge sizes also forced to the global form."""
    nmax = lds_max_n()
    lib = _lib.load()
    assert lib.nlh_covar_lds_bytes(nmax) <= LDS_CAP < lib.nlh_covar_lds_bytes(nmax + 1)
    for n, forms in ((nmax, (None, "global")), (nmax + 1, (None, "lds")), (300, (None,))):
        R, ipvt = dq_factors(ds, 2, n + 20, n, seed=7 * n)
        got = []
        for form in forms:
            cov, rank = check_covar(ds, R, ipvt, form, sample=[0] if got else None)
            assert (rank.cpu().numpy() == n).all()
            got.append(cov)
        for c in got[1:]:
            assert torch.equal(c.view(torch.int64), got[0].view(torch.int64))


def _deficient_batch(ds, m, n, dup, src):
    """Three problems; the middle one has column dup = 2 * column src."""
    A, b, xt, x0 = ds.generate(3, m, n, seed0=900 + n)
    J = ds.jacobian(A, 0.5, x0)
    J[1, dup, :] = 2.0 * J[1, src, :]
    f = ds.residual(A, b, 0.5, x0)
    return ds.lmfactor_exact(J.contiguous(), f)[:2]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m,n,dup,src", [(50, 6, 4, 1), (90, 70, 33, 5)])
def test_rank_deficient_between_full_rank(ds, m, n, dup, src, form):
    R, ipvt = _deficient_batch(ds, m, n, dup, src)
    cov, rank = check_covar(ds, R, ipvt, form, tol=1e-10)
    assert rank.cpu().tolist() == [n, n - 1, n]
    c = cov[1].cpu().numpy()
    dropped = [i for i in range(n) if not c[i].any()]
    assert len(dropped) == 1 and dropped[0] in (dup, src) and not c[:, dropped[0]].any()
    assert dropped[0] == int(ipvt[1, n - 1])
    # the neighbours are what they are alone
    for p in (0, 2):
        alone, r1 = ds.covar(R[p:p + 1].contiguous(), ipvt[p:p + 1].contiguous(), 1e-10)
        assert torch.equal(alone[0].view(torch.int64), cov[p].view(torch.int64)) and int(r1[0]) == n


@pytest.mark.parametrize("form", [None, "lds", "global"])
def test_batch_above_65535(ds, form):
    nprob, m, n = 70000, 8, 3
    A, b, xt, x0 = ds.generate(nprob, m, n, seed0=31)
    J = ds.jacobian(A, 0.5, x0)
    f = ds.residual(A, b, 0.5, x0)
    Rs, ips = [], []
    for p0 in range(0, nprob, 32768):                              # (the stage-level factorisation takes a lock-step slice)
        R, ip = ds.lmfactor_exact(J[p0:p0 + 32768].contiguous(), f[p0:p0 + 32768].contiguous())[:2]
        Rs.append(R); ips.append(ip)
    R, ipvt = torch.cat(Rs).contiguous(), torch.cat(ips).contiguous()
    cov, rank = check_covar(ds, R, ipvt, form, sample=range(0, nprob, 997))
    assert int((rank != n).sum()) == 0
    for p0 in (0, 65535, 69990):
        c, r = ds.covar(R[p0:p0 + 10].contiguous(), ipvt[p0:p0 + 10].contiguous())
        assert torch.equal(c.view(torch.int64), cov[p0:p0 + 10].view(torch.int64))


def test_bad_arguments_launch_nothing(ds):
    from nonlin_amd.api import NL_INVALID_INPUT_ERROR
    R = torch.ones((2, 3, 3), dtype=torch.float64, device=ds.device)
    ip = torch.zeros((2, 3), dtype=torch.int32, device=ds.device)
    cov = torch.full((2, 3, 3), 7.0, dtype=torch.float64, device=ds.device)
    rk = torch.full((2,), 7, dtype=torch.int32, device=ds.device)
    lib = ds.lib
    assert lib.nlh_covar(ds.h.ptr, 2, 0, R.data_ptr(), ip.data_ptr(), 0.0, cov.data_ptr(), rk.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert lib.nlh_covar(ds.h.ptr, -1, 3, R.data_ptr(), ip.data_ptr(), 0.0, cov.data_ptr(), rk.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert lib.nlh_covar(ds.h.ptr, 2, 3, None, ip.data_ptr(), 0.0, cov.data_ptr(), rk.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert lib.nlh_covar(ds.h.ptr, 0, 3, R.data_ptr(), ip.data_ptr(), 0.0, cov.data_ptr(), rk.data_ptr()) == 0
    assert lib.nlh_covar(None, 2, 3, R.data_ptr(), ip.data_ptr(), 0.0, cov.data_ptr(), rk.data_ptr()) == -3
    torch.cuda.synchronize()
    assert (cov == 7.0).all() and (rk == 7).all()
    # an ipvt entry outside [0, n) is skipped, not followed: nothing outside cov is written
    ip2 = torch.tensor([[0, 1, 9], [0, -4, 2]], dtype=torch.int32, device=ds.device)
    guard = torch.full((3, 3, 3), 7.0, dtype=torch.float64, device=ds.device)
    for form in FORMS:
        with _form(form):
            assert lib.nlh_covar(ds.h.ptr, 2, 3, R.data_ptr(), ip2.data_ptr(), 0.0, guard.data_ptr(), rk.data_ptr()) == 0
        torch.cuda.synchronize()
        assert (guard[2] == 7.0).all()


def test_timing_group(ds):
    """One bracket per nlh_covar call, whatever the form launches."""
    assert ds.lib.nlh_kernel_name(15) == b"k_covar"
    R, ipvt = dq_factors(ds, 100, 12, 5, seed=3)
    ds.h.timing_enable(kernels=["covar"])
    ds.h.timing_reset()
    try:
        for form in (None, "lds", "global"):
            with _form(form):
                ds.covar(R, ipvt)
        ms, launches = ds.h.timing("covar")
    finally:
        ds.h.timing_enable(False)
    assert launches == 3 and ms > 0.0


# ------------------------------------------------------------------------------------------------ chain
def _oracle_chain(oracle, host_fcn, host_jac, hctx, m, n, x, scaled, tol):
    """F(x) by the family's host twin, vfh_jac_fcn by the oracle, the oracle's lmfactor, the restatement."""
    x = np.array(x, dtype=np.float64)
    f = np.zeros(m)
    C.cast(host_fcn, oracle.VECFCN)(C.cast(C.byref(hctx), C.c_void_p), n, x.ctypes.data_as(dp), m, f.ctypes.data_as(dp))
    J = np.zeros((m, n), order="F")
    rc = oracle.lib().nlo_fd_jacobian(C.cast(host_fcn, oracle.VECFCN), C.cast(host_jac, oracle.JACFCN), C.byref(hctx), m, n,
                                      x.ctypes.data_as(dp), f.ctypes.data_as(dp), J.ctypes.data_as(dp))
    assert rc == 0
    a, ipvt, rdiag, _ = oracle.lmfactor(J)
    return cr.lm_covariance(cr.r_of_lmfactor(a, rdiag), ipvt, f, scaled=scaled, tol=tol)


def _cmp_chain(got, want, p, what):
    cov, sigma, rank, chi2 = got
    wc, ws, wr, wq = want
    assert int(rank) == wr, (what, p, int(rank), wr)
    assert np.array_equal(_bits(chi2), _bits(wq)), (what, p, float(chi2), wq)
    assert np.array_equal(_bits(cov), _bits(wc)), (what, p, np.abs(np.asarray(cov) - wc).max())
    assert np.array_equal(_bits(sigma), _bits(ws)), (what, p)


def _to_host(res):
    return tuple(t.cpu().numpy() for t in res)


@pytest.mark.parametrize("nprob", [1, 300])
@pytest.mark.parametrize("scaled", [True, False])
def test_chain_lorentz_fd(ds, oracle, nprob, scaled):
    m, K = 64, 2
    n = 3 * K
    t, y, xt, x0 = UM.lorentz_problems(nprob, m, K, seed=77)
    lb = UM.LorentzBatch(t, y)
    try:
        x = torch.from_numpy(x0).to(ds.device)
        keep = x.clone()
        cov, sigma, rank, chi2 = _to_host(ds.lm_covariance_batch_device(lb.launch, lb.ctx, m, x, scaled=scaled))
        assert torch.equal(x.view(torch.int64), keep.view(torch.int64))          # x is not modified
        for p in range(nprob):
            want = _oracle_chain(oracle, lb.host_fcn, None, lb.host_ctx(p), m, n, x0[p], scaled, None)
            _cmp_chain((cov[p], sigma[p], rank[p], chi2[p]), want, p, "lorentz")
        assert (rank == n).all()
        if nprob > 1:                                               # problem p alone: the same bits (its own data: dprob = 0)
            for p in (0, 137, nprob - 1):
                one = UM.LorentzBatch(t[p:p + 1], y[p:p + 1])
                c1, s1, r1, q1 = _to_host(ds.lm_covariance_batch_device(one.launch, one.ctx, m, x[p:p + 1].contiguous(), scaled=scaled))
                one.close()
                assert np.array_equal(_bits(c1[0]), _bits(cov[p])) and np.array_equal(_bits(s1[0]), _bits(sigma[p]))
                assert r1[0] == rank[p] and np.array_equal(_bits(q1), _bits(chi2[p:p + 1]))
    finally:
        lb.close()


@pytest.mark.parametrize("nprob", [1, 300])
def test_chain_analytic_jacobian(ds, oracle, nprob):
    """A family with m > n and a jacfcn: the dense-quadratic family through its launchers, the oracle's nlo_dq_fcn /
    nlo_dq_jac as the host twins."""
    m, n, gamma = 40, 9, 0.5
    A, b, xt, x0 = ds.generate(nprob, m, n, seed0=555)
    fcn, jac, ctx = ds.dq_launchers(A, b, gamma)
    cov, sigma, rank, chi2 = _to_host(ds.lm_covariance_batch_device(fcn, ctx, m, x0, jac=jac, tol=1e-12))
    L = oracle.lib()
    Ah, bh, xh = A.cpu().numpy(), b.cpu().numpy(), x0.cpu().numpy()
    for p in range(nprob):
        Ap = np.asfortranarray(Ah[p].T)
        prob = oracle._dq_problem(Ap, bh[p], gamma)
        want = _oracle_chain(oracle, L.nlo_dq_fcn, L.nlo_dq_jac, prob, m, n, xh[p], True, 1e-12)
        _cmp_chain((cov[p], sigma[p], rank[p], chi2[p]), want, p, "dq analytic")
    # without the jacfcn: forward differences, different bits in general, the same yardstick
    cov2, sigma2, rank2, chi22 = _to_host(ds.lm_covariance_batch_device(fcn, ctx, m, x0, tol=1e-12))
    for p in range(0, nprob, 37):
        Ap = np.asfortranarray(Ah[p].T)
        prob = oracle._dq_problem(Ap, bh[p], gamma)
        want = _oracle_chain(oracle, L.nlo_dq_fcn, None, prob, m, n, xh[p], True, 1e-12)
        _cmp_chain((cov2[p], sigma2[p], rank2[p], chi22[p]), want, p, "dq fd")
    assert np.array_equal(_bits(chi2), _bits(chi22))


def test_chain_above_65535_runs_in_slices(ds):
    """66,000 problems in one call: every row equals the same problem in a call of its own slice of the batch."""
    nprob, m, n, gamma = 66000, 8, 3, 0.5
    A, b, xt, x0 = ds.generate(nprob, m, n, seed0=4242)
    fcn, jac, ctx = ds.dq_launchers(A, b, gamma)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(fcn, ctx, m, x0)
    assert int((rank != n).sum()) == 0
    for p0, cnt in ((0, 50), (65530, 10), (65535, 465)):
        f2, j2, c2 = ds.dq_launchers(A[p0:p0 + cnt].contiguous(), b[p0:p0 + cnt].contiguous(), gamma)
        cs, ss, rs, qs = ds.lm_covariance_batch_device(f2, c2, m, x0[p0:p0 + cnt].contiguous())
        assert torch.equal(cs.view(torch.int64), cov[p0:p0 + cnt].view(torch.int64))
        assert torch.equal(ss.view(torch.int64), sigma[p0:p0 + cnt].view(torch.int64))
        assert torch.equal(qs.view(torch.int64), chi2[p0:p0 + cnt].view(torch.int64))


def test_chain_error_returns_evaluate_nothing(ds):
    from nonlin_amd.api import NL_INVALID_INPUT_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR, NL_UNDEFINED_FUNCTION_ERROR
    t, y, xt, x0 = UM.lorentz_problems(2, 6, 2, seed=1)            # m = 6 = n
    lb = UM.LorentzBatch(t, y)
    calls = [0]

    def counting(ctx, stream, npoints, dprob, n, dX, m, dF):
        calls[0] += 1
        return lb.launch(ctx, stream, npoints, dprob, n, dX, m, dF)
    lb.launch.restype = C.c_int
    lb.launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    cfn = _lib.DEVFCN(counting)
    null = C.cast(None, _lib.DEVFCN)
    x = torch.from_numpy(x0).to(ds.device)
    cov = torch.full((2, 6, 6), 7.0, dtype=torch.float64, device=ds.device)

    def call(m, n, scaled, fcn=cfn):
        return ds.lib.nlh_lm_covariance_batch_device(ds.h.ptr, 2, m, n, fcn, null, lb.ctx, x.data_ptr(), scaled, 0.0, cov.data_ptr(),
                                                     None, None, None)
    try:
        assert call(6, 6, 1) == NL_INVALID_INPUT_ERROR              # scaled with m <= n
        assert call(5, 6, 1) == NL_INVALID_INPUT_ERROR
        assert call(5, 6, 0) == NL_UNDERDEFINED_PROBLEM_ERROR        # m < n
        assert call(6, 6, 1, null) == NL_UNDEFINED_FUNCTION_ERROR
        torch.cuda.synchronize()
        assert calls[0] == 0 and (cov == 7.0).all()
        assert call(6, 6, 0) == 0                                    # m == n unscaled is a valid request, and evaluates
        torch.cuda.synchronize()
        assert calls[0] >= 2 and not (cov == 7.0).all()
        with pytest.raises(RuntimeError):
            ds.lm_covariance_batch_device(cfn, lb.ctx, 6, x, scaled=True)
        # the host-callback form: the counter in the host context
        hc = lb.host_ctx(0)
        xh = x0[0].copy()
        c1 = np.zeros((6, 6))
        for m, scaled, want in ((6, 1, NL_INVALID_INPUT_ERROR), (5, 0, NL_UNDERDEFINED_PROBLEM_ERROR)):
            rc = ds.lib.nlh_lm_covariance(ds.h.ptr, m, 6, C.cast(lb.host_fcn, _lib.VECFCN), C.cast(None, _lib.JACFCN), C.byref(hc),
                                          xh.ctypes.data_as(dp), scaled, 0.0, c1.ctypes.data_as(dp), None, None, None)
            assert rc == want and hc.ncalls == 0
    finally:
        lb.close()


def test_after_a_solve_workspaces_are_shared_safely(ds):
    """solve, covariance, solve again on one handle: the second solve reproduces the first one's bits."""
    nprob, m, K = 40, 97, 2
    t, y, xt, x0 = UM.lorentz_problems(nprob, m, K, seed=9, hard_every=4)
    lb = UM.LorentzBatch(t, y)
    try:
        o = ds.options(max_evals=500)
        x1 = torch.from_numpy(x0).to(ds.device)
        f1, ib1, st1 = ds.lm_solve_batch_device(lb.launch, lb.ctx, m, x1, opts=o)
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(lb.launch, lb.ctx, m, x1)
        x2 = torch.from_numpy(x0).to(ds.device)
        f2, ib2, st2 = ds.lm_solve_batch_device(lb.launch, lb.ctx, m, x2, opts=o)
        torch.cuda.synchronize()
        assert torch.equal(x1.view(torch.int64), x2.view(torch.int64)) and torch.equal(f1.view(torch.int64), f2.view(torch.int64))
        assert ib1 == ib2 and st1 == st2
        assert (rank == 3 * K).all() and bool(torch.isfinite(sigma).all()) and bool((sigma > 0).all())
        # ... and the covariance at the solution does not depend on what ran before it
        cov2, sigma2, rank2, chi22 = ds.lm_covariance_batch_device(lb.launch, lb.ctx, m, x2)
        assert torch.equal(cov.view(torch.int64), cov2.view(torch.int64)) and torch.equal(chi2.view(torch.int64), chi22.view(torch.int64))
    finally:
        lb.close()


def test_host_callback_and_model_forms_same_bits(ds, oracle):
    import nonlin_amd as nl
    nprob, m, K = 5, 64, 2
    n = 3 * K
    t, y, xt, x0 = UM.lorentz_problems(nprob, m, K, seed=21)
    lb = UM.LorentzBatch(t, y)
    try:
        x = torch.from_numpy(x0).to(ds.device)
        cov, sigma, rank, chi2 = _to_host(ds.lm_covariance_batch_device(lb.launch, lb.ctx, m, x))
        # host arrays
        ch, sh, rh, qh = np.zeros((nprob, n, n)), np.zeros((nprob, n)), np.zeros(nprob, dtype=np.int32), np.zeros(nprob)
        rc = ds.lib.nlh_lm_covariance_batch_device_h(ds.h.ptr, nprob, m, n, ds._devfcn(lb.launch), ds._devfcn(None), lb.ctx,
                                                     x0.ctypes.data_as(dp), 1, 0.0, ch.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                                     rh.ctypes.data_as(_lib.c_int32_p), qh.ctypes.data_as(dp))
        assert rc == 0
        assert np.array_equal(_bits(ch), _bits(cov)) and np.array_equal(_bits(sh), _bits(sigma))
        assert np.array_equal(rh, rank) and np.array_equal(_bits(qh), _bits(chi2))
        # a user-launcher model object
        md = C.c_void_p()
        assert ds.lib.nlh_device_fcn_model_create(nprob, m, n, ds._devfcn(lb.launch), ds._devfcn(None), lb.ctx, C.byref(md)) == 0
        try:
            cm, sm, qm = np.zeros((nprob, n, n)), np.zeros((nprob, n)), np.zeros(nprob)
            rm = np.zeros(nprob, dtype=np.int32)
            assert ds.lib.nlh_dq_model_lm_covariance(ds.h.ptr, md, x0.ctypes.data_as(dp), 1, 0.0, cm.ctypes.data_as(dp),
                                                     sm.ctypes.data_as(dp), rm.ctypes.data_as(_lib.c_int32_p), qm.ctypes.data_as(dp)) == 0
            assert np.array_equal(_bits(cm), _bits(cov)) and np.array_equal(_bits(sm), _bits(sigma))
            assert np.array_equal(rm, rank) and np.array_equal(_bits(qm), _bits(chi2))
        finally:
            ds.lib.nlh_dq_model_destroy(md)
        # host callbacks: the C twin (call count: 1 + n, x restored), and the Python API
        for p in range(nprob):
            hc = lb.host_ctx(p)
            xp = x0[p].copy()
            c1, s1, r1, q1 = np.zeros((n, n)), np.zeros(n), C.c_int32(0), C.c_double(0.0)
            rc = ds.lib.nlh_lm_covariance(ds.h.ptr, m, n, C.cast(lb.host_fcn, _lib.VECFCN), C.cast(None, _lib.JACFCN), C.byref(hc),
                                          xp.ctypes.data_as(dp), 1, 0.0, c1.ctypes.data_as(dp), s1.ctypes.data_as(dp),
                                          C.byref(r1), C.byref(q1))
            assert rc == 0 and hc.ncalls == 1 + n and np.array_equal(_bits(xp), _bits(x0[p]))
            assert np.array_equal(_bits(c1), _bits(cov[p])) and np.array_equal(_bits(s1), _bits(sigma[p]))
            assert r1.value == rank[p] and np.array_equal(_bits(q1.value), _bits(chi2[p]))
        helper = nl.vecfcn_helper()
        helper.set_fcn(lambda xx, ff, args: ff.__setitem__(slice(None), UM.lorentz_row_numpy(xx, t[0], y[0])), m, n)
        xp = x0[0].copy()
        c2, s2, r2, q2 = nl.least_squares_solver().covariance(helper, xp)
        assert np.array_equal(_bits(c2), _bits(cov[0])) and np.array_equal(_bits(s2), _bits(sigma[0]))
        assert r2 == rank[0] and np.array_equal(_bits(q2), _bits(chi2[0])) and np.array_equal(_bits(xp), _bits(x0[0]))
    finally:
        lb.close()


def test_builtin_model_forms_same_bits(ds):
    """HostModel.lm_covariance (one device, and dealt over two shares of a device set) = the launcher form on the family."""
    from nonlin_amd.device import DeviceSet
    nprob, m, n, gamma = 7, 30, 5, 0.5
    A, b, xt, x0 = ds.generate(nprob, m, n, seed0=88)
    fcn, jac, ctx = ds.dq_launchers(A, b, gamma)
    cov, sigma, rank, chi2 = _to_host(ds.lm_covariance_batch_device(fcn, ctx, m, x0, scaled=False, tol=1e-9))
    Ah, bh, xh = A.cpu().numpy(), b.cpu().numpy(), x0.cpu().numpy()
    owners = [ds, DeviceSet([0, 0])]
    for owner in owners:
        md = owner.model(Ah, bh, gamma)
        try:
            c, s, r, q = md.lm_covariance(xh, scaled=False, tol=1e-9)
        finally:
            md.close()
        assert np.array_equal(_bits(c), _bits(cov)) and np.array_equal(_bits(s), _bits(sigma))
        assert np.array_equal(r, rank) and np.array_equal(_bits(q), _bits(chi2))
    owners[1].close()


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
    UM.lib()                                                       # (builds tests/device_model/libuser_models.so if missing)
    d = tmp_path_factory.mktemp("fortran_covar")
    exe = str(d / "covar_suite")
    libdir, umdir = os.path.join(ROOT, "nonlin_amd"), os.path.join(HERE, "device_model")
    subprocess.check_call([fc, "-O2", "-I" + shim, "-module-dir", str(d), os.path.join(HERE, "fortran_covar", "covar_suite.f90"),
                           "-o", exe, os.path.join(shim, "libnonlin_shim.a"), "-L" + libdir, "-lnonlin_hip", "-L" + umdir,
                           "-luser_models", "-Wl,-rpath," + libdir, "-Wl,-rpath," + umdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe, d


def test_fortran_covar_suite(fortran_exe, oracle):
    import problems_ref as P
    exe, d = fortran_exe
    nprob, m, K = 3, 64, 2
    n = 3 * K
    t, y, xt, x0 = UM.lorentz_problems(nprob, m, K, seed=63)
    path = str(d / "spectra.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m, n], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(x0.tobytes())     # (row-major [nprob, m] = column-major (m, nprob))
    out = subprocess.run(["timeout", "-k", "10", "300", exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    res = {}
    for line in out.stdout.splitlines():
        tk = line.split()
        if tk:
            res[tk[0]] = np.array([_unhex(v) for v in tk[1:]])
    assert "done" in res

    # README Example 2 through covariance (host callback)
    rc, xo, fo, ibo = oracle.lm_solve(lambda x, f: P.lsfcn1(x, f, None), 21, 4, [1.0] * 4)
    assert rc == 0 and np.array_equal(_bits(res["readme_x"]), _bits(xo))

    def chain(scaled, tol):
        f = np.zeros(21)
        P.lsfcn1(xo, f, None)
        J = oracle.fd_jacobian(lambda x, ff: P.lsfcn1(x, ff, None), 21, 4, xo, fv=f)
        a, ipvt, rdiag, _ = oracle.lmfactor(J)
        return cr.lm_covariance(cr.r_of_lmfactor(a, rdiag), ipvt, f, scaled=scaled, tol=tol)
    wc, ws, wr, wq = chain(True, None)
    assert np.array_equal(_bits(res["readme_cov"]), _bits(wc.ravel())) and np.array_equal(_bits(res["readme_sigma"]), _bits(ws))
    assert res["readme_rank_chi2"][0] == wr == 4 and np.array_equal(_bits(res["readme_rank_chi2"][1]), _bits(wq))
    assert np.array_equal(_bits(res["readme_cov_unscaled"]), _bits(chain(False, 1e-10)[0].ravel()))

    # the device-fcn model: one problem and the batch
    lb = UM.LorentzBatch(t, y)
    try:
        for p in range(nprob):
            wc, ws, wr, wq = _oracle_chain(oracle, lb.host_fcn, None, lb.host_ctx(p), m, n, x0[p], True, None)
            k = p + 1
            assert np.array_equal(_bits(res[f"dev_batch_cov_{k}"]), _bits(wc.ravel()))
            assert np.array_equal(_bits(res[f"dev_batch_sigma_{k}"]), _bits(ws))
            assert res[f"dev_batch_rank_chi2_{k}"][0] == wr and np.array_equal(_bits(res[f"dev_batch_rank_chi2_{k}"][1]), _bits(wq))
            if p == 0:
                assert np.array_equal(_bits(res["dev_one_cov"]), _bits(wc.ravel())) and np.array_equal(_bits(res["dev_one_sigma"]), _bits(ws))
                assert res["dev_one_rank_chi2"][0] == wr and np.array_equal(_bits(res["dev_one_rank_chi2"][1]), _bits(wq))
                wu = _oracle_chain(oracle, lb.host_fcn, None, lb.host_ctx(0), m, n, x0[0], False, None)[0]
                assert np.array_equal(_bits(res["dev_batch_unscaled_1"]), _bits(wu.ravel()))
    finally:
        lb.close()
