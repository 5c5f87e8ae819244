"""GPU tests of the built-in curve models (include/nonlin_hip.h: nlh_curve_*): the kernels bit for bit against the numpy
restatement where no exp occurs and within the stated rounding bound where one does, both workgroup forms and every
launch shape; solves bit for bit against the hand-written user family and against the CPU oracle; nlh_curve_fit_batch as
the composition of the three calls it stands for, with the degrees-of-freedom rule of zero-weight padding; the model
object; the Fortran surface."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import curve_cases as CC
import curve_restatement as R
import user_models as UM
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
dp = C.POINTER(C.c_double)
KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
FORMS = [None, "row", "flat"]               # None: the form m selects; a forced form that cannot hold m falls back to it
U = 2.0 ** -52
NL_INVALID_INPUT_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR = 201, 212
RATIOS = {}                                 # largest observed |dev - numpy| / bound of the exp kinds, printed by the tests


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return all(a[k] == b[k] for k in KEYS)


class _form:
    """NLH_CURVE_FORM for the calls inside (the library reads it at every call)."""

    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = os.environ.pop("NLH_CURVE_FORM", None)
        if self.form is not None:
            os.environ["NLH_CURVE_FORM"] = self.form

    def __exit__(self, *a):
        os.environ.pop("NLH_CURVE_FORM", None)
        if self.old is not None:
            os.environ["NLH_CURVE_FORM"] = self.old


def _dev(ds, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ds.device)


def _launch(ds, fcn, ctx, plist, X, m, jac=False):
    """One call of a launcher on the points X (numpy [npoints, n]) of the problems plist: F [npoints, m] or J [npoints, n, m]."""
    npts, n = X.shape
    dX, dprob = _dev(ds, X), _dev(ds, plist, np.int32)
    out = torch.full((npts, n, m) if jac else (npts, m), np.nan, dtype=torch.float64, device=ds.device)
    stream = torch.cuda.current_stream(ds.device).cuda_stream
    rc = fcn(ds._ctxp(ctx), C.c_void_p(stream), npts, C.c_void_p(dprob.data_ptr()), n, C.c_void_p(dX.data_ptr()), m,
             C.c_void_p(out.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _weights(rng, nprob, m, zeros=True):
    w = rng.uniform(0.5, 2.0, (nprob, m))
    if zeros:
        w[rng.uniform(size=(nprob, m)) < 0.1] = 0.0
    return w


def _shapes(nprob, n):
    """Launch shapes: one point, n + 1 points of one problem, a mixed list."""
    rng = np.random.default_rng(3)
    return [[nprob - 2], [2] * (n + 1), list(rng.integers(0, nprob, 37)) + [0, 0, nprob - 1]]


def _points(x0, plist, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(x0[plist] * (1.0 + 0.01 * rng.uniform(-1, 1, (len(plist), x0.shape[1]))))


# ------------------------------------------------------------------------------------------------ 1. kernels, exp-free
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", [64, 200, 256, 301])
@pytest.mark.parametrize("B,weighted,shared", [(-1, False, False), (-1, True, False), (2, False, False), (2, True, False),
                                               (-1, False, True), (2, True, True)])
def test_lorentz_kernels_bitwise(ds, B, weighted, shared, m, form):
    K, nprob = 2, 5
    kd, n = R.LORENTZ, R.nparams(R.LORENTZ, K, B)
    t, y, xt, x0 = CC.curve_problems("lorentz", K, B, m, nprob=nprob, seed=11 + m)
    if shared:
        t = np.tile(t[0], (nprob, 1))
    w = _weights(np.random.default_rng(m), nprob, m) if weighted else None
    dt, dy, dw = _dev(ds, t[0] if shared else t), _dev(ds, y), (_dev(ds, w) if weighted else None)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, dt, dy, dw)
    for k, plist in enumerate(_shapes(nprob, n)):
        X = _points(x0, plist, k)
        with _form(form):
            F = _launch(ds, fcn, ctx, plist, X, m)
            J = _launch(ds, jac, ctx, plist, X, m, jac=True)
        for q, p in enumerate(plist):
            wp = w[p] if weighted else None
            assert np.array_equal(_bits(F[q]), _bits(R.residual(kd, K, B, X[q], t[p], y[p], wp))), (form, k, q)
            assert np.array_equal(_bits(J[q]), _bits(R.jacobian(kd, K, B, X[q], t[p], wp).T)), (form, k, q)


# ------------------------------------------------------------------------------------------------ 2. the user family
def test_builtin_lorentz_equals_user_written_family(ds):
    nprob, m, K = 300, 512, 4
    t, y, xt, x0 = UM.lorentz_problems(nprob, m, K, hard_every=4)
    lb = UM.LorentzBatch(t, y)
    try:
        o = ds.options(max_evals=500)
        xu = _dev(ds, x0)
        fu, ibu, stu = ds.lm_solve_batch_device(lb.launch, lb.ctx, m, xu, opts=o)
        dt, dy = _dev(ds, t), _dev(ds, y)
        fcn, jac, ctx = ds.curve_launchers("lorentz", K, -1, dt, dy)
        xb = _dev(ds, x0)
        fb, ibb, stb = ds.lm_solve_batch_device(fcn, ctx, m, xb, opts=o)
        torch.cuda.synchronize()
        assert torch.equal(xu.view(torch.int64), xb.view(torch.int64)) and torch.equal(fu.view(torch.int64), fb.view(torch.int64))
        assert ibu == ibb and stu == stb
        assert len({ib["jacobian_count"] for ib in ibb}) > 1         # (a heterogeneous batch)
    finally:
        lb.close()


# ------------------------------------------------------------------------------------------------ 3. solves, the oracle
class _OneProblem:
    """Problem p of a batch alone, on the device: F through a model object's eval (nlh_curve_model_create, host arrays),
    J through fd_jacobian_device with the Jacobian launcher -- one point per call."""

    def __init__(self, ds, kind, K, B, t, y, w=None):
        self.ds, self.m, self.n = ds, len(y), R.nparams(R.KINDS[kind], K, B)
        self.md = C.c_void_p()
        rc = ds.lib.nlh_curve_model_create(ds.h.ptr, R.KINDS[kind], K, B, 1, self.m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp),
                                           w.ctypes.data_as(dp) if w is not None else None, 1, C.byref(self.md))
        assert rc == 0
        self.keep = (_dev(ds, t[None]), _dev(ds, y[None]), _dev(ds, w[None]) if w is not None else None)
        self.fcn_l, self.jac_l, self.ctx = ds.curve_launchers(kind, K, B, *self.keep)

    def fcn(self, x, f):
        xx = np.ascontiguousarray(x)
        out = np.empty(self.m)
        assert self.ds.lib.nlh_dq_model_eval(self.ds.h.ptr, self.md, xx.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
        f[:] = out

    def jac(self, x, J):
        Jd = self.ds.fd_jacobian_device(self.fcn_l, self.ctx, self.m, _dev(self.ds, np.ascontiguousarray(x)[None]), jac=self.jac_l)
        J[:, :] = Jd[0].cpu().numpy().T

    def close(self):
        self.ds.lib.nlh_dq_model_destroy(self.md)


def _oracle_callbacks(ds, kind, K, B, t, y, analytic):
    """(fcn, jac, close) for the oracle: the numpy restatement for the exp-free kind, the device itself for the others."""
    kd = R.KINDS[kind]
    if kd == R.LORENTZ:
        fcn = lambda x, f: f.__setitem__(slice(None), R.residual(kd, K, B, x, t, y))
        jac = (lambda x, J: J.__setitem__((slice(None), slice(None)), R.jacobian(kd, K, B, x, t))) if analytic else None
        return fcn, jac, lambda: None
    one = _OneProblem(ds, kind, K, B, t, y)
    return one.fcn, (one.jac if analytic else None), one.close


def _solve_case(ds, oracle, kind, K, B, m, analytic, bounded=False, **okw):
    kd, n = R.KINDS[kind], R.nparams(R.KINDS[kind], K, B)
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m)
    opt = dict(max_evals=CC.MAX_EVALS, **okw)
    lower = upper = None
    if bounded:                                 # a box some true values lie outside of: bounds that bind
        lower, upper = np.minimum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) - 0.02, np.maximum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) + 0.02
        x0 = np.clip(x0, lower, upper)
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    x = _dev(ds, x0)
    if bounded:
        fvec, ibs, status = ds.cls_solve_batch_device(fcn, ctx, m, x, jac=jac if analytic else None, opts=ds.options(**opt),
                                                      lower=lower, upper=upper)
    else:
        fvec, ibs, status = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=jac if analytic else None, opts=ds.options(**opt))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    counts = [ib["jacobian_count"] for ib in ibs]
    # the exp-free kind: every problem; the others (a device round trip per callback): a sample with every distinct count
    pick = range(CC.NPROB) if kd == R.LORENTZ else CC.sample(counts, 32)
    assert len(pick) >= 32 and {counts[p] for p in pick} == set(counts)
    oo = oracle.default_options(**opt)
    for p in pick:
        f, j, close = _oracle_callbacks(ds, kind, K, B, t[p], y[p], analytic)
        try:
            if bounded:
                rc, xo, fo, ibo = oracle.cls_solve(f, m, n, x0[p], jac=j, opts=oo, lower=lower, upper=upper)
            else:
                rc, xo, fo, ibo = oracle.lm_solve(f, m, n, x0[p], jac=j, opts=oo)
        finally:
            close()
        what = (kind, K, B, m, analytic, p)
        assert status[p] == rc, (what, status[p], rc)
        assert _same(ibs[p], ibo), (what, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), what
    if not bounded:
        assert set(status) == {0}, (kind, K, B, m, sorted(set(status)))
    return counts


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("kind,K,B,m", CC.CASES)
def test_solves_against_oracle(ds, oracle, kind, K, B, m, analytic):
    _solve_case(ds, oracle, kind, K, B, m, analytic)


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("kind,K,B,m", [CC.CASES[1], CC.CASES[4], CC.CASES[6]])
def test_solves_small_factor(ds, oracle, kind, K, B, m, analytic):
    """factor = 0.1: a small first trust region (lmpar's loop, rejected trials)."""
    _solve_case(ds, oracle, kind, K, B, m, analytic, factor=0.1)


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("kind,K,B,m", [CC.CASES[0], CC.CASES[4], CC.CASES[5]])
def test_bounded_solves_against_oracle(ds, oracle, kind, K, B, m, analytic):
    _solve_case(ds, oracle, kind, K, B, m, analytic, bounded=True)


# ------------------------------------------------------------------------------------------------ 4. the exp kinds
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,K,B,m", [c for c in CC.CASES if c[0] != "lorentz"])
def test_exp_kinds_within_rounding_bound(ds, kind, K, B, m, form):
    """|dev - numpy| <= (K + 4) 2^-52 (sum |term_k| + |b| + |y|) per residual row, <= 8 * 2^-52 |entry| per Jacobian entry:
    both exps within 1 ulp, and the operation count.  The largest observed ratios are printed (and copied into
    profiles/curve_rate.txt by profiles/scripts/curve_rate.py --append)."""
    kd, n, nprob = R.KINDS[kind], R.nparams(R.KINDS[kind], K, B), 8
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob)
    dt, dy = _dev(ds, t), _dev(ds, y)                               # (kept alive: the context holds addresses only)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    rf = rj = 0.0
    for k, plist in enumerate(_shapes(nprob, n)):
        X = _points(x0, plist, 20 + k)
        with _form(form):
            F = _launch(ds, fcn, ctx, plist, X, m)
            J = _launch(ds, jac, ctx, plist, X, m, jac=True)
        for q, p in enumerate(plist):
            want = R.residual(kd, K, B, X[q], t[p], y[p])
            bound = (K + 4) * U * R.abs_sum(kd, K, B, X[q], t[p], y[p])
            rf = max(rf, float((np.abs(F[q] - want) / bound).max()))
            wj = R.jacobian(kd, K, B, X[q], t[p]).T
            nz = wj != 0.0
            assert np.array_equal(J[q][~nz], wj[~nz])
            rj = max(rj, float((np.abs(J[q] - wj)[nz] / (8 * U * np.abs(wj[nz]))).max()))
    RATIOS[(kind, K, B, m, form)] = (rf, rj)
    print(f"curve exp bound ratio {kind} K={K} B={B} m={m} form={form}: residual {rf:.3f} jacobian {rj:.3f}")
    assert rf <= 1.0 and rj <= 1.0, (kind, K, B, m, form, rf, rj)


@pytest.mark.parametrize("kind,K,B,m", [c for c in CC.CASES if c[0] != "lorentz" and c[3] <= 256])
def test_exp_kinds_forms_and_shapes_same_bits(ds, kind, K, B, m):
    """A row's bits do not depend on the form or on the launch it sits in."""
    n, nprob = R.nparams(R.KINDS[kind], K, B), 8
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob)
    w = _weights(np.random.default_rng(1), nprob, m)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy, dw)
    plist = _shapes(nprob, n)[2]
    X = _points(x0, plist, 9)
    got = {}
    for form in FORMS:
        with _form(form):
            got[form] = (_launch(ds, fcn, ctx, plist, X, m), _launch(ds, jac, ctx, plist, X, m, jac=True))
    for form in FORMS[1:]:
        assert np.array_equal(_bits(got[form][0]), _bits(got[None][0])) and np.array_equal(_bits(got[form][1]), _bits(got[None][1]))
    for q in (0, 17, len(plist) - 1):                               # ... and a point alone
        F1 = _launch(ds, fcn, ctx, plist[q:q + 1], X[q:q + 1], m)
        J1 = _launch(ds, jac, ctx, plist[q:q + 1], X[q:q + 1], m, jac=True)
        assert np.array_equal(_bits(F1[0]), _bits(got[None][0][q])) and np.array_equal(_bits(J1[0]), _bits(got[None][1][q]))
    assert (got[None][0][:, :][w[plist] == 0.0] == 0.0).all()       # a zero-weight row is exactly zero


# ------------------------------------------------------------------------------------------------ 5. fit + errors
def _fit_by_hand(ds, kind, K, B, dt, dy, dw, x0, m, analytic, o, lower=None, upper=None):
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy, dw)
    j = jac if analytic else None
    x = x0.clone()
    if lower is not None or upper is not None:
        fvec, ibs, st = ds.cls_solve_batch_device(fcn, ctx, m, x, jac=j, opts=o, lower=lower, upper=upper)
    else:
        fvec, ibs, st = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=j, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(fcn, ctx, m, x, jac=j, scaled=True)
    return x, fvec, sigma, cov, chi2, rank, ibs, st


def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("kind,K,B,m", [CC.CASES[0], CC.CASES[1], CC.CASES[4], CC.CASES[6]])
def test_fit_batch_is_the_composition(ds, kind, K, B, m, analytic, bounded):
    n = R.nparams(R.KINDS[kind], K, B)
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    lower = upper = None
    if bounded:
        lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
    o = ds.options(max_evals=CC.MAX_EVALS)
    keep = dx0.clone()
    got = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, lower=lower, upper=upper, analytic=analytic, opts=o)
    assert _eq(dx0, keep)
    want = _fit_by_hand(ds, kind, K, B, dt, dy, None, dx0, m, analytic, o, lower, upper)
    assert _eq(got[0], want[0]) and _eq(got[1], want[1]) and got[6] == want[6] and got[7] == want[7]
    ok = torch.tensor([s == 0 for s in got[7]], device=ds.device)
    assert bounded or bool(ok.all())                                # (a bounded solve may stop at its evaluation limit)
    for g, w_ in zip(got[2:6], want[2:6]):                          # sigma, cov, chi2, rank: the chain's where the solve ended with 0
        assert _eq(g[ok], w_[ok])
    bad = ~ok                                                       # ... NaN and rank -1 elsewhere
    assert bool(torch.isnan(got[2][bad]).all()) and bool(torch.isnan(got[3][bad]).all()) and bool(torch.isnan(got[4][bad]).all())
    assert bool((got[5][bad] == -1).all()) and bool((got[5][ok] == n).all()) and bool((got[2][ok] > 0).all())
    # without errors: the solve alone
    x2, f2, s2, c2, q2, r2, ib2, st2 = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, lower=lower, upper=upper,
                                                          analytic=analytic, covariance=False, opts=o)
    assert _eq(x2, want[0]) and _eq(f2, want[1]) and s2 is c2 is q2 is r2 is None and ib2 == want[6]
    # all weights given and none zero: the same rule, the same bits as the composition with those weights
    w = _dev(ds, _weights(np.random.default_rng(2), CC.NPROB, m, zeros=False))
    gw = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, weights=w, lower=lower, upper=upper, analytic=analytic, opts=o)
    ww = _fit_by_hand(ds, kind, K, B, dt, dy, w, dx0, m, analytic, o, lower, upper)
    okw = torch.tensor([s == 0 for s in gw[7]], device=ds.device)
    assert _eq(gw[0], ww[0]) and _eq(gw[1], ww[1]) and gw[7] == ww[7] and (bounded or bool(okw.all()))
    for g, w_ in zip(gw[2:6], ww[2:6]):
        assert _eq(g[okw], w_[okw])


def test_fit_batch_zero_weight_padding_and_dof(ds):
    """Ragged spectra padded with zero weights: dof = count(w != 0) - n; chi2 = sequential sum f^2 / dof bit for bit; every cov
    entry of the composition times (m - n) / dof once; a problem with dof <= 0 gets the status and NaNs, it alone."""
    kind, K, B, m, nprob = "gauss", 1, 0, 96, 40
    n = R.nparams(R.GAUSS, K, B)
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob, seed=5)
    rng = np.random.default_rng(8)
    w = np.ones((nprob, m))
    length = rng.integers(72, m + 1, nprob)                         # (the peak, at 0.35 .. 0.65, stays inside the data)
    length[3], length[17], length[nprob - 1] = n, n - 2, m          # dof 0, dof < 0, no padding
    for p in range(nprob):
        w[p, length[p]:] = 0.0
        y[p, length[p]:] = 1e3                                        # what lies under the padding does not matter
    dt, dy, dw, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, w), _dev(ds, x0)
    o = ds.options(max_evals=CC.MAX_EVALS)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, weights=dw, opts=o)
    bad = [3, 17]
    good = [p for p in range(nprob) if p not in bad]
    assert [st[p] for p in bad] == [NL_INVALID_INPUT_ERROR] * 2 and {st[p] for p in good} == {0}
    xh, fh, sh, ch, qh, rh = (v.cpu().numpy() for v in (x, fvec, sigma, cov, chi2, rank))
    for p in bad:
        assert np.isnan(sh[p]).all() and np.isnan(ch[p]).all() and np.isnan(qh[p]) and rh[p] == -1
        assert np.array_equal(_bits(xh[p]), _bits(x0[p])) and ibs[p]["fcn_count"] == 0     # nothing was evaluated for it
    # the composition by hand on the good problems (their own data: a problem's bits do not depend on its batch)
    gi = torch.tensor(good, device=ds.device)
    hand = _fit_by_hand(ds, kind, K, B, dt[gi].contiguous(), dy[gi].contiguous(), dw[gi].contiguous(), dx0[gi].contiguous(), m, True, o)
    hx, hf, hs, hc, hq, hr = (v.cpu().numpy() for v in hand[:6])
    for k, p in enumerate(good):
        dof = int(length[p]) - n
        assert np.array_equal(_bits(xh[p]), _bits(hx[k])) and np.array_equal(_bits(fh[p]), _bits(hf[k])) and rh[p] == hr[k] == n
        assert ibs[p] == hand[6][k]
        s = 0.0
        for v in fh[p]:
            s = s + v * v
        assert _bits(qh[p]) == _bits(s / float(dof)), (p, qh[p], s / dof)
        scale = float(m - n) / float(dof)
        wc = hc[k] * scale
        assert np.array_equal(_bits(ch[p]), _bits(wc)), p
        assert np.array_equal(_bits(sh[p]), _bits(np.sqrt(np.diag(wc)))), p
        assert (fh[p][length[p]:] == 0.0).all()
    assert np.array_equal(_bits(qh[nprob - 1]), _bits(hq[len(good) - 1]))       # no padding: the chain's own chi2


def test_fit_alone_and_inside_a_batch_of_300(ds):
    kind, K, B, m, nprob = "gauss", 1, -1, 64, 300
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob, seed=77)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=CC.MAX_EVALS)
    for form in (None, "row"):
        with _form(form):
            big = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, opts=o)
            assert set(big[7]) == {0}
            for p in (0, 137, nprob - 1):
                one = ds.curve_fit_batch(kind, dt[p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dx0[p:p + 1].contiguous(), ncomp=K,
                                         baseline=B, opts=o)
                for g, w_ in zip(one[:6], big[:6]):
                    assert _eq(g, w_[p:p + 1]), (form, p)
                assert one[6][0] == big[6][p]
    # (big: the forced row form) -- and the default form gave the same bits
    auto = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, opts=o)
    for g, w_ in zip(auto[:6], big[:6]):
        assert _eq(g, w_)
    # the host-array twin
    n = 3
    xh, fh = x0.copy(), np.zeros((nprob, m))
    sh, ch, qh, rh = np.zeros((nprob, n)), np.zeros((nprob, n, n)), np.zeros(nprob), np.zeros(nprob, dtype=np.int32)
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    rc = ds.lib.nlh_curve_fit_batch_h(ds.h.ptr, C.byref(o), R.GAUSS, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1,
                                      None, None, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), sh.ctypes.data_as(dp), ch.ctypes.data_as(dp),
                                      qh.ctypes.data_as(dp), rh.ctypes.data_as(_lib.c_int32_p), ib, st)
    assert rc == 0
    for g, w_ in zip((xh, fh, sh, ch, qh), auto[:5]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    assert np.array_equal(rh, auto[5].cpu().numpy()) and [ib[p].as_dict() for p in range(nprob)] == auto[6]


def test_error_returns(ds):
    t, y, xt, x0 = CC.curve_problems("gauss", 2, 1, 8, nprob=2)    # n = 8 = m
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    f = torch.full((2, 8), 7.0, dtype=torch.float64, device=ds.device)
    s = torch.full((2, 8), 7.0, dtype=torch.float64, device=ds.device)

    def fit(kind, K, B, m, sigma=None):
        return ds.lib.nlh_curve_fit_batch(ds.h.ptr, C.byref(o), kind, K, B, 2, m, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                          dx.data_ptr(), f.data_ptr(), sigma, None, None, None, None, None)
    assert fit(7, 2, 1, 8) == NL_INVALID_INPUT_ERROR and fit(0, 0, 1, 8) == NL_INVALID_INPUT_ERROR and fit(0, 2, 9, 30) == NL_INVALID_INPUT_ERROR
    assert fit(0, 2, 1, 7) == NL_UNDERDEFINED_PROBLEM_ERROR
    assert fit(0, 2, 1, 8, s.data_ptr()) == NL_INVALID_INPUT_ERROR   # errors asked for with m <= n
    torch.cuda.synchronize()
    assert (f == 7.0).all() and (s == 7.0).all() and torch.equal(dx, _dev(ds, x0))
    md = C.c_void_p()
    mk = lambda kind, K, B, m: ds.lib.nlh_curve_model_create(ds.h.ptr, kind, K, B, 2, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None,
                                                            1, C.byref(md))
    assert mk(3, 1, 0, 8) == NL_INVALID_INPUT_ERROR and mk(0, 2, 1, 7) == NL_UNDERDEFINED_PROBLEM_ERROR and not md.value
    assert ds.lib.nlh_curve_eval_batch(ds.h.ptr, 0, 2, -2, 2, 8, dt.data_ptr(), 0, dx.data_ptr(), f.data_ptr()) == NL_INVALID_INPUT_ERROR
    with pytest.raises(ValueError):
        ds.curve_fit_batch("gauss", dt, dy, dx, ncomp=3, baseline=1)
    # a context whose n does not match what the solver asks for aborts the solve with the library's error, launching nothing
    fcn, jac, ctx = ds.curve_launchers("gauss", 2, 1, dt, dy)
    with pytest.raises(RuntimeError):
        ds.lm_solve_batch_device(fcn, ctx, 8, dx[:, :7].contiguous())


# ------------------------------------------------------------------------------------------------ 6. eval, the model object
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("kind,K,B,m", CC.CASES)
def test_curve_eval(ds, kind, K, B, m, shared):
    kd, nprob = R.KINDS[kind], 9
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob)
    npts = 2 * m + 3                                                 # abscissae of the caller's choosing, not the data's
    tt = np.linspace(-0.1, 1.1, npts)[None] + np.zeros((nprob, 1)) if shared else np.sort(np.random.default_rng(4).uniform(-0.1, 1.1, (nprob, npts)))
    got = ds.curve_eval(kind, _dev(ds, x0), _dev(ds, tt[0] if shared else tt), ncomp=K, baseline=B).cpu().numpy()
    for p in range(nprob):
        want = R.model(kd, K, B, x0[p], tt[p])
        if kd == R.LORENTZ:
            assert np.array_equal(_bits(got[p]), _bits(want)), p
        else:
            bound = (K + 4) * U * R.abs_sum(kd, K, B, x0[p], tt[p], np.zeros(npts))
            assert (np.abs(got[p] - want) <= bound).all(), (p, (np.abs(got[p] - want) / bound).max())


@pytest.mark.parametrize("analytic", [0, 1])
def test_model_object_is_a_device_function_model(ds, analytic):
    """nlh_curve_model_create's model through _eval, _lm_solve, _cls_solve, _lm_covariance = the launcher forms."""
    kind, K, B, m, nprob = "expdecay", 2, 0, 400, 12
    n = R.nparams(R.EXPDECAY, K, B)
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob)
    w = _weights(np.random.default_rng(6), nprob, m)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy, dw)
    j = jac if analytic else None
    o = ds.options(max_evals=CC.MAX_EVALS)
    md = C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.EXPDECAY, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp),
                                         w.ctypes.data_as(dp), analytic, C.byref(md)) == 0
    try:
        sp, sm, sn = C.c_int32(), C.c_int32(), C.c_int32()
        ds.lib.nlh_dq_model_shape(md, C.byref(sp), C.byref(sm), C.byref(sn))
        assert (sp.value, sm.value, sn.value) == (nprob, m, n)
        f0 = np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_eval(ds.h.ptr, md, x0.ctypes.data_as(dp), f0.ctypes.data_as(dp)) == 0
        assert np.array_equal(_bits(f0), _bits(_launch(ds, fcn, ctx, list(range(nprob)), x0, m)))
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        xh, fh = x0.copy(), np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_lm_solve(ds.h.ptr, C.byref(o), md, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, x0)
        fvec, ibs, status = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=j, opts=o)
        assert np.array_equal(_bits(xh), _bits(x.cpu().numpy())) and np.array_equal(_bits(fh), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(nprob)] == ibs and list(st) == status == [0] * nprob
        ch, sh, rh, qh = np.zeros((nprob, n, n)), np.zeros((nprob, n)), np.zeros(nprob, dtype=np.int32), np.zeros(nprob)
        assert ds.lib.nlh_dq_model_lm_covariance(ds.h.ptr, md, xh.ctypes.data_as(dp), 1, 0.0, ch.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                                 rh.ctypes.data_as(_lib.c_int32_p), qh.ctypes.data_as(dp)) == 0
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(fcn, ctx, m, x, jac=j)
        assert np.array_equal(_bits(ch), _bits(cov.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sigma.cpu().numpy()))
        assert np.array_equal(rh, rank.cpu().numpy()) and np.array_equal(_bits(qh), _bits(chi2.cpu().numpy()))
        lo, hi = xt.min(0) - 0.5, xt.max(0) + 0.5
        xc, fc = x0.copy(), np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_cls_solve(ds.h.ptr, C.byref(o), md, 1.0, 1.0, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp),
                                             xc.ctypes.data_as(dp), fc.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, x0)
        fvec, ibs, status = ds.cls_solve_batch_device(fcn, ctx, m, x, jac=j, opts=o, lower=lo, upper=hi)
        assert np.array_equal(_bits(xc), _bits(x.cpu().numpy())) and np.array_equal(_bits(fc), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(nprob)] == ibs and list(st) == status
    finally:
        ds.lib.nlh_dq_model_destroy(md)


# ------------------------------------------------------------------------------------------------ 7. Fortran
@pytest.fixture(scope="module")
def fortran_curve_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_curve")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "curve_fit")


def test_fortran_curve_fit(ds, fortran_curve_exe, tmp_path):
    """The Fortran user program's printed x, sigma and counts equal Python's for the same inputs, digit for digit (ES24.16)."""
    kind, K, B, m, nprob = "gauss", 2, 0, 120, 6
    n = R.nparams(R.GAUSS, K, B)
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob, seed=31)
    path = str(tmp_path / "curves.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m, K, B], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(x0.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_curve_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    o = ds.options(max_evals=CC.MAX_EVALS)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch(kind, _dev(ds, t), _dev(ds, y), _dev(ds, x0), ncomp=K, baseline=B, opts=o)
    xh, sh = x.cpu().numpy(), sigma.cpu().numpy()
    want = []
    for p in range(nprob):
        want.append("x %d" % (p + 1) + "".join("%24.16E" % v for v in xh[p]))
        want.append("sigma %d" % (p + 1) + "".join("%24.16E" % v for v in sh[p]))
        want.append("counts %d %d %d %d %d" % (p + 1, ibs[p]["iter_count"], ibs[p]["fcn_count"], ibs[p]["jacobian_count"], int(rank[p])))
    lines = [" ".join(ln.split()) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1] == "done"
    assert lines[:-1] == [" ".join(w_.split()) for w_ in want], out.stdout
