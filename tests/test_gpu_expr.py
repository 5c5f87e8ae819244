"""GPU tests of the formula models (include/nonlin_hip.h: nlh_expr_*): the interpreter kernels bit for bit against the numpy
restatement where the formula has no library function and within the restatement's running bound where it has; both
workgroup forms, every launch shape and chunk of Jacobian columns; the header-order Lorentzian and Gaussian against the
built-in curve models; solves bit for bit against the CPU oracle; recovery of generating parameters; nlh_expr_fit_batch
as the composition it stands for; the model object; the Fortran surface; and the measured accuracy of the device
library's functions, which the bound's table U_F rests on."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import curve_cases as CC
import expr_cases as EC
import expr_restatement as R
from nonlin_amd import _lib
import nonlin_amd as nl

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
# (NLH_EXPR_FORM, NLH_EXPR_CHUNK): the form m selects and the chunk the depth selects; each form forced (one that cannot hold
# m falls back); one Jacobian column per pass
VARIANTS = [(None, None), ("row", None), ("flat", None), (None, "1")]
U = 2.0 ** -52
NL_INVALID_INPUT_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR = 201, 212
LORENTZ_HEADER = "0+a/(1.0+((t-mu)/w)*((t-mu)/w))+(c1*t+c0)"            # K = 1, B = 1 in the header's operation order
GAUSS_HEADER = "0+a*exp(-0.5*(((t-mu)/s)*((t-mu)/s)))+(c1*t+c0)"
HEADER = {"lorentz": (LORENTZ_HEADER, "a,mu,w,c0,c1"), "gauss": (GAUSS_HEADER, "a,mu,s,c0,c1")}


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _record(line):
    """Print a measured figure; append it to the file NLH_EXPR_RATE_FILE names, when it names one (profiles/expr_rate.txt)."""
    print(line)
    path = os.environ.get("NLH_EXPR_RATE_FILE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


class _variant:
    """NLH_EXPR_FORM and NLH_EXPR_CHUNK for the calls inside (the library reads them at every call)."""

    def __init__(self, form, chunk=None):
        self.want = {"NLH_EXPR_FORM": form, "NLH_EXPR_CHUNK": chunk}

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.want}
        for k, v in self.want.items():
            if v is not None:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


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
    """Launch shapes (the point lists of tests/test_gpu_curve.py): one point, n + 1 points of one problem, a mixed list."""
    rng = np.random.default_rng(3)
    return [[nprob - 2], [2] * (n + 1), list(rng.integers(0, nprob, 37)) + [0, 0, nprob - 1]]


def _points(x0, plist, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(x0[plist] * (1.0 + 0.01 * rng.uniform(-1, 1, (len(plist), x0.shape[1]))))


def _m_of(name, m):
    return {64: 64, 200: 196, 256: 256, 301: 289}[m] if name == "gauss2d" else m     # (two variables: a square of pixels)


# ------------------------------------------------------------------------------------------------ 1. kernels, exp-free
@pytest.mark.parametrize("m", [64, 200, 256, 301])
@pytest.mark.parametrize("weighted,shared", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", EC.EXP_FREE)
def test_exp_free_kernels_bitwise(ds, name, weighted, shared, m):
    nprob = 5
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, seed=11 + m, prog=e.program())
    n = x0.shape[1]
    if shared:
        t = np.ascontiguousarray(np.broadcast_to(t[:, :1], t.shape))
    w = _weights(np.random.default_rng(m), nprob, m) if weighted else None
    dt, dy, dw = _dev(ds, t[:, 0] if shared else t), _dev(ds, y), (_dev(ds, w) if weighted else None)
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy, dw)
    for k, plist in enumerate(_shapes(nprob, n)):
        X = _points(x0, plist, k)
        wantF = [R.residual(prog, X[q], t[:, p], y[p], w[p] if weighted else None) for q, p in enumerate(plist)]
        wantJ = [R.jacobian(prog, X[q], t[:, p], w[p] if weighted else None).T for q, p in enumerate(plist)]
        for form, chunk in VARIANTS:
            with _variant(form, chunk):
                F = _launch(ds, fcn, ctx, plist, X, m)
                J = _launch(ds, jac, ctx, plist, X, m, jac=True)
            for q in range(len(plist)):
                assert np.array_equal(_bits(F[q]), _bits(wantF[q])), (name, form, chunk, k, q)
                assert np.array_equal(_bits(J[q]), _bits(wantJ[q])), (name, form, chunk, k, q)


@pytest.mark.parametrize("m", [64, 200])
@pytest.mark.parametrize("name", list(EC.FORMULAS))
def test_forms_shapes_and_a_point_alone_same_bits(ds, name, m):
    """A row's bits do not depend on the form, the chunk of columns, or the launch it sits in -- library functions or not."""
    m, nprob = _m_of(name, m), 8
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, prog=e.program())
    n = x0.shape[1]
    w = _weights(np.random.default_rng(1), nprob, m)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy, dw)
    plist = _shapes(nprob, n)[2]
    X = _points(x0, plist, 9)
    got = {}
    for v in VARIANTS:
        with _variant(*v):
            got[v] = (_launch(ds, fcn, ctx, plist, X, m), _launch(ds, jac, ctx, plist, X, m, jac=True))
    base = got[VARIANTS[0]]
    assert np.isfinite(base[0]).all() and np.isfinite(base[1]).all()
    for v in VARIANTS[1:]:
        assert np.array_equal(_bits(got[v][0]), _bits(base[0])) and np.array_equal(_bits(got[v][1]), _bits(base[1])), (name, v)
    for q in (0, 17, len(plist) - 1):                               # ... and a point alone
        F1 = _launch(ds, fcn, ctx, plist[q:q + 1], X[q:q + 1], m)
        J1 = _launch(ds, jac, ctx, plist[q:q + 1], X[q:q + 1], m, jac=True)
        assert np.array_equal(_bits(F1[0]), _bits(base[0][q])) and np.array_equal(_bits(J1[0]), _bits(base[1][q]))
    zero = w[plist] == 0.0                                          # a zero-weight row is exactly zero
    assert (base[0][zero] == 0.0).all() and (np.transpose(base[1], (0, 2, 1))[zero] == 0.0).all()


# ------------------------------------------------------------------------------------------------ 2. the built-ins
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", ["lorentz", "gauss"])
def test_header_order_formula_gives_the_builtin_bits(ds, kind, weighted):
    """The curve models' stated order written as a formula: the same residual bits on the device (the same device exp), so
    with forward differences the whole fit is the built-in fit bit for bit."""
    m, nprob = 301, 64
    e = nl.Expr(HEADER[kind][0], "t", HEADER[kind][1])
    t, y, xt, x0 = CC.curve_problems(kind, 1, 1, m, nprob=nprob)
    w = _weights(np.random.default_rng(4), nprob, m) if weighted else None
    dt, dy, dw = _dev(ds, t), _dev(ds, y), (_dev(ds, w) if weighted else None)
    fe, je, ce = ds.expr_launchers(e, dt, dy, dw)
    fc, jc, cc = ds.curve_launchers(kind, 1, 1, dt, dy, dw)
    plist = list(range(nprob))
    for form in (None, "row", "flat"):
        with _variant(form):
            Fe = _launch(ds, fe, ce, plist, x0, m)
        assert np.array_equal(_bits(Fe), _bits(_launch(ds, fc, cc, plist, x0, m))), (kind, form)
    o = ds.options(max_evals=CC.MAX_EVALS)
    xe, xc = _dev(ds, x0), _dev(ds, x0)
    fve, ibe, ste = ds.lm_solve_batch_device(fe, ce, m, xe, opts=o)
    fvc, ibc, stc = ds.lm_solve_batch_device(fc, cc, m, xc, opts=o)
    torch.cuda.synchronize()
    assert torch.equal(xe.view(torch.int64), xc.view(torch.int64)) and torch.equal(fve.view(torch.int64), fvc.view(torch.int64))
    assert ibe == ibc and ste == stc and set(ste) == {0}


# ------------------------------------------------------------------------------------------------ 3. solves, the oracle
@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("name,m", EC.SOLVE_CASES)
def test_solves_against_oracle(ds, oracle, name, m, analytic, bounded):
    """The parity rule of every user family: the device's solve is the CPU oracle's with the restatement as callback, bit for
    bit in x, fvec, counts and flags, for every problem of the batch."""
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, prog=e.program())
    n = x0.shape[1]
    opt = dict(max_evals=EC.MAX_EVALS)
    lower = upper = None
    if bounded:                                 # a box some true values lie outside of: bounds that bind
        lower, upper = np.minimum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) - 0.02, np.maximum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) + 0.02
        x0 = np.clip(x0, lower, upper)
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy)
    x = _dev(ds, x0)
    if bounded:
        fvec, ibs, status = ds.cls_solve_batch_device(fcn, ctx, m, x, jac=jac if analytic else None, opts=ds.options(**opt),
                                                      lower=lower, upper=upper)
    else:
        fvec, ibs, status = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=jac if analytic else None, opts=ds.options(**opt))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**opt)
    for p in range(EC.NPROB):
        tv = t[:, p]
        f = lambda xx, ff: ff.__setitem__(slice(None), R.residual(prog, xx, tv, y[p]))
        j = (lambda xx, JJ: JJ.__setitem__((slice(None), slice(None)), R.jacobian(prog, xx, tv))) if analytic else None
        if bounded:
            rc, xo, fo, ibo = oracle.cls_solve(f, m, n, x0[p], jac=j, opts=oo, lower=lower, upper=upper)
        else:
            rc, xo, fo, ibo = oracle.lm_solve(f, m, n, x0[p], jac=j, opts=oo)
        what = (name, m, analytic, bounded, p)
        assert status[p] == rc, (what, status[p], rc)
        assert _same(ibs[p], ibo), (what, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), what
    if not bounded:
        assert set(status) == {0}, (name, m, sorted(set(status)))


# ------------------------------------------------------------------------------------------------ 4. library functions
def _ulps(got, ref):
    """|got - ref| in units of the float64 spacing at ref (ref: numpy.longdouble)."""
    r64 = np.abs(ref).astype(np.float64)
    return float((np.abs(got.astype(np.longdouble) - ref) / np.spacing(r64).astype(np.longdouble)).max())


def test_function_accuracy(ds):
    """The error of the device library's exp log sin cos tanh atan pow in ulp, through nlh_expr_eval_batch against
    numpy.longdouble over expr_cases.ACCURACY_RANGES.  The restatement's table U_F is this maximum rounded up to an
    integer: the table must cover what is measured here."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is no wider than float64 here: nothing to measure against"
    rng = np.random.default_rng(12)
    npts = 1 << 18
    ld = {"exp": np.exp, "log": np.log, "sin": np.sin, "cos": np.cos, "tanh": np.tanh, "atan": np.arctan}
    zero = _dev(ds, np.zeros((1, 1)))
    measured = {}
    for f, (lo, hi) in EC.ACCURACY_RANGES.items():
        t = rng.uniform(lo, hi, npts)
        if f == "log" or f == "pow":
            t = np.exp(rng.uniform(math.log(lo), math.log(hi), npts))
        worst = 0.0
        for c in (EC.POW_EXPONENTS if f == "pow" else (None,)):
            e = nl.Expr(f"t^{c!r}+a" if f == "pow" else f"{f}(t)+a", "t", "a")       # a = 0: v + 0 is v
            got = ds.expr_eval(e, zero, _dev(ds, t)).cpu().numpy()[0]
            tl = t.astype(np.longdouble)
            ref = np.power(tl, np.longdouble(c)) if f == "pow" else ld[f](tl)
            worst = max(worst, _ulps(got, ref))
        measured[f] = worst
        _record(f"expr function accuracy {f}: {worst:.3f} ulp over [{lo}, {hi}] (table {R.U_F[f]})")
    for f, worst in measured.items():
        assert math.ceil(worst) <= R.U_F[f], (f, worst, R.U_F[f])


@pytest.mark.parametrize("name", EC.WITH_FUNCTIONS)
def test_formulas_with_functions_within_running_bound(ds, name):
    """|device - numpy| <= the restatement's first-order running bound, residual and Jacobian, entry by entry (where the bound
    is 0 -- a structural zero, an entry no library function reaches -- that is bit equality)."""
    nprob = 8
    e = EC.compile_formula(name)
    rf = rj = 0.0
    for m in (_m_of(name, 64), _m_of(name, 301)):
        prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, prog=e.program())
        n = x0.shape[1]
        w = _weights(np.random.default_rng(2), nprob, m)
        dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
        for wd, wh in ((None, None), (dw, w)):
            fcn, jac, ctx = ds.expr_launchers(e, dt, dy, wd)
            for k, plist in enumerate(_shapes(nprob, n)):
                X = _points(x0, plist, 20 + k)
                F = _launch(ds, fcn, ctx, plist, X, m)
                J = _launch(ds, jac, ctx, plist, X, m, jac=True)
                for q, p in enumerate(plist):
                    wp = wh[p] if wh is not None else None
                    want, bound = R.residual_bound(prog, X[q], t[:, p], y[p], wp)
                    err = np.abs(F[q] - want)
                    assert (err <= bound).all(), (name, m, k, q, float((err[bound > 0] / bound[bound > 0]).max()))
                    rf = max(rf, float((err[bound > 0] / bound[bound > 0]).max()))
                    wj, bj = R.jacobian_bound(prog, X[q], t[:, p], wp)
                    ej = np.abs(J[q].T - wj)
                    assert (ej <= bj).all(), (name, m, k, q, "jacobian", float((ej[bj > 0] / bj[bj > 0]).max()))
                    rj = max(rj, float((ej[bj > 0] / bj[bj > 0]).max()))
    _record(f"expr running-bound ratio {name}: residual {rf:.3f} jacobian {rj:.3f}")


# ------------------------------------------------------------------------------------------------ 5. recovery
@pytest.mark.parametrize("name,m,nprob", [("gauss2d", 225, 256), ("dsine", 200, 64)])
def test_recovers_the_generating_parameters(ds, name, m, nprob):
    """Noise-free data: every parameter of every problem to 1e-8 of its generating value; sigma finite, rank = n."""
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, seed=7, sigma=0.0, prog=e.program())
    n = x0.shape[1]
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.expr_fit_batch(e, _dev(ds, t), _dev(ds, y), _dev(ds, x0), opts=ds.options(max_evals=EC.MAX_EVALS))
    assert set(st) == {0}
    rel = np.abs(x.cpu().numpy() - xt) / np.abs(xt)
    print(f"expr recovery {name}: largest relative error {rel.max():.3e}")
    assert (rel <= 1e-8).all(), (name, rel.max())
    assert bool(torch.isfinite(sigma).all()) and bool((rank == n).all())


# ------------------------------------------------------------------------------------------------ 6. fit + errors
def _fit_by_hand(ds, e, dt, dy, dw, x0, m, analytic, o, lower=None, upper=None):
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy, dw)
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
@pytest.mark.parametrize("name,m", [("mm", 64), ("rational", 256), ("gauss2d", 225), ("dsine", 200)])
def test_fit_batch_is_the_composition(ds, name, m, analytic, bounded):
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, prog=e.program())
    n = x0.shape[1]
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    lower = upper = None
    if bounded:
        lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
    o = ds.options(max_evals=EC.MAX_EVALS)
    keep = dx0.clone()
    got = ds.expr_fit_batch(e, dt, dy, dx0, lower=lower, upper=upper, analytic=analytic, opts=o)
    assert _eq(dx0, keep)
    want = _fit_by_hand(ds, e, dt, dy, None, dx0, m, analytic, o, lower, upper)
    assert _eq(got[0], want[0]) and _eq(got[1], want[1]) and got[6] == want[6] and got[7] == want[7]
    ok = torch.tensor([s == 0 for s in got[7]], device=ds.device)
    assert bounded or bool(ok.all())                                # (a bounded solve may stop at its evaluation limit)
    for g, w_ in zip(got[2:6], want[2:6]):                          # sigma, cov, chi2, rank: the chain's where the solve ended with 0
        assert _eq(g[ok], w_[ok])
    bad = ~ok                                                       # ... NaN and rank -1 elsewhere
    assert bool(torch.isnan(got[2][bad]).all()) and bool(torch.isnan(got[3][bad]).all()) and bool(torch.isnan(got[4][bad]).all())
    assert bool((got[5][bad] == -1).all()) and bool((got[5][ok] == n).all()) and bool((got[2][ok] > 0).all())
    # without errors: the solve alone
    x2, f2, s2, c2, q2, r2, ib2, st2 = ds.expr_fit_batch(e, dt, dy, dx0, lower=lower, upper=upper, analytic=analytic, covariance=False, opts=o)
    assert _eq(x2, want[0]) and _eq(f2, want[1]) and s2 is c2 is q2 is r2 is None and ib2 == want[6]
    # all weights given and none zero: the same rule, the same bits as the composition with those weights
    w = _dev(ds, _weights(np.random.default_rng(2), EC.NPROB, m, zeros=False))
    gw = ds.expr_fit_batch(e, dt, dy, dx0, weights=w, lower=lower, upper=upper, analytic=analytic, opts=o)
    ww = _fit_by_hand(ds, e, dt, dy, w, dx0, m, analytic, o, lower, upper)
    okw = torch.tensor([s == 0 for s in gw[7]], device=ds.device)
    assert _eq(gw[0], ww[0]) and _eq(gw[1], ww[1]) and gw[7] == ww[7] and (bounded or bool(okw.all()))
    for g, w_ in zip(gw[2:6], ww[2:6]):
        assert _eq(g[okw], w_[okw])


def test_fit_batch_zero_weight_padding_and_dof(ds):
    """Ragged data padded with zero weights: dof = count(w != 0) - n; chi2 = sequential sum f^2 / dof bit for bit; every cov
    entry of the composition times (m - n) / dof once; a problem with dof <= 0 gets the status and NaNs, it alone."""
    name, m, nprob = "logistic", 96, 40
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, seed=5, prog=e.program())
    n = x0.shape[1]
    rng = np.random.default_rng(8)
    w = np.ones((nprob, m))
    length = rng.integers(80, m + 1, nprob)                         # (the rise, at t0 = 4 .. 6 of 0 .. 10, stays inside the data)
    length[3], length[17], length[nprob - 1] = n, n - 2, m          # dof 0, dof < 0, no padding
    for p in range(nprob):
        w[p, length[p]:] = 0.0
        y[p, length[p]:] = 1e3                                        # what lies under the padding does not matter
    dt, dy, dw, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, w), _dev(ds, x0)
    o = ds.options(max_evals=EC.MAX_EVALS)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.expr_fit_batch(e, dt, dy, dx0, weights=dw, opts=o)
    bad = [3, 17]
    good = [p for p in range(nprob) if p not in bad]
    assert [st[p] for p in bad] == [NL_INVALID_INPUT_ERROR] * 2 and {st[p] for p in good} == {0}
    xh, fh, sh, ch, qh, rh = (v.cpu().numpy() for v in (x, fvec, sigma, cov, chi2, rank))
    for p in bad:
        assert np.isnan(sh[p]).all() and np.isnan(ch[p]).all() and np.isnan(qh[p]) and rh[p] == -1
        assert np.array_equal(_bits(xh[p]), _bits(x0[p])) and ibs[p]["fcn_count"] == 0     # nothing was evaluated for it
    # the composition by hand on the good problems (their own data: a problem's bits do not depend on its batch)
    gi = torch.tensor(good, device=ds.device)
    hand = _fit_by_hand(ds, e, dt[:, gi].contiguous(), dy[gi].contiguous(), dw[gi].contiguous(), dx0[gi].contiguous(), m, True, o)
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
    name, m, nprob = "gauss2d", 64, 300
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, seed=77, prog=e.program())
    n = x0.shape[1]
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=EC.MAX_EVALS)
    for form in (None, "row"):
        with _variant(form):
            big = ds.expr_fit_batch(e, dt, dy, dx0, opts=o)
            assert set(big[7]) == {0}
            for p in (0, 137, nprob - 1):
                one = ds.expr_fit_batch(e, dt[:, p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dx0[p:p + 1].contiguous(), opts=o)
                for g, w_ in zip(one[:6], big[:6]):
                    assert _eq(g, w_[p:p + 1]), (form, p)
                assert one[6][0] == big[6][p]
    # (big: the forced row form) -- and the default form gave the same bits
    auto = ds.expr_fit_batch(e, dt, dy, dx0, opts=o)
    for g, w_ in zip(auto[:6], big[:6]):
        assert _eq(g, w_)
    # the host-array twin
    xh, fh = x0.copy(), np.zeros((nprob, m))
    sh, ch, qh, rh = np.zeros((nprob, n)), np.zeros((nprob, n, n)), np.zeros(nprob), np.zeros(nprob, dtype=np.int32)
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    rc = ds.lib.nlh_expr_fit_batch_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1,
                                     None, None, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), sh.ctypes.data_as(dp), ch.ctypes.data_as(dp),
                                     qh.ctypes.data_as(dp), rh.ctypes.data_as(_lib.c_int32_p), ib, st)
    assert rc == 0
    for g, w_ in zip((xh, fh, sh, ch, qh), auto[:5]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    assert np.array_equal(rh, auto[5].cpu().numpy()) and [ib[p].as_dict() for p in range(nprob)] == auto[6]


def test_error_returns(ds):
    e = EC.compile_formula("rational")                              # n = 5
    prog, t, y, xt, x0 = EC.expr_problems("rational", 5, nprob=2, prog=e.program())      # m = n
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    f = torch.full((2, 5), 7.0, dtype=torch.float64, device=ds.device)
    s = torch.full((2, 5), 7.0, dtype=torch.float64, device=ds.device)

    def fit(ex, nprob, m, sigma=None, y_=dy):
        return ds.lib.nlh_expr_fit_batch(ds.h.ptr, C.byref(o), ex, nprob, m, dt.data_ptr(), 0, y_.data_ptr() if y_ is not None else None, None,
                                         1, None, None, dx.data_ptr(), f.data_ptr(), sigma, None, None, None, None, None)
    assert fit(None, 2, 5) == NL_INVALID_INPUT_ERROR and fit(e.ptr, -1, 5) == NL_INVALID_INPUT_ERROR and fit(e.ptr, 2, 0) == NL_INVALID_INPUT_ERROR
    assert fit(e.ptr, 2, 5, y_=None) == NL_INVALID_INPUT_ERROR
    assert fit(e.ptr, 2, 4) == NL_UNDERDEFINED_PROBLEM_ERROR
    assert fit(e.ptr, 2, 5, s.data_ptr()) == NL_INVALID_INPUT_ERROR  # errors asked for with m <= n
    torch.cuda.synchronize()
    assert (f == 7.0).all() and (s == 7.0).all() and torch.equal(dx, _dev(ds, x0))
    md = C.c_void_p()
    mk = lambda ex, m: ds.lib.nlh_expr_model_create(ds.h.ptr, ex, 2, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1, C.byref(md))
    assert mk(None, 5) == NL_INVALID_INPUT_ERROR and mk(e.ptr, 4) == NL_UNDERDEFINED_PROBLEM_ERROR and not md.value
    assert ds.lib.nlh_expr_eval_batch(ds.h.ptr, None, 2, 5, dt.data_ptr(), 0, dx.data_ptr(), f.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_expr_eval_batch(ds.h.ptr, e.ptr, 2, 5, None, 0, dx.data_ptr(), f.data_ptr()) == NL_INVALID_INPUT_ERROR
    with pytest.raises(ValueError):
        ds.expr_fit_batch(e, dt, dy, dx[:, :4].contiguous())
    with pytest.raises(ValueError):
        ds.expr_eval(e, dx[:, :4].contiguous(), dt)
    # a context whose n does not match what the solver asks for aborts the solve with the library's error, launching nothing
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy)
    with pytest.raises(RuntimeError):
        ds.lm_solve_batch_device(fcn, ctx, 5, dx[:, :4].contiguous())


# ------------------------------------------------------------------------------------------------ 7. eval, the model object
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("name", ["rational", "roots", "gauss2d", "stretched"])
def test_expr_eval(ds, name, shared):
    nprob, npts = 9, 2 * 200 + 3                                    # abscissae of the caller's choosing, not the data's
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, 225 if name == "gauss2d" else 200, nprob=nprob, prog=e.program())
    lo, hi = EC.FORMULAS[name][3]
    rng = np.random.default_rng(4)
    tt = np.sort(rng.uniform(lo, hi, (e.nvar, nprob, npts)), axis=-1)
    if shared:
        tt = np.ascontiguousarray(np.broadcast_to(tt[:, :1], tt.shape))
    got = ds.expr_eval(e, _dev(ds, x0), _dev(ds, tt[:, 0] if shared else tt)).cpu().numpy()
    for p in range(nprob):
        want, bound = R.residual_bound(prog, x0[p], tt[:, p], np.zeros(npts))
        assert (np.abs(got[p] - want) <= bound).all(), (name, p)
        if name in EC.EXP_FREE:
            assert np.array_equal(_bits(got[p]), _bits(R.value(prog, x0[p], tt[:, p]))), (name, p)
    if e.nvar == 1:                                                  # one variable: [nprob, npts] / [npts] will do for t
        again = ds.expr_eval(e, _dev(ds, x0), _dev(ds, tt[0, 0] if shared else tt[0])).cpu().numpy()
        assert np.array_equal(_bits(again), _bits(got))


@pytest.mark.parametrize("analytic", [0, 1])
def test_model_object_is_a_device_function_model(ds, analytic):
    """nlh_expr_model_create's model through _eval, _lm_solve, _cls_solve, _lm_covariance = the launcher forms; the model
    keeps its own copy of the program."""
    name, m, nprob = "gauss2d", 225, 12
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, prog=e.program())
    n = x0.shape[1]
    w = _weights(np.random.default_rng(6), nprob, m)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy, dw)
    j = jac if analytic else None
    o = ds.options(max_evals=EC.MAX_EVALS)
    md = C.c_void_p()
    mine = EC.compile_formula(name)
    assert ds.lib.nlh_expr_model_create(ds.h.ptr, mine.ptr, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp),
                                        w.ctypes.data_as(dp), analytic, C.byref(md)) == 0
    mine.close()                                                     # the caller's expression may go at once
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


# ------------------------------------------------------------------------------------------------ 8. Fortran
@pytest.fixture(scope="module")
def fortran_expr_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_expr")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "expr_fit")


def test_fortran_expr_fit(ds, fortran_expr_exe, tmp_path):
    """The Fortran user program's printed x, sigma and counts equal Python's for the same inputs, digit for digit (ES24.16)."""
    name, m, nprob = "gauss2d", 225, 6
    e = nl.Expr("b + a*exp(-((x-x0)^2 + (y-y0)^2)/(2*s^2))", "x,y", "a,x0,y0,s,b")      # the program's own string
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, seed=31, prog=e.program())
    n = x0.shape[1]
    path = str(tmp_path / "spots.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m, 2, n], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(x0.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_expr_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    o = ds.options(max_evals=EC.MAX_EVALS)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.expr_fit_batch(e, _dev(ds, t), _dev(ds, y), _dev(ds, x0), opts=o)
    xh, sh = x.cpu().numpy(), sigma.cpu().numpy()
    want = []
    for p in range(nprob):
        want.append("x %d" % (p + 1) + "".join("%24.16E" % v for v in xh[p]))
        want.append("sigma %d" % (p + 1) + "".join("%24.16E" % v for v in sh[p]))
        want.append("counts %d %d %d %d %d" % (p + 1, ibs[p]["iter_count"], ibs[p]["fcn_count"], ibs[p]["jacobian_count"], int(rank[p])))
    lines = [" ".join(ln.split()) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1] == "done"
    assert lines[:-1] == [" ".join(w_.split()) for w_ in want], out.stdout
