"""GPU tests of the separable fits (include/nonlin_hip.h: nlh_sep_*), everything bit for bit: the QR-and-solve and the
projection kernels against the numpy restatement (tests/sep_restatement.py) in both workgroup forms, for every launch shape,
with and without weights, sliced and unsliced, a dead column included; the residual the solver sees against the inner
launcher at the solved parameters; solves through the wrapping launchers against the CPU oracle over the restatement; the
one-call fits as the composition they stand for (plain, with an instrument response, with zero-weight padding, the host
twin, a problem alone against a batch of 300); the error returns; sep_check.  The Lorentzian and an exp-free formula are restated from their parameters; for the widest basis
(L = 32, through a parameter map) and the exp kind the restatement is fed the device's own Phi, f0 and D, so the comparison
of the kernels is bit for bit there too."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import curve_restatement as R
import expr_restatement as XR
import sep_cases as SC
import sep_restatement as SR
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR = 201, 211
FORMS = ("lds", "global")
LOR1 = "a/(1+(t*k)^2)"                        # L = 1, n = 1
LOR4 = "a/(1+((t-mu)/w)^2) + c"               # L = 2, n = 2


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


class _env:
    """Environment variables for the calls inside (the library reads NLH_SEP_* at every call); None: unset."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.kw}
        for k, v in self.kw.items():
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _dev(ds, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ds.device)


def _launch(ds, fcn, ctx, plist, X, m, jac=False, expect=0):
    """One call of a launcher on the points X (numpy [npoints, n]) of the problems plist (None: no dprob): F [npoints, m] or
    J [npoints, n, m]."""
    npts, n = X.shape
    dX = _dev(ds, X)
    dprob = _dev(ds, plist, np.int32) if plist is not None else None
    out = torch.full((npts, n, m) if jac else (npts, m), np.nan, dtype=torch.float64, device=ds.device)
    stream = torch.cuda.current_stream(ds.device).cuda_stream
    rc = fcn(ds._ctxp(ctx), C.c_void_p(stream), npts, C.c_void_p(dprob.data_ptr()) if dprob is not None else None, n,
             C.c_void_p(dX.data_ptr()), m, C.c_void_p(out.data_ptr()))
    assert rc == expect, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _weights(rng, nprob, m, N):
    """Weights with zero rows: the last rows of every problem, and a few inside (never fewer than N + 2 rows left)."""
    w = rng.uniform(0.5, 2.0, (nprob, m))
    spare = m - (N + 2)
    for p in range(nprob):
        z = min(spare, 1 + p)
        if z > 0:
            w[p, m - z:] = 0.0
        if spare > 8:
            w[p, rng.integers(0, m - z, 3)] = 0.0
    return w


def _expected(evalF, evalJ, N, lin, X, rows):
    """The restatement on the points X of the problems `rows`: evalF(P, rows) -> [npts, m], evalJ(P, rows) -> [npts, N, m]
    are the inner model at full parameters P [npts, N].  Returns (P^ [npts, N], rank [npts], F [npts, m], J [npts, n, m])."""
    lin, nln = SR.tables(N, lin)
    P0 = np.zeros((len(X), N))
    P0[:, nln] = X
    J0, F0 = evalJ(P0, rows), evalF(P0, rows)
    qr = [SR.qr_solve(J0[q][lin].T, F0[q]) for q in range(len(X))]
    PH = P0.copy()
    PH[:, lin] = np.stack([c[0] for c in qr])
    F, JH = evalF(PH, rows), evalJ(PH, rows)
    J = np.stack([SR.project(qr[q][2], qr[q][3], qr[q][4], JH[q][nln].T).T for q in range(len(X))])
    return PH, np.array([c[1] for c in qr]), F, J


def _lorentz_eval(K, B, t, y, w):
    def F(P, rows):
        return np.stack([R.residual(R.LORENTZ, K, B, P[q], t[p], y[p], None if w is None else w[p]) for q, p in enumerate(rows)])

    def J(P, rows):
        return np.stack([R.jacobian(R.LORENTZ, K, B, P[q], t[p], None if w is None else w[p]).T for q, p in enumerate(rows)])
    return F, J


def _expr_eval(prog, t, y, w):
    def F(P, rows):
        return np.stack([XR.residual(prog, P[q], [t[p]], y[p], None if w is None else w[p]) for q, p in enumerate(rows)])

    def J(P, rows):
        return np.stack([XR.jacobian(prog, P[q], [t[p]], None if w is None else w[p]).T for q, p in enumerate(rows)])
    return F, J


def _device_eval(ds, fcn, jac, ctx, m):
    """The inner model as the device's own launchers evaluate it."""
    def F(P, rows):
        return _launch(ds, fcn, ctx, list(rows), P, m)

    def J(P, rows):
        return _launch(ds, jac, ctx, list(rows), P, m, jac=True)
    return F, J


def _shapes(nprob, n, rng, mixed):
    """One point; n + 1 points of one problem; a mixed list; no list at all."""
    return [[nprob - 2], [2] * (n + 1), list(rng.integers(0, nprob, mixed)) + [0, 0, nprob - 1], None]


def _check_calls(ds, sp, inner, evals, N, lin, m, x_nl, nprob, mixed, what, jitter=0.01):
    """Every launch shape, both forms, sliced and not, against one restatement per shape."""
    fcn, jac, ctx = inner
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    n = sp.nnonlin
    rng = np.random.default_rng(m + n)
    per_fcn, per_jac = 8 * (2 * N + N * m + m + sp.nlin) + 4, 8 * (2 * N + 2 * N * m + m + sp.nlin) + 4
    for k, plist in enumerate(_shapes(nprob, n, rng, mixed)):
        rows = list(range(nprob)) if plist is None else [int(p) for p in plist]
        X = x_nl[rows] * (1.0 + jitter * np.random.default_rng(k).uniform(-1, 1, (len(rows), n)))
        PH, rank, wantF, wantJ = _expected(*evals, N, lin, X, rows)
        assert np.isfinite(wantF).all() and np.isfinite(wantJ).all()
        for form in FORMS:
            for sliced in (False, True):
                if sliced and len(rows) < 3:
                    continue
                # a cap that holds one point of the call: at least three slices
                with _env(NLH_SEP_FORM=form, NLH_SEP_SCRATCH=per_fcn + 8 if sliced else None):
                    F = _launch(ds, wf, wctx, plist, X, m)
                with _env(NLH_SEP_FORM=form, NLH_SEP_SCRATCH=per_jac + 8 if sliced else None):
                    J = _launch(ds, wj, wctx, plist, X, m, jac=True)
                tag = (what, m, k, form, sliced)
                assert np.array_equal(_bits(F), _bits(wantF)), (tag, np.abs(F - wantF).max())
                assert np.array_equal(_bits(J), _bits(wantJ)), (tag, np.abs(J - wantJ).max())
        if plist is None:                                         # the solve step works on problems 0 .. nprob-1
            for form in FORMS:
                with _env(NLH_SEP_FORM=form):
                    full, rk = ds.sep_solve(wctx, m, _dev(ds, X))
                assert np.array_equal(_bits(full.cpu().numpy()), _bits(PH)), (what, m, form)
                assert rk.cpu().numpy().tolist() == rank.tolist()
    wctx.close()
    return rank


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("m", [64, 200, 256, 257, 301, 513])
@pytest.mark.parametrize("K,B", [(1, 1), (2, 1)])
def test_lorentz_bitwise(ds, K, B, m, weighted):
    """(L, n) = (3, 2) and (4, 4): k_sep_solve and k_sep_project through the wrapping launchers around the Lorentzian, against
    the restatement around the curve restatement."""
    nprob, N = 5, 3 * K + B + 1
    lin = SC.lorentz_linear(K, B)
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=11 + m)
    w = _weights(np.random.default_rng(m), nprob, m, N) if weighted else None
    sp = nl.Separable.for_curve("lorentz", K, B)
    assert sp.tables()[0].tolist() == lin
    dt, dy, dw = _dev(ds, t), _dev(ds, y), (_dev(ds, w) if weighted else None)
    inner = ds.curve_launchers("lorentz", K, B, dt, dy, dw)
    rank = _check_calls(ds, sp, inner, _lorentz_eval(K, B, t, y, w), N, lin, m, x0[:, SR.tables(N, lin)[1]], nprob, 9, "lorentz")
    assert set(rank.tolist()) == {len(lin)}


@pytest.mark.parametrize("m", [2100, 2500])
def test_lorentz_bitwise_at_the_lds_limits(ds, m):
    """K = 2, B = 1 (L = 4, n = 4), 8 m (L + 1 + n) bytes around a workgroup's LDS: m = 2100 is about the lds form's largest
    panel here (151,200 bytes beside the solve kernel's own 10 KB), at m = 2500 and beyond the global form runs whatever is asked."""
    K, B, nprob, N = 2, 1, 3, 8
    lin = SC.lorentz_linear(K, B)
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=11 + m)
    sp = nl.Separable.for_curve("lorentz", K, B)
    inner = ds.curve_launchers("lorentz", K, B, _dev(ds, t), _dev(ds, y))
    _check_calls(ds, sp, inner, _lorentz_eval(K, B, t, y, None), N, lin, m, x0[:, SR.tables(N, lin)[1]], nprob, 2, "lds limits")


@pytest.mark.parametrize("K,B", [(1, 1), (2, 1)])
def test_lorentz_bitwise_at_m_equal_N(ds, K, B):
    """m = N: the smallest data a separable fit accepts."""
    N = 3 * K + B + 1
    nprob, m, lin = 4, N, SC.lorentz_linear(K, B)
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=3)
    sp = nl.Separable.for_curve("lorentz", K, B)
    inner = ds.curve_launchers("lorentz", K, B, _dev(ds, t), _dev(ds, y))
    _check_calls(ds, sp, inner, _lorentz_eval(K, B, t, y, None), N, lin, m, x0[:, SR.tables(N, lin)[1]], nprob, 5, "lorentz m = N")


@pytest.mark.parametrize("m", [2, 64, 257, 513])
def test_formula_L1_n1_bitwise(ds, m):
    """(L, n) = (1, 1): an exp-free formula restated from its parameters."""
    nprob = 4
    e = nl.Expr(LOR1, ("t",), ("a", "k"))
    sp = nl.Separable.for_expr(e, linear=("a",))
    rng = np.random.default_rng(m)
    t = np.tile(np.linspace(-1.0, 1.0, m), (nprob, 1)) + 1e-3 * rng.uniform(-1, 1, (nprob, m))
    xt = np.stack([rng.uniform(1.0, 3.0, nprob), rng.uniform(2.0, 6.0, nprob)], axis=1)
    y = np.stack([xt[p, 0] / (1.0 + (t[p] * xt[p, 1]) ** 2) for p in range(nprob)]) + 1e-3 * rng.uniform(-1, 1, (nprob, m))
    inner = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    _check_calls(ds, sp, inner, _expr_eval(e.program(), t, y, None), 2, [0], m, xt[:, [1]] * 1.1, nprob, 7, "formula")


@pytest.mark.parametrize("m", [34, 200, 513])
def test_L32_n2_bitwise(ds, m):
    """(L, n) = (32, 2): 32 Lorentzians whose centres and widths are tied to the first one's by a parameter map -- 32 amplitudes,
    one centre, one width.  The restatement is fed the device's own inner values."""
    K, nprob = 32, 3
    tied = {}
    for k in range(1, K):
        tied[3 * k + 1] = (1, 1.0, 0.03 * k)                      # mu_k = mu_0 + 0.03 k
        tied[3 * k + 2] = (2, 1.0 + 0.02 * k, 0.0)                # w_k = (1 + 0.02 k) w_0
    pm = nl.ParamMap(3 * K, tied=tied)
    assert pm.nfree == 34
    f2f = pm.tables()[4].tolist()
    lin = [j for j, k in enumerate(f2f) if k % 3 == 0]
    sp = nl.Separable(34, linear=lin)
    assert (sp.nlin, sp.nnonlin) == (32, 2)
    rng = np.random.default_rng(m)
    t = np.tile(np.linspace(0.0, 1.0, m), (nprob, 1))
    y = rng.uniform(0.0, 2.0, (nprob, m))
    cf, cj, cctx = ds.curve_launchers("lorentz", K, -1, _dev(ds, t), _dev(ds, y))
    inner = ds.pmap_launchers(pm, cf, cj, cctx, torch.zeros(3 * K, dtype=torch.float64, device=ds.device))
    x_nl = np.stack([rng.uniform(0.02, 0.04, nprob), rng.uniform(0.01, 0.02, nprob)], axis=1)
    rank = _check_calls(ds, sp, inner, _device_eval(ds, *inner, m), 34, lin, m, x_nl, nprob, 2, "L = 32")
    print(f"L = 32, m = {m}: live columns {sorted(set(rank.tolist()))}")
    assert rank.max() <= 32 and rank.min() >= 1
    inner[2].close()


def test_expdecay_bitwise_on_the_device_s_values(ds):
    """The exp kind (the study's biexponential): the device's own Phi, f0 and D through the restated QR and projection."""
    m, nprob = 128, 4
    t, y, xt, k0 = SC.study_problems(nprob)
    sp = nl.Separable.for_curve("expdecay", 2, 0)
    inner = ds.curve_launchers("expdecay", 2, 0, _dev(ds, t), _dev(ds, y))
    _check_calls(ds, sp, inner, _device_eval(ds, *inner, m), 5, list(SC.STUDY_LINEAR), m, k0, nprob, 5, "expdecay")


def test_dead_column(ds):
    """Two Lorentzians at the same centre and width: the second amplitude's column is the first's, so it is dead -- c = +0.0,
    rank L - 1 --, on the device as in the restatement, in both forms."""
    K, B, m, nprob = 2, 1, 200, 3
    N, lin = 8, SC.lorentz_linear(K, B)
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=21)
    x_nl = x0[:, [1, 2, 1, 2]]
    sp = nl.Separable.for_curve("lorentz", K, B)
    inner = ds.curve_launchers("lorentz", K, B, _dev(ds, t), _dev(ds, y))
    rank = _check_calls(ds, sp, inner, _lorentz_eval(K, B, t, y, None), N, lin, m, x_nl, nprob, 4, "dead", jitter=0.0)
    assert rank.tolist() == [3] * nprob
    wf, wj, wctx = ds.sep_launchers(sp, *inner)
    full, rk = ds.sep_solve(wctx, m, _dev(ds, x_nl))
    c2 = full.cpu().numpy()[:, 3]
    assert np.array_equal(_bits(c2), _bits(np.zeros(nprob))) and rk.cpu().numpy().tolist() == [3] * nprob
    wctx.close()


# ------------------------------------------------------------------------------------------------ 2. the residual the solver sees
@pytest.mark.parametrize("form", FORMS)
def test_residual_is_the_inner_one_at_the_solved_parameters(ds, form):
    K, B, m, nprob = 2, 1, 301, 6
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=8)
    sp = nl.Separable.for_curve("lorentz", K, B)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    alpha = ds.sep_gather(sp, _dev(ds, x0))
    assert np.array_equal(alpha.cpu().numpy(), x0[:, sp.tables()[1]])
    with _env(NLH_SEP_FORM=form):
        F = _launch(ds, wf, wctx, None, alpha.cpu().numpy(), m)
        full, rk = ds.sep_solve(wctx, m, alpha)
    inner = _launch(ds, fcn, ctx, list(range(nprob)), full.cpu().numpy(), m)
    assert np.array_equal(_bits(F), _bits(inner))
    assert np.array_equal(full.cpu().numpy()[:, sp.tables()[1]], alpha.cpu().numpy())
    wctx.close()


# ------------------------------------------------------------------------------------------------ 3. solves against the oracle
def _solve_against_oracle(ds, oracle, sp, inner, evals, N, lin, m, alpha0, analytic, what):
    wf, wj, wctx = ds.sep_launchers(sp, *inner)
    x = _dev(ds, alpha0)
    opt = dict(max_evals=SC.MAX_EVALS)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options(**opt))
    torch.cuda.synchronize()
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**opt)
    F, J = evals
    for p in range(len(alpha0)):
        fcn = lambda P, p=p: F(P[None, :], [p])[0]
        jac = lambda P, p=p: J(P[None, :], [p])[0].T
        f, j = SC.oracle_callbacks(fcn, jac, N, lin, analytic)
        rc, xo, fo, ibo = oracle.lm_solve(f, m, len(alpha0[p]), alpha0[p], jac=j, opts=oo)
        tag = (what, analytic, p)
        assert status[p] == rc, (tag, status[p], rc)
        assert all(ibs[p][k] == ibo[k] for k in KEYS), (tag, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (tag, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), tag
    assert set(status) == {0}
    wctx.close()
    return [ib["iter_count"] for ib in ibs]


@pytest.mark.parametrize("analytic", [True, False])
def test_lorentz_solves_against_oracle(ds, oracle, analytic):
    """lm_solve through the wrapping pair, Lorentz K = 2, B = 1 (L = 4, n = 4), against the oracle's lm_solve over the
    restatement: status, x, fvec and every count, every problem; more than one iteration count in the batch."""
    K, B, m, nprob = 2, 1, 200, 8
    N, lin = 8, SC.lorentz_linear(K, B)
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=31)
    sp = nl.Separable.for_curve("lorentz", K, B)
    inner = ds.curve_launchers("lorentz", K, B, _dev(ds, t), _dev(ds, y))
    iters = _solve_against_oracle(ds, oracle, sp, inner, _lorentz_eval(K, B, t, y, None), N, lin, m,
                                  np.ascontiguousarray(x0[:, SR.tables(N, lin)[1]]), analytic, "lorentz")
    assert len(set(iters)) > 1, iters


@pytest.mark.parametrize("analytic", [True, False])
def test_formula_solves_against_oracle(ds, oracle, analytic):
    """The same through a formula: one Lorentzian on a constant, a and c projected (L = 2, n = 2)."""
    m, nprob = 257, 6
    e = nl.Expr(LOR4, ("t",), ("a", "mu", "w", "c"))
    sp = nl.Separable.for_expr(e, linear=("a", "c"))
    rng = np.random.default_rng(5)
    t = np.tile(np.linspace(0.0, 1.0, m), (nprob, 1))
    xt = np.stack([rng.uniform(1, 3, nprob), rng.uniform(0.4, 0.6, nprob), rng.uniform(0.05, 0.1, nprob), rng.uniform(0.1, 0.5, nprob)], axis=1)
    y = np.stack([xt[p, 0] / (1.0 + ((t[p] - xt[p, 1]) / xt[p, 2]) ** 2) + xt[p, 3] for p in range(nprob)])
    y = y + 1e-3 * rng.uniform(-1, 1, y.shape)
    alpha0 = np.ascontiguousarray(xt[:, [1, 2]] * (1.0 + 0.1 * rng.uniform(-1, 1, (nprob, 2))))
    inner = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    _solve_against_oracle(ds, oracle, sp, inner, _expr_eval(e.program(), t, y, None), 4, [0, 3], m, alpha0, analytic, "formula")


# ------------------------------------------------------------------------------------------------ 4. refusals, sep_check
def test_refusals_leave_the_caller_s_arrays_alone(ds):
    K, B, m, nprob = 1, 1, 64, 3
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=2)
    sp = nl.Separable.for_curve("lorentz", K, B)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, _dev(ds, t), _dev(ds, y))
    out = C.c_void_p(0xdead)
    none = C.cast(None, _lib.DEVFCN)
    assert ds.lib.nlh_sep_wrap(ds.h.ptr, sp.ptr, fcn, none, ds._ctxp(ctx), C.byref(out)) == NL_UNDEFINED_FUNCTION_ERROR and not out.value
    assert ds.lib.nlh_sep_wrap(ds.h.ptr, sp.ptr, none, jac, ds._ctxp(ctx), C.byref(out)) == NL_UNDEFINED_FUNCTION_ERROR and not out.value
    assert ds.lib.nlh_sep_wrap(ds.h.ptr, None, fcn, jac, ds._ctxp(ctx), C.byref(out)) == NL_INVALID_INPUT_ERROR and not out.value
    assert ds.lib.nlh_sep_wrap(ds.h.ptr, sp.ptr, fcn, jac, ds._ctxp(ctx), None) == NL_INVALID_INPUT_ERROR
    with pytest.raises(ValueError):
        ds.sep_launchers(sp, fcn, None, ctx)
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    X = x0[:, [1, 2]]
    for launcher, isjac in ((wf, False), (wj, True)):
        for n_, m_, X_ in ((3, m, x0[:, :3]), (2, 4, X), (2, m + 1, X)):      # n != N - L; m < N; the inner launcher's refusal
            got = _launch(ds, launcher, wctx, None, np.ascontiguousarray(X_), m_, jac=isjac, expect=NL_INVALID_INPUT_ERROR)
            assert np.isnan(got).all()
    full = torch.full((nprob, 5), np.nan, dtype=torch.float64, device=ds.device)
    rank = torch.full((nprob,), -7, dtype=torch.int32, device=ds.device)
    dX = _dev(ds, X)
    assert ds.lib.nlh_sep_solve_batch(ds.h.ptr, wctx.ptr, nprob, 4, dX.data_ptr(), full.data_ptr(), rank.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_sep_solve_batch(ds.h.ptr, wctx.ptr, nprob, m, None, full.data_ptr(), rank.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_sep_solve_batch(ds.h.ptr, None, nprob, m, dX.data_ptr(), full.data_ptr(), rank.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_sep_solve_batch(ds.h.ptr, wctx.ptr, nprob, m + 1, dX.data_ptr(), full.data_ptr(), rank.data_ptr()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(full).all() and (rank == -7).all()
    assert ds.lib.nlh_sep_solve_batch(ds.h.ptr, wctx.ptr, 0, m, None, None, None) == 0
    assert ds.lib.nlh_sep_gather_batch(ds.h.ptr, sp.ptr, nprob, None, dX.data_ptr()) == NL_INVALID_INPUT_ERROR
    wctx.close()


def test_sep_check(ds):
    """0 for a curve model's amplitudes and baseline; above 0 for a formula that is not affine in the declared parameter."""
    K, B, m, nprob = 2, 1, 64, 3
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=4)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, _dev(ds, t), _dev(ds, y))
    assert ds.sep_check(nl.Separable.for_curve("lorentz", K, B), fcn, jac, ctx, m, _dev(ds, x0)) == 0.0
    e = nl.Expr("a*a*t + k", ("t",), ("a", "k"))
    ef, ej, ectx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    full = _dev(ds, np.tile([1.5, 0.2], (nprob, 1)))
    assert ds.sep_check(nl.Separable.for_expr(e, linear=("a",)), ef, ej, ectx, m, full) > 0.1
    assert ds.sep_check(nl.Separable.for_expr(e, linear=("k",)), ef, ej, ectx, m, full) == 0.0


# ------------------------------------------------------------------------------------------------ 5. the one-call fits
def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


def _by_hand(ds, sp, inner, m, dx0, analytic, o):
    """gather; the solve through the projecting pair; sep_solve; the covariance of the INNER pair at the full solution."""
    fcn, jac, ctx = inner
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    alpha = ds.sep_gather(sp, dx0)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, alpha, jac=wj if analytic else None, opts=o)
    full, _ = ds.sep_solve(wctx, m, alpha)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(fcn, ctx, m, full, jac=jac if analytic else None)
    wctx.close()
    return full, fvec, sigma, cov, chi2, rank, ibs, status


@pytest.mark.parametrize("analytic", [True, False])
@pytest.mark.parametrize("model", ["curve", "formula", "curve-conv"])
def test_one_call_is_the_composition(ds, model, analytic):
    """curve_fit_batch / expr_fit_batch with sep= give the bits of the composition by hand; the linear positions of x0 are not read."""
    import conv_cases as CV
    K, B, m, nprob = 2, 1, 200, 6
    o = ds.options(max_evals=SC.MAX_EVALS)
    conv = None
    if model == "curve-conv":
        t, y, xt, x0 = CV.line_problems(K, B, m, nprob)
        k, origin = CV.line_shape(), CV.LINE_ORIGIN
        conv = nl.Convolve(k, origin=origin, extend=CV.LINE_EXTEND)
    else:
        t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=13)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    if model == "formula":
        e = nl.Expr("a1/(1+((t-m1)/w1)^2) + a2/(1+((t-m2)/w2)^2) + c0 + c1*t", ("t",), ("a1", "m1", "w1", "a2", "m2", "w2", "c0", "c1"))
        sp = nl.Separable.for_expr(e, linear=("a1", "a2", "c0", "c1"))
        inner = ds.expr_launchers(e, dt, dy)
        got = ds.expr_fit_batch(e, dt, dy, dx0, analytic=analytic, opts=o, sep=sp)
    else:
        sp = nl.Separable.for_curve("lorentz", K, B)
        inner = ds.curve_launchers("lorentz", K, B, dt, dy)
        if conv is not None:
            inner = ds.conv_launchers(conv, *inner, dy)
        got = ds.curve_fit_batch("lorentz", dt, dy, dx0, ncomp=K, baseline=B, analytic=analytic, opts=o, sep=sp, conv=conv)
    hand = _by_hand(ds, sp, inner, m, dx0, analytic, o)
    assert set(got[7]) == {0} and got[7] == hand[7] and got[6] == hand[6]
    for g, w_ in zip(got[:6], hand[:6]):
        assert _eq(g, w_), (model, analytic)
    junk = dx0.clone()
    junk[:, torch.from_numpy(sp.tables()[0].astype("int64")).to(ds.device)] = 1e30
    if model == "formula":
        again = ds.expr_fit_batch(e, dt, dy, junk, analytic=analytic, opts=o, sep=sp)
    else:
        again = ds.curve_fit_batch("lorentz", dt, dy, junk, ncomp=K, baseline=B, analytic=analytic, opts=o, sep=sp, conv=conv)
    for g, w_ in zip(again[:6], got[:6]):
        assert _eq(g, w_)
    # against the full fit from the same start: the same minimum within the recorded 1e-2 sigma
    if model == "curve" and analytic:
        start = hand[0].clone()
        start[:, 1::3][:, :K] = dx0[:, 1::3][:, :K]
        start[:, 2::3][:, :K] = dx0[:, 2::3][:, :K]
        fullfit = ds.curve_fit_batch("lorentz", dt, dy, start, ncomp=K, baseline=B, opts=o)
        assert set(fullfit[7]) == {0}
        assert float(torch.max(torch.abs(fullfit[0] - got[0]) / fullfit[2])) <= 1e-2


def test_one_call_zero_weight_padding_and_dof(ds):
    """Ragged data padded with zero weights: the degrees of freedom count N, all the parameters, not the nonlinear ones; a
    problem without any keeps its x and gets the status and NaNs, it alone; chi2 and cov follow the curve fits' rule."""
    K, B, m, nprob = 1, 1, 96, 12
    N = 5
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=6)
    rng = np.random.default_rng(8)
    w = np.ones((nprob, m))
    length = rng.integers(80, m + 1, nprob)
    length[3], length[7], length[nprob - 1] = N, N - 1, m           # dof 0 (although 3 more rows than nonlinear unknowns), dof < 0, no padding
    for p in range(nprob):
        w[p, length[p]:] = 0.0
        y[p, length[p]:] = 1e3
    dt, dy, dw, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, w), _dev(ds, x0)
    o = ds.options(max_evals=SC.MAX_EVALS)
    sp = nl.Separable.for_curve("lorentz", K, B)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch("lorentz", dt, dy, dx0, ncomp=K, baseline=B, weights=dw, opts=o, sep=sp)
    bad = [3, 7]
    good = [p for p in range(nprob) if p not in bad]
    assert [st[p] for p in bad] == [NL_INVALID_INPUT_ERROR] * 2 and {st[p] for p in good} == {0}
    xh, fh, sh, ch, qh, rh = (v.cpu().numpy() for v in (x, fvec, sigma, cov, chi2, rank))
    for p in bad:
        assert np.isnan(sh[p]).all() and np.isnan(ch[p]).all() and np.isnan(qh[p]) and rh[p] == -1
        assert np.array_equal(_bits(xh[p]), _bits(x0[p])) and ibs[p]["fcn_count"] == 0
    gi = torch.tensor(good, device=ds.device)
    inner = ds.curve_launchers("lorentz", K, B, dt[gi].contiguous(), dy[gi].contiguous(), dw[gi].contiguous())
    hand = _by_hand(ds, sp, inner, m, dx0[gi].contiguous(), True, o)
    hx, hf, hs, hc, hq, hr = (v.cpu().numpy() for v in hand[:6])
    for k, p in enumerate(good):
        dof = int(length[p]) - N
        assert np.array_equal(_bits(xh[p]), _bits(hx[k])) and np.array_equal(_bits(fh[p]), _bits(hf[k])) and rh[p] == hr[k] == N
        assert ibs[p] == hand[6][k]
        s = 0.0
        for v in fh[p]:
            s = s + v * v
        assert _bits(qh[p]) == _bits(s / float(dof)), (p, qh[p], s / dof)
        wc = hc[k] * (float(m - N) / float(dof))
        assert np.array_equal(_bits(ch[p]), _bits(wc)), p
        assert np.array_equal(_bits(sh[p]), _bits(np.sqrt(np.diag(wc)))), p
        assert (fh[p][length[p]:] == 0.0).all()


def test_one_call_alone_inside_300_and_host_twin(ds):
    K, B, m, nprob, N = 1, 0, 64, 300, 4
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=77)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=SC.MAX_EVALS)
    sp = nl.Separable.for_curve("lorentz", K, B)
    big = ds.curve_fit_batch("lorentz", dt, dy, dx0, ncomp=K, baseline=B, opts=o, sep=sp)
    assert set(big[7]) == {0}
    for p in (0, 137, nprob - 1):
        one = ds.curve_fit_batch("lorentz", dt[p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dx0[p:p + 1].contiguous(), ncomp=K,
                                 baseline=B, opts=o, sep=sp)
        for g, w_ in zip(one[:6], big[:6]):
            assert _eq(g, w_[p:p + 1]), p
        assert one[6][0] == big[6][p]
    with _env(NLH_SEP_FORM="global"):
        other = ds.curve_fit_batch("lorentz", dt, dy, dx0, ncomp=K, baseline=B, opts=o, sep=sp)
    for g, w_ in zip(other[:6], big[:6]):
        assert _eq(g, w_)
    dp = C.POINTER(C.c_double)
    xh, fh = x0.copy(), np.zeros((nprob, m))
    sh, ch, qh, rh = np.zeros((nprob, N)), np.zeros((nprob, N, N)), np.zeros(nprob), np.zeros(nprob, dtype=np.int32)
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    rc = ds.lib.nlh_curve_fit_batch_sep_h(ds.h.ptr, C.byref(o), R.LORENTZ, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None,
                                          1, None, None, None, None, sp.ptr, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp),
                                          sh.ctypes.data_as(dp), ch.ctypes.data_as(dp), qh.ctypes.data_as(dp),
                                          rh.ctypes.data_as(_lib.c_int32_p), ib, st)
    assert rc == 0
    for g, w_ in zip((xh, fh, sh, ch, qh), big[:5]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    assert np.array_equal(rh, big[5].cpu().numpy()) and [ib[p].as_dict() for p in range(nprob)] == big[6]


def test_one_call_refusals(ds):
    """In the documented order after the plain entry point's: a NULL sp, an sp of another N, a shared linear parameter, a finite bound at a linear
    position; the caller's arrays stay untouched."""
    K, B, m, nprob, N = 1, 1, 64, 2, 5
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=2)
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    f = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)
    sp, other = nl.Separable.for_curve("lorentz", K, B), nl.Separable(6, linear=(0,))
    g = nl.Group(N, shared=(1, 0), nsets=2)
    inf = np.full(N, np.inf)
    dp = C.POINTER(C.c_double)

    def fit(mm=m, sep=sp, grp=None, lo=None, hi=None, kind=R.LORENTZ):
        return ds.lib.nlh_curve_fit_batch_sep(ds.h.ptr, C.byref(o), kind, K, B, nprob, mm, dt.data_ptr(), 0, dy.data_ptr(), None, 1,
                                              None if lo is None else lo.ctypes.data_as(dp), None if hi is None else hi.ctypes.data_as(dp),
                                              grp.ptr if grp is not None else None, None, sep.ptr if sep is not None else None,
                                              dx.data_ptr(), f.data_ptr(), None, None, None, None, None, None)
    assert fit(kind=7) == NL_INVALID_INPUT_ERROR
    assert fit(mm=N - 1) == 212                                    # NLH_UNDERDEFINED_PROBLEM_ERROR: m >= N, not m >= n
    assert fit(sep=None) == NL_INVALID_INPUT_ERROR
    assert fit(sep=other) == NL_INVALID_INPUT_ERROR
    assert fit(grp=g) == NL_INVALID_INPUT_ERROR                     # a shared linear parameter (the amplitude)
    lo = -inf.copy()
    lo[0] = 0.0
    assert fit(lo=lo) == NL_INVALID_INPUT_ERROR                     # a finite bound on an amplitude
    hi = inf.copy()
    hi[4] = 10.0
    assert fit(hi=hi) == NL_INVALID_INPUT_ERROR
    torch.cuda.synchronize()
    assert np.array_equal(_bits(dx.cpu().numpy()), _bits(x0)) and (f == 7.0).all()
    lo = -inf.copy()
    lo[2] = 1e-3                                                    # a bound on a width: honoured, by the bounded solver
    assert fit(lo=lo, hi=inf) == 0
    torch.cuda.synchronize()
    assert (dx[:, 2] >= 1e-3).all() and not (f == 7.0).any()
    with pytest.raises(ValueError):
        ds.curve_fit_batch("lorentz", dt, dy, dx, ncomp=K, baseline=B, sep=sp, pmap=nl.ParamMap(N, fixed=(1,)))
    with pytest.raises(ValueError):
        ds.curve_fit_batch("lorentz", dt, dy, dx, ncomp=K, baseline=B, sep=other)


@pytest.mark.parametrize("analytic", [True, False])
def test_one_call_with_a_group_is_the_composition(ds, analytic):
    """group= with sep=, with and without conv=: one Lorentzian on a line, the width shared by the G = 4 data sets of a group,
    amplitude and baseline projected out per data set.  By hand: the group of the same shared
    parameter over the nonlinear unknowns around the projecting pair; gather, gather; solve; expand; sep_solve; then the
    caller's group around the unprojected pair for the errors at the full solution."""
    import conv_cases as CV
    K, B, m, G, ngroup, N = 1, 1, 96, 4, 5, 5
    nprob = G * ngroup
    t, y, xt, x0 = CV.line_problems(K, B, m, nprob, shared=(2,), G=G)
    conv = nl.Convolve(CV.line_shape(), origin=CV.LINE_ORIGIN, extend=CV.LINE_EXTEND)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=SC.MAX_EVALS)
    sp = nl.Separable.for_curve("lorentz", K, B)                  # linear 0, 3, 4; nonlinear (mu, w) = 1, 2
    g = nl.Group(N, shared=(2,), nsets=G)
    gred = nl.Group(2, shared=(1,), nsets=G)
    for cv in (None, conv):
        inner = ds.curve_launchers("lorentz", K, B, dt, dy)
        if cv is not None:
            inner = ds.conv_launchers(cv, *inner, dy)
        got = ds.curve_fit_batch("lorentz", dt, dy, dx0, ncomp=K, baseline=B, analytic=analytic, opts=o, sep=sp, group=g, conv=cv)
        wf, wj, wctx = ds.sep_launchers(sp, *inner)
        gf, gj, gctx = ds.group_launchers(gred, wf, wj if analytic else None, wctx)
        xo = ds.group_gather(gred, ds.sep_gather(sp, dx0))
        fvec, ibs, status = ds.lm_solve_batch_device(gf, gctx, G * m, xo, jac=gj if analytic else None, opts=o)
        full, _ = ds.sep_solve(wctx, m, ds.group_expand(gred, xo))
        ff, fj, fctx = ds.group_launchers(g, inner[0], inner[1] if analytic else None, inner[2])
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(ff, fctx, G * m, ds.group_gather(g, full), jac=fj if analytic else None)
        hand = (full, fvec.reshape(nprob, m), ds.group_sigma(g, sigma), cov, chi2, rank)
        assert got[7] == status and got[6] == ibs and len(status) == ngroup and (cv is None or set(status) == {0})
        for a_, b_ in zip(got[:6], hand):
            assert _eq(a_, b_), (analytic, cv is not None)
        w_all = got[0][:, 2].reshape(ngroup, G)
        assert (w_all == w_all[:, :1]).all()                      # the shared width is equal across a group


# ------------------------------------------------------------------------------------------------ 6. the model object
def test_model_object(ds):
    """nlh_sep_model_create over a curve model, through _eval, _lm_solve, _lm_covariance = the launcher forms; its refusals."""
    K, B, m, nprob, N, n = 2, 1, 200, 6, 8, 4
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=19)
    sp = nl.Separable.for_curve("lorentz", K, B)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    a0 = np.ascontiguousarray(x0[:, sp.tables()[1]])
    o = ds.options(max_evals=SC.MAX_EVALS)
    dp = C.POINTER(C.c_double)
    inner, md, fd = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.LORENTZ, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 1, C.byref(inner)) == 0
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.LORENTZ, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 0, C.byref(fd)) == 0
    assert ds.lib.nlh_sep_model_create(ds.h.ptr, inner, sp.ptr, C.byref(md)) == 0
    try:
        s_ = [C.c_int32() for _ in range(3)]
        ds.lib.nlh_dq_model_shape(md, *[C.byref(v) for v in s_])
        assert [v.value for v in s_] == [nprob, m, n]
        f0 = np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_eval(ds.h.ptr, md, a0.ctypes.data_as(dp), f0.ctypes.data_as(dp)) == 0
        assert np.array_equal(_bits(f0), _bits(_launch(ds, wf, wctx, list(range(nprob)), a0, m)))
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        xh, fh = a0.copy(), np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_lm_solve(ds.h.ptr, C.byref(o), md, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, a0)
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj, opts=o)
        assert np.array_equal(_bits(xh), _bits(x.cpu().numpy())) and np.array_equal(_bits(fh), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(nprob)] == ibs and list(st) == status and set(status) == {0}
        ch, sh, rh, qh = np.zeros((nprob, n, n)), np.zeros((nprob, n)), np.zeros(nprob, dtype=np.int32), np.zeros(nprob)
        assert ds.lib.nlh_dq_model_lm_covariance(ds.h.ptr, md, xh.ctypes.data_as(dp), 1, 0.0, ch.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                                 rh.ctypes.data_as(_lib.c_int32_p), qh.ctypes.data_as(dp)) == 0
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=wj, scaled=True)
        assert np.array_equal(_bits(ch), _bits(cov.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sigma.cpu().numpy()))
        assert np.array_equal(rh, rank.cpu().numpy()) and np.array_equal(_bits(qh), _bits(chi2.cpu().numpy()))
        out = C.c_void_p(7)
        other = nl.Separable(6, linear=(0,))
        assert ds.lib.nlh_sep_model_create(None, inner, sp.ptr, C.byref(out)) == -3
        assert ds.lib.nlh_sep_model_create(ds.h.ptr, inner, other.ptr, C.byref(out)) == NL_INVALID_INPUT_ERROR and not out.value
        assert ds.lib.nlh_sep_model_create(ds.h.ptr, None, sp.ptr, C.byref(out)) == NL_INVALID_INPUT_ERROR
        assert ds.lib.nlh_sep_model_create(ds.h.ptr, inner, None, C.byref(out)) == NL_INVALID_INPUT_ERROR
        assert ds.lib.nlh_sep_model_create(ds.h.ptr, fd, sp.ptr, C.byref(out)) == NL_UNDEFINED_FUNCTION_ERROR and not out.value
        A, b = np.zeros((1, m, N)), np.zeros((1, m))
        dq = C.c_void_p()
        assert ds.lib.nlh_dq_model_create(ds.h.ptr, 1, m, N, A.ctypes.data_as(dp), b.ctypes.data_as(dp), 0.5, C.byref(dq)) == 0
        assert ds.lib.nlh_sep_model_create(ds.h.ptr, dq, sp.ptr, C.byref(out)) == NL_INVALID_INPUT_ERROR
        ds.lib.nlh_dq_model_destroy(dq)
    finally:
        ds.lib.nlh_dq_model_destroy(md)
        ds.lib.nlh_dq_model_destroy(inner)
        ds.lib.nlh_dq_model_destroy(fd)
        wctx.close()
