"""GPU tests of the parameter maps (include/nonlin_hip.h: nlh_pmap_*), everything bit for bit: the four kernels against the
numpy restatement (tests/pmap_restatement.py) in both workgroup forms, with and without the column split, sliced and
unsliced; the identity map against the unmapped call; solves through the wrapping launchers against the CPU oracle on the
reduced problem; a formula through a map against the curve model through the same map; the one-call fits as the
composition they stand for; a problem alone against the same problem inside a batch of 300; the model object; the error
returns.  The bitwise tests use the Lorentzian and exp-free formulas only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import curve_cases as CC
import curve_restatement as R
import expr_restatement as XR
import pmap_cases as PC
import pmap_restatement as PR
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
dp = C.POINTER(C.c_double)
KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
FORMS = [None, "row", "flat"]               # None: the form m selects; a forced form that cannot hold m falls back to it
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR = 201, 211, 212
FORMULA = "a1/(1+((t-m1)/w1)^2) + a2/(1+((t-m2)/w2)^2) + c"
PARAMS = ("a1", "m1", "w1", "a2", "m2", "w2", "c")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


class _env:
    """Environment variables for the calls inside (the library reads NLH_PMAP_* at every call); None: unset."""

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


def _launch(ds, fcn, ctx, plist, X, m, jac=False):
    """One call of a launcher on the points X (numpy [npoints, n]) of the problems plist (None: no dprob, point q is problem
    q): F [npoints, m] or J [npoints, n, m]."""
    npts, n = X.shape
    dX = _dev(ds, X)
    dprob = _dev(ds, plist, np.int32) if plist is not None else None
    out = torch.full((npts, n, m) if jac else (npts, m), np.nan, dtype=torch.float64, device=ds.device)
    stream = torch.cuda.current_stream(ds.device).cuda_stream
    rc = fcn(ds._ctxp(ctx), C.c_void_p(stream), npts, C.c_void_p(dprob.data_ptr()) if dprob is not None else None, n,
             C.c_void_p(dX.data_ptr()), m, C.c_void_p(out.data_ptr()))
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _pmap(T):
    """The library's map of a restatement's tables."""
    kind, index, scale, offset, f2f = T
    fixed = [int(k) for k in np.flatnonzero(kind == PR.FIXED)]
    tied = {int(k): (int(index[k]), float(scale[k]), float(offset[k])) for k in np.flatnonzero(kind == PR.TIED)}
    return nl.ParamMap(len(kind), fixed=fixed, tied=tied)


# a map with everything in it over the nine parameters of two Lorentzians on a parabola: two ties on one free column, a
# negative scale, a tie to a fixed source (a derived constant), a non-zero offset
KERNEL_MAP = (9, [1, 8], {5: (2, 1.25, 0.0), 6: (0, -0.5, 0.1), 7: (8, -2.0, 0.5), 3: (2, 0.5, 0.02)})


# ------------------------------------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("m", [64, 200, 256, 301])
def test_launchers_bitwise(ds, m, shared, form):
    """k_pmap_expand and k_pmap_jac through the wrapping launchers around the Lorentzian: F = residual(expand(x)) and
    J = contract(jacobian(expand(x))) of the restatements, for every launch shape, form, column split and slicing."""
    K, B, nprob = 2, 2, 5
    kd, N = R.LORENTZ, 9
    T = PR.tables(*KERNEL_MAP)
    n = len(T[4])
    pm = _pmap(T)
    t, y, xt, x0 = CC.curve_problems("lorentz", K, B, m, nprob=nprob, seed=11 + m)
    rng = np.random.default_rng(m)
    w = rng.uniform(0.5, 2.0, (nprob, m))
    full = x0 * (1.0 + 0.01 * rng.uniform(-1, 1, x0.shape))
    if shared:
        full = np.ascontiguousarray(full[0])
    dt, dy, dw, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, w), _dev(ds, full)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, dt, dy, dw)
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, dfull)
    shapes = [[nprob - 2], [2] * (n + 1), list(np.random.default_rng(3).integers(0, nprob, 37)) + [0, 0, nprob - 1], None]
    for k, plist in enumerate(shapes):
        rows = list(range(nprob)) if plist is None else plist
        X = PR.gather(T, x0[rows]) * (1.0 + 0.01 * np.random.default_rng(k).uniform(-1, 1, (len(rows), n)))
        P = [PR.expand(T, X[q], full if shared else full[p]) for q, p in enumerate(rows)]
        wantF = [R.residual(kd, K, B, P[q], t[p], y[p], w[p]) for q, p in enumerate(rows)]
        wantJ = [PR.contract(T, R.jacobian(kd, K, B, P[q], t[p], w[p])).T for q, p in enumerate(rows)]
        # (split: column groups; scratch: a cap that cuts the call into slices of one (fcn) or two (jac) points)
        for split, sliced in ((None, False), (1, False), (2, False), (n, True), (None, True)):
            with _env(NLH_PMAP_FORM=form, NLH_PMAP_SPLIT=split, NLH_PMAP_SCRATCH=100 if sliced else None):
                F = _launch(ds, wf, wctx, plist, X, m)
            with _env(NLH_PMAP_FORM=form, NLH_PMAP_SPLIT=split, NLH_PMAP_SCRATCH=2 * 8 * N * (m + 1) + 16 if sliced else None):
                J = _launch(ds, wj, wctx, plist, X, m, jac=True)
            for q in range(len(rows)):
                assert np.array_equal(_bits(F[q]), _bits(wantF[q])), (form, k, q, split, sliced)
                assert np.array_equal(_bits(J[q]), _bits(wantJ[q])), (form, k, q, split, sliced)
    wctx.close()


def test_gather_expand_cov_bitwise(ds):
    rng = np.random.default_rng(21)
    specs = [KERNEL_MAP, (4, [], {}), (6, [0, 1, 2, 4, 5], {}), (33, list(range(0, 33, 3)), {k: (k + 1, 0.3 * k - 4.0, 0.01 * k) for k in range(1, 33, 6)})]
    for nfull, fixed, tied in specs:
        T = PR.tables(nfull, fixed, tied)
        pm = _pmap(T)
        n, nprob = len(T[4]), 37
        full = rng.standard_normal((nprob, nfull))
        x = rng.standard_normal((nprob, n))
        assert np.array_equal(_bits(ds.pmap_gather(pm, _dev(ds, full)).cpu().numpy()), _bits(PR.gather(T, full)))
        for fl in (full, full[3]):
            got = ds.pmap_expand(pm, _dev(ds, x), _dev(ds, fl)).cpu().numpy()
            assert np.array_equal(_bits(got), _bits(PR.expand(T, x, fl))), (nfull, fl.ndim)
        A = rng.standard_normal((nprob, n, n))
        cov = A @ A.transpose(0, 2, 1)
        sigma = np.sqrt(np.einsum("pii->pi", cov))
        fail = (rng.uniform(size=nprob) < 0.2).astype(np.int32)
        cov[fail != 0] = np.nan
        sigma[fail != 0] = np.nan
        for fl in (fail, None):
            cf, sf = ds.pmap_cov(pm, _dev(ds, cov), _dev(ds, sigma), _dev(ds, fl) if fl is not None else None)
            cf, sf = cf.cpu().numpy(), sf.cpu().numpy()
            for p in range(nprob):
                wc, ws = PR.cov_expand(T, cov[p], sigma[p], failed=fl is not None and bool(fl[p]))
                if fl is None and fail[p]:                              # NaN passes through wherever a factor exists
                    jk, g = PR.factors(T)
                    assert np.isnan(cf[p][np.ix_(jk >= 0, jk >= 0)]).all() and np.isnan(sf[p][jk >= 0]).all()
                    assert (cf[p][jk < 0] == 0.0).all() and (sf[p][jk < 0] == 0.0).all()
                    continue
                assert np.array_equal(np.isnan(cf[p]), np.isnan(wc)) and np.array_equal(np.isnan(sf[p]), np.isnan(ws))
                ok = ~np.isnan(wc)
                assert np.array_equal(_bits(cf[p][ok]), _bits(wc[ok])) and np.array_equal(_bits(sf[p][~np.isnan(ws)]), _bits(ws[~np.isnan(ws)]))


# ------------------------------------------------------------------------------------------------ 2. the identity map
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("kind,K,B,m", [CC.CASES[0], CC.CASES[3], CC.CASES[4]])
def test_identity_map_equals_the_unmapped_call(ds, kind, K, B, m, analytic):
    N = R.nparams(R.KINDS[kind], K, B)
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m)
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    o = ds.options(max_evals=CC.MAX_EVALS)
    xa = _dev(ds, x0)
    fa, iba, sta = ds.lm_solve_batch_device(fcn, ctx, m, xa, jac=jac if analytic else None, opts=o)
    pm = nl.ParamMap(N)
    assert pm.nfree == N
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, _dev(ds, x0))
    xb = _dev(ds, x0)
    fb, ibb, stb = ds.lm_solve_batch_device(wf, wctx, m, xb, jac=wj if analytic else None, opts=o)
    assert _eq(xa, xb) and _eq(fa, fb) and iba == ibb and sta == stb
    wctx.close()


# ------------------------------------------------------------------------------------------------ 3. the oracle
def _reduced_callbacks(T, kd, K, B, t, y, full, analytic):
    f = lambda x, out: out.__setitem__(slice(None), R.residual(kd, K, B, PR.expand(T, x, full), t, y))
    j = (lambda x, J: J.__setitem__((slice(None), slice(None)), PR.contract(T, R.jacobian(kd, K, B, PR.expand(T, x, full), t)))) \
        if analytic else None
    return f, j


@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("case,mp", PC.PAIRS)
def test_solves_against_oracle(ds, oracle, case, mp, analytic):
    """lm_solve on the reduced problem, the restatement's expand and contract as callbacks, every problem: status, x, fvec and
    every count identical, and status 0 for the whole batch.  With forward differences the inner launcher is asked for
    fcn_count + nfree * jacobian_count points in all: nfree, not N, perturbed evaluations per Jacobian, beside the one at x
    that fcn_count counts.  (The reference's fcn_count does not count the perturbed evaluations -- tests/test_pmap_cpu.py
    shows the same relation on the oracle's own callback --, so the points are counted where they are evaluated.)"""
    kind, K, B, m = case
    kd, N = R.KINDS[kind], R.nparams(R.KINDS[kind], K, B)
    t, y, xt, x0 = PC.problems(kind, K, B, m)
    T = PR.tables(N, *PC.map_spec(mp, K, B))
    n = len(T[4])
    pm = _pmap(T)
    full = PC.full_start(T, xt, x0)
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    asked = [0]

    def counting(c, stream, npoints, dprob, nn, dX, mm, dF):
        assert nn == N
        asked[0] += npoints
        return ds.lib.nlh_curve_device_fcn(c, stream, npoints, dprob, nn, dX, mm, dF)
    inner = _lib.DEVFCN(counting)
    wf, wj, wctx = ds.pmap_launchers(pm, inner, jac, ctx, dfull)
    x = ds.pmap_gather(pm, dfull)
    assert x.shape == (PC.NPROB, n)
    opt = dict(max_evals=PC.MAX_EVALS)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options(**opt))
    torch.cuda.synchronize()
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**opt)
    for p in range(PC.NPROB):
        f, j = _reduced_callbacks(T, kd, K, B, t[p], y[p], full[p], analytic)
        rc, xo, fo, ibo = oracle.lm_solve(f, m, n, PR.gather(T, full[p]), jac=j, opts=oo)
        what = (case, mp, analytic, p)
        assert status[p] == rc, (what, status[p], rc)
        assert _same(ibs[p], ibo), (what, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), what
    assert set(status) == {0}
    evals = sum(ib["fcn_count"] + (0 if analytic else n * ib["jacobian_count"]) for ib in ibs)
    print(f"pmap {case} {mp} analytic={analytic}: n = {n} of N = {N}, inner points asked {asked[0]}, counted {evals}")
    assert asked[0] == evals
    wctx.close()


@pytest.mark.parametrize("analytic", [False, True])
def test_bounded_solve_against_oracle(ds, oracle, analytic):
    """One bounded pair against oracle.cls_solve on the reduced problem: equality only, no claim on the status."""
    (kind, K, B, m), mp = PC.CASES[1], "both"
    kd, N = R.KINDS[kind], R.nparams(R.KINDS[kind], K, B)
    t, y, xt, x0 = PC.problems(kind, K, B, m)
    T = PR.tables(N, *PC.map_spec(mp, K, B))
    n, f2f = len(T[4]), T[4]
    pm = _pmap(T)
    lower = np.minimum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) - 0.02       # a box some true values lie outside of: bounds that bind
    upper = np.maximum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) + 0.02
    full = PC.full_start(T, xt, np.clip(x0, lower, upper))
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, dfull)
    x = ds.pmap_gather(pm, dfull)
    opt = dict(max_evals=PC.MAX_EVALS)
    fvec, ibs, status = ds.cls_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options(**opt),
                                                  lower=lower[f2f], upper=upper[f2f])
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**opt)
    for p in range(PC.NPROB):
        f, j = _reduced_callbacks(T, kd, K, B, t[p], y[p], full[p], analytic)
        rc, xo, fo, ibo = oracle.cls_solve(f, m, n, PR.gather(T, full[p]), jac=j, opts=oo, lower=lower[f2f], upper=upper[f2f])
        assert status[p] == rc and _same(ibs[p], ibo), (p, status[p], rc, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)) and np.array_equal(_bits(fg[p]), _bits(fo)), p
    wctx.close()


# ------------------------------------------------------------------------------------------------ 4. a formula through the map
def test_formula_through_the_map(ds):
    """The two-Lorentzian formula with w2 tied to w1 and c fixed, by name: its residuals -- and so a forward-difference solve
    and the covariance at its solution -- have the bits of the curve model through the same map (the formula's value program
    makes the curve model's operations in the curve model's order); its analytic Jacobian, whose tangents are the formula
    table's and not the curve table's, has the bits of contract(the formula restatement's Jacobian)."""
    kind, K, B, m = "lorentz", 2, 0, 200
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    pm = nl.ParamMap.for_expr(e, fixed=("c",), tied={"w2": ("w1", 1.25, 0.0)})
    T = PR.tables(7, [6], {5: (2, 1.25, 0.0)})
    for g, w_ in zip(pm.tables(), T):
        assert np.array_equal(g, w_)
    t, y, xt, x0 = PC.problems(kind, K, B, m)
    full = PC.full_start(T, xt, x0)
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    cf, cj, cctx = ds.curve_launchers(kind, K, B, dt, dy)
    ef, ej, ectx = ds.expr_launchers(e, dt, dy)
    wcf, wcj, wcctx = ds.pmap_launchers(pm, cf, cj, cctx, dfull)
    wef, wej, wectx = ds.pmap_launchers(pm, ef, ej, ectx, dfull)
    o = ds.options(max_evals=PC.MAX_EVALS)
    xc, xe = ds.pmap_gather(pm, dfull), ds.pmap_gather(pm, dfull)
    fc, ibc, stc = ds.lm_solve_batch_device(wcf, wcctx, m, xc, opts=o)
    fe, ibe, ste = ds.lm_solve_batch_device(wef, wectx, m, xe, opts=o)
    assert _eq(xc, xe) and _eq(fc, fe) and ibc == ibe and stc == ste and set(ste) == {0}
    for a, b in zip(ds.lm_covariance_batch_device(wcf, wcctx, m, xc), ds.lm_covariance_batch_device(wef, wectx, m, xe)):
        assert _eq(a, b)
    prog = e.program()
    plist = [0, 5, 5, PC.NPROB - 1]
    X = xe.cpu().numpy()[plist]
    J = _launch(ds, wej, wectx, plist, X, m, jac=True)
    for q, p in enumerate(plist):
        want = PR.contract(T, XR.jacobian(prog, PR.expand(T, X[q], full[p]), t[p][None])).T
        assert np.array_equal(_bits(J[q]), _bits(want)), q
    # the analytic solve through the formula: the oracle's, with those callbacks
    xa = ds.pmap_gather(pm, dfull)
    fa, iba, sta = ds.lm_solve_batch_device(wef, wectx, m, xa, jac=wej, opts=o)
    assert set(sta) == {0}
    for c in (wcctx, wectx):
        c.close()


# ------------------------------------------------------------------------------------------------ 5. the composition
def _fit_by_hand(ds, pm, T, launchers, dfull, m, analytic, o, lower=None, upper=None, weights_zero=None):
    """gather, solve, covariance, expand, cov_expand of the restatement."""
    fcn, jac, ctx = launchers
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, dfull)
    j = wj if analytic else None
    x = ds.pmap_gather(pm, dfull)
    f2f = T[4]
    if lower is not None or upper is not None:
        fvec, ibs, st = ds.cls_solve_batch_device(wf, wctx, m, x, jac=j, opts=o, lower=None if lower is None else lower[f2f],
                                                  upper=None if upper is None else upper[f2f])
    else:
        fvec, ibs, st = ds.lm_solve_batch_device(wf, wctx, m, x, jac=j, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=j, scaled=True)
    p = ds.pmap_expand(pm, x, dfull)
    wctx.close()
    return p, fvec, sigma.cpu().numpy(), cov.cpu().numpy(), chi2, rank, ibs, st


def _check_composition(ds, T, got, want, N, n):
    assert _eq(got[0], want[0]) and _eq(got[1], want[1]) and got[6] == want[6] and got[7] == want[7]
    sg, cg, qg, rg = got[2].cpu().numpy(), got[3].cpu().numpy(), got[4].cpu().numpy(), got[5].cpu().numpy()
    qw, rw = want[4].cpu().numpy(), want[5].cpu().numpy()
    assert sg.shape[1:] == (N,) and cg.shape[1:] == (N, N)
    for p, st in enumerate(got[7]):
        if st != 0:                                                     # NaN and rank -1 pass through to every entry
            assert np.isnan(sg[p]).all() and np.isnan(cg[p]).all() and np.isnan(qg[p]) and rg[p] == -1
            continue
        wc, ws = PR.cov_expand(T, want[3][p], want[2][p])
        assert np.array_equal(_bits(cg[p]), _bits(wc)) and np.array_equal(_bits(sg[p]), _bits(ws)), p
        assert _bits(qg[p]) == _bits(qw[p]) and rg[p] == rw[p] == n


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("case,mp", [PC.PAIRS[1], PC.PAIRS[2], PC.PAIRS[4]])
def test_curve_fit_batch_is_the_composition(ds, case, mp, analytic, bounded):
    kind, K, B, m = case
    N = R.nparams(R.KINDS[kind], K, B)
    t, y, xt, x0 = PC.problems(kind, K, B, m)
    T = PR.tables(N, *PC.map_spec(mp, K, B))
    n = len(T[4])
    pm = _pmap(T)
    full = PC.full_start(T, xt, x0)
    full[:, T[0] == PR.TIED] = 1e300                                    # tied positions are ignored on entry
    lower = upper = None
    if bounded:
        lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
        lower[T[0] != PR.FREE], upper[T[0] != PR.FREE] = np.nan, np.nan  # bound entries at fixed and tied positions are not read
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    keep = dfull.clone()
    o = ds.options(max_evals=PC.MAX_EVALS)
    got = ds.curve_fit_batch(kind, dt, dy, dfull, ncomp=K, baseline=B, lower=lower, upper=upper, analytic=analytic, opts=o, pmap=pm)
    assert _eq(dfull, keep)
    want = _fit_by_hand(ds, pm, T, ds.curve_launchers(kind, K, B, dt, dy), dfull, m, analytic, o, lower, upper)
    _check_composition(ds, T, got, want, N, n)
    assert bounded or set(got[7]) == {0}
    xg = got[0].cpu().numpy()
    assert np.array_equal(_bits(xg[:, T[0] == PR.FIXED]), _bits(full[:, T[0] == PR.FIXED]))
    for k in np.flatnonzero(T[0] == PR.TIED):
        assert np.array_equal(_bits(xg[:, k]), _bits(T[2][k] * xg[:, T[1][k]] + T[3][k]))
    # without errors: the solve alone
    x2, f2, s2, c2, q2, r2, ib2, st2 = ds.curve_fit_batch(kind, dt, dy, dfull, ncomp=K, baseline=B, lower=lower, upper=upper,
                                                          analytic=analytic, covariance=False, opts=o, pmap=pm)
    assert _eq(x2, want[0]) and _eq(f2, want[1]) and s2 is c2 is q2 is r2 is None and ib2 == want[6] and st2 == want[7]


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
def test_expr_fit_batch_is_the_composition(ds, analytic, bounded):
    kind, K, B, m = "lorentz", 2, 0, 200
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    pm = nl.ParamMap.for_expr(e, fixed=("c", "m1"), tied={"w2": ("w1", 1.25, 0.0)})
    T = PR.tables(7, [1, 6], {5: (2, 1.25, 0.0)})
    t, y, xt, x0 = PC.problems(kind, K, B, m)
    full = PC.full_start(T, xt, x0)
    lower = upper = None
    if bounded:
        lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    o = ds.options(max_evals=PC.MAX_EVALS)
    got = ds.expr_fit_batch(e, dt, dy, dfull, lower=lower, upper=upper, analytic=analytic, opts=o, pmap=pm)
    want = _fit_by_hand(ds, pm, T, ds.expr_launchers(e, dt, dy), dfull, m, analytic, o, lower, upper)
    _check_composition(ds, T, got, want, 7, pm.nfree)
    assert bounded or set(got[7]) == {0}


def test_no_map_is_the_old_entry_point(ds):
    kind, K, B, m = "lorentz", 2, 0, 200
    t, y, xt, x0 = PC.problems(kind, K, B, m)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=PC.MAX_EVALS)
    old = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, opts=o)
    nprob, n = x0.shape
    x = dx0.clone()
    fvec = torch.empty((nprob, m), dtype=torch.float64, device=ds.device)
    sigma, cov = torch.empty((nprob, n), dtype=torch.float64, device=ds.device), torch.empty((nprob, n, n), dtype=torch.float64, device=ds.device)
    chi2, rank = torch.empty((nprob,), dtype=torch.float64, device=ds.device), torch.empty((nprob,), dtype=torch.int32, device=ds.device)
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    rc = ds.lib.nlh_curve_fit_batch_pmap(ds.h.ptr, C.byref(o), R.LORENTZ, K, B, nprob, m, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                         None, x.data_ptr(), fvec.data_ptr(), sigma.data_ptr(), cov.data_ptr(), chi2.data_ptr(),
                                         rank.data_ptr(), ib, st)
    assert rc == 0
    for g, w_ in zip((x, fvec, sigma, cov, chi2, rank), old[:6]):
        assert _eq(g, w_)
    assert [ib[p].as_dict() for p in range(nprob)] == old[6] and list(st) == old[7]
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    olde = ds.expr_fit_batch(e, dt, dy, dx0, opts=o)
    x = dx0.clone()
    rc = ds.lib.nlh_expr_fit_batch_pmap(ds.h.ptr, C.byref(o), e.ptr, nprob, m, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None, None,
                                        x.data_ptr(), fvec.data_ptr(), sigma.data_ptr(), cov.data_ptr(), chi2.data_ptr(), rank.data_ptr(), ib, st)
    assert rc == 0
    for g, w_ in zip((x, fvec, sigma, cov, chi2, rank), olde[:6]):
        assert _eq(g, w_)


def test_fit_zero_weight_padding_and_dof_on_nfree(ds):
    """Ragged spectra padded with zero weights through a map: dof = count(w != 0) - nfree.  A problem with nfree < count <= N
    rows is solved (the unmapped fit refuses it); one with count <= nfree gets the status and NaNs, it alone, and keeps its x."""
    kind, K, B, m, nprob = "lorentz", 1, 1, 96, 24
    N = R.nparams(R.LORENTZ, K, B)                                      # 5
    T = PR.tables(N, [3, 4], {})                                        # the baseline fixed: nfree = 3
    n = 3
    pm = _pmap(T)
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob, seed=5)
    rng = np.random.default_rng(8)
    w = np.ones((nprob, m))
    length = rng.integers(72, m + 1, nprob)
    length[3], length[7], length[nprob - 1] = n, n - 1, m              # dof 0, dof < 0, no padding
    for p in range(nprob):
        w[p, length[p]:] = 0.0
        y[p, length[p]:] = 1e3                                          # what lies under the padding does not matter
    # problem 11: N = 5 non-zero weights spread over the peak -- more than nfree, not more than N
    w[11] = 0.0
    w[11, [30, 40, 48, 56, 66]] = 1.0
    length[11] = 5
    full = PC.full_start(T, xt, x0)
    dt, dy, dw, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, w), _dev(ds, full)
    o = ds.options(max_evals=CC.MAX_EVALS)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch(kind, dt, dy, dfull, ncomp=K, baseline=B, weights=dw, opts=o, pmap=pm)
    bad = [3, 7]
    good = [p for p in range(nprob) if p not in bad]
    assert [st[p] for p in bad] == [NL_INVALID_INPUT_ERROR] * 2 and st[11] != NL_INVALID_INPUT_ERROR
    old = ds.curve_fit_batch(kind, dt, dy, dfull, ncomp=K, baseline=B, weights=dw, opts=o)
    assert old[7][11] == NL_INVALID_INPUT_ERROR
    xh, fh, sh, ch, qh, rh = (v.cpu().numpy() for v in (x, fvec, sigma, cov, chi2, rank))
    for p in bad:
        assert np.isnan(sh[p]).all() and np.isnan(ch[p]).all() and np.isnan(qh[p]) and rh[p] == -1
        assert np.array_equal(_bits(xh[p]), _bits(full[p])) and ibs[p]["fcn_count"] == 0
    gi = torch.tensor(good, device=ds.device)
    hand = _fit_by_hand(ds, pm, T, ds.curve_launchers(kind, K, B, dt[gi].contiguous(), dy[gi].contiguous(), dw[gi].contiguous()),
                        dfull[gi].contiguous(), m, True, o)
    hx, hf = hand[0].cpu().numpy(), hand[1].cpu().numpy()
    for k, p in enumerate(good):
        assert st[p] == hand[7][k] and ibs[p] == hand[6][k]
        assert np.array_equal(_bits(xh[p]), _bits(hx[k])) and np.array_equal(_bits(fh[p]), _bits(hf[k]))
        if st[p] != 0:
            continue
        dof = int((w[p] != 0).sum()) - n
        s = 0.0
        for v in fh[p]:
            s = s + v * v
        assert _bits(qh[p]) == _bits(s / float(dof)), p
        wc = hand[3][k] * (float(m - n) / float(dof))
        cf, sf = PR.cov_expand(T, wc, np.sqrt(np.diag(wc)))
        assert np.array_equal(_bits(ch[p]), _bits(cf)) and np.array_equal(_bits(sh[p]), _bits(sf)), p
    assert {st[p] for p in good if p != 11} == {0}


# ------------------------------------------------------------------------------------------------ 6. alone and in a batch
def test_alone_and_inside_a_batch_of_300(ds):
    """300 problems reach the sub-batches (concurrent calls of the wrapping launchers on different streams)."""
    kind, K, B, m, nprob = "lorentz", 2, 0, 64, 300
    N = R.nparams(R.LORENTZ, K, B)
    T = PR.tables(N, [6], {5: (2, 1.25, 0.0)})
    pm = _pmap(T)
    t, y, xt, x0 = PC.problems(kind, K, B, m, nprob=nprob, seed=77)
    full = PC.full_start(T, xt, x0)
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    o = ds.options(max_evals=PC.MAX_EVALS)
    big = None
    for analytic in (True, False):
        for form in (None, "row"):
            with _env(NLH_PMAP_FORM=form):
                big = ds.curve_fit_batch(kind, dt, dy, dfull, ncomp=K, baseline=B, analytic=analytic, opts=o, pmap=pm)
                for p in (0, 137, nprob - 1):
                    one = ds.curve_fit_batch(kind, dt[p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dfull[p:p + 1].contiguous(),
                                             ncomp=K, baseline=B, analytic=analytic, opts=o, pmap=pm)
                    for g, w_ in zip(one[:6], big[:6]):
                        assert _eq(g, w_[p:p + 1]), (analytic, form, p)
                    assert one[6][0] == big[6][p]
    # the host-array twin of the last (forward differences)
    xh, fh = full.copy(), np.zeros((nprob, m))
    sh, ch, qh, rh = np.zeros((nprob, N)), np.zeros((nprob, N, N)), np.zeros(nprob), np.zeros(nprob, dtype=np.int32)
    ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
    rc = ds.lib.nlh_curve_fit_batch_pmap_h(ds.h.ptr, C.byref(o), R.LORENTZ, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None,
                                           0, None, None, pm.ptr, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                           ch.ctypes.data_as(dp), qh.ctypes.data_as(dp), rh.ctypes.data_as(_lib.c_int32_p), ib, st)
    assert rc == 0
    for g, w_ in zip((xh, fh, sh, ch, qh), big[:5]):
        assert np.array_equal(_bits(g), _bits(w_.cpu().numpy()))
    assert np.array_equal(rh, big[5].cpu().numpy()) and [ib[p].as_dict() for p in range(nprob)] == big[6]
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    sh2, ch2 = np.zeros((nprob, N)), np.zeros((nprob, N, N))
    xh2, fh2 = full.copy(), np.zeros((nprob, m))
    rc = ds.lib.nlh_expr_fit_batch_pmap_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 0, None,
                                          None, pm.ptr, xh2.ctypes.data_as(dp), fh2.ctypes.data_as(dp), sh2.ctypes.data_as(dp),
                                          ch2.ctypes.data_as(dp), None, None, None, None)
    assert rc == 0                                                      # (the formula's residual bits are the curve model's)
    for g, w_ in zip((xh2, fh2, sh2, ch2), (xh, fh, sh, ch)):
        assert np.array_equal(_bits(g), _bits(w_))


# ------------------------------------------------------------------------------------------------ 7. the model object
@pytest.mark.parametrize("analytic", [0, 1])
@pytest.mark.parametrize("shared", [False, True])
def test_model_object(ds, analytic, shared):
    """nlh_pmap_model_create over a curve model, through _eval, _lm_solve, _cls_solve, _lm_covariance = the launcher forms."""
    (kind, K, B, m), mp = PC.CASES[1], "both"
    N = R.nparams(R.LORENTZ, K, B)
    nprob = 12
    t, y, xt, x0 = PC.problems(kind, K, B, m, nprob=nprob)
    T = PR.tables(N, *PC.map_spec(mp, K, B))
    n = len(T[4])
    pm = _pmap(T)
    full = PC.full_start(T, xt, x0)
    if shared:
        full = np.ascontiguousarray(np.tile(full.mean(0), (nprob, 1)))
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full[0] if shared else full)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, dfull)
    j = wj if analytic else None
    o = ds.options(max_evals=PC.MAX_EVALS)
    inner, md = C.c_void_p(), C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.LORENTZ, K, B, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, analytic,
                                         C.byref(inner)) == 0
    fh_ = np.ascontiguousarray(full[0] if shared else full)
    assert ds.lib.nlh_pmap_model_create(ds.h.ptr, inner, pm.ptr, fh_.ctypes.data_as(dp), int(shared), C.byref(md)) == 0
    try:
        sp, sm, sn = C.c_int32(), C.c_int32(), C.c_int32()
        ds.lib.nlh_dq_model_shape(md, C.byref(sp), C.byref(sm), C.byref(sn))
        assert (sp.value, sm.value, sn.value) == (nprob, m, n)
        xs = PR.gather(T, full)
        f0 = np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_eval(ds.h.ptr, md, xs.ctypes.data_as(dp), f0.ctypes.data_as(dp)) == 0
        assert np.array_equal(_bits(f0), _bits(_launch(ds, wf, wctx, list(range(nprob)), xs, m)))
        for p in range(nprob):
            assert np.array_equal(_bits(f0[p]), _bits(R.residual(R.LORENTZ, K, B, PR.expand(T, xs[p], full[p]), t[p], y[p])))
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        xh, fh = xs.copy(), np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_lm_solve(ds.h.ptr, C.byref(o), md, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, xs)
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=j, opts=o)
        assert np.array_equal(_bits(xh), _bits(x.cpu().numpy())) and np.array_equal(_bits(fh), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(nprob)] == ibs and list(st) == status
        ch, sh, rh, qh = np.zeros((nprob, n, n)), np.zeros((nprob, n)), np.zeros(nprob, dtype=np.int32), np.zeros(nprob)
        assert ds.lib.nlh_dq_model_lm_covariance(ds.h.ptr, md, xh.ctypes.data_as(dp), 1, 0.0, ch.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                                 rh.ctypes.data_as(_lib.c_int32_p), qh.ctypes.data_as(dp)) == 0
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=j)
        assert np.array_equal(_bits(ch), _bits(cov.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sigma.cpu().numpy()))
        assert np.array_equal(rh, rank.cpu().numpy()) and np.array_equal(_bits(qh), _bits(chi2.cpu().numpy()))
        lo, hi = (xt.min(0) - 0.5)[T[4]], (xt.max(0) + 0.5)[T[4]]
        xc, fc = xs.copy(), np.zeros((nprob, m))
        assert ds.lib.nlh_dq_model_cls_solve(ds.h.ptr, C.byref(o), md, 1.0, 1.0, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp),
                                             xc.ctypes.data_as(dp), fc.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, xs)
        fvec, ibs, status = ds.cls_solve_batch_device(wf, wctx, m, x, jac=j, opts=o, lower=lo, upper=hi)
        assert np.array_equal(_bits(xc), _bits(x.cpu().numpy())) and np.array_equal(_bits(fc), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(nprob)] == ibs and list(st) == status
    finally:
        ds.lib.nlh_dq_model_destroy(md)
        ds.lib.nlh_dq_model_destroy(inner)
        wctx.close()


@pytest.fixture(scope="module")
def fortran_pmap_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_pmap")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "pmap_fit")


def test_fortran_pmap_fit(ds, fortran_pmap_exe, tmp_path):
    """The Fortran user program (create_curve -> create_mapped -> solve_batch -> covariance_batch: a Lorentzian doublet with
    tied widths and a fixed baseline) prints the x, sigma and counts of the Python path, digit for digit (ES24.16)."""
    kind, K, B, m, nprob = "lorentz", 2, 0, 120, 6
    ratio = 1.25
    T = PR.tables(7, [6], {5: (2, ratio, 0.0)})
    pm = _pmap(T)
    t, y, xt, x0 = PC.problems(kind, K, B, m, nprob=nprob, seed=31)
    full = PC.full_start(T, xt, x0)
    path = str(tmp_path / "doublets.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m], dtype=np.int32).tobytes())
        fh.write(np.array([ratio]).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(full.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_pmap_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    o = ds.options(max_evals=PC.MAX_EVALS)
    dt, dy, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, full)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, dfull)
    x = ds.pmap_gather(pm, dfull)
    fvec, ibs, st = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, x, jac=wj)
    xh, sh = x.cpu().numpy(), sigma.cpu().numpy()
    want = []
    for p in range(nprob):
        want.append("x %d" % (p + 1) + "".join("%24.16E" % v for v in xh[p]))
        want.append("sigma %d" % (p + 1) + "".join("%24.16E" % v for v in sh[p]))
        want.append("counts %d %d %d %d %d" % (p + 1, ibs[p]["iter_count"], ibs[p]["fcn_count"], ibs[p]["jacobian_count"], int(rank[p])))
    lines = [" ".join(ln.split()) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1] == "done"
    assert lines[:-1] == [" ".join(w_.split()) for w_ in want], out.stdout
    # the one-call fit reports the same solution, expanded
    full_fit = ds.curve_fit_batch(kind, dt, dy, dfull, ncomp=K, baseline=B, opts=o, pmap=pm)
    assert _eq(full_fit[0], ds.pmap_expand(pm, x, dfull)) and full_fit[6] == ibs
    wctx.close()


# ------------------------------------------------------------------------------------------------ 8. error returns
def test_error_returns(ds):
    """In the documented order; nothing is written where a call is refused."""
    kind, K, B, m, nprob = "lorentz", 2, 0, 6, 2                       # N = 7 > m = 6 >= nfree = 5
    t, y, xt, x0 = CC.curve_problems(kind, K, B, m, nprob=nprob)
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    pm = nl.ParamMap(7, fixed=(6,), tied={5: (2, 1.25, 0.0)})           # nfree 5
    pm6 = nl.ParamMap(7, fixed=(6,))                                    # nfree 6 = m
    pm4 = nl.ParamMap(4)
    f = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)
    s = torch.full((nprob, 7), 7.0, dtype=torch.float64, device=ds.device)

    def fit(kd, KK, BB, mm, p, sigma=None, x=dx, h=ds.h.ptr):
        return ds.lib.nlh_curve_fit_batch_pmap(h, C.byref(o), kd, KK, BB, nprob, mm, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                               p.ptr, x.data_ptr() if x is not None else None, f.data_ptr(), sigma, None, None, None, None, None)
    assert fit(1, K, B, m, pm, h=None) == -3                            # NLH_ERR_BAD_HANDLE first
    assert fit(7, K, B, m, pm) == NL_INVALID_INPUT_ERROR and fit(1, 0, B, m, pm) == NL_INVALID_INPUT_ERROR
    assert fit(1, K, B, m, pm4) == NL_INVALID_INPUT_ERROR               # a map of another model
    assert fit(1, K, B, 4, pm) == NL_UNDERDEFINED_PROBLEM_ERROR         # m < nfree
    assert fit(1, K, B, m, pm, x=None) == NL_INVALID_INPUT_ERROR        # a NULL array
    assert fit(1, K, B, m, pm6, s.data_ptr()) == NL_INVALID_INPUT_ERROR  # errors asked for with m <= nfree
    torch.cuda.synchronize()
    assert (f == 7.0).all() and (s == 7.0).all() and torch.equal(dx, _dev(ds, x0))
    assert fit(1, K, B, m, pm, s.data_ptr()) == 0                       # N = 7 > m = 6 > nfree = 5: the count that matters is nfree
    assert ds.lib.nlh_curve_fit_batch(ds.h.ptr, C.byref(o), 1, K, B, nprob, m, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                      dx.data_ptr(), f.data_ptr(), None, None, None, None, None, None) == NL_UNDERDEFINED_PROBLEM_ERROR
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    assert ds.lib.nlh_expr_fit_batch_pmap(ds.h.ptr, C.byref(o), e.ptr, nprob, m, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                          pm4.ptr, dx.data_ptr(), f.data_ptr(), None, None, None, None, None, None) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_expr_fit_batch_pmap(ds.h.ptr, C.byref(o), e.ptr, nprob, 4, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                          pm.ptr, dx.data_ptr(), f.data_ptr(), None, None, None, None, None, None) == NL_UNDERDEFINED_PROBLEM_ERROR
    # the wrapping context and its launchers
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    out = C.c_void_p(7)
    none = C.cast(None, _lib.DEVFCN)
    assert ds.lib.nlh_pmap_wrap(ds.h.ptr, None, fcn, jac, ds._ctxp(ctx), dx.data_ptr(), 0, C.byref(out)) == NL_INVALID_INPUT_ERROR and not out.value
    assert ds.lib.nlh_pmap_wrap(ds.h.ptr, pm.ptr, none, jac, ds._ctxp(ctx), dx.data_ptr(), 0, C.byref(out)) == NL_UNDEFINED_FUNCTION_ERROR
    assert ds.lib.nlh_pmap_wrap(ds.h.ptr, pm.ptr, fcn, jac, ds._ctxp(ctx), None, 0, C.byref(out)) == NL_INVALID_INPUT_ERROR   # fixed values needed
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, None, ctx, dx)
    assert wj is None
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    X = ds.pmap_gather(pm, dx)
    J = torch.full((nprob, 5, m), 7.0, dtype=torch.float64, device=ds.device)
    args = lambda n_, m_: (wctx.ptr, stream, nprob, None, n_, C.c_void_p(X.data_ptr()), m_, C.c_void_p(J.data_ptr()))
    assert ds.lib.nlh_pmap_device_fcn(*args(7, m)) == NL_INVALID_INPUT_ERROR        # n != nfree
    assert ds.lib.nlh_pmap_device_fcn(*args(5, 0)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_pmap_device_jac(*args(5, m)) == NL_UNDEFINED_FUNCTION_ERROR   # no inner Jacobian launcher
    assert ds.lib.nlh_pmap_device_fcn(*args(5, m + 1)) == NL_INVALID_INPUT_ERROR    # the inner launcher's refusal (m != ctx.m) comes back
    torch.cuda.synchronize()
    assert (J == 7.0).all()
    with pytest.raises(RuntimeError):                                   # a solve with the wrong n aborts, launching nothing
        ds.lm_solve_batch_device(wf, wctx, m, dx.clone())
    wctx.close()
    # the model object
    md, inner = C.c_void_p(7), C.c_void_p()
    A, b = np.ones((1, 2, 2)), np.ones((1, 2))
    assert ds.lib.nlh_dq_model_create(ds.h.ptr, 1, 2, 2, A.ctypes.data_as(dp), b.ctypes.data_as(dp), 0.5, C.byref(inner)) == 0
    pm2 = nl.ParamMap(2, fixed=(1,))
    one = np.ones(8)
    assert ds.lib.nlh_pmap_model_create(ds.h.ptr, inner, pm2.ptr, one.ctypes.data_as(dp), 1, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    ds.lib.nlh_dq_model_destroy(inner)                                  # (a dense-quadratic model has no launchers to wrap)
    inner = C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, 1, K, B, nprob, 7, np.ones((nprob, 7)).ctypes.data_as(dp), 0,
                                         np.ones((nprob, 7)).ctypes.data_as(dp), None, 1, C.byref(inner)) == 0
    assert ds.lib.nlh_pmap_model_create(ds.h.ptr, inner, pm4.ptr, one.ctypes.data_as(dp), 1, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    assert ds.lib.nlh_pmap_model_create(ds.h.ptr, inner, pm.ptr, None, 1, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    assert ds.lib.nlh_pmap_model_create(ds.h.ptr, inner, pm.ptr, one.ctypes.data_as(dp), 1, C.byref(md)) == 0 and md.value
    ds.lib.nlh_dq_model_destroy(md)
    ds.lib.nlh_dq_model_destroy(inner)


# ------------------------------------------------------------------------------------------------ 9. the edges of the rules
def test_refused_problem_leaves_the_expansion_of_its_x(ds):
    """On exit dx obeys the map for every problem: one refused on its degrees of freedom keeps its free and fixed values, and
    its tied positions -- ignored on entry -- hold the ties evaluated at them."""
    kind, K, B, m, nprob = "lorentz", 2, 0, 64, 3
    T = PR.tables(7, [6], {5: (2, 1.25, 0.0)})                          # nfree = 5
    pm = _pmap(T)
    t, y, xt, x0 = PC.problems(kind, K, B, m, nprob=nprob)
    full = PC.full_start(T, xt, x0)
    full[:, 5] = -77.0                                                  # tied positions on entry: not read
    w = np.ones((nprob, m))
    w[1] = 0.0
    w[1, [10, 20, 30, 40, 50]] = 1.0                                    # problem 1: nfree non-zero weights, dof 0
    dt, dy, dw, dfull = _dev(ds, t), _dev(ds, y), _dev(ds, w), _dev(ds, full)
    o = ds.options(max_evals=PC.MAX_EVALS)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch(kind, dt, dy, dfull, ncomp=K, baseline=B, weights=dw, opts=o, pmap=pm)
    assert st[1] == NL_INVALID_INPUT_ERROR and ibs[1]["fcn_count"] == 0 and NL_INVALID_INPUT_ERROR not in (st[0], st[2])
    xh = x.cpu().numpy()
    assert np.array_equal(_bits(xh[1]), _bits(PR.expand(T, PR.gather(T, full[1]), full[1])))
    assert _bits(xh[1, 5]) == _bits(1.25 * full[1, 2]) and np.isnan(sigma[1].cpu().numpy()).all()
    for p in (0, 2):
        assert _bits(xh[p, 5]) == _bits(1.25 * xh[p, 2]) and _bits(xh[p, 6]) == _bits(full[p, 6])


def test_expand_without_fixed_parameters_needs_no_full(ds):
    """nlh_pmap_expand_batch follows nlh_pmap_wrap: full is read at fixed positions only, so a map without one takes NULL."""
    T = PR.tables(5, [], {3: (1, -0.5, 2.0)})
    pm = _pmap(T)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((9, 4))
    dx = _dev(ds, x)
    p = torch.full((9, 5), 7.0, dtype=torch.float64, device=ds.device)
    assert ds.lib.nlh_pmap_expand_batch(ds.h.ptr, pm.ptr, 9, dx.data_ptr(), None, 0, p.data_ptr()) == 0
    torch.cuda.synchronize()
    want = np.stack([PR.expand(T, x[q], np.zeros(5)) for q in range(9)])
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(want))
    pmf = nl.ParamMap(5, fixed=(0,))
    q = torch.full((9, 5), 7.0, dtype=torch.float64, device=ds.device)
    assert ds.lib.nlh_pmap_expand_batch(ds.h.ptr, pmf.ptr, 9, dx.data_ptr(), None, 0, q.data_ptr()) == NL_INVALID_INPUT_ERROR
    torch.cuda.synchronize()
    assert (q == 7.0).all()


def test_python_refuses_a_map_of_another_model(ds):
    kind, K, B, m = "lorentz", 2, 0, 64
    t, y, xt, x0 = PC.problems(kind, K, B, m, nprob=2)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    with pytest.raises(ValueError, match="4 parameters"):
        ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, pmap=nl.ParamMap(4))
    with pytest.raises(ValueError, match="4 parameters"):
        ds.expr_fit_batch(nl.Expr(FORMULA, ("t",), PARAMS), dt, dy, dx0, pmap=nl.ParamMap(4))
