"""GPU tests of the global fits (include/nonlin_hip.h: nlh_group_*), everything bit for bit: the kernels against the numpy
restatement (tests/group_restatement.py) through the wrapping launchers, in both workgroup forms, with and without the column
split, sliced and unsliced; G = 1 with nothing shared against the unwrapped launchers; solves through the wrapper against the
CPU oracle on the restated stacked problem; the group around the Poisson pair, a loss and a parameter map; the one-call fits
as the composition they stand for; a group alone against the same group inside a batch of 300; the degrees-of-freedom rule;
the model object; the error returns.  The bitwise tests use the Lorentzian and exp-free formulas only."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import curve_cases as CC
import curve_restatement as R
import group_cases as GC
import group_restatement as GR
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

dp = C.POINTER(C.c_double)
KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
FORMS = [None, "row", "flat"]               # None: the form m selects; a forced form that cannot hold m falls back to it
NL_INVALID_INPUT_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR = 201, 211, 212
FORMULA = "a1/(1+((t-m1)/w1)^2) + a2/(1+((t-m2)/w2)^2) + c"
PARAMS = ("a1", "m1", "w1", "a2", "m2", "w2", "c")
KIND, K, B, N = "lorentz", 2, 0, 7          # the model of the kernel tests: two Lorentzians on a constant
SHARED_SETS = [(), tuple(range(N)), (1, 4)]  # none, all, and a non-leading pair: the peak positions


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


class _env:
    """Environment variables for the calls inside (the library reads NLH_GROUP_* at every call); None: unset."""

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
    q): F [npoints, m] or J [npoints, n, m], pre-filled with NaN."""
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


def _group(T):
    """The library's group of a restatement's tables."""
    N_, sidx, lidx, G = T
    return nl.Group(N_, shared=[int(k) for k in sidx[::-1]], nsets=G)    # (given in descending order: the order does not matter)


def _stack_want(T, P, rows, resid, jacob):
    """F [npoints, G m] and J [npoints, n, G m] of the restatement: data set g of outer point q is inner problem rows[q] G + g
    at the inner parameters P[q G + g]."""
    G = T[3]
    F = [np.concatenate([resid(p * G + g, P[q * G + g]) for g in range(G)]) for q, p in enumerate(rows)]
    J = [GR.scatter(T, [jacob(p * G + g, P[q * G + g]) for g in range(G)]).T for q, p in enumerate(rows)]
    return F, J


# ------------------------------------------------------------------------------------------------ 1. the kernels
@functools.lru_cache(maxsize=None)
def _kernel_data(m, G):
    """The data and the point lists of one (m, G), shared by the forms: ngroup = 3 groups."""
    ngroup = 3
    t, y, xt, x0 = CC.curve_problems(KIND, K, B, m, nprob=ngroup * G, seed=11 + m + G)
    w = np.random.default_rng(m).uniform(0.5, 2.0, (ngroup * G, m))
    shapes = [[ngroup - 2], [2] * 4, list(np.random.default_rng(3).integers(0, ngroup, 9)) + [0, 0, ngroup - 1], None]
    return ngroup, t, y, w, x0, shapes


@functools.lru_cache(maxsize=None)
def _kernel_want(m, G, shared, k):
    """(X, wantF, wantJ) of point list k: computed once, read by every form, split and slicing."""
    ngroup, t, y, w, x0, shapes = _kernel_data(m, G)
    T = GR.tables(N, shared, G)
    n = GR.nouter(T)
    rows = list(range(ngroup)) if shapes[k] is None else [int(p) for p in shapes[k]]
    X = GR.gather(T, x0)[rows] * (1.0 + 0.01 * np.random.default_rng(k).uniform(-1, 1, (len(rows), n)))
    P = GR.expand(T, X)
    kd = R.LORENTZ
    F, J = _stack_want(T, P, rows, lambda p, q: R.residual(kd, K, B, q, t[p], y[p], w[p]), lambda p, q: R.jacobian(kd, K, B, q, t[p], w[p]))
    return X, F, J


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("G", [1, 2, 3, 5])
@pytest.mark.parametrize("m", [24, 64, 200, 256, 301])
def test_launchers_bitwise(ds, m, G, form):
    """k_group_expand and k_group_jac through the wrapping launchers around the Lorentzian: F = the inner residuals one after
    the other and J = scatter(the inner Jacobians) of the restatements, every entry written over the NaN it held, for every
    shared set, launch shape, form, column split and slicing.  m = 200 and 301 put a data-set boundary inside a wave, m = 24
    with G = 5 several data sets in one wave."""
    ngroup, t, y, w, x0, shapes = _kernel_data(m, G)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    fcn, jac, ctx = ds.curve_launchers(KIND, K, B, dt, dy, dw)
    M = G * m
    for shared in SHARED_SETS:
        T = GR.tables(N, shared, G)
        n = GR.nouter(T)
        grp = _group(T)
        wf, wj, wctx = ds.group_launchers(grp, fcn, jac, ctx)
        for k, plist in enumerate(shapes):
            X, wantF, wantJ = _kernel_want(m, G, shared, k)
            # (split: column groups; scratch: a cap that cuts the call into slices of one (fcn) or two (jac) outer points)
            per = 8 * (G * N * (m + 1) + (G + 1) // 2) + 4
            for split, sliced in ((sp, sl) for sp in (None, 1, 2, n) for sl in (False, True)):
                with _env(NLH_GROUP_FORM=form, NLH_GROUP_SPLIT=split, NLH_GROUP_SCRATCH=64 if sliced else None):
                    F = _launch(ds, wf, wctx, plist, X, M)
                with _env(NLH_GROUP_FORM=form, NLH_GROUP_SPLIT=split, NLH_GROUP_SCRATCH=2 * per + 16 if sliced else None):
                    J = _launch(ds, wj, wctx, plist, X, M, jac=True)
                for q in range(len(X)):
                    assert np.array_equal(_bits(F[q]), _bits(wantF[q])), (shared, form, k, q, split, sliced)
                    assert np.array_equal(_bits(J[q]), _bits(wantJ[q])), (shared, form, k, q, split, sliced)
        wctx.close()


def test_gather_expand_sigma_bitwise(ds):
    rng = np.random.default_rng(21)
    for nfull, shared, G in ((7, (1, 4), 3), (7, (), 2), (4, (0, 1, 2, 3), 5), (3, (1,), 8), (33, (32, 5, 17), 6), (5, (4,), 1)):
        T = GR.tables(nfull, shared, G)
        grp = _group(T)
        n, ngroup = GR.nouter(T), 37
        full = rng.standard_normal((ngroup * G, nfull))
        x = rng.standard_normal((ngroup, n))
        assert np.array_equal(_bits(ds.group_gather(grp, _dev(ds, full)).cpu().numpy()), _bits(GR.gather(T, full)))
        assert np.array_equal(_bits(ds.group_expand(grp, _dev(ds, x)).cpu().numpy()), _bits(GR.expand(T, x)))
        sigma = np.abs(x)
        fail = (rng.uniform(size=ngroup) < 0.2).astype(np.int32)
        want = GR.expand(T, sigma)
        got = ds.group_sigma(grp, _dev(ds, sigma)).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want))
        got = ds.group_sigma(grp, _dev(ds, sigma), _dev(ds, fail)).cpu().numpy().reshape(ngroup, G, nfull)
        want = want.reshape(ngroup, G, nfull)
        assert np.isnan(got[fail != 0]).all() and np.array_equal(_bits(got[fail == 0]), _bits(want[fail == 0]))


# ------------------------------------------------------------------------------------------------ 2. G = 1, nothing shared
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("kind,K_,B_,m", [CC.CASES[3], CC.CASES[4]])
def test_group_of_one_equals_the_unwrapped_launchers(ds, kind, K_, B_, m, analytic):
    n = R.nparams(R.KINDS[kind], K_, B_)
    t, y, xt, x0 = CC.curve_problems(kind, K_, B_, m, nprob=12)
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.curve_launchers(kind, K_, B_, dt, dy)
    grp = nl.Group(n, shared=(), nsets=1)
    assert grp.nouter == n
    wf, wj, wctx = ds.group_launchers(grp, fcn, jac, ctx)
    for plist in (None, [3, 3, 0, 11]):
        X = x0 if plist is None else x0[plist]
        rows = list(range(12)) if plist is None else plist              # (the curve launchers themselves take a problem list)
        assert np.array_equal(_bits(_launch(ds, wf, wctx, plist, X, m)), _bits(_launch(ds, fcn, ctx, rows, X, m)))
        assert np.array_equal(_bits(_launch(ds, wj, wctx, plist, X, m, jac=True)), _bits(_launch(ds, jac, ctx, rows, X, m, jac=True)))
    o = ds.options(max_evals=CC.MAX_EVALS)
    xa, xb = _dev(ds, x0), _dev(ds, x0)
    fa, iba, sta = ds.lm_solve_batch_device(fcn, ctx, m, xa, jac=jac if analytic else None, opts=o)
    fb, ibb, stb = ds.lm_solve_batch_device(wf, wctx, m, xb, jac=wj if analytic else None, opts=o)
    assert _eq(xa, xb) and _eq(fa, fb) and iba == ibb and sta == stb
    wctx.close()


# ------------------------------------------------------------------------------------------------ 3. the oracle
def _stacked_callbacks(T, kd, K_, B_, t, y, analytic):
    f, j = GR.stacked(T, lambda g, q: R.residual(kd, K_, B_, q, t[g], y[g]), lambda g, q: R.jacobian(kd, K_, B_, q, t[g]))
    return f, (j if analytic else None)


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("case", GC.CASES)
def test_solves_against_oracle(ds, oracle, case, analytic, bounded):
    """lm_solve (bounded: cls_solve) on the restated stacked problem, every group: status, x, fvec and every
    count identical.  With forward differences the inner launcher is asked for exactly G (fcn_count + n jacobian_count) points:
    n perturbed evaluations per Jacobian, each of G inner points, beside the ones fcn_count counts."""
    kind, K_, B_, m, G, shared = case
    kd, N_ = R.KINDS[kind], R.nparams(R.KINDS[kind], K_, B_)
    t, y, xt, x0 = GC.problems(kind, K_, B_, m, G, shared)
    T = GR.tables(N_, shared, G)
    n, M = GR.nouter(T), G * m
    grp = _group(T)
    lower = upper = None
    if bounded:                                                         # a box some true values lie outside of: bounds that bind
        lower = np.minimum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) - 0.02
        upper = np.maximum(0.9 * xt.mean(0), 1.1 * xt.mean(0)) + 0.02
        x0 = np.clip(x0, lower, upper)
        oi = GR.outer_index(T)
        lo, hi = np.empty(n), np.empty(n)
        lo[oi], hi[oi] = np.broadcast_to(lower, oi.shape), np.broadcast_to(upper, oi.shape)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    fcn, jac, ctx = ds.curve_launchers(kind, K_, B_, dt, dy)
    asked = [0]

    def counting(c, stream, npoints, dprob, nn, dX, mm, dF):
        assert nn == N_ and mm == m
        asked[0] += npoints
        return ds.lib.nlh_curve_device_fcn(c, stream, npoints, dprob, nn, dX, mm, dF)
    inner = _lib.DEVFCN(counting)
    wf, wj, wctx = ds.group_launchers(grp, inner, jac, ctx)
    x = ds.group_gather(grp, dx0)
    assert x.shape == (GC.NGROUP, n)
    opt = dict(max_evals=GC.MAX_EVALS)
    if bounded:
        fvec, ibs, status = ds.cls_solve_batch_device(wf, wctx, M, x, jac=wj if analytic else None, opts=ds.options(**opt), lower=lo, upper=hi)
    else:
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, M, x, jac=wj if analytic else None, opts=ds.options(**opt))
    torch.cuda.synchronize()
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**opt)
    xs = GR.gather(T, x0)
    for p in range(GC.NGROUP):
        d = slice(p * G, (p + 1) * G)
        f, j = _stacked_callbacks(T, kd, K_, B_, t[d], y[d], analytic)
        if bounded:
            rc, xo, fo, ibo = oracle.cls_solve(f, M, n, xs[p], jac=j, opts=oo, lower=lo, upper=hi)
        else:
            rc, xo, fo, ibo = oracle.lm_solve(f, M, n, xs[p], jac=j, opts=oo)
        what = (case, analytic, bounded, p)
        assert status[p] == rc, (what, status[p], rc)
        assert _same(ibs[p], ibo), (what, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), what
    assert set(status) == {0}                                           # (the oracle returns 0 for every one of them, bounded too)
    evals = G * sum(ib["fcn_count"] + (0 if analytic else n * ib["jacobian_count"]) for ib in ibs)
    print(f"group {case} analytic={analytic} bounded={bounded}: n = {n}, inner points asked {asked[0]}, counted {evals}")
    assert asked[0] == evals
    wctx.close()


# ------------------------------------------------------------------------------------------------ 4. wrapper stacks
@pytest.mark.parametrize("stack", ["pois", "loss", "pmap"])
def test_group_around_another_wrapper(ds, stack):
    """group(pois(model)), group(loss(model)) and group(pmap(model)): the restated composition -- the inner pair's own F one
    after the other and scatter of its own J, on the expanded points and the inner problems p G + g -- for a point list with
    repeats and without one.  Every inner context indexes its data (counts and mask, scales, fixed values) by inner problem."""
    m, G, ngroup = 96, 3, 4
    nprob = ngroup * G
    t, y, xt, x0 = CC.curve_problems(KIND, K, B, m, nprob=nprob, seed=5)
    rng = np.random.default_rng(9)
    dt = _dev(ds, t)
    Ni = N
    if stack == "pois":
        yc = rng.poisson(40.0 * np.abs(y) + 3.0).astype(np.float64)
        w = (rng.uniform(size=(nprob, m)) < 0.9).astype(np.float64)
        x0 = x0 * np.array([40.0, 1, 1, 40.0, 1, 1, 1.0]) + np.array([0, 0, 0, 0, 0, 0, 3.0])
        dy, dw = _dev(ds, yc), _dev(ds, w)
        base = ds.curve_launchers(KIND, K, B, dt, dy)
        inner = ds.pois_launchers(nl.Poisson(), base[0], base[1], base[2], dy, dw)
    elif stack == "loss":
        dy = _dev(ds, y + 0.3 * (rng.uniform(size=(nprob, m)) < 0.05))
        base = ds.curve_launchers(KIND, K, B, dt, dy)
        inner = ds.loss_launchers(nl.Loss("huber", rng.uniform(0.005, 0.05, nprob)), base[0], base[1], base[2])
    else:
        dy = _dev(ds, y)
        base = ds.curve_launchers(KIND, K, B, dt, dy)
        pm = nl.ParamMap(7, fixed=(6,), tied={5: (2, 1.25, 0.0)})
        dfull = _dev(ds, x0)
        inner = ds.pmap_launchers(pm, base[0], base[1], base[2], dfull)
        x0 = ds.pmap_gather(pm, dfull).cpu().numpy()
        Ni = pm.nfree
    for shared in ((1,), ()):
        T = GR.tables(Ni, shared, G)
        n, M = GR.nouter(T), G * m
        grp = _group(T)
        wf, wj, wctx = ds.group_launchers(grp, *inner)
        for plist in ([2, 0, 2, 3, 3], None):
            rows = list(range(ngroup)) if plist is None else plist
            X = GR.gather(T, x0)[rows] * (1.0 + 0.01 * rng.uniform(-1, 1, (len(rows), n)))
            P = GR.expand(T, X)
            ilist = [p * G + g for p in rows for g in range(G)]
            Fi = _launch(ds, inner[0], inner[2], ilist, P, m)
            Ji = _launch(ds, inner[1], inner[2], ilist, P, m, jac=True)
            F = _launch(ds, wf, wctx, plist, X, M)
            J = _launch(ds, wj, wctx, plist, X, M, jac=True)
            for q in range(len(rows)):
                assert np.array_equal(_bits(F[q]), _bits(Fi[q * G:(q + 1) * G].ravel())), (stack, shared, q)
                want = GR.scatter(T, [Ji[q * G + g].T for g in range(G)]).T
                assert np.array_equal(_bits(J[q]), _bits(want)), (stack, shared, q)
        wctx.close()
    inner[2].close()


# ------------------------------------------------------------------------------------------------ 5. the composition
def _fit_by_hand(ds, grp, launchers, dx0, M, analytic, o, lo=None, hi=None, scaled=True):
    """gather, solve, covariance, expand, sigma."""
    fcn, jac, ctx = launchers
    wf, wj, wctx = ds.group_launchers(grp, fcn, jac, ctx)
    j = wj if analytic else None
    x = ds.group_gather(grp, dx0)
    if lo is not None or hi is not None:
        fvec, ibs, st = ds.cls_solve_batch_device(wf, wctx, M, x, jac=j, opts=o, lower=lo, upper=hi)
    else:
        fvec, ibs, st = ds.lm_solve_batch_device(wf, wctx, M, x, jac=j, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, M, x, jac=j, scaled=scaled)
    p = ds.group_expand(grp, x)
    sf = ds.group_sigma(grp, sigma, _dev(ds, np.array(st, dtype=np.int32)))
    wctx.close()
    return p, fvec, sf, cov, chi2, rank, ibs, st


def _check_composition(got, want, nprob, m, Ni, n):
    ngroup = len(want[7])
    assert got[0].shape == (nprob, Ni) and got[1].shape == (nprob, m) and got[2].shape == (nprob, Ni) and got[3].shape == (ngroup, n, n)
    assert got[4].shape == (ngroup,) and got[5].shape == (ngroup,) and len(got[6]) == len(got[7]) == ngroup
    assert _eq(got[0], want[0]) and _eq(got[1].reshape(ngroup, -1), want[1]) and got[6] == want[6] and got[7] == want[7]
    sg, cg, qg, rg = (v.cpu().numpy() for v in got[2:6])
    sw, cw, qw, rw = (v.cpu().numpy() for v in want[2:6])
    G = nprob // ngroup
    for p, st in enumerate(got[7]):
        if st != 0:                                                     # NaN and rank -1 pass through to every entry
            assert np.isnan(sg[p * G:(p + 1) * G]).all() and np.isnan(cg[p]).all() and np.isnan(qg[p]) and rg[p] == -1
            continue
        assert np.array_equal(_bits(cg[p]), _bits(cw[p])) and np.array_equal(_bits(sg[p * G:(p + 1) * G]), _bits(sw[p * G:(p + 1) * G])), p
        assert _bits(qg[p]) == _bits(qw[p]) and rg[p] == rw[p] == n


def _outer_bounds(T, lower, upper):
    oi = GR.outer_index(T)
    lo, hi = np.empty(GR.nouter(T)), np.empty(GR.nouter(T))
    lo[oi], hi[oi] = np.broadcast_to(lower, oi.shape), np.broadcast_to(upper, oi.shape)
    return lo, hi


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
@pytest.mark.parametrize("case", GC.CASES)
def test_curve_fit_batch_is_the_composition(ds, case, analytic, bounded):
    kind, K_, B_, m, G, shared = case
    N_ = R.nparams(R.KINDS[kind], K_, B_)
    t, y, xt, x0 = GC.problems(kind, K_, B_, m, G, shared)
    T = GR.tables(N_, shared, G)
    n, M, nprob = GR.nouter(T), G * m, GC.NGROUP * G
    grp = _group(T)
    x0[1::G, list(shared)] = 1e300                                      # a shared parameter starts from data set 0's value
    lower = upper = lo = hi = None
    if bounded:
        lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
        lo, hi = _outer_bounds(T, lower, upper)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    keep = dx0.clone()
    o = ds.options(max_evals=GC.MAX_EVALS)
    got = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, lower=lower, upper=upper, analytic=analytic, opts=o, group=grp)
    assert _eq(dx0, keep)
    want = _fit_by_hand(ds, grp, ds.curve_launchers(kind, K_, B_, dt, dy), dx0, M, analytic, o, lo, hi)
    _check_composition(got, want, nprob, m, N_, n)
    assert bounded or set(got[7]) == {0}
    xg = got[0].cpu().numpy().reshape(GC.NGROUP, G, N_)
    for k in shared:                                                    # on exit a shared parameter is equal across the group
        assert all(np.array_equal(_bits(xg[:, g, k]), _bits(xg[:, 0, k])) for g in range(G))
    sg = got[2].cpu().numpy().reshape(GC.NGROUP, G, N_)
    cg = got[3].cpu().numpy()
    for g in range(G):                                                  # nlh_group_index locates the entries of cov
        for k in range(N_):
            jj = grp.index(g, k)
            assert np.array_equal(_bits(sg[:, g, k]), _bits(np.sqrt(cg[:, jj, jj])))
    # without errors: the solve alone
    x2, f2, s2, c2, q2, r2, ib2, st2 = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, lower=lower, upper=upper,
                                                          analytic=analytic, covariance=False, opts=o, group=grp)
    assert _eq(x2, want[0]) and _eq(f2.reshape(GC.NGROUP, -1), want[1]) and s2 is c2 is q2 is r2 is None and ib2 == want[6] and st2 == want[7]


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
def test_expr_fit_batch_is_the_composition(ds, analytic, bounded):
    kind, K_, B_, m, G, shared = GC.CASES[0]
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    grp = nl.Group.for_expr(e, shared=("m2", "m1"), nsets=G)
    T = GR.tables(7, shared, G)
    assert [grp.index(g, k) for g in range(G) for k in range(7)] == list(GR.outer_index(T).ravel())
    t, y, xt, x0 = GC.problems(kind, K_, B_, m, G, shared)
    n, M, nprob = GR.nouter(T), G * m, GC.NGROUP * G
    lower = upper = lo = hi = None
    if bounded:
        lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
        lo, hi = _outer_bounds(T, lower, upper)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=GC.MAX_EVALS)
    got = ds.expr_fit_batch(e, dt, dy, dx0, lower=lower, upper=upper, analytic=analytic, opts=o, group=grp)
    want = _fit_by_hand(ds, grp, ds.expr_launchers(e, dt, dy), dx0, M, analytic, o, lo, hi)
    _check_composition(got, want, nprob, m, 7, n)
    assert bounded or set(got[7]) == {0}


def test_fit_with_a_loss_and_with_the_poisson_deviance(ds):
    """The loss (one scale per DATA SET) and the Poisson pair wrap the model per data set, the group wraps the result."""
    kind, K_, B_, m, G, shared = GC.CASES[0]
    N_ = 7
    t, y, xt, x0 = GC.problems(kind, K_, B_, m, G, shared)
    T = GR.tables(N_, shared, G)
    n, M, nprob = GR.nouter(T), G * m, GC.NGROUP * G
    grp = _group(T)
    rng = np.random.default_rng(4)
    o = ds.options(max_evals=GC.MAX_EVALS)
    dt, dx0 = _dev(ds, t), _dev(ds, x0)
    yo = y + 0.3 * (rng.uniform(size=y.shape) < 0.03)
    dy = _dev(ds, yo)
    for loss in (nl.Loss("huber", rng.uniform(0.004, 0.02, nprob)), nl.Loss("soft_l1", 0.01)):
        got = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, opts=o, group=grp, loss=loss)
        base = ds.curve_launchers(kind, K_, B_, dt, dy)
        inner = ds.loss_launchers(loss, *base)
        want = _fit_by_hand(ds, grp, inner, dx0, M, True, o)
        _check_composition(got, want, nprob, m, N_, n)
        inner[2].close()
    scale = np.array([40.0, 1, 1, 40.0, 1, 1, 1.0])
    yc = rng.poisson(np.stack([R.model(R.LORENTZ, K_, B_, xt[p] * scale + np.array([0, 0, 0, 0, 0, 0, 3.0]), t[p]) for p in range(nprob)])).astype(np.float64)
    w = (rng.uniform(size=yc.shape) < 0.95).astype(np.float64)
    dyc, dw = _dev(ds, yc), _dev(ds, w)
    dxc = _dev(ds, x0 * scale + np.array([0, 0, 0, 0, 0, 0, 3.0]))
    got = ds.curve_fit_batch(kind, dt, dyc, dxc, ncomp=K_, baseline=B_, weights=dw, opts=o, group=grp, stat=nl.Poisson())
    base = ds.curve_launchers(kind, K_, B_, dt, dyc)
    inner = ds.pois_launchers(nl.Poisson(), base[0], base[1], base[2], dyc, dw)
    want = list(_fit_by_hand(ds, grp, inner, dxc, M, True, o, scaled=False))
    # chi2 of a Poisson fit: the deviance over dof = unmasked rows of the GROUP - n
    fh = want[1].cpu().numpy()
    q = []
    for p in range(GC.NGROUP):
        s = 0.0
        for v in fh[p]:
            s = s + v * v
        q.append(s / float(int((w[p * G:(p + 1) * G] != 0).sum()) - n))
    want[4] = _dev(ds, np.array(q))
    _check_composition(got, want, nprob, m, N_, n)
    inner[2].close()
    with pytest.raises(ValueError):
        ds.curve_fit_batch(kind, dt, dyc, dxc, ncomp=K_, baseline=B_, group=grp, stat=nl.Poisson(), loss=nl.Loss("huber", 0.1))


def test_group_with_pmap_raises_and_a_group_of_another_model(ds):
    kind, K_, B_, m, G, shared = GC.CASES[0]
    t, y, xt, x0 = GC.problems(kind, K_, B_, m, G, shared, ngroup=1)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    grp = nl.Group(7, shared=shared, nsets=G)
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    with pytest.raises(ValueError, match="pmap"):
        ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, group=grp, pmap=nl.ParamMap(7, fixed=(6,)))
    with pytest.raises(ValueError, match="pmap"):
        ds.expr_fit_batch(e, dt, dy, dx0, group=grp, pmap=nl.ParamMap(7, fixed=(6,)))
    with pytest.raises(ValueError, match="4 parameters"):
        ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, group=nl.Group(4, nsets=G))
    with pytest.raises(ValueError, match="multiple"):
        ds.expr_fit_batch(e, dt, dy, dx0, group=nl.Group(7, shared=shared, nsets=2))


def test_no_group_is_the_old_entry_point(ds):
    """group=None calls exactly what is called without it: the same results as the same call without the keyword."""
    kind, K_, B_, m = "lorentz", 2, 0, 64
    t, y, xt, x0 = CC.curve_problems(kind, K_, B_, m, nprob=8)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=CC.MAX_EVALS)
    a, b = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, opts=o), ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, opts=o, group=None)
    assert all(_eq(u, v) for u, v in zip(a[:6], b[:6])) and a[6:] == b[6:]
    # and a group of one data set with nothing shared gives the plain fit's results
    c = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, opts=o, group=nl.Group(7, nsets=1))
    assert all(_eq(u, v) for u, v in zip(a[:6], c[:6])) and a[6:] == c[6:]


# ------------------------------------------------------------------------------------------------ 6. alone and in a batch
def test_alone_and_inside_a_batch_of_300(ds):
    """300 groups reach the sub-batches (concurrent calls of the wrapping launchers on different streams)."""
    kind, K_, B_, m, G, shared = "lorentz", 2, 0, 64, 3, (1, 4)
    ngroup = 300
    t, y, xt, x0 = GC.problems(kind, K_, B_, m, G, shared, ngroup=ngroup, seed=77)
    grp = nl.Group(7, shared=shared, nsets=G)
    n = grp.nouter
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=GC.MAX_EVALS)
    big = None
    for analytic in (True, False):
        for form in (None, "row"):
            with _env(NLH_GROUP_FORM=form):
                big = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, analytic=analytic, opts=o, group=grp)
                for p in (0, 137, ngroup - 1):
                    d = slice(p * G, (p + 1) * G)
                    one = ds.curve_fit_batch(kind, dt[d].contiguous(), dy[d].contiguous(), dx0[d].contiguous(), ncomp=K_, baseline=B_,
                                             analytic=analytic, opts=o, group=grp)
                    for k in (0, 1, 2):
                        assert _eq(one[k], big[k][d]), (analytic, form, p, k)
                    for k in (3, 4, 5):
                        assert _eq(one[k], big[k][p:p + 1]), (analytic, form, p, k)
                    assert one[6][0] == big[6][p] and one[7][0] == big[7][p]
    # the host-array twin of the last (forward differences), and the formula's
    nprob = ngroup * G
    ib, st = (_lib.IterationBehavior * ngroup)(), (C.c_int32 * ngroup)()
    e = nl.Expr(FORMULA, ("t",), PARAMS)
    for which in ("curve", "expr"):
        xh, fh = x0.copy(), np.zeros((nprob, m))
        sh, ch, qh, rh = np.zeros((nprob, 7)), np.zeros((ngroup, n, n)), np.zeros(ngroup), np.zeros(ngroup, dtype=np.int32)
        tail = (t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, 0, None, None, grp.ptr, 0, None, 0, 0, 0.0, xh.ctypes.data_as(dp),
                fh.ctypes.data_as(dp), sh.ctypes.data_as(dp), ch.ctypes.data_as(dp), qh.ctypes.data_as(dp), rh.ctypes.data_as(_lib.c_int32_p), ib, st)
        if which == "curve":
            rc = ds.lib.nlh_curve_fit_batch_group_h(ds.h.ptr, C.byref(o), R.LORENTZ, K_, B_, nprob, m, *tail)
        else:
            rc = ds.lib.nlh_expr_fit_batch_group_h(ds.h.ptr, C.byref(o), e.ptr, nprob, m, *tail)
        assert rc == 0                                                  # (the formula's residual bits are the curve model's)
        for g, w_ in zip((xh, fh, sh, ch, qh), big[:5]):
            assert np.array_equal(_bits(g), _bits(w_.cpu().numpy())), which
        assert np.array_equal(rh, big[5].cpu().numpy()) and [ib[p].as_dict() for p in range(ngroup)] == big[6] and list(st) == big[7]


# ------------------------------------------------------------------------------------------------ 7. degrees of freedom
def test_degrees_of_freedom_are_the_groups(ds):
    """dof = count(w != 0) over the group's G m rows - n.  A group with every row of ONE data set at weight 0 has rows enough
    overall and is solved (the local columns of that data set are zero: the rank says so); a group with count <= n gets the
    status and NaNs, it alone, and keeps its x (its shared parameters made equal)."""
    kind, K_, B_, m, G, shared = "lorentz", 1, 1, 40, 3, (2,)
    N_, ngroup = 5, 5
    T = GR.tables(N_, shared, G)
    n, M, nprob = GR.nouter(T), G * m, ngroup * G                       # n = 13
    grp = _group(T)
    t, y, xt, x0 = GC.problems(kind, K_, B_, m, G, shared, ngroup=ngroup, seed=5)
    rng = np.random.default_rng(8)
    w = np.ones((nprob, m))
    w[0 * G + 1, 30:] = 0.0                                             # group 0: ragged padding
    w[1 * G + 1, :] = 0.0                                               # group 1: data set 1 absent altogether
    y[1 * G + 1, :] = 1e3                                               #          (what lies under the padding does not matter)
    w[3 * G:4 * G, :] = 0.0                                             # group 3: n rows in all, dof 0
    w[3 * G, :7], w[3 * G + 1, :3], w[3 * G + 2, :3] = 1.0, 1.0, 1.0
    dt, dy, dw, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, w), _dev(ds, x0)
    o = ds.options(max_evals=CC.MAX_EVALS)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K_, baseline=B_, weights=dw, opts=o, group=grp)
    assert st[3] == NL_INVALID_INPUT_ERROR and NL_INVALID_INPUT_ERROR not in [st[p] for p in (0, 1, 2, 4)]
    xh, fh, sh, ch, qh, rh = (v.cpu().numpy() for v in (x, fvec, sigma, cov, chi2, rank))
    assert np.isnan(sh[3 * G:4 * G]).all() and np.isnan(ch[3]).all() and np.isnan(qh[3]) and rh[3] == -1 and ibs[3]["fcn_count"] == 0
    assert np.array_equal(_bits(xh[3 * G:4 * G]), _bits(GR.expand(T, GR.gather(T, x0[3 * G:4 * G])[0])))
    good = [0, 1, 2, 4]
    gi = torch.tensor([p * G + g for p in good for g in range(G)], device=ds.device)
    hand = _fit_by_hand(ds, grp, ds.curve_launchers(kind, K_, B_, dt[gi].contiguous(), dy[gi].contiguous(), dw[gi].contiguous()),
                        dx0[gi].contiguous(), M, True, o)
    hx, hf, hc, hr = hand[0].cpu().numpy(), hand[1].cpu().numpy(), hand[3].cpu().numpy(), hand[5].cpu().numpy()
    for k, p in enumerate(good):
        d, dk = slice(p * G, (p + 1) * G), slice(k * G, (k + 1) * G)
        assert st[p] == hand[7][k] and ibs[p] == hand[6][k]
        assert np.array_equal(_bits(xh[d]), _bits(hx[dk])) and np.array_equal(_bits(fh[d].ravel()), _bits(hf[k]))
        if st[p] != 0:
            continue
        dof = int((w[d] != 0).sum()) - n
        s = 0.0
        for v in fh[d].ravel():
            s = s + v * v
        assert _bits(qh[p]) == _bits(s / float(dof)), p
        wc = hc[k] * (float(M - n) / float(dof))
        assert np.array_equal(_bits(ch[p]), _bits(wc)), p
        assert np.array_equal(_bits(sh[d]), _bits(GR.expand(T, np.sqrt(np.diag(wc))))), p
        assert rh[p] == hr[k]
    # every one of them solves -- the oracle returns 0 on group 1's stacked problem too --, and the absent data set's four
    # local columns are zero: the rank falls short by exactly them
    assert {st[p] for p in good} == {0} and rh[0] == rh[2] == rh[4] == n
    assert rh[1] == hr[1] == n - (N_ - len(shared))


# ------------------------------------------------------------------------------------------------ 8. the model object
@pytest.mark.parametrize("analytic", [0, 1])
def test_model_object(ds, analytic):
    """nlh_group_model_create over a curve model, through _eval, _lm_solve, _cls_solve, _lm_covariance = the launcher forms."""
    kind, K_, B_, m, G, shared = GC.CASES[1]
    N_ = R.nparams(R.LORENTZ, K_, B_)
    ngroup = 4
    nprob = ngroup * G
    t, y, xt, x0 = GC.problems(kind, K_, B_, m, G, shared, ngroup=ngroup)
    T = GR.tables(N_, shared, G)
    n, M = GR.nouter(T), G * m
    grp = _group(T)
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.curve_launchers(kind, K_, B_, dt, dy)
    wf, wj, wctx = ds.group_launchers(grp, fcn, jac, ctx)
    j = wj if analytic else None
    o = ds.options(max_evals=GC.MAX_EVALS)
    inner, md = C.c_void_p(), C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.LORENTZ, K_, B_, nprob, m, t.ctypes.data_as(dp), 0, y.ctypes.data_as(dp), None, analytic,
                                         C.byref(inner)) == 0
    assert ds.lib.nlh_group_model_create(ds.h.ptr, inner, grp.ptr, C.byref(md)) == 0
    try:
        sp, sm, sn = C.c_int32(), C.c_int32(), C.c_int32()
        ds.lib.nlh_dq_model_shape(md, C.byref(sp), C.byref(sm), C.byref(sn))
        assert (sp.value, sm.value, sn.value) == (ngroup, M, n)
        xs = GR.gather(T, x0)
        f0 = np.zeros((ngroup, M))
        assert ds.lib.nlh_dq_model_eval(ds.h.ptr, md, xs.ctypes.data_as(dp), f0.ctypes.data_as(dp)) == 0
        assert np.array_equal(_bits(f0), _bits(_launch(ds, wf, wctx, list(range(ngroup)), xs, M)))
        P = GR.expand(T, xs)
        for p in range(nprob):
            assert np.array_equal(_bits(f0.reshape(nprob, m)[p]), _bits(R.residual(R.LORENTZ, K_, B_, P[p], t[p], y[p])))
        ib, st = (_lib.IterationBehavior * ngroup)(), (C.c_int32 * ngroup)()
        xh, fh = xs.copy(), np.zeros((ngroup, M))
        assert ds.lib.nlh_dq_model_lm_solve(ds.h.ptr, C.byref(o), md, xh.ctypes.data_as(dp), fh.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, xs)
        fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, M, x, jac=j, opts=o)
        assert np.array_equal(_bits(xh), _bits(x.cpu().numpy())) and np.array_equal(_bits(fh), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(ngroup)] == ibs and list(st) == status and set(status) == {0}
        ch, sh, rh, qh = np.zeros((ngroup, n, n)), np.zeros((ngroup, n)), np.zeros(ngroup, dtype=np.int32), np.zeros(ngroup)
        assert ds.lib.nlh_dq_model_lm_covariance(ds.h.ptr, md, xh.ctypes.data_as(dp), 1, 0.0, ch.ctypes.data_as(dp), sh.ctypes.data_as(dp),
                                                 rh.ctypes.data_as(_lib.c_int32_p), qh.ctypes.data_as(dp)) == 0
        cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, M, x, jac=j)
        assert np.array_equal(_bits(ch), _bits(cov.cpu().numpy())) and np.array_equal(_bits(sh), _bits(sigma.cpu().numpy()))
        assert np.array_equal(rh, rank.cpu().numpy()) and np.array_equal(_bits(qh), _bits(chi2.cpu().numpy()))
        lo, hi = _outer_bounds(T, xt.min(0) - 0.5, xt.max(0) + 0.5)
        xc, fc = xs.copy(), np.zeros((ngroup, M))
        assert ds.lib.nlh_dq_model_cls_solve(ds.h.ptr, C.byref(o), md, 1.0, 1.0, lo.ctypes.data_as(dp), hi.ctypes.data_as(dp),
                                             xc.ctypes.data_as(dp), fc.ctypes.data_as(dp), ib, st) == 0
        x = _dev(ds, xs)
        fvec, ibs, status = ds.cls_solve_batch_device(wf, wctx, M, x, jac=j, opts=o, lower=lo, upper=hi)
        assert np.array_equal(_bits(xc), _bits(x.cpu().numpy())) and np.array_equal(_bits(fc), _bits(fvec.cpu().numpy()))
        assert [ib[p].as_dict() for p in range(ngroup)] == ibs and list(st) == status
    finally:
        ds.lib.nlh_dq_model_destroy(md)
        ds.lib.nlh_dq_model_destroy(inner)
        wctx.close()


# ------------------------------------------------------------------------------------------------ 9. error returns
def test_error_returns(ds):
    """In the documented order; nothing is written where a call is refused."""
    kind, K_, B_, m, G = "lorentz", 2, 0, 6, 2                          # N = 7; shared (1, 4): n = 2 + 2 * 5 = 12 = M
    nprob = 2 * G
    t, y, xt, x0 = CC.curve_problems(kind, K_, B_, m, nprob=nprob)
    dt, dy, dx = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options()
    g12 = nl.Group(7, shared=(1, 4), nsets=G)                           # n = 12 = M
    g10 = nl.Group(7, shared=(1, 2, 4, 5), nsets=G)                     # n = 4 + 2 * 3 = 10 < M
    g14 = nl.Group(7, nsets=G)                                          # n = 14 > M
    g4 = nl.Group(4, nsets=G)
    g3 = nl.Group(7, shared=(1, 4), nsets=3)
    f = torch.full((nprob, m), 7.0, dtype=torch.float64, device=ds.device)
    s = torch.full((nprob, 7), 7.0, dtype=torch.float64, device=ds.device)

    def fit(kd, KK, mm, grp, sigma=None, x=dx, h=ds.h.ptr, loss=0, stat=0, floor=0.0, scale=None):
        return ds.lib.nlh_curve_fit_batch_group(h, C.byref(o), kd, KK, B_, nprob, mm, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                                grp.ptr if grp is not None else None, loss, scale, 0, stat, floor,
                                                x.data_ptr() if x is not None else None, f.data_ptr(), sigma, None, None, None, None, None)
    assert fit(1, K_, m, g10, h=None) == -3                             # NLH_ERR_BAD_HANDLE first
    assert fit(7, K_, m, g10) == NL_INVALID_INPUT_ERROR and fit(1, 0, m, g10) == NL_INVALID_INPUT_ERROR
    assert fit(1, K_, m, None) == NL_INVALID_INPUT_ERROR                # no group
    assert fit(1, K_, m, g4) == NL_INVALID_INPUT_ERROR                  # a group of another model
    assert fit(1, K_, m, g3) == NL_INVALID_INPUT_ERROR                  # nprob is no multiple of G
    assert fit(1, K_, m, g14) == NL_UNDERDEFINED_PROBLEM_ERROR          # G m < n
    assert fit(1, K_, m, g14, loss=9) == NL_UNDERDEFINED_PROBLEM_ERROR  # ... before the loss is looked at
    assert fit(1, K_, m, g10, loss=9) == NL_INVALID_INPUT_ERROR         # a loss outside 0 .. 3
    assert fit(1, K_, m, g10, stat=2) == NL_INVALID_INPUT_ERROR         # a stat outside 0 .. 1
    assert fit(1, K_, m, g10, x=None) == NL_INVALID_INPUT_ERROR         # a NULL array
    assert fit(1, K_, m, g10, loss=1) == NL_INVALID_INPUT_ERROR         # a loss without scales
    assert fit(1, K_, m, g12, s.data_ptr()) == NL_INVALID_INPUT_ERROR   # errors asked for with G m <= n
    assert fit(1, K_, m, g10, stat=1, floor=0.0) == NL_INVALID_INPUT_ERROR   # a bad mu_floor
    torch.cuda.synchronize()
    assert (f == 7.0).all() and (s == 7.0).all() and torch.equal(dx, _dev(ds, x0))
    assert fit(1, K_, m, g12) == 0                                      # N = 7 > m = 6, but G m = 12 >= n = 12: the group's counts matter
    assert fit(1, K_, m, g10, s.data_ptr()) == 0
    e = nl.Expr(FORMULA, ("t",), PARAMS)

    def efit(grp):
        return ds.lib.nlh_expr_fit_batch_group(ds.h.ptr, C.byref(o), e.ptr, nprob, m, dt.data_ptr(), 0, dy.data_ptr(), None, 1, None, None,
                                               grp.ptr if grp is not None else None, 0, None, 0, 0, 0.0, dx.data_ptr(), f.data_ptr(), None, None,
                                               None, None, None, None)
    assert efit(None) == efit(g4) == efit(g3) == NL_INVALID_INPUT_ERROR and efit(g14) == NL_UNDERDEFINED_PROBLEM_ERROR
    # the wrapping context and its launchers
    fcn, jac, ctx = ds.curve_launchers(kind, K_, B_, dt, dy)
    out = C.c_void_p(7)
    none = C.cast(None, _lib.DEVFCN)
    assert ds.lib.nlh_group_wrap(ds.h.ptr, None, fcn, jac, ds._ctxp(ctx), C.byref(out)) == NL_INVALID_INPUT_ERROR and not out.value
    assert ds.lib.nlh_group_wrap(ds.h.ptr, g10.ptr, none, jac, ds._ctxp(ctx), C.byref(out)) == NL_UNDEFINED_FUNCTION_ERROR
    assert ds.lib.nlh_group_wrap(ds.h.ptr, g10.ptr, fcn, jac, ds._ctxp(ctx), None) == NL_INVALID_INPUT_ERROR
    wf, wj, wctx = ds.group_launchers(g10, fcn, None, ctx)
    assert wj is None
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    X = ds.group_gather(g10, dx)
    J = torch.full((2, 10, G * m + 2), 7.0, dtype=torch.float64, device=ds.device)
    args = lambda n_, M_: (wctx.ptr, stream, 2, None, n_, C.c_void_p(X.data_ptr()), M_, C.c_void_p(J.data_ptr()))
    assert ds.lib.nlh_group_device_fcn(*args(7, G * m)) == NL_INVALID_INPUT_ERROR       # n != S + G L
    assert ds.lib.nlh_group_device_fcn(*args(10, G * m + 1)) == NL_INVALID_INPUT_ERROR  # M is no multiple of G
    assert ds.lib.nlh_group_device_fcn(*args(10, 0)) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_group_device_jac(*args(10, G * m)) == NL_UNDEFINED_FUNCTION_ERROR  # no inner Jacobian launcher
    assert ds.lib.nlh_group_device_fcn(*args(10, G * m + 2)) == NL_INVALID_INPUT_ERROR  # the inner launcher's refusal (m != ctx.m) comes back
    torch.cuda.synchronize()
    assert (J == 7.0).all()
    wctx.close()
    # the batch steps
    assert ds.lib.nlh_group_gather_batch(ds.h.ptr, None, 2, dx.data_ptr(), X.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_group_gather_batch(ds.h.ptr, g10.ptr, 2, None, X.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_group_expand_batch(ds.h.ptr, g10.ptr, 2, X.data_ptr(), None) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_group_sigma_batch(ds.h.ptr, g10.ptr, 2, None, None, s.data_ptr()) == NL_INVALID_INPUT_ERROR
    assert ds.lib.nlh_group_gather_batch(ds.h.ptr, g10.ptr, 0, None, None) == 0
    # the model object
    md, inner = C.c_void_p(7), C.c_void_p()
    A, b = np.ones((2, 2, 2)), np.ones((2, 2))
    assert ds.lib.nlh_dq_model_create(ds.h.ptr, 2, 2, 2, A.ctypes.data_as(dp), b.ctypes.data_as(dp), 0.5, C.byref(inner)) == 0
    g2 = nl.Group(2, nsets=2)
    assert ds.lib.nlh_group_model_create(ds.h.ptr, inner, g2.ptr, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    ds.lib.nlh_dq_model_destroy(inner)                                  # (a dense-quadratic model has no launchers to wrap)
    inner = C.c_void_p()
    assert ds.lib.nlh_curve_model_create(ds.h.ptr, 1, K_, B_, nprob, 7, np.ones((nprob, 7)).ctypes.data_as(dp), 0,
                                         np.ones((nprob, 7)).ctypes.data_as(dp), None, 1, C.byref(inner)) == 0
    assert ds.lib.nlh_group_model_create(ds.h.ptr, inner, g4.ptr, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    assert ds.lib.nlh_group_model_create(ds.h.ptr, inner, g3.ptr, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value   # 4 is no multiple of 3
    assert ds.lib.nlh_group_model_create(ds.h.ptr, inner, None, C.byref(md)) == NL_INVALID_INPUT_ERROR and not md.value
    assert ds.lib.nlh_group_model_create(ds.h.ptr, inner, g10.ptr, C.byref(md)) == 0 and md.value
    ds.lib.nlh_dq_model_destroy(md)
    ds.lib.nlh_dq_model_destroy(inner)
