"""GPU tests of the formulas' special functions (include/nonlin_hip.h: NLH_EXPR_ERF .. NLH_EXPR_VOIGT, nlh_faddeeva_batch):
the Faddeeva kernel and the interpreter on voigt formulas bit for bit against the numpy restatement
(tests/specfun_restatement.py) in both workgroup forms, at their size edges and for every chunk of Jacobian columns; the
device library's erf, erfc, erfcx in ulp against the 40-digit fixture, which the running bound's table rests on, and
formulas that use them within that bound; solves bit for bit against the CPU oracle over the restatement, alone, through a
parameter map, a projection and a robust loss; the one-call fit as the composition it stands for; recovery of noisy peaks."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import loss_restatement as LR
import pmap_restatement as PR
import sep_cases as SEPC
import specfun_cases as SC
import specfun_restatement as S
import nonlin_amd as nl

BOUND = SC.BOUND
pytestmark = pytest.mark.gpu

KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
# (NLH_EXPR_FORM, NLH_EXPR_CHUNK): what m and the depth select; each form forced (one that cannot hold m falls back); one
# Jacobian column per pass
VARIANTS = [(None, None), ("row", None), ("flat", None), (None, "1")]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


def _record(line):
    """Print a measured figure; append it to the file NLH_SPECFUN_FILE names, when it names one (profiles/specfun_accuracy.txt)."""
    print(line)
    path = os.environ.get("NLH_SPECFUN_FILE")
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


def _points(x0, plist, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(x0[plist] * (1.0 + 0.01 * rng.uniform(-1, 1, (len(plist), x0.shape[1]))))


# ------------------------------------------------------------------------------------------------ 1. the Faddeeva kernel
@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_faddeeva_batch(ds, count):
    """A thread per element: one element, a partial block, a full one, a second block of one -- the restatement's bits, the
    host entry's, and within the CPU bound of the fixture's 40-digit values."""
    F = SC.fixture()
    off = 400 - count // 2                                              # (a window over the fixture's mixed region and its tails)
    re, im = F["w_re"][off:off + count], F["w_im"][off:off + count]
    z = torch.complex(_dev(ds, re), _dev(ds, im))
    got = ds.wofz_batch(z).cpu().numpy()
    wr, wi = S.faddeeva_w(re, im)
    assert np.array_equal(_bits(got.real), _bits(wr)) and np.array_equal(_bits(got.imag), _bits(wi))
    host = nl.wofz(re + 1j * im)
    assert np.array_equal(_bits(got.real), _bits(host.real)) and np.array_equal(_bits(got.imag), _bits(host.imag))
    ref = F["w_wr"][off:off + count] + 1j * F["w_wi"][off:off + count]
    assert (np.abs(got - ref) <= BOUND["w"] * np.abs(ref)).all()
    # the array past the count is not written
    wr_t = torch.full((count + 3,), 7.0, dtype=torch.float64, device=ds.device)
    wi_t = torch.full((count + 3,), 7.0, dtype=torch.float64, device=ds.device)
    dre, dim = _dev(ds, re), _dev(ds, im)
    assert ds.lib.nlh_faddeeva_batch(ds.h.ptr, count, dre.data_ptr(), dim.data_ptr(), wr_t.data_ptr(), wi_t.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((wr_t[count:] == 7.0).all()) and bool((wi_t[count:] == 7.0).all()) and np.array_equal(_bits(wr_t[:count].cpu().numpy()), _bits(wr))
    assert ds.lib.nlh_faddeeva_batch(ds.h.ptr, 0, None, None, None, None) == 0
    assert ds.lib.nlh_faddeeva_batch(ds.h.ptr, -1, dre.data_ptr(), dim.data_ptr(), wr_t.data_ptr(), wi_t.data_ptr()) == 201
    assert ds.lib.nlh_faddeeva_batch(ds.h.ptr, 1, None, dim.data_ptr(), wr_t.data_ptr(), wi_t.data_ptr()) == 201


# ------------------------------------------------------------------------------------------------ 2. the interpreter on voigt
@pytest.mark.parametrize("m", [5, 128, 129, 257])
@pytest.mark.parametrize("weighted,shared", [(False, False), (True, False), (False, True), (True, True)])
def test_doublet_kernels_bitwise(ds, weighted, shared, m):
    """Nine parameters: the first chunk holds 8 columns at most, so the Jacobian takes two passes (one per column with
    NLH_EXPR_CHUNK = 1).  m = 5 and 128: the flat form -- 51 and 2 points per workgroup, the 60-point list ending in a
    partial workgroup for m = 5; m = 129 and 257: the row form, one partial block, and a second block of one row."""
    nprob = 7
    e = SC.compile_formula("doublet")
    prog, t, y, xt, x0 = SC.problems("doublet", m, nprob=nprob, seed=11 + m, prog=e.program())
    n = x0.shape[1]
    assert n == 9
    if shared:
        t = np.ascontiguousarray(np.broadcast_to(t[:, :1], t.shape))
    rng = np.random.default_rng(m)
    w = None
    if weighted:
        w = rng.uniform(0.5, 2.0, (nprob, m))
        w[rng.uniform(size=(nprob, m)) < 0.1] = 0.0
        w[:, 0] = 0.0
    dt, dy, dw = _dev(ds, t[:, 0] if shared else t), _dev(ds, y), (_dev(ds, w) if weighted else None)
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy, dw)
    for k, plist in enumerate([[nprob - 2], [2] * (n + 1), list(rng.integers(0, nprob, 57)) + [0, 0, nprob - 1]]):
        X = _points(x0, plist, k)
        wantF = [S.residual(prog, X[q], t[:, p], y[p], w[p] if weighted else None) for q, p in enumerate(plist)]
        wantJ = [S.jacobian(prog, X[q], t[:, p], w[p] if weighted else None).T for q, p in enumerate(plist)]
        for form, chunk in VARIANTS:
            with _variant(form, chunk):
                F = _launch(ds, fcn, ctx, plist, X, m)
                J = _launch(ds, jac, ctx, plist, X, m, jac=True)
            for q, p in enumerate(plist):
                assert np.array_equal(_bits(F[q]), _bits(wantF[q])), (form, chunk, k, q)
                assert np.array_equal(_bits(J[q]), _bits(wantJ[q])), (form, chunk, k, q)
                if weighted:                                           # a zero-weight row is exactly 0
                    assert (F[q][w[p] == 0.0] == 0.0).all() and (J[q][:, w[p] == 0.0] == 0.0).all()


@pytest.mark.parametrize("formula,params", SC.PATTERNS)
def test_presence_patterns_bitwise(ds, formula, params):
    m, nprob = 64, 3
    e = nl.Expr(formula, "t", params)
    prog = e.program()
    names = params.split(",")
    rng = np.random.default_rng(len(formula))
    t = np.sort(rng.uniform(0.0, 10.0, (1, nprob, m)), axis=-1)
    y = rng.uniform(0.0, 1.0, (nprob, m))
    x0 = np.array([[SC.PATTERN_X[k] for k in names]] * nprob) * (1.0 + 0.05 * rng.uniform(-1, 1, (nprob, len(names))))
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    plist = list(range(nprob))
    for form, chunk in VARIANTS:
        with _variant(form, chunk):
            F = _launch(ds, fcn, ctx, plist, x0, m)
            J = _launch(ds, jac, ctx, plist, x0, m, jac=True)
        for p in plist:
            assert np.array_equal(_bits(F[p]), _bits(S.residual(prog, x0[p], t[:, p], y[p]))), (formula, form, chunk)
            assert np.array_equal(_bits(J[p]), _bits(S.jacobian(prog, x0[p], t[:, p]).T)), (formula, form, chunk)


def test_negative_sigma_and_gamma_on_the_device(ds):
    m = 64
    e = nl.Expr("voigt(t-mu,s,g)", "t", "mu,s,g")
    t = np.linspace(0.0, 10.0, m)[None, None]
    y = np.zeros((1, m))
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    X = np.array([[4.7, 0.45, 0.35], [4.7, -0.45, 0.35], [4.7, 0.45, -0.35], [4.7, -0.45, -0.35]])
    F = _launch(ds, fcn, ctx, [0] * 4, X, m)
    J = _launch(ds, jac, ctx, [0] * 4, X, m, jac=True)
    for q in range(4):
        assert np.array_equal(_bits(F[q]), _bits(F[0]))
        assert np.array_equal(_bits(J[q]), _bits(J[0] * np.sign(X[q])[:, None]))
        assert np.array_equal(_bits(J[q]), _bits(S.jacobian(e.program(), X[q], t[:, 0]).T))


# ------------------------------------------------------------------------------------------------ 3. erf, erfc, erfcx
def test_erf_family_accuracy(ds):
    """The device library's erf, erfc, erfcx in ulp, through nlh_expr_eval_batch against the fixture (|a| <= 26, dense near 0).
    The restatement's table U_F is this maximum rounded up: it must cover what is measured here."""
    F = SC.fixture()
    a = F["erf_a"]
    zero = _dev(ds, np.zeros((1, 1)))
    measured = {}
    for f in ("erf", "erfc", "erfcx"):
        e = nl.Expr(f"{f}(t)+a", "t", "a")                               # a = 0: v + 0 is v
        got = ds.expr_eval(e, zero, _dev(ds, a)).cpu().numpy()[0]
        ref = F[f]
        ok = ref != 0.0                                                  # erf(0) = 0 exactly; every other value is a normal number
        assert (got[~ok] == 0.0).all() and (np.abs(ref[ok]) >= 2.3e-308).all()
        ulp = np.abs(got[ok] - ref[ok]) / np.spacing(np.abs(ref[ok]))
        measured[f] = float(ulp.max())
        _record(f"specfun device accuracy {f}: {measured[f]:.3f} ulp at a = {float(a[ok][np.argmax(ulp)])!r}, {int(ok.sum())} arguments, |a| <= 26 "
                f"(table {S.U_F[f]})")
    for f, worst in measured.items():
        assert math.ceil(worst) <= S.U_F[f], (f, worst, S.U_F[f])


@pytest.mark.parametrize("name", SC.WITH_FUNCTIONS)
def test_erf_family_formulas_within_running_bound(ds, name):
    """|device - numpy| <= the restatement's first-order running bound, residual and Jacobian, entry by entry."""
    nprob = 6
    e = SC.compile_formula(name)
    rf = rj = 0.0
    for m in (64, 200):
        prog, t, y, xt, x0 = SC.problems(name, m, nprob=nprob, prog=e.program())
        w = np.random.default_rng(2).uniform(0.5, 2.0, (nprob, m))
        w[:, 3] = 0.0
        dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
        for wd, wh in ((None, None), (dw, w)):
            fcn, jac, ctx = ds.expr_launchers(e, dt, dy, wd)
            plist = list(range(nprob)) + [1, 1]
            X = _points(x0, plist, 20)
            F = _launch(ds, fcn, ctx, plist, X, m)
            J = _launch(ds, jac, ctx, plist, X, m, jac=True)
            for q, p in enumerate(plist):
                wp = wh[p] if wh is not None else None
                want, bound = S.residual_bound(prog, X[q], t[:, p], y[p], wp)
                err = np.abs(F[q] - want)
                assert (err <= bound).all(), (name, m, q, float((err[bound > 0] / bound[bound > 0]).max()))
                rf = max(rf, float((err[bound > 0] / bound[bound > 0]).max()))
                wj, bj = S.jacobian_bound(prog, X[q], t[:, p], wp)
                ej = np.abs(J[q].T - wj)
                assert (ej <= bj).all(), (name, m, q, "jacobian", float((ej[bj > 0] / bj[bj > 0]).max()))
                rj = max(rj, float((ej[bj > 0] / bj[bj > 0]).max()))
    _record(f"specfun running-bound ratio {name}: residual {rf:.3f} jacobian {rj:.3f}")


# ------------------------------------------------------------------------------------------------ 4. solves, the oracle
def _box(xt):
    """A box that keeps sigma and gamma positive and binds for some problems."""
    lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
    for k in (2, 3, 6, 7):
        lower[k], upper[k] = 0.05, xt[:, k].mean() + 0.02
    return lower, upper


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
def test_doublet_solves_against_oracle(ds, oracle, analytic, bounded):
    """The device's solve is the CPU oracle's with the restatement as callback, bit for bit in x, fvec, counts and flags."""
    m, nprob = 129, 8
    e = SC.compile_formula("doublet")
    prog, t, y, xt, x0 = SC.problems("doublet", m, nprob=nprob, prog=e.program())
    n = x0.shape[1]
    opt = dict(max_evals=SC.MAX_EVALS)
    lower = upper = None
    if bounded:
        lower, upper = _box(xt)
        x0 = np.clip(x0, lower, upper)
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    x = _dev(ds, x0)
    if bounded:
        fvec, ibs, status = ds.cls_solve_batch_device(fcn, ctx, m, x, jac=jac if analytic else None, opts=ds.options(**opt), lower=lower, upper=upper)
    else:
        fvec, ibs, status = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=jac if analytic else None, opts=ds.options(**opt))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**opt)
    for p in range(nprob):
        tv = t[:, p]
        f = lambda xx, ff: ff.__setitem__(slice(None), S.residual(prog, xx, tv, y[p]))
        j = (lambda xx, JJ: JJ.__setitem__((slice(None), slice(None)), S.jacobian(prog, xx, tv))) if analytic else None
        if bounded:
            rc, xo, fo, ibo = oracle.cls_solve(f, m, n, x0[p], jac=j, opts=oo, lower=lower, upper=upper)
        else:
            rc, xo, fo, ibo = oracle.lm_solve(f, m, n, x0[p], jac=j, opts=oo)
        what = (analytic, bounded, p)
        assert status[p] == rc, (what, status[p], rc)
        assert _same(ibs[p], ibo), (what, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), what
    if not bounded:
        assert set(status) == {0}, sorted(set(status))


def _fit_by_hand(ds, e, dt, dy, x0, m, analytic, o, lower=None, upper=None):
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy, None)
    j = jac if analytic else None
    x = x0.clone()
    if lower is not None:
        fvec, ibs, st = ds.cls_solve_batch_device(fcn, ctx, m, x, jac=j, opts=o, lower=lower, upper=upper)
    else:
        fvec, ibs, st = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=j, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(fcn, ctx, m, x, jac=j, scaled=True)
    return x, fvec, sigma, cov, chi2, rank, ibs, st


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
def test_fit_batch_is_the_composition(ds, analytic, bounded):
    """expr_fit_batch = solve (or bounded solve), then covariance, by hand; a problem alone gives its bits in the batch."""
    m, nprob = 129, 8
    e = SC.compile_formula("doublet")
    prog, t, y, xt, x0 = SC.problems("doublet", m, nprob=nprob, prog=e.program())
    n = x0.shape[1]
    lower, upper = _box(xt) if bounded else (None, None)
    if bounded:
        x0 = np.clip(x0, lower, upper)
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=SC.MAX_EVALS)
    got = ds.expr_fit_batch(e, dt, dy, dx0, lower=lower, upper=upper, analytic=analytic, opts=o)
    want = _fit_by_hand(ds, e, dt, dy, dx0, m, analytic, o, lower, upper)
    assert _eq(got[0], want[0]) and _eq(got[1], want[1]) and got[6] == want[6] and got[7] == want[7]
    ok = torch.tensor([s == 0 for s in got[7]], device=ds.device)
    assert bounded or bool(ok.all())
    for g, w_ in zip(got[2:6], want[2:6]):
        assert _eq(g[ok], w_[ok])
    assert bool((got[5][ok] == n).all()) and bool((got[2][ok] > 0).all())
    for p in (0, nprob - 1):
        one = ds.expr_fit_batch(e, dt[:, p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dx0[p:p + 1].contiguous(), lower=lower, upper=upper,
                                analytic=analytic, opts=o)
        for g, w_ in zip(one[:6], got[:6]):
            assert _eq(g, w_[p:p + 1]), p
        assert one[6][0] == got[6][p] and one[7][0] == got[7][p]


# ------------------------------------------------------------------------------------------------ 5. composition
def _check(status, ibs, xg, fg, p, rc, xo, fo, ibo, what):
    assert status[p] == rc, (what, p, status[p], rc)
    assert _same(ibs[p], ibo), (what, p, ibs[p], ibo)
    assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, p, np.abs(xg[p] - xo).max())
    assert np.array_equal(_bits(fg[p]), _bits(fo)), (what, p)


@pytest.mark.parametrize("analytic", [False, True])
def test_doublet_through_a_map_against_oracle(ds, oracle, analytic):
    """ParamMap.for_expr ties s2 to s1 (the Gaussian width is the instrument's): the oracle on the reduced problem, the
    restated expand and contract around the restated formula as callbacks."""
    m, nprob = 128, 4
    e = SC.compile_formula("doublet")
    prog, t, y, xt, x0 = SC.problems("doublet", m, nprob=nprob, prog=e.program())
    pm = nl.ParamMap.for_expr(e, tied={"s2": ("s1", 1.0, 0.0)})
    T = PR.tables(9, [], {6: (2, 1.0, 0.0)})
    for g, w_ in zip(pm.tables(), T):
        assert np.array_equal(g, w_)
    n = len(T[4])
    full = np.ascontiguousarray(x0)
    dfull = _dev(ds, full)
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, dfull)
    x = ds.pmap_gather(pm, dfull)
    o = dict(max_evals=SC.MAX_EVALS)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options(**o))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**o)
    for p in range(nprob):
        tv = t[:, p]
        f = lambda xx, out: out.__setitem__(slice(None), S.residual(prog, PR.expand(T, xx, full[p]), tv, y[p]))
        j = (lambda xx, J: J.__setitem__((slice(None), slice(None)), PR.contract(T, S.jacobian(prog, PR.expand(T, xx, full[p]), tv)))) if analytic else None
        rc, xo, fo, ibo = oracle.lm_solve(f, m, n, PR.gather(T, full[p]), jac=j, opts=oo)
        _check(status, ibs, xg, fg, p, rc, xo, fo, ibo, ("map", analytic))
    assert set(status) == {0}
    wctx.close()


@pytest.mark.parametrize("analytic", [False, True])
def test_doublet_projected_against_oracle(ds, oracle, analytic):
    """Separable.for_expr(linear = a1, a2, c): the amplitudes and the baseline are projected out, six unknowns remain."""
    m, nprob = 128, 4
    e = SC.compile_formula("doublet")
    prog, t, y, xt, x0 = SC.problems("doublet", m, nprob=nprob, prog=e.program())
    sp = nl.Separable.for_expr(e, linear=("a1", "a2", "c"))
    lin, nonlin = [0, 4, 8], [1, 2, 3, 5, 6, 7]
    alpha0 = np.ascontiguousarray(x0[:, nonlin])
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    x = _dev(ds, alpha0)
    o = dict(max_evals=SC.MAX_EVALS)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options(**o))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**o)
    for p in range(nprob):
        tv = t[:, p]
        f, j = SEPC.oracle_callbacks(lambda P: S.residual(prog, P, tv, y[p]), lambda P: S.jacobian(prog, P, tv), 9, lin, analytic)
        rc, xo, fo, ibo = oracle.lm_solve(f, m, 6, alpha0[p], jac=j, opts=oo)
        _check(status, ibs, xg, fg, p, rc, xo, fo, ibo, ("sep", analytic))
    assert set(status) == {0}
    wctx.close()


@pytest.mark.parametrize("analytic", [False, True])
def test_single_voigt_with_huber_against_oracle(ds, oracle, analytic):
    """Loss("huber", c) around a single Voigt peak with outliers: the oracle over the restated transform of the restated formula."""
    m, nprob = 128, 4
    e = SC.compile_formula("voigt1")
    prog, t, y, xt, x0 = SC.problems("voigt1", m, nprob=nprob, prog=e.program())
    y = y.copy()
    y[:, 17::31] += 0.4                                                 # four outliers per data set, far beyond the scale
    c = 0.02 * (1.0 + 0.5 * np.arange(nprob) / nprob)
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.loss_launchers(nl.Loss("huber", c), fcn, jac, ctx)
    x = _dev(ds, x0)
    o = dict(max_evals=SC.MAX_EVALS)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options(**o))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**o)
    k = LR.KINDS["huber"]
    for p in range(nprob):
        tv = t[:, p]
        f = lambda xx, out: out.__setitem__(slice(None), LR.residual(k, c[p], S.residual(prog, xx, tv, y[p])))
        j = (lambda xx, J: J.__setitem__((slice(None), slice(None)), LR.jacobian(k, c[p], S.residual(prog, xx, tv, y[p]), S.jacobian(prog, xx, tv)))) \
            if analytic else None
        rc, xo, fo, ibo = oracle.lm_solve(f, m, 5, x0[p], jac=j, opts=oo)
        _check(status, ibs, xg, fg, p, rc, xo, fo, ibo, ("huber", analytic))
    wctx.close()


# ------------------------------------------------------------------------------------------------ 6. recovery
def test_recovery(ds):
    """64 noisy single Voigt peaks, sigma and gamma of comparable size: every parameter within 3 reported standard errors of its
    generating value in at least 60 problems (tests/test_specfun_cpu.py holds the seed to that on the CPU oracle)."""
    m, nprob = SC.RECOVERY_M, SC.RECOVERY_NPROB
    e = SC.compile_formula("voigt1")
    prog, t, y, xt, x0 = SC.problems("voigt1", m, nprob=nprob, seed=SC.RECOVERY_SEED, gaussian=SC.RECOVERY_NOISE, prog=e.program())
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.expr_fit_batch(e, _dev(ds, t), _dev(ds, y), _dev(ds, x0), opts=ds.options(max_evals=SC.MAX_EVALS))
    assert set(st) == {0} and bool((rank == 5).all())
    good = int((np.abs(x.cpu().numpy() - xt) <= 3.0 * sigma.cpu().numpy()).all(axis=1).sum())
    print(f"voigt recovery: {good} of {nprob} within 3 standard errors")
    assert good >= 60
