"""GPU tests of the formulas' j0, j1, i0e, i1e, lgamma, expm1 and log1p (include/nonlin_hip.h: NLH_EXPR_J0 ..
NLH_EXPR_LOG1P): the interpreter's newer instantiation on a ten-parameter i0e / i1e formula bit for bit against the numpy
restatement (tests/specfun2_restatement.py) and on a twelve-parameter formula of every library function within the running
bound, in both workgroup forms, at their size edges and for every chunk of Jacobian columns; a definition that holds a new
function against the substituted formula by bits; the older instantiation still chosen for a formula without one; the edge
rows of the header's table; the seven functions in ulp against the 40-digit fixture, which the running bound's table rests
on; fits against the CPU oracle over the restatement, alone, projected, as a Poisson likelihood; the band."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import band_restatement as BR
import defs_restatement as D
import pois_restatement as PR
import sep_cases as SEPC
import specfun2_cases as SC
import specfun2_restatement as S2
import nonlin_amd as nl

pytestmark = pytest.mark.gpu

KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
# (NLH_EXPR_FORM, NLH_EXPR_CHUNK): what m and the depth select; each form forced (one that cannot hold m falls back); one
# Jacobian column per pass
VARIANTS = [(None, None), ("row", None), ("flat", None), (None, "1")]
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -52


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_bits(got, want):
    """Bit equality, a NaN matching any NaN (the payload and sign of a NaN are not part of the table)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def _same(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _record(line):
    """Print a measured figure; append it to the file NLH_SPECFUN2_FILE names, when it names one (profiles/specfun2_accuracy.txt)."""
    print(line)
    path = os.environ.get("NLH_SPECFUN2_FILE")
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


def _ratio(err, bound):
    """The largest |device - numpy| / bound over the entries whose bound is not 0 (those are compared by <=, that is exactly)."""
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. the kernels at their edges
@pytest.mark.parametrize("m", [5, 128, 129, 257])
@pytest.mark.parametrize("weighted,shared", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", ["bessel10", "mixed"])
def test_kernels_at_the_size_edges(ds, name, weighted, shared, m):
    """Ten and twelve parameters: the first chunk holds 8 columns at most, so the Jacobian takes two passes (one per column
    with NLH_EXPR_CHUNK = 1).  m = 5 and 128: the flat form -- 51 and 2 points per workgroup, the 60-point list ending in a
    partial workgroup for m = 5; m = 129 and 257: the row form, one partial block, and a second block of one row.  bessel10
    (i0e and i1e only, arguments of both signs and on both sides of 8): the restatement's bits.  mixed (every library
    function): within the running bound, entry by entry."""
    nprob = 7
    e = SC.compile_formula(name)
    prog, t, y, xt, x0 = SC.problems(name, m, nprob=nprob, seed=11 + m, prog=e.program())
    n = x0.shape[1]
    assert n > 8
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
    exact = name in SC.EXACT
    for k, plist in enumerate([[nprob - 2], list(rng.integers(0, nprob, 57)) + [0, 0, nprob - 1]]):
        X = _points(x0, plist, k)
        wp = [w[p] if weighted else None for p in plist]
        if exact:
            wantF = [(S2.residual(prog, X[q], t[:, p], y[p], wp[q]), None) for q, p in enumerate(plist)]
            wantJ = [(S2.jacobian(prog, X[q], t[:, p], wp[q]), None) for q, p in enumerate(plist)]
        else:
            wantF = [S2.residual_bound(prog, X[q], t[:, p], y[p], wp[q]) for q, p in enumerate(plist)]
            wantJ = [S2.jacobian_bound(prog, X[q], t[:, p], wp[q]) for q, p in enumerate(plist)]
        first = None
        for form, chunk in VARIANTS:
            with _variant(form, chunk):
                F = _launch(ds, fcn, ctx, plist, X, m)
                J = _launch(ds, jac, ctx, plist, X, m, jac=True)
            if first is None:
                first = (F, J)
            assert np.array_equal(_bits(F), _bits(first[0])) and np.array_equal(_bits(J), _bits(first[1])), (form, chunk)   # the bits do not depend on the form
            for q, p in enumerate(plist):
                if exact:
                    assert np.array_equal(_bits(F[q]), _bits(wantF[q][0])), (form, chunk, k, q)
                    assert np.array_equal(_bits(J[q]), _bits(wantJ[q][0].T)), (form, chunk, k, q)
                else:
                    err, ej = np.abs(F[q] - wantF[q][0]), np.abs(J[q].T - wantJ[q][0])
                    assert (err <= wantF[q][1]).all(), (form, chunk, k, q, _ratio(err, wantF[q][1]))
                    assert (ej <= wantJ[q][1]).all(), (form, chunk, k, q, "jacobian", _ratio(ej, wantJ[q][1]))
                if weighted:                                           # a zero-weight row is exactly 0
                    assert (F[q][w[p] == 0.0] == 0.0).all() and (J[q][:, w[p] == 0.0] == 0.0).all()
    if exact and m >= 128 and not weighted:                            # both ranges and both signs are reached within a data set
        a = x0[0, 1] * (t[0, 0] - x0[0, 2])
        assert (a < -8.0).any() and (a > 8.0).any() and ((a > -8.0) & (a < 0.0)).any() and ((a > 0.0) & (a < 8.0)).any()


@pytest.mark.parametrize("name", ["airy", "vonmises", "gammapdf", "planck"])
def test_model_formulas_within_running_bound(ds, name):
    """The four models of the README: |device - numpy| <= the restatement's first-order running bound, residual and
    Jacobian, entry by entry."""
    nprob = 6
    e = SC.compile_formula(name)
    rf = rj = 0.0
    for m in (64, 200):
        prog, t, y, xt, x0 = SC.problems(name, m, nprob=nprob, prog=e.program())
        fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
        plist = list(range(nprob)) + [1, 1]
        X = _points(x0, plist, 20)
        F = _launch(ds, fcn, ctx, plist, X, m)
        J = _launch(ds, jac, ctx, plist, X, m, jac=True)
        assert np.isfinite(F).all() and np.isfinite(J).all()
        for q, p in enumerate(plist):
            want, bound = S2.residual_bound(prog, X[q], t[:, p], y[p])
            err = np.abs(F[q] - want)
            assert (err <= bound).all(), (name, m, q, _ratio(err, bound))
            wj, bj = S2.jacobian_bound(prog, X[q], t[:, p])
            ej = np.abs(J[q].T - wj)
            assert (ej <= bj).all(), (name, m, q, "jacobian", _ratio(ej, bj))
            rf, rj = max(rf, _ratio(err, bound)), max(rj, _ratio(ej, bj))
    _record(f"specfun2 running-bound ratio {name}: residual {rf:.3f} jacobian {rj:.3f}")


# ------------------------------------------------------------------------------------------------ 2. definitions, the older kernels
def _run_rows(ds, formula, params, X, t, var="t"):
    """Value and Jacobian of a one-variable formula at the rows t for each parameter row of X, in every variant (all the
    same bits): F [npoints, m], J [npoints, n, m], and the program."""
    e = nl.Expr(formula, var, params)
    t = np.asarray(t, dtype=np.float64)
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    m = len(t)
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t[None, None]), _dev(ds, np.zeros((1, m))))       # y = 0: r = v - 0.0 is v, -0.0 included
    plist = [0] * len(X)
    out = None
    for form, chunk in VARIANTS:
        with _variant(form, chunk):
            F = _launch(ds, fcn, ctx, plist, X, m)
            J = _launch(ds, jac, ctx, plist, X, m, jac=True)
        if out is None:
            out = (F, J)
        assert _same_bits(F, out[0]) and _same_bits(J, out[1]), (formula, form, chunk)
    return out[0], out[1], e.program()


def test_a_definition_holding_a_new_function_is_the_substituted_formula(ds):
    """u = k*r; a*(2*j1(u)/u)^2+b and v = j1(k*r); ... : LOAD in the newer instantiation.  Bit for bit the device's run of the
    formula with the definition substituted."""
    r = np.linspace(0.05, 10.0, 131)
    X = np.array([[3.0, 1.2, 0.1], [2.5, 0.9, 0.15]])
    for formula in (SC.FORMULAS["airy_def"][0], "v = j1(k*r); w = 2*v/(k*r); a*w*w+b", "s = i0e(k*r); g = lgamma(1+s); a*s+b*g+expm1(-s)"):
        F, J, prog = _run_rows(ds, formula, "a,k,b", X, r, var="r")
        F2, J2, prog2 = _run_rows(ds, D.substituted(formula), "a,k,b", X, r, var="r")
        assert (prog[0] == D.LOAD).any() and not (prog2[0] == D.LOAD).any()
        assert _same_bits(F, F2) and _same_bits(J, J2), formula


def test_an_older_formula_gives_the_same_bits_around_a_new_one(ds):
    """A formula without a new function, run before and after one with: the same bits, and the restatement's (it is in the
    bit-exact class).  This shows that running a new formula leaves nothing behind that changes an older one's results.  It
    does not show which instantiation ran: an exp-free formula has the same bits in either.  That the older instantiation is
    the one chosen is in the launcher's code (the compile step sets nlh_expr::sf2 only for an opcode >= 28)."""
    t = np.linspace(0.1, 5.0, 129)
    X = np.array([[1.3, 0.7, 0.2]])
    for old in ("a/(1+((t-b)/c)^2)", "u = (t-b)/c; a/(1+u*u)"):
        F, J, prog = _run_rows(ds, old, "a,b,c", X, t)
        _run_rows(ds, "a*j0(b*t)+c*log1p(t)", "a,b,c", X, t)
        F2, J2, _ = _run_rows(ds, old, "a,b,c", X, t)
        assert _same_bits(F, F2) and _same_bits(J, J2)
        assert _same_bits(F[0], S2.value(prog, X[0], [t])) and _same_bits(J[0], S2.jacobian(prog, X[0], [t]).T)


# ------------------------------------------------------------------------------------------------ 3. edge rows
def test_edge_rows_on_the_device(ds):
    """j1(0) with tangent 1/2; i1e(0) = 0 with tangent 1/2; i0e(+-0) and its tangent -+i0e; i0e(1e6) finite; lgamma(0.5) and
    lgamma(-1.5) with its NaN tangent; expm1(1e-18) and log1p(-1e-18) exact."""
    t = np.array([0.0, -0.0, 1e6, -1e6, 8.0, -8.0])
    F, J, prog = _run_rows(ds, "i0e(p*t)", "p", [[1.0]], t)
    assert _same_bits(F[0], S2.value(prog, [1.0], [t])) and _same_bits(J[0], S2.jacobian(prog, [1.0], [t]).T)
    assert np.isfinite(F).all() and F[0][0] == F[0][1] and abs(F[0][0] - 1.0) <= SC.CONDITION and 0.0 < F[0][2] == F[0][3] < 1e-3
    F, J, prog = _run_rows(ds, "i1e(p*t)", "p", [[1.0]], t)
    assert _same_bits(F[0], S2.value(prog, [1.0], [t])) and _same_bits(J[0], S2.jacobian(prog, [1.0], [t]).T)
    assert np.array_equal(_bits(F[0][:2]), _bits([0.0, 0.0])) and F[0][2] == -F[0][3] > 0.0 and np.array_equal(_bits(J[0][0][:2]), _bits([0.0, -0.0]))
    F, J, prog = _run_rows(ds, "i1e(p+t)", "p", [[0.0]], t[:2])       # da = 1: the a == 0 row of the table, g = 0.5
    assert np.array_equal(_bits(J[0][0]), _bits([0.5, 0.5]))
    F, J, prog = _run_rows(ds, "j1(p+t)", "p", [[0.0]], t[:2])
    assert (F[0] == 0.0).all() and np.array_equal(_bits(J[0][0]), _bits([0.5, 0.5]))
    F, J, prog = _run_rows(ds, "j0(p+t)", "p", [[0.0]], t[:2])
    assert (F[0] == 1.0).all() and (J[0][0] == 0.0).all()
    F, J, prog = _run_rows(ds, "lgamma(p+t)", "p", [[0.0]], [0.5, -1.5, 1.0, 2.0])
    assert abs(F[0][0] - 0.5 * math.log(math.pi)) <= 4 * U and abs(F[0][1] - math.lgamma(-1.5)) <= 4 * U and (np.abs(F[0][2:]) <= 4 * U).all()
    assert np.isnan(J[0][0][1]) and abs(J[0][0][0] - S2.digamma(np.array([0.5]))[0]) <= 8 * U * 2.0 and np.isfinite(J[0][0][[0, 2, 3]]).all()
    F, J, prog = _run_rows(ds, "expm1(p*t)+log1p(-(q*t))", "p,q", [[1.0, 1.0]], [1e-18])
    assert F[0][0] == 1e-18 + -1e-18 and np.array_equal(_bits(J[0][:, 0]), _bits([1e-18, -1e-18]))
    F, J, prog = _run_rows(ds, "expm1(p*t)", "p", [[1.0]], [1e-18, -1e-18])
    assert np.array_equal(_bits(F[0]), _bits([1e-18, -1e-18]))
    F, J, prog = _run_rows(ds, "log1p(p*t)", "p", [[1.0]], [1e-18, -1e-18])
    assert np.array_equal(_bits(F[0]), _bits([1e-18, -1e-18]))


# ------------------------------------------------------------------------------------------------ 4. device accuracy
def test_function_accuracy(ds):
    """The seven functions through nlh_expr_eval_batch on the fixture's arguments, and digamma as lgamma's tangent, in the
    measures of specfun2_cases.MEASURES.  i0e and i1e: the restatement's bits, so within CONDITION and BOUND.  The library
    functions: the restatement's table U_F is the measured maximum rounded up to an integer and must cover what is measured
    here."""
    fx = SC.fixture()
    measured = {}
    for f in ("j0", "j1", "i0e", "i1e", "lgamma", "expm1", "log1p"):
        a = fx[SC.MEASURES[f][0]].copy()                              # (the fixture is read-only; torch wants a writable array)
        e = nl.Expr(f"{f}(t)+c", "t", "c")                            # c = 0: v + 0 is v
        got = ds.expr_eval(e, _dev(ds, np.zeros((1, 1))), _dev(ds, a)).cpu().numpy()[0]
        err, at = SC.error(f, got)
        measured[f] = err / U
        _record(f"specfun2 device accuracy {f}: {err / U:.3f} ulp of its scale at a = {at!r}; {len(a)} points"
                + (f" (table {S2.U_F[f]})" if f in S2.U_F else f" (bound {SC.BOUND[f] / U:.2f})"))
        if f in ("i0e", "i1e"):
            assert np.array_equal(_bits(got), _bits(getattr(S2, f)(a))), f
    a = fx["lg_a"].copy()
    F, J, prog = _run_rows(ds, "lgamma(p+t)", "p", [[0.0]], a)
    err, at = SC.error("digamma", J[0][0])
    _record(f"specfun2 device accuracy digamma: {err / U:.3f} ulp of max(|v|, 1) at a = {at!r}; {len(a)} points (bound {SC.BOUND['digamma'] / U:.2f})")
    assert err <= SC.BOUND["digamma"]
    for f in ("i0e", "i1e"):
        assert measured[f] * U <= min(SC.CONDITION, SC.BOUND[f]), (f, measured[f])
    for f in ("j0", "j1", "lgamma", "expm1", "log1p"):
        assert math.ceil(measured[f]) <= S2.U_F[f], (f, measured[f], S2.U_F[f])


# ------------------------------------------------------------------------------------------------ 5. fits, the oracle
def _solve(ds, fcn, jac, ctx, m, x0, analytic=True):
    x = _dev(ds, x0)
    fvec, ibs, status = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=jac if analytic else None, opts=ds.options(max_evals=SC.MAX_EVALS))
    return x.cpu().numpy(), fvec.cpu().numpy(), ibs, status


@pytest.mark.parametrize("case", ["vonmises", "airy"])
def test_fits_against_oracle(ds, oracle, case):
    """expr_fit_batch against the CPU oracle with the restatement as callback: statuses equal, x within FIT_TOL, four times
    what the library functions' ulps move the oracle's own x (specfun2_cases.fit_shift)."""
    e = SC.compile_formula(case)
    prog, t, y, xt, x0 = SC.problems(case, SC.FIT_M, nprob=SC.FIT_NPROB, prog=e.program())
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.expr_fit_batch(e, _dev(ds, t), _dev(ds, y), _dev(ds, x0), opts=ds.options(max_evals=SC.MAX_EVALS))
    xg, worst = x.cpu().numpy(), 0.0
    for p in range(SC.FIT_NPROB):
        rc, xo, fo, ibo = SC.oracle_fit(oracle, prog, t[:, p], y[p], x0[p], True)
        assert st[p] == rc == 0, (case, p, st[p], rc)
        worst = max(worst, float((np.abs(xg[p] - xo) / np.maximum(np.abs(xo), 1.0)).max()))
    print(f"{case}: device x against the oracle's, worst {worst:.3e} (tolerance {SC.FIT_TOL[case]:.3e})")
    assert worst <= SC.FIT_TOL[case], (case, worst)
    assert bool((rank == x0.shape[1]).all()) and bool((sigma > 0).all())


@pytest.mark.parametrize("analytic", [False, True])
def test_toy_fit_is_the_oracles_bit_for_bit(ds, oracle, analytic):
    """i0e and i1e only: the device's solve is the CPU oracle's with the restatement as callback -- x, fvec, counts and flags."""
    m, nprob = 129, 8
    e = SC.compile_formula("toy")
    prog, t, y, xt, x0 = SC.problems("toy", m, nprob=nprob, prog=e.program())
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    xg, fg, ibs, status = _solve(ds, fcn, jac, ctx, m, x0, analytic)
    for p in range(nprob):
        rc, xo, fo, ibo = SC.oracle_fit(oracle, prog, t[:, p], y[p], x0[p], analytic)
        assert status[p] == rc, (p, status[p], rc)
        assert _same(ibs[p], ibo), (p, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)) and np.array_equal(_bits(fg[p]), _bits(fo)), p
    assert set(status) == {0}


def test_airy_projected_against_oracle(ds, oracle):
    """Separable.for_expr(linear = a, b) on the Airy pattern: the scale alone remains; against the oracle over the restated
    projection (tests/sep_restatement.py) around the restated formula."""
    m, nprob = SC.FIT_M, SC.FIT_NPROB
    e = SC.compile_formula("airy")
    prog, t, y, xt, x0 = SC.problems("airy", m, nprob=nprob, prog=e.program())
    sp = nl.Separable.for_expr(e, linear=("a", "b"))
    alpha0 = np.ascontiguousarray(x0[:, [1]])
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    xg, fg, ibs, status = _solve(ds, wf, wj, wctx, m, alpha0)
    worst = 0.0
    for p in range(nprob):
        f, j = SC.wrapped_callbacks(prog, t[:, p], y[p], "sep")
        rc, xo, fo, ibo = oracle.lm_solve(f, m, 1, alpha0[p], jac=j, opts=oracle.default_options(max_evals=SC.MAX_EVALS))
        assert status[p] == rc == 0, (p, status[p], rc)
        worst = max(worst, float((np.abs(xg[p] - xo) / np.maximum(np.abs(xo), 1.0)).max()))
    print(f"airy projected: worst {worst:.3e} (tolerance {SC.FIT_TOL['airy/sep']:.3e})")
    assert worst <= SC.FIT_TOL["airy/sep"]
    wctx.close()


def test_gamma_pdf_poisson_against_oracle(ds, oracle):
    """stat = Poisson() on the gamma-pdf histogram model: against the oracle over the restated deviance residuals
    (tests/pois_restatement.py) around the restated formula."""
    m, nprob = SC.FIT_M, SC.FIT_NPROB
    e = SC.compile_formula("gammapdf")
    prog, t, y, xt, x0 = SC.poisson_problems(prog=e.program())
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.pois_launchers(nl.Poisson(), fcn, jac, ctx, _dev(ds, y))
    xg, fg, ibs, status = _solve(ds, wf, wj, wctx, m, x0)
    worst = 0.0
    for p in range(nprob):
        f, j = SC.wrapped_callbacks(prog, t[:, p], y[p], "pois")
        rc, xo, fo, ibo = oracle.lm_solve(f, m, 3, x0[p], jac=j, opts=oracle.default_options(max_evals=SC.MAX_EVALS))
        assert status[p] == rc == 0, (p, status[p], rc)
        worst = max(worst, float((np.abs(xg[p] - xo) / np.maximum(np.abs(xo), 1.0)).max()))
    print(f"gamma pdf, Poisson: worst {worst:.3e} (tolerance {SC.FIT_TOL['gammapdf/pois']:.3e})")
    assert worst <= SC.FIT_TOL["gammapdf/pois"]
    wctx.close()


def test_airy_band(ds):
    """expr_band on the Airy pattern: y is expr_eval's bits; sd against band_restatement.propagate of the restated Jacobian
    within the first-order bound of the Jacobian's running bound through sd = sqrt(J C J^T), plus the sums' own roundings."""
    e = SC.compile_formula("airy")
    prog = e.program()
    nprob, npts, n = 5, 131, 3
    rng = np.random.default_rng(9)
    box = np.array(SC.FORMULAS["airy"][4])
    x = rng.uniform(box[:, 0], box[:, 1], (nprob, n))
    tt = np.sort(rng.uniform(0.05, 10.0, (nprob, npts)))
    A = rng.uniform(-1.0, 1.0, (nprob, n, n))
    cov = (A @ np.transpose(A, (0, 2, 1)) + 0.5 * np.eye(n)) * 1e-4
    Jb = [S2.jacobian_bound(prog, x[p], [tt[p]]) for p in range(nprob)]
    J, eJ = np.stack([j.T for j, _ in Jb]), np.stack([b.T for _, b in Jb])
    y0 = ds.expr_eval(e, _dev(ds, x), _dev(ds, tt)).cpu().numpy()
    y, sd = ds.expr_band(e, _dev(ds, x), _dev(ds, cov), _dev(ds, tt))
    assert np.array_equal(_bits(y.cpu().numpy()), _bits(y0))
    want = BR.propagate(J, cov)
    ac = np.abs(cov)
    dv = 2.0 * np.einsum("pji,pjk,pki->pi", np.abs(J), ac, eJ) + (n * n + n) * U * np.einsum("pji,pjk,pki->pi", np.abs(J), ac, np.abs(J))
    bound = dv / (2.0 * want) + U * want
    err = np.abs(sd.cpu().numpy() - want)
    assert (err <= bound).all(), _ratio(err, bound)


def test_recovery(ds):
    """64 noisy Airy patterns and 64 noisy gamma-pdf curves: every fit returns 0 and every parameter is within 3 reported
    standard errors of its generating value in at least RECOVERY_N - 4 problems (RECOVERY_N: what the CPU oracle gives for the
    seed; tests/test_specfun2_cpu.py::test_recovery_seed_on_the_oracle asserts it)."""
    for name in SC.RECOVERY:
        e = SC.compile_formula(name)
        prog, t, y, xt, x0 = SC.recovery_problems(name, e.program())
        x, fvec, sigma, cov, chi2, rank, ibs, st = ds.expr_fit_batch(e, _dev(ds, t), _dev(ds, y), _dev(ds, x0), opts=ds.options(max_evals=SC.MAX_EVALS))
        assert set(st) == {0} and bool((rank == x0.shape[1]).all()), name
        good = int((np.abs(x.cpu().numpy() - xt) <= 3.0 * sigma.cpu().numpy()).all(axis=1).sum())
        print(f"{name} recovery: {good} of {len(y)} within 3 standard errors")
        assert good >= SC.RECOVERY_N[name] - 4, name
