"""GPU tests of the formulas' pow, atan2, min, max and where (include/nonlin_hip.h: NLH_EXPR_POW .. NLH_EXPR_WHERE): the
interpreter on a ten-parameter piecewise formula bit for bit against the numpy restatement (tests/pwfun_restatement.py) in
both workgroup forms, at their size edges and for every chunk of Jacobian columns; the presence patterns and the edge rows
of the header's table -- ties, signed zeros, NaN, the branch not taken, POW at a = 0 -- by bits; the device library's pow
with a fitted exponent and atan2 in ulp against numpy.longdouble, which the running bound's table rests on, and formulas
that use them within that bound; hinge solves bit for bit against the CPU oracle over the restatement, alone, boxed,
through a parameter map and a projection; the one-call fit as the composition it stands for; recovery of noisy power laws
sampled from t = 0."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import expr_cases as EC
import pmap_restatement as PR
import pwfun_cases as PC
import pwfun_restatement as W
import sep_cases as SEPC
import nonlin_amd as nl

pytestmark = pytest.mark.gpu

KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
# (NLH_EXPR_FORM, NLH_EXPR_CHUNK): what m and the depth select; each form forced (one that cannot hold m falls back); one
# Jacobian column per pass
VARIANTS = [(None, None), ("row", None), ("flat", None), (None, "1")]
NAN, INF = float("nan"), float("inf")


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_bits(got, want):
    """Bit equality, a NaN matching any NaN (the payload and sign of a NaN are not part of the table)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(want[~nan]))


def _same(a, b):
    return all(a[k] == b[k] for k in KEYS)


def _eq(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


def _record(line):
    """Print a measured figure; append it to the file NLH_PWFUN_FILE names, when it names one (profiles/pwfun_accuracy.txt)."""
    print(line)
    path = os.environ.get("NLH_PWFUN_FILE")
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


# ------------------------------------------------------------------------------------------------ 1. the exact class
@pytest.mark.parametrize("m", [5, 128, 129, 257])
@pytest.mark.parametrize("weighted,shared", [(False, False), (True, False), (False, True), (True, True)])
def test_piecewise_kernels_bitwise(ds, weighted, shared, m):
    """Two hinges, a min and a where onset, ten parameters: the first chunk holds 8 columns at most, so the Jacobian takes two
    passes (one per column with NLH_EXPR_CHUNK = 1).  m = 5 and 128: the flat form -- 51 and 2 points per workgroup, the
    60-point list ending in a partial workgroup for m = 5; m = 129 and 257: the row form, one partial block, and a second
    block of one row.  Every predicate compares exact values, so no row is excluded."""
    nprob = 7
    e = PC.compile_formula("piecewise")
    prog, t, y, xt, x0 = PC.problems("piecewise", m, nprob=nprob, seed=11 + m, prog=e.program())
    n = x0.shape[1]
    assert n == 10
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
        wantF = [W.residual(prog, X[q], t[:, p], y[p], w[p] if weighted else None) for q, p in enumerate(plist)]
        wantJ = [W.jacobian(prog, X[q], t[:, p], w[p] if weighted else None).T for q, p in enumerate(plist)]
        for form, chunk in VARIANTS:
            with _variant(form, chunk):
                F = _launch(ds, fcn, ctx, plist, X, m)
                J = _launch(ds, jac, ctx, plist, X, m, jac=True)
            for q, p in enumerate(plist):
                assert np.array_equal(_bits(F[q]), _bits(wantF[q])), (form, chunk, k, q)
                assert np.array_equal(_bits(J[q]), _bits(wantJ[q])), (form, chunk, k, q)
                if weighted:                                           # a zero-weight row is exactly 0
                    assert (F[q][w[p] == 0.0] == 0.0).all() and (J[q][:, w[p] == 0.0] == 0.0).all()
    if m >= 128 and not weighted:                                      # every selection goes both ways within a data set
        v = t[0, 0]
        assert ((v - x0[0, 2]) > 0).any() and ((v - x0[0, 2]) < 0).any() and ((v - x0[0, 7]) >= 0).any() and ((v - x0[0, 7]) < 0).any()
        assert (x0[0, 5] * v < x0[0, 6]).any() and (x0[0, 5] * v > x0[0, 6]).any()


# ------------------------------------------------------------------------------------------------ 2. patterns, edge rows
def _run_rows(ds, formula, params, X, t):
    """Value and Jacobian of a one-variable formula at the rows t for each parameter row of X, in every variant (all the
    same bits): F [npoints, m], J [npoints, n, m], and the program."""
    e = nl.Expr(formula, "t", params)
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


@pytest.mark.parametrize("formula,params", PC.PATTERNS)
def test_presence_patterns_on_the_device(ds, formula, params):
    """The tangent on a only, on b only, on both, a parameter in both operands; where with the tangent in each operand and in
    the condition alone.  Selections: the restatement's bits.  POW and ATAN2: within the running bound, entry by entry."""
    names = params.split(",")
    rng = np.random.default_rng(len(formula))
    X = np.array([[PC.PATTERN_X[k] for k in names]] * 3)
    X[1:] *= 1.0 + 0.05 * rng.uniform(-1, 1, (2, len(names)))
    t = np.linspace(0.0, 3.0, 49)                                      # t = 1.25 is in it: a where whose c is exactly 0
    F, J, prog = _run_rows(ds, formula, params, X, t)
    exact = not formula.startswith(("pow", "atan2"))
    for q in range(3):
        if exact:
            assert np.array_equal(_bits(F[q]), _bits(W.value(prog, X[q], [t]))), formula
            assert np.array_equal(_bits(J[q]), _bits(W.jacobian(prog, X[q], [t]).T)), formula
        else:
            want, bound = W.residual_bound(prog, X[q], [t], np.zeros(49))
            assert (np.abs(F[q] - want) <= bound).all(), (formula, _ratio(np.abs(F[q] - want), bound))
            wj, bj = W.jacobian_bound(prog, X[q], [t])
            assert (np.abs(J[q].T - wj) <= bj).all(), (formula, "jacobian")
    if formula == "where(t-p,1+t,2)":                                  # only the condition names p: the column is there and +0.0
        assert np.array_equal(_bits(J[:, 0]), _bits(np.zeros((3, 49))))


def test_min_max_edge_rows_on_the_device(ds):
    """Ties keep a, signed zeros included; a NaN b is dropped, a NaN a stays; the tangent follows the selection."""
    t = np.array([0.0, -0.0, 1.0, NAN, 2.0])
    for f in ("max", "min"):
        for formula, x in ((f"{f}(t,p)", 0.0), (f"{f}(p,t)", 0.0), (f"{f}(p,-t)", -0.0), (f"{f}(t,p)", 1.0), (f"{f}(p,t)", NAN), (f"{f}(t*p,t)", 1.0)):
            F, J, prog = _run_rows(ds, formula, "p", [[x]], t)
            assert _same_bits(F[0], W.value(prog, np.array([x]), [t])), (formula, x, F[0])
            assert _same_bits(J[0], W.jacobian(prog, np.array([x]), [t]).T), (formula, x, J[0])
    F, J, prog = _run_rows(ds, "max(t,p)", "p", [[0.0]], t)
    assert np.array_equal(_bits(F[0][:3]), _bits([0.0, -0.0, 1.0])) and np.isnan(F[0][3]) and np.array_equal(_bits(J[0][0]), _bits([0.0, 0.0, 0.0, 0.0, 0.0]))
    F, J, prog = _run_rows(ds, "max(p,t)", "p", [[0.0]], t)
    assert np.array_equal(_bits(F[0]), _bits([0.0, 0.0, 1.0, 0.0, 2.0])) and np.array_equal(_bits(J[0][0]), _bits([1.0, 1.0, 0.0, 1.0, 0.0]))


def test_where_edge_rows_on_the_device(ds):
    """-0.0 selects a, NaN selects b; sqrt of a negative number in the branch not taken: exact +0.0 in value and tangent."""
    t = np.array([-0.0, 0.0, NAN, -1e-300, 1e-300])
    F, J, prog = _run_rows(ds, "where(t,p,q)", "p,q", [[2.0, 3.0]], t)
    assert np.array_equal(_bits(F[0]), _bits([2.0, 2.0, 3.0, 3.0, 2.0]))
    assert np.array_equal(_bits(J[0]), _bits([[1.0, 1.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0, 0.0]]))
    t = np.array([-4.0, -1.0, -1e-9, 0.0, 1.0, 4.0])
    F, J, prog = _run_rows(ds, "where(t,p*sqrt(t),0)", "p", [[3.0]], t)
    assert np.array_equal(_bits(F[0]), _bits([0.0, 0.0, 0.0, 0.0, 3.0, 6.0])) and np.array_equal(_bits(J[0][0]), _bits([0.0, 0.0, 0.0, 0.0, 1.0, 2.0]))
    F, J, prog = _run_rows(ds, "where(t-p,sqrt(t-p),0)", "p", [[0.5]], t)
    assert np.array_equal(_bits(F[0]), _bits(W.value(prog, np.array([0.5]), [t]))) and np.array_equal(_bits(J[0]), _bits(W.jacobian(prog, np.array([0.5]), [t]).T))
    assert np.array_equal(_bits(F[0][:4]), _bits(np.zeros(4))) and np.array_equal(_bits(J[0][0][:4]), _bits(np.zeros(4))) and np.isfinite(J).all()
    F, J, prog = _run_rows(ds, "where(t,1/t,p)", "p", [[7.0]], [0.0, -0.0])
    assert np.array_equal(_bits(F[0]), _bits([INF, -INF])) and np.array_equal(_bits(J[0][0]), _bits([0.0, 0.0]))


def test_pow_at_zero_on_the_device(ds):
    """a = 0: gb is +0.0 and the da guard holds -- the t = 0 row is exact, the others within the running bound."""
    t = np.array([0.0, 0.5, 2.0, 3.75])
    for formula, params, x, row0 in (("a*pow(t,b)+c", "a,b,c", [1.3, 0.7, 0.2], [0.0, 0.0, 1.0]),
                                     ("a*exp(-pow(t/tau,beta))+c", "a,tau,beta,c", [1.3, 1.1, 0.6, 0.1], [1.0, -0.0, -0.0, 1.0]),
                                     ("a*exp(-pow(t/tau,beta))+c", "a,tau,beta,c", [1.3, 1.1, 1.4, 0.1], [1.0, -0.0, -0.0, 1.0])):
        x = np.array(x)
        F, J, prog = _run_rows(ds, formula, params, [x], t)
        assert np.isfinite(F).all() and np.isfinite(J).all()
        assert np.array_equal(_bits(J[0][:, 0]), _bits(row0)), (formula, J[0][:, 0])
        want, bound = W.residual_bound(prog, x, [t], np.zeros(4))
        wj, bj = W.jacobian_bound(prog, x, [t])
        assert (np.abs(F[0] - want) <= bound).all() and (np.abs(J[0].T - wj) <= bj).all(), formula
    F, J, prog = _run_rows(ds, "pow(t-p,b)", "p,b", [[3.0, 2.0]], t[:3])          # a negative base, a fitted exponent: outside the domain
    assert np.isnan(J[0][1]).all() and (np.abs(F[0] - [9.0, 6.25, 1.0]) <= 3 * 2.0 ** -52 * np.array([9.0, 6.25, 1.0])).all()


# ------------------------------------------------------------------------------------------------ 3. device accuracy
def _ulps(got, ref):
    """|got - ref| in units of the float64 spacing at ref (ref: numpy.longdouble)."""
    r64 = np.abs(ref).astype(np.float64)
    return np.abs(got.astype(np.longdouble) - ref) / np.spacing(r64).astype(np.longdouble)


def test_pow_and_atan2_accuracy(ds):
    """pow(a, b) with b a parameter and atan2 in ulp, through nlh_expr_eval_batch against numpy.longdouble.  POW: the bases of
    expr_cases.ACCURACY_RANGES["pow"] (log-uniform) times 38 exponents in [-2.5, 2.5], the literal ones of the POWC test among
    them -- the same device function, held to the same U_F.  ATAN2: [-20, 20]^2 away from the origin (radius >= 1/16).  The
    restatement's table U_F is the measured maximum rounded up to an integer: it must cover what is measured here."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is no wider than float64 here: nothing to measure against"
    rng = np.random.default_rng(13)
    npts = 1 << 14
    lo, hi = EC.ACCURACY_RANGES["pow"]
    t = np.exp(rng.uniform(math.log(lo), math.log(hi), npts))
    b = np.concatenate((EC.POW_EXPONENTS, rng.uniform(-2.5, 2.5, 32)))
    e = nl.Expr("pow(t,b)+a", "t", "b,a")                                # a = 0: v + 0 is v
    got = ds.expr_eval(e, _dev(ds, np.stack((b, np.zeros(len(b))), axis=1)), _dev(ds, t)).cpu().numpy()
    ref = np.power(t.astype(np.longdouble)[None, :], b.astype(np.longdouble)[:, None])
    ulp = _ulps(got, ref)
    k = np.unravel_index(np.argmax(ulp), ulp.shape)
    measured = {"pow": float(ulp.max())}
    _record(f"pwfun device accuracy pow(a, b), b a parameter: {measured['pow']:.3f} ulp at a = {float(t[k[1]])!r}, b = {float(b[k[0]])!r}; "
            f"{npts} bases in [{lo}, {hi}] x {len(b)} exponents in [-2.5, 2.5] (table {W.U_F['pow']})")
    npts = 1 << 18
    uv = rng.uniform(-20.0, 20.0, (2, npts))
    uv = np.ascontiguousarray(uv[:, np.hypot(uv[0], uv[1]) >= 1.0 / 16.0])
    uv[:, :8] = [[0.0, 0.0, 3.0, -3.0, 1e-3, -1e-3, 20.0, -20.0], [2.0, -2.0, 0.0, 0.0, -20.0, -20.0, 1e-3, -1e-3]]   # the axes, next to the cut
    e = nl.Expr("atan2(u,v)+a", "u,v", "a")
    got = ds.expr_eval(e, _dev(ds, np.zeros((1, 1))), _dev(ds, uv)).cpu().numpy()[0]
    ref = np.arctan2(uv[0].astype(np.longdouble), uv[1].astype(np.longdouble))
    ok = ref != 0.0                                                     # atan2(0, v > 0) = 0 exactly
    assert (got[~ok] == 0.0).all()
    ulp = _ulps(got[ok], ref[ok])
    k = int(np.argmax(ulp))
    measured["atan2"] = float(ulp.max())
    _record(f"pwfun device accuracy atan2(y, x): {measured['atan2']:.3f} ulp at y = {float(uv[0][ok][k])!r}, x = {float(uv[1][ok][k])!r}; "
            f"{int(ok.sum())} points of [-20, 20]^2 at radius >= 1/16 (table {W.U_F['atan2']})")
    for f, worst in measured.items():
        assert math.ceil(worst) <= W.U_F[f], (f, worst, W.U_F[f])


# ------------------------------------------------------------------------------------------------ 4. within the running bound
def _ratio(err, bound):
    """The largest |device - numpy| / bound over the entries whose bound is not 0 (those are compared by <=, that is exactly)."""
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


@pytest.mark.parametrize("name", PC.WITH_FUNCTIONS)
def test_library_formulas_within_running_bound(ds, name):
    """The power law and the stretched exponential from t = 0, the phase model: |device - numpy| <= the restatement's
    first-order running bound, residual and Jacobian, entry by entry (a bound of 0 -- the t = 0 row's zeros -- is bit
    equality)."""
    nprob = 6
    e = PC.compile_formula(name)
    rf = rj = 0.0
    for m in (64, 200):
        prog, t, y, xt, x0 = PC.problems(name, m, nprob=nprob, prog=e.program(), zero=name != "phase")
        assert name == "phase" or (t[0, :, 0] == 0.0).all()
        w = np.random.default_rng(2).uniform(0.5, 2.0, (nprob, m))
        w[:, 3] = 0.0
        dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
        for wd, wh in ((None, None), (dw, w)):
            fcn, jac, ctx = ds.expr_launchers(e, dt, dy, wd)
            plist = list(range(nprob)) + [1, 1]
            X = _points(x0, plist, 20)
            F = _launch(ds, fcn, ctx, plist, X, m)
            J = _launch(ds, jac, ctx, plist, X, m, jac=True)
            assert np.isfinite(F).all() and np.isfinite(J).all()
            for q, p in enumerate(plist):
                wp = wh[p] if wh is not None else None
                want, bound = W.residual_bound(prog, X[q], t[:, p], y[p], wp)
                err = np.abs(F[q] - want)
                assert (err <= bound).all(), (name, m, q, _ratio(err, bound))
                rf = max(rf, _ratio(err, bound))
                wj, bj = W.jacobian_bound(prog, X[q], t[:, p], wp)
                ej = np.abs(J[q].T - wj)
                assert (ej <= bj).all(), (name, m, q, "jacobian", _ratio(ej, bj))
                rj = max(rj, _ratio(ej, bj))
    _record(f"pwfun running-bound ratio {name}: residual {rf:.3f} jacobian {rj:.3f}")


# ------------------------------------------------------------------------------------------------ 5. hinge solves, the oracle
def _box(xt):
    """A box that binds for some problems: the second slope is capped at the mean of the true ones."""
    lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
    upper[2] = xt[:, 2].mean()
    return lower, upper


def _check(status, ibs, xg, fg, p, rc, xo, fo, ibo, what):
    assert status[p] == rc, (what, p, status[p], rc)
    assert _same(ibs[p], ibo), (what, p, ibs[p], ibo)
    assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, p, np.abs(xg[p] - xo).max())
    assert np.array_equal(_bits(fg[p]), _bits(fo)), (what, p)


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("analytic", [False, True])
def test_hinge_solves_against_oracle(ds, oracle, analytic, bounded):
    """max is a selection: the device's solve is the CPU oracle's with the restatement as callback, bit for bit in x, fvec,
    counts and flags."""
    m, nprob = 129, 8
    e = PC.compile_formula("hinge")
    prog, t, y, xt, x0 = PC.problems("hinge", m, nprob=nprob, prog=e.program())
    n = x0.shape[1]
    opt = dict(max_evals=PC.MAX_EVALS)
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
        f = lambda xx, ff: ff.__setitem__(slice(None), W.residual(prog, xx, tv, y[p]))
        j = (lambda xx, JJ: JJ.__setitem__((slice(None), slice(None)), W.jacobian(prog, xx, tv))) if analytic else None
        if bounded:
            rc, xo, fo, ibo = oracle.cls_solve(f, m, n, x0[p], jac=j, opts=oo, lower=lower, upper=upper)
        else:
            rc, xo, fo, ibo = oracle.lm_solve(f, m, n, x0[p], jac=j, opts=oo)
        _check(status, ibs, xg, fg, p, rc, xo, fo, ibo, (analytic, bounded))
    if not bounded:
        assert set(status) == {0}, sorted(set(status))


@pytest.mark.parametrize("analytic", [False, True])
def test_hinge_through_a_map_against_oracle(ds, oracle, analytic):
    """ParamMap.for_expr fixes the knot t0 (a known change point): the oracle on the reduced problem, the restated expand and
    contract around the restated formula as callbacks."""
    m, nprob = 128, 4
    e = PC.compile_formula("hinge")
    prog, t, y, xt, x0 = PC.problems("hinge", m, nprob=nprob, prog=e.program())
    pm = nl.ParamMap.for_expr(e, fixed=("t0",))
    T = PR.tables(4, [3], {})
    for g, w_ in zip(pm.tables(), T):
        assert np.array_equal(g, w_)
    n = len(T[4])
    assert n == 3
    full = np.ascontiguousarray(x0)
    full[:, 3] = xt[:, 3]
    dfull = _dev(ds, full)
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, dfull)
    x = ds.pmap_gather(pm, dfull)
    o = dict(max_evals=PC.MAX_EVALS)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options(**o))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**o)
    for p in range(nprob):
        tv = t[:, p]
        f = lambda xx, out: out.__setitem__(slice(None), W.residual(prog, PR.expand(T, xx, full[p]), tv, y[p]))
        j = (lambda xx, J: J.__setitem__((slice(None), slice(None)), PR.contract(T, W.jacobian(prog, PR.expand(T, xx, full[p]), tv)))) if analytic else None
        rc, xo, fo, ibo = oracle.lm_solve(f, m, n, PR.gather(T, full[p]), jac=j, opts=oo)
        _check(status, ibs, xg, fg, p, rc, xo, fo, ibo, ("map", analytic))
    assert set(status) == {0}
    wctx.close()


@pytest.mark.parametrize("analytic", [False, True])
def test_hinge_projected_against_oracle(ds, oracle, analytic):
    """Separable.for_expr(linear = b, s1, s2): the intercept and both slopes are projected out, the knot alone remains."""
    m, nprob = 128, 4
    e = PC.compile_formula("hinge")
    prog, t, y, xt, x0 = PC.problems("hinge", m, nprob=nprob, prog=e.program())
    sp = nl.Separable.for_expr(e, linear=("b", "s1", "s2"))
    lin, nonlin = [0, 1, 2], [3]
    alpha0 = np.ascontiguousarray(x0[:, nonlin])
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    x = _dev(ds, alpha0)
    o = dict(max_evals=PC.MAX_EVALS)
    fvec, ibs, status = ds.lm_solve_batch_device(wf, wctx, m, x, jac=wj if analytic else None, opts=ds.options(**o))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    oo = oracle.default_options(**o)
    for p in range(nprob):
        tv = t[:, p]
        f, j = SEPC.oracle_callbacks(lambda P: W.residual(prog, P, tv, y[p]), lambda P: W.jacobian(prog, P, tv), 4, lin, analytic)
        rc, xo, fo, ibo = oracle.lm_solve(f, m, 1, alpha0[p], jac=j, opts=oo)
        _check(status, ibs, xg, fg, p, rc, xo, fo, ibo, ("sep", analytic))
    assert set(status) == {0}
    wctx.close()


# ------------------------------------------------------------------------------------------------ 6. the one-call fit
def _fit_by_hand(ds, e, dt, dy, x0, m, analytic, o):
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy, None)
    j = jac if analytic else None
    x = x0.clone()
    fvec, ibs, st = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=j, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(fcn, ctx, m, x, jac=j, scaled=True)
    return x, fvec, sigma, cov, chi2, rank, ibs, st


@pytest.mark.parametrize("analytic", [False, True])
def test_fit_batch_is_the_composition(ds, analytic):
    """expr_fit_batch of the power law, t = 0 in every data set = solve, then covariance, by hand; a problem alone gives its
    bits in the batch."""
    m, nprob = 64, 8
    e = PC.compile_formula("powerlaw")
    prog, t, y, xt, x0 = PC.problems("powerlaw", m, nprob=nprob, prog=e.program(), zero=True)
    n = x0.shape[1]
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=PC.MAX_EVALS)
    got = ds.expr_fit_batch(e, dt, dy, dx0, analytic=analytic, opts=o)
    want = _fit_by_hand(ds, e, dt, dy, dx0, m, analytic, o)
    assert _eq(got[0], want[0]) and _eq(got[1], want[1]) and got[6] == want[6] and got[7] == want[7]
    assert set(got[7]) == {0}, got[7]
    for g, w_ in zip(got[2:6], want[2:6]):
        assert _eq(g, w_)
    assert bool((got[5] == n).all()) and bool((got[2] > 0).all()) and bool(torch.isfinite(got[0]).all())
    for p in (0, nprob - 1):
        one = ds.expr_fit_batch(e, dt[:, p:p + 1].contiguous(), dy[p:p + 1].contiguous(), dx0[p:p + 1].contiguous(), analytic=analytic, opts=o)
        for g, w_ in zip(one[:6], got[:6]):
            assert _eq(g, w_[p:p + 1]), p
        assert one[6][0] == got[6][p] and one[7][0] == got[7][p]


def test_recovery(ds):
    """64 noisy power laws on a grid that starts at t = 0: every fit returns 0 and every parameter is within 3 reported standard
    errors of its generating value in at least RECOVERY_N - 4 problems (RECOVERY_N: what the CPU oracle gives for the seed;
    tests/test_pwfun_cpu.py::test_recovery_seed_on_the_oracle asserts it)."""
    e = PC.compile_formula("powerlaw")
    prog, t, y, xt, x0 = PC.recovery_problems(e.program())
    assert t[0] == 0.0
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.expr_fit_batch(e, _dev(ds, t), _dev(ds, y), _dev(ds, x0), opts=ds.options(max_evals=PC.MAX_EVALS))
    assert set(st) == {0} and bool((rank == 3).all())
    good = int((np.abs(x.cpu().numpy() - xt) <= 3.0 * sigma.cpu().numpy()).all(axis=1).sum())
    print(f"power-law recovery: {good} of {len(y)} within 3 standard errors")
    assert good >= PC.RECOVERY_N - 4
