"""GPU tests of the formula interpreter at its documented limits (include/nonlin_hip.h: 256 instructions, 64 constants, stack
depth 16, 4 variables, 32 parameters), where the everyday formulas of tests/test_gpu_expr.py never take it: launches above
64 KB of dynamic LDS, Jacobian passes of 1 < C < n columns with a shorter last pass, passes skipped because the formula names
none of their columns, parameter bit 31, operand-root fields at and above 128, variables 3 and 4 and a padded stride between
their blocks, and m at the edges of the flat form.  Every program is in the bit-exact class: the kernels are held to the numpy
restatement bit for bit (tests/expr_limit_cases.py), under every form and chunk override, and every output is checked to be
finite first -- the launch helper prefills it with NaN, so a launch that did not happen fails as that."""
import ctypes as C

import numpy as np
import pytest
import torch

import expr_cases as EC
import expr_limit_cases as LC
import expr_restatement as R
import nonlin_amd as nl
from nonlin_amd import _lib
from nonlin_amd.device import expr_plan
from test_gpu_expr import _bits, _dev, _eq, _fit_by_hand, _launch, _points, _same, _shapes, _variant, _weights

pytestmark = pytest.mark.gpu

FORMS = [(None, None), ("row", None), ("flat", None)]
# NLH_EXPR_CHUNK values that leave a shorter last pass (n = 32: 2 | 32, so wide32's default 5 and 3 do; deep16's default is 1)
CHUNKS = {"deep16": [], "wide32": ["1", "2", "3", "4"], "full256": ["1", "3", "5", "7"], "where256": ["1", "3", "5", "7"],
          "vars4": ["1", "3", "5", "7"], "sparse32": ["1", "3", "5"]}


def _compile(name):
    return LC.compile_formula(name) if name in LC.FORMULAS else EC.compile_formula(name)


def _problems(name, m, nprob, seed, prog):
    if name in LC.FORMULAS:
        return LC.limit_problems(name, m, nprob=nprob, seed=seed, prog=prog)
    return EC.expr_problems(name, m, nprob=nprob, seed=seed, prog=prog)


def _both(ds, fcn, jac, ctx, plist, X, m, what):
    """F [npoints, m] and J [npoints, n, m] of one launch each, finite everywhere."""
    F = _launch(ds, fcn, ctx, plist, X, m)
    J = _launch(ds, jac, ctx, plist, X, m, jac=True)
    assert np.isfinite(F).all() and np.isfinite(J).all(), what
    return F, J


def _same_bits(got, want, what):
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (what, "residual")
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "jacobian")


# ------------------------------------------------------------------------------------------------ a. the limit programs
@pytest.mark.parametrize("m", [5, 129])
@pytest.mark.parametrize("weighted,shared", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", list(LC.FORMULAS))
def test_limit_programs_bitwise(ds, name, weighted, shared, m):
    nprob = 5
    e = LC.compile_formula(name)
    prog, t, y, xt, x0 = LC.limit_problems(name, m, nprob=nprob, seed=11 + m, prog=e.program())
    n = x0.shape[1]
    if shared:
        t = np.ascontiguousarray(np.broadcast_to(t[:, :1], t.shape))
    w = _weights(np.random.default_rng(m), nprob, m) if weighted else None
    dt, dy, dw = _dev(ds, t[:, 0] if shared else t), _dev(ds, y), (_dev(ds, w) if weighted else None)
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy, dw)
    variants = FORMS + [(None, c) for c in CHUNKS[name]]
    with _variant(None):
        assert expr_plan(e.depth, n, m)["flat"] == (m == 5)
    for k, plist in enumerate(_shapes(nprob, n)):
        X = _points(x0, plist, k)
        want = LC.restate(prog, X, t[:, plist], y[plist], w[plist] if weighted else None)
        for form, chunk in variants:
            with _variant(form, chunk):
                got = _both(ds, fcn, jac, ctx, plist, X, m, (name, form, chunk, k))
            _same_bits(got, want, (name, form, chunk, k))
    for q in (0, 17, len(plist) - 1):                               # a point alone: the bits it has inside the mixed list
        one = _both(ds, fcn, jac, ctx, plist[q:q + 1], X[q:q + 1], m, (name, q))
        _same_bits(one, (want[0][q:q + 1], want[1][q:q + 1]), (name, "alone", q))


# ------------------------------------------------------------------------------------------------ b. chunk tails, n = 5, 6
@pytest.mark.parametrize("m", [5, 129])
@pytest.mark.parametrize("name,chunks", [("rational", ["2", "3", "4"]), ("lorentz2", ["4", "5"])])
def test_chunk_tails_on_the_everyday_formulas(ds, name, chunks, m):
    """A pass of 1 < C < n columns and a shorter last one: the default's bits, and the restatement's."""
    nprob = 5
    e = EC.compile_formula(name)
    prog, t, y, xt, x0 = EC.expr_problems(name, m, nprob=nprob, seed=3 + m, prog=e.program())
    n = x0.shape[1]
    w = _weights(np.random.default_rng(m), nprob, m)
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y), _dev(ds, w))
    with _variant(None):
        assert expr_plan(e.depth, n, m)["chunk"] == 5               # (rational: every column; lorentz2, depth 6: five of six)
    plist = _shapes(nprob, n)[2]
    X = _points(x0, plist, 4)
    want = LC.restate(prog, X, t[:, plist], y[plist], w[plist])
    with _variant(None):
        base = _both(ds, fcn, jac, ctx, plist, X, m, (name, m))
    _same_bits(base, want, (name, m))
    for chunk in chunks:
        with _variant(None, chunk):
            assert expr_plan(e.depth, n, m)["chunk"] == int(chunk) and n % int(chunk)
            got = _both(ds, fcn, jac, ctx, plist, X, m, (name, m, chunk))
        _same_bits(got, base, (name, m, chunk))


# ------------------------------------------------------------------------------------------------ c. m at the forms' edges
@pytest.mark.parametrize("name,m", [("rational", m) for m in (1, 2, 3, 85, 86, 127, 255, 512, 513)] + [("wide32", m) for m in (1, 86, 257)])
def test_m_edges(ds, name, m):
    """m = 1, 2; three points per workgroup with an idle thread (85) and the switch to two (86); the last flat m by default
    (127 < 128) and forced (255); two and three row blocks; lists of 1 and 7 points and one that leaves the last flat
    workgroup with a single point."""
    nprob = 5
    e = _compile(name)
    prog, t, y, xt, x0 = _problems(name, m, nprob, 40 + m, e.program())
    n = x0.shape[1]
    w = _weights(np.random.default_rng(m), nprob, m)
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y), _dev(ds, w))
    plans = {}
    for form, chunk in FORMS:
        with _variant(form):
            plans[form] = expr_plan(e.depth, n, m)
    assert plans[None]["flat"] == (m <= 128) and plans["flat"]["flat"] == (m <= 256) and not plans["row"]["flat"]
    assert plans["flat"]["ppw"] == (256 // m if m <= 256 else 1) and plans["row"]["nblk"] == -(-m // 256)
    most = max(7, max(p["ppw"] for p in plans.values()) + 1)
    plist = list(np.random.default_rng(m).integers(0, nprob, most))
    X = _points(x0, plist, 5)
    want = LC.restate(prog, X, t[:, plist], y[plist], w[plist])
    for form, chunk in FORMS:
        for count in (1, 7, plans[form]["ppw"] + 1):
            with _variant(form):
                got = _both(ds, fcn, jac, ctx, plist[:count], X[:count], m, (name, m, form, count))
            _same_bits(got, (want[0][:count], want[1][:count]), (name, m, form, count))


# ------------------------------------------------------------------------------------------------ d. the largest launch
def test_largest_lds_launch(ds):
    """Depth 16, n = 32, m = 1: 256 points per workgroup stage 64 KB of x beside two 32 KB stacks -- 131,072 bytes, the most
    the Jacobian kernel ever asks for, and 98,304 for the residual kernel; both above the 64 KB a kernel gets unasked."""
    e = nl.Expr(*LC.DEEP16_PADDED)
    n, m, nprob, npoints = 32, 1, 7, 300
    assert (e.nparams, e.depth) == (n, 16)
    with _variant(None):
        assert expr_plan(16, n, m, npoints) == {"flat": True, "ppw": 256, "nblk": 1, "grid": 2, "chunk": 1, "lds_bytes": 131072}
        assert expr_plan(16, n, m, npoints, jac=False)["lds_bytes"] == 98304
    rng = np.random.default_rng(16)
    t, y, x0 = rng.uniform(0.0, 1.0, (1, nprob, m)), rng.uniform(-1.0, 1.0, (nprob, m)), rng.uniform(0.5, 1.5, (nprob, n))
    w = rng.uniform(0.5, 2.0, (nprob, m))
    plist = list(rng.integers(0, nprob, npoints))
    X = _points(x0, plist, 6)
    prog = e.program()
    for wh in (None, w):
        fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y), _dev(ds, wh) if wh is not None else None)
        want = LC.restate(prog, X, t[:, plist], y[plist], wh[plist] if wh is not None else None)
        with _variant(None):
            got = _both(ds, fcn, jac, ctx, plist, X, m, "largest")
        _same_bits(got, want, "largest")
        assert (_bits(got[1][:, 15:]) == 0).all() and (got[1][:, :15] != 0).all()     # the unused names: +0.0


# ------------------------------------------------------------------------------------------------ e. skipped passes
@pytest.mark.parametrize("m", [5, 129])
def test_sparse32_skipped_passes_and_zero_columns(ds, m):
    """p31*t-p0 names two of 32 parameters: column 0 is -1.0, column 31 is t, the thirty between are +0.0 -- the bit pattern,
    not a value equal to zero -- also when whole passes are skipped (default: 8 columns a pass, passes 2 and 3; chunk 3: nine
    of eleven; chunk 5: five of seven) and in a pass of one column; weights multiply through."""
    nprob = 5
    e = LC.compile_formula("sparse32")
    prog, t, y, xt, x0 = LC.limit_problems("sparse32", m, nprob=nprob, seed=m, prog=e.program())
    w = np.random.default_rng(m).uniform(0.5, 2.0, (nprob, m))
    plist = _shapes(nprob, 32)[2]
    X = _points(x0, plist, 7)
    tq = t[0, plist]
    with _variant(None):
        assert expr_plan(e.depth, 32, m)["chunk"] == 8
    for wh in (None, w):
        fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y), _dev(ds, wh) if wh is not None else None)
        wq = wh[plist] if wh is not None else np.ones_like(tq)
        for chunk in (None, "1", "3", "5"):
            with _variant(None, chunk):
                F, J = _both(ds, fcn, jac, ctx, plist, X, m, (m, chunk))
            what = (m, chunk, wh is not None)
            assert (_bits(J[:, 1:31]) == 0).all(), what
            assert np.array_equal(_bits(J[:, 0]), _bits(wq * -1.0)) and np.array_equal(_bits(J[:, 31]), _bits(wq * tq)), what
            assert np.array_equal(_bits(F), _bits(wq * ((X[:, 31:32] * tq - X[:, 0:1]) - y[plist]))), what


# ------------------------------------------------------------------------------------------------ f. four variables, a stride
def _by_hand(ds, e, shared, m, dt, dy, stride):
    ctx = _lib.ExprCtx(e.ptr, int(shared), m, dt.data_ptr(), dy.data_ptr(), None, stride)
    ctx._keep = (e, dt, dy)
    return C.cast(ds.lib.nlh_expr_device_fcn, _lib.DEVFCN), C.cast(ds.lib.nlh_expr_device_jac, _lib.DEVFCN), ctx


@pytest.mark.parametrize("m", [5, 129])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("which", ["vars4", "vars3"])
def test_variables_with_a_padded_stride(ds, which, shared, m):
    """dt_stride is the distance between the variables' blocks, whatever lies between them: nprob*m + 7 (shared: m + 3) with
    NaN in the gaps gives the bits of the tight layout, for four variables and for three."""
    nprob = 5
    if which == "vars4":
        e = LC.compile_formula("vars4")
        prog, t, y, xt, x0 = LC.limit_problems("vars4", m, nprob=nprob, seed=m, prog=e.program())
    else:
        e = nl.Expr("p0*x+p1*y*z", "x,y,z", "p0,p1")
        prog = e.program()
        rng = np.random.default_rng(m)
        t, y, x0 = rng.uniform(-1.0, 1.0, (3, nprob, m)), rng.uniform(-1.0, 1.0, (nprob, m)), rng.uniform(0.5, 1.5, (nprob, 2))
    nvar, n = t.shape[0], x0.shape[1]
    if shared:
        t = np.ascontiguousarray(np.broadcast_to(t[:, :1], t.shape))
    block = m if shared else nprob * m
    stride = block + (3 if shared else 7)
    padded = np.full(nvar * stride, np.nan)
    for v in range(nvar):
        padded[v * stride:v * stride + block] = (t[v, 0] if shared else t[v]).ravel()
    dy = _dev(ds, y)
    loose = _by_hand(ds, e, shared, m, _dev(ds, padded), dy, stride)
    tight = ds.expr_launchers(e, _dev(ds, t[:, 0] if shared else t), dy)
    plist = _shapes(nprob, n)[2]
    X = _points(x0, plist, 8)
    want = LC.restate(prog, X, t[:, plist], y[plist])
    for form, chunk in FORMS:
        with _variant(form):
            got = _both(ds, *loose, plist, X, m, (which, shared, m, form))
            _same_bits(_both(ds, *tight, plist, X, m, (which, shared, m, form, "tight")), got, (which, shared, m, form, "tight"))
        _same_bits(got, want, (which, shared, m, form))


# ------------------------------------------------------------------------------------------------ g. solves at n = 32
def _wide32(ds):
    e = LC.compile_formula(LC.SOLVE_NAME)
    prog, t, y, xt, x0 = LC.limit_problems(LC.SOLVE_NAME, LC.SOLVE_M, nprob=LC.SOLVE_NPROB, prog=e.program())
    return e, prog, t, y, x0


@pytest.mark.parametrize("analytic", [False, True])
def test_solves_at_n32_against_oracle(ds, oracle, analytic):
    """tests/test_gpu_expr.py::test_solves_against_oracle on sixteen Lorentzians, 32 parameters: the device's solve is the CPU
    oracle's with the restatement as callback, bit for bit in x, fvec, counts and flags; every status 0."""
    e, prog, t, y, x0 = _wide32(ds)
    m, n = LC.SOLVE_M, x0.shape[1]
    opt = dict(max_evals=LC.MAX_EVALS)
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    x = _dev(ds, x0)
    fvec, ibs, status = ds.lm_solve_batch_device(fcn, ctx, m, x, jac=jac if analytic else None, opts=ds.options(**opt))
    xg, fg = x.cpu().numpy(), fvec.cpu().numpy()
    assert np.isfinite(xg).all() and np.isfinite(fg).all()
    oo = oracle.default_options(**opt)
    for p in range(LC.SOLVE_NPROB):
        tv = t[:, p]
        f = lambda xx, ff: ff.__setitem__(slice(None), R.residual(prog, xx, tv, y[p]))
        j = (lambda xx, JJ: JJ.__setitem__((slice(None), slice(None)), R.jacobian(prog, xx, tv))) if analytic else None
        rc, xo, fo, ibo = oracle.lm_solve(f, m, n, x0[p], jac=j, opts=oo)
        what = (analytic, p)
        assert status[p] == rc, (what, status[p], rc)
        assert _same(ibs[p], ibo), (what, ibs[p], ibo)
        assert np.array_equal(_bits(xg[p]), _bits(xo)), (what, np.abs(xg[p] - xo).max())
        assert np.array_equal(_bits(fg[p]), _bits(fo)), what
    assert set(status) == {0}, sorted(set(status))


def test_fit_batch_at_n32_is_the_composition(ds):
    """nlh_expr_fit_batch with 32 parameters -- a 32 x 32 covariance per problem -- is the solve and the covariance call by
    hand, bit for bit (tests/test_gpu_expr.py::test_fit_batch_is_the_composition)."""
    e, prog, t, y, x0 = _wide32(ds)
    m, n = LC.SOLVE_M, x0.shape[1]
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=LC.MAX_EVALS)
    keep = dx0.clone()
    got = ds.expr_fit_batch(e, dt, dy, dx0, analytic=True, opts=o)
    assert _eq(dx0, keep)
    want = _fit_by_hand(ds, e, dt, dy, None, dx0, m, True, o)
    assert set(got[7]) == {0} and got[7] == want[7] and got[6] == want[6]
    assert tuple(got[3].shape) == (LC.SOLVE_NPROB, n, n) and bool((got[5] == n).all())
    for g, w_ in zip(got[:6], want[:6]):                            # x, fvec, sigma, cov, chi2, rank
        assert bool(torch.isfinite(g.double()).all()) and _eq(g, w_)
    assert bool((got[2] > 0).all())


# ------------------------------------------------------------------------------------------------ h. the zero-weight rule
@pytest.mark.parametrize("name,m", [("rational", 129), ("wide32", 86)])
def test_zero_weight_rows_are_zeros_of_the_products_sign(ds, name, m):
    """The weight multiplies (r = w*r, every Jacobian entry once by w): where the model value is finite a row of weight 0 is
    a zero with the sign of what it multiplied -- -0.0 under a negative residual or derivative --, as the restatement's."""
    nprob = 5
    e = _compile(name)
    prog, t, y, xt, x0 = _problems(name, m, nprob, 9, e.program())
    w = _weights(np.random.default_rng(2), nprob, m)
    w[:, 1::2] = 0.0
    dt, dy = _dev(ds, t), _dev(ds, y)
    plist = list(range(nprob))
    bare = _both(ds, *ds.expr_launchers(e, dt, dy), plist, x0, m, (name, "unweighted"))
    got = _both(ds, *ds.expr_launchers(e, dt, dy, _dev(ds, w)), plist, x0, m, (name, "weighted"))
    _same_bits(got, LC.restate(prog, x0, t, y, w), name)
    zero = w == 0.0
    zJ = np.broadcast_to(zero[:, None, :], got[1].shape)
    assert (got[0][zero] == 0.0).all() and (got[1][zJ] == 0.0).all()
    assert np.array_equal(np.signbit(got[0][zero]), np.signbit(bare[0][zero]))
    assert np.array_equal(np.signbit(got[1][zJ]), np.signbit(bare[1][zJ]))
    assert np.signbit(got[0][zero]).any() and not np.signbit(got[0][zero]).all()     # both signs occur
    assert np.signbit(got[1][zJ]).any() and not np.signbit(got[1][zJ]).all()
