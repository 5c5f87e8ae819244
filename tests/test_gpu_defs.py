"""GPU tests of definitions in formulas (include/nonlin_hip.h: name = expr; ..., NLH_EXPR_LOAD): the interpreter kernels on
programs with LOAD, bit for bit -- the residual and every Jacobian column -- against the numpy restatement of the expanded
program (tests/defs_restatement.py, tests/pwfun_restatement.py) where the formula has no library function: every small
program of tests/test_defs_cpu.py, a rotated 2-D model of two variables, the formula that passes 256 instructions once
substituted, and the frame of 16 in the largest launch; m at the forms' edges, both forms, 1 to 8 points and a list of 7,
one column a pass, the default and a pass count that leaves a shorter last pass, a pass skipped although a definition names
its column, with and without weights.  A formula with exp, cos, sin or erfcx is no restatement's bits: the rotated Gaussian,
the EMG and the pseudo-Voigt are held bit for bit to the device's own run of the substituted formula -- the statement the
header makes -- and to the restatement within its running bound.  Then expr_eval, expr_fit_batch (plain, and with a map and
a Huber loss) and expr_band of the rotated Gaussian with definitions against the same call on the substituted Expr, bit for
bit.  Every output is checked to be finite first: the launch helper prefills it with NaN."""
import numpy as np
import pytest
import torch

import defs_cases as DC
import defs_restatement as D
import nonlin_amd as nl
import pwfun_restatement as PW
from nonlin_amd.device import expr_plan
from test_gpu_expr import _bits, _dev, _eq, _launch, _points, _variant, _weights

pytestmark = pytest.mark.gpu

NPROB = 5


def _both(ds, fcn, jac, ctx, plist, X, m, what):
    F = _launch(ds, fcn, ctx, plist, X, m)
    J = _launch(ds, jac, ctx, plist, X, m, jac=True)
    assert np.isfinite(F).all() and np.isfinite(J).all(), what
    return F, J


def _same_bits(got, want, what):
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (what, "residual")
    assert np.array_equal(_bits(got[1]), _bits(want[1])), (what, "jacobian")


def _forms(m):
    """The form m selects, and each form forced where it can hold m (flat: m <= 256)."""
    return [None, "row"] + (["flat"] if m <= 256 else [])


def _short_tail_chunk(n, default):
    """A pass of 1 < C < n columns, fewer than the default, that leaves a shorter last pass; None where there is none."""
    for c in range(2, min(n, default)):
        if n % c:
            return str(c)
    return None


@pytest.fixture(scope="module")
def cases():
    """name -> (Expr, expanded program, t, y, x0, w, plist, X, restatement unweighted, restatement weighted), per m: computed
    once and shared."""
    store = {}

    def get(name, m):
        if (name, m) not in store:
            e = DC.compile_formula(name)
            prog, t, y, xt, x0 = DC.problems(name, m, nprob=NPROB, seed=31 + m)
            rng = np.random.default_rng(m)
            w = _weights(rng, NPROB, m)
            plist = [3, 0, 4, 4, 1, 2, 0, 3]                        # 8 points; its first 7 are the list of 7
            X = _points(x0, plist, 9)
            want = {False: DC.restate(prog, X, t[:, plist], y[plist]), True: DC.restate(prog, X, t[:, plist], y[plist], w[plist])}
            store[name, m] = (e, prog, t, y, x0, w, plist, X, want)
        return store[name, m]
    return get


# ------------------------------------------------------------------------------------------------ a. the exact class
@pytest.mark.parametrize("m", [1, 2, 86, 255, 257])
@pytest.mark.parametrize("name", [k for k in DC.EXACT if k != "frame16"])
def test_exact_programs_bitwise(ds, cases, name, m):
    """m = 1, 2; 86: two points per flat workgroup and a partly filled last one; 255 and 257: one and two row blocks."""
    e, prog, t, y, x0, w, plist, X, want = cases(name, m)
    n = x0.shape[1]
    assert (e.program()[0] == D.LOAD).any() == (name != "unused") and D.frame(e.program()[0]) == e.depth
    with _variant(None):
        plan = expr_plan(e.depth, n, m)
    assert plan["flat"] == (m <= 128)
    chunks = [None] + (["1"] if plan["chunk"] > 1 else []) + [c for c in [_short_tail_chunk(n, plan["chunk"])] if c]
    dt, dy = _dev(ds, t), _dev(ds, y)
    for weighted in (False, True):
        fcn, jac, ctx = ds.expr_launchers(e, dt, dy, _dev(ds, w) if weighted else None)
        for form in _forms(m):
            for chunk in chunks:
                for count in ((1, 7, 8) if chunk is None else (7,)):
                    what = (name, m, weighted, form, chunk, count)
                    with _variant(form, chunk):
                        got = _both(ds, fcn, jac, ctx, plist[:count], X[:count], m, what)
                    _same_bits(got, (want[weighted][0][:count], want[weighted][1][:count]), what)


def test_skipped_pass_with_a_definition_that_names_it(ds, cases):
    """z = b*t; a*t+1 over (a, b, c): the root names a alone, so with one column a pass the passes of b and c are skipped --
    although the definition names b -- and their columns are +0.0, the bit pattern; with every column in one pass the
    definition's tangent is carried and never read."""
    m = 86
    e, prog, t, y, x0, w, plist, X, want = cases("unused", m)
    masks = e.program()[3]
    assert int(masks[-1]) == 1 and int(masks[2]) == 2 and e.defs == ("z",)
    dt, dy = _dev(ds, t), _dev(ds, y)
    for weighted in (False, True):
        fcn, jac, ctx = ds.expr_launchers(e, dt, dy, _dev(ds, w) if weighted else None)
        for chunk in ("1", "2", None):
            with _variant(None, chunk):
                assert expr_plan(e.depth, 3, m)["chunk"] == (3 if chunk is None else int(chunk))
                F, J = _both(ds, fcn, jac, ctx, plist, X, m, (weighted, chunk))
            _same_bits((F, J), want[weighted], (weighted, chunk))
            wq = w[plist] if weighted else np.ones_like(F)
            assert np.array_equal(_bits(J[:, 1:]), _bits(wq[:, None, :] * np.zeros((len(plist), 2, m)))), (weighted, chunk)
            assert np.array_equal(_bits(J[:, 0]), _bits(wq * t[0, plist])), (weighted, chunk)


def test_frame16_in_the_largest_launch(ds):
    """Eight definitions under an expression eight deep, 32 parameters, m = 1: 256 points per workgroup stage 64 KB of x
    beside two 32 KB stacks -- 131,072 bytes, the most the Jacobian kernel ever asks for; the model value and its tangents
    come out of slot 8."""
    e = DC.compile_formula("frame16")
    n, m, npoints = 32, 1, 300
    assert (e.nparams, e.depth, len(e.defs)) == (n, 16, 8)
    with _variant(None):
        assert expr_plan(16, n, m, npoints) == {"flat": True, "ppw": 256, "nblk": 1, "grid": 2, "chunk": 1, "lds_bytes": 131072}
    prog, t, y, xt, x0 = DC.problems("frame16", m, nprob=7, seed=16)
    rng = np.random.default_rng(16)
    w = rng.uniform(0.5, 2.0, y.shape)
    plist = list(rng.integers(0, 7, npoints))
    X = _points(x0, plist, 6)
    for wh in (None, w):
        fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y), _dev(ds, wh) if wh is not None else None)
        want = DC.restate(prog, X, t[:, plist], y[plist], wh[plist] if wh is not None else None)
        with _variant(None):
            got = _both(ds, fcn, jac, ctx, plist, X, m, "frame16")
        _same_bits(got, want, "frame16")
        assert (_bits(got[1][:, 17:]) == 0).all() and (got[1][:, :17] != 0).all()      # p17 .. p31 are not named: +0.0


# ------------------------------------------------------------------------------------------------ b. with library functions
@pytest.mark.parametrize("m", [2, 86, 257])
@pytest.mark.parametrize("name", ["gauss_u", "rot2d", "emg", "pvoigt2"])
def test_models_equal_their_substituted_form_bitwise(ds, name, m):
    """The same operations on the same operands: the device's residual and Jacobian of the formula with definitions are those
    of the substituted formula, bit for bit, under every form and pass width; and the restatement's within its running
    bound."""
    e, s = DC.compile_formula(name), DC.compile_formula(name, substituted=True)
    assert e.defs and not s.defs
    prog, t, y, xt, x0 = DC.problems(name, m, nprob=NPROB, seed=7 + m)
    n = x0.shape[1]
    w = _weights(np.random.default_rng(m), NPROB, m)
    plist = [3, 0, 4, 4, 1, 2, 0]
    X = _points(x0, plist, 2)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), _dev(ds, w)
    with _variant(None):
        c_e, c_s = expr_plan(e.depth, n, m)["chunk"], expr_plan(s.depth, n, m)["chunk"]
    chunks = [None, "1"] + [c for c in [_short_tail_chunk(n, min(c_e, c_s))] if c]
    for wh in (None, dw):
        with_defs, plain = ds.expr_launchers(e, dt, dy, wh), ds.expr_launchers(s, dt, dy, wh)
        for form in _forms(m):
            for chunk in chunks:
                what = (name, m, wh is not None, form, chunk)
                with _variant(form, chunk):
                    got = _both(ds, *with_defs, plist, X, m, what)
                    want = _both(ds, *plain, plist, X, m, what)
                _same_bits(got, want, what)
    with _variant(None):
        F, J = _both(ds, *ds.expr_launchers(e, dt, dy), plist, X, m, name)
    worst = 0.0
    for q, p in enumerate(plist):
        r, eb = PW.residual_bound(prog, X[q], t[:, p], y[p])
        Jr, eJ = PW.jacobian_bound(prog, X[q], t[:, p])
        for got, ref, bound in ((F[q], r, eb), (J[q].T, Jr, eJ)):
            assert (bound > 0.0).any()
            worst = max(worst, float((np.abs(got - ref) / np.where(bound > 0.0, bound, np.inf)).max()))
            assert (np.abs(got - ref) <= bound).all(), (name, m, q)
    print(f"{name} m={m}: largest |device - numpy| / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ c. the callers of an Expr
@pytest.fixture(scope="module")
def rot2d():
    """16 problems of the rotated Gaussian on 64 pixels each; the Expr with definitions and the substituted one."""
    e, s = DC.compile_formula("rot2d"), DC.compile_formula("rot2d", substituted=True)
    prog, t, y, xt, x0 = DC.problems("rot2d", 64, nprob=16, seed=5, spread=0.02)
    return e, s, t, y, xt, x0


def _same_fit(got, want):
    assert got[7] == want[7] and got[6] == want[6]                     # status, iteration behaviour
    for g, w_ in zip(got[:6], want[:6]):                               # x, fvec, sigma, cov, chi2, rank
        assert bool(torch.isfinite(g.double()).all()) and _eq(g, w_)


def test_expr_eval_pair(ds, rot2d):
    e, s, t, y, xt, x0 = rot2d
    dt, dx = _dev(ds, t), _dev(ds, x0)
    got, want = ds.expr_eval(e, dx, dt), ds.expr_eval(s, dx, dt)
    assert bool(torch.isfinite(got).all()) and _eq(got, want)
    prog = DC.expanded(e)
    for p in (0, 15):
        r, eb = PW.residual_bound(prog, x0[p], t[:, p], np.zeros(64))
        assert (np.abs(got[p].cpu().numpy() - r) <= eb).all()


def test_expr_fit_batch_pair(ds, rot2d):
    e, s, t, y, xt, x0 = rot2d
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=500)
    got, want = ds.expr_fit_batch(e, dt, dy, dx0, opts=o), ds.expr_fit_batch(s, dt, dy, dx0, opts=o)
    _same_fit(got, want)
    assert not _eq(got[0], dx0)                                        # (the fit moved)


def test_expr_fit_batch_pmap_loss_pair(ds, rot2d):
    e, s, t, y, xt, x0 = rot2d
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    o = ds.options(max_evals=500)
    loss = nl.Loss("huber", 3e-3 * float(np.abs(y).max()))
    fits = [ds.expr_fit_batch(f, dt, dy, dx0, opts=o, pmap=nl.ParamMap.for_expr(f, fixed=("b",), tied={"sy": ("sx", 1.5, 0.0)}), loss=loss)
            for f in (e, s)]
    _same_fit(*fits)


def test_expr_band_pair(ds, rot2d):
    e, s, t, y, xt, x0 = rot2d
    dt, dy, dx0 = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
    x, fvec, sigma, cov, chi2, rank, ibs, st = ds.expr_fit_batch(e, dt, dy, dx0, opts=ds.options(max_evals=500))
    got, want = ds.expr_band(e, x, cov, dt), ds.expr_band(s, x, cov, dt)
    for g, w_ in zip(got, want):
        assert bool(torch.isfinite(g).all()) and _eq(g, w_)
    assert bool((got[1] > 0).all())
