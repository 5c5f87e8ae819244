"""GPU tests of what the six pairs of wrapping launchers share (parameter maps, robust losses, Poisson fits, global fits,
instrument responses, separable fits; nlh_launch.h): a context is a context of ONE kind -- the launchers and the unwrap of
every other kind leave it alone --, and layers stacked as model objects give the bits of the one-call fit and can be
destroyed outermost first, with and without grown scratch.  The Lorentzian family of tests/curve_cases.py with one component
on a constant: 3 problems of 40 rows, 4 parameters."""
import ctypes as C

import numpy as np
import pytest
import torch

import curve_cases as CC
import curve_restatement as R
import nonlin_amd as nl
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

NL_INVALID_INPUT_ERROR = 201
KINDS = ("pmap", "loss", "pois", "group", "conv", "sep")
KIND, K, B, NPROB, M, N = "lorentz", 1, 0, 3, 40, 4
TAPS, ORIGIN, EXTEND = (0.25, 0.5, 0.25), 1, "hold"
SENTINEL = -7.25


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    """Bit for bit, the sign of zero included; NaN against NaN."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb])


def _dev(ds, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ds.device)


def _problems():
    """t, y [3, 40], x_true, x0 [3, 4] with width = 0.2 amplitude + 0.05 at the truth: the tie of test 3 holds there."""
    t, _, xt, _ = CC.curve_problems(KIND, K, B, M, nprob=NPROB, seed=77)
    rng = np.random.default_rng(78)
    xt[:, 2] = 0.2 * xt[:, 0] + 0.05
    y = np.stack([R.model(R.KINDS[KIND], K, B, xt[p], t[p]) + 1e-3 * rng.uniform(-1, 1, M) for p in range(NPROB)])
    x0 = xt * (1.0 + 0.05 * rng.uniform(-1, 1, xt.shape))
    return t, np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


class _Layers:
    """One context of every kind around the curve's launchers, and for each kind the shape (points, n, m) its launchers take."""

    def __init__(self, ds):
        self.ds = ds
        t, y, xt, x0 = _problems()
        self.dt, self.dy, self.dfull = _dev(ds, t), _dev(ds, y), _dev(ds, x0)
        fcn, jac, ctx = ds.curve_launchers(KIND, K, B, self.dt, self.dy)
        self.inner = ctx
        pm, grp, sep = nl.ParamMap(N, fixed=(3,), tied={2: (0, 0.2, 0.05)}), nl.Group(N, shared=(2,), nsets=NPROB), nl.Separable(N, linear=(0, 3))
        self.ctx = {"pmap": ds.pmap_launchers(pm, fcn, jac, ctx, self.dfull)[2],
                    "loss": ds.loss_launchers(nl.Loss("huber", 0.01), fcn, jac, ctx)[2],
                    "pois": ds.pois_launchers(nl.Poisson(), fcn, jac, ctx, self.dy)[2],
                    "group": ds.group_launchers(grp, fcn, jac, ctx)[2],
                    "conv": ds.conv_launchers(nl.Convolve(TAPS, origin=ORIGIN, extend=EXTEND), fcn, jac, ctx, self.dy)[2],
                    "sep": ds.sep_launchers(sep, fcn, jac, ctx)[2]}
        self.shape = {"pmap": (NPROB, pm.nfree, M), "loss": (NPROB, N, M), "pois": (NPROB, N, M), "group": (1, grp.nouter, NPROB * M),
                      "conv": (NPROB, N, M), "sep": (NPROB, sep.nnonlin, M)}
        self.X = {"pmap": ds.pmap_gather(pm, self.dfull), "loss": self.dfull, "pois": self.dfull, "group": ds.group_gather(grp, self.dfull),
                  "conv": self.dfull, "sep": ds.sep_gather(sep, self.dfull)}

    def call(self, kind, which, ctx):
        """nlh_<kind>_device_<which> on `ctx` with the shapes of `kind`: (rc, the output buffer, which held SENTINEL)."""
        ds = self.ds
        npts, n, m = self.shape[kind]
        X = self.X[kind]
        assert tuple(X.shape) == (npts, n)
        out = torch.full((npts, n, m) if which == "jac" else (npts, m), SENTINEL, dtype=torch.float64, device=ds.device)
        stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
        rc = getattr(ds.lib, f"nlh_{kind}_device_{which}")(ctx.ptr, stream, npts, None, n, X.data_ptr(), m, out.data_ptr())
        torch.cuda.synchronize()
        return rc, out.cpu().numpy()

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def layers(ds):
    ly = _Layers(ds)
    yield ly
    ly.close()


# ------------------------------------------------------------------------------ 1. a context of another kind is refused
@pytest.mark.parametrize("b", KINDS)
@pytest.mark.parametrize("a", KINDS)
def test_context_of_another_kind_is_refused(layers, a, b):
    """nlh_<a>_device_fcn / _jac on a context nlh_<b>_wrap made: NLH_INVALID_INPUT_ERROR, and nothing is written."""
    if a == b:
        for which in ("fcn", "jac"):                                   # (the shapes of this file's calls are ones the kind accepts)
            rc, out = layers.call(a, which, layers.ctx[a])
            assert rc == 0 and not np.any(out == SENTINEL), (a, which, rc)
        return
    for which in ("fcn", "jac"):
        rc, out = layers.call(a, which, layers.ctx[b])
        assert rc == NL_INVALID_INPUT_ERROR, (a, b, which, rc)
        assert np.all(out == SENTINEL), (a, b, which)


# ------------------------------------------------------------------------------ 2. the unwrap of another kind does nothing
@pytest.mark.parametrize("b", KINDS)
def test_unwrap_of_another_kind_does_nothing(ds, b):
    """nlh_<a>_unwrap of a context of kind b != a, and of NULL: the context's launchers give the same bits afterwards; then
    nlh_<b>_unwrap releases it."""
    ly = _Layers(ds)
    try:
        before = [ly.call(b, which, ly.ctx[b]) for which in ("fcn", "jac")]
        assert [rc for rc, _ in before] == [0, 0]
        for a in KINDS:
            unwrap = getattr(ds.lib, f"nlh_{a}_unwrap")
            unwrap(None)
            if a != b:
                unwrap(ly.ctx[b].ptr)
        after = [ly.call(b, which, ly.ctx[b]) for which in ("fcn", "jac")]
        for (rc0, o0), (rc1, o1) in zip(before, after):
            assert rc1 == rc0 == 0 and _same(o0, o1)
        ly.ctx[b].close()                                               # nlh_<b>_unwrap
        assert not ly.ctx[b].ptr.value
    finally:
        ly.close()


# ------------------------------------------------------------------------------ 3. layers stacked as model objects
def test_stacked_model_objects_are_the_one_call_fit(ds):
    """pmap_model(loss_model(conv_model(curve_model))) through nlh_dq_model_lm_solve from the gathered free parameters = the
    _conv one-call fit with the same map, loss and response: fvec, status and the free entries of x, bit for bit.  A stack
    is destroyed outermost first, untouched and after two solves (grown scratch)."""
    t, y, xt, x0 = _problems()
    scale = np.array([0.004, 0.01, 0.02])
    k = np.array(TAPS)
    pm = nl.ParamMap(N, fixed=(3,), tied={2: (0, 0.2, 0.05)})
    o = ds.options()
    x, fvec, _, _, _, _, ibs, status = ds.curve_fit_batch(KIND, _dev(ds, t), _dev(ds, y), _dev(ds, x0), ncomp=K, baseline=B, pmap=pm,
                                                         loss=nl.Loss("huber", scale), conv=nl.Convolve(k, origin=ORIGIN, extend=EXTEND),
                                                         covariance=False, opts=o)
    torch.cuda.synchronize()
    x, fvec = x.cpu().numpy(), fvec.cpu().numpy()
    print("one-call fit: status", status, "iterations", [ib["iter_count"] for ib in ibs])
    f2f = np.zeros(pm.nfree, dtype=np.int32)
    assert ds.lib.nlh_pmap_tables(pm.ptr, None, None, None, None, f2f.ctypes.data_as(_lib.c_int32_p)) == 0
    assert list(f2f) == [0, 1]
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)

    def stack():
        md = [C.c_void_p() for _ in range(4)]
        cv = _lib.ConvStruct(len(k), ORIGIN, nl.CONV_HOLD, 1, k.ctypes.data)
        assert ds.lib.nlh_curve_model_create(ds.h.ptr, R.KINDS[KIND], K, B, NPROB, M, ptr(t), 0, ptr(y), None, 1, C.byref(md[0])) == 0
        assert ds.lib.nlh_conv_model_create(ds.h.ptr, md[0], C.byref(cv), ptr(y), None, C.byref(md[1])) == 0
        assert ds.lib.nlh_loss_model_create(ds.h.ptr, md[1], nl.LOSS_HUBER, ptr(scale), 0, C.byref(md[2])) == 0
        assert ds.lib.nlh_pmap_model_create(ds.h.ptr, md[2], pm.ptr, ptr(x0), 0, C.byref(md[3])) == 0
        return md

    def destroy(md):
        for m_ in reversed(md):                                        # outermost first
            ds.lib.nlh_dq_model_destroy(m_)

    destroy(stack())                                                   # a stack no call went through
    md = stack()
    try:
        sp, sm, sn = C.c_int32(), C.c_int32(), C.c_int32()
        ds.lib.nlh_dq_model_shape(md[3], C.byref(sp), C.byref(sm), C.byref(sn))
        assert (sp.value, sm.value, sn.value) == (NPROB, M, pm.nfree)
        for _ in range(2):
            xh, fh = np.ascontiguousarray(x0[:, f2f]), np.zeros((NPROB, M))
            ib, st = (_lib.IterationBehavior * NPROB)(), (C.c_int32 * NPROB)()
            assert ds.lib.nlh_dq_model_lm_solve(ds.h.ptr, C.byref(o), md[3], ptr(xh), ptr(fh), ib, st) == 0
            print("stacked models: status", list(st), "iterations", [ib[p].iter_count for p in range(NPROB)])
            assert list(st) == status
            assert _same(fh, fvec)
            assert _same(xh, x[:, f2f])
    finally:
        destroy(md)
    torch.cuda.synchronize()
