"""Device-model ("mode D") front end: batches of independent dense-quadratic problems
resident in HBM, solved by the batched entry points of include/nonlin_hip.h.

torch is plumbing only (device memory, streams); every computation is a call into
libnonlin_hip.so.  Layout: A [nprob, n, m] (each problem column-major m-by-n, i.e.
A[p, j, i] = A_p(i, j)), b/fvec [nprob, m], x [nprob, n], all float64 on the GPU.
"""
import collections
import contextlib
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import (CURVE_GAUSS, CURVE_LORENTZ, CURVE_EXPDECAY, CURVE_KINDS, curve_kind, curve_nparams,  # noqa: F401
                   Expr, ParamMap, Loss, Poisson, Convolve)

# nlh_iteration_behavior as a numpy structured dtype (the batch forms of the one-variable solvers return arrays of it)
IB_DTYPE = np.dtype([(k, np.int32) for k, _ in _lib.IterationBehavior._fields_])


def _chk(t, shape, name):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: expected contiguous float64 GPU tensor of shape {tuple(shape)}, "
                         f"got {t.dtype} {tuple(t.shape)} cuda={t.is_cuda}")


def _ib_status(nprob):
    """(ib, status): the arrays a batched solver fills with its iteration records and status codes."""
    return (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()


def _ib_lists(ib, status):
    """Those arrays as the solvers return them: (a list of dicts, a list of ints)."""
    return [ib[k].as_dict() for k in range(len(ib))], [int(status[k]) for k in range(len(status))]


def _host_bounds(lower, upper, n=None, refusal=None):
    """(plo, phi): the box of a bounded solve as pointers to host arrays of doubles (None: no bound; a pointer keeps its
    array).  n: the entries each must have -- not checked when None --, refusal: the text of the ValueError otherwise."""
    lo, hi = (None if b is None else np.ascontiguousarray(b, dtype=np.float64) for b in (lower, upper))
    if n is not None and any(b is not None and b.shape != (n,) for b in (lo, hi)):
        raise ValueError(refusal or f"bounds: expected {n} entries")
    return tuple(None if b is None else b.ctypes.data_as(_lib.c_double_p) for b in (lo, hi))


# What the one-call fits and bootstraps pass around.  _Model binds a model -- a built-in curve or an Expr -- once: name
# ("curve" / "expr"), head (the model's own arguments of _lib.fit_args by name), n parameters, nvar variables, and closures on
# the public methods: data(t, y, weights) -> (nprob, m, shared_t) checked, launchers(t, y, weights), eval(x, t) and
# guess(t, y, weights) (None: a formula has no guess).  _Keywords holds the keywords every path hands on; kw._replace(...)
# copies it with some fields replaced.
_Model = collections.namedtuple("_Model", "name head n nvar data launchers eval guess")
_Keywords = collections.namedtuple("_Keywords", "lower upper analytic covariance opts pmap loss stat group conv sep")


def _refuse_sep(kw, n):
    """What a separable fit refuses, worded once."""
    if kw.sep is None:
        return
    if kw.pmap is not None or kw.loss is not None or kw.stat is not None:
        raise ValueError("sep excludes pmap, loss and stat: a map, a loss and a statistic are nonlinear in the projected parameters")
    if kw.sep.nparams != n:
        raise ValueError(f"sep is over {kw.sep.nparams} parameters, the model has {n}")


# names of the NLH_QRX_SWEEP_* / INIT_* / PIVOT_* / PASS_* values of include/nonlin_hip.h, in order
QRX_SWEEPS = ("column", "lane")
QRX_INITS = ("split", "fused")
QRX_PIVOT_FORMS = ("few32", "batch32", "few64", "batch64", "long", "long_scaled", "long_split")
QRX_PASS_FORMS = ("column", "wide", "wide_half", "four_wave", "wave", "wave_shared")


def qrx_plan(nprob, m, n, nact=0, have_stages=False):
    """The launch plan of the exact lmfactor (nlh_qrx_plan: host code, needs no GPU) for nprob m-by-n problems of which
    nact need factoring (0: all), under this process's NLH_QRX_* environment.  Returns (head, steps): dicts of the
    fields of nlh_qrx_plan_head / nlh_qrx_plan_step, one per Householder step, with the forms by name."""
    head = _lib.QrxPlanHead()
    steps = (_lib.QrxPlanStep * max(n, 1))()
    rc = _lib.load().nlh_qrx_plan(nprob, m, n, nact, int(bool(have_stages)), C.byref(head), steps, n)
    if rc != n:
        raise ValueError(f"nlh_qrx_plan({nprob}, {m}, {n}, {nact}): error {rc}")
    names = {"sweep": QRX_SWEEPS, "init": QRX_INITS, "pivot": QRX_PIVOT_FORMS, "pass": QRX_PASS_FORMS}

    def rec(r):
        return {k: names[k][getattr(r, k)] if k in names else int(getattr(r, k)) for k, _ in r._fields_}
    return rec(head), [rec(steps[i]) for i in range(n)]


# names of the NLH_GRAM_FORM_* values of include/nonlin_hip.h, in order
GRAM_FORMS = ("block", "tri8", "tri16", "512")


def gram_plan(m, n):
    """The kernel form and K-split count of G = J^T J for an m-by-n problem (nlh_gram_plan: host code, needs no GPU; the
    function the launch itself dispatches through), under this process's NLH_GRAM512 / NLH_GRAM_TRI environment as it is
    now.  Returns {"form": one of GRAM_FORMS, "nsplit": K-splits, "direct": no reduce launch}."""
    ns, direct = C.c_int32(), C.c_int32()
    rc = _lib.load().nlh_gram_plan(m, n, C.byref(ns), C.byref(direct))
    if rc < 0:
        raise ValueError(f"nlh_gram_plan({m}, {n}): error {rc}")
    return {"form": GRAM_FORMS[rc], "nsplit": int(ns.value), "direct": bool(direct.value)}


# names of the NLH_HOUSE_FORM_* values of include/nonlin_hip.h, in order
HOUSE_FORMS = ("fused4", "fused16", "dot2", "dot_lds", "dot_global")


def house_plan(nprob, rows, ncA, ncE):
    """The kernel form of the Householder steps (DeviceSolver.house_steps, and every QR built on them) for nprob work
    arrays [A | E] of rows x ncA | rows x ncE (nlh_house_plan: host code, needs no GPU; the function the launch itself
    dispatches through).  Returns {"form": one of HOUSE_FORMS, "tiles": product tiles the form keeps in LDS}."""
    tiles = C.c_int32()
    rc = _lib.load().nlh_house_plan(nprob, rows, ncA, ncE, C.byref(tiles))
    if rc < 0:
        raise ValueError(f"nlh_house_plan({nprob}, {rows}, {ncA}, {ncE}): error {rc}")
    return {"form": HOUSE_FORMS[rc], "tiles": int(tiles.value)}


def expr_plan(depth, n, m, npoints=1, jac=True):
    """The launch shape of the formula kernels for a program of stack depth `depth` with n parameters on m rows, npoints
    points in the call (nlh_expr_plan: host code, needs no GPU; the function the launchers themselves dispatch through), under
    this process's NLH_EXPR_FORM / NLH_EXPR_CHUNK environment as it is now.  jac: the Jacobian kernel (False: the residual
    kernel, chunk 0).  Returns {"flat", "ppw", "nblk", "grid", "chunk", "lds_bytes"}."""
    flat, ppw, nblk, chunk = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    grid, lds = C.c_int64(), C.c_int64()
    rc = _lib.load().nlh_expr_plan(depth, n, m, npoints, int(bool(jac)), C.byref(flat), C.byref(ppw), C.byref(nblk), C.byref(grid),
                                   C.byref(chunk), C.byref(lds))
    if rc:
        raise ValueError(f"nlh_expr_plan({depth}, {n}, {m}, {npoints}): error {rc}")
    return {"flat": bool(flat.value), "ppw": int(ppw.value), "nblk": int(nblk.value), "grid": int(grid.value),
            "chunk": int(chunk.value), "lds_bytes": int(lds.value)}


class _Wrapped(_lib.Owner):
    """The context of a pair of wrapping launchers (nlh_pmap_ctx, nlh_loss_ctx, ...: what an nlh_*_wrap made), with everything
    it points at kept alive; free: the name of the nlh_*_unwrap that takes it back."""

    def __init__(self, lib, ptr, keep, free):
        self.lib, self.ptr, self._keep, self._free = lib, ptr, keep, free


class DeviceSolver:
    """Owns an nlh handle bound to torch's current stream on `device`."""

    def __init__(self, device=0):
        if not torch.cuda.is_available():
            raise _lib.NonlinHipUnavailable("no GPU visible: nonlin_amd has no CPU fallback")
        self.device = torch.device("cuda", device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
        self.h = _lib.Handle(device, stream)
        self.lib = self.h.lib

    def check(self, rc, what):
        return self.h.check(rc, what)

    def _checked(self, rc, what):
        """A return code that must be 0: Handle.check's error, with the library's message, for a negative one."""
        self.h.check(rc, what)
        if rc:
            raise RuntimeError(f"{what} returned {rc}")

    def _call(self, name, *args):
        """The library's entry point `name` on this solver's handle, checked."""
        self._checked(getattr(self.lib, name)(self.h.ptr, *args), name)

    def model(self, A, b, gamma):
        """A device residual model behind host arrays on this solver's device (HostModel)."""
        return HostModel(self, A, b, gamma)

    # -- inputs -------------------------------------------------------------
    def generate(self, nprob, m, n, seed0=12345, gamma=0.5, sigma=1e-3, spread=0.3, square_shift=False,
                 seed_stride=1):
        """SURVEY.md 8(d) generator, on the device; problem p uses seed0 + p*seed_stride.
        Returns (A, b, x_true, x0)."""
        dev = self.device
        A = torch.empty((nprob, n, m), dtype=torch.float64, device=dev)
        b = torch.empty((nprob, m), dtype=torch.float64, device=dev)
        xt = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        x0 = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        rc = self.lib.nlh_dq_generate(self.h.ptr, nprob, m, n, seed0, seed_stride, gamma, sigma, spread, int(square_shift),
                                      A.data_ptr(), b.data_ptr(), xt.data_ptr(), x0.data_ptr())
        self.h.check(rc, "nlh_dq_generate")
        return A, b, xt, x0

    # -- solvers ------------------------------------------------------------
    def options(self, **kw):
        o = _lib.default_options()
        for k, v in kw.items():
            if k == "factor":      # lss_set_factor clamp, src/nonlin_least_squares.f90:108-114
                v = min(max(float(v), 0.1), 100.0)
            if not hasattr(o, k):
                raise AttributeError(k)
            setattr(o, k, v)
        return o

    def lm_solve_batch(self, A, b, gamma, x, opts=None):
        """least_squares_solver%solve for every problem.  x is updated in place.
        Returns (fvec, ib_list, status_list)."""
        nprob, n, m = A.shape
        _chk(A, (nprob, n, m), "A"); _chk(b, (nprob, m), "b"); _chk(x, (nprob, n), "x")
        fvec = torch.empty((nprob, m), dtype=torch.float64, device=A.device)
        ib, status = _ib_status(nprob)
        o = opts or self.options()
        self._call("nlh_dq_lm_solve_batch", C.byref(o), nprob, m, n, A.data_ptr(), b.data_ptr(),
                   float(gamma), x.data_ptr(), fvec.data_ptr(), ib, status)
        return (fvec,) + _ib_lists(ib, status)

    def newton_solve_batch(self, A, b, gamma, x, analytic=True, opts=None):
        """newton_solver%solve for every (square) problem.  x is updated in place."""
        nprob, n, m = A.shape
        assert m == n
        _chk(A, (nprob, n, n), "A"); _chk(b, (nprob, n), "b"); _chk(x, (nprob, n), "x")
        fvec = torch.empty((nprob, n), dtype=torch.float64, device=A.device)
        ib, status = _ib_status(nprob)
        o = opts or self.options()
        self._call("nlh_dq_newton_solve_batch", C.byref(o), nprob, n, A.data_ptr(), b.data_ptr(),
                   float(gamma), int(analytic), x.data_ptr(), fvec.data_ptr(), ib, status)
        return (fvec,) + _ib_lists(ib, status)

    def quasi_newton_solve_batch(self, A, b, gamma, x, analytic=True, opts=None, jdelta=5):
        """quasi_newton_solver%solve for every (square) problem.  x is updated in place."""
        nprob, n, m = A.shape
        assert m == n
        _chk(A, (nprob, n, n), "A"); _chk(b, (nprob, n), "b"); _chk(x, (nprob, n), "x")
        fvec = torch.empty((nprob, n), dtype=torch.float64, device=A.device)
        ib, status = _ib_status(nprob)
        o = opts or self.options()
        self._call("nlh_dq_quasi_newton_solve_batch", C.byref(o), int(jdelta), nprob, n, A.data_ptr(),
                   b.data_ptr(), float(gamma), int(analytic), x.data_ptr(), fvec.data_ptr(), ib, status)
        return (fvec,) + _ib_lists(ib, status)

    def cls_solve_batch(self, A, b, gamma, x, opts=None, lower=None, upper=None, delta=1.0, stepscale=1.0):
        """constrained_least_squares_solver%solve for every problem (the same bounds for all).  x in place."""
        nprob, n, m = A.shape
        _chk(A, (nprob, n, m), "A"); _chk(b, (nprob, m), "b"); _chk(x, (nprob, n), "x")
        fvec = torch.empty((nprob, m), dtype=torch.float64, device=A.device)
        ib, status = _ib_status(nprob)
        o = opts or self.options()
        plo, phi = _host_bounds(lower, upper)
        self._call("nlh_dq_cls_solve_batch", C.byref(o), float(delta), float(stepscale), plo, phi, nprob, m, n,
                   A.data_ptr(), b.data_ptr(), float(gamma), x.data_ptr(), fvec.data_ptr(), ib, status)
        return (fvec,) + _ib_lists(ib, status)

    def bfgs_solve_batch(self, A, b, gamma, x, opts=None):
        """bfgs%solve on f(x) = 0.5 ||r(x)||^2 of every problem (FD gradient on the device).  x in place.
        Returns (fout list, ib list, status list)."""
        nprob, n, m = A.shape
        _chk(A, (nprob, n, m), "A"); _chk(b, (nprob, m), "b"); _chk(x, (nprob, n), "x")
        ib, status = _ib_status(nprob)
        fout = (C.c_double * nprob)()
        o = opts or self.options(max_evals=500)
        self._call("nlh_dq_bfgs_solve_batch", C.byref(o), nprob, m, n, A.data_ptr(), b.data_ptr(), float(gamma),
                   x.data_ptr(), fout, ib, status)
        return ([float(v) for v in fout],) + _ib_lists(ib, status)

    # -- user-supplied device residuals (launchers) ------------------------------
    @staticmethod
    def _devfcn(f):
        """A launcher as ctypes sees it: a symbol of a user's shared object, an address, or None."""
        if f is None:
            return C.cast(None, _lib.DEVFCN)
        return f if isinstance(f, _lib.DEVFCN) else C.cast(f, _lib.DEVFCN)

    def dq_launchers(self, A, b, gamma):
        """The built-in dense-quadratic family expressed through the open path: (fcn, jac, ctx) for the *_device entry
        points.  Keep the returned ctx (and A, b) alive while solving."""
        ctx = _lib.DqDeviceCtx(A.data_ptr(), b.data_ptr(), float(gamma))
        return (C.cast(self.lib.nlh_dq_device_fcn, _lib.DEVFCN), C.cast(self.lib.nlh_dq_device_jac, _lib.DEVFCN), ctx)

    # -- built-in curve models ---------------------------------------------------
    def _curve_data(self, t, y, weights):
        """(nprob, m, shared_t) of the data tensors of a curve model, checked."""
        nprob, m = y.shape
        _chk(y, (nprob, m), "y")
        shared = t.dim() == 1
        _chk(t, (m,) if shared else (nprob, m), "t")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        return nprob, m, int(shared)

    def _curve_model(self, kind, ncomp, baseline):
        """The _Model of a built-in curve."""
        k = curve_kind(kind)
        return _Model("curve", dict(kind=k, ncomp=int(ncomp), nbase=int(baseline)), curve_nparams(k, ncomp, baseline), 1,
                      self._curve_data,
                      lambda t, y, weights: self.curve_launchers(k, ncomp, baseline, t, y, weights),
                      lambda x, t: self.curve_eval(k, x, t, ncomp, baseline),
                      lambda t, y, weights: self.curve_guess(k, t, y, ncomp, baseline, weights))

    def curve_launchers(self, kind, ncomp, baseline, t, y, weights=None):
        """A built-in curve model (kind: "gauss", "lorentz", "expdecay" or a CURVE_* constant; ncomp components; baseline:
        degree of the polynomial baseline, -1 for none) on the data t, y [nprob, m] (t may be one shared [m] tensor) with
        optional weights [nprob, m], as (fcn, jac, ctx) for lm_solve_batch_device, cls_solve_batch_device,
        lm_covariance_batch_device and fd_jacobian_device.  Keep ctx alive while solving (it keeps the tensors)."""
        nprob, m, shared = self._curve_data(t, y, weights)
        k = curve_kind(kind)
        curve_nparams(k, ncomp, baseline)
        ctx = _lib.CurveCtx(k, int(ncomp), int(baseline), shared, m, t.data_ptr(), y.data_ptr(),
                            weights.data_ptr() if weights is not None else None)
        ctx._tensors = (t, y, weights)                                # the context holds addresses: the tensors live as long as it does
        return (C.cast(self.lib.nlh_curve_device_fcn, _lib.DEVFCN), C.cast(self.lib.nlh_curve_device_jac, _lib.DEVFCN), ctx)

    def curve_eval(self, kind, x, t, ncomp=1, baseline=-1):
        """Model values (no data term, no weights) of x [nprob, n] at the abscissae t [nprob, npts] (or one shared [npts]
        tensor): y [nprob, npts]."""
        k = curve_kind(kind)
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        if n != curve_nparams(k, ncomp, baseline):
            raise ValueError(f"x has {n} columns, the model {curve_nparams(k, ncomp, baseline)} parameters")
        shared = t.dim() == 1
        npts = t.shape[-1]
        _chk(t, (npts,) if shared else (nprob, npts), "t")
        y = torch.empty((nprob, npts), dtype=torch.float64, device=x.device)
        self._call("nlh_curve_eval_batch", k, int(ncomp), int(baseline), nprob, npts, t.data_ptr(), int(shared),
                   x.data_ptr(), y.data_ptr())
        return y

    def curve_guess(self, kind, t, y, ncomp=1, baseline=-1, weights=None, smooth=2):
        """Starting values for curve_fit_batch from the data alone (nlh_curve_guess_batch): (x0 [nprob, n], flag [nprob],
        int32).  The positions and widths of the ncomp highest peaks of the detrended data, smoothed with a moving mean over
        2 smooth + 1 rows -- or the rates of one or two decays from the integral-equation regression --, then the best
        linear fit of the amplitudes and the baseline at those values, weights honoured.  Rows with weight 0 are left out.
        flag is a sum of nonlin_amd.GUESS_FALLBACK (a width or rate is the documented fallback), GUESS_RANKDEF (a dead column in
        the linear fit: that amplitude is 0) and GUESS_NONE (not guessed, the row of x0 is NaN: fewer valid rows than
        parameters, a value that is not finite, abscissae that do not ascend).  Deterministic: the same data give the same
        bits.  At most 8192 rows; peaks are positive; ncomp <= 2 for "expdecay"."""
        k = curve_kind(kind)
        nprob, m, shared = self._curve_data(t, y, weights)
        n = curve_nparams(k, ncomp, baseline)
        x0 = torch.empty((nprob, n), dtype=torch.float64, device=y.device)
        flag = torch.empty((nprob,), dtype=torch.int32, device=y.device)
        self._call("nlh_curve_guess_batch", k, int(ncomp), int(baseline), nprob, m, t.data_ptr(), shared, y.data_ptr(),
                   weights.data_ptr() if weights is not None else None, int(smooth), x0.data_ptr(), flag.data_ptr())
        return x0, flag

    # -- starts: starting values for any launcher from a box ------------------------------
    def starts_search(self, fcn, ctx, nprob, m, starts, positions=None):
        """The box scan of a Starts for ANY residual launcher (fcn, ctx) -- a user's, curve_launchers', expr_launchers', or one
        composed with pmap_launchers, group_launchers and the others -- over nprob problems of m rows
        (nlh_starts_search_batch_device): the cost sum F^2 at starts.ncand candidates of the box for every problem, and per
        problem the starts.keep candidates of smallest finite cost.  positions: the entries of the box that are the launcher's
        unknowns, in the launcher's order (None: all of them) -- what a reduced launcher needs: Separable.tables()[1] for
        sep_launchers, the free parameters for pmap_launchers.  Returns (x0 [nprob, keep, n], cost [nprob, keep],
        index [nprob, keep] int32), ordered by (cost, index); a slot with no finite cost left has cost +Inf, index -1 and a
        row of NaN.  Deterministic, and a problem's result does not depend on its batch."""
        lo, hi, lg = starts.box(positions)
        n, keep = len(lo), starts.keep
        dev = self.device
        x0 = torch.empty((nprob, keep, n), dtype=torch.float64, device=dev)
        cost = torch.empty((nprob, keep), dtype=torch.float64, device=dev)
        index = torch.empty((nprob, keep), dtype=torch.int32, device=dev)
        self._call("nlh_starts_search_batch_device", int(nprob), int(m), n, self._devfcn(fcn), self._ctxp(ctx),
                   lo.ctypes.data_as(_lib.c_double_p), hi.ctypes.data_as(_lib.c_double_p), lg.ctypes.data_as(_lib.c_int32_p),
                   starts.ncand, keep, x0.data_ptr(), cost.data_ptr(), index.data_ptr())
        return x0, cost, index

    def starts_cost(self, F):
        """cost [npoints] = sum F^2 of every row of F [npoints, m] in the scan's stated order (nlh_starts_cost_batch)."""
        npoints, m = F.shape
        _chk(F, (npoints, m), "F")
        cost = torch.empty((npoints,), dtype=torch.float64, device=F.device)
        self._call("nlh_starts_cost_batch", npoints, m, F.data_ptr(), cost.data_ptr())
        return cost

    def starts_pick(self, cost):
        """which [nprob] (int32) = the k of the smallest finite cost[k, p] of cost [keep, nprob], the lowest k on a tie, -1 when
        none is finite (nlh_starts_pick_batch)."""
        keep, nprob = cost.shape
        _chk(cost, (keep, nprob), "cost")
        which = torch.empty((nprob,), dtype=torch.int32, device=cost.device)
        self._call("nlh_starts_pick_batch", nprob, keep, cost.data_ptr(), which.data_ptr())
        return which

    def starts_take(self, src, which):
        """dst [nprob, ...] = src[which[p], p] of src [keep, nprob, ...] (float64), NaN where which[p] is -1
        (nlh_starts_take_batch)."""
        keep, nprob = src.shape[:2]
        _chk(src, src.shape, "src")
        if not (which.is_cuda and which.dtype == torch.int32 and which.is_contiguous() and tuple(which.shape) == (nprob,)):
            raise ValueError(f"which: expected a contiguous int32 GPU tensor of shape ({nprob},)")
        dst = torch.empty(src.shape[1:], dtype=torch.float64, device=src.device)
        width = dst.numel() // nprob if nprob else 1
        self._call("nlh_starts_take_batch", nprob, keep, width, src.data_ptr(), which.data_ptr(), dst.data_ptr())
        return dst

    def _starts_fit(self, model, t, shared, y, weights, starts, kw):
        """A one-call fit with starts=: starts_search on the launcher stack of the fit, the one-call fit from every kept start,
        and the fit of smallest cost per problem (starts_cost on fvec, starts_pick, starts_take)."""
        if kw.pmap is not None or kw.group is not None:
            raise ValueError("starts excludes pmap and group: compose pmap_launchers / group_launchers and call starts_search")
        n = model.n
        if starts.n != n:
            raise ValueError(f"starts: a box over {starts.n} parameters, the model has {n}")
        _refuse_sep(kw, n)
        nprob, m = y.shape
        with self._stack(model, t, y, weights, kw) as (fcn, _, ctx, positions):
            x0s, cost, index = self.starts_search(fcn, ctx, nprob, m, starts, positions)
            runs = []
            for k in range(starts.keep):
                if positions is None:
                    x0 = x0s[:, k].contiguous()
                else:                                                # the linear positions of a separable fit's x0 are 0.0
                    x0 = torch.zeros((nprob, n), dtype=torch.float64, device=y.device)
                    x0[:, positions] = x0s[:, k]
                runs.append(self._fit(model, t, shared, y, weights, x0, kw))
            which = self.starts_pick(torch.stack([self.starts_cost(r[1]) for r in runs]))
            take = lambda j: self.starts_take(torch.stack([r[j] for r in runs]), which)
            x, fvec = take(0), take(1)
            sigma = cov = chi2 = rank = None
            if kw.covariance:
                sigma, cov, chi2 = take(2), take(3), take(4)
                # (rank is int32: as float64, exactly, through the same take; NaN -- no fit was picked -- is -1)
                rank = torch.nan_to_num(self.starts_take(torch.stack([r[5] for r in runs]).to(torch.float64), which), nan=-1.0).to(torch.int32)
            wh = which.cpu().tolist()                                # ibs and status: the chosen fit's; of fit 0 where none was picked
            ibs = [runs[max(k, 0)][6][p] for p, k in enumerate(wh)]
            status = [runs[max(k, 0)][7][p] for p, k in enumerate(wh)]
            starts.which, starts.index, starts.cost = which, index, cost
        return x, fvec, sigma, cov, chi2, rank, ibs, status

    # -- bootstrap: intervals of any fit from refits of resampled data --------------------
    def boot_resample(self, boot, mu, y, weights=None, prob0=0, rep0=0, nrep=None):
        """The replicas rep0 .. rep0 + nrep - 1 (nrep=None: boot.nrep) of a Bootstrap for the data y [nprob, m] with the fitted
        values mu [nprob, m] -- curve_eval / expr_eval at the fit's x, through conv_apply where the fit has a response -- and
        optional weights (nlh_boot_resample_batch): (ystar, wstar), ystar [nrep, nprob, m], replica-major, so that
        ystar.reshape(nrep * nprob, m) is a batch for a fit; wstar the same shape for kind "pairs", None otherwise (the
        replicas keep the caller's weights).  prob0: the index of y[0] in the caller's whole data, when y is a slice of it.
        Rows of weight 0 stay as they are.  A replica depends on (boot.seed, problem, replica) alone."""
        nprob, m = y.shape
        _chk(y, (nprob, m), "y")
        pairs = boot.kind == _lib.BOOT_PAIRS
        if not pairs or mu is not None:
            _chk(mu, (nprob, m), "mu")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        nrep = boot.nrep if nrep is None else int(nrep)
        ystar = torch.empty((max(nrep, 0), nprob, m), dtype=torch.float64, device=y.device)
        wstar = torch.empty_like(ystar) if pairs else None
        self._call("nlh_boot_resample_batch", boot.kind, boot.seed, nprob, int(prob0), m, int(rep0), nrep,
                   mu.data_ptr() if mu is not None else None, y.data_ptr(), weights.data_ptr() if weights is not None else None,
                   int(boot.centre), ystar.data_ptr(), wstar.data_ptr() if pairs else None)
        return ystar, wstar

    def boot_poisson(self, boot, mu, y, weights=None, prob0=0, rep0=0, nrep=None):
        """The replicas rep0 .. rep0 + nrep - 1 (nrep=None: boot.nrep) of a PoissonBootstrap for the counts y [nprob, m] with the
        fitted values mu [nprob, m] and the optional 0 / 1 mask weights (nlh_boot_poisson_batch): (ystar, bad), ystar
        [nrep, nprob, m], replica-major, counts drawn from Poisson(mu) row by row -- a row of weight 0 keeps y, a row with
        mu == 0 is 0 --; bad [nprob] int32: how many unmasked rows of each problem have a mu that is a NaN, negative or above
        2^24 (they keep y: such a problem's replicas are not to be used).  prob0: the index of y[0] in the caller's whole data,
        when y is a slice of it.  A replica depends on (boot.seed, problem, replica, mu) alone."""
        nprob, m = y.shape
        _chk(y, (nprob, m), "y")
        _chk(mu, (nprob, m), "mu")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        nrep = boot.nrep if nrep is None else int(nrep)
        ystar = torch.empty((max(nrep, 0), nprob, m), dtype=torch.float64, device=y.device)
        bad = torch.zeros((nprob,), dtype=torch.int32, device=y.device)
        self._call("nlh_boot_poisson_batch", boot.seed, nprob, int(prob0), m, int(rep0), nrep, mu.data_ptr(), y.data_ptr(),
                   weights.data_ptr() if weights is not None else None, ystar.data_ptr(), bad.data_ptr())
        return ystar, bad

    def boot_summary(self, xs, level=0.95):
        """(lo, hi, mean, sd [nprob, n], nvalid [nprob] int32) of xs [nrep, nprob, n], the parameters the refits of the replicas
        gave (nlh_boot_summary_batch): a replica whose row holds a value that is not finite does not count; lo and hi are the
        (1 - level)/2 and 1 - (1 - level)/2 quantiles of the others (linear interpolation), mean and sd their mean and
        standard deviation.  No valid replica: NaN; one: sd is NaN."""
        nrep, nprob, n = xs.shape
        _chk(xs, (nrep, nprob, n), "xs")
        lo, hi, mean, sd = (torch.empty((nprob, n), dtype=torch.float64, device=xs.device) for _ in range(4))
        nvalid = torch.empty((nprob,), dtype=torch.int32, device=xs.device)
        self._call("nlh_boot_summary_batch", nrep, nprob, n, xs.data_ptr(), float(level), mean.data_ptr(), sd.data_ptr(), lo.data_ptr(),
                   hi.data_ptr(), nvalid.data_ptr())
        return lo, hi, mean, sd, nvalid

    # -- studentised and BCa intervals (include/nonlin_hip_boot_ci.h) --------------------
    def boot_student(self, xs, sigs, x, sigma, level=0.95):
        """(lo, hi [nprob, n], nvalid_t [nprob, n] int32): the bootstrap-t interval of the fit x with standard errors sigma
        [nprob, n] from the refits xs and their own standard errors sigs [nrep, nprob, n] (nlh_boot_student_batch).  A replica
        counts for a parameter when its whole row of xs is finite and its sigs there is finite and > 0; the quantiles T of
        (xs - x)/sigs give lo = x - T_hi sigma, hi = x - T_lo sigma.  No such replica, or an x or sigma that will not do: NaN."""
        nrep, nprob, n = xs.shape
        _chk(xs, (nrep, nprob, n), "xs"); _chk(sigs, (nrep, nprob, n), "sigs"); _chk(x, (nprob, n), "x"); _chk(sigma, (nprob, n), "sigma")
        lo, hi = (torch.empty((nprob, n), dtype=torch.float64, device=xs.device) for _ in range(2))
        nvalid_t = torch.empty((nprob, n), dtype=torch.int32, device=xs.device)
        self._call("nlh_boot_student_batch", nrep, nprob, n, xs.data_ptr(), sigs.data_ptr(), x.data_ptr(), sigma.data_ptr(), float(level),
                   lo.data_ptr(), hi.data_ptr(), nvalid_t.data_ptr())
        return lo, hi, nvalid_t

    def boot_jackknife(self, weights, nprob, m, row0=0, nrows=None):
        """The delete-one weights of the rows row0 .. row0 + nrows - 1 (nrows=None: up to m) of nprob data sets of m rows
        (nlh_boot_jackknife_batch): wout [nrows, nprob, m], deletion-major, so that wout.reshape(nrows * nprob, m) is the
        weights of a batch for a fit -- the caller's weights [nprob, m] (None: 1.0) with row row0 + r set to 0.0."""
        nprob, m, row0 = int(nprob), int(m), int(row0)
        nrows = m - row0 if nrows is None else int(nrows)
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        wout = torch.empty((max(nrows, 0), nprob, m), dtype=torch.float64, device=self.device)
        self._call("nlh_boot_jackknife_batch", nprob, m, row0, nrows, weights.data_ptr() if weights is not None else None, wout.data_ptr())
        return wout

    def boot_accel(self, xjack, weights=None):
        """(accel [nprob, n], njack [nprob] int32): the acceleration of a BCa interval from the delete-one refits xjack
        [m, nprob, n] (nlh_boot_accel_batch): a = sum d^3 / (6 (sum d^2)^1.5), d = mean - xjack_i, over the deletions of rows
        of non-zero weight whose refit is finite, njack of them.  Fewer than two, or no spread: 0.0."""
        m, nprob, n = xjack.shape
        _chk(xjack, (m, nprob, n), "xjack")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        accel = torch.empty((nprob, n), dtype=torch.float64, device=xjack.device)
        njack = torch.empty((nprob,), dtype=torch.int32, device=xjack.device)
        self._call("nlh_boot_accel_batch", m, nprob, n, xjack.data_ptr(), weights.data_ptr() if weights is not None else None,
                   accel.data_ptr(), njack.data_ptr())
        return accel, njack

    def boot_bca(self, xs, x, accel, level=0.95):
        """(lo, hi, z0, alpha_lo, alpha_hi [nprob, n], flags [nprob, n] int32, nvalid [nprob] int32): the BCa interval of the fit
        x [nprob, n] from the refits xs [nrep, nprob, n] and boot_accel's accel (nlh_boot_bca_batch): the quantiles of the valid
        replicas at the levels alpha, which are the percentile levels moved by z0 -- from the share of replicas below x -- and
        by accel.  flags: a sum of nonlin_amd.BCA_DEGENERATE (every replica on one side of x: the percentile interval),
        BCA_NO_ACCEL (accel not finite: taken as 0), BCA_BAD_DENOM (an end's adjustment has no meaning: that end keeps its
        percentile level) and BCA_NO_REPLICA (nothing to work with: NaN)."""
        nrep, nprob, n = xs.shape
        _chk(xs, (nrep, nprob, n), "xs"); _chk(x, (nprob, n), "x"); _chk(accel, (nprob, n), "accel")
        lo, hi, z0, alo, ahi = (torch.empty((nprob, n), dtype=torch.float64, device=xs.device) for _ in range(5))
        flags = torch.empty((nprob, n), dtype=torch.int32, device=xs.device)
        nvalid = torch.empty((nprob,), dtype=torch.int32, device=xs.device)
        self._call("nlh_boot_bca_batch", nrep, nprob, n, xs.data_ptr(), x.data_ptr(), accel.data_ptr(), float(level), lo.data_ptr(),
                   hi.data_ptr(), z0.data_ptr(), alo.data_ptr(), ahi.data_ptr(), flags.data_ptr(), nvalid.data_ptr())
        return lo, hi, z0, alo, ahi, flags, nvalid

    @staticmethod
    def _replicas(r, t, shared, weights, x, kw):
        """(t, weights, x, kw) of a chunk of r replicas, replica-major: what is per problem -- t unless shared, the weights, x,
        a Loss's scales and a Convolve's taps -- repeated r times."""
        loss, conv = kw.loss, kw.conv
        if loss is not None and not loss.shared:
            loss = _lib.Loss(loss.kind, np.tile(loss.scale, r))
        if conv is not None and not conv.shared:
            conv = _lib.Convolve(np.tile(conv.kernel, (r, 1)), conv.origin, conv.ext)
        return (t if shared else t.repeat(1, r, 1) if t.dim() == 3 else t.repeat(r, 1),
                weights.repeat(r, 1) if weights is not None else None, x.repeat(r, 1), kw._replace(loss=loss, conv=conv))

    def _boot_fit(self, model, t, y, x, boot, weights, kw, sigma=None):
        """The one-call bootstrap behind curve_boot_batch and expr_boot_batch: the fitted values -- model.eval(x, t), through
        conv_apply with conv --, then chunks of replicas whose y* stays within 256 MiB (the environment variable
        NLH_BOOT_REPS, read at every call, sets the replicas of a chunk instead: tests), each chunk one _fit call without
        covariance from x repeated, and the summary of what the fits returned, NaN where a fit's status is not 0.  A
        PoissonBootstrap takes boot_poisson's replicas and passes stat on to the refits; the refits of a problem with a bad
        fitted value are set to NaN on the device.
        boot.interval "percentile" makes exactly these calls.  "student": the refits run with covariance, their sigma is kept
        (NaN where the status is not 0), and boot_student replaces lo and hi.  "bca": after the replicas the m delete-one
        refits of every data set run through the same _fit from x, in chunks of deletions by the same rule -- y and what is per
        problem repeated as for replicas, the weights boot_jackknife's (of the caller's weights, or mask) --, then boot_accel
        and boot_bca.  Both return summary's mean, sd and nvalid, and a dict of what they computed on the way."""
        nprob, m, shared = model.data(t, y, weights)
        n, stat, group, conv = model.n, kw.stat, kw.group, kw.conv
        pois = isinstance(boot, _lib.PoissonBootstrap)
        if pois:
            if stat is None:
                raise ValueError("a PoissonBootstrap needs stat=Poisson(): its replicas are counts, refitted with the deviance")
            if group is not None:
                raise ValueError("a PoissonBootstrap excludes group: a group needs its own resampling")
        elif stat is not None or group is not None:
            raise ValueError("a bootstrap excludes stat and group: counts need a parametric sampler, a group its own resampling")
        pairs = not pois and boot.kind == _lib.BOOT_PAIRS
        if pairs and conv is not None:
            raise ValueError('kind "pairs" excludes conv: a convolution needs every row')
        kind = getattr(boot, "interval", "percentile")
        if kind == "student" and sigma is None:
            raise ValueError('interval "student" needs sigma=: the standard errors [nprob, n] of the fit x')
        _chk(x, (nprob, n), "x")
        if kind == "student":
            _chk(sigma, (nprob, n), "sigma")
        mu = None
        if not pairs:
            mu = model.eval(x, t)
            if conv is not None:
                mu = self.conv_apply(conv, mu)
        per = max(1, (256 << 20) // (8 * max(nprob * m, 1)))
        env = os.environ.get("NLH_BOOT_REPS")
        if env is not None and int(env) >= 1:
            per = int(env)
        refit = kw._replace(covariance=kind == "student", group=None)
        xs = torch.empty((boot.nrep, nprob, n), dtype=torch.float64, device=y.device)
        sigs = torch.empty_like(xs) if kind == "student" else None
        for rep0 in range(0, boot.nrep, per):
            r = min(per, boot.nrep - rep0)
            if pois:
                ystar, nbad = self.boot_poisson(boot, mu, y, weights, 0, rep0, r)
            else:
                ystar, wstar = self.boot_resample(boot, mu, y, weights, 0, rep0, r)
            tc, wc, xc, kc = self._replicas(r, t, shared, None if pairs else weights, x, refit)
            out = self._fit(model, tc, shared, ystar.reshape(r * nprob, m), wstar.reshape(r * nprob, m) if pairs else wc, xc, kc)
            bad = torch.tensor([s != 0 for s in out[7]], dtype=torch.bool, device=y.device)
            xs[rep0:rep0 + r] = out[0].masked_fill(bad[:, None], float("nan")).reshape(r, nprob, n)
            if sigs is not None:
                sigs[rep0:rep0 + r] = out[2].masked_fill(bad[:, None], float("nan")).reshape(r, nprob, n)
            if pois:                                                 # a problem with a bad fitted value has no valid replica
                xs[rep0:rep0 + r].masked_fill_((nbad > 0)[None, :, None], float("nan"))
        summary = self.boot_summary(xs, boot.level)
        if kind == "percentile":
            return summary + (xs,)
        if kind == "student":
            lo, hi, nvalid_t = self.boot_student(xs, sigs, x, sigma, boot.level)
            return (lo, hi) + summary[2:] + (xs, dict(sigs=sigs, nvalid_t=nvalid_t))
        xjack = torch.empty((m, nprob, n), dtype=torch.float64, device=y.device)
        for row0 in range(0, m, per):
            r = min(per, m - row0)
            wj = self.boot_jackknife(weights, nprob, m, row0, r)
            tc, _, xc, kc = self._replicas(r, t, shared, None, x, refit)
            out = self._fit(model, tc, shared, y.repeat(r, 1), wj.reshape(r * nprob, m), xc, kc)
            bad = torch.tensor([s != 0 for s in out[7]], dtype=torch.bool, device=y.device)
            xjack[row0:row0 + r] = out[0].masked_fill(bad[:, None], float("nan")).reshape(r, nprob, n)
        accel, njack = self.boot_accel(xjack, weights)
        lo, hi, z0, alo, ahi, flags, _ = self.boot_bca(xs, x, accel, boot.level)
        return (lo, hi) + summary[2:] + (xs, dict(xjack=xjack, njack=njack, accel=accel, z0=z0, alpha_lo=alo, alpha_hi=ahi, flags=flags))

    def curve_boot_batch(self, kind, t, y, x, boot, ncomp=1, baseline=-1, weights=None, lower=None, upper=None, analytic=True,
                         opts=None, pmap=None, loss=None, stat=None, group=None, conv=None, sep=None, sigma=None):
        """The bootstrap of curve_fit_batch's fit x [nprob, n] of the data t, y (a Bootstrap: nlh_boot_resample_batch, the fit
        itself, nlh_boot_summary_batch): boot.nrep replicas of every data set are made from the fitted values and the data,
        each is fitted exactly as the keywords say -- the caller's bounds, pmap, loss, conv and sep, started from x, without
        covariance --, and what comes back is (lo, hi, mean, sd, nvalid, xs): the percentile interval of boot.level, the mean
        and the standard deviation of every parameter over the replicas whose fit ended with status 0 ([nprob, n]), how many
        those are ([nprob], int32), and the refits' parameters themselves, xs [nrep, nprob, n], NaN where a fit failed.  The
        result depends on (boot, the data, x) alone, not on how the replicas are chunked.  stat= and group= raise ValueError,
        and so does kind "pairs" with conv=.
        Counts: boot a PoissonBootstrap together with stat=Poisson() (nlh_boot_poisson_batch) -- the replicas are counts drawn
        from Poisson(fitted values), each refitted with stat and the caller's bounds, pmap, conv and mask; a problem whose
        fitted values hold a NaN, a negative value or one above 2^24 on an unmasked row comes back with nvalid 0 and NaN.  A
        PoissonBootstrap without stat=, or with group=, raises ValueError.
        boot.interval (of either kind of boot) chooses the interval; "percentile" is everything above.  "student": sigma= is
        required -- the fit's own standard errors [nprob, n], curve_fit_batch's sigma; without it ValueError --, every refit
        runs WITH covariance, and lo, hi are the bootstrap-t interval x - T sigma from the quantiles T of (x* - x)/sigma* over
        the replicas whose sigma* is finite and > 0 (a fixed parameter of a pmap has none: NaN).  "bca": after the replicas
        every data set is refitted m more times, each with one row's weight (or mask entry) set to 0 -- m extra fits per data
        set, so the cost grows with the SQUARE of m: 128 rows at 200 replicas make 328 fits per data set --, and lo, hi are
        the quantiles at the bias-corrected and accelerated levels.  Both return (lo, hi, mean, sd, nvalid, xs, info): mean,
        sd and nvalid are the summary's, info a dict -- sigs [nrep, nprob, n] and nvalid_t [nprob, n] for "student"; xjack
        [m, nprob, n], njack [nprob], accel, z0, alpha_lo, alpha_hi and flags [nprob, n] (BCA_* bits) for "bca".  conv= is
        allowed with both: a zero weight removes a row of the residual, not of the convolution."""
        return self._boot_fit(self._curve_model(kind, ncomp, baseline), t, y, x, boot, weights,
                              _Keywords(lower, upper, analytic, False, opts, pmap, loss, stat, group, conv, sep), sigma)

    def expr_boot_batch(self, expr, t, y, x, boot, weights=None, lower=None, upper=None, analytic=True, opts=None, pmap=None,
                        loss=None, stat=None, group=None, conv=None, sep=None, sigma=None):
        """curve_boot_batch with an Expr in the place of (kind, ncomp, baseline): the bootstrap of expr_fit_batch's fit x."""
        return self._boot_fit(self._expr_model(expr), t, y, x, boot, weights,
                              _Keywords(lower, upper, analytic, False, opts, pmap, loss, stat, group, conv, sep), sigma)

    @staticmethod
    def _fit_outputs(x0, m, covariance, nsolve, nunk):
        """What a one-call fit writes: x (a copy of x0 [nprob, n]), fvec [nprob, m], sigma [nprob, n] and, per problem of the
        solve -- nsolve of them over nunk unknowns: the data sets themselves, or the groups of a global fit --, cov, chi2, rank
        (None with covariance=False), the iteration records and the status array."""
        nprob, n = x0.shape
        dev = x0.device
        x = x0.clone()
        fvec = torch.empty((nprob, m), dtype=torch.float64, device=dev)
        sigma = cov = chi2 = rank = None
        if covariance:
            sigma = torch.empty((nprob, n), dtype=torch.float64, device=dev)
            cov = torch.empty((nsolve, nunk, nunk), dtype=torch.float64, device=dev)
            chi2 = torch.empty((nsolve,), dtype=torch.float64, device=dev)
            rank = torch.empty((nsolve,), dtype=torch.int32, device=dev)
        return (x, fvec, sigma, cov, chi2, rank) + _ib_status(nsolve)

    def curve_fit_batch(self, kind, t, y, x0, ncomp=1, baseline=-1, weights=None, lower=None, upper=None, analytic=True,
                        covariance=True, opts=None, pmap=None, loss=None, stat=None, group=None, conv=None, sep=None, starts=None,
                        bins=None):
        """Fit + errors of y.shape[0] curves in one call (nlh_curve_fit_batch): least_squares_solver%solve -- or, with lower /
        upper ([n], one box for every problem), constrained_least_squares_solver%solve -- from x0 [nprob, n] (not modified),
        then the scaled parameter covariance at the solution.  Rows with weight 0 pad ragged data: they do not count as
        degrees of freedom.  Returns (x, fvec, sigma, cov, chi2, rank, ibs, status); sigma, cov, chi2, rank are None with
        covariance=False, NaN / -1 for a problem whose status is not 0.
        x0=None: the fit starts from curve_guess(kind, t, y, ncomp, baseline, weights)[0]; together with pmap or group it
        raises ValueError.
        pmap (a ParamMap over the model's n parameters): fixed and tied parameters (nlh_curve_fit_batch_pmap).  Every array
        keeps its full size; a fixed parameter keeps the value x0 holds for its problem, tied positions of x0 are ignored,
        bound entries at fixed and tied positions are not read, and sigma / cov are those of the full parameters.
        loss (a Loss): a robust fit (nlh_curve_fit_batch_loss), with or without pmap.  fvec is then the transformed residual
        rho~, chi2 = sum rho~^2 / dof, and sigma / cov are those of the transformed problem; loss_apply on the raw residuals
        gives the weights that flag outliers.  None calls exactly what is called without it.
        stat (a Poisson): y are counts and the fit minimises their Poisson deviance (nlh_curve_fit_batch_pois), with or without
        pmap.  weights is then the 0 / 1 mask of the rows, fvec the deviance residual, chi2 the deviance / dof, and sigma / cov
        are unscaled: the inverse Fisher information.  stat together with loss raises ValueError.
        group (a Group over the model's n parameters): a global fit (nlh_curve_fit_batch_group), with or without loss or stat:
        every group.nsets consecutive rows of y are one group, whose shared parameters have one value.  x0, x, fvec and sigma
        stay per data set (a shared parameter starts from the value of the group's first data set and comes back equal across
        the group); cov [ngroup, nouter, nouter] (group.index locates entries), chi2, rank, ibs and status are per group.
        group together with pmap raises ValueError.  None calls exactly what is called without it.
        conv (a Convolve): the model is convolved with an instrument response before it is compared with y
        (nlh_curve_fit_batch_conv), with or without pmap, loss, stat or group: t must be a uniform grid and y finite on every
        row, padded ones included.  fvec is the residual of the convolved model; conv_apply on curve_eval's values gives the
        convolved model itself.  None calls exactly what is called without it.
        sep (a Separable, e.g. Separable.for_curve(kind, ncomp, baseline)): a separable fit (nlh_curve_fit_batch_sep), with or
        without conv: the linear parameters are solved for exactly at every trial point (variable projection) and the solver
        iterates over the others, so x0 needs no values at the linear positions.  Everything that comes back is full -- x the
        solution with its linear parameters, fvec the model's residual there, sigma / cov / chi2 / rank those of the full
        model at x.  Bounds at linear positions must be infinite.  With group the shared parameters must all be nonlinear
        (shared lifetimes, amplitudes projected out per data set) and cov, chi2, rank, ibs, status are per group, as from
        group= alone.  sep together with pmap, loss or stat raises ValueError: those are nonlinear in the projected parameters.
        starts (a Starts over the model's n parameters, with x0=None): the fit starts from a scan of the box instead of a
        guess -- starts.ncand candidates are scored, for every problem at once, with the cost this fit minimises (through conv,
        loss, stat; with sep over the nonlinear parameters only, the linear positions of x0 being 0.0), the fit runs from each of
        the starts.keep best, and what comes back is, per problem, the fit of smallest final cost (sum fvec^2; NaN and rank -1
        where no fit ended finite; ibs and status are the chosen fit's).  The record -- which start, which candidates, their
        scan cost -- is left on the Starts object (see there).  lower / upper stay the solver's box, independent of the
        scan's.  starts together with an x0, with pmap or with group raises ValueError.  None calls exactly what is called
        without it.
        bins (a Binned over y's m bins): y was recorded in bins -- counts of a histogram, the pixels of an image -- and the
        model is integrated (or averaged) over every bin by the Binned's rule before it is compared with y.  t is then not
        read -- the model is evaluated at bins.nodes() -- and must be None.  The call is composed here from the launchers, in
        the order of the library's own pipeline: the model on the nodes, bin_launchers, then conv_launchers, then
        pois_launchers or loss_launchers, lm_solve_batch_device (cls_solve_batch_device with bounds) and
        lm_covariance_batch_device; with weights the zero-weight rule of the header (dof = rows with non-zero weight - n,
        chi2 and cov times (m - n) / dof, sigma from that cov) is applied in torch: that arithmetic is torch's, not
        bit-stated.  A problem with dof <= 0 raises ValueError.  bins together with pmap, group, sep, starts or x0=None raises
        ValueError: use bin_launchers with pmap_launchers, group_launchers, sep_launchers or starts_search.  There is no
        bins= in the bootstrap calls and no curve_guess on binned data.  None calls exactly what is called without it."""
        return self._fit_front(self._curve_model(kind, ncomp, baseline), t, y, x0, weights, starts, bins,
                               _Keywords(lower, upper, analytic, covariance, opts, pmap, loss, stat, group, conv, sep))

    def _fit_front(self, model, t, y, x0, weights, starts, bins, kw):
        """curve_fit_batch and expr_fit_batch once they have bound their model: what is refused before the data are looked
        at, then bins= (_bin_fit), the data, starts= (_starts_fit), the guess of a model that has one for x0=None, and _fit."""
        if kw.stat is not None and kw.loss is not None:
            raise ValueError("stat and loss exclude each other: a Poisson fit has no robust loss")
        if bins is not None:
            for name, v in (("pmap", kw.pmap), ("group", kw.group), ("sep", kw.sep), ("starts", starts)):
                if v is not None:
                    raise ValueError(f"bins excludes {name}: compose bin_launchers with the other launchers and call the solver")
            return self._bin_fit(model, t, y, weights, x0, bins, kw)
        nprob, m, shared = model.data(t, y, weights)
        if starts is not None:
            if x0 is not None:
                raise ValueError("starts excludes x0: the scan makes the starting values")
            return self._starts_fit(model, t, shared, y, weights, starts, kw)
        if x0 is None and model.guess is not None:
            if kw.pmap is not None or kw.group is not None:
                raise ValueError("x0=None excludes pmap and group: a fixed or a shared parameter needs the caller's value")
            x0 = model.guess(t, y, weights)[0]
        _chk(x0, (nprob, model.n), "x0")
        return self._fit(model, t, shared, y, weights, x0, kw)

    def _fit(self, model, t, shared, y, weights, x0, kw):
        """The one-call fit of a bound model on checked data: what the features refuse, the entry point they select, its
        outputs -- per group with a group, per data set without --, and the call, its arguments in the order of
        _lib.fit_args.  A feature that is None gives what the entry points read as "none": a NULL pointer, kind 0, shared 0,
        stat 0, mu_floor 0.0."""
        lower, upper, analytic, covariance, opts, pmap, loss, stat, group, conv, sep = kw
        (nprob, m), n = y.shape, model.n
        _refuse_sep(kw, n)
        if group is not None:
            if pmap is not None:
                raise ValueError("group and pmap exclude each other: a map inside a group works through pmap_launchers and group_launchers")
            if group.nparams != n:
                raise ValueError(f"group is over {group.nparams} parameters, the model has {n}")
            if nprob % group.nsets:
                raise ValueError(f"{nprob} data sets: no multiple of the group's {group.nsets}")
        if pmap is not None and pmap.nfull != n:
            raise ValueError(f"pmap maps {pmap.nfull} parameters, the {'formula' if model.name == 'expr' and conv is None else 'model'} has {n}")
        variant = ("_sep" if sep is not None else "_conv" if conv is not None else "_group" if group is not None else
                   "_pois" if stat is not None else "_loss" if loss is not None else "_pmap" if pmap is not None else "")
        nsolve, nunk = (nprob // group.nsets, group.nouter) if group is not None else (nprob, n)
        x, fvec, sigma, cov, chi2, rank, ib, status = self._fit_outputs(x0, m, covariance, nsolve, nunk)
        plo, phi = _host_bounds(lower, upper, n)
        o = opts or self.options()
        dscale, sh = self._loss_scale(loss, nprob, y.device) if loss is not None else (None, 0)     # dscale, dk: alive across the call
        cv, dk = self._conv_struct(conv, nprob, y.device) if conv is not None else (None, None)
        ptr = lambda a: a.data_ptr() if a is not None else None
        obj = lambda a: a.ptr if a is not None else None
        val = dict(model.head, opts=C.byref(o), nprob=nprob, m=m, t=t.data_ptr(), shared_t=shared, y=y.data_ptr(), w=ptr(weights),
                   analytic=int(bool(analytic)), xl=plo, xu=phi, pm=obj(pmap), g=obj(group), sp=obj(sep),
                   cv=C.byref(cv) if cv is not None else None, loss=loss.kind if loss is not None else 0, scale=ptr(dscale),
                   shared_scale=sh, stat=1 if stat is not None else 0, mu_floor=stat.mu_floor if stat is not None else 0.0,
                   x=x.data_ptr(), fvec=fvec.data_ptr(), sigma=ptr(sigma), cov=ptr(cov), chi2=ptr(chi2), rank=ptr(rank), ib=ib,
                   status=status)
        self._call(f"nlh_{model.name}_fit_batch{variant}", *[val[name] for name, _ in _lib.fit_args(model.name, variant)])
        return (x, fvec, sigma, cov, chi2, rank) + _ib_lists(ib, status)

    # -- formula models ----------------------------------------------------------
    @staticmethod
    def _expr_t(expr, t, nprob, m):
        """shared_t of the abscissae t of a formula model, checked: [nvar, nprob, m], or shared [nvar, m]; with one variable
        [nprob, m] or shared [m] will do."""
        if expr.nvar == 1 and t.dim() == 2 and tuple(t.shape) == (nprob, m):
            shape, shared = (nprob, m), 0
        elif t.dim() == 3:
            shape, shared = (expr.nvar, nprob, m), 0
        elif t.dim() == 1:
            shape, shared = (m,) if expr.nvar == 1 else (expr.nvar, m), 1
        else:
            shape, shared = (expr.nvar, m), 1
        _chk(t, shape, "t")
        return shared

    def _expr_data(self, expr, t, y, weights):
        """(nprob, m, shared_t) of the data tensors of a formula model, checked."""
        nprob, m = y.shape
        _chk(y, (nprob, m), "y")
        shared = self._expr_t(expr, t, nprob, m)
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        return nprob, m, shared

    def _expr_model(self, expr):
        """The _Model of a formula: it has no guess."""
        return _Model("expr", dict(expr=expr.ptr), expr.nparams, expr.nvar,
                      lambda t, y, weights: self._expr_data(expr, t, y, weights),
                      lambda t, y, weights: self.expr_launchers(expr, t, y, weights),
                      lambda x, t: self.expr_eval(expr, x, t), None)

    def expr_launchers(self, expr, t, y, weights=None):
        """A formula model (nonlin_amd.Expr) on the data t [nvar, nprob, m] (or shared [nvar, m]; one variable: [nprob, m] or
        [m]), y [nprob, m] with optional weights [nprob, m], as (fcn, jac, ctx) for lm_solve_batch_device,
        cls_solve_batch_device, lm_covariance_batch_device and fd_jacobian_device.  Keep ctx alive while solving (it keeps
        the tensors and the expression)."""
        nprob, m, shared = self._expr_data(expr, t, y, weights)
        ctx = _lib.ExprCtx(expr.ptr, shared, m, t.data_ptr(), y.data_ptr(), weights.data_ptr() if weights is not None else None,
                           m if shared else nprob * m)
        ctx._keep = (expr, t, y, weights)                             # the context holds addresses: they live as long as it does
        return (C.cast(self.lib.nlh_expr_device_fcn, _lib.DEVFCN), C.cast(self.lib.nlh_expr_device_jac, _lib.DEVFCN), ctx)

    def expr_eval(self, expr, x, t):
        """Model values (no data term, no weights) of x [nprob, n] at t [nvar, nprob, npts] (or shared [nvar, npts]; one
        variable: [nprob, npts] or [npts]): y [nprob, npts]."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        if n != expr.nparams:
            raise ValueError(f"x has {n} columns, the formula {expr.nparams} parameters")
        npts = t.shape[-1]
        shared = self._expr_t(expr, t, nprob, npts)
        y = torch.empty((nprob, npts), dtype=torch.float64, device=x.device)
        self._call("nlh_expr_eval_batch", expr.ptr, nprob, npts, t.data_ptr(), int(shared), x.data_ptr(), y.data_ptr())
        return y

    def wofz_batch(self, z):
        """The Faddeeva function w(z) of a complex128 device tensor with Im z >= 0 (nlh_faddeeva_batch: a thread per element; the
        bits of nonlin_amd.wofz).  Below the real axis is outside the domain: what comes back there is not w."""
        if z.dtype != torch.complex128:
            raise ValueError("z must be complex128")
        re, im = z.real.contiguous().reshape(-1), z.imag.contiguous().reshape(-1)
        wr, wi = torch.empty_like(re), torch.empty_like(re)
        self._call("nlh_faddeeva_batch", re.numel(), re.data_ptr(), im.data_ptr(), wr.data_ptr(), wi.data_ptr())
        return torch.complex(wr, wi).reshape(z.shape)

    def expr_fit_batch(self, expr, t, y, x0, weights=None, lower=None, upper=None, analytic=True, covariance=True, opts=None,
                       pmap=None, loss=None, stat=None, group=None, conv=None, sep=None, starts=None, bins=None):
        """Fit + errors of y.shape[0] data sets to a formula in one call (nlh_expr_fit_batch): curve_fit_batch with an Expr in
        the place of (kind, ncomp, baseline), pmap (e.g. ParamMap.for_expr(expr, ...)), loss (a Loss), stat (a Poisson) and
        group (e.g. Group.for_expr(expr, shared=("k",), nsets=8): nlh_expr_fit_batch_group) included.  Returns (x, fvec, sigma,
        cov, chi2, rank, ibs, status).  x0=None with starts (e.g. Starts.for_expr(expr, lower={..}, upper={..})): the fit starts
        from the best candidates of a box, as in curve_fit_batch.  bins (a Binned; Binned.pixels for a formula of two
        variables): the formula is integrated or averaged over the bins y was recorded in, as in curve_fit_batch; t is then
        not read and must be None."""
        # conv (a Convolve) and sep (a Separable, e.g. Separable.for_expr(expr, linear=("a", "c"))): as in curve_fit_batch
        return self._fit_front(self._expr_model(expr), t, y, x0, weights, starts, bins,
                               _Keywords(lower, upper, analytic, covariance, opts, pmap, loss, stat, group, conv, sep))

    # -- parameter maps ------------------------------------------------------------
    def pmap_launchers(self, pmap, fcn, jac, ctx, full):
        """Fixed and tied parameters for any launcher pair: wraps (fcn, jac, ctx) -- of curve_launchers, expr_launchers,
        dq_launchers or a user's own -- in the map's launchers (nlh_pmap_wrap) and returns (fcn, jac, ctx) for
        lm_solve_batch_device, cls_solve_batch_device, lm_covariance_batch_device and fd_jacobian_device, which then work on
        x [nprob, pmap.nfree].  full: the full parameters [nprob, pmap.nfull], or one shared [pmap.nfull] tensor; it is read at
        fixed positions only.  jac is None without an inner Jacobian launcher (pass jac=None to the solver: forward
        differences over the free unknowns).  Keep the returned ctx alive while solving; ctx.close() frees it (so does
        garbage collection)."""
        shared = full.dim() == 1
        _chk(full, (pmap.nfull,) if shared else (full.shape[0], pmap.nfull), "full")
        return self._wrap("pmap", (pmap, fcn, jac, ctx, full), fcn, jac, ctx, (pmap.ptr,), (full.data_ptr(), int(shared)))

    def pmap_gather(self, pmap, full):
        """The free unknowns x [nprob, nfree] of full parameters [nprob, nfull] (nlh_pmap_gather_batch)."""
        nprob = full.shape[0]
        _chk(full, (nprob, pmap.nfull), "full")
        x = torch.empty((nprob, pmap.nfree), dtype=torch.float64, device=full.device)
        self._call("nlh_pmap_gather_batch", pmap.ptr, nprob, full.data_ptr(), x.data_ptr())
        return x

    def pmap_expand(self, pmap, x, full):
        """The full parameters [nprob, nfull] of the free unknowns x [nprob, nfree]: fixed values from full ([nprob, nfull] or
        one shared [nfull] tensor), ties evaluated (nlh_pmap_expand_batch)."""
        nprob = x.shape[0]
        _chk(x, (nprob, pmap.nfree), "x")
        shared = full.dim() == 1
        _chk(full, (pmap.nfull,) if shared else (nprob, pmap.nfull), "full")
        p = torch.empty((nprob, pmap.nfull), dtype=torch.float64, device=x.device)
        self._call("nlh_pmap_expand_batch", pmap.ptr, nprob, x.data_ptr(), full.data_ptr(), int(shared), p.data_ptr())
        return p

    def pmap_cov(self, pmap, cov, sigma, fail=None):
        """Covariance [nprob, nfull, nfull] and standard errors [nprob, nfull] of the full parameters from those of the free
        unknowns (nlh_pmap_cov_batch); fail: int32 [nprob], non-zero for a problem that did not solve (NaN everywhere)."""
        nprob = cov.shape[0]
        _chk(cov, (nprob, pmap.nfree, pmap.nfree), "cov"); _chk(sigma, (nprob, pmap.nfree), "sigma")
        cf = torch.empty((nprob, pmap.nfull, pmap.nfull), dtype=torch.float64, device=cov.device)
        sf = torch.empty((nprob, pmap.nfull), dtype=torch.float64, device=cov.device)
        self._call("nlh_pmap_cov_batch", pmap.ptr, nprob, cov.data_ptr(), sigma.data_ptr(),
                   fail.data_ptr() if fail is not None else None, cf.data_ptr(), sf.data_ptr())
        return cf, sf

    # -- profile-likelihood intervals ------------------------------------------------
    @staticmethod
    def _pin_tables(src, pos, theta):
        """nend of the three tables of a pin pair, checked: src, pos int32 and theta float64, contiguous GPU tensors [nend]."""
        nend = theta.shape[0] if theta.dim() == 1 else -1
        _chk(theta, (nend,), "theta")
        for name, v in (("src", src), ("pos", pos)):
            if not (v.is_cuda and v.dtype == torch.int32 and v.is_contiguous() and tuple(v.shape) == (nend,)):
                raise ValueError(f"{name}: expected a contiguous int32 GPU tensor of shape ({nend},)")
        return nend

    def pin_launchers(self, fcn, jac, ctx, N, src, pos, theta):
        """One parameter per wrapped problem held at its own value, the data shared, for any launcher pair: wraps (fcn, jac,
        ctx) over N unknowns in the pin pair (nlh_pin_wrap) and returns (fcn, jac, ctx) for lm_solve_batch_device,
        cls_solve_batch_device and fd_jacobian_device, which then work on x [nend, N - 1]: wrapped problem w is the inner
        problem src[w] (int32) with its unknown pos[w] (int32) held at theta[w]; the others keep their order.  Only copies
        happen, and no data are replicated: the inner launchers are called with src as their problem list.  jac is None
        without an inner Jacobian launcher.  An entry of src or pos out of range is the caller's error.  Keep the returned ctx
        alive while solving; ctx.close() frees it (so does garbage collection)."""
        nend = self._pin_tables(src, pos, theta)
        return self._wrap("pin", [(fcn, jac, ctx), (src, pos, theta)], fcn, jac, ctx, (int(N),),
                          (nend, src.data_ptr(), pos.data_ptr(), theta.data_ptr()))

    def pin_set(self, pin_ctx, src, pos, theta):
        """Swaps the three tables of a pin pair, and with them the number of wrapped problems, between solves (nlh_pin_set)."""
        nend = self._pin_tables(src, pos, theta)
        rc = self.lib.nlh_pin_set(pin_ctx.ptr, nend, src.data_ptr(), pos.data_ptr(), theta.data_ptr())
        if rc:
            raise ValueError(f"nlh_pin_set returned {rc}")
        pin_ctx._keep[1] = (src, pos, theta)

    def _profile_state(self, nprob, n):
        """(the tensors of a profile's state by name, the nlh_profile_state that holds their addresses)."""
        dev, nend = self.device, nprob * n * 2
        st = {k: torch.empty((nprob,) if k in ("C0", "delta") else (nend,),
                             dtype=torch.float64 if i < 11 else torch.int32, device=dev)
              for i, (k, _) in enumerate(_lib.ProfileState._fields_)}
        return st, _lib.ProfileState(**{k: v.data_ptr() for k, v in st.items()})

    def profile_start(self, fcn, ctx, m, x, sigma, prof, dof=None, scaled=True, lower=None, upper=None):
        """The start of a Profile's root finder at the fit x, sigma [nprob, n] of the UNPINNED launcher (fcn, ctx) over m rows
        (nlh_profile_start_batch_device): the state, a dict of device tensors by the names of nlh_profile_state -- C0, delta
        [nprob]; xhat, width, bound, theta, a, ga, b, gb, end (float64) and phase, flag, last, nexp, nev, nfail (int32), each
        [nprob * n * 2], end (p*n + j)*2 + s.  dof: int32 [nprob] or None (m - n); lower, upper: one box [n] or None."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x"); _chk(sigma, (nprob, n), "sigma")
        if dof is not None and not (dof.is_cuda and dof.dtype == torch.int32 and dof.is_contiguous() and tuple(dof.shape) == (nprob,)):
            raise ValueError(f"dof: expected a contiguous int32 GPU tensor of shape ({nprob},)")
        st, cs = self._profile_state(nprob, n)
        plo, phi = _host_bounds(lower, upper, n)
        self._call("nlh_profile_start_batch_device", self._devfcn(fcn), self._ctxp(ctx), nprob, int(m), n, x.data_ptr(), sigma.data_ptr(),
                   dof.data_ptr() if dof is not None else None, prof.crit, int(bool(scaled)), plo, phi, C.byref(cs))
        st["_struct"] = cs
        return st

    def profile_step(self, state, act, cost, fail, prof):
        """One step of the root finder for the active ends act [nact] (int32) with the costs cost [nact] of their refits and
        fail [nact] (int32, non-zero: the refit did not end well) or None (nlh_profile_step_batch): the state is updated in
        place; returns how many ends are still running."""
        nact = act.shape[0]
        _chk(cost, (nact,), "cost")
        for name, v in (("act", act), ("fail", fail)):
            if v is not None and not (v.is_cuda and v.dtype == torch.int32 and v.is_contiguous() and tuple(v.shape) == (nact,)):
                raise ValueError(f"{name}: expected a contiguous int32 GPU tensor of shape ({nact},)")
        nprob = state["C0"].shape[0]
        n = state["theta"].shape[0] // (2 * nprob) if nprob else 1
        left = C.c_int32()
        self._call("nlh_profile_step_batch", nprob, n, nact, act.data_ptr(), cost.data_ptr(), fail.data_ptr() if fail is not None else None,
                   C.byref(state["_struct"]), prof.tol, prof.xtol, prof.max_expand, prof.maxit, C.byref(left))
        return int(left.value)

    def profile_batch_device(self, fcn, jac, ctx, m, x, sigma, prof, dof=None, scaled=True, lower=None, upper=None, opts=None):
        """The profile-likelihood intervals (a Profile) of the fit x with the standard errors sigma [nprob, n] of ANY launcher pair
        (fcn, jac, ctx) over m rows -- a user's, a model's, or one composed with the wrapping launchers: (lo, hi [nprob, n],
        flags, nev [nprob, n, 2] int32).  For every problem, parameter and side the root finder of nlh_profile_* looks for the
        value of the parameter at which the cost of the refit of all the others has risen by delta = crit * C0 / dof (scaled;
        dof: int32 [nprob], None: m - n) or crit (scaled=False: a deviance): start, then rounds of -- the tables of the active
        ends (pin_set), ONE lm_solve_batch_device over all of them through the pin pair, each from the solution of its latest
        successful refit (at first x without the pinned entry), starts_cost of the fvec, step -- until no end is left.  With
        lower / upper (one box [n]) the refits are cls_solve_batch_device's, one call per parameter on the box without its
        entry, and an interval ends at the bound.  jac=None: forward differences over the N - 1 unknowns.  A refit whose
        status is not 0 counts as failed.  flags holds a PROFILE_* code per end plus the bit PROFILE_LOWER; lo / hi are -Inf /
        +Inf for an open end and NaN where there is none.  The ends are chunked so that the refits' fvec stays within 256 MiB
        (the environment variable NLH_PROFILE_ENDS, read at every call, sets the ends of a chunk instead: tests); the result does
        not depend on the chunks.  n = 1 raises ValueError."""
        nprob, n = x.shape
        if n < 2:
            raise ValueError("profile: a model of one parameter has no other to refit (n = 1 is not implemented)")
        plo, phi = _host_bounds(lower, upper, n)                      # (the shapes, before any device work)
        st = self.profile_start(fcn, ctx, m, x, sigma, prof, dof, scaled, lower, upper)
        dev, nend = x.device, nprob * n * 2
        e = torch.arange(nend, dtype=torch.int64, device=dev)
        src, pos = (e // (2 * n)).to(torch.int32), ((e // 2) % n).to(torch.int32)
        keep = torch.tensor([[k for k in range(n) if k != j] for j in range(n)], dtype=torch.int64, device=dev)     # [n, n - 1]
        warm = x[:, None, None, :].expand(nprob, n, 2, n).reshape(nend, n).gather(1, keep[pos.long()])
        per = max(1, (256 << 20) // (8 * m))
        env = os.environ.get("NLH_PROFILE_ENDS")
        if env is not None and int(env) >= 1:
            per = int(env)
        o = opts or self.options()
        bounded = lower is not None or upper is not None
        box = [tuple(None if b is None else np.delete(np.asarray(b, dtype=np.float64), j) for b in (lower, upper)) for j in range(n)]
        seed = (src[:1].contiguous(), pos[:1].contiguous(), st["theta"][:1].contiguous())
        pfcn, pjac, pctx = self.pin_launchers(fcn, jac, ctx, n, *seed)
        try:
            while True:
                act = (st["phase"] != _lib.PROFILE_DONE).nonzero().reshape(-1)
                nact = act.shape[0]
                if nact == 0:
                    break
                cost = torch.empty((nact,), dtype=torch.float64, device=dev)
                fail = torch.empty((nact,), dtype=torch.int32, device=dev)
                for c0 in range(0, nact, per):
                    ch = act[c0:c0 + per]
                    groups = [ch[pos[ch] == j] for j in range(n)] if bounded else [ch]
                    for j, sel in enumerate(groups):
                        if sel.shape[0] == 0:
                            continue
                        self.pin_set(pctx, src[sel].contiguous(), pos[sel].contiguous(), st["theta"][sel].contiguous())
                        xw = warm[sel].contiguous()
                        if bounded:
                            fvec, _, status = self.cls_solve_batch_device(pfcn, pctx, m, xw, jac=pjac, opts=o, lower=box[j][0], upper=box[j][1])
                        else:
                            fvec, _, status = self.lm_solve_batch_device(pfcn, pctx, m, xw, jac=pjac, opts=o)
                        cs = self.starts_cost(fvec)
                        bad = torch.tensor([s != 0 for s in status], dtype=torch.bool, device=dev)
                        good = ~bad & torch.isfinite(cs)
                        warm[sel[good]] = xw[good]
                        where = (ch[:, None] == sel[None, :]).nonzero()[:, 0] + c0 if bounded else torch.arange(c0, c0 + sel.shape[0], device=dev)
                        cost[where] = cs
                        fail[where] = bad.to(torch.int32)
                self.profile_step(st, act.to(torch.int32), cost, fail, prof)
        finally:
            pctx.close()
        end = st["end"].reshape(nprob, n, 2)
        return (end[:, :, 0].contiguous(), end[:, :, 1].contiguous(), st["flag"].reshape(nprob, n, 2), st["nev"].reshape(nprob, n, 2))

    def _profile_fit(self, model, t, y, x, sigma, prof, weights, kw, bins=None, starts=None):
        """The one-call profile behind curve_profile_batch and expr_profile_batch: profile_batch_device on the launcher stack of
        the fit (_stack), through pmap_launchers with pmap=, with scaled = stat is None and dof the rows with non-zero weight
        minus the free parameters."""
        if starts is not None:
            raise ValueError("a profile excludes starts: it starts from the fit x")
        for name, v in (("sep", kw.sep), ("group", kw.group)):
            if v is not None:
                raise ValueError(f"a profile excludes {name}: compose the launchers and call profile_batch_device")
        if kw.stat is not None and kw.loss is not None:
            raise ValueError("stat and loss exclude each other: a Poisson fit has no robust loss")
        if not isinstance(prof, _lib.Profile):
            raise ValueError("prof: expected a Profile")
        if bins is not None:
            if t is not None:
                raise ValueError("bins excludes t: the model is evaluated at bins.nodes(); pass t=None")
            if bins.nvar != model.nvar:
                raise ValueError(f"bins are over {bins.nvar} variable(s), the model has {model.nvar}")
            nprob, m = y.shape
            _chk(y, (nprob, m), "y")
            if weights is not None:
                _chk(weights, (nprob, m), "weights")
        else:
            nprob, m, _ = model.data(t, y, weights)
        n, pmap, dev = model.n, kw.pmap, y.device
        _chk(x, (nprob, n), "x"); _chk(sigma, (nprob, n), "sigma")
        if pmap is not None and pmap.nfull != n:
            raise ValueError(f"pmap maps {pmap.nfull} parameters, the model has {n}")
        nfree = pmap.nfree if pmap is not None else n
        if nfree < 2:
            raise ValueError("profile: a model of one free parameter has no other to refit (n = 1 is not implemented)")
        _host_bounds(kw.lower, kw.upper, n)
        rows = (weights != 0).sum(dim=1) if weights is not None else torch.full((nprob,), m, dtype=torch.int64, device=dev)
        dof = (rows - nfree).to(torch.int32)
        with self._stack(model, t, y, weights, kw, bins) as (fcn, jac, ctx, _):
            jac = jac if kw.analytic else None
            if pmap is None:
                return self.profile_batch_device(fcn, jac, ctx, m, x, sigma, prof, dof, kw.stat is None, kw.lower, kw.upper, kw.opts)
            free = torch.from_numpy(pmap.tables()[4][:nfree].astype("int64")).to(dev)
            cut = lambda b: None if b is None else np.asarray(b, dtype=np.float64)[free.cpu().numpy()]
            mfcn, mjac, mctx = self.pmap_launchers(pmap, fcn, jac, ctx, x)
            try:
                lo_f, hi_f, fl_f, nev_f = self.profile_batch_device(mfcn, mjac, mctx, m, self.pmap_gather(pmap, x), sigma[:, free].contiguous(),
                                                                    prof, dof, kw.stat is None, cut(kw.lower), cut(kw.upper), kw.opts)
            finally:
                mctx.close()
            lo, hi = (torch.full((nprob, n), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
            flags = torch.full((nprob, n, 2), _lib.PROFILE_NOT_FREE, dtype=torch.int32, device=dev)
            nev = torch.zeros((nprob, n, 2), dtype=torch.int32, device=dev)
            lo[:, free], hi[:, free], flags[:, free], nev[:, free] = lo_f, hi_f, fl_f, nev_f
            return lo, hi, flags, nev

    def curve_profile_batch(self, kind, t, y, x, sigma, prof, ncomp=1, baseline=-1, weights=None, lower=None, upper=None, analytic=True,
                            opts=None, pmap=None, loss=None, stat=None, conv=None, bins=None, sep=None, group=None, starts=None):
        """The profile-likelihood intervals (a Profile) of curve_fit_batch's fit x with its standard errors sigma [nprob, n] of the
        data t, y: (lo, hi [nprob, n], flags, nev [nprob, n, 2] int32), as profile_batch_device returns them, on the launchers
        the fit itself ran on -- the caller's weights, bounds, loss, stat and conv.  Every parameter in turn is held at trial
        values while all the others are refitted; the interval ends where the cost has risen by crit * chi2 (least squares:
        scaled, dof the rows with non-zero weight minus the free parameters) or by crit (stat=Poisson(): the deviance).  No data
        are replicated: all 2 n ends of all problems refit against the nprob data sets.  pmap: the ends are those of the free
        parameters; lo and hi are NaN with flag PROFILE_NOT_FREE at fixed and tied positions, whose values x holds.  bins (a
        Binned): as in curve_fit_batch, with t=None.  sep=, group= and starts= raise ValueError."""
        return self._profile_fit(self._curve_model(kind, ncomp, baseline), t, y, x, sigma, prof, weights,
                                 _Keywords(lower, upper, analytic, False, opts, pmap, loss, stat, group, conv, sep), bins, starts)

    def expr_profile_batch(self, expr, t, y, x, sigma, prof, weights=None, lower=None, upper=None, analytic=True, opts=None, pmap=None,
                           loss=None, stat=None, conv=None, bins=None, sep=None, group=None, starts=None):
        """curve_profile_batch with an Expr in the place of (kind, ncomp, baseline): the profile of expr_fit_batch's fit x."""
        return self._profile_fit(self._expr_model(expr), t, y, x, sigma, prof, weights,
                                 _Keywords(lower, upper, analytic, False, opts, pmap, loss, stat, group, conv, sep), bins, starts)

    # -- global fits ---------------------------------------------------------------
    def group_launchers(self, group, fcn, jac, ctx):
        """Parameters shared across data sets for any launcher pair: wraps (fcn, jac, ctx) -- of curve_launchers,
        expr_launchers, loss_launchers, pois_launchers, pmap_launchers or a user's own, over nprob = ngroup * group.nsets
        problems of m rows -- in the group's launchers (nlh_group_wrap) and returns (fcn, jac, ctx) for lm_solve_batch_device,
        cls_solve_batch_device, lm_covariance_batch_device and fd_jacobian_device, which then work on x [ngroup, group.nouter]
        with m = group.nsets * m rows: y, weights and fvec [nprob, m] are [ngroup, nsets * m] as they stand.  jac is None
        without an inner Jacobian launcher (pass jac=None to the solver: forward differences over the outer unknowns).  Keep
        the returned ctx alive while solving; ctx.close() frees it (so does garbage collection)."""
        return self._wrap("group", (group, fcn, jac, ctx), fcn, jac, ctx, (group.ptr,))

    def group_gather(self, group, full):
        """The outer unknowns x [ngroup, nouter] of per-data-set parameters [ngroup * nsets, nparams] (nlh_group_gather_batch):
        a shared parameter takes the value of the group's data set 0."""
        nprob = full.shape[0]
        _chk(full, (nprob, group.nparams), "full")
        if nprob % group.nsets:
            raise ValueError(f"full has {nprob} rows: no multiple of the group's {group.nsets} data sets")
        ngroup = nprob // group.nsets
        x = torch.empty((ngroup, group.nouter), dtype=torch.float64, device=full.device)
        self._call("nlh_group_gather_batch", group.ptr, ngroup, full.data_ptr(), x.data_ptr())
        return x

    def group_expand(self, group, x):
        """The per-data-set parameters [ngroup * nsets, nparams] of the outer unknowns x [ngroup, nouter] (nlh_group_expand_batch)."""
        ngroup = x.shape[0]
        _chk(x, (ngroup, group.nouter), "x")
        p = torch.empty((ngroup * group.nsets, group.nparams), dtype=torch.float64, device=x.device)
        self._call("nlh_group_expand_batch", group.ptr, ngroup, x.data_ptr(), p.data_ptr())
        return p

    def group_sigma(self, group, sigma, fail=None):
        """The per-data-set standard errors [ngroup * nsets, nparams] of those of the outer unknowns [ngroup, nouter]
        (nlh_group_sigma_batch); fail: int32 [ngroup], non-zero for a group that did not solve (NaN everywhere)."""
        ngroup = sigma.shape[0]
        _chk(sigma, (ngroup, group.nouter), "sigma")
        sf = torch.empty((ngroup * group.nsets, group.nparams), dtype=torch.float64, device=sigma.device)
        self._call("nlh_group_sigma_batch", group.ptr, ngroup, sigma.data_ptr(), fail.data_ptr() if fail is not None else None,
                   sf.data_ptr())
        return sf

    # -- robust losses -------------------------------------------------------------
    def _loss_scale(self, loss, nprob, dev=None):
        """(device tensor of the scales of a Loss for nprob problems, shared flag)."""
        sc, sh = loss.scale_for(nprob)
        return torch.from_numpy(sc).to(dev if dev is not None else self.device), sh

    def loss_launchers(self, loss, fcn, jac, ctx, nprob=None):
        """A robust loss for any launcher pair: wraps (fcn, jac, ctx) -- of curve_launchers, expr_launchers, dq_launchers,
        pmap_launchers or a user's own -- in the loss's launchers (nlh_loss_wrap) and returns (fcn, jac, ctx) for
        lm_solve_batch_device, cls_solve_batch_device, lm_covariance_batch_device, fd_jacobian_device and pmap_launchers.
        A Loss with one scale per problem fixes the number of problems (nprob, when given, is checked against it).  jac is
        None without an inner Jacobian launcher (pass jac=None to the solver: forward differences of the wrapped residual).
        Keep the returned ctx alive while solving; ctx.close() frees it (so does garbage collection)."""
        dscale, sh = self._loss_scale(loss, len(loss.scale) if nprob is None or loss.shared else nprob)
        return self._wrap("loss", (loss, fcn, jac, ctx, dscale), fcn, jac, ctx, (loss.kind, dscale.data_ptr(), sh))

    def loss_apply(self, loss, r):
        """(out, g, wgt) of raw residuals r [nprob, m] under a Loss (nlh_loss_apply_batch): the transformed residual rho~, the
        row factor of the Jacobian, and the weight rho' -- 1.0 for a residual the loss leaves alone, towards 0.0 for an
        outlier: threshold it to flag outliers."""
        nprob, m = r.shape
        _chk(r, (nprob, m), "r")
        dscale, sh = self._loss_scale(loss, nprob, r.device)
        out, g, wgt = (torch.empty_like(r) for _ in range(3))
        self._call("nlh_loss_apply_batch", loss.kind, nprob, m, dscale.data_ptr(), sh, r.data_ptr(), out.data_ptr(),
                   g.data_ptr(), wgt.data_ptr())
        return out, g, wgt

    # -- Poisson likelihood fits ---------------------------------------------------
    def pois_launchers(self, stat, fcn, jac, ctx, y, weights=None):
        """The Poisson deviance for any launcher pair: wraps (fcn, jac, ctx) -- of curve_launchers or expr_launchers made
        WITHOUT weights on the same counts y [nprob, m], or a user's own whose residual is model - y -- in the Poisson
        launchers (nlh_pois_wrap) and returns (fcn, jac, ctx) for lm_solve_batch_device, cls_solve_batch_device,
        lm_covariance_batch_device (scaled=False: the inverse Fisher information), fd_jacobian_device and pmap_launchers.
        weights: the 0 / 1 mask [nprob, m] of the rows, or None.  jac is None without an inner Jacobian launcher (pass jac=None
        to the solver: forward differences of the wrapped residual).  Keep the returned ctx alive while solving; ctx.close()
        frees it (so does garbage collection)."""
        nprob, m = y.shape
        _chk(y, (nprob, m), "y")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        return self._wrap("pois", (stat, fcn, jac, ctx, y, weights), fcn, jac, ctx,
                          (y.data_ptr(), weights.data_ptr() if weights is not None else None, stat.mu_floor))

    def pois_apply(self, stat, r, y, weights=None):
        """(out, g, dev) of raw residuals r = model - y [nprob, m] for counts y under a Poisson (nlh_pois_apply_batch): the
        deviance residual, the row factor of the Jacobian, and the row's deviance (0.0 on a masked row)."""
        nprob, m = r.shape
        _chk(r, (nprob, m), "r"); _chk(y, (nprob, m), "y")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        out, g, dev = (torch.empty_like(r) for _ in range(3))
        self._call("nlh_pois_apply_batch", nprob, m, y.data_ptr(), weights.data_ptr() if weights is not None else None,
                   stat.mu_floor, r.data_ptr(), out.data_ptr(), g.data_ptr(), dev.data_ptr())
        return out, g, dev

    # -- instrument-response fits ---------------------------------------------------
    def _conv_struct(self, conv, nprob, dev=None):
        """(nlh_conv of a Convolve for nprob problems, the device tensor of its taps: keep it alive)."""
        k, _ = conv.kernel_for(nprob)
        dk = torch.from_numpy(np.ascontiguousarray(k)).to(dev if dev is not None else self.device)
        return conv.struct(dk.data_ptr()), dk

    def conv_launchers(self, conv, fcn, jac, ctx, y, weights=None):
        """An instrument response for any launcher pair: wraps (fcn, jac, ctx) -- of curve_launchers or expr_launchers made
        WITHOUT weights on the same data y [nprob, m], or a user's own whose residual is model - y -- in the convolving
        launchers (nlh_conv_wrap) and returns (fcn, jac, ctx) for lm_solve_batch_device, cls_solve_batch_device,
        lm_covariance_batch_device, fd_jacobian_device, loss_launchers, pois_launchers, pmap_launchers and group_launchers:
        the residual is conv(model) - y, times weights [nprob, m] when given.  jac is None without an inner Jacobian launcher
        (pass jac=None to the solver: forward differences of the wrapped residual).  Keep the returned ctx alive while
        solving; ctx.close() frees it (so does garbage collection)."""
        nprob, m = y.shape
        _chk(y, (nprob, m), "y")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        cv, dk = self._conv_struct(conv, nprob, y.device)
        return self._wrap("conv", (conv, dk, fcn, jac, ctx, y, weights), fcn, jac, ctx,
                          (C.byref(cv), y.data_ptr(), weights.data_ptr() if weights is not None else None))

    def conv_apply(self, conv, v):
        """The bare convolution of columns v [nprob, m] or [nprob, ncol, m] under a Convolve (nlh_conv_apply_batch), e.g. of
        curve_eval's model values for plotting the convolved model.  Returns a new tensor of v's shape."""
        if v.dim() not in (2, 3):
            raise ValueError("v: expected [nprob, m] or [nprob, ncol, m]")
        nprob, m = v.shape[0], v.shape[-1]
        ncol = v.shape[1] if v.dim() == 3 else 1
        _chk(v, v.shape, "v")
        cv, dk = self._conv_struct(conv, nprob, v.device)
        out = torch.empty_like(v)
        self._call("nlh_conv_apply_batch", C.byref(cv), nprob, m, ncol, v.data_ptr(), out.data_ptr())
        torch.cuda.current_stream(v.device).synchronize()             # (dk goes with this frame)
        return out

    # -- bin-integrated fits ----------------------------------------------------------
    def _bin_struct(self, bins, nprob, dev=None):
        """(nlh_bin of a Binned for nprob problems, the device tensor of its scale or None: keep it alive)."""
        sc, sh = bins.scale_for(nprob)
        dsc = None if sc is None else torch.from_numpy(np.ascontiguousarray(sc)).to(dev if dev is not None else self.device)
        return bins.struct(dsc.data_ptr() if dsc is not None else None, sh), dsc

    def bin_nodes(self, bins, nprob, dev=None):
        """bins.nodes() for a call on nprob problems as a device tensor: the abscissae to bind the inner model on."""
        return torch.from_numpy(np.ascontiguousarray(bins.nodes_for(nprob))).to(dev if dev is not None else self.device)

    def bin_launchers(self, bins, fcn, jac, ctx, y, weights=None):
        """The bins of a histogram or the pixels of an image for any launcher pair (a Binned): wraps (fcn, jac, ctx) -- of
        curve_launchers or expr_launchers made on bin_nodes(bins, nprob) with a ZERO y [nprob, Q m] and WITHOUT weights, or a
        user's own that returns model values on those rows -- in the bin-summing launchers (nlh_bin_wrap) and returns
        (fcn, jac, ctx) for lm_solve_batch_device, cls_solve_batch_device, lm_covariance_batch_device, fd_jacobian_device,
        conv_launchers, loss_launchers, pois_launchers, pmap_launchers and group_launchers, which then work on the m = bins.m
        bins: the residual is the rule's sum over every bin minus y [nprob, m], times weights [nprob, m] when given.  jac is
        None without an inner Jacobian launcher (pass jac=None to the solver: forward differences of the wrapped residual).
        Keep the returned ctx alive while solving; ctx.close() frees it (so does garbage collection)."""
        nprob, m = y.shape
        _chk(y, (nprob, m), "y")
        if m != bins.m:
            raise ValueError(f"y has {m} columns, the Binned {bins.m} bins")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
        bn, dsc = self._bin_struct(bins, nprob, y.device)
        return self._wrap("bin", (bins, dsc, fcn, jac, ctx, y, weights), fcn, jac, ctx,
                          (C.byref(bn), y.data_ptr(), weights.data_ptr() if weights is not None else None))

    def bin_apply(self, bins, v):
        """The bare sum over the bins of columns v [nprob, Q m] or [nprob, ncol, Q m] under a Binned (nlh_bin_apply_batch), e.g. of
        curve_eval's model values at bin_nodes for plotting the binned model.  Returns a new tensor [nprob, m] or
        [nprob, ncol, m]."""
        if v.dim() not in (2, 3):
            raise ValueError("v: expected [nprob, Q m] or [nprob, ncol, Q m]")
        nprob = v.shape[0]
        ncol = v.shape[1] if v.dim() == 3 else 1
        _chk(v, tuple(v.shape[:-1]) + (bins.Q * bins.m,), "v")
        bn, dsc = self._bin_struct(bins, nprob, v.device)
        out = torch.empty(tuple(v.shape[:-1]) + (bins.m,), dtype=torch.float64, device=v.device)
        self._call("nlh_bin_apply_batch", C.byref(bn), nprob, bins.m, ncol, v.data_ptr(), out.data_ptr())
        torch.cuda.current_stream(v.device).synchronize()             # (dsc goes with this frame)
        return out

    def _bin_fit(self, model, t, y, weights, x0, bins, kw):
        """A one-call fit with bins=: the solve and the covariance on the launcher stack of the fit (_stack, with the bin pair
        in it), and the zero-weight rule of the header where there are weights."""
        if x0 is None:
            raise ValueError("bins excludes x0=None: there is no guess on binned data; compose bin_launchers and call starts_search")
        if t is not None:
            raise ValueError("bins excludes t: the model is evaluated at bins.nodes(); pass t=None")
        if bins.nvar != model.nvar:
            raise ValueError(f"bins are over {bins.nvar} variable(s), the model has {model.nvar}")
        (nprob, m), n = y.shape, model.n
        _chk(y, (nprob, m), "y")
        _chk(x0, (nprob, n), "x0")
        if weights is not None:
            _chk(weights, (nprob, m), "weights")
            dof = (weights != 0).sum(dim=1) - n
            if bool((dof <= 0).any()):
                raise ValueError("bins: a problem has no degree of freedom left (rows with non-zero weight <= parameters)")
        with self._stack(model, None, y, weights, kw, bins) as (fcn, jac, ctx, _):
            jac = jac if kw.analytic else None
            x = x0.clone()
            o = kw.opts or self.options()
            if kw.lower is not None or kw.upper is not None:
                fvec, ibs, status = self.cls_solve_batch_device(fcn, ctx, m, x, jac=jac, opts=o, lower=kw.lower, upper=kw.upper)
            else:
                fvec, ibs, status = self.lm_solve_batch_device(fcn, ctx, m, x, jac=jac, opts=o)
            sigma = cov = chi2 = rank = None
            if kw.covariance:
                cov, sigma, rank, chi2 = self.lm_covariance_batch_device(fcn, ctx, m, x, jac=jac, scaled=kw.stat is None)
                if weights is not None:                              # the header's zero-weight rule, in torch
                    f = float(m - n) / dof.to(torch.float64)
                    chi2 = chi2 * f
                    if kw.stat is None:
                        cov = cov * f[:, None, None]
                        sigma = torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2)).contiguous()
                bad = torch.tensor([s != 0 for s in status], dtype=torch.bool, device=y.device)
                nan = float("nan")
                sigma, cov, chi2 = sigma.masked_fill(bad[:, None], nan), cov.masked_fill(bad[:, None, None], nan), chi2.masked_fill(bad, nan)
                rank = rank.masked_fill(bad, -1)
        return x, fvec, sigma, cov, chi2, rank, ibs, status

    # -- separable fits (variable projection) --------------------------------------
    def sep_launchers(self, sep, fcn, jac, ctx):
        """Wraps any inner launcher pair (fcn, jac, ctx) -- curve_launchers, expr_launchers, conv_launchers or a user's own,
        over sep.nparams parameters -- in the projecting launchers (nlh_sep_wrap) and returns (fcn, jac, ctx) for
        lm_solve_batch_device, cls_solve_batch_device, fd_jacobian_device and group_launchers over the sep.nnonlin nonlinear
        unknowns; the linear parameters are solved for at every point.  The inner jac is required (its linear columns are the
        basis); pass jac=None to the solver for a forward-difference outer Jacobian.  Keep the returned ctx alive while
        solving; ctx.close() frees its scratch."""
        if jac is None:
            raise ValueError("sep_launchers: the inner Jacobian launcher is required (its linear columns are the basis)")
        return self._wrap("sep", (sep, fcn, jac, ctx), fcn, jac, ctx, (sep.ptr,))

    def sep_gather(self, sep, full):
        """The nonlinear unknowns alpha [nprob, nnonlin] of full parameters [nprob, nparams] (nlh_sep_gather_batch)."""
        nprob = full.shape[0]
        _chk(full, (nprob, sep.nparams), "full")
        x = torch.empty((nprob, sep.nnonlin), dtype=torch.float64, device=full.device)
        self._call("nlh_sep_gather_batch", sep.ptr, nprob, full.data_ptr(), x.data_ptr())
        return x

    def sep_solve(self, sep_ctx, m, alpha):
        """(full, rank): the full parameters (c(alpha), alpha) [nprob, nparams] of the nonlinear unknowns alpha [nprob, nnonlin]
        of problems 0 .. nprob-1 of m rows, and the live columns of each basis (nlh_sep_solve_batch).  sep_ctx: the context
        sep_launchers returned."""
        sep = sep_ctx._keep[0]
        nprob = alpha.shape[0]
        _chk(alpha, (nprob, sep.nnonlin), "alpha")
        full = torch.empty((nprob, sep.nparams), dtype=torch.float64, device=alpha.device)
        rank = torch.empty((nprob,), dtype=torch.int32, device=alpha.device)
        self._call("nlh_sep_solve_batch", sep_ctx.ptr, nprob, int(m), alpha.data_ptr(), full.data_ptr(), rank.data_ptr())
        return full, rank

    def sep_check(self, sep, fcn, jac, ctx, m, full):
        """How far the inner model is from affine in the parameters sep declares linear, at the full parameters
        full [nprob, nparams]: the inner Jacobian is evaluated there and with every linear parameter c replaced by 2 c + 1;
        returns the largest difference of a linear column between the two, relative to the largest entry of the linear
        columns.  0.0: the declaration holds at these points."""
        lin = torch.from_numpy(sep.tables()[0].astype("int64")).to(full.device)
        other = full.clone()
        other[:, lin] = 2.0 * full[:, lin] + 1.0
        J1 = self.fd_jacobian_device(fcn, ctx, m, full, jac=jac)[:, lin]
        J2 = self.fd_jacobian_device(fcn, ctx, m, other, jac=jac)[:, lin]
        scale = float(torch.max(torch.abs(J1)))
        return float(torch.max(torch.abs(J1 - J2))) / scale if scale > 0.0 else float(torch.max(torch.abs(J2)))

    def _ctxp(self, ctx):
        if isinstance(ctx, _Wrapped):
            return ctx.ptr
        return ctx if isinstance(ctx, (int, C.c_void_p)) or ctx is None else C.cast(C.byref(ctx), C.c_void_p)

    def _wrap(self, kind, keep, fcn, jac, ctx, before, after=()):
        """The tail of every *_launchers: nlh_<kind>_wrap around the inner (fcn, jac, ctx), its other arguments before and
        after them, then (fcn, jac -- None without an inner one --, ctx) of the wrapping launchers; ctx owns what the wrap
        made and keeps `keep` alive."""
        out = C.c_void_p()
        self._call(f"nlh_{kind}_wrap", *before, self._devfcn(fcn), self._devfcn(jac), self._ctxp(ctx), *after, C.byref(out))
        launcher = lambda f: C.cast(getattr(self.lib, f"nlh_{kind}_device_{f}"), _lib.DEVFCN)
        return (launcher("fcn"), launcher("jac") if jac is not None else None,
                _Wrapped(self.lib, out, keep, f"nlh_{kind}_unwrap"))

    @contextlib.contextmanager
    def _stack(self, model, t, y, weights, kw, bins=None):
        """The launchers of a one-call fit, composed in the order of the library's own pipeline: the model's pair -- under
        bins on bin_nodes with a zero y --, then bin_launchers, conv_launchers, pois_launchers, loss_launchers and
        sep_launchers for what is given.  The weights go to the Poisson pair if there is one, else to the conv pair, else to
        the bin pair, else to the model; the layers inside get None.  Yields (fcn, jac, ctx, positions) of the outermost pair,
        positions the nonlinear unknowns with sep (None without); on the way out every wrapped context is closed, the
        outermost first."""
        nprob = y.shape[0]
        taker = "pois" if kw.stat is not None else "conv" if kw.conv is not None else "bin" if bins is not None else "model"
        w = lambda layer: weights if layer == taker else None
        if bins is not None:
            t, y0 = self.bin_nodes(bins, nprob, y.device), torch.zeros((nprob, bins.Q * bins.m), dtype=torch.float64, device=y.device)
        with contextlib.ExitStack() as made:
            def wrapped(pair):
                made.callback(pair[2].close)
                return pair
            pair = model.launchers(t, y if bins is None else y0, w("model"))
            if bins is not None:
                pair = wrapped(self.bin_launchers(bins, *pair, y, w("bin")))
            if kw.conv is not None:
                pair = wrapped(self.conv_launchers(kw.conv, *pair, y, w("conv")))
            if kw.stat is not None:
                pair = wrapped(self.pois_launchers(kw.stat, *pair, y, w("pois")))
            if kw.loss is not None:
                pair = wrapped(self.loss_launchers(kw.loss, *pair, nprob))
            positions = None
            if kw.sep is not None:
                pair = wrapped(self.sep_launchers(kw.sep, *pair))
                positions = [int(k) for k in kw.sep.tables()[1]]
            yield pair + (positions,)

    def lm_solve_batch_device(self, fcn, ctx, m, x, jac=None, opts=None):
        """least_squares_solver%solve on x.shape[0] problems of a USER'S device residual (launcher fcn, context ctx).
        x [nprob, n] is updated in place.  Returns (fvec, ib_list, status_list)."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        fvec = torch.empty((nprob, m), dtype=torch.float64, device=x.device)
        ib, status = _ib_status(nprob)
        o = opts or self.options()
        self._call("nlh_lm_solve_batch_device", C.byref(o), nprob, m, n, self._devfcn(fcn), self._devfcn(jac),
                   self._ctxp(ctx), x.data_ptr(), fvec.data_ptr(), ib, status)
        return (fvec,) + _ib_lists(ib, status)

    def cls_solve_batch_device(self, fcn, ctx, m, x, jac=None, opts=None, lower=None, upper=None, delta=1.0, stepscale=1.0):
        """constrained_least_squares_solver%solve on x.shape[0] problems of a user's device residual (the same box for all)."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        fvec = torch.empty((nprob, m), dtype=torch.float64, device=x.device)
        ib, status = _ib_status(nprob)
        o = opts or self.options()
        plo, phi = _host_bounds(lower, upper)
        self._call("nlh_cls_solve_batch_device", C.byref(o), float(delta), float(stepscale), plo, phi, nprob, m, n,
                   self._devfcn(fcn), self._devfcn(jac), self._ctxp(ctx), x.data_ptr(), fvec.data_ptr(), ib, status)
        return (fvec,) + _ib_lists(ib, status)

    def square_solve_batch_device(self, fcn, ctx, x, jac=None, opts=None, broyden=False, jdelta=5):
        """newton_solver%solve (or quasi_newton_solver%solve) on x.shape[0] square problems of a user's device residual."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        fvec = torch.empty((nprob, n), dtype=torch.float64, device=x.device)
        ib, status = _ib_status(nprob)
        o = opts or self.options()
        tail = (nprob, n, self._devfcn(fcn), self._devfcn(jac), self._ctxp(ctx), x.data_ptr(), fvec.data_ptr(), ib, status)
        if broyden:
            self._call("nlh_quasi_newton_solve_batch_device", C.byref(o), int(jdelta), *tail)
        else:
            self._call("nlh_newton_solve_batch_device", C.byref(o), *tail)
        return (fvec,) + _ib_lists(ib, status)

    def bfgs_solve_batch_device(self, fcn, ctx, x, grad=None, opts=None):
        """bfgs%solve for every problem with the USER'S device fcnnvar: fcn a launcher called with m = 1 (dF[npoints] = f),
        grad (optional) one that fills dJ[npoints][n] with the gradients.  x [nprob][n] device tensor, in place.
        Returns (fout list, ib list, status list)."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        ib, status = _ib_status(nprob)
        fout = (C.c_double * nprob)()
        o = opts or self.options(max_evals=500)
        self._call("nlh_bfgs_solve_batch_device", C.byref(o), nprob, n, self._devfcn(fcn), self._devfcn(grad), self._ctxp(ctx),
                   x.data_ptr(), fout, ib, status)
        return ([float(v) for v in fout],) + _ib_lists(ib, status)

    def nelder_mead_solve_batch_device(self, fcn, ctx, x, simplex=None, init_size=1.0, opts=None):
        """nelder_mead%solve for every problem with the USER'S device fcnnvar (fcn a launcher called with m = 1).  x [nprob][n]
        device tensor, in place (the best vertex on convergence, untouched after max evaluations).  simplex: None (built
        from x and init_size) or a [nprob][n+1][n] device tensor to start from (x ignored), updated in place to the final
        simplex.  Returns (fout list, ib list, status list)."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        if simplex is not None:
            _chk(simplex, (nprob, n + 1, n), "simplex")
        ib, status = _ib_status(nprob)
        fout = (C.c_double * nprob)()
        o = opts or self.options(max_evals=500)
        self._call("nlh_nelder_mead_solve_batch_device", C.byref(o), float(init_size), nprob, n, self._devfcn(fcn),
                   self._ctxp(ctx), x.data_ptr(), simplex.data_ptr() if simplex is not None else None,
                   0 if simplex is None else 1, fout, ib, status)
        return ([float(v) for v in fout],) + _ib_lists(ib, status)

    def _root1v_batch(self, entry, fcns, ctx, lim, x, opts):
        nprob = x.shape[0]
        _chk(lim, (nprob, 2), "lim")
        _chk(x, (nprob,), "x")
        ibc = (_lib.IterationBehavior * nprob)()
        ib = np.frombuffer(ibc, dtype=IB_DTYPE)             # a structured view on the ctypes buffer
        status = np.zeros(nprob, dtype=np.int32)
        fout = np.zeros(nprob, dtype=np.float64)
        o = opts or self.options()
        self._call(entry, C.byref(o), nprob, *[self._devfcn(f) for f in fcns], self._ctxp(ctx), lim.data_ptr(), x.data_ptr(),
                   fout.ctypes.data_as(_lib.c_double_p), ibc, status.ctypes.data_as(_lib.c_int32_p))
        return fout, status, ib

    def brent_solve_batch_device(self, fcn, ctx, lim, x, opts=None):
        """brent_solver%solve for every problem with the USER'S device fcn1var (fcn: a launcher called with n = m = 1).
        lim [nprob, 2] and x [nprob]: float64 device tensors; x is written in place (0 unless the problem converged).
        Returns numpy arrays (fout float64, status int32, ib: a structured array of the iteration_behavior fields)."""
        return self._root1v_batch("nlh_brent_solve_batch_device", (fcn,), ctx, lim, x, opts)

    def newton_1var_solve_batch_device(self, fcn, ctx, lim, x, diff=None, opts=None):
        """newton_1var_solver%solve (with f present) for every problem: diff, the user's derivative launcher (n = m = 1),
        or None for forward differences.  As brent_solve_batch_device."""
        return self._root1v_batch("nlh_newton_1var_solve_batch_device", (fcn, diff), ctx, lim, x, opts)

    def fd_jacobian_device(self, fcn, ctx, m, x, fv=None, jac=None):
        """vecfcn_helper%jacobian of every problem of a user's device residual: J [nprob, n, m]."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        J = torch.empty((nprob, n, m), dtype=torch.float64, device=x.device)
        self._call("nlh_fd_jacobian_device", nprob, m, n, self._devfcn(fcn), self._devfcn(jac), self._ctxp(ctx),
                   x.data_ptr(), fv.data_ptr() if fv is not None else None, J.data_ptr())
        return J

    # -- stage-level kernels (parity tests, roofline) --------------------------
    def residual(self, A, b, gamma, x):
        nprob, n, m = A.shape
        f = torch.empty((nprob, m), dtype=torch.float64, device=A.device)
        self.h.check(self.lib.nlh_dq_residual(self.h.ptr, nprob, m, n, A.data_ptr(), b.data_ptr(), float(gamma),
                                              x.data_ptr(), f.data_ptr()), "nlh_dq_residual")
        return f

    def fd_panel(self, A, b, gamma, x):
        nprob, n, m = A.shape
        P = torch.empty((nprob, n, m), dtype=torch.float64, device=A.device)
        self.h.check(self.lib.nlh_dq_fd_panel(self.h.ptr, nprob, m, n, A.data_ptr(), b.data_ptr(), float(gamma),
                                              x.data_ptr(), P.data_ptr()), "nlh_dq_fd_panel")
        return P

    def fd_jacobian_panel(self, P, f0, x, out=None):
        nprob, n, m = P.shape
        J = out if out is not None else torch.empty_like(P)
        self.h.check(self.lib.nlh_fd_jacobian_panel(self.h.ptr, nprob, m, n, P.data_ptr(), f0.data_ptr(),
                                                    x.data_ptr(), J.data_ptr()), "nlh_fd_jacobian_panel")
        return J

    def jacobian(self, A, gamma, x):
        nprob, n, m = A.shape
        J = torch.empty_like(A)
        self.h.check(self.lib.nlh_dq_jacobian(self.h.ptr, nprob, m, n, A.data_ptr(), float(gamma), x.data_ptr(),
                                              J.data_ptr()), "nlh_dq_jacobian")
        return J

    def gram(self, J, f):
        nprob, n, m = J.shape
        G = torch.empty((nprob, n, n), dtype=torch.float64, device=J.device)
        g = torch.empty((nprob, n), dtype=torch.float64, device=J.device)
        self.h.check(self.lib.nlh_gram(self.h.ptr, nprob, m, n, J.data_ptr(), f.data_ptr(), G.data_ptr(),
                                       g.data_ptr()), "nlh_gram")
        return G, g

    def chol_factor(self, G, g):
        """Overwrites G's upper triangle (G[p, c, r], r <= c) with R.  Returns (ipvt0, acnorm, qtf, info)."""
        nprob, n, _ = G.shape
        dev = G.device
        ipvt = torch.empty((nprob, n), dtype=torch.int32, device=dev)
        acnorm = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        qtf = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        info = torch.empty((nprob,), dtype=torch.int32, device=dev)
        self.h.check(self.lib.nlh_chol_factor(self.h.ptr, nprob, n, G.data_ptr(), g.data_ptr(), ipvt.data_ptr(),
                                              acnorm.data_ptr(), qtf.data_ptr(), info.data_ptr()), "nlh_chol_factor")
        return ipvt, acnorm, qtf, info

    def chol_natural(self, G, g, pivot_tol=0.0, form=0):
        """The natural-order blocked Cholesky of the normal-equations policy on G [nprob, n, n], g [nprob, n] (neither is
        modified).  form 0: one workgroup per problem, form 1: the multi-CU launches.  Returns (R, ipvt0, acnorm, qtf,
        info): R[p, c, r], r <= c, is R(r, c), the strict lower triangle is G's; info[p] is 0 or the 1-based index of
        the first bad pivot."""
        nprob, n, _ = G.shape
        _chk(G, (nprob, n, n), "G"); _chk(g, (nprob, n), "g")
        dev = G.device
        R = torch.empty_like(G)
        ipvt = torch.empty((nprob, n), dtype=torch.int32, device=dev)
        acnorm = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        qtf = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        info = torch.empty((nprob,), dtype=torch.int32, device=dev)
        self.h.check(self.lib.nlh_chol_natural(self.h.ptr, nprob, n, G.data_ptr(), g.data_ptr(), float(pivot_tol), int(form),
                                               R.data_ptr(), ipvt.data_ptr(), acnorm.data_ptr(), qtf.data_ptr(),
                                               info.data_ptr()), "nlh_chol_natural")
        return R, ipvt, acnorm, qtf, info

    def ne_signs(self, J, ipvt, R, qtf):
        """lmfactor's row signs for the pivoted Cholesky factors of J^T J (chol_factor's ipvt0, R in G's upper triangle and
        qtf): R and qtf are signed in place.  J [nprob, n, m], m >= n.  Returns the signs [nprob, n] (+-1)."""
        nprob, n, m = J.shape
        _chk(J, (nprob, n, m), "J"); _chk(R, (nprob, n, n), "R"); _chk(qtf, (nprob, n), "qtf")
        sign = torch.empty((nprob, n), dtype=torch.float64, device=J.device)
        self.h.check(self.lib.nlh_ne_signs(self.h.ptr, nprob, m, n, J.data_ptr(), ipvt.data_ptr(), R.data_ptr(),
                                           qtf.data_ptr(), sign.data_ptr()), "nlh_ne_signs")
        return sign

    def qr_factor(self, J, f):
        """lmfactor + Q^T f.  J [nprob, n, m] is overwritten.  Returns (ipvt0, rdiag, acnorm, qtf, wa4)."""
        nprob, n, m = J.shape
        dev = J.device
        ipvt = torch.empty((nprob, n), dtype=torch.int32, device=dev)
        rdiag = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        acnorm = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        qtf = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        wa4 = torch.empty((nprob, m), dtype=torch.float64, device=dev)
        self.h.check(self.lib.nlh_qr_factor(self.h.ptr, nprob, m, n, J.data_ptr(), f.data_ptr(), ipvt.data_ptr(),
                                            rdiag.data_ptr(), acnorm.data_ptr(), qtf.data_ptr(), wa4.data_ptr()),
                     "nlh_qr_factor")
        return ipvt, rdiag, acnorm, qtf, wa4

    def lmfactor_exact(self, J, f):
        """lmfactor + Q^T f in the reference's operation order (the exact LM policy's factorisation, bit-identical to
        the CPU path).  J [nprob, n, m] (column-major problems, not modified), f [nprob, m], m >= n.
        Returns (R [nprob, n, n] column-major: R[p].T is R with rdiag on the diagonal, ipvt0, rdiag, acnorm, qtf, wa4)."""
        nprob, n, m = J.shape
        _chk(J, (nprob, n, m), "J"); _chk(f, (nprob, m), "f")
        dev = J.device
        R = torch.zeros((nprob, n, n), dtype=torch.float64, device=dev)
        ipvt = torch.empty((nprob, n), dtype=torch.int32, device=dev)
        rdiag = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        acnorm = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        qtf = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        wa4 = torch.empty((nprob, m), dtype=torch.float64, device=dev)
        self.h.check(self.lib.nlh_lmfactor_exact(self.h.ptr, nprob, m, n, J.data_ptr(), f.data_ptr(), R.data_ptr(),
                                                 ipvt.data_ptr(), rdiag.data_ptr(), acnorm.data_ptr(), qtf.data_ptr(),
                                                 wa4.data_ptr()), "nlh_lmfactor_exact")
        return R, ipvt, rdiag, acnorm, qtf, wa4

    def qrx_second_matrix_bytes(self):
        """Bytes this solver's handle (sub-batch workers included) holds for second copies of the exact factorisation's
        working matrix (nlh_qrx_second_matrix_bytes): 0 until an out-of-place flush wanted one and the device had room."""
        return int(self.lib.nlh_qrx_second_matrix_bytes(self.h.ptr))

    def lmpar(self, R, ipvt, diag, qtf, delta, tailsq, par):
        """R [nprob, n, ldr] column-major n-by-n blocks with leading dimension ldr."""
        nprob, n, ldr = R.shape
        dev = R.device
        for t, nm in ((R, "R"), (diag, "diag"), (qtf, "qtf"), (delta, "delta"), (tailsq, "tailsq"), (par, "par")):
            if t.dtype != torch.float64 or not t.is_cuda:
                raise ValueError(f"{nm} must be a float64 GPU tensor")
        x = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        sdiag = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        par = par.clone()
        self.h.check(self.lib.nlh_lmpar(self.h.ptr, nprob, n, R.data_ptr(), ldr, ipvt.data_ptr(), diag.data_ptr(),
                                        qtf.data_ptr(), delta.data_ptr(), tailsq.data_ptr(), par.data_ptr(),
                                        x.data_ptr(), sdiag.data_ptr()), "nlh_lmpar")
        return par, x, sdiag

    def lu_factor(self, A):
        nprob, n, _ = A.shape
        ipvt = torch.empty((nprob, n), dtype=torch.int32, device=A.device)
        info = torch.empty((nprob,), dtype=torch.int32, device=A.device)
        self.h.check(self.lib.nlh_lu_factor(self.h.ptr, nprob, n, A.data_ptr(), ipvt.data_ptr(), info.data_ptr()),
                     "nlh_lu_factor")
        return ipvt, info

    def qr_factor_full(self, B):
        """Householder QR with Q formed.  B: [nprob, n, n] column-major problems (B[p].T is the matrix).
        Returns (Q column-major like B, Rt = R stored row-major, i.e. Rt[p] IS R as a torch matrix)."""
        nprob, n, _ = B.shape
        _chk(B, (nprob, n, n), "B")
        Q = torch.empty_like(B)
        Rt = torch.empty_like(B)
        self._call("nlh_qr_factor_full", nprob, n, B.data_ptr(), Q.data_ptr(), Rt.data_ptr())
        return Q, Rt

    def house_steps(self, A, E):
        """The Householder steps of every QR here, in place: A [nprob, rows, ncA] and E [nprob, rows, ncE] (ncE may be 0)
        are the ROW-major work arrays, i.e. A[p] and E[p] ARE the matrices.  On return A[p] holds R (exact zeros below
        the diagonal) and E[p] = Q^T E[p].  Returns (A, E)."""
        nprob, rows, ncA = A.shape
        ncE = E.shape[2]
        _chk(A, (nprob, rows, ncA), "A"); _chk(E, (nprob, rows, ncE), "E")
        rc = self.h.check(self.lib.nlh_house_steps(self.h.ptr, nprob, rows, ncA, ncE, A.data_ptr(),
                                                   E.data_ptr() if ncE else None), "nlh_house_steps")
        if rc:
            raise ValueError(f"nlh_house_steps({nprob}, {rows}, {ncA}, {ncE}) returned {rc}")
        return A, E

    def qr_rank1_update(self, Q, Rt, u, v):
        """In place: Q1 R1 = Q R + u v^T."""
        nprob, n, _ = Q.shape
        _chk(Q, (nprob, n, n), "Q"); _chk(Rt, (nprob, n, n), "Rt"); _chk(u, (nprob, n), "u"); _chk(v, (nprob, n), "v")
        self._call("nlh_qr_rank1_update", nprob, n, Q.data_ptr(), Rt.data_ptr(), u.data_ptr(), v.data_ptr())
        return Q, Rt

    def solve_upper(self, Rt, x):
        nprob, n, _ = Rt.shape
        _chk(Rt, (nprob, n, n), "Rt"); _chk(x, (nprob, n), "x")
        self._call("nlh_solve_upper", nprob, n, Rt.data_ptr(), x.data_ptr())
        return x

    def poly_fit_batch(self, x, y, order, thru_zero=False):
        """polynomial%fit for every row of x / y ([nprob, npts]).  Returns coefficients [nprob, order + 1]."""
        nprob, npts = x.shape
        _chk(x, (nprob, npts), "x"); _chk(y, (nprob, npts), "y")
        coef = torch.empty((nprob, order + 1), dtype=torch.float64, device=x.device)
        self._call("nlh_poly_fit_batch", nprob, npts, int(order), int(thru_zero), x.data_ptr(), y.data_ptr(), coef.data_ptr())
        return coef

    def poly_roots_batch(self, coef):
        """polynomial%roots for every row of coef ([nprob, order + 1], constant first).  Returns (z complex128
        [nprob, order], info int32 [nprob]): see nlh_poly_roots_batch in include/nonlin_hip.h for the order of the roots and
        the per-row info codes.  A row's failure touches no other row and raises nothing."""
        nprob, ncoef = coef.shape
        _chk(coef, (nprob, ncoef), "coef")
        order = ncoef - 1
        z = torch.empty((nprob, order, 2), dtype=torch.float64, device=coef.device)
        info = torch.zeros((nprob,), dtype=torch.int32, device=coef.device)
        self._call("nlh_poly_roots_batch", nprob, order, coef.data_ptr(), z.data_ptr(), info.data_ptr())
        return torch.view_as_complex(z), info

    def poly_eval_batch(self, coef, x):
        """polynomial%evaluate for every row: coef [nprob, order + 1], x [nprob, npts] float64 or complex128.  Returns y
        like x."""
        nprob, ncoef = coef.shape
        _chk(coef, (nprob, ncoef), "coef")
        npts = x.shape[1]
        if x.dtype == torch.complex128:
            if tuple(x.shape) != (nprob, npts) or not x.is_contiguous() or x.device != coef.device:
                raise ValueError("x: expected a contiguous complex128 [nprob, npts] tensor on coef's device")
            y = torch.empty_like(x)
            rc = self.lib.nlh_poly_eval_complex_batch(self.h.ptr, nprob, ncoef - 1, npts, coef.data_ptr(), x.data_ptr(),
                                                      y.data_ptr())
        else:
            _chk(x, (nprob, npts), "x")
            y = torch.empty_like(x)
            rc = self.lib.nlh_poly_eval_batch(self.h.ptr, nprob, ncoef - 1, npts, coef.data_ptr(), x.data_ptr(), y.data_ptr())
        self._checked(rc, "nlh_poly_eval_batch")                     # (the complex entry reports under this name too)
        return y

    def covar(self, R, ipvt, tol=None):
        """MINPACK's covar on the pivoted factor lmfactor_exact returns: R [nprob, n, n] (column-major problems, upper
        triangle with rdiag on the diagonal, not modified), ipvt [nprob, n] int32, 0-based.  tol: None or <= 0 means
        machine epsilon.  Returns (cov [nprob, n, n], rank int32 [nprob]); rows and columns of the n - rank variables
        pivoted last are exactly zero."""
        nprob, n, _ = R.shape
        _chk(R, (nprob, n, n), "R")
        if not (ipvt.is_cuda and ipvt.dtype == torch.int32 and ipvt.is_contiguous() and tuple(ipvt.shape) == (nprob, n)):
            raise ValueError("ipvt: expected a contiguous int32 GPU tensor of shape [nprob, n]")
        cov = torch.empty((nprob, n, n), dtype=torch.float64, device=R.device)
        rank = torch.empty((nprob,), dtype=torch.int32, device=R.device)
        self._call("nlh_covar", nprob, n, R.data_ptr(), ipvt.data_ptr(), 0.0 if tol is None else float(tol),
                   cov.data_ptr(), rank.data_ptr())
        return cov, rank

    def lm_covariance_batch_device(self, fcn, ctx, m, x, jac=None, scaled=True, tol=None):
        """Parameter covariance of x.shape[0] least-squares problems of a USER'S device residual AT x ([nprob, n], not
        modified): F(x), a fresh Jacobian (jac, or forward differences), the exact lmfactor, covar.  Returns (cov
        [nprob, n, n], sigma [nprob, n], rank int32 [nprob], chi2 [nprob]); scaled: cov is multiplied by chi2 =
        ||F(x)||^2 / (m - n).  Raises NonlinError-coded RuntimeError for m < n (212) and for scaled with m <= n (201)."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        dev = x.device
        cov = torch.empty((nprob, n, n), dtype=torch.float64, device=dev)
        sigma = torch.empty((nprob, n), dtype=torch.float64, device=dev)
        rank = torch.empty((nprob,), dtype=torch.int32, device=dev)
        chi2 = torch.empty((nprob,), dtype=torch.float64, device=dev)
        self._call("nlh_lm_covariance_batch_device", nprob, int(m), n, self._devfcn(fcn), self._devfcn(jac),
                   self._ctxp(ctx), x.data_ptr(), int(bool(scaled)), 0.0 if tol is None else float(tol), cov.data_ptr(),
                   sigma.data_ptr(), rank.data_ptr(), chi2.data_ptr())
        return cov, sigma, rank, chi2

    # -- confidence and prediction bands: the covariance propagated through a function of the parameters ---------------
    @staticmethod
    def _band_args(nprob, n, cov, noise):
        _chk(cov, (nprob, n, n), "cov")
        if noise is not None:
            _chk(noise, (nprob,), "noise")
        return noise.data_ptr() if noise is not None else None

    def propagate(self, J, cov, noise=None):
        """The delta method, the raw kernel (nlh_propagate): sd [npoints, m] = sqrt(J_i cov J_i^T) for every row i of the
        Jacobians J [npoints, n, m] (each point column-major m x n, as a Jacobian launcher writes it) under the covariances
        cov [npoints, n, n], read by their lower triangle.  noise [npoints]: a variance added once to every row of its
        point (None: none).  One standard deviation: the coverage factor is the caller's.  A NaN matrix gives NaN rows."""
        npoints, n, m = J.shape
        _chk(J, (npoints, n, m), "J")
        pn = self._band_args(npoints, n, cov, noise)
        sd = torch.empty((npoints, m), dtype=torch.float64, device=J.device)
        self._call("nlh_propagate", npoints, m, n, J.data_ptr(), cov.data_ptr(), pn, sd.data_ptr())
        return sd

    def propagate_batch_device(self, fcn, ctx, m, x, cov, jac=None, noise=None):
        """Values and standard deviations of ANY launcher pair at x [nprob, n] under the parameter covariances cov
        [nprob, n, n] (nlh_propagate_batch_device): val = F(x) [nprob, m], a Jacobian (jac, or forward differences by
        fd_jacobian_device's rule), then propagate.  Returns (val, sd).  noise [nprob]: a variance added to every row --
        None gives the confidence band, the fit's chi2 (with the scaled covariance of an unweighted fit) the prediction
        band.  m may be smaller than n: the standard error of a derived quantity is this call on a one-row model, e.g. an
        Expr of the parameters through expr_launchers with y = 0.
        After a fit with conv=: run it over conv_launchers around the plotting grid's launchers with y = 0.  After a fit
        with group=: run it over group_launchers, with the per-group cov the fit returned and x = group_gather(group, x)."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        pn = self._band_args(nprob, n, cov, noise)
        m = int(m)
        val = torch.empty((nprob, m), dtype=torch.float64, device=x.device)
        sd = torch.empty((nprob, m), dtype=torch.float64, device=x.device)
        self._call("nlh_propagate_batch_device", nprob, m, n, self._devfcn(fcn), self._devfcn(jac), self._ctxp(ctx),
                   x.data_ptr(), cov.data_ptr(), pn, val.data_ptr(), sd.data_ptr())
        return val, sd

    def curve_band(self, kind, x, cov, t, ncomp=1, baseline=-1, noise=None):
        """curve_eval plus the band (nlh_curve_band_batch): the model values y [nprob, npts] of x [nprob, n] at the abscissae
        t [nprob, npts] (or one shared [npts] tensor) and their standard deviations sd [nprob, npts] under the parameter
        covariances cov [nprob, n, n], with the analytic Jacobian.  Returns (y, sd); noise as in propagate_batch_device.
        After a fit with pmap=, sep=, loss= or stat= the one-call fits return full-size x and cov: this applies as it
        is (a fixed parameter's zero row and column contribute nothing).  conv= and group=: propagate_batch_device."""
        k = curve_kind(kind)
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        if n != curve_nparams(k, ncomp, baseline):
            raise ValueError(f"x has {n} columns, the model {curve_nparams(k, ncomp, baseline)} parameters")
        shared = t.dim() == 1
        npts = t.shape[-1]
        _chk(t, (npts,) if shared else (nprob, npts), "t")
        pn = self._band_args(nprob, n, cov, noise)
        y = torch.empty((nprob, npts), dtype=torch.float64, device=x.device)
        sd = torch.empty((nprob, npts), dtype=torch.float64, device=x.device)
        self._call("nlh_curve_band_batch", k, int(ncomp), int(baseline), nprob, npts, t.data_ptr(), int(shared),
                   x.data_ptr(), cov.data_ptr(), pn, y.data_ptr(), sd.data_ptr())
        return y, sd

    def expr_band(self, expr, x, cov, t, noise=None):
        """expr_eval plus the band (nlh_expr_band_batch): curve_band with an Expr in the place of (kind, ncomp, baseline); t
        as expr_eval takes it.  Returns (y, sd).  The same rules after pmap=, sep=, loss=, stat=, conv= and group= fits."""
        nprob, n = x.shape
        _chk(x, (nprob, n), "x")
        if n != expr.nparams:
            raise ValueError(f"x has {n} columns, the formula {expr.nparams} parameters")
        npts = t.shape[-1]
        shared = self._expr_t(expr, t, nprob, npts)
        pn = self._band_args(nprob, n, cov, noise)
        y = torch.empty((nprob, npts), dtype=torch.float64, device=x.device)
        sd = torch.empty((nprob, npts), dtype=torch.float64, device=x.device)
        self._call("nlh_expr_band_batch", expr.ptr, nprob, npts, t.data_ptr(), int(shared), x.data_ptr(),
                   cov.data_ptr(), pn, y.data_ptr(), sd.data_ptr())
        return y, sd

    def chol_rank1(self, Rt, u, downdate=False):
        """In place on the row-major upper Cholesky factor Rt (n x n): R1^T R1 = R^T R +- u u^T.  Returns info."""
        n = Rt.shape[0]
        _chk(Rt, (n, n), "Rt"); _chk(u, (n,), "u")
        info = C.c_int32(0)
        self.h.check(self.lib.nlh_chol_rank1(self.h.ptr, n, int(downdate), Rt.data_ptr(), u.data_ptr(), C.byref(info)),
                     "nlh_chol_rank1")
        return int(info.value)

    def bf_chol_factor(self, B):
        """R = chol(B) as bfgs%solve forms it: B [nprob, n, n] symmetric.  Returns (Rt [nprob, n, n] row-major upper
        factors, info list: 0 or the 1-based row of a non-positive pivot)."""
        nprob, n, _ = B.shape
        _chk(B, (nprob, n, n), "B")
        Rt = torch.empty_like(B)
        info = (C.c_int32 * nprob)()
        self._call("nlh_bf_chol_factor", nprob, n, B.data_ptr(), Rt.data_ptr(), info)
        return Rt, [int(v) for v in info]

    def bf_chol_form(self, n):
        """The form bf_chol_factor takes for n: 4, 2, 1 blocked with that many thread groups per column; -4, -8 the column
        form with that many columns per thread."""
        return int(self.lib.nlh_bf_chol_form(int(n)))

    def bf_solve_cholesky(self, Rt, x):
        """x <- (R^T R)^-1 x in place, Rt [nprob, n, n] row-major upper factors, x [nprob, n]."""
        nprob, n, _ = Rt.shape
        _chk(Rt, (nprob, n, n), "Rt"); _chk(x, (nprob, n), "x")
        self._call("nlh_bf_solve_cholesky", nprob, n, Rt.data_ptr(), x.data_ptr())
        return x

    def lu_solve(self, LU, ipvt, b):
        nprob, n, _ = LU.shape
        self.h.check(self.lib.nlh_lu_solve(self.h.ptr, nprob, n, LU.data_ptr(), ipvt.data_ptr(), b.data_ptr()),
                     "nlh_lu_solve")
        return b


class HostModel(_lib.Owner):
    """A device residual model behind HOST arrays (nlh_dq_model): the boundary object the Fortran shim's
    `device_model_batch` wraps.  A [nprob, n, m] (each problem column-major m x n), b [nprob, m] are numpy arrays;
    the copies live on one device (`owner` a DeviceSolver) or are dealt over the devices of a DeviceSet."""
    _slot, _free = "_md", "nlh_dq_model_destroy"

    def __init__(self, owner, A, b, gamma):
        self.owner = owner
        self.lib = owner.lib
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        self.nprob, self.n, self.m = A.shape
        if b.shape != (self.nprob, self.m):
            raise ValueError("b must be [nprob, m]")
        self._md = C.c_void_p()
        dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
        if isinstance(owner, DeviceSet):
            rc = self.lib.nlh_dq_model_create_on(owner.ptr, self.nprob, self.m, self.n, dp(A), dp(b), float(gamma), C.byref(self._md))
        else:
            rc = self.lib.nlh_dq_model_create(owner.h.ptr, self.nprob, self.m, self.n, dp(A), dp(b), float(gamma), C.byref(self._md))
        self._checked(rc, "nlh_dq_model_create")

    def _checked(self, rc, what):
        """A return code that must be 0: the owner's error, with the library's message, for a negative one."""
        self.owner.check(rc, what)
        if rc != 0:
            raise RuntimeError(f"{what}: {rc}")

    @property
    def _hptr(self):
        """The handle the model's entry points take: the solver's, or NULL for a model dealt over a DeviceSet."""
        return None if isinstance(self.owner, DeviceSet) else self.owner.h.ptr

    @property
    def shares(self):
        return int(self.lib.nlh_dq_model_device_count(self._md))

    def _solve(self, fn, x, opts, *extra):
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        f = np.empty((self.nprob, self.m))
        ib, st = _ib_status(self.nprob)
        dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
        rc = fn(self._hptr, C.byref(opts if opts is not None else _lib.default_options()), self._md, *extra, dp(x), dp(f), ib, st)
        self._checked(rc, fn.__name__)
        return (x, f) + _ib_lists(ib, st)

    def lm_solve(self, x, opts=None):
        """least_squares_solver%solve on every problem: returns (x, fvec, iteration behaviours, status codes)."""
        return self._solve(self.lib.nlh_dq_model_lm_solve, x, opts)

    def newton_solve(self, x, analytic=True, opts=None):
        return self._solve(self.lib.nlh_dq_model_newton_solve, x, opts, 1 if analytic else 0)

    def quasi_newton_solve(self, x, analytic=True, jdelta=5, opts=None):
        """quasi_newton_solver%solve on every (square) problem; jdelta: iterations between fresh Jacobians."""
        return self._solve(self.lib.nlh_dq_model_quasi_newton_solve, x, opts, int(jdelta), 1 if analytic else 0)

    def cls_solve(self, x, lower=None, upper=None, delta=1.0, stepscale=1.0, opts=None):
        """constrained_least_squares_solver%solve on every problem inside the box [lower, upper] (n entries each, or None)."""
        return self._solve(self.lib.nlh_dq_model_cls_solve, x, opts, float(delta), float(stepscale),
                           *_host_bounds(lower, upper, self.n, "bounds must have n entries"))

    def bfgs_solve(self, x, opts=None):
        """bfgs%solve on 0.5 ||F(x)||^2 of every problem: returns (x, F(x), objective values, behaviours, status codes)."""
        x = np.ascontiguousarray(x, dtype=np.float64).copy()
        f = np.empty((self.nprob, self.m))
        fo = np.empty(self.nprob)
        ib, st = _ib_status(self.nprob)
        dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
        rc = self.lib.nlh_dq_model_bfgs_solve(self._hptr, C.byref(opts if opts is not None else _lib.default_options()), self._md,
                                              dp(x), dp(f), dp(fo), ib, st)
        self._checked(rc, "nlh_dq_model_bfgs_solve")
        return (x, f, fo) + _ib_lists(ib, st)

    def lm_covariance(self, x, scaled=True, tol=None):
        """Parameter covariance of every problem at x ([nprob, n] host array, not modified): returns numpy arrays (cov
        [nprob, n, n], sigma [nprob, n], rank int32 [nprob], chi2 [nprob]).  See nlh_dq_model_lm_covariance."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.nprob, self.n):
            raise ValueError("x must be [nprob, n]")
        cov = np.empty((self.nprob, self.n, self.n))
        sigma = np.empty((self.nprob, self.n))
        rank = np.empty(self.nprob, dtype=np.int32)
        chi2 = np.empty(self.nprob)
        dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
        rc = self.lib.nlh_dq_model_lm_covariance(self._hptr, self._md, dp(x), int(bool(scaled)), 0.0 if tol is None else float(tol),
                                                 dp(cov), dp(sigma), rank.ctypes.data_as(_lib.c_int32_p), dp(chi2))
        self._checked(rc, "nlh_dq_model_lm_covariance")
        return cov, sigma, rank, chi2


class DeviceSet(_lib.Owner):
    """nlh_device_set: one handle per listed device inside ONE process; models created on it are dealt over the devices
    block-cyclically and solved by one host thread per device (no collective).  devices=None: every visible device;
    an id may repeat (two shares on one GPU)."""
    _slot, _free = "_s", "nlh_device_set_destroy"

    def __init__(self, devices=None):
        self.lib = _lib.load()
        if self.lib.nlh_device_count() <= 0:
            raise _lib.NonlinHipUnavailable("no HIP device visible: the nonlin_amd compute path needs a GPU "
                                          "(there is no CPU fallback)")
        self._s = C.c_void_p()
        if devices is None:
            rc = self.lib.nlh_device_set_create(C.byref(self._s), None, 0)
        else:
            arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            rc = self.lib.nlh_device_set_create(C.byref(self._s), arr, len(devices))
        if rc != 0:
            raise _lib.NonlinHipUnavailable(f"nlh_device_set_create failed with {rc}")

    @property
    def ptr(self):
        return self._s

    def __len__(self):
        return int(self.lib.nlh_device_set_size(self._s))

    def check(self, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what}: library error {rc}: {self.lib.nlh_device_set_last_error(self._s).decode()}")
        return rc

    def model(self, A, b, gamma):
        return HostModel(self, A, b, gamma)
