"""The seeded batch and the callers of tests/test_gpu_fit_entry_points.py and tests/golden/make_fit_entry_points.py: one
small batch through each of the twelve one-call fits nlh_{curve,expr}_fit_batch{,_pmap,_loss}{,_h}, aimed at the offsets of
a run of problems.  Three problems of m = 12 rows with their own abscissae and weights; problem 1 has two rows with a weight
that is not zero, so it has no degree of freedom with or without the map and the runs of solvable problems start at problems
0 and 2.  Built on curve_cases.curve_problems (the Lorentzian data) and on expr_restatement as expr_cases.expr_problems is.
Test infrastructure, not part of the product."""
import ctypes as C
import itertools

import numpy as np

import curve_cases as CC
import curve_restatement as CR
import expr_restatement as XR

NPROB, M, N, SEED = 3, 12, 4, 2027
REFUSED = 1
KIND, K, B = "lorentz", 1, 0                                        # (a, mu, w) on a constant c
FORMULA, VARS, PARAMS = "a/(1+((t-mu)/w)^2)+c*u", "t,u", "a,mu,w,c"    # two variables: the stride between their blocks of t matters
MAP_FIXED, MAP_TIED = (3,), {0: (2, 3.3, 0.05)}                     # c fixed, a tied to w: free unknowns mu, w
HUBER = 1
MODELS = ("curve", "expr")
VARIANTS = ("fit", "pmap", "loss")
ENTRIES = [(md, v, host) for md in MODELS for v in VARIANTS for host in (False, True)]
ARRAYS = ("x", "fvec", "sigma", "cov", "chi2", "rank", "status", "ib")
IB_FIELDS = ("iter_count", "fcn_count", "jacobian_count", "gradient_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")

dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def entry_name(model, variant, host):
    return "nlh_%s_fit_batch%s%s" % (model, "" if variant == "fit" else "_" + variant, "_h" if host else "")


def configs(variant):
    """(mapped, robust, analytic, bounded) of every call an entry point gets."""
    ab = list(itertools.product((0, 1), (False, True)))
    if variant == "fit":
        return [(False, False, a, b) for a, b in ab]
    if variant == "pmap":
        return [(True, False, a, b) for a, b in ab]
    return [(mp, True, a, b) for mp in (False, True) for a, b in ab]


def batch(expr):
    """The data of both models: dict of numpy arrays.  expr: the compiled FORMULA (nonlin_amd.Expr)."""
    rng = np.random.default_rng(SEED)
    t, y, xt, x0 = CC.curve_problems(KIND, K, B, M, nprob=NPROB, seed=SEED, sigma=1e-3)
    u = rng.uniform(0.0, 1.0, (NPROB, M))
    tt = np.ascontiguousarray(np.stack([t, u]))                     # [nvar][nprob][m]
    prog = expr.program()
    ye = np.stack([XR.value(prog, xt[p], tt[:, p]) for p in range(NPROB)]) + 1e-3 * rng.uniform(-1, 1, (NPROB, M))
    for yy in (y, ye):                                              # a spike in problems 0 and 2: Huber's outer branch is taken
        yy[0, 4] += 0.05
        yy[2, 9] -= 0.04
    w = rng.uniform(0.5, 2.0, (NPROB, M))
    w[REFUSED] = 0.0
    w[REFUSED, [2, 8]] = [1.0, 1.5]                                 # 2 rows count: no degree of freedom for 2 unknowns or for 4
    w[2, [3, 7]] = 0.0                                              # padding in a problem that is solved: dof = 10 - n
    scale = 3e-3 * (1.0 + 0.5 * np.arange(NPROB))                   # a scale per problem
    lower, upper = xt.min(0) - 0.5, xt.max(0) + 0.5
    assert CR.nparams(CR.KINDS[KIND], K, B) == N == expr.nparams and expr.nvar == 2
    return dict(t=t, tt=tt, y=np.ascontiguousarray(y), ye=np.ascontiguousarray(ye), w=np.ascontiguousarray(w), x0=x0, scale=scale,
                lower=np.ascontiguousarray(lower), upper=np.ascontiguousarray(upper))


def _p(a):
    """What ctypes gets for an array: a device address, a host pointer, or NULL."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ip if a.dtype == np.int32 else dp)
    return a.data_ptr()


def call(ds, model, variant, host, opts, expr, nprob, m, t, y, w, analytic, lower, upper, pm, loss, scale, shared_scale, x, fvec, sigma,
         cov, chi2, rank, ib, status, handle=True, kind=CR.LORENTZ, ncomp=K, nbase=B):
    """One call of an entry point by its C signature.  Arrays: torch tensors on the device (host = False) or numpy arrays;
    lower / upper: numpy; pm: a ParamMap, its address, or None; expr: an Expr or None (a NULL formula)."""
    fn = getattr(ds.lib, entry_name(model, variant, host))
    head = [ds.h.ptr if handle else None, C.byref(opts) if opts is not None else None]
    head += [kind, ncomp, nbase] if model == "curve" else [expr.ptr if expr is not None else None]
    args = head + [nprob, m, _p(t), 0, _p(y), _p(w), analytic, _p(lower), _p(upper)]
    if variant != "fit":
        args.append(getattr(pm, "ptr", pm))
    if variant == "loss":
        args += [loss, _p(scale), shared_scale]
    return fn(*(args + [_p(x), _p(fvec), _p(sigma), _p(cov), _p(chi2), _p(rank), ib, status]))


def run_entry(ds, data, expr, pm, model, variant, host, sel=None):
    """Every configuration of one entry point on the problems sel (None: the whole batch): {array: [ncfg, nprob, ...]}.
    Floats come back as their uint64 bits.  fvec is preset to 7.0, so a row no call writes compares as that -- except the
    refused problem's row of a host-array form, which is read back from device memory nothing ever wrote: it is set to 0."""
    import torch
    from nonlin_amd import _lib
    rows = list(range(NPROB)) if sel is None else list(sel)
    nprob = len(rows)
    t = np.ascontiguousarray(data["t"][rows] if model == "curve" else data["tt"][:, rows])
    y = np.ascontiguousarray((data["y"] if model == "curve" else data["ye"])[rows])
    w, x0, scale = (np.ascontiguousarray(data[k][rows]) for k in ("w", "x0", "scale"))
    dev = (lambda a: a) if host else (lambda a: torch.from_numpy(a).to(ds.device))
    dt, dy, dw, dscale = dev(t), dev(y), dev(w), dev(scale)
    o = ds.options()
    out = {k: [] for k in ARRAYS}
    for mapped, robust, analytic, bounded in configs(variant):
        x = dev(x0.copy())
        res = dict(x=x, fvec=dev(np.full((nprob, M), 7.0)), sigma=dev(np.zeros((nprob, N))), cov=dev(np.zeros((nprob, N, N))),
                   chi2=dev(np.zeros(nprob)), rank=dev(np.zeros(nprob, dtype=np.int32)))
        ib, status = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        rc = call(ds, model, variant, host, o, expr, nprob, M, dt, dy, dw, analytic, data["lower"] if bounded else None,
                  data["upper"] if bounded else None, pm if mapped else None, HUBER if robust else 0, dscale if robust else None, 0,
                  res["x"], res["fvec"], res["sigma"], res["cov"], res["chi2"], res["rank"], ib, status)
        assert rc == 0, (entry_name(model, variant, host), mapped, robust, analytic, bounded, rc)
        if not host:
            torch.cuda.synchronize()
        for k, v in res.items():
            a = np.ascontiguousarray(v if host else v.cpu().numpy())
            if k == "fvec" and host and REFUSED in rows:
                a[rows.index(REFUSED)] = 0.0
            out[k].append(a if k == "rank" else a.view(np.uint64))
        out["status"].append(np.array(list(status), dtype=np.int32))
        out["ib"].append(np.array([[getattr(ib[p], f) for f in IB_FIELDS] for p in range(nprob)], dtype=np.int32))
    return {k: np.stack(v) for k, v in out.items()}
