"""The cases and the recorder behind tests/test_front_calls_cpu.py and tests/golden/make_front_calls.py: what the composed
one-call paths of DeviceSolver -- curve_fit_batch / expr_fit_batch with starts= or bins=, curve_boot_batch / expr_boot_batch,
and the refusals of all of them and of the plain front -- hand to the library, call by call: every entry point in order, every
scalar, every host array, what every pointer points at, what comes back and what is left on the Starts object, or the text the
call is refused with.  fit_call_cases.py pins the single call of a plain fit; this pins the sequences around it.

No device.  The data and the feature objects are fit_call_cases.Bench's (four data sets, m = 12, n = 3), on the host.  Inside
a MonkeyPatch context DeviceSolver._call appends (entry, arguments) to a trace and returns; torch.empty / empty_like give
zeros, so that what the Python reads back -- which start won, the statuses, the bad-problem mask -- is all zero and the code
after it runs; Tensor.is_cuda answers True; torch.cuda.current_stream gives an object whose synchronize() does nothing; and
Tensor.data_ptr notes the tensor it was asked of, so that an address met in a call can be traced back to its contents.
A pointer is recorded as the name of the caller's tensor it equals; failing that as {"from": [i, k]}, argument k of the
earlier call i of the trace that received the same address (the bootstrap's y*); failing that by its dtype, shape and
contents (the tiled t, weights, x, scales and taps, the nodes and the zero y under bins=).  The context a *_wrap makes is
["ctx", i], the wrap being call i; a model's own context is recorded field by field; closing a context is a call of the
trace as well.  Test infrastructure, not part of the product."""
import ctypes as C
import json

import numpy as np

import fit_call_cases as FC

NPROB, M, N = FC.NPROB, FC.M, FC.N
MODELS = FC.MODELS
NREP, KEEP, NCAND, ORDER = 5, 2, 16, 3
LAUNCHER_KINDS = ("curve", "expr", "pmap", "group", "loss", "pois", "conv", "bin", "sep")

# every entry point the composed paths can reach (the _group fits belong to the plain front: fit_call_cases has them)
REACHABLE = sorted(
    ["nlh_%s_fit_batch%s" % (md, v) for md in MODELS for v in ("", "_pmap", "_loss", "_pois", "_conv", "_sep")] +
    ["nlh_%s_%s" % (k, w) for k in ("bin", "conv", "pois", "loss", "sep") for w in ("wrap", "unwrap")] +
    ["nlh_starts_search_batch_device", "nlh_starts_cost_batch", "nlh_starts_pick_batch", "nlh_starts_take_batch",
     "nlh_lm_solve_batch_device", "nlh_cls_solve_batch_device", "nlh_lm_covariance_batch_device",
     "nlh_curve_eval_batch", "nlh_expr_eval_batch", "nlh_conv_apply_batch", "nlh_curve_guess_batch",
     "nlh_boot_resample_batch", "nlh_boot_poisson_batch", "nlh_boot_summary_batch"])

# features a case names, in the order its key lists them
STARTS_CASES = ("", "weights", "conv", "loss", "stat", "conv+loss", "conv+stat", "sep", "sep+conv", "weights+conv", "weights+stat",
                "weights+conv+stat", "weights+loss", "weights+sep", "conv_each+loss_each", "bounds", "nocov", "fd", "sep+bounds+nocov")
BINS_CASES = ("", "weights", "conv", "loss", "mask+stat", "conv+stat", "mask+conv+stat", "weights+conv", "weights+loss",
              "weights+conv+loss", "conv_each+loss_each", "bounds", "fd", "nocov", "weights+bounds+nocov", "mask+stat+nocov")
BOOT_CASES = ("residual", "wild", "pairs", "pairs+weights", "residual+weights", "residual+conv", "residual+conv_each", "wild+loss",
              "residual+loss_each", "residual+pmap", "wild+sep", "residual+sep+conv", "residual+bounds", "pairs+bounds+fd",
              "poisson+stat", "poisson+stat+mask", "poisson+stat+conv+pmap", "poisson+stat+loss", "residual+weights+conv+loss")
BOOT_T = {"curve": ("residual+t2", "pairs+weights+t2"), "expr": ("residual+tshared", "residual+t3", "pairs+weights+t3", "poisson+stat+t3")}
GUESS_CASES = ("x0none", "x0none+weights+conv", "x0none+bounds+sep")   # a curve guesses its start; a formula has no guess and fails
REFUSED = {
    "fit": ("starts+x0given+pmap", "starts+x0given", "starts+pmap", "starts4+group", "starts+group", "starts4", "starts+stat+loss",
            "starts+sep+loss", "starts+sep+stat", "starts+sep4", "starts4+sep+loss", "starts+pmap+stat+loss",
            "bins+pmap+starts", "bins+x0none+tgiven", "bins+x0none", "bins+tgiven", "pixels", "pixels+tgiven", "bins+nodof", "bins+group",
            "bins+sep", "bins+starts", "bins+stat+loss", "bins+pmap+x0none",
            "x0none+pmap", "x0none+group", "x0none+pmap+stat+loss"),
    "boot": ("residual+stat+group", "residual+stat", "residual+group", "poisson", "poisson+group", "poisson+stat+group", "pairs+conv",
             "pairs+conv+stat", "poisson+conv", "residual+sep+pmap", "residual+pmap4"),
}


def cases():
    """[(key, path, model, features)]: path is "fit" or "boot"; the key is "<path> <model> <features>"."""
    out = []
    for model in MODELS:
        out += [("fit", model, "+".join(f for f in ("starts", c) if f)) for c in STARTS_CASES]
        out += [("fit", model, "+".join(f for f in ("bins", c) if f)) for c in BINS_CASES]
        for c in BOOT_CASES + BOOT_T[model]:
            out += [("boot", model, c), ("boot", model, c + "+reps2")]
        out += [("fit", model, c) for c in GUESS_CASES]
        out += [(path, model, c) for path in ("fit", "boot") for c in REFUSED[path]]
    return [("%s %s %s" % c,) + c for c in out]


def group_of(key):
    """The cases one test checks together: a path, a model and the leading feature."""
    path, model, feats = key.split(" ")
    return "%s %s %s" % (path, model, feats.split("+")[0])


class _Stream:
    def synchronize(self):
        pass


class _Lib:
    """The library, except that closing a wrapped context is a call of the trace: the contexts of a trace are made up."""

    def __init__(self, lib, front):
        self._lib, self._front = lib, front

    def __getattr__(self, name):
        if name.endswith("_unwrap"):
            return lambda p: self._front.calls.append({"entry": name, "args": [self._front.enc(p)]})
        return getattr(self._lib, name)


class Front:
    """fit_call_cases.Bench with the tracing solver, the objects the composed paths add, and the recorder."""
    FAKE = 0x7A0000000000                                             # where the made-up contexts of a trace start

    def __init__(self):
        import torch
        from nonlin_amd import _lib
        self.b = b = FC.Bench()
        self.nl, self.ds = b.nl, b.ds
        self.real = _lib.load()
        self.ds.lib = _Lib(self.real, self)
        addr = lambda f: C.cast(f, C.c_void_p).value
        self.launchers = {addr(getattr(self.real, "nlh_%s_device_%s" % (k, f))): "nlh_%s_device_%s" % (k, f)
                          for k in LAUNCHER_KINDS for f in ("fcn", "jac")}
        nl = b.nl
        ten = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        mask = np.ones((NPROB, M))
        mask[:, ::5] = 0.0
        nodof = np.zeros((NPROB, M))
        nodof[:, :N] = 1.0
        self.mask, self.nodof = ten(mask), ten(nodof)
        self.t2 = {"curve": b.t["expr"], "expr": b.t["curve"]}        # the other model's form: per problem for a curve, shared for a formula
        self.t3 = b.t["expr"].reshape(1, NPROB, M).clone()
        box = dict(lower=[0.1, 0.01, -1.0], upper=[10.0, 5.0, 1.0], ncand=NCAND, keep=KEEP, log=(1,))
        self.starts = lambda: nl.Starts(**box)
        self.starts4 = lambda: nl.Starts(box["lower"] + [0.0], box["upper"] + [1.0], ncand=NCAND, keep=KEEP)
        e = np.linspace(0.0, 3.0, M + 1)
        self.bins = nl.Binned.edges(e, order=ORDER)
        self.pixels = nl.Binned.pixels((e[:-1], e[1:]), (e[:-1], e[1:]))
        self.boots = {k: nl.Bootstrap(nrep=NREP, kind=k, seed=11) for k in ("residual", "wild", "pairs")}
        self.boots["poisson"] = nl.PoissonBootstrap(nrep=NREP, seed=11)
        self.calls, self.names, self.tensors, self.seen, self.ctxs = [], {}, {}, {}, {}

    # -- the recorder ---------------------------------------------------------------------------------------------------
    def note(self, t, addr):
        if addr:
            self.tensors[addr] = t

    def pointee(self, addr):
        """A device address by name, by the earlier call that received it, or by contents."""
        if addr is None or addr == 0:
            return None
        if addr in self.names:
            return self.names[addr]
        if addr in self.seen:
            return {"from": list(self.seen[addr])}
        return self.contents(self.tensors[addr])

    def contents(self, t):
        a = t.detach().numpy()
        rec = {"dtype": str(t.dtype).replace("torch.", ""), "shape": list(t.shape)}
        flat = np.ascontiguousarray(a).reshape(-1)
        if not flat.any():
            return dict(rec, data="zeros")
        for name, src in self.named.items():                          # the tiled copies of a bootstrap chunk
            s = src.numpy().reshape(-1)
            if flat.dtype == s.dtype and flat.size >= s.size and flat.size % s.size == 0 and np.array_equal(flat, np.tile(s, flat.size // s.size)):
                return dict(rec, tile=name, reps=flat.size // s.size)
        return dict(rec, data=flat.tolist())

    def model_ctx(self, kind, addr):
        from nonlin_amd import _lib
        ctx = (_lib.CurveCtx if kind == "curve" else _lib.ExprCtx).from_address(addr)
        rec = {}
        for k, _ in ctx._fields_:
            v = getattr(ctx, k)
            rec[k] = self.pointee(v) if k in ("dt", "dy", "dw") else self.names.get(v, v) if k == "e" else int(v)
        return rec

    def enc(self, a, inner=None):
        """One argument as the library would read it; inner: the launcher the argument is the context of."""
        from nonlin_amd import _lib
        if a is None or isinstance(a, (bool, float, str)):
            return a
        if isinstance(a, (int, np.integer)):
            return self.pointee(int(a)) if int(a) in self.tensors or int(a) in self.names else int(a)
        if isinstance(a, _lib.DEVFCN):
            return self.launchers[C.cast(a, C.c_void_p).value] if a else None
        if isinstance(a, C.c_void_p):
            if a.value in self.ctxs:
                return ["ctx", self.ctxs[a.value]]
            if a.value is None or a.value in self.names:
                return self.names.get(a.value)
            assert inner and inner.split("_")[1] in ("curve", "expr"), (inner, a)
            return self.model_ctx(inner.split("_")[1], a.value)
        if hasattr(a, "_arr"):                                        # ndarray.ctypes.data_as keeps its array
            return {"host": str(a._arr.dtype), "data": a._arr.tolist()}
        if isinstance(a, C.Array):
            return ["array", type(a)._type_.__name__, len(a)]
        obj = a._obj                                                  # byref
        if isinstance(obj, _lib.Options):
            o = {k: getattr(obj, k) for k, _ in _lib.Options._fields_}
            return "default options" if o == self.b.default_options else o
        if isinstance(obj, _lib.ConvStruct):
            return {"L": obj.L, "origin": obj.origin, "ext": obj.ext, "shared_k": obj.shared_k, "k": self.pointee(obj.k)}
        if isinstance(obj, _lib.BinStruct):
            return {"Q": obj.Q, "c": list(obj.c), "s": self.pointee(obj.s), "shared_s": obj.shared_s}
        assert isinstance(obj, C.c_void_p), obj                       # where a *_wrap leaves its context
        obj.value = self.FAKE + 64 * len(self.calls)
        self.ctxs[obj.value] = len(self.calls)
        return "out"

    def call(self, _ds, entry, *args):
        rec, inner = [], None
        for a in args:
            rec.append(self.enc(a, inner))
            inner = rec[-1] if isinstance(rec[-1], str) and "_device_" in rec[-1] else inner
        for k, a in enumerate(args):                                  # what a later call can refer to
            if isinstance(a, int) and a in self.tensors and a not in self.names:
                self.seen.setdefault(a, (len(self.calls), k))
        self.calls.append({"entry": entry, "args": rec})

    def origin(self, v):
        """A tensor that comes back: [dtype, shape, where the trace filled it -- None: torch made it]."""
        import torch
        if not isinstance(v, torch.Tensor):
            return v if v is None else ["list", len(v)]
        raw = self.raw_data_ptr(v)
        where = self.names.get(raw) or (list(self.seen[raw]) if raw in self.seen else None)
        return [str(v.dtype).replace("torch.", ""), list(v.shape), where]

    # -- the cases --------------------------------------------------------------------------------------------------------
    def keywords(self, model, feats):
        b, f = self.b, set(feats)
        pick = lambda name, each: b.twisted["each"][name] if each in f else b.right[name] if name in f else None
        kw = dict(weights=self.mask if "mask" in f else self.nodof if "nodof" in f else b.w if "weights" in f else None,
                  lower=b.lower if "bounds" in f else None, upper=b.upper if "bounds" in f else None, analytic="fd" not in f,
                  loss=pick("loss", "loss_each"), conv=pick("conv", "conv_each"), stat=b.right["stat"] if "stat" in f else None,
                  pmap=b.twisted["size"]["pmap"] if "pmap4" in f else b.right["pmap"] if "pmap" in f else None,
                  sep=b.twisted["size"]["sep"] if "sep4" in f else b.right["sep"] if "sep" in f else None,
                  group=b.right["group"] if "group" in f else None)
        t = self.t3 if "t3" in f else self.t2[model] if "t2" in f or "tshared" in f else b.t[model]
        return t, kw

    def run(self, mp, path, model, feats):
        """One case: {"trace": [calls], "ret": ..., "starts": ...}, or {"trace", "raises": the refusal}."""
        b, f = self.b, feats.split("+")
        t, kw = self.keywords(model, f)
        named = {"t": t, "y": b.y, "w": kw["weights"], "x": b.x0}
        self.named = {k: v for k, v in named.items() if v is not None}
        self.calls, self.tensors, self.seen, self.ctxs = [], {}, {}, {}
        self.names = {self.raw_data_ptr(v): k for k, v in self.named.items()}
        self.names.update({b.expr.ptr.value: "expr"})
        self.names.update({kw[k].ptr.value: k for k in ("pmap", "group", "sep") if kw[k] is not None and hasattr(kw[k], "ptr")})
        head = (FC.KIND,) if model == "curve" else (b.expr,)
        shape = dict(ncomp=FC.NCOMP, baseline=FC.BASELINE) if model == "curve" else {}
        starts = None
        if "reps2" in f:
            mp.setenv("NLH_BOOT_REPS", "2")
        else:
            mp.delenv("NLH_BOOT_REPS", raising=False)
        try:
            if path == "boot":
                boot = self.boots[f[0]]
                ret = getattr(self.ds, model + "_boot_batch")(*head, t, b.y, b.x0, boot, **shape, **kw)
            else:
                starts = self.starts4() if "starts4" in f else self.starts() if "starts" in f else None
                bins = self.pixels if "pixels" in f else self.bins if "bins" in f else None
                x0 = b.x0 if "x0given" in f or not (starts is not None or "x0none" in f) else None
                tt = None if bins is not None and "tgiven" not in f else t
                ret = getattr(self.ds, model + "_fit_batch")(*head, tt, b.y, x0, covariance="nocov" not in f, starts=starts, bins=bins,
                                                             **shape, **kw)
        except Exception as e:                                        # a ValueError by its text, anything else by its type
            return {"trace": self.calls, "raises": "ValueError: %s" % e if type(e) is ValueError else type(e).__name__}
        out = {"trace": self.calls, "ret": [self.origin(v) for v in ret]}
        if starts is not None:
            out["starts"] = {k: self.origin(getattr(starts, k)) for k in ("which", "index", "cost")}
        return out

    def record_all(self):
        import pytest
        import torch
        from nonlin_amd import device
        self.raw_data_ptr = raw = torch.Tensor.data_ptr

        def data_ptr(t):
            addr = raw(t)
            self.note(t, addr)
            return addr

        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(device.DeviceSolver, "_call", lambda ds, entry, *args: self.call(ds, entry, *args))
            mp.setattr(torch, "empty", torch.zeros)
            mp.setattr(torch, "empty_like", torch.zeros_like)
            mp.setattr(torch.Tensor, "is_cuda", property(lambda t: True))
            mp.setattr(torch.Tensor, "data_ptr", data_ptr)
            mp.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())
            return json.loads(json.dumps({key: self.run(mp, *c) for key, *c in cases()}))


def record_all():
    """{key: what Front.run gives}, as JSON gives it back."""
    return Front().record_all()


# -- the golden file: the distinct calls once, every case a list of positions in them ------------------------------------------
def dump(rec, path):
    enc = lambda v: json.dumps(v, separators=(",", ":"))
    table, lines = {}, []
    for key, case in rec.items():
        idx = [table.setdefault(enc(c), len(table)) for c in case["trace"]]
        lines.append("%s: %s" % (json.dumps(key), enc(dict(case, trace=idx))))
    with open(path, "w") as f:
        f.write('{"calls": [\n' + ",\n".join(table) + '\n],\n"cases": {\n' + ",\n".join(lines) + "\n}}\n")


def load(path):
    with open(path) as f:
        g = json.load(f)
    return {key: dict(case, trace=[g["calls"][i] for i in case["trace"]]) for key, case in g["cases"].items()}
