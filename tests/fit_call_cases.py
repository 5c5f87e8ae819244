"""The cases, the recorder and the snapshot of the signature table behind tests/test_fit_calls_cpu.py and
tests/golden/make_fit_calls.py: what DeviceSolver.curve_fit_batch and expr_fit_batch hand to the library -- which entry
point, every scalar, what every pointer points at -- for every subset of {pmap, loss, stat, group, conv, sep}, crossed with
weights, bounds, analytic and covariance on and off, or the text of the ValueError the call is refused with.  No device: the
solver is made with __new__, its library is a recorder that answers 0 for the fit entry points, and the tensors live on the
host (the test lifts the is_cuda clause of device._chk).  Four data sets of m = 12 rows: a one-component exponential decay
on a constant baseline, and the formula a*exp(-k*t)+c.  Further cases ("twists", every switch on) reach what the crossing
cannot: objects of the wrong size, a group that does not divide the data sets, bounds of the wrong length, options of the
caller's, and scales and taps per problem.  Test infrastructure, not part of the product."""
import ctypes as C
import itertools
import json

import numpy as np

NPROB, M, N, NSETS, SEED = 4, 12, 3, 2, 2031
KIND, NCOMP, BASELINE = "expdecay", 1, 0                              # (a, k) on a constant c
FORMULA, VARS, PARAMS = "a*exp(-k*t)+c", ("t",), ("a", "k", "c")
MODELS = ("curve", "expr")
FEATURES = ("pmap", "loss", "stat", "group", "conv", "sep")
SWITCHES = ("weights", "bounds", "analytic", "covariance")
# twist -> the features of which a case needs at least one for the twist to change anything (None: any case)
TWISTS = {"size": ("pmap", "group", "sep"), "rows": ("group",), "bounds": None, "opts": None, "each": ("loss", "conv")}
MU_FLOOR = 2.0 ** -9

# the argument list of a fit entry point by name, as include/nonlin_hip.h declares it
HEAD = {"curve": ("handle", "opts", "kind", "ncomp", "nbase"), "expr": ("handle", "opts", "expr")}
DATA = ("nprob", "m", "t", "shared_t", "y", "w", "analytic", "xl", "xu")
MIDDLE = {"": (),
          "_pmap": ("pm",),
          "_loss": ("pm", "loss", "scale", "shared_scale"),
          "_pois": ("pm", "mu_floor"),
          "_group": ("g", "loss", "scale", "shared_scale", "stat", "mu_floor"),
          "_conv": ("g", "pm", "cv", "loss", "scale", "shared_scale", "stat", "mu_floor"),
          "_sep": ("g", "cv", "sp")}
TAIL = ("x", "fvec", "sigma", "cov", "chi2", "rank", "ib", "status")
INTS = ("kind", "ncomp", "nbase", "nprob", "m", "shared_t", "analytic", "loss", "shared_scale", "stat")
OBJECTS = ("handle", "expr", "pm", "g", "sp")
ARRAYS = ("t", "y", "w", "x", "fvec", "sigma", "cov", "chi2", "rank")
ENTRY_NAMES = ["nlh_%s_fit_batch%s" % (md, v) for md in MODELS for v in MIDDLE]

# every refusal of the two methods, as the cases word it
REFUSALS = (
    "stat and loss exclude each other: a Poisson fit has no robust loss",
    "sep excludes pmap, loss and stat: a map, a loss and a statistic are nonlinear in the projected parameters",
    "group and pmap exclude each other: a map inside a group works through pmap_launchers and group_launchers",
    "sep is over 4 parameters, the model has 3",
    "group is over 4 parameters, the model has 3",
    "4 data sets: no multiple of the group's 3",
    "pmap maps 4 parameters, the model has 3",
    "pmap maps 4 parameters, the formula has 3",
    "bounds: expected 3 entries",
)


def arg_names(entry):
    model, variant = entry[len("nlh_"):].split("_fit_batch")
    return HEAD[model] + DATA + MIDDLE[variant] + TAIL


def chk_any_device(t, shape, name):
    """device._chk without its is_cuda clause."""
    import torch
    if not (t.dtype == torch.float64 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise ValueError(f"{name}: expected contiguous float64 GPU tensor of shape {tuple(shape)}, "
                         f"got {t.dtype} {tuple(t.shape)} cuda={t.is_cuda}")


def cases():
    """[(key, model, features, switches, twist)]: the crossing, then the twists with every switch on."""
    subsets = [tuple(f for f, on in zip(FEATURES, bits) if on) for bits in itertools.product((0, 1), repeat=len(FEATURES))]
    out = []
    for model in MODELS:
        for feats in subsets:
            for sw in itertools.product((0, 1), repeat=len(SWITCHES)):
                out.append((model, feats, sw, None))
            for twist, needs in TWISTS.items():
                if needs is None or set(needs) & set(feats):
                    out.append((model, feats, (1, 1, 1, 1), twist))
    return [(case_key(*c),) + c for c in out]


def case_key(model, feats, sw, twist):
    return "%s %s %s%s" % (model, "+".join(feats) or "plain", "".join(n[0] + str(b) for n, b in zip(SWITCHES, sw)),
                           " " + twist if twist else "")


def group_of(key):
    """The cases one test checks together: a model and a subset of the features."""
    return " ".join(key.split(" ")[:2])


class _Handle:
    """What DeviceSolver needs of a Handle when nothing fails."""
    ptr = C.c_void_p(0x1000)

    def check(self, rc, what):
        assert rc >= 0, (rc, what)
        return rc


class Recorder:
    """A library whose fit entry points take their arguments down and answer 0; every other name is the library's."""

    def __init__(self, lib):
        self._lib, self.calls, self.names = lib, [], {}

    def __getattr__(self, name):
        if "fit_batch" in name:
            return lambda *args: self._fit(name, args)
        return getattr(self._lib, name)

    @staticmethod
    def _doubles(addr, count):
        return list((C.c_double * count).from_address(addr))

    def _fit(self, entry, args):
        """The arguments as the library would read them, while everything they point at is still alive."""
        from nonlin_amd import _lib
        names = arg_names(entry)
        assert len(args) == len(names), (entry, len(args), len(names))
        raw = dict(zip(names, args))
        addr = lambda a: a.value if isinstance(a, C.c_void_p) else a
        rec = []
        for nm in names:
            a = raw[nm]
            if nm in INTS:
                v = C.c_int32(a).value
            elif nm == "mu_floor":
                v = C.c_double(a).value
            elif nm in OBJECTS or nm in ARRAYS:
                v = None if addr(a) is None else self.names.get(addr(a), addr(a))     # an address nobody named: resolved on return
            elif nm == "opts":
                assert isinstance(a._obj, _lib.Options)
                v = {k: getattr(a._obj, k) for k, _ in _lib.Options._fields_}
            elif nm in ("xl", "xu"):
                v = None if a is None else [a[i] for i in range(N)]
            elif nm == "scale":
                v = None if addr(a) is None else self._doubles(addr(a), 1 if raw["shared_scale"] else raw["nprob"])
            elif nm == "cv":
                if a is None or addr(a) is None:
                    v = None
                else:
                    cv = a._obj if hasattr(a, "_obj") else _lib.ConvStruct.from_address(addr(a))
                    assert isinstance(cv, _lib.ConvStruct)
                    v = {"L": cv.L, "origin": cv.origin, "ext": cv.ext, "shared_k": cv.shared_k,
                         "k": self._doubles(cv.k, cv.L * (1 if cv.shared_k else raw["nprob"]))}
            else:                                                     # ib, status: arrays of the caller's
                v = len(a)
            rec.append(v)
        self.calls.append({"entry": entry, "args": rec})
        return 0


class Bench:
    """The solver without a device, the data of both models and the objects of every feature, right and wrong."""

    def __init__(self):
        import torch
        import nonlin_amd as nl
        from nonlin_amd import _lib, device
        self.nl = nl
        self.ds = device.DeviceSolver.__new__(device.DeviceSolver)
        self.ds.device, self.ds.h = torch.device("cpu"), _Handle()
        self.ds.lib = self.rec = Recorder(_lib.load())
        rng = np.random.default_rng(SEED)
        ten = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        self.expr = nl.Expr(FORMULA, VARS, PARAMS)
        self.t = {"curve": ten(np.linspace(0.0, 3.0, M)), "expr": ten(np.tile(np.linspace(0.0, 3.0, M), (NPROB, 1)))}   # shared, and not
        self.y, self.w, self.x0 = ten(rng.uniform(1.0, 9.0, (NPROB, M))), ten(rng.uniform(0.5, 2.0, (NPROB, M))), ten(rng.uniform(0.5, 1.5, (NPROB, N)))
        self.lower, self.upper = np.array([0.0, 0.01, -1.0]), np.array([10.0, 5.0, 1.0])
        taps = np.array([0.25, 0.5, 0.25])
        self.right = {"pmap": nl.ParamMap(N, fixed=(2,)), "loss": nl.Loss("huber", 0.75), "stat": nl.Poisson(MU_FLOOR),
                      "group": nl.Group(N, shared=(1,), nsets=NSETS), "conv": nl.Convolve(taps, origin=1, extend="hold"),
                      "sep": nl.Separable(N, linear=(0, 2))}
        self.twisted = {
            "size": {"pmap": nl.ParamMap(N + 1, fixed=(2,)), "group": nl.Group(N + 1, shared=(1,), nsets=NSETS),
                     "sep": nl.Separable(N + 1, linear=(0, 2))},
            "rows": {"group": nl.Group(N, shared=(1,), nsets=3)},
            "each": {"loss": nl.Loss("cauchy", 0.5 + 0.25 * np.arange(NPROB)),
                     "conv": nl.Convolve(taps[None, :] * (1.0 + np.arange(NPROB))[:, None], origin=0, extend="zero")}}
        self.default_options = {k: getattr(self.ds.options(), k) for k, _ in _lib.Options._fields_}

    def run(self, model, feats, sw, twist):
        """One case: the index of its refusal in REFUSALS, or {"entry", "args", "ret"}."""
        import torch
        weights, bounds, analytic, covariance = (bool(b) for b in sw)
        obj = {f: self.twisted.get(twist, {}).get(f, self.right[f]) for f in feats}
        t, w = self.t[model], self.w if weights else None
        lower = (self.lower[:2] if twist == "bounds" else self.lower) if bounds else None
        upper = (self.upper[:2] if twist == "bounds" else self.upper) if bounds else None
        opts = self.ds.options(max_evals=77, ftol=1e-6, sub_batches=2) if twist == "opts" else None
        named = {"t": t, "y": self.y, "w": self.w, "x0": self.x0}
        self.rec.names = {v.data_ptr(): k for k, v in named.items()}
        self.rec.names.update({_Handle.ptr.value: "handle", self.expr.ptr.value: "expr"})
        self.rec.names.update({obj[f].ptr.value: f for f in ("pmap", "group", "sep") if f in obj})
        self.rec.calls = []
        kw = dict(weights=w, lower=lower, upper=upper, analytic=analytic, covariance=covariance, opts=opts, **obj)
        try:
            if model == "curve":
                ret = self.ds.curve_fit_batch(KIND, t, self.y, self.x0, ncomp=NCOMP, baseline=BASELINE, **kw)
            else:
                ret = self.ds.expr_fit_batch(self.expr, t, self.y, self.x0, **kw)
        except ValueError as e:
            assert not self.rec.calls
            return REFUSALS.index(str(e))
        (call,) = self.rec.calls
        outs = {v.data_ptr(): "ret%d" % i for i, v in enumerate(ret) if isinstance(v, torch.Tensor)}
        call["args"] = [outs.get(a, "?") if isinstance(a, int) and nm in ARRAYS else a for nm, a in zip(arg_names(call["entry"]), call["args"])]
        if call["args"][1] == self.default_options:
            call["args"][1] = "default"
        call["ret"] = [[str(v.dtype)] + list(v.shape) if isinstance(v, torch.Tensor) else v if v is None else len(v) for v in ret]
        assert torch.equal(ret[0], self.x0)                          # x starts as a copy of x0
        return call


def record_all():
    """{"default_options", "refusals", "cases": {key: what Bench.run gives}}: what load gives of the golden file."""
    b = Bench()
    return {"default_options": b.default_options, "refusals": list(REFUSALS),
            "cases": {key: b.run(*c) for key, *c in cases()}}


# -- the golden file holds the cases packed by group, without loss: unpack(pack(cases)) == cases, which pack asserts ----------
def _delta(a, b):
    """What turns the call a into the call b of the same entry point: {"args": {name: value}, "ret": {position: value}}."""
    da = {n: y for n, x, y in zip(arg_names(a["entry"]), a["args"], b["args"]) if x != y}
    dr = {str(i): y for i, (x, y) in enumerate(zip(a["ret"], b["ret"])) if x != y}
    return {k: v for k, v in (("args", da), ("ret", dr)) if v}


def _apply(a, d):
    names = arg_names(a["entry"])
    out = {"entry": a["entry"], "args": list(a["args"]), "ret": list(a["ret"])}
    for n, v in d.get("args", {}).items():
        out["args"][names.index(n)] = v
    for i, v in d.get("ret", {}).items():
        out["ret"][int(i)] = v
    return out


def _split(suffix):
    """("w1b0a1c1", twist or None) -> (the switches that are on, twist)."""
    bits, _, twist = suffix.partition(" ")
    return [s for s in SWITCHES if s[0] + "1" in bits], twist or None


def _unpack_case(g, suffix):
    """A case of a packed group g: one refusal for every case; or the case as it stands in "cases"; or "base" (every switch
    off) with what each switch that is on changes ("on"), then what the twist changes or the refusal it meets ("twist")."""
    if isinstance(g, int):
        return g
    if suffix in g.get("cases", {}):
        return g["cases"][suffix]
    on, twist = _split(suffix)
    changes, twists = g.get("on", {}), g.get("twist", {})
    if twist and isinstance(twists.get(twist), int):
        return twists[twist]
    if "base" not in g or any(s not in changes for s in on) or (twist and twist not in twists):
        return None
    rec = g["base"]
    for s in on:
        rec = _apply(rec, changes[s])
    return _apply(rec, twists[twist]) if twist else rec


def pack(cases):
    """{key: case} -> {group: packed group}."""
    groups = {}
    for key, v in cases.items():
        groups.setdefault(group_of(key), {})[key[len(group_of(key)) + 1:]] = v
    off = "".join(s[0] + "0" for s in SWITCHES)
    top = "".join(s[0] + "1" for s in SWITCHES)
    out = {}
    for name, vals in groups.items():
        if len({json.dumps(v) for v in vals.values()}) == 1 and isinstance(vals[off], int):
            out[name] = vals[off]
            continue
        g = {"on": {}, "twist": {}, "cases": {}}
        if isinstance(vals[off], dict):
            g["base"] = vals[off]
            for s in SWITCHES:
                one = vals[off.replace(s[0] + "0", s[0] + "1")]
                if isinstance(one, dict):
                    g["on"][s] = _delta(vals[off], one)
        for suffix, v in vals.items():
            twist = _split(suffix)[1]
            if twist and isinstance(v, int):
                g["twist"][twist] = v
            elif twist and isinstance(vals[top], dict) and vals[top]["entry"] == v["entry"]:
                g["twist"][twist] = _delta(vals[top], v)
        for suffix, v in vals.items():
            if _unpack_case(g, suffix) != v:
                g["cases"][suffix] = v
        out[name] = {k: v for k, v in g.items() if v}
        assert all(_unpack_case(out[name], suffix) == v for suffix, v in vals.items()), name
    return out


def unpack(groups):
    """{group: packed group} -> {key: case}, for every case of cases()."""
    return {key: _unpack_case(groups[group_of(key)], key[len(group_of(key)) + 1:]) for key, *_ in cases()}


def dump(rec, path):
    """The golden file: a line per group."""
    enc = lambda v: json.dumps(v, separators=(",", ":"))
    packed = pack(json.loads(json.dumps(rec["cases"])))
    with open(path, "w") as f:
        f.write('{"default_options": %s,\n"refusals": %s,\n"groups": {\n' % (json.dumps(rec["default_options"]), json.dumps(rec["refusals"], indent=1)))
        f.write(",\n".join("%s: %s" % (json.dumps(k), enc(v)) for k, v in packed.items()))
        f.write("\n}}\n")


def load(path):
    """The golden file as record_all gives it: {"default_options", "refusals", "cases"}."""
    with open(path) as f:
        g = json.load(f)
    return {"default_options": g["default_options"], "refusals": g["refusals"], "cases": unpack(g["groups"])}


def symbols_snapshot():
    """_lib.SYMBOLS as the golden file holds it: {"types": {letter: name of a frequent type}, "symbols": {name: "result argument
    argument ..."}}, a ctypes type by its letter or its name, a callback type by the name _lib gives it, no result as "None"."""
    from nonlin_amd import _lib
    callbacks = {}
    for nm in ("VECFCN", "JACFCN", "FCNNVAR", "GRADFCN", "DEVFCN"):
        callbacks.setdefault(getattr(_lib, nm), nm)                   # (ctypes makes one type of equal signatures: the first name stands)
    letters = {"i": "c_int", "d": "c_double", "p": "c_void_p", "D": "LP_c_double", "I": "LP_c_int", "O": "LP_Options",
               "B": "LP_IterationBehavior"}
    short = {v: k for k, v in letters.items()}
    name = lambda t: "None" if t is None else callbacks[t] if t in callbacks else short.get(t.__name__, t.__name__)
    return {"types": letters, "symbols": {k: " ".join([name(res)] + [name(a) for a in args]) for k, (res, args) in _lib.SYMBOLS.items()}}
