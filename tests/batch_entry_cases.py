"""The solver entry points that take a user's launcher, as one table for tests/test_gpu_batch_entry_points.py: for each the
device-pointer form and its host-array twin, the argument list, the user family of tests/device_model (tests/device_1var
for the scalar roots) it is tested on at that family's smallest shape, a raw call with any argument replaced, and the CPU
oracle on one problem.  Test infrastructure, not part of the product."""
import ctypes as C
import functools

import numpy as np

import covar_restatement as cr
import scalar_models as SM
import user_models as UM
from nonlin_amd import _lib

dp = C.POINTER(C.c_double)
NP = 65541                                        # six problems past NLH_MAX_LOCKSTEP = 65535
SAMPLE = (0, 1, 65534, 65535, 65536, NP - 1)      # first, second, either side of the slice boundary, last
IB = 7                                            # int32 fields of nlh_iteration_behavior

# nlh_nm_solve_batch_device_h and nlh_root1v_solve_batch_device_h are the library's own (nlh_internal.h; what the
# nlh_dq_model_* entry points of a user's model run): C++ linkage, so _function looks their mangled names up in the
# library's dynamic symbol table by the function's name
NM_H, R1_H = "nlh_nm_solve_batch_device_h", "nlh_root1v_solve_batch_device_h"
INTERNAL = (NM_H, R1_H)

SOLVE = "h o nprob n fcn jac ctx x f ib st"
R1_HOST = "h o newton nprob fcn jac ctx lim x f ib st"
# entry: (family, device symbol, its arguments, host symbol, its arguments, the arrays the device form takes as device pointers)
ENTRIES = {
    "lm": ("lorentz", "nlh_lm_solve_batch_device", "h o nprob m n fcn jac ctx x f ib st", "nlh_lm_solve_batch_device_h", None, "x f"),
    "cls": ("lorentz", "nlh_cls_solve_batch_device", "h o delta stepscale xl xu nprob m n fcn jac ctx x f ib st",
            "nlh_cls_solve_batch_device_h", None, "x f"),
    "covar": ("lorentz", "nlh_lm_covariance_batch_device", "h nprob m n fcn jac ctx x scaled tol cov sigma rank chi2",
              "nlh_lm_covariance_batch_device_h", None, "x cov sigma rank chi2"),
    "newton": ("btri", "nlh_newton_solve_batch_device", SOLVE, "nlh_newton_solve_batch_device_h", None, "x f"),
    "qn": ("btri", "nlh_quasi_newton_solve_batch_device", "h o jdelta nprob n fcn jac ctx x f ib st",
           "nlh_quasi_newton_solve_batch_device_h", None, "x f"),
    "bfgs": ("crosen", "nlh_bfgs_solve_batch_device", SOLVE, "nlh_bfgs_solve_batch_device_h", None, "x"),
    "nm": ("crosen", "nlh_nelder_mead_solve_batch_device", "h o init nprob n fcn ctx x simplex use_simplex f ib st",
           NM_H, "h o init nprob n fcn ctx x f ib st", "x"),
    "brent": ("cubic", "nlh_brent_solve_batch_device", "h o nprob fcn ctx lim x f ib st", R1_H, R1_HOST, "x lim"),
    "n1v": ("cubic", "nlh_newton_1var_solve_batch_device", "h o nprob fcn jac ctx lim x f ib st", R1_H, R1_HOST, "x lim"),
}
INTS = ("nprob", "m", "n", "jdelta", "use_simplex", "newton", "scaled")
REALS = ("delta", "stepscale", "init", "tol")
OUTPUTS = ("x", "f", "ib", "st", "cov", "sigma", "rank", "chi2")
BOX = (np.array([0.4, -1.0, 0.02]), np.array([1.2, 2.0, 0.2]))      # the box of the bounded solver: amplitudes bind
MAX_EVALS = {"bfgs": 500, "nm": 500}                                 # (the other solvers: the default 100)

_raw = None


def _dynamic_symbols(path):
    """The names of a shared library's dynamic symbol table, read from the file itself (no nm on the test machines is
    assumed).  Assumes what hipcc links on x86-64 Linux: a little-endian ELF64 file that keeps its section headers."""
    import struct
    with open(path, "rb") as fh:
        d = fh.read()
    assert d[:5] == b"\x7fELF\x02", path
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", d, 0x3A)
    sec = [struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for s in sec:
        if s[1] == 11:                             # SHT_DYNSYM; its sh_link is the string table
            stroff = sec[s[6]][4]
            for o in range(s[4], s[4] + s[5], s[9]):
                k, = struct.unpack_from("<I", d, o)
                names.append(d[stroff + k:d.index(b"\0", stroff + k)].decode())
    return names


@functools.lru_cache(maxsize=None)
def _mangled(name):
    """The one exported C++ symbol of the function `name` taking a handle first."""
    prefix = "_Z%d%sP10nlh_handle" % (len(name), name)
    found = [s for s in _dynamic_symbols(_lib.LIB_PATH) if s.startswith(prefix)]
    assert len(found) == 1, ("libnonlin_hip.so no longer exports exactly one %s(nlh_handle *, ...): %r -- the host-array twins of "
                             "nelder_mead and the scalar roots are tested through it; bind the tests to its new name" % (name, found))
    return found[0]


def _function(symbol, spec):
    """The symbol with every pointer argument a void pointer, on a library object of this module's own."""
    global _raw
    if _raw is None:
        _lib.load()
        _raw = C.CDLL(_lib.LIB_PATH)
    fn = getattr(_raw, _mangled(symbol) if symbol in INTERNAL else symbol)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32 if k in INTS else C.c_double if k in REALS else C.c_void_p for k in spec.split()]
    return fn


def _addr(v):
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    if hasattr(v, "data_ptr"):
        return v.data_ptr()
    if isinstance(v, (int, C.c_void_p)):
        return v
    if isinstance(v, C._CFuncPtr):
        return C.cast(v, C.c_void_p)
    return C.addressof(v)


def call(entry, host, a):
    """The raw call of an entry point's device or host form with the arguments of dict a; returns its code."""
    fam, dsym, dspec, hsym, hspec, _ = ENTRIES[entry]
    spec = (hspec or dspec) if host else dspec
    return _function(hsym if host else dsym, spec)(*[a[k] if k in INTS + REALS else _addr(a[k]) for k in spec.split()])


class Problems:
    """nprob problems of one family at its smallest shape: the per-problem data, the start, and a context for any subset."""

    def __init__(self, family, nprob, seed=5):
        self.family, self.nprob = family, nprob
        if family == "lorentz":                   # K = 1: n = 3; m = 4: the fewest rows a scaled covariance accepts
            self.m, self.n = 4, 3
            t, y, _, self.x0 = UM.lorentz_problems(nprob, self.m, 1, seed=seed)
            self.data = (t, y)
        elif family == "btri":
            self.m = self.n = 2
            c, self.x0 = UM.btri_problems(nprob, 2, seed=seed)
            self.data = (c,)
        elif family == "crosen":
            self.m, self.n = 1, 2
            c, self.x0 = UM.crosen_problems(nprob, 2, seed=seed)
            self.data = (c,)
        else:                                      # cubic: brackets instead of a start; x comes back
            self.m = self.n = 1
            c, self.lim = SM.cubic_problems(nprob, seed=seed)
            self.data, self.x0 = (c,), np.zeros(nprob)

    def batch(self, sel):
        d = [np.ascontiguousarray(v[sel]) for v in self.data]
        return UM.LorentzBatch(*d) if self.family == "lorentz" else SM.CubicBatch(*d) if self.family == "cubic" else UM.BtriBatch(*d)

    def launchers(self, b, entry, analytic):
        if self.family == "lorentz":
            return b.launch, None
        if self.family == "btri":
            return b.launch, b.launch_jac if analytic else None
        if self.family == "crosen":
            return b.crosen_launch, b.crosen_launch_grad if analytic and entry == "bfgs" else None
        return b.launch, b.launch_diff if analytic and entry == "n1v" else None


def arguments(ds, entry, host, pr, sel, b, analytic=False, opts=None):
    """The accepted call's arguments for the problems sel of pr through the context b, outputs filled with sevens."""
    import torch
    sel = np.arange(pr.nprob)[sel]
    nprob, m, n = len(sel), pr.m, pr.n
    fcn, jac = pr.launchers(b, entry, analytic)
    fshape = {"lm": (nprob, m), "cls": (nprob, m), "newton": (nprob, n), "qn": (nprob, n)}.get(entry, (nprob,))
    a = dict(h=ds.h.ptr, o=opts or ds.options(max_evals=MAX_EVALS.get(entry, 100)), nprob=nprob, m=m, n=n, fcn=fcn, jac=jac,
             ctx=b.ctx, x=np.ascontiguousarray(pr.x0[sel]), f=np.full(fshape, 7.0), ib=np.full((nprob, IB), 7, dtype=np.int32),
             st=np.full(nprob, 7, dtype=np.int32), jdelta=5, delta=1.0, stepscale=1.0, xl=BOX[0], xu=BOX[1], init=1.0,
             simplex=None, use_simplex=0, newton=int(entry == "n1v"), scaled=1, tol=0.0)
    if pr.family == "cubic":
        a["lim"] = np.ascontiguousarray(pr.lim[sel])
    if entry == "covar":
        a.update(cov=np.full((nprob, n, n), 7.0), sigma=np.full((nprob, n), 7.0), rank=np.full(nprob, 7, dtype=np.int32),
                 chi2=np.full(nprob, 7.0))
        del a["f"], a["ib"], a["st"]
    if not host:
        for k in ENTRIES[entry][5].split():
            a[k] = torch.from_numpy(a[k]).to(ds.device)
    return a


def outputs(a):
    """The output arrays of a call's arguments as host arrays."""
    return {k: (a[k] if isinstance(a[k], np.ndarray) else a[k].cpu().numpy()) for k in OUTPUTS if a.get(k) is not None}


def solve(ds, entry, host, pr, sel=slice(None), analytic=False):
    b = pr.batch(sel)
    try:
        a = arguments(ds, entry, host, pr, sel, b, analytic)
        rc = call(entry, host, a)
        assert rc == 0, (entry, host, rc, ds.lib.nlh_last_error(ds.h.ptr))
        return outputs(a)
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ the CPU oracle, one problem
def _ib(ibo):
    return np.array([getattr(ibo, k) for k, _ in ibo._fields_], dtype=np.int32)


def oracle_solve(oracle, entry, pr, p, analytic):
    """Problem p by the CPU oracle driving the family's host twin: the outputs of solve() for that problem."""
    L, so = oracle.lib(), UM.lib()
    m, n = pr.m, pr.n
    oo = oracle.default_options(max_evals=MAX_EVALS.get(entry, 100))
    x, ibo = pr.x0[p].copy(), oracle.IterationBehavior()
    xp = x.ctypes.data_as(dp)
    if pr.family == "lorentz":
        t, y = pr.data
        hc = UM.LorentzHost(m, t[p].ctypes.data_as(dp), y[p].ctypes.data_as(dp), 0)
        fcn, nojac, f = C.cast(so.lorentz_host_fcn, oracle.VECFCN), C.cast(None, oracle.JACFCN), np.zeros(m)
        if entry == "lm":
            rc = L.nlo_lm_solve(C.byref(oo), fcn, nojac, C.byref(hc), m, n, xp, f.ctypes.data_as(dp), C.byref(ibo))
        elif entry == "cls":
            rc = L.nlo_cls_solve(C.byref(oo), C.c_double(1.0), C.c_double(1.0), BOX[0].ctypes.data_as(dp), BOX[1].ctypes.data_as(dp),
                                 fcn, nojac, C.byref(hc), m, n, xp, f.ctypes.data_as(dp), C.byref(ibo))
        else:                                      # F(x), vfh_jac_fcn and lmfactor by the oracle, then the restatement
            fcn(C.cast(C.byref(hc), C.c_void_p), n, xp, m, f.ctypes.data_as(dp))
            J = np.zeros((m, n), order="F")
            assert L.nlo_fd_jacobian(fcn, nojac, C.byref(hc), m, n, xp, f.ctypes.data_as(dp), J.ctypes.data_as(dp)) == 0
            fa, ipvt, rdiag, _ = oracle.lmfactor(J)
            cov, sigma, rank, chi2 = cr.lm_covariance(cr.r_of_lmfactor(fa, rdiag), ipvt, f, scaled=True, tol=None)
            return dict(x=x, cov=np.asarray(cov, dtype=np.float64), sigma=np.asarray(sigma, dtype=np.float64), rank=np.int32(rank),
                        chi2=np.float64(chi2))
        return dict(x=x, f=f, ib=_ib(ibo), st=np.int32(rc))
    c = float(pr.data[0][p])
    if pr.family == "btri":
        hc, f = UM.BtriHost(c, 0, 0), np.zeros(n)
        fcn, jac = C.cast(so.btri_host_fcn, oracle.VECFCN), C.cast(so.btri_host_jac if analytic else None, oracle.JACFCN)
        if entry == "qn":
            rc = L.nlo_quasi_newton_solve(C.byref(oo), 5, fcn, jac, C.byref(hc), n, xp, f.ctypes.data_as(dp), C.byref(ibo))
        else:
            rc = L.nlo_newton_solve(C.byref(oo), fcn, jac, C.byref(hc), n, xp, f.ctypes.data_as(dp), C.byref(ibo))
        return dict(x=x, f=f, ib=_ib(ibo), st=np.int32(rc))
    assert entry == "bfgs"
    f_host = lambda xx: so.crosen_host_f(c, n, np.ascontiguousarray(xx).ctypes.data_as(dp))          # noqa: E731
    g_host = (lambda xx, g: so.crosen_host_grad(c, n, np.ascontiguousarray(xx).ctypes.data_as(dp), g.ctypes.data_as(dp))) if analytic else None
    rc, xo, fo, ibd = oracle.bfgs_solve(f_host, n, x, grad=g_host, opts=oo)
    return dict(x=xo, f=np.float64(fo), ib=np.array([ibd[k] for k, _ in oracle.IterationBehavior._fields_], dtype=np.int32), st=np.int32(rc))


# ------------------------------------------------------------------------------------------------ the check ladders
# What a rung replaces in the accepted call (a batch of two).
FAULT = {
    "H": dict(h=None), "F": dict(fcn=None), "O": dict(o=None), "X": dict(x=None), "V": dict(f=None), "L": dict(lim=None),
    "C": dict(cov=None), "S": dict(use_simplex=1, simplex=None), "P0": dict(nprob=0), "PNEG": dict(nprob=-1),
    "N0": dict(n=0),                              # n < 1
    "NM0": dict(n=3, m=0),                        # n > m and m < 1: which of the two checks comes first
    "NM": dict(n=3, m=2, scaled=0),               # n > m alone
    "SC": dict(scaled=1, n=3, m=3),               # a scaled covariance without a degree of freedom
}
BAD, INV, UNDEF, UNDER = -3, 201, 211, 212
_R1 = [("H", BAD, 0), ("F", UNDEF, 1), ("O", INV, 1), ("PNEG", INV, 0, "P0"), ("L", INV, 1, "P0"), ("X", INV, 1, "P0"), ("P0", 0, 0)]
_SQ = [("H", BAD, 0), ("F", UNDEF, 1), ("P0", 0, 0), ("O", INV, 1), ("X", INV, 1), ("V", INV, 1), ("N0", INV, 1)]
_SQH = [("H", BAD, 0), ("P0", 0, 0), ("O", INV, 0), ("X", INV, 0), ("V", INV, 0), ("N0", INV, 0), ("F", UNDEF, 0)]
_CV = [("H", BAD, 0), ("F", UNDEF, 0), ("P0", 0, 0), ("X", INV, 0), ("C", INV, 0), ("N0", INV, 0), ("SC", INV, 0), ("NM", UNDER, 0)]
# (entry, host form): the rungs in the order the entry point checks them -- (fault, the code it answers with, whether ib
# has been zeroed by then, later rungs the call cannot carry: a NULL array is no fault in a batch of none)
LADDERS = {
    ("lm", False): [("H", BAD, 0), ("F", UNDEF, 1), ("O", INV, 1), ("X", INV, 1, "P0"), ("V", INV, 1, "P0"), ("P0", 0, 0),
                    ("NM0", UNDER, 1), ("N0", INV, 1)],
    ("lm", True): [("H", BAD, 0), ("P0", 0, 0), ("X", INV, 0), ("V", INV, 0), ("O", INV, 0), ("F", UNDEF, 0), ("NM0", UNDER, 0),
                   ("N0", INV, 0)],
    ("cls", False): [("H", BAD, 0), ("F", UNDEF, 1), ("P0", 0, 0), ("O", INV, 1), ("N0", INV, 1), ("NM0", INV, 1), ("X", INV, 1),
                     ("V", INV, 1), ("NM", UNDER, 1)],
    ("cls", True): [("H", BAD, 0), ("P0", 0, 0), ("O", INV, 0), ("X", INV, 0), ("V", INV, 0), ("N0", INV, 0), ("NM0", INV, 0),
                    ("F", UNDEF, 0), ("NM", UNDER, 1)],          # (n > m is the device form's answer: it has zeroed ib)
    ("covar", False): _CV, ("covar", True): _CV,
    ("newton", False): _SQ, ("qn", False): _SQ, ("newton", True): _SQH, ("qn", True): _SQH,
    ("bfgs", False): [("H", BAD, 0), ("F", UNDEF, 1), ("O", INV, 1), ("N0", INV, 1), ("X", INV, 1, "P0"), ("P0", 0, 0)],
    ("bfgs", True): [("H", BAD, 0), ("P0", 0, 0), ("X", INV, 0), ("O", INV, 0), ("N0", INV, 0), ("F", UNDEF, 0)],
    ("nm", False): [("H", BAD, 0), ("F", UNDEF, 1), ("O", INV, 1), ("N0", INV, 1), ("PNEG", INV, 0, "P0"), ("X", INV, 1, "P0"),
                    ("S", INV, 1), ("P0", 0, 0)],
    ("nm", True): [("H", BAD, 0), ("F", UNDEF, 1), ("O", INV, 1), ("N0", INV, 1), ("PNEG", INV, 0, "P0"), ("X", INV, 1, "P0"),
                   ("P0", 0, 0)],
    ("brent", False): _R1, ("brent", True): _R1, ("n1v", False): _R1, ("n1v", True): _R1,
}


def rung_arguments(a, row, i, carry):
    """The accepted call a with the fault of rung i of a row and, with carry, the faults of the later rungs whose code differs."""
    label, code, _, *skip = row[i]
    out = dict(a)
    if carry:
        for lab, c, *_ in reversed(row[i + 1:]):
            if c != code and lab not in skip:
                out.update(FAULT[lab])
    out.update(FAULT[label])
    return out
