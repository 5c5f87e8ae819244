"""What j0, j1, i0e, i1e, lgamma, expm1 and log1p cost: k_expr_fcn / k_expr_jac (nlh_expr_device_fcn / _jac), one launcher
call over the whole batch each, of two existing formulas -- the Lorentzian of tests/specfun_cases.py and the power law of
tests/pwfun_cases.py, which do not use the new instructions and run the older instantiations; the same rows from a build of
the parent commit (--lib, --existing-only) show whether they still run at the parent's rate --, then of the Airy pattern, the
von Mises distribution and the gamma pdf (tests/specfun2_cases.py), and a 16,384-problem Airy fit with standard errors
(nlh_expr_fit_batch).  There is no gate.

    python profiles/scripts/specfun2_rate.py [--out FILE] [--commit ID] [--lib LIBRARY] [--existing-only] [--append FILE]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max), the
procedure of profiles/scripts/pwfun_rate.py (the fit: 2 warm-ups, 7 calls).  --lib LIBRARY: load that libnonlin_hip.so instead
of the package's (a parent build).  --out FILE: appended to, so that the parent's rows, this commit's and the parent's again
stand in the order they were measured in.  --existing-only: the older formulas' rows alone.  --append FILE: lines of FILE
(what tests/test_gpu_specfun2.py measured) are copied under the table."""
import argparse
import ctypes as C
import datetime
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NPROB, M = 4096, 512
FIT_NPROB, FIT_M = 1 << 14, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--lib")
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--append")
    a = ap.parse_args()
    import torch
    from nonlin_amd import _lib
    if a.lib:                                                       # (a parent build may lack newer symbols: bind what it has)
        _lib.LIB_PATH = os.path.abspath(a.lib)
        other = C.CDLL(_lib.LIB_PATH)
        for name in [k for k in _lib.SYMBOLS if not hasattr(other, k)]:
            del _lib.SYMBOLS[name]
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = []
    if not (a.out and os.path.exists(a.out)):                       # (the first run into a file heads it)
        lines += ["# j0, j1, i0e, i1e, lgamma, expm1 and log1p in formulas: ms per call, median (min .. max) of 21 calls after 5 warm-ups, HIP events",
                  f"# {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}"]

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(call, warm=5, calls=21):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        ms = [timed(call) for _ in range(calls)]
        return statistics.median(ms), min(ms), max(ms)

    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)

    def tiled(t, y, x0, nprob):
        rep = nprob // 64
        return np.tile(t, (1, rep, 1)), np.tile(y, (rep, 1)), np.tile(x0, (rep, 1))

    def kernels(e, t, y, x0, nprob, m):
        """(fcn, jac) timings of one launcher call over the whole batch."""
        n = x0.shape[1]
        dt, dy, dx0 = (torch.from_numpy(np.ascontiguousarray(v)).to(ds.device) for v in (t, y, x0))
        dprob = torch.arange(nprob, dtype=torch.int32, device=ds.device)
        F = torch.empty((nprob, m), dtype=torch.float64, device=ds.device)
        J = torch.empty((nprob, n, m), dtype=torch.float64, device=ds.device)
        fcn, jac, ctx = ds.expr_launchers(e, dt, dy)
        cp = ds._ctxp(ctx)

        def launch(fn, out):
            assert fn(cp, stream, nprob, C.c_void_p(dprob.data_ptr()), n, C.c_void_p(dx0.data_ptr()), m, C.c_void_p(out.data_ptr())) == 0
        return measure(lambda: launch(fcn, F)), measure(lambda: launch(jac, J))

    fmt = "%-34s %7d %5d %10.3f %16s"
    head = "%-34s %7s %5s %10s %16s" % ("what", "nprob", "m", "ms", "(min..max)")

    def rows(name, nprob, m, f, j):
        lines.append(fmt % (name + " fcn", nprob, m, f[0], "%.3f..%.3f" % f[1:]))
        lines.append(fmt % (name + " jac", nprob, m, j[0], "%.3f..%.3f" % j[1:]))
        print("\n".join(lines[-2:]), flush=True)

    # existing formulas: these rows are the ones to compare between commits
    import pwfun_cases as PC
    import specfun_cases as OC
    lines += [f"# {a.commit}" + (f" (library {os.path.basename(os.path.dirname(a.lib))}/{os.path.basename(a.lib)})" if a.lib else "")
              + ": k_expr_fcn / k_expr_jac of formulas without the new instructions", head]
    for cases, name in ((OC, "lorentz1"), (PC, "powerlaw")):
        prog, t, y, xt, x0 = cases.problems(name, M, nprob=64, seed=3)
        rows(name, NPROB, M, *kernels(cases.compile_formula(name), *tiled(t, y, x0, NPROB), NPROB, M))

    if not a.existing_only:
        import specfun2_cases as SC
        lines += ["# the Airy pattern (j1), the von Mises distribution (i0e beside exp and cos), the gamma pdf (lgamma; digamma in the Jacobian)", head]
        for name in ("airy", "vonmises", "gammapdf"):
            prog, t, y, xt, x0 = SC.problems(name, M, nprob=64, seed=3)
            rows(name, NPROB, M, *kernels(SC.compile_formula(name), *tiled(t, y, x0, NPROB), NPROB, M))
        e = SC.compile_formula("airy")
        prog, t, y, xt, x0 = SC.problems("airy", FIT_M, nprob=64, seed=3, gaussian=0.02)
        dt, dy, dx0 = (torch.from_numpy(np.ascontiguousarray(v)).to(ds.device) for v in tiled(t, y, x0, FIT_NPROB))
        st = []

        def fit():
            st[:] = [ds.expr_fit_batch(e, dt, dy, dx0, opts=ds.options(max_evals=SC.MAX_EVALS))[7]]
        f = measure(fit, warm=2, calls=7)
        lines += [f"# expr_fit_batch of the Airy pattern with standard errors, analytic Jacobian; {sum(1 for s in st[0] if s == 0)} of {FIT_NPROB} return 0", head,
                  fmt % ("airy fit + errors", FIT_NPROB, FIT_M, f[0], "%.3f..%.3f" % f[1:])]
        print(lines[-1], flush=True)
    if a.append and os.path.exists(a.append):
        lines.append("# measured by tests/test_gpu_specfun2.py (device function error in ulp of its scale against the 40-digit fixture; largest |device - numpy| / bound):")
        lines += ["# " + ln.rstrip() for ln in open(a.append)]
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
