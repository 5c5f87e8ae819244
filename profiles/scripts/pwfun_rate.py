"""What pow, atan2, min, max and where cost: k_expr_fcn / k_expr_jac (nlh_expr_device_fcn / _jac), one launcher call over the
whole batch each, of an existing formula (gauss2d of tests/expr_cases.py), which does not use the new instructions -- the
same rows from a build of the parent commit (--lib, --existing-only) show what the larger dispatch costs the formulas that
were there before --, then of the power law against its exp(b*log(t)) form and of the hinge against 0.5*(u+abs(u))
(tests/pwfun_cases.py).  There is no gate.

    python profiles/scripts/pwfun_rate.py [--out FILE] [--commit ID] [--lib LIBRARY] [--existing-only] [--append FILE]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max), the
procedure of profiles/scripts/specfun_rate.py.  --lib LIBRARY: load that libnonlin_hip.so instead of the package's (a parent
build).  --out FILE: appended to, so that the parent's rows, this commit's and the parent's again
stand in the order they were measured in.  --existing-only: the gauss2d rows alone.  --append FILE: lines of FILE (what
tests/test_gpu_pwfun.py measured) are copied under the table."""
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

ROWS = [(4096, 512), (1 << 16, 64)]                                 # (nprob, m)
PAIRS = (("powerlaw_explog", "powerlaw"), ("hinge_abs", "hinge"))


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
    import expr_cases as EC
    ds = DeviceSolver(0)
    warm, calls = 5, 21
    lines = []
    if not (a.out and os.path.exists(a.out)):                       # (the first run into a file heads it)
        lines += ["# pow, atan2, min, max and where in formulas: ms per call, median (min .. max) of 21 calls after 5 warm-ups, HIP events",
                  f"# {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}"]

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(call):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        ms = [timed(call) for _ in range(calls)]
        return statistics.median(ms), min(ms), max(ms)

    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)

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

    # an existing formula: these rows are the ones to compare between commits
    lines += [f"# {a.commit}" + (f" (library {os.path.basename(os.path.dirname(a.lib))}/{os.path.basename(a.lib)})" if a.lib else "")
              + ": k_expr_fcn / k_expr_jac of gauss2d, a formula without the new instructions", head]
    for nprob, m in ((4096, 484), (1 << 16, 64)):
        prog, t, y, xt, x0 = EC.expr_problems("gauss2d", m, nprob=64, seed=3)
        rep = nprob // 64
        t, y, x0 = np.tile(t, (1, rep, 1)), np.tile(y, (rep, 1)), np.tile(x0, (rep, 1))
        rows("gauss2d", nprob, m, *kernels(EC.compile_formula("gauss2d"), t, y, x0, nprob, m))

    if not a.existing_only:
        import pwfun_cases as PC
        lines += ["# the power law a*pow(t,b)+c against a*exp(b*log(t))+c, the hinge with max(t-t0,0) against 0.5*((t-t0)+abs(t-t0)); t > 0", head]
        for nprob, m in ROWS:
            for pair in PAIRS:
                for name in pair:
                    prog, t, y, xt, x0 = PC.problems(name, m, nprob=64, seed=3)
                    rep = nprob // 64
                    t, y, x0 = np.tile(t, (1, rep, 1)), np.tile(y, (rep, 1)), np.tile(x0, (rep, 1))
                    rows(name, nprob, m, *kernels(PC.compile_formula(name), t, y, x0, nprob, m))
    if a.append and os.path.exists(a.append):
        lines.append("# measured by tests/test_gpu_pwfun.py (device function error in ulp against numpy.longdouble; largest |device - numpy| / bound):")
        lines += ["# " + ln.rstrip() for ln in open(a.append)]
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
