"""What the special functions cost: k_expr_fcn / k_expr_jac (nlh_expr_device_fcn / _jac) of a single-Voigt formula against
the Lorentzian formula of the same parameter count, one launcher call over the whole batch each; the one-call fit of 16,384
Voigt peaks; and k_expr_jac of an existing formula (gauss2d of tests/expr_cases.py), which does not use the new
instructions, so that the same rows from a build of the parent commit (--lib, --existing-only) show what the larger
dispatch costs the formulas that were there before.  There is no gate.

    python profiles/scripts/specfun_rate.py [--out FILE] [--commit ID] [--lib LIBRARY] [--existing-only] [--append FILE]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max).
--lib LIBRARY: load that libnonlin_hip.so instead of the package's (a parent build).  --existing-only: the gauss2d rows
alone, appended to --out.  --append FILE: lines of FILE (what tests/test_gpu_specfun.py measured) are copied under the
table."""
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
FIT = (16384, 200)


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
    if a.lib:                                                       # (a parent build lacks the newer symbols: bind what it has)
        _lib.LIB_PATH = os.path.abspath(a.lib)
        other = C.CDLL(_lib.LIB_PATH)
        for name in [k for k in _lib.SYMBOLS if not hasattr(other, k)]:
            del _lib.SYMBOLS[name]
    import nonlin_amd as nl
    from nonlin_amd.device import DeviceSolver
    import expr_cases as EC
    ds = DeviceSolver(0)
    warm, calls = 5, 21
    lines = []
    if not a.existing_only:
        lines += ["# special functions in formulas: ms per call, median (min .. max) of 21 calls after 5 warm-ups, HIP events",
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

    # an existing formula: this row is the one to compare between commits
    lines += [f"# commit {a.commit}" + (f" (library {a.lib})" if a.lib else "") + ": k_expr_fcn / k_expr_jac of gauss2d, a formula without the new instructions",
              head]
    for nprob, m in ((4096, 484), (1 << 16, 64)):
        prog, t, y, xt, x0 = EC.expr_problems("gauss2d", m, nprob=64, seed=3)
        rep = nprob // 64
        t, y, x0 = np.tile(t, (1, rep, 1)), np.tile(y, (rep, 1)), np.tile(x0, (rep, 1))
        f, j = kernels(EC.compile_formula("gauss2d"), t, y, x0, nprob, m)
        lines.append(fmt % ("gauss2d fcn", nprob, m, f[0], "%.3f..%.3f" % f[1:]))
        lines.append(fmt % ("gauss2d jac", nprob, m, j[0], "%.3f..%.3f" % j[1:]))
        print("\n".join(lines[-2:]), flush=True)

    if not a.existing_only:
        import specfun_cases as SC
        lines += ["# a single Voigt peak against the Lorentzian formula of the same parameter count (n = 5)", head]
        for nprob, m in ROWS:
            for name in ("lorentz1", "voigt1"):
                prog, t, y, xt, x0 = SC.problems(name, m, nprob=64, seed=3)
                rep = nprob // 64
                t, y, x0 = np.tile(t, (1, rep, 1)), np.tile(y, (rep, 1)), np.tile(x0, (rep, 1))
                f, j = kernels(SC.compile_formula(name), t, y, x0, nprob, m)
                lines.append(fmt % (name + " fcn", nprob, m, f[0], "%.3f..%.3f" % f[1:]))
                lines.append(fmt % (name + " jac", nprob, m, j[0], "%.3f..%.3f" % j[1:]))
                print("\n".join(lines[-2:]), flush=True)
        nprob, m = FIT
        e = SC.compile_formula("voigt1")
        prog, t, y, xt, x0 = SC.problems("voigt1", m, nprob=64, seed=SC.RECOVERY_SEED, gaussian=SC.RECOVERY_NOISE)
        rep = nprob // 64
        dt, dy, dx0 = (torch.from_numpy(np.ascontiguousarray(v)).to(ds.device) for v in (np.tile(t, (1, rep, 1)), np.tile(y, (rep, 1)), np.tile(x0, (rep, 1))))
        o = ds.options(max_evals=500)
        for analytic in (True, False):
            status = []

            def fit():
                status[:] = ds.expr_fit_batch(e, dt, dy, dx0, analytic=analytic, opts=o)[7]
            r = measure(fit)
            assert set(status) == {0}
            lines.append(fmt % ("voigt1 fit + errors, " + ("analytic" if analytic else "forward differences"), nprob, m, r[0], "%.3f..%.3f" % r[1:]))
            print(lines[-1], flush=True)
    if a.append and os.path.exists(a.append):
        lines.append("# measured by tests/test_gpu_specfun.py (device function error in ulp against the 40-digit fixture; largest |device - numpy| / bound):")
        lines += ["# " + ln.rstrip() for ln in open(a.append)]
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "a" if a.existing_only else "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
