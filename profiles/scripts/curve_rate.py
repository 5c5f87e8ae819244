"""LM iterations per second of least_squares_solver on the built-in curve models (nlh_curve_device_fcn / _jac), with forward
differences and with the analytic Jacobian, next to the yardstick of the Lorentzian row: the same spectra through the
user-written family of tests/device_model (lorentz_launch) -- a path this library's curve models do not touch -- timed in
the same session.

    python profiles/scripts/curve_rate.py [--out FILE] [--commit ID] [--trace] [--append FILE]

One process on the GPU.  HIP events around the library call (nlh_lm_solve_batch_device on preallocated arrays, x reset by
a device copy inside the bracket), 5 warm-up calls, then 21 timed calls: median (min .. max).  A row whose solve takes
longer than SLOW_MS is timed with 1 warm-up and 5 calls instead (the long-tailed Lorentzian batch runs for seconds per
solve) and says so in its `calls` column.  LM it/s = sum of the problems' iter_count / time; rounds = the largest
iter_count of the batch (a lock-step batch runs at least that many rounds).  --trace: built-in rows only, one warm-up
and two calls (for a run under rocprofv3 --kernel-trace --stats).  --append FILE: lines of FILE (the tests' observed
rounding-bound ratios) are copied under the table."""
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

SLOW_MS = 1000.0
# (label, kind, K, B, nprob, m)
ROWS = [("lorentz", "lorentz", 8, -1, 4096, 2048), ("gauss", "gauss", 1, -1, 1 << 16, 64), ("expdecay", "expdecay", 2, 0, 1 << 14, 400)]


def problems(kind, K, B, nprob, m):
    import curve_cases as CC
    import user_models as UM
    if kind == "lorentz":                                            # the spectra DESIGN section 0 quotes for the user family
        return UM.lorentz_problems(nprob, m, K, seed=2024)
    return CC.curve_problems(kind, K, B, m, nprob=nprob, seed=2024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--append")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import torch
    import user_models as UM
    from nonlin_amd import _lib
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    o = ds.options(max_evals=500)
    lines = ["# least_squares_solver on the built-in curve models: LM it/s, ms per solve: median (min .. max) of the timed calls",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             "# jacobian: user-fd = the user-written Lorentzian family of tests/device_model (the yardstick), fd / analytic = built-in",
             "%-9s %7s %5s %3s %-9s %6s %12s %10s %10s %10s %7s %8s" % ("model", "nprob", "m", "n", "jacobian", "calls", "LM it/s", "ms median",
                                                                         "ms min", "ms max", "rounds", "status0")]
    for label, kind, K, B, nprob, m in ROWS:
        t, y, xt, x0 = problems(kind, K, B, nprob, m)
        n = x0.shape[1]
        dt, dy = torch.from_numpy(t).to(ds.device), torch.from_numpy(y).to(ds.device)
        dx0 = torch.from_numpy(x0).to(ds.device)
        x, f = torch.empty_like(dx0), torch.empty((nprob, m), dtype=torch.float64, device=ds.device)
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
        null = C.cast(None, _lib.DEVFCN)
        variants = [("fd", fcn, null, ds._ctxp(ctx)), ("analytic", fcn, jac, ds._ctxp(ctx))]
        lb = None
        if kind == "lorentz" and not a.trace:
            lb = UM.LorentzBatch(t, y)
            variants.insert(0, ("user-fd", ds._devfcn(lb.launch), null, lb.ctx))
        for name, fc, jc, cp in variants:
            def call():
                x.copy_(dx0)
                rc = ds.lib.nlh_lm_solve_batch_device(ds.h.ptr, C.byref(o), nprob, m, n, fc, jc, cp, x.data_ptr(), f.data_ptr(), ib, st)
                assert rc == 0

            def timed():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            first = timed()                                          # (the first warm-up, and the size of the row)
            slow = first > SLOW_MS
            warm, calls = (0, 2) if a.trace else ((0, 5) if slow else (4, 21))
            for _ in range(warm):
                call()
            torch.cuda.synchronize()
            ms = [timed() for _ in range(calls)]
            its = np.array([ib[p].iter_count for p in range(nprob)])
            ok = sum(1 for p in range(nprob) if st[p] == 0)
            med, lo, hi = statistics.median(ms), min(ms), max(ms)
            lines.append("%-9s %7d %5d %3d %-9s %6s %12.5g %10.2f %10.2f %10.2f %7d %8d" % (
                label, nprob, m, n, name, "%d+%d" % (warm + 1, calls), its.sum() / med * 1e3, med, lo, hi, its.max(), ok))
            print(lines[-1], flush=True)
        if lb is not None:
            lb.close()
        del dt, dy, dx0, x, f
        torch.cuda.empty_cache()
    if a.append and os.path.exists(a.append):
        lines.append("# largest observed |device - numpy| / bound of the exp kinds (tests/test_gpu_curve.py, item 4 of its list):")
        lines += ["# " + ln.rstrip() for ln in open(a.append)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
