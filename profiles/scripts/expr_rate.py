"""What interpreting a formula costs: k_expr_fcn / k_expr_jac (nlh_expr_device_fcn / _jac) against the compiled built-in
k_curve_fcn / k_curve_jac (nlh_curve_device_fcn / _jac) on the same model and data, one launcher call over the whole batch
each, with full least_squares_solver solves beside them.  The model is a sum of two Gaussians on a constant baseline
(K = 2, B = 0, n = 7), written as a formula in the curve table's operation order, so both sides compute the same bits.
The yardstick is the built-in kernels, which this feature does not touch (they are the parent commit's), timed in the
same session.  There is no gate.

    python profiles/scripts/expr_rate.py [--out FILE] [--commit ID] [--append FILE] [--quick]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max).
--append FILE: lines of FILE (what tests/test_gpu_expr.py measured: function accuracy, bound ratios) are copied under the
table.  --quick: 1 warm-up and 3 calls (for a run under rocprofv3 --kernel-trace --stats)."""
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

TERM = "a%d*exp(-0.5*(((t-m%d)/s%d)*((t-m%d)/s%d)))"
FORMULA = "0+" + "+".join(TERM % ((k,) * 5) for k in (1, 2)) + "+c0"
PARAMS = "a1,m1,s1,a2,m2,s2,c0"
ROWS = [(4096, 512), (1 << 16, 64)]                                 # (nprob, m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--append")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    import curve_cases as CC
    import nonlin_amd as nl
    from nonlin_amd import _lib
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    o = ds.options(max_evals=500)
    e = nl.Expr(FORMULA, "t", PARAMS)
    warm, calls = (1, 3) if a.quick else (5, 21)
    lines = ["# formula interpreter against the built-in curve kernels, gauss K = 2, B = 0 (n = 7): ms per call, median (min .. max)",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# formula: {FORMULA}  ({e.ninstr} instructions, depth {e.depth})",
             "# fcn / jac: one launcher call over the whole batch; solve-fd / solve-analytic: nlh_lm_solve_batch_device; ratio = formula / built-in",
             "%-15s %7s %5s %12s %12s %12s %12s %7s" % ("what", "nprob", "m", "builtin ms", "(min..max)", "formula ms", "(min..max)", "ratio")]

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

    for nprob, m in ROWS:
        t, y, xt, x0 = CC.curve_problems("gauss", 2, 0, m, nprob=nprob, seed=2024)
        n = x0.shape[1]
        dt, dy, dx0 = (torch.from_numpy(v).to(ds.device) for v in (t, y, x0))
        dprob = torch.arange(nprob, dtype=torch.int32, device=ds.device)
        F = torch.empty((nprob, m), dtype=torch.float64, device=ds.device)
        J = torch.empty((nprob, n, m), dtype=torch.float64, device=ds.device)
        x = torch.empty_like(dx0)
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        sides = {"builtin": ds.curve_launchers("gauss", 2, 0, dt, dy), "formula": ds.expr_launchers(e, dt, dy)}
        stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
        null = C.cast(None, _lib.DEVFCN)
        got, bits = {}, {}
        for side, (fcn, jac, ctx) in sides.items():
            cp = ds._ctxp(ctx)

            def launch(fn, out):
                assert fn(cp, stream, nprob, C.c_void_p(dprob.data_ptr()), n, C.c_void_p(dx0.data_ptr()), m, C.c_void_p(out.data_ptr())) == 0

            def solve(jc):
                x.copy_(dx0)
                assert ds.lib.nlh_lm_solve_batch_device(ds.h.ptr, C.byref(o), nprob, m, n, fcn, jc, cp, x.data_ptr(), F.data_ptr(), ib, st) == 0
            got[side, "fcn"] = measure(lambda: launch(fcn, F))
            bits[side] = F.clone()
            got[side, "jac"] = measure(lambda: launch(jac, J))
            got[side, "solve-fd"] = measure(lambda: solve(null))
            got[side, "solve-analytic"] = measure(lambda: solve(jac))
            assert all(st[p] == 0 for p in range(nprob))
        assert torch.equal(bits["builtin"].view(torch.int64), bits["formula"].view(torch.int64))     # the same residual bits
        for what in ("fcn", "jac", "solve-fd", "solve-analytic"):
            b, f = got["builtin", what], got["formula", what]
            lines.append("%-15s %7d %5d %12.3f %12s %12.3f %12s %7.2f" % (what, nprob, m, b[0], "%.3f..%.3f" % b[1:], f[0], "%.3f..%.3f" % f[1:],
                                                                     f[0] / b[0]))
            print(lines[-1], flush=True)
        del dt, dy, dx0, F, J, x
        torch.cuda.empty_cache()
    if a.append and os.path.exists(a.append):
        lines.append("# measured by tests/test_gpu_expr.py (device function error in ulp against numpy.longdouble; largest |device - numpy| / bound):")
        lines += ["# " + ln.rstrip() for ln in open(a.append)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
