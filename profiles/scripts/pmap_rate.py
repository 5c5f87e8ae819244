"""What a parameter map costs and buys (nlh_pmap_*): the contraction kernel k_pmap_jac alone, as a fraction
of the read + write stream rate this part delivers, and full Lorentzian fits three ways on the same data -- mapped with
forward differences, mapped with the analytic Jacobian, unmapped -- in the same session.

    python profiles/scripts/pmap_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max).
The contraction is timed through nlh_pmap_device_jac with an inner Jacobian launcher that launches nothing (the scratch
Jacobian keeps whatever it held: the kernel's time does not depend on the values), so a call is k_pmap_expand -- a few
microseconds -- and k_pmap_jac, in as many slices as the 1 GiB scratch cap makes; bytes = 8 m (columns read + columns
written) per point."""
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

STREAM_GBS = 5018.0                     # profiles/r04_ubench.txt: the read + write stream rate this part delivers
# (K, B, nprob, m, map): the widths of peaks 2 .. 5 tied to peak 1 (24 -> 20); the baseline fixed (9 -> 6)
KERNEL_ROWS = [(8, -1, 4096, 2048, "tied4"), (2, 2, 1 << 16, 64, "fixed_baseline")]
FIT_ROWS = [(4, -1, 4096, 512, "tied_widths"), (2, 2, 1 << 14, 301, "both")]


def spec(name, K, B):
    import pmap_cases as PC
    if name == "tied4":
        return [], {3 * k + 2: (2, PC.width_scale(k), 0.0) for k in range(1, 5)}
    return PC.map_spec(name, K, B)


def bracket(torch, call, warm=4, calls=21):
    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    timed()
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ms = [timed() for _ in range(calls)]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import torch
    import nonlin_amd as nl
    import pmap_cases as PC
    import pmap_restatement as PR
    from nonlin_amd import _lib
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = ["# parameter maps: the contraction kernel alone, and full Lorentzian fits mapped and unmapped; ms: median (min .. max) of 21 calls after 5",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# k_pmap_jac (with k_pmap_expand) through nlh_pmap_device_jac, inner Jacobian launcher a no-op; stream rate {STREAM_GBS:.0f} GB/s",
             "%7s %5s %3s %3s %5s %7s %10s %10s %10s %10s %9s" % ("points", "m", "N", "n", "read", "slices", "ms median", "ms min", "ms max", "GB/s",
                                                                  "of stream")]
    noop = _lib.DEVFCN(lambda c, s, npts, dprob, n, dX, m, dJ: 0)
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    for K, B, npts, m, name in KERNEL_ROWS:
        N = 3 * K + B + 1
        T = PR.tables(N, *spec(name, K, B))
        pm = nl.ParamMap(N, *spec(name, K, B))
        n = pm.nfree
        jk, g = PR.factors(T)
        read = int((jk >= 0).sum())
        full = torch.ones((N,), dtype=torch.float64, device=ds.device)
        X = torch.ones((npts, n), dtype=torch.float64, device=ds.device)
        J = torch.empty((npts, n, m), dtype=torch.float64, device=ds.device)
        fcn = C.cast(ds.lib.nlh_curve_device_fcn, _lib.DEVFCN)          # (never called: only the Jacobian launcher is)
        wf, wj, wctx = ds.pmap_launchers(pm, fcn, noop, None, full)

        def call():
            rc = ds.lib.nlh_pmap_device_jac(wctx.ptr, stream, npts, None, n, X.data_ptr(), m, J.data_ptr())
            assert rc == 0
        med, lo, hi = bracket(torch, call)
        per = 8 * N * (m + 1) + 4
        slices = -(-npts // max(1, min(npts, (1 << 30) // per)))
        gbs = 8.0 * m * (read + n) * npts / (med * 1e-3) / 1e9
        lines.append("%7d %5d %3d %3d %5d %7d %10.3f %10.3f %10.3f %10.0f %9.2f" % (npts, m, N, n, read, slices, med, lo, hi, gbs, gbs / STREAM_GBS))
        print(lines[-1], flush=True)
        wctx.close()
        del X, J
        torch.cuda.empty_cache()
    lines += ["# least_squares_solver on Lorentzian data whose truth obeys the ties (tests/pmap_cases.py), the same data three ways",
              "%-12s %7s %5s %3s %3s %-15s %12s %10s %10s %10s %7s %8s" % ("map", "nprob", "m", "N", "n", "jacobian", "LM it/s", "ms median", "ms min",
                                                                       "ms max", "rounds", "status0")]
    o = ds.options(max_evals=500)
    null = C.cast(None, _lib.DEVFCN)
    for K, B, nprob, m, name in FIT_ROWS:
        N = 3 * K + B + 1
        t, y, xt, x0 = PC.problems("lorentz", K, B, m, nprob=nprob, seed=2024)
        T = PR.tables(N, *PC.map_spec(name, K, B))
        pm = nl.ParamMap(N, *PC.map_spec(name, K, B))
        n = pm.nfree
        full = PC.full_start(T, xt, x0)
        dt, dy, dfull = (torch.from_numpy(v).to(ds.device) for v in (t, y, full))
        fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, dt, dy)
        wf, wj, wctx = ds.pmap_launchers(pm, fcn, jac, ctx, dfull)
        xs = ds.pmap_gather(pm, dfull)
        f = torch.empty((nprob, m), dtype=torch.float64, device=ds.device)
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        variants = [("mapped fd", n, wf, null, wctx.ptr, xs), ("mapped analytic", n, wf, wj, wctx.ptr, xs),
                    ("unmapped fd", N, fcn, null, ds._ctxp(ctx), dfull), ("unmapped analytic", N, fcn, jac, ds._ctxp(ctx), dfull)]
        for label, nn, fc, jc, cp, start in variants:
            x = torch.empty_like(start)

            def call():
                x.copy_(start)
                rc = ds.lib.nlh_lm_solve_batch_device(ds.h.ptr, C.byref(o), nprob, m, nn, fc, jc, cp, x.data_ptr(), f.data_ptr(), ib, st)
                assert rc == 0
            med, lo, hi = bracket(torch, call)
            its = np.array([ib[p].iter_count for p in range(nprob)])
            ok = sum(1 for p in range(nprob) if st[p] == 0)
            lines.append("%-12s %7d %5d %3d %3d %-15s %12.5g %10.2f %10.2f %10.2f %7d %8d" % (name, nprob, m, N, nn, label, its.sum() / med * 1e3, med,
                                                                                            lo, hi, its.max(), ok))
            print(lines[-1], flush=True)
        wctx.close()
        del dt, dy, dfull, f
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
