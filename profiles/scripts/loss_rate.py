"""What a robust loss costs (nlh_loss_*): the row-scaling kernel k_loss_jac alone, as a fraction of the
read + write stream rate this part delivers, and a full Lorentzian fit with a Huber loss against the same fit without a
loss on the same spiked data (tests/loss_cases.py), in the same session.

    python profiles/scripts/loss_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max).
The row scaling is timed through nlh_loss_device_jac with a dprob and with inner launchers that launch nothing (the
scratch residual and the caller's Jacobian keep whatever they held: the kernel's time does not depend on the values, Huber's
branch aside), so a call launches k_loss_jac alone; bytes = 8 m (2 n + 1) per point.  The inner launchers are Python
callbacks, two per call, whose host time would sit between the events; so for these rows a spin kernel of about a millisecond
is enqueued ahead of the first event and the host runs ahead of the device: the events then bracket device time only."""
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
KERNEL_ROWS = [(4096, 2048, 24), (1 << 16, 64, 9)]      # (points, m, n)
FIT_ROWS = [(1 << 14, 64, 4), (4096, 200, 12)]          # (nprob, m, outliers per spectrum)


def bracket(torch, call, warm=4, calls=21, ahead=0):
    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if ahead:
            torch.cuda._sleep(ahead)                                    # device cycles: the host gets ahead of the stream
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
    import loss_cases as LC
    from nonlin_amd import _lib
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = ["# robust losses: the row-scaling kernel alone, and full Lorentzian fits with and without a Huber loss; ms: median (min .. max) of 21 calls after 5",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# k_loss_jac through nlh_loss_device_jac with a dprob, inner launchers no-ops, host ahead of the device (a spin kernel before the first event); stream rate {STREAM_GBS:.0f} GB/s",
             "%7s %5s %3s %-8s %10s %10s %10s %10s %9s" % ("points", "m", "n", "kind", "ms median", "ms min", "ms max", "GB/s", "of stream")]
    noop = _lib.DEVFCN(lambda c, s, npts, dprob, n, dX, m, out: 0)
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    for npts, m, n in KERNEL_ROWS:
        X = torch.ones((npts, n), dtype=torch.float64, device=ds.device)
        J = torch.ones((npts, n, m), dtype=torch.float64, device=ds.device)
        plist = torch.arange(npts, dtype=torch.int32, device=ds.device)
        for kind in ("huber", "soft_l1"):
            wf, wj, wctx = ds.loss_launchers(nl.Loss(kind, 1.0), noop, noop, None)

            def call():
                rc = ds.lib.nlh_loss_device_jac(wctx.ptr, stream, npts, plist.data_ptr(), n, X.data_ptr(), m, J.data_ptr())
                assert rc == 0
            med, lo, hi = bracket(torch, call, ahead=2_000_000)
            gbs = 8.0 * m * (2 * n + 1) * npts / (med * 1e-3) / 1e9
            lines.append("%7d %5d %3d %-8s %10.3f %10.3f %10.3f %10.0f %9.2f" % (npts, m, n, kind, med, lo, hi, gbs, gbs / STREAM_GBS))
            print(lines[-1], flush=True)
            wctx.close()
        del X, J, plist
        torch.cuda.empty_cache()
    lines += ["# least_squares_solver on a Lorentzian on a constant with spikes (tests/loss_cases.py), the same data with and without the loss",
              "%7s %5s %3s %-16s %12s %10s %10s %10s %7s %8s %10s" % ("nprob", "m", "n", "fit", "LM it/s", "ms median", "ms min", "ms max", "rounds",
                                                                      "status0", "worst err")]
    o = ds.options(max_evals=500)
    null = C.cast(None, _lib.DEVFCN)
    for nprob, m, nout in FIT_ROWS:
        t, y, xt, x0 = LC.outlier_problems(m, nout, nprob=nprob, seed=2024)
        dt, dy, dx0 = (torch.from_numpy(v).to(ds.device) for v in (t, y, x0))
        fcn, jac, ctx = ds.curve_launchers(LC.KIND, LC.K, LC.B, dt, dy)
        wf, wj, wctx = ds.loss_launchers(nl.Loss("huber", LC.SCALE), fcn, jac, ctx)
        f = torch.empty((nprob, m), dtype=torch.float64, device=ds.device)
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        variants = [("plain fd", fcn, null, ds._ctxp(ctx)), ("plain analytic", fcn, jac, ds._ctxp(ctx)),
                    ("huber fd", wf, null, wctx.ptr), ("huber analytic", wf, wj, wctx.ptr)]
        for label, fc, jc, cp in variants:
            x = torch.empty_like(dx0)

            def call():
                x.copy_(dx0)
                rc = ds.lib.nlh_lm_solve_batch_device(ds.h.ptr, C.byref(o), nprob, m, 4, fc, jc, cp, x.data_ptr(), f.data_ptr(), ib, st)
                assert rc == 0
            med, lo, hi = bracket(torch, call)
            its = np.array([ib[p].iter_count for p in range(nprob)])
            ok = sum(1 for p in range(nprob) if st[p] == 0)
            err = float(np.abs(x.cpu().numpy() - xt).max())
            lines.append("%7d %5d %3d %-16s %12.5g %10.2f %10.2f %10.2f %7d %8d %10.3g" % (nprob, m, 4, label, its.sum() / med * 1e3, med, lo, hi,
                                                                                         its.max(), ok, err))
            print(lines[-1], flush=True)
        wctx.close()
        del dt, dy, dx0, f
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
