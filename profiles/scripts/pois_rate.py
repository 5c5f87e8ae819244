"""What a Poisson fit costs (nlh_pois_*): the row-scaling kernel k_pois_jac against the robust losses'
k_loss_jac at the same (points, m, n) in the same session -- the byte ratio (2 n + 3) / (2 n + 1) is the expectation: the
Poisson kernel also reads y and the mask --, both as a fraction of the read + write stream rate this part delivers, and a
full decay fit minimising the Poisson deviance against the weighted least-squares fit of the same counts
(tests/pois_cases.py).

    python profiles/scripts/pois_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max).
The row scalings are timed through nlh_pois_device_jac / nlh_loss_device_jac with a dprob and with inner launchers that
launch nothing, so a call launches the one kernel alone; the first call's inner residual launcher copies realistic raw
residuals (Poisson counts around a decay) into the context's scratch, which later calls find as it was: the branches of the
table are taken in the mix a fit sees.  The rows are sized past the last-level cache (KERNEL_ROWS).  bytes = 8 m (2 n + 3) per point (k_loss_jac: 8 m (2 n + 1)).  The inner launchers are
Python callbacks, two per call, whose host time would sit between the events; so for these rows a spin kernel of about a
millisecond is enqueued ahead of the first event and the host runs ahead of the device: the events then bracket device time
only."""
import argparse
import ctypes as C
import datetime
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from loss_rate import STREAM_GBS, bracket  # noqa: E402

# (points, m, n): every row's working set -- J, the scratch residual, y and the mask, 8 m (n + 3) bytes per point -- is 1.6 GB or
# more, several times the 256 MiB Infinity Cache, so that a call's bytes come from and go to HBM
KERNEL_ROWS = [(4096, 2048, 24), (1 << 18, 64, 9), (1 << 19, 64, 3)]
FIT_ROWS = [(1 << 14, 50.0), (1 << 14, 1000.0)]                            # (nprob, amplitude)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import torch
    import nonlin_amd as nl
    import pois_cases as PC
    from nonlin_amd import _lib
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lines = ["# Poisson fits: the row-scaling kernel against the robust losses', and full decay fits by deviance and by weighted least squares; ms: median (min .. max) of 21 calls after 5",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# through nlh_*_device_jac with a dprob, inner launchers no-ops, host ahead of the device (a spin kernel before the first event); stream rate {STREAM_GBS:.0f} GB/s",
             "%7s %5s %3s %-10s %10s %10s %10s %10s %9s %12s" % ("points", "m", "n", "kernel", "ms median", "ms min", "ms max", "GB/s", "of stream",
                                                               "time / loss")]
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    rng = np.random.default_rng(1)
    for npts, m, n in KERNEL_ROWS:
        X = torch.ones((npts, n), dtype=torch.float64, device=ds.device)
        J = torch.ones((npts, n, m), dtype=torch.float64, device=ds.device)
        plist = torch.arange(npts, dtype=torch.int32, device=ds.device)
        mu = 50.0 * np.exp(-np.linspace(0.0, 4.0, m)) + 0.5
        yh = rng.poisson(np.broadcast_to(mu, (npts, m))).astype(np.float64)
        y = torch.from_numpy(yh).to(ds.device)
        r = torch.from_numpy(mu[None, :] * (1.0 + 0.05 * rng.standard_normal((npts, 1))) - yh).to(ds.device)
        w = torch.ones_like(y)
        fill = [True]

        def inner_fcn(c, s, np_, dprob, n_, dX, m_, out):
            if fill[0]:                                                 # once: the scratch then holds raw residuals of counts
                hip.hipMemcpyAsync(out, r.data_ptr(), 8 * np_ * m_, 3, s)
                fill[0] = False
            return 0
        noop = _lib.DEVFCN(lambda c, s, np_, dprob, n_, dX, m_, out: 0)
        filler = _lib.DEVFCN(inner_fcn)
        base = None
        for kernel in ("k_loss_jac", "k_pois_jac"):
            if kernel == "k_loss_jac":
                wf, wj, wctx = ds.loss_launchers(nl.Loss("soft_l1", 1.0), filler, noop, None)
                entry, nbytes = ds.lib.nlh_loss_device_jac, 8.0 * m * (2 * n + 1) * npts
            else:
                wf, wj, wctx = ds.pois_launchers(nl.Poisson(), filler, noop, None, y, w)
                entry, nbytes = ds.lib.nlh_pois_device_jac, 8.0 * m * (2 * n + 3) * npts
            fill[0] = True

            def call():
                rc = entry(wctx.ptr, stream, npts, plist.data_ptr(), n, X.data_ptr(), m, J.data_ptr())
                assert rc == 0
                J.fill_(1.0)
            call()
            torch.cuda.synchronize()

            def timed_call():
                rc = entry(wctx.ptr, stream, npts, plist.data_ptr(), n, X.data_ptr(), m, J.data_ptr())
                assert rc == 0
            med, lo, hi = bracket(torch, timed_call, ahead=2_000_000)
            gbs = nbytes / (med * 1e-3) / 1e9
            base = med if base is None else base
            lines.append("%7d %5d %3d %-10s %10.3f %10.3f %10.3f %10.0f %9.2f %12.3f" % (npts, m, n, kernel, med, lo, hi, gbs, gbs / STREAM_GBS, med / base))
            print(lines[-1], flush=True)
            wctx.close()
        lines.append("# expected time ratio from the bytes: %.3f" % ((2 * n + 3) / (2 * n + 1)))
        del X, J, plist, y, r, w
        torch.cuda.empty_cache()
    lines += ["# least_squares_solver on a decay on a constant with Poisson noise (tests/pois_cases.py), the same counts by deviance and by weighted least squares",
              "%7s %5s %3s %-18s %12s %10s %10s %10s %7s %8s %10s" % ("nprob", "m", "n", "fit", "LM it/s", "ms median", "ms min", "ms max", "rounds",
                                                                      "status0", "k bias %")]
    o = ds.options(max_evals=500)
    null = C.cast(None, _lib.DEVFCN)
    for nprob, amp in FIT_ROWS:
        t, y, xt, x0 = PC.decay_problems(amp, nprob, seed=2024, spread=0.0)
        dt, dy, dx0 = (torch.from_numpy(v).to(ds.device) for v in (t, y, x0))
        dwl = torch.from_numpy(PC.ls_weights(y)).to(ds.device)
        lf, lj, lctx = ds.curve_launchers(PC.KIND, PC.K, PC.B, dt, dy, dwl)
        fcn, jac, ctx = ds.curve_launchers(PC.KIND, PC.K, PC.B, dt, dy)
        wf, wj, wctx = ds.pois_launchers(nl.Poisson(), fcn, jac, ctx, dy)
        f = torch.empty((nprob, PC.M), dtype=torch.float64, device=ds.device)
        ib, st = (_lib.IterationBehavior * nprob)(), (C.c_int32 * nprob)()
        variants = [("weighted ls fd", lf, null, ds._ctxp(lctx)), ("weighted ls analytic", lf, lj, ds._ctxp(lctx)),
                    ("poisson fd", wf, null, wctx.ptr), ("poisson analytic", wf, wj, wctx.ptr)]
        for label, fc, jc, cp in variants:
            x = torch.empty_like(dx0)

            def call():
                x.copy_(dx0)
                rc = ds.lib.nlh_lm_solve_batch_device(ds.h.ptr, C.byref(o), nprob, PC.M, 3, fc, jc, cp, x.data_ptr(), f.data_ptr(), ib, st)
                assert rc == 0
            med, lo, hi = bracket(torch, call)
            its = np.array([ib[p].iter_count for p in range(nprob)])
            ok = sum(1 for p in range(nprob) if st[p] == 0)
            bias = 100.0 * float(((x.cpu().numpy()[:, 1] - xt[:, 1]) / xt[:, 1]).mean())
            lines.append("%7d %5d %3d %-18s %12.5g %10.2f %10.2f %10.2f %7d %8d %10.2f" % (nprob, PC.M, 3, label, its.sum() / med * 1e3, med, lo, hi,
                                                                                         its.max(), ok, bias))
            print(lines[-1], flush=True)
        wctx.close()
        del dt, dy, dx0, f, dwl
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
