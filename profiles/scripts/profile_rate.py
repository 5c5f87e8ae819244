"""What the profile-likelihood intervals cost (nlh_pin_*, nlh_profile_*), on one MI355X.

1. k_pin_jac alone against k_pmap_jac under the equivalent fixed map -- ParamMap(N, fixed=(pos,)) -- at equal bytes in the same
   run, alternating, two passes each: 16,384 x (m = 256, N = 3), 4,096 x (2048, 9) and 512 x (4096, 24), pos = N // 2, and the pin
   kernel once more with pos varying per point.  Both are timed through their Jacobian launcher with an inner Jacobian launcher
   that launches nothing (the scratch Jacobian keeps whatever it held: the kernels' time does not depend on the values), so a
   call is the expansion -- a few microseconds -- and the streaming kernel; bytes = 8 m (n read + n written) per point, n = N - 1,
   as a share of the 5,018 GB/s read + write stream rate of profiles/group_rate.txt.
2. The one call (curve_profile_batch) on 1,000 decays of 128 rows -- profiles/scripts/boot_rate.py's shape -- beside
   curve_boot_batch at 200 replicas of the same data in the same run: wall time, the refits per end, the flags, and -- from a
   second, instrumented call that synchronises around every solve -- the share of the wall time spent in the solves.

    python profiles/scripts/profile_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the timed window; kernels: 5 warm-up calls, then 21 calls; one-calls: 1 warm-up call,
then 5 calls.  median (min .. max)."""
import argparse
import ctypes as C
import datetime
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STREAM_GBS = 5018.0                     # profiles/group_rate.txt: the read + write stream rate this part delivers
KERNEL_ROWS = [(1 << 14, 256, 3), (4096, 2048, 9), (512, 4096, 24)]


def bracket(torch, call, warm, calls):
    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(warm):
        timed()
    ms = [timed() for _ in range(calls)]
    return statistics.median(ms), min(ms), max(ms)


def fmt(v):
    return "%9.3f (%9.3f .. %9.3f)" % v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import torch
    import nonlin_amd as nl
    from nonlin_amd import _lib, Bootstrap, Profile
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    dev = ds.device
    lines = ["# profile-likelihood intervals: the pin kernel against the map kernel at equal bytes, and the one call beside the bootstrap; ms: median (min .. max)",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# k_pin_jac / k_pmap_jac (with their expansion) through the Jacobian launcher, inner Jacobian launcher a no-op; stream rate {STREAM_GBS:.0f} GB/s",
             "%-22s %7s %5s %3s %5s %34s %8s %9s" % ("kernel", "points", "m", "N", "pass", "ms", "GB/s", "of stream")]
    noop = _lib.DEVFCN(lambda c, s, npts, dprob, n, dX, m, dJ: 0)
    fcn = C.cast(ds.lib.nlh_curve_device_fcn, _lib.DEVFCN)              # (never called: only the Jacobian launchers are)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(1)
    for npts, m, N in KERNEL_ROWS:
        n = N - 1
        X = torch.ones((npts, n), dtype=torch.float64, device=dev)
        J = torch.empty((npts, n, m), dtype=torch.float64, device=dev)
        src = torch.arange(npts, dtype=torch.int32, device=dev)
        theta = torch.ones((npts,), dtype=torch.float64, device=dev)
        pos_c = torch.full((npts,), N // 2, dtype=torch.int32, device=dev)
        pos_v = torch.from_numpy(rng.integers(0, N, npts).astype(np.int32)).to(dev)
        pf, pj, pctx = ds.pin_launchers(fcn, noop, None, N, src, pos_c, theta)
        vf, vj, vctx = ds.pin_launchers(fcn, noop, None, N, src, pos_v, theta)
        mf, mj, mctx = ds.pmap_launchers(nl.ParamMap(N, fixed=(N // 2,)), fcn, noop, None, torch.ones((N,), dtype=torch.float64, device=dev))

        def launcher(entry, ctx):
            def call():
                assert entry(ctx.ptr, stream, npts, None, n, X.data_ptr(), m, J.data_ptr()) == 0
            return call
        calls = {"k_pin_jac": launcher(ds.lib.nlh_pin_device_jac, pctx), "k_pmap_jac fixed=(pos,)": launcher(ds.lib.nlh_pmap_device_jac, mctx),
                 "k_pin_jac, pos varying": launcher(ds.lib.nlh_pin_device_jac, vctx)}
        nbytes = 8.0 * m * 2 * n * npts
        for rep in (1, 2):
            for name, call in calls.items():
                t = bracket(torch, call, 5, 21)
                gbs = nbytes / (t[0] * 1e-3) / 1e9
                lines.append("%-22s %7d %5d %3d %5d %34s %8.0f %9.2f" % (name, npts, m, N, rep, fmt(t), gbs, gbs / STREAM_GBS))
                print(lines[-1], flush=True)
        for c in (pctx, vctx, mctx):
            c.close()
        del X, J
        torch.cuda.empty_cache()
    # 2. the one call beside the bootstrap
    nprob, m, nrep = 1000, 128, 200
    t = np.linspace(0.0, 1.0, m)
    xt = np.stack([rng.uniform(2.0, 5.0, nprob), rng.uniform(0.4, 0.9, nprob), rng.uniform(-1.0, 1.0, nprob)], axis=1)
    yy = xt[:, 0:1] * np.exp(-xt[:, 1:2] * t[None, :]) + xt[:, 2:3] + 0.05 * rng.standard_normal((nprob, m))
    dt, dy, dx0 = torch.from_numpy(t).to(dev), torch.from_numpy(yy).to(dev), torch.from_numpy(xt).to(dev)
    x, _, sigma = ds.curve_fit_batch("expdecay", dt, dy, dx0, baseline=0)[:3]
    prof, boot = Profile(), Bootstrap(nrep=nrep, kind="residual", seed=5)
    one = lambda: ds.curve_profile_batch("expdecay", dt, dy, x, sigma, prof, baseline=0)
    p = bracket(torch, one, 1, 5)
    b = bracket(torch, lambda: ds.curve_boot_batch("expdecay", dt, dy, x, boot, baseline=0), 1, 5)
    lo, hi, flags, nev = one()
    # the instrumented call: the stream drained before and after every solve, host clock
    spent, solves, inner = [0.0], [0], ds.lm_solve_batch_device

    def timed_solve(*args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(*args, **kw)
        torch.cuda.synchronize()
        spent[0] += time.perf_counter() - t0
        solves[0] += 1
        return out
    ds.lm_solve_batch_device = timed_solve
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    one()
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    ds.lm_solve_batch_device = inner
    counts = {_lib.PROFILE_FLAGS[int(c) & 15] + ("+LOWER" if int(c) & _lib.PROFILE_LOWER else ""): int(k)
              for c, k in zip(*np.unique(flags.cpu().numpy(), return_counts=True))}
    lines += ["# the one call on decays a*exp(-k*t)+c, noise 0.05, least squares, analytic Jacobian, default Profile() and Bootstrap(200, 'residual')",
              "%-28s %6s %4s %34s" % ("call", "nprob", "m", "ms"),
              "%-28s %6d %4d %34s" % ("curve_profile_batch", nprob, m, fmt(p)),
              "%-28s %6d %4d %34s" % ("curve_boot_batch, 200 reps", nprob, m, fmt(b)),
              f"# profile: {nprob * 3 * 2} ends, refits per end {float(nev.double().mean()):.3f}, most {int(nev.max())}; flags {counts}",
              f"# profile, instrumented call: {total * 1e3:.1f} ms wall, {spent[0] * 1e3:.1f} ms in {solves[0]} lm_solve_batch_device calls: "
              f"{spent[0] / total:.2f} of the wall time in the solves"]
    for ln in lines[-6:]:
        print(ln, flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
