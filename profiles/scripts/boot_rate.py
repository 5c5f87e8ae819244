"""What the bootstrap costs (nlh_boot_*), on one MI355X.

1. k_boot_resample alone (nlh_boot_resample_batch into an output allocated once) at 16,384 problems x 128 rows x 64 replicas --
   1 GiB of y*, past the Infinity Cache -- for every kind, with and without weights, as bytes stored / time, next to torch
   writing an array of the SAME size in the same run (Tensor.fill_: a plain store kernel, the yardstick of what a write stream
   reaches on this part from this process; profiles/group_rate.txt recorded 3,671 GB/s for the part's write-only stream).
   pairs stores y* and w*: twice the bytes.
2. The summary (nlh_boot_summary_batch) of 1,000 problems x 3 parameters at 200 and at 4,096 replicas.
3. The one call (expr_boot_batch) on 1,000 decays of 128 rows at 200 replicas, beside 200 x the plain fit of the same data
   (expr_fit_batch without covariance from the same x): what the replicas cost beyond their fits.

    python profiles/scripts/boot_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the timed window; kernels: 3 warm-up windows, then 7 windows of `reps` calls each,
per-call time = window / reps; fits and one-calls: 1 warm-up call, then 5 calls.  median (min .. max)."""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def bracket(torch, call, warm, windows, reps=1):
    def timed():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    for _ in range(warm):
        timed()
    ms = [timed() for _ in range(windows)]
    return statistics.median(ms), min(ms), max(ms)


def fmt(v):
    return "%9.3f (%9.3f .. %9.3f)" % v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import torch
    from nonlin_amd import Bootstrap, Expr
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    dev = ds.device
    lines = ["# bootstrap: the resampling kernel against a plain write of the same size, the summary, and the one call beside its fits; ms: median (min .. max)",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             "# write yardstick: Tensor.fill_ over an array of the same size, same run; profiles/group_rate.txt: 3,671 GB/s write-only stream"]
    # 1. the resampling kernel
    nprob, m, nrep = 1 << 14, 128, 64
    rng = np.random.default_rng(1)
    mu = torch.from_numpy(rng.standard_normal((nprob, m))).to(dev)
    y = mu + 0.1 * torch.from_numpy(rng.standard_normal((nprob, m))).to(dev)
    w = torch.from_numpy(np.where(rng.random((nprob, m)) < 0.1, 0.0, rng.uniform(0.5, 2.0, (nprob, m)))).to(dev)
    yo = torch.empty((nrep, nprob, m), dtype=torch.float64, device=dev)
    wo = torch.empty_like(yo)
    nbytes = yo.numel() * 8
    reps = 400                                                        # windows of about 0.1 s
    tb = lambda v, nb: nb / (v[0] * 1e-3) / 1e12
    f = bracket(torch, lambda: yo.fill_(1.0), 3, 7, reps)
    lines.append("%-34s %8s %34s %8s %8s" % (f"k_boot_resample {nprob} x {m} x {nrep}", "MiB", "ms", "TB/s", "of fill"))
    lines.append("%-34s %8d %34s %8.2f %8.2f" % ("torch fill_ (yardstick)", nbytes >> 20, fmt(f), tb(f, nbytes), 1.0))
    print(lines[-1], flush=True)
    for kind in ("residual", "wild", "pairs"):
        for wt in (None, w):
            boot = Bootstrap(nrep=nrep, kind=kind, seed=5)
            call = lambda: ds._call("nlh_boot_resample_batch", boot.kind, boot.seed, nprob, 0, m, 0, nrep, mu.data_ptr(), y.data_ptr(),
                                    wt.data_ptr() if wt is not None else None, 1, yo.data_ptr(), wo.data_ptr())
            nb = nbytes * (2 if kind == "pairs" else 1)
            c = bracket(torch, call, 3, 7, reps)
            lines.append("%-34s %8d %34s %8.2f %8.2f" % (f"{kind}, {'10 % zero weights' if wt is not None else 'no weights'}", nb >> 20, fmt(c),
                                                         tb(c, nb), tb(c, nb) / tb(f, nbytes)))
            print(lines[-1], flush=True)
    del yo, wo, mu, y, w
    # 2. the summary
    lines.append("%-34s %8s %34s" % ("k_boot_summary 1000 x 3", "nrep", "ms"))
    for nr in (200, 4096):
        xs = torch.randn((nr, 1000, 3), dtype=torch.float64, device=dev)
        xs[::17, ::5] = float("nan")
        s = bracket(torch, lambda: ds.boot_summary(xs, 0.95), 3, 7, 200 if nr == 200 else 10)
        lines.append("%-34s %8d %34s" % ("", nr, fmt(s)))
        print(lines[-1], flush=True)
    # 3. the one call beside its fits
    nprob, m, nrep = 1000, 128, 200
    e = Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
    t = np.linspace(0.0, 1.0, m)
    xt = np.stack([rng.uniform(2.0, 5.0, nprob), rng.uniform(0.4, 0.9, nprob), rng.uniform(-1.0, 1.0, nprob)], axis=1)
    yy = xt[:, 0:1] * np.exp(-xt[:, 1:2] * t[None, :]) + xt[:, 2:3] + 0.05 * rng.standard_normal((nprob, m))
    dt, dy, dx0 = torch.from_numpy(t).to(dev), torch.from_numpy(yy).to(dev), torch.from_numpy(xt).to(dev)
    x = ds.expr_fit_batch(e, dt, dy, dx0)[0]
    fit = bracket(torch, lambda: ds.expr_fit_batch(e, dt, dy, x, covariance=False), 1, 5)
    full = bracket(torch, lambda: ds.expr_fit_batch(e, dt, dy, dx0), 1, 5)
    lines.append("%-34s %6s %4s %5s %34s %34s %12s %8s" % ("one call (expr_boot_batch)", "nprob", "m", "nrep", "one call ms", "plain fit ms",
                                                        "nrep x fit", "nvalid"))
    lines.append("%-34s %6d %4d %5s %34s %34s" % ("the fit with covariance, from truth", nprob, m, "", "", fmt(full)))
    for kind in ("residual", "wild", "pairs"):
        boot = Bootstrap(nrep=nrep, kind=kind, seed=5)
        o = bracket(torch, lambda: ds.expr_boot_batch(e, dt, dy, x, boot), 1, 5)
        nv = ds.expr_boot_batch(e, dt, dy, x, boot)[4]
        lines.append("%-34s %6d %4d %5d %34s %34s %12.3f %8.1f" % (kind, nprob, m, nrep, fmt(o), fmt(fit), nrep * fit[0], float(nv.double().mean())))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
