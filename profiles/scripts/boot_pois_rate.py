"""What the Poisson bootstrap costs (nlh_boot_poisson_*), on one MI355X.

1. k_boot_poisson alone (nlh_boot_poisson_batch into an output allocated once) at 16,384 problems x 128 rows x 64 replicas --
   1 GiB of y* -- for fitted values around 5, 50, 1000 and 10^5 (mu = centre * U(0.8, 1.2) per row), next to `wild` at the same
   shape in the same run: wild's store stream is the floor for this kernel, which stores the same bytes after walking
   O(sqrt(mu)) steps per value.
2. The same kernel at 128 problems x 32 rows x 64 replicas, where 16 replica slots share a row's setup through LDS.
3. The one call (expr_boot_batch with a PoissonBootstrap and stat=Poisson()) on 1,000 decays of 128 bins at 200 replicas,
   beside 200 x the deviance fit of the same data (expr_fit_batch(stat=) without covariance from the same x).

    python profiles/scripts/boot_pois_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the timed window; kernels: 3 warm-up windows, then 7 windows of `reps` calls each
(reps sized to windows of about 0.1 s), per-call time = window / reps; fits and one-calls: 1 warm-up call, then 5 calls.
median (min .. max).  Everything is measured twice, one run after the other in the same process: both are printed."""
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


def kernel(torch, call):
    """bracket with reps sized from one call to windows of about 0.1 s."""
    call()
    one = bracket(torch, call, 1, 1)[0]
    return bracket(torch, call, 3, 7, max(1, min(400, int(100.0 / max(one, 1e-3)))))


def fmt(v):
    return "%9.3f (%9.3f .. %9.3f)" % v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import torch
    from nonlin_amd import PoissonBootstrap, Poisson, Expr
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    dev = ds.device
    lines = ["# Poisson bootstrap: the sampling kernel beside wild's store stream, a short shape with the setup staged in LDS, and the one call beside its fits; ms: median (min .. max)",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             "# every figure twice: run 1 and run 2 of the same process, one after the other"]

    def add(s):
        lines.append(s)
        print(s, flush=True)
    rng = np.random.default_rng(1)
    centres = (5.0, 50.0, 1000.0, 1e5)
    for run in (1, 2):
        add(f"## run {run}")
        for nprob, m, nrep in ((1 << 14, 128, 64), (128, 32, 64)):
            u = torch.from_numpy(rng.uniform(0.8, 1.2, (nprob, m))).to(dev)
            y = torch.zeros((nprob, m), dtype=torch.float64, device=dev)
            yo = torch.empty((nrep, nprob, m), dtype=torch.float64, device=dev)
            bad = torch.zeros((nprob,), dtype=torch.int32, device=dev)
            nbytes = yo.numel() * 8
            add("%-34s %8s %34s %10s %12s" % (f"{nprob} x {m} x {nrep}", "KiB", "ms", "GB/s", "Gdraws/s"))
            mu = (u * 50.0).contiguous()
            c = kernel(torch, lambda: ds._call("nlh_boot_resample_batch", 1, 5, nprob, 0, m, 0, nrep, mu.data_ptr(), y.data_ptr(), None, 1,
                                               yo.data_ptr(), None))
            add("%-34s %8d %34s %10.1f %12.2f" % ("k_boot_resample, wild (the floor)", nbytes >> 10, fmt(c), nbytes / c[0] / 1e6,
                                                 yo.numel() / c[0] / 1e6))
            for centre in centres:
                mu = (u * centre).contiguous()
                c = kernel(torch, lambda: ds._call("nlh_boot_poisson_batch", 5, nprob, 0, m, 0, nrep, mu.data_ptr(), y.data_ptr(), None,
                                                   yo.data_ptr(), bad.data_ptr()))
                assert int(bad.sum()) == 0
                add("%-34s %8d %34s %10.1f %12.2f" % (f"k_boot_poisson, mu ~ {centre:g}", nbytes >> 10, fmt(c), nbytes / c[0] / 1e6,
                                                     yo.numel() / c[0] / 1e6))
            del yo, u, y
        # the one call beside its fits
        nprob, m, nrep = 1000, 128, 200
        e = Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
        t = np.linspace(0.0, 4.0, m)
        r2 = np.random.default_rng(2)
        xt = np.stack([r2.uniform(35.0, 65.0, nprob), r2.uniform(0.8, 1.2, nprob), r2.uniform(0.3, 1.0, nprob)], axis=1)
        yy = r2.poisson(xt[:, 0:1] * np.exp(-xt[:, 1:2] * t[None, :]) + xt[:, 2:3]).astype(np.float64)
        dt, dy, dx0 = torch.from_numpy(t).to(dev), torch.from_numpy(yy).to(dev), torch.from_numpy(xt).to(dev)
        stat = Poisson()
        x = ds.expr_fit_batch(e, dt, dy, dx0, stat=stat)[0]
        fit = bracket(torch, lambda: ds.expr_fit_batch(e, dt, dy, x, covariance=False, stat=stat), 1, 5)
        boot = PoissonBootstrap(nrep=nrep, seed=5)
        o = bracket(torch, lambda: ds.expr_boot_batch(e, dt, dy, x, boot, stat=stat), 1, 5)
        nv = ds.expr_boot_batch(e, dt, dy, x, boot, stat=stat)[4]
        add("%-34s %6s %4s %5s %34s %34s %12s %8s" % ("one call (expr_boot_batch, stat=)", "nprob", "m", "nrep", "one call ms", "deviance fit ms",
                                                  "nrep x fit", "nvalid"))
        add("%-34s %6d %4d %5d %34s %34s %12.3f %8.1f" % ("PoissonBootstrap", nprob, m, nrep, fmt(o), fmt(fit), nrep * fit[0],
                                                         float(nv.double().mean())))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
