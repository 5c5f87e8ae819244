"""What the studentised and the BCa interval of the bootstrap cost (nlh_boot_student_batch, nlh_boot_bca_batch,
nlh_boot_jackknife_batch), on one MI355X.

1. k_boot_student and k_boot_bca (with their validity pass, as the calls run them) on 1,000 problems x 3 parameters at 200 and at
   4,096 replicas, next to k_boot_summary on the SAME xs in the same run: the ratio is stated, not set beforehand.
2. k_boot_jackknife alone (into an output allocated once) on 8,192 problems x 128 rows x 128 deletions -- 1 GiB, past the
   Infinity Cache --, with and without weights, as bytes stored / time next to torch's Tensor.fill_ of the SAME size in the same run.
3. The one call (expr_boot_batch) on 1,000 decays of 128 rows at 200 replicas with each of the three intervals; the "student"
   call beyond the "percentile" one is the refits' covariances (and one kernel), the "bca" call beyond it the 128 delete-one fits
   per data set (and two kernels).

    python profiles/scripts/boot_ci_rate.py [--out FILE] [--commit ID] [--only-percentile] [--root DIR]

--only-percentile: part 3's "percentile" line alone.  --root DIR: import nonlin_amd from DIR, a built checkout of another commit
-- with --only-percentile this measures the parent commit's call in the same session, which is how the baseline lines at the
end of profiles/boot_ci_rate.txt were made (the parent before and after this commit's run).

One process on the GPU.  HIP events around the timed window; kernels: 3 warm-up windows, then 7 windows of `reps` calls each,
per-call time = window / reps; one-calls: 1 warm-up call, then 5 calls.  median (min .. max)."""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--only-percentile", action="store_true")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from nonlin_amd import Bootstrap, Expr
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    dev = ds.device
    rng = np.random.default_rng(1)
    lines = []
    if not a.only_percentile:
        lines += ["# studentised and BCa intervals: their kernels beside k_boot_summary, the jackknife weights beside a plain write, and the one call "
                  "with each interval; ms: median (min .. max)",
                  f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
                  "# baselines: k_boot_summary on the same xs, Tensor.fill_ over an array of the same size, and the parent commit's percentile call "
                  "-- all in this session"]
        # 1. the two reductions beside the summary
        lines.append("%-34s %8s %34s %12s" % ("1000 x 3, with the validity pass", "nrep", "ms", "of summary"))
        for nr in (200, 4096):
            xs = torch.randn((nr, 1000, 3), dtype=torch.float64, device=dev)
            xs[::17, ::5] = float("nan")
            sigs = torch.rand((nr, 1000, 3), dtype=torch.float64, device=dev) + 0.5
            x = torch.zeros((1000, 3), dtype=torch.float64, device=dev)
            sg = torch.ones_like(x)
            acc = torch.full_like(x, 0.02)
            reps = 200 if nr == 200 else 10
            s = bracket(torch, lambda: ds.boot_summary(xs, 0.95), 3, 7, reps)
            for name, call in (("k_boot_summary (baseline)", None), ("k_boot_student", lambda: ds.boot_student(xs, sigs, x, sg, 0.95)),
                               ("k_boot_bca", lambda: ds.boot_bca(xs, x, acc, 0.95))):
                c = s if call is None else bracket(torch, call, 3, 7, reps)
                lines.append("%-34s %8d %34s %12.2f" % (name, nr, fmt(c), c[0] / s[0]))
                print(lines[-1], flush=True)
        # 2. the jackknife weights beside a plain write
        nprob, m = 8192, 128
        w = torch.from_numpy(np.where(rng.random((nprob, m)) < 0.1, 0.0, rng.uniform(0.5, 2.0, (nprob, m)))).to(dev)
        wo = torch.empty((m, nprob, m), dtype=torch.float64, device=dev)
        nbytes = wo.numel() * 8
        tb = lambda v: nbytes / (v[0] * 1e-3) / 1e12
        f = bracket(torch, lambda: wo.fill_(1.0), 3, 7, 400)
        lines.append("%-34s %8s %34s %8s %8s" % (f"k_boot_jackknife {nprob} x {m} x {m}", "MiB", "ms", "TB/s", "of fill"))
        lines.append("%-34s %8d %34s %8.2f %8.2f" % ("torch fill_ (baseline)", nbytes >> 20, fmt(f), tb(f), 1.0))
        print(lines[-1], flush=True)
        for wt in (None, w):
            call = lambda: ds._call("nlh_boot_jackknife_batch", nprob, m, 0, m, wt.data_ptr() if wt is not None else None, wo.data_ptr())
            c = bracket(torch, call, 3, 7, 400)
            lines.append("%-34s %8d %34s %8.2f %8.2f" % ("weights" if wt is not None else "no weights", nbytes >> 20, fmt(c), tb(c), tb(c) / tb(f)))
            print(lines[-1], flush=True)
        del wo, w
    # 3. the one call with each interval
    nprob, m, nrep = 1000, 128, 200
    e = Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c"))
    t = np.linspace(0.0, 1.0, m)
    xt = np.stack([rng.uniform(2.0, 5.0, nprob), rng.uniform(0.4, 0.9, nprob), rng.uniform(-1.0, 1.0, nprob)], axis=1)
    yy = xt[:, 0:1] * np.exp(-xt[:, 1:2] * t[None, :]) + xt[:, 2:3] + 0.05 * rng.standard_normal((nprob, m))
    dt, dy, dx0 = torch.from_numpy(t).to(dev), torch.from_numpy(yy).to(dev), torch.from_numpy(xt).to(dev)
    x, _, sigma, *_ = ds.expr_fit_batch(e, dt, dy, dx0)
    if a.only_percentile:
        o = bracket(torch, lambda: ds.expr_boot_batch(e, dt, dy, x, Bootstrap(nrep=nrep, seed=5)), 1, 5)
        lines.append("%-34s %6d %4d %5d %34s" % (f"percentile, commit {a.commit}", nprob, m, nrep, fmt(o)))
        print(lines[-1], flush=True)
    else:
        lines.append("%-34s %6s %4s %5s %34s %14s %10s" % ("one call (expr_boot_batch)", "nprob", "m", "nrep", "one call ms", "beyond perc.", "share"))
        base = None
        for kind in ("percentile", "student", "bca"):
            boot = Bootstrap(nrep=nrep, seed=5, interval=kind)
            o = bracket(torch, lambda: ds.expr_boot_batch(e, dt, dy, x, boot, sigma=sigma), 1, 5)
            base = base or o
            what = {"percentile": "", "student": "the covariances", "bca": f"the {m} delete-one fits"}[kind]
            lines.append("%-34s %6d %4d %5d %34s %14.3f %10.2f  %s" % (kind, nprob, m, nrep, fmt(o), o[0] - base[0], (o[0] - base[0]) / o[0], what))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "a" if a.only_percentile else "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
