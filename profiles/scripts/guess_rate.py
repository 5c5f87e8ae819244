"""What a starting value costs (nlh_curve_guess_batch): curve_guess alone, curve_fit_batch from the guess handed
in as x0, and curve_fit_batch(x0=None), which makes the guess itself -- at 16,384 problems of 128 rows of the two studies the
tests record on the CPU: (b) biexponentials (600, 1.5, 400, 0.3, 20) U(0.8, 1.2) on [0, 8] with Poisson noise, and (c) two
Gaussian peaks on a constant on [-5, 5] with unit noise.  Next to the times: the share of the problems whose fit from the guess
ends at or below 1.05 x the cost at the truth, and the share that carries a flag.

    python profiles/scripts/guess_rate.py [--out FILE] [--commit ID] [--nprob N]

One process on the GPU.  HIP events around the call, 3 warm-up calls, then 11 timed calls: median (min .. max)."""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bracket(torch, call, warm=2, calls=11):
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


def problems(name, nprob):
    """(kind, K, B, t [128], y [nprob, 128], truth [nprob, n]) of study (b) or (c) at nprob problems."""
    import curve_restatement as R
    rng = np.random.default_rng(20261024)
    if name == "b_biexp":
        kind, K, B = R.EXPDECAY, 2, 0
        t = np.linspace(0.0, 8.0, 128)
        xt = np.array([600.0, 1.5, 400.0, 0.3, 20.0]) * rng.uniform(0.8, 1.2, (nprob, 5))
        mu = np.stack([R.model(kind, K, B, xt[p], t) for p in range(nprob)])
        return kind, K, B, t, rng.poisson(mu).astype(np.float64), xt
    kind, K, B = R.GAUSS, 2, 0
    t = np.linspace(-5.0, 5.0, 128)
    xt = np.stack([rng.uniform(40, 60, nprob), rng.uniform(-2.5, -1.5, nprob), rng.uniform(0.4, 0.7, nprob), rng.uniform(20, 30, nprob),
                   rng.uniform(1.5, 2.5, nprob), rng.uniform(0.4, 0.7, nprob), rng.uniform(1, 3, nprob)], axis=1)
    mu = np.stack([R.model(kind, K, B, xt[p], t) for p in range(nprob)])
    return kind, K, B, t, mu + rng.standard_normal((nprob, 128)), xt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--nprob", type=int, default=1 << 14)
    a = ap.parse_args()
    import torch
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = ["# curve_guess: the guess alone, the fit from it, and the fit that makes it (x0=None); ms: median (min .. max) of 11 calls after 3",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             "# reached: the share of the problems whose fit ends at or below 1.05 x the cost at the truth; flagged: a non-zero guess flag",
             "%-9s %6s %4s %22s %26s %26s %8s %8s" % ("study", "nprob", "m", "guess ms", "fit from x0 ms", "fit x0=None ms", "reached", "flagged")]
    for name in ("b_biexp", "c_gauss2"):
        kind, K, B, t, y, xt = problems(name, a.nprob)
        dt, dy, dxt = (torch.from_numpy(np.ascontiguousarray(v)).to(ds.device) for v in (t, y, xt))
        opts = ds.options(max_evals=500)
        x0, flag = ds.curve_guess(kind, dt, dy, ncomp=K, baseline=B)
        g = bracket(torch, lambda: ds.curve_guess(kind, dt, dy, ncomp=K, baseline=B))
        f = bracket(torch, lambda: ds.curve_fit_batch(kind, dt, dy, x0, ncomp=K, baseline=B, opts=opts))
        fn = bracket(torch, lambda: ds.curve_fit_batch(kind, dt, dy, None, ncomp=K, baseline=B, opts=opts))
        fvec = ds.curve_fit_batch(kind, dt, dy, None, ncomp=K, baseline=B, opts=opts)[1]
        truth = ((ds.curve_eval(kind, dxt, dt, ncomp=K, baseline=B) - dy) ** 2).sum(dim=1)
        cost = (fvec ** 2).sum(dim=1)
        reached = float((torch.isfinite(cost) & (cost <= 1.05 * truth)).double().mean())
        fmt = lambda v: "%7.3f (%6.3f .. %6.3f)" % v
        lines.append("%-9s %6d %4d %22s %26s %26s %8.4f %8.4f" % (name, a.nprob, 128, fmt(g), fmt(f), fmt(fn), reached,
                                                                  float((flag != 0).double().mean())))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
