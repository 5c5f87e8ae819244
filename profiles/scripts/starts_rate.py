"""What the box scan costs (nlh_starts_*), on one MI355X at 16,384 problems of 256 rows of the sinusoid family the
tests study on the CPU (tests/starts_cases.py, here drawn at nprob problems from the same distributions).

1. k_starts_cost alone (DeviceSolver.starts_cost) on the residuals of one launcher call at the 256 MiB budget (131,072 points of
   256 rows) and on 2 GiB (1,048,576 points: past the Infinity Cache), as bytes read / time, next to a plain read of the SAME
   array measured in the same run: torch.sum over it (torch's own reduction kernel, used here only as the yardstick of what a
   read stream reaches on this part from this process).
2. The whole scan (DeviceSolver.starts_search) at 4096 candidates x 4 parameters on the full model a*sin(w*t+ph)+c, and at 64
   candidates x 1 parameter under sep= on a*sin(w*t)+b*cos(w*t)+c, each beside the fit it feeds (expr_fit_batch from the scan's
   best candidate) and the share of those fits that end at or below 1.05 x the cost at the truth.

    python profiles/scripts/starts_rate.py [--out FILE] [--commit ID] [--nprob N]

One process on the GPU.  HIP events around the timed window; kernels: 3 warm-up windows, then 7 windows of `reps` calls each,
per-call time = window / reps; scans and fits: 1 warm-up call, then 5 calls.  median (min .. max)."""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--nprob", type=int, default=1 << 14)
    a = ap.parse_args()
    import torch
    import starts_cases as SC
    from nonlin_amd import Expr, Separable, Starts
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    m = SC.M
    lines = ["# starts: the cost kernel against a plain read of the same array, and the scan beside the fit it feeds; ms: median (min .. max)",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             "# read yardstick: torch.sum over the same array, same run (a plain read kernel; no profile's figure is used)"]
    # 1. the cost kernel
    lines.append("%-28s %10s %34s %10s %34s %10s %8s" % ("k_starts_cost", "MiB", "cost ms", "TB/s", "torch.sum ms", "TB/s", "share"))
    for points in (131072, 1048576):
        F = torch.randn((points, m), dtype=torch.float64, device=ds.device)
        nbytes = F.numel() * 8
        reps = max(4, int(0.1 * 4e12 / nbytes))                       # windows of about 0.1 s
        c = bracket(torch, lambda: ds.starts_cost(F), 3, 7, reps)
        r = bracket(torch, lambda: torch.sum(F), 3, 7, reps)
        tb = lambda v: nbytes / (v[0] * 1e-3) / 1e12
        lines.append("%-28s %10d %34s %10.2f %34s %10.2f %8.2f" % (f"{points} points x {m} rows", nbytes >> 20, fmt(c), tb(c), fmt(r), tb(r), r[0] / c[0]))
        print(lines[-1], flush=True)
        del F
    # 2. the scans, each beside its fit
    rng = np.random.default_rng(SC.SEED + 1)
    n = a.nprob
    t = np.linspace(0.0, 10.0, m)
    xt = np.stack([rng.uniform(1.0, 5.0, n), rng.uniform(5.0, 50.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(-1.0, 1.0, n)], axis=1)
    y = SC.full_model(xt, t) + SC.NOISE * rng.standard_normal((n, m))
    cap = torch.from_numpy(1.05 * SC.truth_cost(t, y, xt)).to(ds.device)
    dt, dy = torch.from_numpy(t).to(ds.device), torch.from_numpy(y).to(ds.device)
    opts = ds.options(max_evals=SC.MAX_EVALS)
    lines.append("%-28s %6s %4s %7s %34s %34s %34s %8s" % ("scan", "nprob", "m", "ncand", "scan ms", "fit from its x0 ms", "one call (starts=) ms", "reached"))
    full = Expr("a*sin(w*t+ph)+c", ("t",), ("a", "w", "ph", "c"))
    sepe = Expr(SC.SEP_FORMULA, ("t",), SC.SEP_PARAMS)
    sep = Separable.for_expr(sepe, linear=("a", "b", "c"))
    cases = (("full, 4 parameters", full, None, Starts(SC.FULL_LOWER, SC.FULL_UPPER, ncand=4096, keep=1, log=SC.FULL_LOG)),
             ("sep, w alone", sepe, sep, Starts((-10.0, SC.SEP_LOWER[0], -10.0, -10.0), (10.0, SC.SEP_UPPER[0], 10.0, 10.0), ncand=64, keep=1)))
    for name, e, sp, st in cases:
        fcn, jac, ctx = ds.expr_launchers(e, dt, dy)
        pos = None
        if sp is not None:
            fcn, jac, ctx = ds.sep_launchers(sp, fcn, jac, ctx)
            pos = [int(k) for k in sp.tables()[1]]
        x0s = ds.starts_search(fcn, ctx, n, m, st, pos)[0]
        x0 = x0s[:, 0].contiguous()
        if pos is not None:
            x0 = torch.zeros((n, 4), dtype=torch.float64, device=ds.device)
            x0[:, pos] = x0s[:, 0]
        s = bracket(torch, lambda: ds.starts_search(fcn, ctx, n, m, st, pos), 1, 5)
        f = bracket(torch, lambda: ds.expr_fit_batch(e, dt, dy, x0, sep=sp, opts=opts), 1, 5)
        o = bracket(torch, lambda: ds.expr_fit_batch(e, dt, dy, None, sep=sp, starts=st, opts=opts), 1, 5)
        fvec = ds.expr_fit_batch(e, dt, dy, None, sep=sp, starts=st, opts=opts)[1]
        cost = (fvec ** 2).sum(dim=1)
        reached = float((torch.isfinite(cost) & (cost <= cap)).double().mean())
        lines.append("%-28s %6d %4d %7d %34s %34s %34s %8.4f" % (name, n, m, st.ncand, fmt(s), fmt(f), fmt(o), reached))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
