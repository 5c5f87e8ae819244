"""What integrating over bins costs (nlh_bin_*): the bin-summing kernel alone at three sizes against its byte
bound -- 8 (Q + 1) m n bytes per point (the Q node planes of a column in, a column out) at the read + write stream rate
measured in the same run, a torch copy that moves the same number of bytes; the 5,018 GB/s of profiles/group_rate.txt beside
it -- and the one-call Poisson fit of Gaussian histograms with bins=Binned(order=3) next to the same call with bins=None on
the centre-value formula.

    python profiles/scripts/bin_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max).
The kernel is timed through nlh_bin_apply_batch with ncol = n: the launch nlh_bin_device_jac makes after the inner Jacobian
launcher (k_bin in Jacobian mode, without weights, with a shared scale), and nothing else; inputs are random, not zeros.  Its
2 Q unfused fp64 operations per output are far from binding: bytes bind."""
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

from loss_rate import bracket  # noqa: E402

STREAM_GBS = 5018.0                     # profiles/group_rate.txt: the read + write stream rate this part delivers
KERNEL_ROWS = [(16384, 256, 3, 3), (4096, 2048, 9, 4), (512, 4096, 24, 16)]      # (points, m, n, Q)
FIT = (16384, 128, 3)                   # (nprob, m, order)
FIT_H = 0.5                             # bin width over sigma: 128 bins span +- 32 sigma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import torch
    import nonlin_amd as nl
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = ["# bin-integrated fits: the bin-summing kernel alone against its byte bound, and a binned fit next to the centre-value fit; ms: median (min .. max) of 21 calls after 5",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# through nlh_bin_apply_batch (ncol = n); the copy: torch's copy_ of half the kernel's bytes, so the same bytes moved; profiles/group_rate.txt has {STREAM_GBS:.0f} GB/s",
             "%7s %5s %3s %3s %10s %10s %10s %10s %10s %10s %9s %9s" % ("points", "m", "n", "Q", "MB moved", "ms median", "ms min", "ms max", "ms copy",
                                                                   "copy GB/s", "of copy", "of 5018")]
    gen = torch.Generator(device=ds.device)
    gen.manual_seed(1)
    for npts, m, n, Q in KERNEL_ROWS:
        v = torch.randn((npts, n, Q * m), dtype=torch.float64, device=ds.device, generator=gen)
        out = torch.empty((npts, n, m), dtype=torch.float64, device=ds.device)
        xi = np.linspace(-1.0, 1.0, Q)
        bins = nl.Binned(np.arange(m, dtype=np.float64), np.arange(m) + 1.0, rule=(xi, np.random.default_rng(Q).uniform(0.1, 1.0, Q)))
        bn, dsc = ds._bin_struct(bins, npts)

        def call():
            rc = ds.lib.nlh_bin_apply_batch(ds.h.ptr, C.byref(bn), npts, m, n, v.data_ptr(), out.data_ptr())
            assert rc == 0
        med, lo, hi = bracket(torch, call)
        nbytes = 8.0 * (Q + 1) * m * n * npts
        src = torch.empty((int(nbytes // 16),), dtype=torch.float64, device=ds.device).normal_(generator=gen)
        dst = torch.empty_like(src)
        cmed, clo, chi = bracket(torch, lambda: dst.copy_(src))
        copy_gbs = 16.0 * src.numel() / (cmed * 1e-3) / 1e9
        t_5018 = nbytes / (STREAM_GBS * 1e9) * 1e3
        lines.append("%7d %5d %3d %3d %10.1f %10.3f %10.3f %10.3f %10.3f %10.0f %9.2f %9.2f" % (
            npts, m, n, Q, nbytes / 1e6, med, lo, hi, cmed, copy_gbs, cmed / med, t_5018 / med))
        print(lines[-1], flush=True)
        if cmed / med < 0.5:
            lines.append("#   below half of the byte bound (%.2f of the copy): the stream is not full at this shape" % (cmed / med))
        del v, out, src, dst
        torch.cuda.empty_cache()
    nprob, m, order = FIT
    lines += [f"# expr_fit_batch (one Gaussian as a formula, analytic Jacobian, covariance, Poisson deviance) of {nprob} histograms of {m} bins of width {FIT_H:g} sigma: bins=Binned(order={order}), and bins=None on the formula of the centre value times the width, 7 calls after 2",
              "%-16s %10s %10s %10s %8s %12s" % ("fit", "ms median", "ms min", "ms max", "status0", "sigma bias %")]
    h, sigma, counts = FIT_H, 1.0, 20000.0
    e = h * (np.arange(m + 1) - m / 2)
    import math
    mu = 0.2 * h
    cdf = np.array([0.5 * (1.0 + math.erf((q - mu) / (sigma * math.sqrt(2.0)))) for q in e])
    y = np.random.default_rng(7).poisson(np.tile(counts * (cdf[1:] - cdf[:-1]), (nprob, 1))).astype(np.float64)
    xt = np.array([counts / math.sqrt(2.0 * math.pi), mu, sigma])
    x0 = np.tile(xt * np.array([1.1, 1.0, 1.15]) + np.array([0.0, 0.1, 0.0]), (nprob, 1))
    dy, dx0 = (torch.from_numpy(np.ascontiguousarray(q)).to(ds.device) for q in (y, x0))
    dt = torch.from_numpy(0.5 * (e[:-1] + e[1:])).to(ds.device)
    o = ds.options(max_evals=500)
    ex = nl.Expr(f"{h!r}*a*exp(-0.5*((t-mu)/s)^2)", ("t",), ("a", "mu", "s"))
    exb = nl.Expr("a*exp(-0.5*((t-mu)/s)^2)", ("t",), ("a", "mu", "s"))
    bins = nl.Binned.edges(e, order=order)
    base = None
    for label in ("centre x width", "binned"):
        res = [None]

        def call():
            if label == "binned":
                res[0] = ds.expr_fit_batch(exb, None, dy, dx0, opts=o, stat=nl.Poisson(), bins=bins)
            else:
                res[0] = ds.expr_fit_batch(ex, dt, dy, dx0, opts=o, stat=nl.Poisson())
        med, lo, hi = bracket(torch, call, warm=2, calls=7)
        ok = sum(1 for s in res[0][7] if s == 0)
        bias = 100.0 * float((res[0][0].cpu().numpy()[:, 2] / sigma - 1.0).mean())
        base = med if base is None else base
        lines.append("%-16s %10.2f %10.2f %10.2f %8d %12.3f" % (label, med, lo, hi, ok, bias))
        print(lines[-1], flush=True)
        ratio = med / base
    lines.append("# binned / centre x width: %.2f (the inner model is evaluated at %d times the rows)" % (ratio, order))
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
