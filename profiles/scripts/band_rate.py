"""What a band costs (nlh_propagate*): the kernel k_band alone against its two bounds -- the bytes it has to
move at the stream rate this part delivers, and its unfused fp64 operations at the vector rate -- and a full curve_band call
(values, analytic Jacobian, kernel) against curve_eval of the same grid, in the same session.

    python profiles/scripts/band_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max).
Per point the kernel reads 8 m n bytes of J and 8 n (n + 1) / 2 of the covariance (once per workgroup: per 256 rows, or per
point in the flat form), writes 8 m, and does n (n + 1) + 2 n unfused operations per row."""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_GBS = 5018.0                     # profiles/r04_ubench.txt: the read + write stream rate this part delivers
FP64_OPS = 39.3e12                      # unfused fp64 vector operations per second (the figure of profiles/sep_rate.txt)
KERNEL_ROWS = [(1 << 16, 64, 9), (4096, 2048, 24), (512, 4096, 96)]      # (points, m, n)
BAND_ROWS = [(1 << 14, 256, 2, 0), (4096, 2048, 4, 1)]                    # (nprob, npts, Lorentzians, baseline degree)


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
    import curve_cases as CC
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = ["# bands: the kernel alone against its byte bound and its operation bound, and curve_band against curve_eval; ms: median (min .. max) of 21 calls after 5",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# nlh_propagate on resident J and cov; stream rate {STREAM_GBS:.0f} GB/s, {FP64_OPS / 1e12:.1f}e12 unfused fp64 operations / s",
             "%7s %5s %3s %-5s %10s %10s %10s %10s %9s %10s %9s" % ("points", "m", "n", "form", "ms median", "ms min", "ms max", "GB/s", "of stream",
                                                                  "Gop/s", "of vector")]
    for npts, m, n in KERNEL_ROWS:
        J = torch.randn((npts, n, m), dtype=torch.float64, device=ds.device)
        A = torch.randn((npts, n, n + 2), dtype=torch.float64, device=ds.device)
        cov = (A @ A.transpose(1, 2)).contiguous()
        sd = torch.empty((npts, m), dtype=torch.float64, device=ds.device)
        del A
        for form in ("row", "flat"):
            if form == "flat" and m > 256:
                continue
            os.environ["NLH_BAND_FORM"] = form

            def call():
                rc = ds.lib.nlh_propagate(ds.h.ptr, npts, m, n, J.data_ptr(), cov.data_ptr(), None, sd.data_ptr())
                assert rc == 0
            med, lo, hi = bracket(torch, call)
            wgs = npts * ((m + 255) // 256) if form == "row" else npts
            byts = 8.0 * m * (n + 1) * npts + 8.0 * (n * (n + 1) // 2) * wgs
            ops = float(n * (n + 1) + 2 * n) * m * npts
            gbs, gops = byts / (med * 1e-3) / 1e9, ops / (med * 1e-3) / 1e9
            lines.append("%7d %5d %3d %-5s %10.3f %10.3f %10.3f %10.0f %9.2f %10.0f %9.2f" % (npts, m, n, form, med, lo, hi, gbs, gbs / STREAM_GBS, gops,
                                                                                             gops / (FP64_OPS / 1e9)))
            print(lines[-1], flush=True)
        os.environ.pop("NLH_BAND_FORM", None)
        del J, cov, sd
        torch.cuda.empty_cache()
    lines += ["# curve_band (values + analytic Jacobian + kernel) against curve_eval (values) of Lorentzians on the same grid",
              "%7s %5s %3s %12s %10s %10s %12s %10s %10s %7s" % ("nprob", "npts", "n", "band ms med", "ms min", "ms max", "eval ms med", "ms min", "ms max", "ratio")]
    for nprob, npts, K, B in BAND_ROWS:
        _, _, x, _ = CC.curve_problems("lorentz", K, B, 64, nprob=nprob, seed=7)
        n = x.shape[1]
        dx = torch.from_numpy(x).to(ds.device)
        t = torch.linspace(-0.1, 1.1, npts, dtype=torch.float64, device=ds.device)
        A = torch.randn((nprob, n, n + 2), dtype=torch.float64, device=ds.device)
        cov = (1e-4 * (A @ A.transpose(1, 2))).contiguous()
        bm = bracket(torch, lambda: ds.curve_band("lorentz", dx, cov, t, ncomp=K, baseline=B))
        em = bracket(torch, lambda: ds.curve_eval("lorentz", dx, t, ncomp=K, baseline=B))
        lines.append("%7d %5d %3d %12.3f %10.3f %10.3f %12.3f %10.3f %10.3f %7.1f" % (nprob, npts, n, *bm, *em, bm[0] / em[0]))
        print(lines[-1], flush=True)
        del dx, cov, A
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
