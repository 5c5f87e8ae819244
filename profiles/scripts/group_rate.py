"""What a global fit costs and buys (nlh_group_*): the scatter kernel k_group_jac alone, as a fraction of the
read + write stream rate this part delivers, beside k_pmap_jac (identity map) at the nearest byte count in the same run; and
the one-call global fit of 16,384 groups of 8 decays against the 131,072 separate fits of the same data.

    python profiles/scripts/group_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls (fits: 2 and 7): median
(min .. max).  Either kernel is timed through its wrapper's Jacobian launcher with an inner Jacobian launcher that launches
nothing (the scratch Jacobian keeps whatever it held: a copy's time does not depend on the values), so a call is the
expansion -- a few microseconds -- and the kernel, in as many slices as the 1 GiB scratch cap makes.  Bytes per outer point:
8 G m N read + 8 G m (S + G L) written for the scatter, 8 m (N + N) for the identity map."""
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
KERNEL_ROWS = [(1 << 16, 8, 64, 3, (1,)), (1 << 12, 4, 2048, 9, (0, 1))]        # (groups, G, m, N, shared)
FIT = dict(ngroup=1 << 14, G=8, m=64, seed=11)


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
    import nonlin_amd as nl
    import group_cases as GC
    from nonlin_amd import _lib
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = ["# global fits: the scatter kernel alone beside the identity parameter map, and decays fitted globally and separately; ms: median (min .. max)",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# through nlh_group_device_jac / nlh_pmap_device_jac, inner Jacobian launcher a no-op, 21 calls after 5; stream rate {STREAM_GBS:.0f} GB/s",
             "%-11s %8s %3s %5s %3s %3s %7s %8s %10s %10s %10s %8s %9s" % ("kernel", "points", "G", "m", "N", "n", "slices", "GB", "ms median", "ms min",
                                                                        "ms max", "GB/s", "of stream")]
    noop = _lib.DEVFCN(lambda c, s, npts, dprob, n, dX, m, dJ: 0)
    fcn = C.cast(ds.lib.nlh_curve_device_fcn, _lib.DEVFCN)              # (never called: only the Jacobian launcher is)
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    fractions = []
    for ngroup, G, m, N, shared in KERNEL_ROWS:
        grp = nl.Group(N, shared=shared, nsets=G)
        n, M = grp.nouter, G * m
        X = torch.ones((ngroup, n), dtype=torch.float64, device=ds.device)
        J = torch.empty((ngroup, n, M), dtype=torch.float64, device=ds.device)
        wf, wj, wctx = ds.group_launchers(grp, fcn, noop, None)

        def call():
            rc = ds.lib.nlh_group_device_jac(wctx.ptr, stream, ngroup, None, n, X.data_ptr(), M, J.data_ptr())
            assert rc == 0
        med, lo, hi = bracket(torch, call)
        per = 8 * (G * N * (m + 1) + (G + 1) // 2) + 4
        slices = -(-ngroup // max(1, min(ngroup, (1 << 30) // per)))
        nbytes = 8.0 * G * m * (N + n) * ngroup
        gbs = nbytes / (med * 1e-3) / 1e9
        lines.append("%-11s %8d %3d %5d %3d %3d %7d %8.2f %10.3f %10.3f %10.3f %8.0f %9.2f" % ("k_group_jac", ngroup, G, m, N, n, slices, nbytes / 1e9, med,
                                                                                           lo, hi, gbs, gbs / STREAM_GBS))
        print(lines[-1], flush=True)
        wctx.close()
        del X, J, wctx
        torch.cuda.empty_cache()
        # the identity map over the same m and N, as many points as make the same bytes
        npts = int(round(nbytes / (16.0 * m * N)))
        pm = nl.ParamMap(N)
        full = torch.ones((N,), dtype=torch.float64, device=ds.device)
        X = torch.ones((npts, N), dtype=torch.float64, device=ds.device)
        J = torch.empty((npts, N, m), dtype=torch.float64, device=ds.device)
        pf, pj, pctx = ds.pmap_launchers(pm, fcn, noop, None, full)

        def pcall():
            rc = ds.lib.nlh_pmap_device_jac(pctx.ptr, stream, npts, None, N, X.data_ptr(), m, J.data_ptr())
            assert rc == 0
        pmed, plo, phi = bracket(torch, pcall)
        pper = 8 * N * (m + 1) + 4
        pslices = -(-npts // max(1, min(npts, (1 << 30) // pper)))
        pbytes = 16.0 * m * N * npts
        pgbs = pbytes / (pmed * 1e-3) / 1e9
        lines.append("%-11s %8d %3s %5d %3d %3d %7d %8.2f %10.3f %10.3f %10.3f %8.0f %9.2f" % ("k_pmap_jac", npts, "-", m, N, N, pslices, pbytes / 1e9, pmed,
                                                                                           plo, phi, pgbs, pgbs / STREAM_GBS))
        print(lines[-1], flush=True)
        fractions.append((gbs / STREAM_GBS) / (pgbs / STREAM_GBS))
        pctx.close()
        del X, J, pctx
        torch.cuda.empty_cache()
    lines.append("# k_group_jac's fraction of the stream rate over k_pmap_jac's: " + ", ".join("%.2f" % f for f in fractions))
    # the fits: a exp(-k t) + c, k shared by the 8 decays of a group (tests/group_cases.py: study_data)
    ngroup, G, m = FIT["ngroup"], FIT["G"], FIT["m"]
    nprob = ngroup * G
    t, y, xt = GC.study_data(**FIT)
    x0 = np.tile(np.array([50.0, 1.2, 0.0]), (nprob, 1))
    dt, dy, dx0 = (torch.from_numpy(np.ascontiguousarray(v)).to(ds.device) for v in (t, y, x0))
    o = ds.options(max_evals=500)
    grp = nl.Group(3, shared=(1,), nsets=G)
    lines += [f"# curve_fit_batch (expdecay, 1 component, constant baseline, analytic Jacobian, covariance) of {nprob} decays of {m} points, 7 calls after 2",
              "%-22s %8s %5s %3s %10s %10s %10s %8s %12s %12s" % ("fit", "problems", "rows", "n", "ms median", "ms min", "ms max", "status0", "scatter of k",
                                                                 "mean sigma_k")]
    out = {}
    for label, kw, nq, rows, nn in (("global, k shared", dict(group=grp), ngroup, G * m, grp.nouter), ("separate", {}, nprob, m, 3)):
        def call():
            out[label] = ds.curve_fit_batch("expdecay", dt, dy, dx0, ncomp=1, baseline=0, opts=o, **kw)
        med, lo, hi = bracket(torch, call, warm=1, calls=7)
        x, fvec, sigma, cov, chi2, rank, ibs, st = out[label]
        k = x[:, 1].cpu().numpy()
        ok = sum(1 for s in st if s == 0)
        lines.append("%-22s %8d %5d %3d %10.2f %10.2f %10.2f %8d %12.5f %12.5f" % (label, nq, rows, nn, med, lo, hi, ok, float(np.std(k - 1.0)),
                                                                             float(np.nanmean(sigma[:, 1].cpu().numpy()))))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
