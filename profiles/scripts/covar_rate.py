"""Time of nlh_covar, form by form, next to the factorisation it follows (nlh_lmfactor_exact on the same batch, same run)
and to the host path a user has without it (numpy.linalg.inv on the n x n Gram matrices, 16 processes of the same machine).

    python profiles/scripts/covar_rate.py [--out FILE] [--trace]

One process on the GPU.  Jacobians are standard-normal m x n matrices (the kernels' work does not depend on the values).
Device time: HIP events around the library call on preallocated outputs; covar: 3 warm-up calls, then 11 timed calls,
median (min .. max); lmfactor: 1 warm-up, 3 timed calls, median -- a batch beyond 65535 problems is factored in lock-step
slices, their times summed.  Host time: the whole batch of Gram matrices split evenly over 16 worker processes (one LAPACK
thread each), wall clock of the slowest worker's numpy.linalg.inv call.  The workers run and end before the GPU is opened.
--trace: warm-up and two calls per form only, no host leg (for a run under rocprofv3 --kernel-trace --stats)."""
import os
os.environ["OPENBLAS_NUM_THREADS"] = "1"
os.environ["OMP_NUM_THREADS"] = "1"
import argparse
import multiprocessing as mp
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BATCHES = [(1 << 20, 64, 3), (65536, 512, 12), (4096, 2048, 24), (2048, 4096, 96), (256, 4096, 256)]
WORKERS = 16
SLICE = 65535


def _host_worker(g):
    t = time.perf_counter()
    np.linalg.inv(g)
    return time.perf_counter() - t


def host_ms(nprob, n):
    a = np.random.default_rng(n).standard_normal((nprob, n, n + 4))
    g = a @ a.transpose(0, 2, 1)
    with mp.get_context("fork").Pool(WORKERS) as pool:
        pool.map(_host_worker, np.array_split(g[:WORKERS * 4], WORKERS))          # start the workers, load LAPACK
        times = pool.map(_host_worker, np.array_split(g, WORKERS))
    return max(times) * 1e3


def timed(torch, call, warm, reps):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    host = {} if a.trace else {n: host_ms(nprob, n) for nprob, _, n in BATCHES}
    import torch
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lib = ds.lib
    cap = 160 * 1024 - 2048
    lines = ["# nlh_covar per form, nlh_lmfactor_exact on the same batch, numpy.linalg.inv(J^T J) on 16 host processes; milliseconds",
             "# covar: median (min .. max) of 11 calls after 3 warm-ups; lmfactor: median of 3 after 1 (slices of 65535 problems summed)",
             f"# device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             "%9s %5s %4s %-7s %10s %10s %10s %12s %12s %9s" % ("nprob", "m", "n", "form", "covar ms", "min", "max", "lmfactor ms",
                                                                 "host16 ms", "default")]
    verdict = []
    for nprob, m, n in BATCHES:
        gen = torch.Generator(device=ds.device).manual_seed(n)
        J = torch.randn((nprob, n, m), dtype=torch.float64, device=ds.device, generator=gen)
        f = torch.randn((nprob, m), dtype=torch.float64, device=ds.device, generator=gen)
        R = torch.zeros((nprob, n, n), dtype=torch.float64, device=ds.device)
        ipvt = torch.empty((nprob, n), dtype=torch.int32, device=ds.device)
        vec = [torch.empty((nprob, n), dtype=torch.float64, device=ds.device) for _ in range(3)]
        wa4 = torch.empty((nprob, m), dtype=torch.float64, device=ds.device)
        cov = torch.empty((nprob, n, n), dtype=torch.float64, device=ds.device)
        rank = torch.empty((nprob,), dtype=torch.int32, device=ds.device)

        def factor():
            for p0 in range(0, nprob, SLICE):
                c = min(SLICE, nprob - p0)
                rc = lib.nlh_lmfactor_exact(ds.h.ptr, c, m, n, J[p0:].data_ptr(), f[p0:].data_ptr(), R[p0:].data_ptr(), ipvt[p0:].data_ptr(),
                                            vec[0][p0:].data_ptr(), vec[1][p0:].data_ptr(), vec[2][p0:].data_ptr(), wa4[p0:].data_ptr())
                assert rc == 0

        def covar():
            assert lib.nlh_covar(ds.h.ptr, nprob, n, R.data_ptr(), ipvt.data_ptr(), 0.0, cov.data_ptr(), rank.data_ptr()) == 0
        fac = timed(torch, factor, 1, 2 if a.trace else 3)[0]
        default = "lane" if n <= 8 else ("lds" if lib.nlh_covar_lds_bytes(n) <= cap else "global")
        forms = [fm for fm in ("lane", "lds", "global") if (fm != "lane" or n <= 8) and (fm != "lds" or lib.nlh_covar_lds_bytes(n) <= cap)]
        best = None
        for fm in forms:
            os.environ["NLH_COVAR_FORM"] = fm
            med, lo, hi = timed(torch, covar, 3, 2 if a.trace else 11)
            os.environ.pop("NLH_COVAR_FORM")
            assert int((rank != n).sum()) == 0
            lines.append("%9d %5d %4d %-7s %10.4f %10.4f %10.4f %12.3f %12.3f %9s" % (nprob, m, n, fm, med, lo, hi, fac, host.get(n, float("nan")),
                                                                                     "default" if fm == default else ""))
            if best is None or med < best[1]:
                best = (fm, med)
            if fm == default:
                dmed = med
        verdict.append("# %d x n = %d: default form %s %.4f ms, lmfactor %.3f ms: covar / lmfactor = %.4f (%s); fastest form: %s"
                       % (nprob, n, default, dmed, fac, dmed / fac, "below the factorisation" if dmed < fac else "NOT below the factorisation",
                          best[0]))
        del J, f, R, ipvt, vec, wa4, cov, rank
        torch.cuda.empty_cache()
    text = "\n".join(lines + verdict) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
