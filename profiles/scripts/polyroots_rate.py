"""Polynomials per second of nlh_poly_roots_batch next to the host path a user has without it: LAPACK (numpy.linalg.eigvals
on the companion matrices, one thread per process) on 16 processes of the same machine.

    python profiles/scripts/polyroots_rate.py [--out FILE] [--trace]

One process on the GPU.  Device time: HIP events around the library call on preallocated outputs, 5 warm-up calls, then 21
timed calls: median, min, max.  Host time: a sample of each size (the whole batch would take minutes at the larger
orders), split evenly over 16 worker processes, wall clock of the slowest worker's eigvals calls; the rate is
sample / that time.  The workers run and end before the GPU is opened.  --trace: warm-up and three calls per size only
(for a run under rocprofv3 --kernel-trace --stats)."""
import os
os.environ["OPENBLAS_NUM_THREADS"] = "1"        # 16 worker processes, one LAPACK thread each: 16 cores in all
os.environ["OMP_NUM_THREADS"] = "1"
import argparse
import multiprocessing as mp
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SIZES = [(1 << 20, 3), (1 << 18, 8), (1 << 14, 32), (4096, 100), (1024, 200)]
HOST_SAMPLE = {3: 1 << 18, 8: 1 << 16, 32: 1 << 12, 100: 512, 200: 256}
WORKERS = 16


def coefficients(nprob, order):
    return np.random.default_rng(1000 + order).standard_normal((nprob, order + 1))


def _host_worker(c):
    n = c.shape[1] - 1
    m = np.zeros((c.shape[0], n, n))
    m[:, :, n - 1] = -c[:, :n] / c[:, n:]
    idx = np.arange(n - 1)
    m[:, idx + 1, idx] = 1.0
    t = time.perf_counter()
    np.linalg.eigvals(m)
    return time.perf_counter() - t


def host_rate(order):
    c = coefficients(HOST_SAMPLE[order], order)
    with mp.get_context("fork").Pool(WORKERS) as pool:
        pool.map(_host_worker, np.array_split(c[:WORKERS * 8], WORKERS))          # start the workers, load LAPACK
        times = pool.map(_host_worker, np.array_split(c, WORKERS))
    return c.shape[0] / max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    host = {} if a.trace else {order: host_rate(order) for _, order in SIZES}
    import torch
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = ["# nlh_poly_roots_batch, polynomials per second; device: median (min .. max) of 21 calls after 5 warm-ups;",
             "# host: numpy.linalg.eigvals on the companion matrices, 16 processes, one LAPACK thread each, same machine",
             f"# device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             "%10s %6s %-7s %14s %14s %14s %14s %8s" % ("nprob", "order", "form", "median p/s", "min p/s", "max p/s", "host16 p/s",
                                                       "x host")]
    for nprob, order in SIZES:
        form = "lane" if order <= 8 else ("wave" if order <= 128 else "global")
        c = torch.from_numpy(coefficients(nprob, order)).to(ds.device)
        z = torch.empty((nprob, order, 2), dtype=torch.float64, device=ds.device)
        info = torch.empty((nprob,), dtype=torch.int32, device=ds.device)

        def call():
            rc = ds.lib.nlh_poly_roots_batch(ds.h.ptr, nprob, order, c.data_ptr(), z.data_ptr(), info.data_ptr())
            assert rc == 0
        for _ in range(5):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3 if a.trace else 21):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        assert int((info != 0).sum()) == 0
        med, lo, hi = statistics.median(ms), min(ms), max(ms)
        h = host.get(order, float("nan"))
        lines.append("%10d %6d %-7s %14.4g %14.4g %14.4g %14.4g %8.2f" % (nprob, order, form, nprob / med * 1e3, nprob / hi * 1e3,
                                                                         nprob / lo * 1e3, h, nprob / med * 1e3 / h))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
