#!/usr/bin/env python3
"""nelder_mead on the user's device objective (chained Rosenbrock, crosen_launch of tests/device_model) at 65536 problems
for n = 2, 8, 16, default max_evals (500): one JSON line with wall ms, lock-step rounds, ms per round, points evaluated and
problems/s per n.  Rounds and points come from a second, untimed solve whose launcher is a counting wrapper (same bits).

    python profiles/scripts/nm_batch.py [--nprob 65536] [--n 2 8 16]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/scripts/nm_batch.py --n 8
    python profiles/scripts/nm_batch.py --stats DIR      # share of kernel time: the library's k_nm_* vs the user's kernel
"""
import argparse
import ctypes as C
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def shares(d):
    """Kernel time of a rocprofv3 --stats run: the library's own kernels (k_nm_*) against the user's (k_crosen)."""
    import csv
    import sqlite3
    rows = []
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    for fn in files:
        rows += [(r["Name"], float(r["TotalDurationNs"])) for r in csv.DictReader(open(fn))]
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)       # rocprofv3's default rocpd output
    for fn in dbs:
        rows += [(r[0], float(r[1])) for r in sqlite3.connect(fn).execute("select name, sum(end - start) from kernels group by name")]
    files += dbs
    lib_ns = user_ns = 0.0
    per = {}
    for name, ns in rows:
        if "k_nm_" in name:
            k = name.split("(")[0]
            lib_ns += ns
            per[k] = per.get(k, 0.0) + ns
        elif "k_crosen" in name:
            user_ns += ns
    tot = lib_ns + user_ns
    return {"files": len(files), "library_kernel_ms": lib_ns / 1e6, "user_kernel_ms": user_ns / 1e6,
            "library_share": lib_ns / tot if tot else None, "per_kernel_ms": {k: v / 1e6 for k, v in per.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=65536)
    ap.add_argument("--n", type=int, nargs="+", default=[2, 8, 16])
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        print(json.dumps({"kernel_stats": shares(a.stats)}))
        return
    import torch
    from nonlin_amd import _lib
    from nonlin_amd.device import DeviceSolver
    import user_models as UM
    ds = DeviceSolver(0)
    out = {"nprob": a.nprob, "max_evals": 500, "objective": "crosen", "cases": []}
    for n in a.n:
        c, x0 = UM.crosen_problems(a.nprob, n, seed=100 + n)
        batch = UM.BtriBatch(c)
        opts = ds.options(max_evals=500)
        launch = ds._devfcn(batch.crosen_launch)
        xw = torch.tensor(x0, dtype=torch.float64, device="cuda")
        ds.nelder_mead_solve_batch_device(launch, batch.ctx, xw, opts=opts)           # warm-up (workspace, code objects)
        xd = torch.tensor(x0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fo, ibs, st = ds.nelder_mead_solve_batch_device(launch, batch.ctx, xd, opts=opts)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        count = {"rounds": 0, "points": 0}

        def counting(ctx, stream, npoints, dprob, nn, dX, m, dF):
            count["rounds"] += 1
            count["points"] += npoints
            return launch(ctx, stream, npoints, dprob, nn, dX, m, dF)
        cw = _lib.DEVFCN(counting)
        xc = torch.tensor(x0, dtype=torch.float64, device="cuda")
        fo2, ibs2, st2 = ds.nelder_mead_solve_batch_device(cw, batch.ctx, xc, opts=opts)
        torch.cuda.synchronize()
        assert torch.equal(xc, xd) and fo2 == fo and ibs2 == ibs
        batch.close()
        out["cases"].append({
            "n": n, "wall_ms": round(ms, 3), "rounds": count["rounds"], "ms_per_round": round(ms / max(count["rounds"], 1), 4),
            "points": count["points"], "problems_per_s": round(a.nprob / (ms / 1e3), 1),
            "converged": sum(1 for s in st if s == 0), "max_iter": max(b["iter_count"] for b in ibs)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
