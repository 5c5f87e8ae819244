#!/usr/bin/env python3
"""brent_solver / newton_1var_solver on the user's device fcn1var (the cubic family of tests/device_1var: cubic_launch,
cubic_launch_diff) at 2^20 problems of scalar_models.cubic_problems (every exit of both solvers, invalid brackets
included), options max_evals 40, ftol 1e-12, xtol 1e-12, gtol 1e-10: one JSON line with, per case (brent, newton with
forward differences, newton with the user's derivative), wall ms per solve (median of --reps), lock-step rounds, ms per
round, points evaluated and problems/s.  Rounds and points come from a further, untimed solve whose launcher is a
counting wrapper (same bits).

    python profiles/scripts/root1v_batch.py [--nprob 1048576] [--reps 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/scripts/root1v_batch.py --reps 1
    python profiles/scripts/root1v_batch.py --stats DIR      # kernel time: the library's k_r1_* / scan vs the user's k_cubic
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LIB_KERNELS = ("k_r1_", "k_nm_scan_top")


def shares(d):
    """Kernel time of a rocprofv3 --stats run: the library's own kernels against the user's (k_cubic)."""
    import csv
    import sqlite3
    rows = []
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    for fn in files:
        rows += [(r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])) for r in csv.DictReader(open(fn))]
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)       # rocprofv3's default rocpd output
    for fn in dbs:
        rows += [(r[0], float(r[1]), int(r[2])) for r in
                 sqlite3.connect(fn).execute("select name, sum(end - start), count(*) from kernels group by name")]
    files += dbs
    lib_ns = user_ns = 0.0
    per = {}
    for name, ns, calls in rows:
        k = name.split("(")[0]
        if any(t in name for t in LIB_KERNELS):
            lib_ns += ns
        elif "k_cubic" in name:
            user_ns += ns
        else:
            continue
        ms, n = per.get(k, (0.0, 0))
        per[k] = (ms + ns / 1e6, n + calls)
    tot = lib_ns + user_ns
    return {"files": len(files), "library_kernel_ms": round(lib_ns / 1e6, 3), "user_kernel_ms": round(user_ns / 1e6, 3),
            "library_share": round(lib_ns / tot, 4) if tot else None,
            "per_kernel": {k: {"ms": round(v[0], 3), "calls": v[1], "us_per_call": round(1e3 * v[0] / max(v[1], 1), 2)}
                           for k, v in sorted(per.items())}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        print(json.dumps({"kernel_stats": shares(a.stats)}))
        return
    import numpy as np
    import torch
    from nonlin_amd import _lib
    from nonlin_amd.device import DeviceSolver
    import scalar_models as SM
    ds = DeviceSolver(0)
    c, lim = SM.cubic_problems(a.nprob, seed=11)
    batch = SM.CubicBatch(c)
    dlim = torch.tensor(lim, dtype=torch.float64, device="cuda")
    opts = ds.options(max_evals=40, ftol=1e-12, xtol=1e-12, gtol=1e-10)
    out = {"nprob": a.nprob, "family": "cubic_problems(seed=11)", "max_evals": 40, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "cases": []}
    fcn, dfcn = ds._devfcn(batch.launch), ds._devfcn(batch.launch_diff)

    def solve(kind, f, d, x):
        if kind == "brent":
            return ds.brent_solve_batch_device(f, batch.ctx, dlim, x, opts=opts)
        return ds.newton_1var_solve_batch_device(f, batch.ctx, dlim, x, diff=d, opts=opts)

    for name, kind, d in (("brent", "brent", None), ("newton_fd", "newton", None), ("newton_diff", "newton", dfcn)):
        x = torch.zeros(a.nprob, dtype=torch.float64, device="cuda")
        solve(kind, fcn, d, x)                                                      # warm-up (workspace, code objects)
        times = []
        for _ in range(a.reps):
            x = torch.zeros(a.nprob, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fo, st, ib = solve(kind, fcn, d, x)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(times)
        count = {"rounds": 0, "points": 0}

        def counting(ctx, stream, npoints, dprob, nn, dX, m, dF):
            count["rounds"] += 1
            count["points"] += npoints
            return fcn(ctx, stream, npoints, dprob, nn, dX, m, dF)
        cw = _lib.DEVFCN(counting)
        xc = torch.zeros(a.nprob, dtype=torch.float64, device="cuda")
        fo2, st2, ib2 = solve(kind, cw, d, xc)
        torch.cuda.synchronize()
        assert torch.equal(xc, x) and np.array_equal(fo2, fo) and np.array_equal(ib2, ib) and np.array_equal(st2, st)
        out["cases"].append({
            "case": name, "wall_ms": round(ms, 3), "wall_ms_min": round(min(times), 3), "rounds": count["rounds"],
            "ms_per_round": round(ms / max(count["rounds"], 1), 4), "points": count["points"],
            "problems_per_s": round(a.nprob / (ms / 1e3), 1),
            "status": {str(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
            "fcn_count_total": int(ib["fcn_count"].sum()), "max_iter": int(ib["iter_count"].max())})
    batch.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
