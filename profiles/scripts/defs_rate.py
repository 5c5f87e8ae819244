"""What definitions in formulas cost and save: k_expr_fcn / k_expr_jac (nlh_expr_device_fcn / _jac), one launcher call over
the whole batch each, and the one-call fit nlh_expr_fit_batch.

1. The formulas profiles/scripts/pwfun_rate.py times (gauss2d of tests/expr_cases.py, the power law and the hinge of
   tests/pwfun_cases.py and their workarounds), none of which has a definition, at its sizes: the same rows from a build of the
   parent commit (--lib, --existing-only), before and after this commit's, show what the larger dispatch costs the formulas
   that were there before; the spread of the parent's two runs is the margin.
2. The rotated 2-D Gaussian (with all six definitions, and with cos and sin alone named: rot2d_cs), the exponentially modified
   Gaussian and the two-peak pseudo-Voigt (tests/defs_cases.py) with definitions and in substituted form, at 4096 x 512 and 65536 x 64: the kernels and the fit, and the ratios.
3. Instruction counts, constants and frames of the models both ways and the most peaks of each that compile
   (--counts: compile-time facts, no GPU needed).  There is no gate.

    python profiles/scripts/defs_rate.py [--out FILE] [--commit ID] [--lib LIBRARY] [--existing-only] [--counts]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls (the fit: 2 and 7): median
(min .. max), the procedure of profiles/scripts/pwfun_rate.py.  --out FILE is appended to, so that the parent's rows, this
commit's and the parent's again stand in the order they were measured in."""
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

ROWS = [(4096, 512), (1 << 16, 64)]                                 # (nprob, m)
fmt = "%-34s %7d %5d %10.3f %16s"
head = "%-34s %7s %5s %10s %16s" % ("what", "nprob", "m", "ms", "(min..max)")


def counts():
    """Section 3: what the compiler makes of the models, with definitions and substituted."""
    import defs_cases as DC
    import defs_restatement as D
    lines = ["# instructions, constants and frame (depth) of the models as written with definitions and with every definition substituted;",
             "# LOADs: uses of a definition; Jacobian columns a pass carries at that depth (n parameters, m = 64)",
             "%-10s %-12s %7s %7s %6s %6s %6s" % ("model", "form", "ninstr", "nconst", "frame", "LOADs", "chunk")]
    from nonlin_amd.device import expr_plan
    for name in DC.MODELS:
        for sub in (False, True):
            e = DC.compile_formula(name, substituted=sub)
            loads = int((e.program()[0] == D.LOAD).sum())
            lines.append("%-10s %-12s %7d %7d %6d %6d %6d" % (name, "substituted" if sub else "definitions", e.ninstr, e.nconst, e.depth, loads,
                                                            expr_plan(e.depth, e.nparams, 64)["chunk"]))
    lines += ["# the most peaks of a sum of such peaks on a constant that compile (256 instructions, 64 constants, frame 16, 32 parameters):",
              "# the pseudo-Voigt (4 parameters a peak) and the EMG (4) end at the 32 parameters either way; the rotated Gaussian (6) with",
              "# all six definitions per peak ends at the frame -- six slots a peak -- and substituted at the parameters",
              "%-10s %12s %12s" % ("model", "definitions", "substituted")]
    for name, v in DC.PEAKS.items():
        lines.append("%-10s %12d %12d" % ((name,) + DC.most_peaks(*v)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--lib")
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--counts", action="store_true")
    a = ap.parse_args()
    lines = []

    def flush():
        text = "\n".join(lines) + "\n"
        print(text, end="", flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(text)
        del lines[:]

    if a.counts:
        lines += counts()
        flush()
        return
    import torch
    from nonlin_amd import _lib
    if a.lib:                                                       # (a parent build may lack newer symbols: bind what it has)
        _lib.LIB_PATH = os.path.abspath(a.lib)
        other = C.CDLL(_lib.LIB_PATH)
        for name in [k for k in _lib.SYMBOLS if not hasattr(other, k)]:
            del _lib.SYMBOLS[name]
    from nonlin_amd.device import DeviceSolver
    import expr_cases as EC
    import pwfun_cases as PC
    ds = DeviceSolver(0)
    if not (a.out and os.path.exists(a.out)):                       # (the first run into a file heads it)
        lines += ["# definitions in formulas: ms per call, median (min .. max) of 21 calls after 5 warm-ups (fits: 7 after 2), HIP events",
                  f"# {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}"]

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def measure(call, warm=5, calls=21):
        for _ in range(warm):
            call()
        torch.cuda.synchronize()
        ms = [timed(call) for _ in range(calls)]
        return statistics.median(ms), min(ms), max(ms)

    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)

    def tiled(t, y, x0, nprob):
        rep = nprob // 64
        return [torch.from_numpy(np.ascontiguousarray(v)).to(ds.device) for v in (np.tile(t, (1, rep, 1)), np.tile(y, (rep, 1)), np.tile(x0, (rep, 1)))]

    def kernels(e, dt, dy, dx0, nprob, m):
        """(fcn, jac) timings of one launcher call over the whole batch."""
        n = dx0.shape[1]
        dprob = torch.arange(nprob, dtype=torch.int32, device=ds.device)
        F = torch.empty((nprob, m), dtype=torch.float64, device=ds.device)
        J = torch.empty((nprob, n, m), dtype=torch.float64, device=ds.device)
        fcn, jac, ctx = ds.expr_launchers(e, dt, dy)
        cp = ds._ctxp(ctx)

        def launch(fn, out):
            assert fn(cp, stream, nprob, C.c_void_p(dprob.data_ptr()), n, C.c_void_p(dx0.data_ptr()), m, C.c_void_p(out.data_ptr())) == 0
        return measure(lambda: launch(fcn, F)), measure(lambda: launch(jac, J)), F, J

    def rows(name, nprob, m, **what):
        for k, v in what.items():
            lines.append(fmt % (name + " " + k, nprob, m, v[0], "%.3f..%.3f" % v[1:]))

    # 1. formulas without definitions: these rows are the ones to compare between commits
    lines += [f"# {a.commit}" + (f" (library {os.path.basename(os.path.dirname(a.lib))}/{os.path.basename(a.lib)})" if a.lib else "")
              + ": k_expr_fcn / k_expr_jac of formulas without definitions", head]
    for nprob, m in ((4096, 484), (1 << 16, 64)):
        prog, t, y, xt, x0 = EC.expr_problems("gauss2d", m, nprob=64, seed=3)
        f, j, F, J = kernels(EC.compile_formula("gauss2d"), *tiled(t, y, x0, nprob), nprob, m)
        rows("gauss2d", nprob, m, fcn=f, jac=j)
    for nprob, m in ROWS:
        for name in ("powerlaw_explog", "powerlaw", "hinge_abs", "hinge"):
            prog, t, y, xt, x0 = PC.problems(name, m, nprob=64, seed=3)
            f, j, F, J = kernels(PC.compile_formula(name), *tiled(t, y, x0, nprob), nprob, m)
            rows(name, nprob, m, fcn=f, jac=j)
    flush()
    if a.existing_only:
        return

    # 2. definitions against substitution
    import defs_cases as DC
    lines += ["# the models with definitions (defs) and with every definition substituted (subst): the kernels, the one-call fit",
              "# (analytic Jacobian, covariance) and the ratio defs / subst of the medians; outputs of the two forms compared bit for bit", head]
    o = ds.options(max_evals=200)
    for nprob, m in ROWS:
        for name in DC.MODELS:
            prog, t, y, xt, x0 = DC.problems(name, m, nprob=64, seed=3)
            dt, dy, dx0 = tiled(t, y, x0, nprob)
            got = {}
            for form, sub in (("defs", False), ("subst", True)):
                e = DC.compile_formula(name, substituted=sub)
                f, j, F, J = kernels(e, dt, dy, dx0, nprob, m)
                fit = measure(lambda: ds.expr_fit_batch(e, dt, dy, dx0, opts=o), warm=2, calls=7)
                x = ds.expr_fit_batch(e, dt, dy, dx0, opts=o)[0]
                rows(f"{name} {form}", nprob, m, fcn=f, jac=j, fit=fit)
                got[form] = (f[0], j[0], fit[0], F, J, x)
            d, s = got["defs"], got["subst"]
            same = all(bool(torch.equal(u.view(torch.int64), v.view(torch.int64))) for u, v in zip(d[3:], s[3:]))
            lines.append("# %s %d x %d: defs / subst  fcn %.3f  jac %.3f  fit %.3f;  F, J and the fitted x bit for bit equal: %s"
                         % (name, nprob, m, d[0] / s[0], d[1] / s[1], d[2] / s[2], same))
            flush()


if __name__ == "__main__":
    main()
