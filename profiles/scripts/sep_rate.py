"""What variable projection costs (nlh_sep_*): the projecting Jacobian launcher at three sizes, split into the
inner launchers' calls (Jacobian and residual at p0, Jacobian at p^: timed alone on the same points) and the rest -- the
QR-and-solve and the projection kernels --, the rest against two bounds computed here: one read and one write of the panel,
16 m (L + 1 + n) bytes per point, at the read + write stream rate recorded in profiles/group_rate.txt, and 2 m (L + 1 + n) L
unfused fp64 operations at the vector fp64 rate (profiles/scripts/conv_rate.py derives it).  Then the one-call projected fit of
the study's biexponentials (tests/sep_cases.py) next to curve_fit_batch of the same data without sep, started from the same
rates with the amplitudes from the linear solve at the start.

    python profiles/scripts/sep_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max)."""
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
FP64_OPS = 39.3e12                      # unfused vector fp64 operations per second
KERNEL_ROWS = [(16384, 128, 3, 2), (4096, 2048, 6, 6), (512, 4096, 32, 2)]      # (points, m, L, n)
FIT_NPROB = 16384


def model_for(ds, nl, torch, npts, m, L, n, gen):
    """(sep, inner pair, full parameters at which the model is sane, keep-alive) of a model with L linear and n nonlinear
    parameters: the study's biexponential, three Lorentzians on a parabola, 32 Lorentzians tied to one centre and width."""
    t = torch.linspace(0.0, 1.0, m, dtype=torch.float64, device=ds.device).repeat(npts, 1).contiguous()
    y = torch.rand((npts, m), dtype=torch.float64, device=ds.device, generator=gen)
    u = lambda lo, hi, k: lo + (hi - lo) * torch.rand((npts, k), dtype=torch.float64, device=ds.device, generator=gen)
    if (L, n) == (3, 2):
        sp = nl.Separable.for_curve("expdecay", 2, 0)
        inner = ds.curve_launchers("expdecay", 2, 0, t, y)
        alpha = torch.cat([u(4.0, 6.0, 1), u(0.5, 1.5, 1)], dim=1)
        return sp, inner, alpha, (t, y)
    if (L, n) == (6, 6):
        sp = nl.Separable.for_curve("lorentz", 3, 2)
        inner = ds.curve_launchers("lorentz", 3, 2, t, y)
        alpha = torch.cat([u(0.2, 0.3, 1), u(0.03, 0.06, 1), u(0.45, 0.55, 1), u(0.03, 0.06, 1), u(0.7, 0.8, 1), u(0.03, 0.06, 1)], dim=1)
        return sp, inner, alpha, (t, y)
    K = 32
    tied = {}
    for k in range(1, K):
        tied[3 * k + 1] = (1, 1.0, 0.03 * k)
        tied[3 * k + 2] = (2, 1.0 + 0.02 * k, 0.0)
    pm = nl.ParamMap(3 * K, tied=tied)
    lin = [j for j, k in enumerate(pm.tables()[4].tolist()) if k % 3 == 0]
    sp = nl.Separable(34, linear=lin)
    cf, cj, cctx = ds.curve_launchers("lorentz", K, -1, t, y)
    inner = ds.pmap_launchers(pm, cf, cj, cctx, torch.zeros(3 * K, dtype=torch.float64, device=ds.device))
    alpha = torch.cat([u(0.02, 0.04, 1), u(0.01, 0.02, 1)], dim=1)
    return sp, inner, alpha, (t, y, pm, cctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import torch
    import nonlin_amd as nl
    import sep_cases as SC
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    stream = C.c_void_p(torch.cuda.current_stream(ds.device).cuda_stream)
    lines = ["# separable fits: the projecting Jacobian launcher, the inner launchers' three calls inside it, and the rest (the QR-and-solve and projection kernels) against their byte and operation bounds; ms: median (min .. max) of 21 calls after 5",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# stream rate {STREAM_GBS:.0f} GB/s; unfused vector fp64 {FP64_OPS / 1e12:.1f} Top/s; expected form (computed here by the library's rule, not read back from it): lds while 8 m (L + 1 + n) bytes fit a workgroup's LDS beside the kernels' own; rest = call - inner calls: the two kernels, the expansion, the list kernel and the launch gaps, so an upper bound on the kernels' time",
             "%7s %5s %3s %3s %-6s %10s %10s %10s %10s %10s %10s %9s %9s %11s" % ("points", "m", "L", "n", "expected", "jac ms", "jac min", "jac max", "inner ms",
                                                                                  "rest ms", "ms bytes", "ms ops", "of bound", "inner share")]
    gen = torch.Generator(device=ds.device)
    gen.manual_seed(1)
    for npts, m, L, n in KERNEL_ROWS:
        sp, inner, alpha, keep = model_for(ds, nl, torch, npts, m, L, n, gen)
        N = L + n
        wf, wj, wctx = ds.sep_launchers(sp, *inner)
        full, rank = ds.sep_solve(wctx, m, alpha)
        plist = torch.arange(npts, dtype=torch.int32, device=ds.device)
        J = torch.empty((npts, n, m), dtype=torch.float64, device=ds.device)
        JF = torch.empty((npts, N, m), dtype=torch.float64, device=ds.device)
        F = torch.empty((npts, m), dtype=torch.float64, device=ds.device)

        def call_sep():
            assert wj(wctx.ptr, stream, npts, C.c_void_p(plist.data_ptr()), n, C.c_void_p(alpha.data_ptr()), m, C.c_void_p(J.data_ptr())) == 0

        p0 = full.clone()                                        # (c = 0, alpha): where the basis is evaluated
        p0[:, torch.from_numpy(sp.tables()[0].astype("int64")).to(ds.device)] = 0.0

        def call_inner():                                         # what a Jacobian call asks of the inner pair: jac and fcn at p0, jac at p^
            ictx = ds._ctxp(inner[2])
            for launcher, at, out in ((inner[1], p0, JF), (inner[0], p0, F), (inner[1], full, JF)):
                assert launcher(ictx, stream, npts, C.c_void_p(plist.data_ptr()), N, C.c_void_p(at.data_ptr()), m, C.c_void_p(out.data_ptr())) == 0
        med, lo, hi = bracket(torch, call_sep)
        imed, _, _ = bracket(torch, call_inner)
        rest = med - imed
        t_bytes = 16.0 * m * (L + 1 + n) * npts / (STREAM_GBS * 1e9) * 1e3
        t_ops = 2.0 * m * (L + 1 + n) * L * npts / FP64_OPS * 1e3
        form = "lds" if 8 * m * (L + 1 + n) + 10400 <= 160 * 1024 - 2048 else "global"     # (the library's rule: beside the solve kernel's own LDS)
        lines.append("%7d %5d %3d %3d %-6s %10.3f %10.3f %10.3f %10.3f %10.3f %10.3f %9.3f %9.2f %11.2f" % (
            npts, m, L, n, form, med, lo, hi, imed, rest, t_bytes, t_ops, max(t_bytes, t_ops) / rest if rest > 0 else float("nan"), imed / med))
        print(lines[-1], flush=True)
        lines.append("#   live columns of the bases: %s" % sorted(set(rank.cpu().numpy().tolist())))
        wctx.close()
        del J, JF, F, full, p0, alpha, keep, inner
        torch.cuda.empty_cache()
    # the one-call fit of the study's biexponentials, projected and not
    m = SC.STUDY_M
    t, y, xt, k0 = SC.study_problems(FIT_NPROB, seed=SC.STUDY_SEED)
    dev = lambda q: torch.from_numpy(np.ascontiguousarray(q)).to(ds.device)
    dt, dy = dev(t), dev(y)
    sp = nl.Separable.for_curve("expdecay", 2, 0)
    inner = ds.curve_launchers("expdecay", 2, 0, dt, dy)
    wf, wj, wctx = ds.sep_launchers(sp, *inner)
    start, _ = ds.sep_solve(wctx, m, dev(k0))                      # the rates of the start with the amplitudes of the linear solve there
    wctx.close()
    truth = ((xt[:, 0:1] * np.exp(-(xt[:, 1:2] * t)) + xt[:, 2:3] * np.exp(-(xt[:, 3:4] * t)) + xt[:, 4:5] - y) ** 2).sum(1)
    o = ds.options(max_evals=SC.MAX_EVALS)
    lines += [f"# curve_fit_batch (expdecay, 2 components, constant baseline, analytic Jacobian, covariance) of {FIT_NPROB} of the study's biexponentials of {m} points, with sep and without (both from the start rates with the amplitudes of the linear solve there), 7 calls after 2",
              "%-12s %10s %10s %10s %10s %12s %10s" % ("fit", "ms median", "ms min", "ms max", "status != 0", "above 1.05", "mean evals")]
    base = None
    for label, sepobj in (("full", None), ("projected", sp)):
        res = [None]

        def call():
            res[0] = ds.curve_fit_batch("expdecay", dt, dy, start, ncomp=2, baseline=0, opts=o, sep=sepobj)
        med, lo, hi = bracket(torch, call, warm=2, calls=7)
        cost = (res[0][1] ** 2).sum(1).cpu().numpy()
        bad = sum(1 for s in res[0][7] if s != 0)
        above = int(np.sum(~(cost <= 1.05 * truth)))
        evals = float(np.mean([ib["fcn_count"] + ib["jacobian_count"] for ib in res[0][6]]))
        base = med if base is None else base
        lines.append("%-12s %10.2f %10.2f %10.2f %10d %12d %10.1f" % (label, med, lo, hi, bad, above, evals))
        print(lines[-1], flush=True)
        ratio = med / base
    lines.append("# projected / full: %.2f" % ratio)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
