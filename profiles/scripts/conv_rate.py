"""What an instrument response costs (nlh_conv_*): the convolution kernel alone at three sizes against two
bounds computed here -- its bytes, 16 m n per point (a column in, a column out), at the read + write stream rate recorded in
profiles/group_rate.txt, and its 2 m L n unfused fp64 operations (a multiply and an add per tap and row) at the vector fp64
rate -- and the one-call reconvolution fit of decays under the Poisson deviance next to the same call without conv.

    python profiles/scripts/conv_rate.py [--out FILE] [--commit ID]

One process on the GPU.  HIP events around the library call, 5 warm-up calls, then 21 timed calls: median (min .. max).
The kernel is timed through nlh_conv_apply_batch with ncol = n: the launch nlh_conv_device_jac makes after the inner Jacobian
launcher (k_conv_row in Jacobian mode, without weights), and nothing else; inputs are random, not zeros.
The vector fp64 rate: the microarchitecture guide lists 157.3 TFLOP/s of vector fp32 (fused multiply-adds counted twice), that
is 78.6e12 fp32 instructions-lanes per second; a CDNA vector unit issues fp64 at half the fp32 rate, so 39.3e12 unfused fp64
operations per second (the part's public 78.6 TFLOP/s of vector fp64 counts a fused operation twice).  -ffp-contract=off and the
interface's two roundings per tap keep the kernel from the fused form, so this, not 78.6, is its ceiling."""
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
FP64_OPS = 39.3e12                      # unfused vector fp64 operations per second (see above)
KERNEL_ROWS = [(16384, 256, 3, 32), (4096, 2048, 9, 128), (512, 4096, 3, 1024)]      # (points, m, n, L)
FIT = (16384, 256, 32)                  # (nprob, m, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--commit", default="unknown")
    a = ap.parse_args()
    import torch
    import nonlin_amd as nl
    import conv_cases as CV
    import conv_restatement as CR
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    lines = ["# instrument-response fits: the convolution kernel alone against its byte and operation bounds, and a reconvolution fit next to the plain fit; ms: median (min .. max) of 21 calls after 5",
             f"# commit {a.commit}; {datetime.date.today().isoformat()}; device: {torch.cuda.get_device_name(0)}; numpy {np.__version__}",
             f"# through nlh_conv_apply_batch (ncol = n); stream rate {STREAM_GBS:.0f} GB/s; unfused vector fp64 {FP64_OPS / 1e12:.1f} Top/s",
             "%7s %5s %3s %5s %-5s %10s %10s %10s %10s %10s %9s %9s %-8s" % ("points", "m", "n", "L", "ext", "ms median", "ms min", "ms max", "ms bytes",
                                                                        "ms ops", "of bytes", "of ops", "binding")]
    gen = torch.Generator(device=ds.device)
    gen.manual_seed(1)
    for npts, m, n, L in KERNEL_ROWS:
        v = torch.randn((npts, n, m), dtype=torch.float64, device=ds.device, generator=gen)
        out = torch.empty_like(v)
        for ext in ("zero", "hold"):
            conv = nl.Convolve(np.random.default_rng(L).uniform(0.1, 1.0, L), origin=0, extend=ext)
            cv, dk = ds._conv_struct(conv, npts)

            def call():
                rc = ds.lib.nlh_conv_apply_batch(ds.h.ptr, C.byref(cv), npts, m, n, v.data_ptr(), out.data_ptr())
                assert rc == 0
            med, lo, hi = bracket(torch, call)
            t_bytes = 16.0 * m * n * npts / (STREAM_GBS * 1e9) * 1e3
            t_ops = 2.0 * m * L * n * npts / FP64_OPS * 1e3
            bound = max(t_bytes, t_ops)
            lines.append("%7d %5d %3d %5d %-5s %10.3f %10.3f %10.3f %10.3f %10.3f %9.2f %9.2f %-8s" % (
                npts, m, n, L, ext, med, lo, hi, t_bytes, t_ops, t_bytes / med, t_ops / med, "bytes" if t_bytes >= t_ops else "ops"))
            print(lines[-1], flush=True)
            if bound / med < 0.5:
                lines.append("#   below half of the binding bound (%.2f): neither the stream nor the fp64 pipe is full at this shape" % (bound / med))
        del v, out
        torch.cuda.empty_cache()
    nprob, m, L = FIT
    lines += [f"# curve_fit_batch (expdecay, 1 component, constant baseline, analytic Jacobian, covariance, Poisson deviance) of {nprob} decays of {m} bins, with and without conv ({L} taps, causal, zero), 7 calls after 2",
              "%-16s %10s %10s %10s %8s %10s" % ("fit", "ms median", "ms min", "ms max", "status0", "k bias %")]
    rng = np.random.default_rng(2024)
    k = CV.irf()
    assert len(k) == L
    t = np.tile(CV.BIN * np.arange(m), (nprob, 1))
    xt = np.tile(np.array(CV.TRUTHS[0]), (nprob, 1))
    model = xt[:, :1] * np.exp(-(xt[:, 1:2] * t)) + xt[:, 2:3]
    x0 = xt * (1.0 + 0.1 * rng.uniform(-1, 1, xt.shape))
    o = ds.options(max_evals=500)
    base = None
    for label, conv in (("plain", None), ("reconvolution", nl.Convolve(k, origin=CV.ORIGIN, extend=CV.EXTEND))):
        mu = model if conv is None else CR.convolve(model, k, CV.ORIGIN, CV.EXT[CV.EXTEND])
        y = np.random.default_rng(7).poisson(mu).astype(np.float64)
        dt, dy, dx0 = (torch.from_numpy(np.ascontiguousarray(q)).to(ds.device) for q in (t, y, x0))
        res = [None]

        def call():
            res[0] = ds.curve_fit_batch(CV.KIND, dt, dy, dx0, ncomp=CV.K, baseline=CV.B, opts=o, stat=nl.Poisson(), conv=conv)
        med, lo, hi = bracket(torch, call, warm=2, calls=7)
        ok = sum(1 for s in res[0][7] if s == 0)
        bias = 100.0 * float(((res[0][0].cpu().numpy()[:, 1] - xt[:, 1]) / xt[:, 1]).mean())
        base = med if base is None else base
        lines.append("%-16s %10.2f %10.2f %10.2f %8d %10.3f" % (label, med, lo, hi, ok, bias))
        print(lines[-1], flush=True)
        ratio = med / base
    lines.append("# reconvolution / plain: %.2f" % ratio)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
