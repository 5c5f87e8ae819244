"""GPU test of the separable fits through the Fortran drop-in layer (device_model_batch%create_separable and the one-call
interface nlh_curve_fit_batch_sep_h of nonlin_hip_c): the user program tests/fortran_sep/sep_fit.f90, linked with
nonlin_amd/fortran and libnonlin_hip.so, against the Python front end."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sep_cases as SC
import nonlin_amd as nl

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fortran_sep_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_sep")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "sep_fit")


def test_fortran_separable_fit(ds, fortran_sep_exe, tmp_path):
    """The Fortran user program (create_curve -> create_separable -> solve_batch -> covariance_batch, then the one-call
    nlh_curve_fit_batch_sep_h: Lorentzian doublets on a line, amplitudes and baseline projected out) prints the x, sigma and
    counts of the Python path, digit for digit (ES24.16)."""
    import torch
    K, B, m, nprob = 2, 1, 120, 5
    t, y, xt, x0 = SC.lorentz_problems(K, B, m, nprob, seed=23)
    path = str(tmp_path / "sep.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(x0.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_sep_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ds.device)
    o = ds.options(max_evals=SC.MAX_EVALS)
    dt, dy, dx0 = dev(t), dev(y), dev(x0)
    sp = nl.Separable.for_curve("lorentz", K, B)
    fcn, jac, ctx = ds.curve_launchers("lorentz", K, B, dt, dy)
    wf, wj, wctx = ds.sep_launchers(sp, fcn, jac, ctx)
    a = ds.sep_gather(sp, dx0)
    fvec, ibs, st = ds.lm_solve_batch_device(wf, wctx, m, a, jac=wj, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, m, a, jac=wj)
    fit = ds.curve_fit_batch("lorentz", dt, dy, dx0, ncomp=K, baseline=B, opts=o, sep=sp)
    assert set(st) == {0} and set(fit[7]) == {0}
    want = []
    for tag, xs, ss, ib, rk in (("a", a, sigma, ibs, rank), ("", fit[0], fit[2], fit[6], fit[5])):
        xh, sh = xs.cpu().numpy(), ss.cpu().numpy()
        names = ("a", "asigma", "acounts") if tag else ("x", "sigma", "counts")
        for p in range(nprob):
            want.append("%s %d" % (names[0], p + 1) + "".join("%24.16E" % v for v in xh[p]))
            want.append("%s %d" % (names[1], p + 1) + "".join("%24.16E" % v for v in sh[p]))
            want.append("%s %d %d %d %d %d" % (names[2], p + 1, ib[p]["iter_count"], ib[p]["fcn_count"], ib[p]["jacobian_count"], int(rk[p])))
    lines = [" ".join(ln.split()) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1] == "done"
    assert lines[:-1] == [" ".join(w_.split()) for w_ in want], out.stdout
    wctx.close()
