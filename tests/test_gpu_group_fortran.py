"""GPU test of the global fits through the Fortran drop-in layer (device_model_batch%create_global): the user program
tests/fortran_group/group_fit.f90, linked with nonlin_amd/fortran and libnonlin_hip.so, against the Python front end."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import group_cases as GC
import group_restatement as GR
import nonlin_amd as nl

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fortran_group_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_group")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "group_fit")


def test_fortran_global_fit(ds, fortran_group_exe, tmp_path):
    """The Fortran user program (create_curve -> create_global -> solve_batch -> covariance_batch: Lorentzian doublets whose
    peak positions are common to a group of three) prints the x, sigma and counts of the Python path, digit for digit
    (ES24.16); the one-call fit reports the same solution per data set."""
    import torch
    kind, K, B, m, G, shared = "lorentz", 2, 0, 120, 3, (1, 4)
    ngroup = 4
    nprob = ngroup * G
    t, y, xt, x0 = GC.problems(kind, K, B, m, G, shared, ngroup=ngroup, seed=31)
    path = str(tmp_path / "groups.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, m, G], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(y.tobytes()); fh.write(x0.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_group_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ds.device)
    o = ds.options(max_evals=GC.MAX_EVALS)
    dt, dy, dx0 = dev(t), dev(y), dev(x0)
    grp = nl.Group(7, shared=shared, nsets=G)
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy)
    wf, wj, wctx = ds.group_launchers(grp, fcn, jac, ctx)
    x = ds.group_gather(grp, dx0)
    assert np.array_equal(x.cpu().numpy(), GR.gather(GR.tables(7, shared, G), x0))
    fvec, ibs, st = ds.lm_solve_batch_device(wf, wctx, G * m, x, jac=wj, opts=o)
    cov, sigma, rank, chi2 = ds.lm_covariance_batch_device(wf, wctx, G * m, x, jac=wj)
    xh, sh = x.cpu().numpy(), sigma.cpu().numpy()
    want = []
    for p in range(ngroup):
        want.append("x %d" % (p + 1) + "".join("%24.16E" % v for v in xh[p]))
        want.append("sigma %d" % (p + 1) + "".join("%24.16E" % v for v in sh[p]))
        want.append("counts %d %d %d %d %d" % (p + 1, ibs[p]["iter_count"], ibs[p]["fcn_count"], ibs[p]["jacobian_count"], int(rank[p])))
    lines = [" ".join(ln.split()) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1] == "done"
    assert lines[:-1] == [" ".join(w_.split()) for w_ in want], out.stdout
    fit = ds.curve_fit_batch(kind, dt, dy, dx0, ncomp=K, baseline=B, opts=o, group=grp)
    assert torch.equal(fit[0], ds.group_expand(grp, x)) and fit[6] == ibs and set(fit[7]) == {0}
    wctx.close()
