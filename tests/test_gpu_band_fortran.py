"""GPU test of the bands through the Fortran drop-in layer (least_squares_solver%propagate_batch over
nlh_dq_model_propagate): the user program tests/fortran_band/band.f90, linked with nonlin_amd/fortran and
libnonlin_hip.so, against the Python front end."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import curve_cases as CC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fortran_band_exe():
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if fc is None:
        pytest.skip("no Fortran compiler")
    d = os.path.join(HERE, "fortran_band")
    subprocess.check_call(["make", "-C", d, "-s", "FC=" + fc])
    return os.path.join(d, "band")


def test_fortran_propagate_batch(ds, fortran_band_exe, tmp_path):
    """create_curve on a grid (y = 0), then propagate_batch without and with noise: the printed val, sd and prediction sd are
    those of DeviceSolver.curve_band for the same x and cov, digit for digit (ES24.16)."""
    import torch
    K, B, nprob, npts = 2, 0, 4, 45
    _, _, x, _ = CC.curve_problems("lorentz", K, B, 64, nprob=nprob, seed=19)
    n = x.shape[1]
    rng = np.random.default_rng(19)
    t = np.sort(rng.uniform(-0.1, 1.1, (nprob, npts)))
    a = rng.standard_normal((nprob, n, n + 2))
    c = a @ np.transpose(a, (0, 2, 1)) * 1e-4
    cov = 0.5 * (c + np.transpose(c, (0, 2, 1)))                     # symmetric to the bit: either memory order is the same matrix
    assert np.array_equal(cov, np.transpose(cov, (0, 2, 1)))
    noise = rng.uniform(1e-4, 1e-3, nprob)
    path = str(tmp_path / "band.bin")
    with open(path, "wb") as fh:
        fh.write(np.array([nprob, npts, K, B], dtype=np.int32).tobytes())
        fh.write(t.tobytes()); fh.write(x.tobytes()); fh.write(cov.tobytes()); fh.write(noise.tobytes())
    out = subprocess.run(["timeout", "-k", "10", "300", fortran_band_exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(ds.device)
    y, sd = ds.curve_band("lorentz", dev(x), dev(cov), dev(t), ncomp=K, baseline=B)
    _, pred = ds.curve_band("lorentz", dev(x), dev(cov), dev(t), ncomp=K, baseline=B, noise=dev(noise))
    yh, sh, ph = y.cpu().numpy(), sd.cpu().numpy(), pred.cpu().numpy()
    want = []
    for p in range(nprob):
        for name, v in (("val", yh), ("sd", sh), ("pred", ph)):
            want.append("%s %d" % (name, p + 1) + "".join("%24.16E" % w for w in v[p]))
    lines = [" ".join(ln.split()) for ln in out.stdout.splitlines() if ln.strip()]
    assert lines[-1] == "done"
    assert lines[:-1] == [" ".join(w_.split()) for w_ in want], out.stdout
