"""The kernels that keep n-vectors in dynamic LDS, at the n where their request reaches the cap of nlh_create
(NLH_LDS_MAX = 160 KiB - 2 KiB = 161,792 B) and where each one switches to its global-memory form or refuses the size:

  k_lmpar<EXACT>  (6 n + 72 + 2736) doubles      in LDS to n = 2902, global memory beyond (nlh_lm.hip)
  k_lu_solve      12 n + 4144 B                  in LDS to n = 13137, global memory beyond (nlh_kernels_lu.h)
  nlh_lmpar       (6 n + 72) doubles             to n = 3358, NLH_ARRAY_SIZE_ERROR beyond
  k_lmpar<EXACT>, n <= 256: lmsolve's ring behind the exact reductions' scratch (160,832 B at n = 256)

Each side of each switch is compared with the CPU oracle bit for bit where the oracle is affordable, else with an
independent evaluation of the residual at the returned point."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
COUNT_KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLH_ARRAY_SIZE_ERROR = 202


def _oracle_lm(oracle, A, b, gamma, x0, **o):
    Ah = np.asfortranarray(A.cpu().numpy().T)
    return oracle.dq_lm_solve(Ah, b.cpu().numpy(), gamma, x0.cpu().numpy(), opts=oracle.default_options(**o))


# ---- 1. the exact policy's lmpar across its LDS / global-memory switch ---------------------------------------------------
@pytest.mark.parametrize("n", [2902, 2903, 2950, 3000, 3001])
def test_exact_lm_across_the_lmpar_lds_switch(ds, n):
    """n = 2902 is the last size whose k_lmpar<EXACT> request (incl. the exact reductions' scratch) fits the LDS cap; from
    2903 on lmpar's vectors go to global memory.  A linear zero-residual problem (gamma = 0, sigma = 0), m = n + 32: the
    solve must end converged, at a residual of rounding level that an independent evaluation at the returned x reproduces
    bit for bit.  (The oracle needs minutes per factorisation at this size; the bits of the two forms are held to each
    other by test_lmpar_lds_and_global_forms_agree_at_the_edge.)"""
    m = n + 32
    A, b, xt, x0 = ds.generate(1, m, n, seed0=n, gamma=0.0, sigma=0.0, spread=0.1)
    x = x0.clone()
    f, ibs, st = ds.lm_solve_batch(A, b, 0.0, x, ds.options(max_evals=50, factor_policy=2))
    assert st[0] == 0, (n, st, ibs)
    assert ibs[0]["converge_on_fcn"] or ibs[0]["converge_on_chng"] or ibs[0]["converge_on_zero_diff"], ibs[0]
    assert float(f.abs().max()) < 1e-6
    assert torch.equal(ds.residual(A, b, 0.0, x), f)


# ---- 2. the two forms of k_lmpar<EXACT> agree bit for bit at the real edge ------------------------------------------------
_LM_EDGE = '''
import numpy as np, sys
from nonlin_amd.device import DeviceSolver
ds = DeviceSolver(0)
m, n = 2934, 2902
A, b, xt, x0 = ds.generate(1, m, n, seed0=2902, gamma=10.0, sigma=1.0, spread=50.0)
x = x0.clone()
f, ibs, st = ds.lm_solve_batch(A, b, 10.0, x, ds.options(max_evals=3, factor=0.1, factor_policy=2))
np.savez(sys.argv[1], x=x.cpu().numpy(), f=f.cpu().numpy(), st=np.array(st),
         counts=np.array([ibs[0][k] for k in ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng",
                                              "converge_on_zero_diff")]))
print("ok")
'''


def _run_py(code, env, *args):
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout, out.stderr


def _slow_lmpar(stderr):
    """slow_lmpar of problem 0 from the NLH_DEBUG_LAG line: how often lmpar ended with par != 0 (its iteration ran)."""
    lines = [ln.split() for ln in stderr.splitlines() if ln.startswith("lag 0 ")]
    assert len(lines) == 1, stderr[-2000:]
    w = lines[0]
    return int(w[w.index("slow_lmpar") + 1])


def test_lmpar_lds_and_global_forms_agree_at_the_edge(tmp_path):
    """n = 2902, m = 2934, a family whose trust region binds (factor 0.1): once with lmpar's vectors in LDS (the default
    there) and once in global memory (NLH_LM_LDS_MAX_N=2901; read once per process, hence the subprocesses).  x, fvec,
    status and every count bit for bit, and lmpar's iteration ran (slow_lmpar > 0)."""
    res = []
    for tag, env in (("lds", {}), ("global", {"NLH_LM_LDS_MAX_N": "2901"})):
        path = str(tmp_path / f"{tag}.npz")
        out, err = _run_py(_LM_EDGE, dict(env, NLH_DEBUG_LAG="1"), path)
        assert "ok" in out
        assert _slow_lmpar(err) > 0, tag
        res.append(np.load(path))
    a, g = res
    for k in ("st", "counts", "x", "f"):
        assert np.array_equal(a[k], g[k]), k


# ---- 3. the exact-policy-only code of k_lmpar at the ring's edges --------------------------------------------------------
@pytest.mark.parametrize("n", [64, 65, 128, 129, 255, 256])
def test_exact_lmpar_ring_edges_match_oracle_and_global_sweep(ds, oracle, n):
    """k_lmpar<EXACT> with lmsolve's ring behind the exact reductions' scratch, the single-wave back substitution and the
    lanes form of the NORM2 chain: 256 / 512 / 1024-thread workgroups on either side of 64 and 128, and n = 255 / 256
    within 1 KB of the LDS cap.  m = 2 n, two problems of a family whose trust region binds: x, fvec, status and every count
    bit-identical to the oracle, the oracle's lmpar iteration entered, and the same bits again with the global-memory
    wavefront of lmsolve (NLH_LMSOLVE_GLOBAL=1, read on every call)."""
    m, nprob, gamma = 2 * n, 2, 10.0
    opts = dict(max_evals=30, factor=0.1)
    A, b, xt, x0 = ds.generate(nprob, m, n, seed0=4000 + n, gamma=gamma, sigma=1.0, spread=50.0)
    x = x0.clone()
    f, ibs, st = ds.lm_solve_batch(A, b, gamma, x, ds.options(factor_policy=2, **opts))
    oracle.lmpar_loop_entries(reset=True)
    for p in range(nprob):
        rc, xo, fo, ibo = _oracle_lm(oracle, A[p], b[p], gamma, x0[p], **opts)[:4]
        assert st[p] == rc, (n, p, st[p], rc)
        for k in COUNT_KEYS:
            assert ibs[p][k] == ibo[k], (n, p, k, ibs[p], ibo)
        assert np.array_equal(x[p].cpu().numpy(), xo) and np.array_equal(f[p].cpu().numpy(), fo), (n, p)
    assert oracle.lmpar_loop_entries(reset=True) > 0
    xg = x0.clone()
    os.environ["NLH_LMSOLVE_GLOBAL"] = "1"
    try:
        fg, ibg, stg = ds.lm_solve_batch(A, b, gamma, xg, ds.options(factor_policy=2, **opts))
        torch.cuda.synchronize()
    finally:
        os.environ.pop("NLH_LMSOLVE_GLOBAL", None)
    assert stg == st and ibg == ibs
    assert torch.equal(xg, x) and torch.equal(fg, f)


# ---- 4. k_lu_solve on either side of its LDS switch ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [13137, 13138, 13200, 13312])
def test_lu_solve_across_its_lds_switch(ds, oracle, n):
    """solve_lu on a packed LU built directly (no factorisation: both sides stay O(n^2)): a unit-lower L and an upper U with
    entries of size 1/n and a diagonal in [1, 2), random valid pivots (0-based, as lu_factor returns them).  n = 13137 is the
    last size whose LDS form fits the cap; 13138 and 13200 take the global-memory form; 13312 also exceeds the 160 KiB of a
    CU, which the LDS form could not be launched with at all.  Bit-identical to the oracle.  (One n-by-n host array alive
    at a time: 1.4 GB each.)"""
    rng = np.random.default_rng(n)
    M = rng.random((n, n))                              # M[j, i] = a(i, j): column-major problem storage
    M -= 0.5
    M *= 2.0 / n
    M.flat[::n + 1] = 1.0 + rng.random(n)
    ipvt = np.array([rng.integers(j, n) for j in range(n)], dtype=np.int32)
    bh = rng.standard_normal(n)
    xo = bh.copy()
    oracle.lib().nlo_lu_solve(n, M.ctypes.data_as(C.POINTER(C.c_double)), n, ipvt.ctypes.data_as(C.POINTER(C.c_int32)),
                              xo.ctypes.data_as(C.POINTER(C.c_double)))
    LU = torch.from_numpy(M).to(ds.device).unsqueeze(0)
    del M
    bd = torch.tensor(bh, device=ds.device).unsqueeze(0)
    ds.lu_solve(LU, torch.tensor(ipvt, device=ds.device).unsqueeze(0), bd)
    torch.cuda.synchronize()
    del LU
    assert np.isfinite(xo).all()
    assert np.array_equal(bd[0].cpu().numpy(), xo)


# ---- 5. Newton beyond the LDS form of k_lu_solve ---------------------------------------------------------------------------
def test_newton_at_13138_unknowns(ds):
    """newton_solver at n = 13138 (the LU solve in global memory; the built-in family goes to 20000): a linear system
    (gamma = 0, sigma = 0) with a shifted diagonal, analytic Jacobian: one Newton step lands on the solution.  The solve
    must end converged, with a residual that an independent evaluation at the returned x reproduces bit for bit.  (The
    oracle's LU alone takes many minutes at this size; the bits of the LU solve are held to it by
    test_lu_solve_across_its_lds_switch.)"""
    n = 13138
    A, b, xt, x0 = ds.generate(1, n, n, seed0=13138, gamma=0.0, sigma=0.0, spread=0.1, square_shift=True)
    x = x0.clone()
    f, ibs, st = ds.newton_solve_batch(A, b, 0.0, x, analytic=True, opts=ds.options(max_evals=4))
    assert st[0] == 0, (st, ibs)
    assert ibs[0]["converge_on_fcn"] == 1 and ibs[0]["jacobian_count"] <= 2, ibs[0]
    assert float(f.abs().max()) < 1e-8
    assert torch.equal(ds.residual(A, b, 0.0, x), f)
    assert float((x - xt).abs().max()) < 1e-8


# ---- 6. nlh_lmpar, the single-stage entry point: its size bound ------------------------------------------------------------
def _lmpar_inputs(n, seed):
    """A well-conditioned upper-triangular R (diagonal in [1, 2), entries of size 1/n above it), the identity pivot order,
    diag = 1 and a delta large enough that the Gauss-Newton step is accepted (lmpar returns par = 0 after one triangular
    solve: O(n^2) in the oracle)."""
    rng = np.random.default_rng(seed)
    R = np.triu(rng.random((n, n)) - 0.5) * (2.0 / n)
    R[np.arange(n), np.arange(n)] = 1.0 + rng.random(n)
    qtf = rng.standard_normal(n)
    return R, np.arange(n, dtype=np.int32), np.ones(n), qtf, 10.0 * np.linalg.norm(qtf)


@pytest.mark.parametrize("n", [3358, 3359])
def test_lmpar_entry_point_at_its_lds_bound(ds, oracle, n):
    """n = 3358: (6 n + 72) doubles = 161,760 B fit the cap, and the result agrees with the oracle (to the tolerance of
    test_lmpar_binding_trust_region); n = 3359 does not fit, and nlh_lmpar says NLH_ARRAY_SIZE_ERROR before it touches
    anything (its outputs keep their values)."""
    R, ip, diag, qtf, delta = _lmpar_inputs(n, n)
    dev = ds.device
    f64 = dict(dtype=torch.float64, device=dev)
    Rd = torch.tensor(np.ascontiguousarray(R.T), **f64).unsqueeze(0)          # [1, n (column), n (row)]
    ipd = torch.tensor(ip, device=dev).unsqueeze(0)
    diagd, qtfd = torch.tensor(diag, **f64).unsqueeze(0), torch.tensor(qtf, **f64).unsqueeze(0)
    deltad, tailsq, par = torch.tensor([delta], **f64), torch.tensor([0.0], **f64), torch.tensor([0.0], **f64)
    x = torch.full((1, n), -7.0, **f64)
    sdiag = torch.full((1, n), -7.0, **f64)
    rc = ds.lib.nlh_lmpar(ds.h.ptr, 1, n, Rd.data_ptr(), n, ipd.data_ptr(), diagd.data_ptr(), qtfd.data_ptr(),
                          deltad.data_ptr(), tailsq.data_ptr(), par.data_ptr(), x.data_ptr(), sdiag.data_ptr())
    torch.cuda.synchronize()
    if n > 3358:
        assert rc == NLH_ARRAY_SIZE_ERROR
        assert bool((x == -7.0).all()) and bool((sdiag == -7.0).all()) and float(par[0]) == 0.0
        return
    assert rc == 0
    a = np.zeros((n, n), order="F")
    a[:, :] = R
    par_o, x_o, sdiag_o, _ = oracle.lmpar(a, ip, diag, qtf, delta, 0.0, qtf.copy())
    assert par_o == 0.0 == float(par[0])
    np.testing.assert_allclose(x[0].cpu().numpy(), x_o, rtol=0, atol=1e-10 * np.abs(x_o).max())
