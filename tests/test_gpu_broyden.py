"""GPU parity tests for quasi_newton_solver (qns_solve, src/nonlin_solve.f90:156-427) and the dense
kernels behind it: Householder QR with Q formed, the rank-one QR update, the triangular solve.

The CPU restatement performs every sum in ascending index order and the kernels do exactly the same
operations on every element, so the comparisons are bitwise.  Problems follow the reference's
test_quasinewton_1..4 (tests/nonlin_test_solve.f90:187-360, 851-896)."""
import numpy as np
import pytest
import torch

import problems_ref as P

pytestmark = pytest.mark.gpu

COUNT_KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng",
              "converge_on_zero_diff")


def _dev(M, dev):
    """numpy matrix -> device tensor holding it column-major (tensor[j][i] = M[i, j])."""
    return torch.from_numpy(np.ascontiguousarray(M.T)).to(dev)


@pytest.mark.parametrize("n", [1, 2, 7, 64, 130, 300])
def test_qr_factor_full_bitwise(ds, oracle, n):
    rng = np.random.default_rng(n)
    Ms = [rng.standard_normal((n, n)) for _ in range(2)]
    if n >= 7:
        Ms[1][3:, 2] = 0.0                         # an H = I step (column already upper triangular)
    B = torch.stack([_dev(M, ds.device) for M in Ms])
    Q, Rt = ds.qr_factor_full(B)
    for p, M in enumerate(Ms):
        qo, ro = oracle.qr_factor_full(M)
        assert np.array_equal(Rt[p].cpu().numpy(), ro)
        assert np.array_equal(Q[p].cpu().numpy().T, qo)
        assert np.abs(qo @ ro - M).max() <= 1e-12 * max(1.0, np.abs(M).max()) * n


@pytest.mark.parametrize("n", [1, 2, 7, 64, 300, 1100])
def test_qr_rank1_update_bitwise(ds, oracle, n):
    rng = np.random.default_rng(100 + n)
    nprob = 2
    Ms = [rng.standard_normal((n, n)) for _ in range(nprob)]
    us = [rng.standard_normal(n) for _ in range(nprob)]
    vs = [rng.standard_normal(n) for _ in range(nprob)]
    qr = [oracle.qr_factor_full(M) for M in Ms]
    Q = torch.stack([_dev(q, ds.device) for q, r in qr])
    Rt = torch.stack([torch.from_numpy(np.ascontiguousarray(r)).to(ds.device) for q, r in qr])
    u = torch.from_numpy(np.stack(us)).to(ds.device)
    v = torch.from_numpy(np.stack(vs)).to(ds.device)
    ds.qr_rank1_update(Q, Rt, u, v)
    for p in range(nprob):
        q1, r1 = oracle.qr_rank1_update(qr[p][0], qr[p][1], us[p], vs[p])
        assert np.array_equal(Rt[p].cpu().numpy(), r1)
        assert np.array_equal(Q[p].cpu().numpy().T, q1)
        assert np.abs(q1 @ r1 - (Ms[p] + np.outer(us[p], vs[p]))).max() <= 1e-11 * n


@pytest.mark.parametrize("n", [1, 5, 64, 700])
def test_solve_upper_bitwise(ds, oracle, n):
    rng = np.random.default_rng(7 * n)
    R = np.triu(rng.standard_normal((n, n))) + 3.0 * np.eye(n)
    b = rng.standard_normal(n)
    b[n // 2] = 0.0
    Rt = torch.from_numpy(np.ascontiguousarray(R)).to(ds.device)[None]
    x = torch.from_numpy(b.copy()).to(ds.device)[None]
    ds.solve_upper(Rt, x)
    assert np.array_equal(x[0].cpu().numpy(), oracle.solve_upper(R, b))


# ---- the size edges of the two neighbours of the Householder steps (tests/test_gpu_house.py has those) ----
NLH_ARRAY_SIZE_ERROR = 202


def _rand(rng, shape):
    """Generic float64 values, uniform in [-1/2, 1/2) (a fraction of the time a normal draw takes at 8192 x 8192; the
    comparisons below are operation for operation, so any generic value serves)."""
    return rng.random(shape) - 0.5


def _upper_t(rng, n, zero_rows=()):
    """L = R^T (C order, so that L.T is R in Fortran order without a copy) of a well-conditioned upper triangular R:
    off-diagonal entries of size 1 / sqrt(n), diagonal near 3, a few exact zeros above the diagonal, and the rows of
    zero_rows zero to the right of their diagonal."""
    L = np.tril(_rand(rng, (n, n)))
    L *= 1.0 / np.sqrt(n)
    L[np.arange(n), np.arange(n)] += 3.0
    for i, j in zip(rng.integers(0, n, 8), rng.integers(0, n, 8)):
        if i < j:
            L[j, i] = 0.0
    for i in zero_rows:
        L[i + 1:, i] = 0.0
    return L


def _solve_upper_ref(oracle, Rf, b):
    """nlo_solve_upper on a Fortran-order R that is passed as it is (oracle.solve_upper copies R on every call)."""
    import ctypes
    assert Rf.flags.f_contiguous and Rf.dtype == np.float64
    x = np.array(b, dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    oracle.lib().nlo_solve_upper(Rf.shape[0], Rf.ctypes.data_as(dp), x.ctypes.data_as(dp))
    return x


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097, 8192])
def test_solve_upper_bitwise_at_the_edges(ds, oracle, n):
    """k_qn_solve_upper at one, two and several 16-column blocks, a partial last block, one and several rows a thread
    (n > 1024: the rows a thread did not prefetch), with right-hand sides that make it skip columns: an x(j) that is
    exactly zero WHEN ITS TURN COMES -- not merely on entry -- which needs the row of R zero to the right of the diagonal.
    Five right-hand sides per R: dense; zeros scattered over such rows; one whole aligned block of sixteen of them (the
    block's skip); the last entry; all zero.  Two problems with their own R below n = 4097, one from there."""
    rng = np.random.default_rng(9000 + n)
    nprob = 2 if n < 4097 else 1
    nblk = (n + 15) // 16
    blk = np.arange(16 * (nblk // 2), min(n, 16 * (nblk // 2) + 16))     # an aligned block (n < 16: all there is)
    scat = np.unique(np.concatenate([rng.integers(0, n, max(1, n // 7)), [0, n - 1, min(n - 1, 1030)]]))
    Ls = [_upper_t(rng, n, zero_rows=np.union1d(blk, scat)) for _ in range(nprob)]
    Rfs = [L.T for L in Ls]
    Rt = torch.stack([torch.from_numpy(L) for L in Ls]).to(ds.device).transpose(1, 2).contiguous()     # row-major R
    for pattern in ("dense", "scattered", "block", "last", "allzero"):
        b = _rand(rng, (nprob, n))
        b[b == 0.0] = 1.0
        if pattern == "scattered":
            b[:, scat] = 0.0
        elif pattern == "block":
            b[:, blk] = 0.0
        elif pattern == "last":
            b[:, n - 1] = 0.0
        elif pattern == "allzero":
            b[:] = 0.0
        x = torch.from_numpy(b.copy()).to(ds.device)
        ds.solve_upper(Rt, x)
        xg = x.cpu().numpy()
        for p in range(nprob):
            xo = _solve_upper_ref(oracle, Rfs[p], b[p])
            assert np.isfinite(xo).all()
            assert np.array_equal(xg[p], xo), (pattern, p, int(np.argmax(xg[p] != xo)))
            if pattern == "scattered":
                assert not xo[scat].any()
            elif pattern == "block":
                assert not xo[blk].any() and (n <= 16 or np.count_nonzero(xo) == n - len(blk))


def test_solve_upper_refuses_what_lds_cannot_hold(ds):
    """x lives in LDS: n = 20225 is beyond any workgroup's share and is refused with NLH_ARRAY_SIZE_ERROR before the
    launch, x untouched (the tensors are of the full size, on the device only)."""
    n = 20225
    Rt = torch.zeros((1, n, n), dtype=torch.float64, device=ds.device)
    x = torch.full((1, n), 7.0, dtype=torch.float64, device=ds.device)
    assert ds.lib.nlh_solve_upper(ds.h.ptr, 1, n, Rt.data_ptr(), x.data_ptr()) == NLH_ARRAY_SIZE_ERROR
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())
    with pytest.raises(RuntimeError):
        ds.solve_upper(Rt, x)


def _arrow_solve_ref(d, c, f, b):
    """x = R^-1 b in nlo_solve_upper's order of operations for R = diag(d) with a dense last column c (c[n-1] = d[n-1])
    and a dense first row f (f[0] = d[0], f[n-1] = c[0]), every other entry zero: columns from the last to the first,
    x(j) = x(j) / r(j,j), then x(i) = x(i) - x(j) r(i,j) for the rows above -- which leaves x(i) as it is wherever r(i,j) = 0."""
    n = len(d)
    x = np.array(b, dtype=np.float64)
    if n > 1:
        x[n - 1] = x[n - 1] / d[n - 1]
        x[:n - 1] = x[:n - 1] - x[n - 1] * c[:n - 1]
        x[1:n - 1] = x[1:n - 1] / d[1:n - 1]
        x0 = float(x[0])
        for xj, fj in zip(x[n - 2:0:-1].tolist(), f[n - 2:0:-1].tolist()):
            x0 = x0 - xj * fj
        x[0] = x0
    x[0] = x[0] / d[0]
    return x


def test_solve_upper_at_the_lds_edge(ds, oracle):
    """x (8 n bytes) and the kernel's own 4,104 bytes of LDS fill the 161,792 bytes a workgroup may have exactly at
    n = 19711: that size is solved, to the bit, and n = 19712 is refused with x untouched.  A dense R of this size would
    be 3 GB on the host, so R is built on the device -- a diagonal, a dense last column and a dense first row -- and the
    reference is the restatement's operations written out for that pattern (_arrow_solve_ref), itself held to
    nlo_solve_upper at a small size here."""
    def parts(n, seed):
        rng = np.random.default_rng(seed)
        d, c, f, b = 3.0 + _rand(rng, n), _rand(rng, n), _rand(rng, n), _rand(rng, n) + 2.0
        c[n - 1], f[0], f[n - 1] = d[n - 1], d[0], c[0]
        return d, c, f, b

    d, c, f, b = parts(40, 1)
    R = np.diag(d)
    R[:, 39], R[0, :] = c, f
    assert np.array_equal(_arrow_solve_ref(d, c, f, b), oracle.solve_upper(R, b))

    n = 19711
    buf = torch.zeros((n + 1) * (n + 1), dtype=torch.float64, device=ds.device)
    d, c, f, b = parts(n, 2)
    Rt = buf[:n * n].view(1, n, n)
    Rt[0].diagonal().copy_(torch.from_numpy(d))
    Rt[0][:, n - 1] = torch.from_numpy(c).to(ds.device)
    Rt[0][0, :] = torch.from_numpy(f).to(ds.device)
    x = torch.from_numpy(b.copy()).to(ds.device)[None]
    ds.solve_upper(Rt, x)
    xo = _arrow_solve_ref(d, c, f, b)
    assert np.isfinite(xo).all() and np.array_equal(x[0].cpu().numpy(), xo)

    n = 19712
    buf.zero_()
    x = torch.full((1, n), 7.0, dtype=torch.float64, device=ds.device)
    assert ds.lib.nlh_solve_upper(ds.h.ptr, 1, n, buf.data_ptr(), x.data_ptr()) == NLH_ARRAY_SIZE_ERROR
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())


@pytest.mark.parametrize("n", [1, 2, 3, 9, 10, 255, 256, 257, 1024, 1025, 4096, 4097, 8192])
def test_qr_rank1_update_bitwise_at_the_edges(ds, oracle, n):
    """The switches of k_qn_retri (one, four, eight columns a thread: 1024 / 1025, 4096 / 4097) and the tile edges of the
    kernels around it.  The comparison is operation for operation, so Q need not be orthogonal: Q is random dense, scaled
    by 1 / sqrt(n), R random upper triangular, and the oracle stays O(n^2).  Problem 0 (below n = 4096, where there are
    two) is dense: every rotation takes the general branch of the Givens routine.  The last problem reaches both early
    ones: some columns of its Q are unit vectors e_k with u_k = 0, so Q^T u is exactly zero there -- a run at the end
    (g = 0) and one in the middle (f = 0) -- and its v has zeros."""
    rng = np.random.default_rng(9100 + n)
    nprob = 2 if n < 4096 else 1
    Qt = _rand(rng, (nprob, n, n)) / np.sqrt(n)                 # Qt[p][j, i] = Q_p(i, j): the device layout
    Lt = np.stack([np.tril(_rand(rng, (n, n))) for _ in range(nprob)])      # Lt[p] = R_p^T, so Lt[p].T is R_p in Fortran order
    u, v = _rand(rng, (nprob, n)), _rand(rng, (nprob, n))
    p = nprob - 1
    cols = list(range(n - max(1, n // 4), n)) + ([n // 3] if n >= 9 else [])
    if n >= 2:
        ks = rng.choice(n, size=len(cols), replace=False)
        Qt[p][cols, :] = 0.0
        Qt[p][cols, ks] = 1.0
        u[p][ks] = 0.0
        v[p][rng.integers(0, n, max(1, n // 5))] = 0.0
        w = Qt[p] @ u[p]
        assert not w[cols].any() and np.count_nonzero(w) == n - len(cols)
    Qd = torch.from_numpy(Qt).to(ds.device)
    Rd = torch.from_numpy(Lt).to(ds.device).transpose(1, 2).contiguous()                # row-major R
    ds.qr_rank1_update(Qd, Rd, torch.from_numpy(u.copy()).to(ds.device), torch.from_numpy(v.copy()).to(ds.device))
    for p in range(nprob):
        q1, r1 = oracle.qr_rank1_update(Qt[p].T, Lt[p].T, u[p], v[p])
        assert np.isfinite(r1).all() and np.isfinite(q1).all()
        # compared on the device, in the layouts the arrays have (q1.T and r1.T are C-contiguous views)
        assert torch.equal(Rd[p].t(), torch.from_numpy(r1.T).to(ds.device)), (p, "R")
        assert torch.equal(Qd[p], torch.from_numpy(q1.T).to(ds.device)), (p, "Q")
        assert not bool(torch.tril(Rd[p], -1).any())


def test_qr_entry_points_refuse_beyond_8192(ds):
    """n = 8193: nlh_qr_rank1_update and nlh_qr_factor_full return NLH_ARRAY_SIZE_ERROR (the quasi-Newton solver's own
    bound; the factorisation's launch arithmetic is sized for it) and leave Q and R untouched."""
    n = 8193
    Q = torch.full((1, n, n), 3.0, dtype=torch.float64, device=ds.device)
    Rt = torch.full((1, n, n), 4.0, dtype=torch.float64, device=ds.device)
    u = torch.ones((1, n), dtype=torch.float64, device=ds.device)
    assert ds.lib.nlh_qr_rank1_update(ds.h.ptr, 1, n, Q.data_ptr(), Rt.data_ptr(), u.data_ptr(), u.data_ptr()) == NLH_ARRAY_SIZE_ERROR
    B = torch.zeros((1, n, n), dtype=torch.float64, device=ds.device)
    assert ds.lib.nlh_qr_factor_full(ds.h.ptr, 1, n, B.data_ptr(), Q.data_ptr(), Rt.data_ptr()) == NLH_ARRAY_SIZE_ERROR
    torch.cuda.synchronize()
    assert bool((Q == 3.0).all()) and bool((Rt == 4.0).all())
    with pytest.raises(RuntimeError):
        ds.qr_rank1_update(Q, Rt, u, u)


def _solve_host(fcn, n, x0, jac=None, use_ls=True, args=None, jdelta=None):
    import nonlin_amd as nl
    obj = nl.vecfcn_helper()
    obj.set_fcn(fcn, n, n)
    if jac is not None:
        obj.set_jacobian(jac)
    s = nl.quasi_newton_solver()
    s.set_use_line_search(use_ls)
    if jdelta is not None:
        s.set_jacobian_interval(jdelta)
    x = np.array(x0, dtype=np.float64)
    f = np.zeros(n)
    ib = nl.iteration_behavior()
    s.solve(obj, x, f, ib, args=args)
    return x, f, ib


def _same(ib, ibo):
    return all(getattr(ib, k) == ibo[k] for k in COUNT_KEYS)


@pytest.mark.parametrize("ic", [(0.5, 0.5), (1.0, 1.0)])
@pytest.mark.parametrize("with_jac", [True, False])
def test_host_quasinewton_1(oracle, ic, with_jac):
    """test_quasinewton_1 / 3 (:187-234, :290-360): x -> (+-5, +-3) within 1e-6."""
    x, f, ib = _solve_host(P.fcn1, 2, ic, jac=P.jac1 if with_jac else None)
    rc, xo, fo, ibo = oracle.quasi_newton_solve(lambda a, b: P.fcn1(a, b, None), 2, ic,
                                                jac=(lambda a, b: P.jac1(a, b, None)) if with_jac else None)
    assert rc == 0
    assert abs(abs(x[0]) - 5.0) <= 1e-6 and abs(abs(x[1]) - 3.0) <= 1e-6
    assert _same(ib, ibo), (ib.as_dict(), ibo)
    assert np.array_equal(x, xo) and np.array_equal(f, fo)


@pytest.mark.parametrize("ic", [(0.5, 0.5), (1.0, 1.0)])
def test_host_quasinewton_2_no_linesearch(oracle, ic):
    """test_quasinewton_2 (:237-287): badly scaled, FD Jacobian, line search off."""
    x, f, ib = _solve_host(P.fcn2, 2, ic, use_ls=False)
    rc, xo, fo, ibo = oracle.quasi_newton_solve(lambda a, b: P.fcn2(a, b, None), 2, ic,
                                                opts=oracle.default_options(use_line_search=0))
    assert rc == 0
    assert abs(abs(x[0]) - 5.0e3) <= 1e-6 and abs(abs(x[1]) - 10.0) <= 1e-6
    assert _same(ib, ibo)
    assert np.array_equal(x, xo)


@pytest.mark.parametrize("with_jac", [False, True])
def test_host_quasinewton_3_args(oracle, with_jac):
    """test_quasinewton_3 (:290-360): the optional args reaches the user's routines."""
    x, f, ib = _solve_host(P.fcn1a, 2, [1.0, 1.0], jac=P.jac1a if with_jac else None, args=2.0)
    assert abs(abs(x[0]) - 5.0) <= 1e-6 and abs(abs(x[1]) - 3.0) <= 1e-6
    rc, xo, fo, ibo = oracle.quasi_newton_solve(lambda a, b: P.fcn1a(a, b, 2.0), 2, [1.0, 1.0],
                                                jac=(lambda a, b: P.jac1a(a, b, 2.0)) if with_jac else None)
    assert _same(ib, ibo)
    assert np.array_equal(x, xo)


def test_host_quasinewton_4_powell(oracle):
    """test_quasinewton_4 (:851-896): Powell badly scaled, analytic Jacobian, line search off, tol 1e-5."""
    x, f, ib = _solve_host(P.powell, 2, [0.0, 1.0], jac=P.powell_jac, use_ls=False)
    assert abs(x[0] - 1.098159e-5) <= 1e-5 and abs(x[1] - 9.106146) <= 1e-5
    rc, xo, fo, ibo = oracle.quasi_newton_solve(lambda a, b: P.powell(a, b, None), 2, [0.0, 1.0],
                                                jac=lambda a, b: P.powell_jac(a, b, None),
                                                opts=oracle.default_options(use_line_search=0))
    assert _same(ib, ibo)
    assert np.array_equal(x, xo)


def test_host_quasinewton_jacobian_interval(oracle):
    """set_jacobian_interval (:439-447) changes when the Jacobian is recomputed."""
    x1, f1, ib1 = _solve_host(P.fcn1, 2, [1.0, 1.0], jac=P.jac1, jdelta=1)
    rc, xo, fo, ibo = oracle.quasi_newton_solve(lambda a, b: P.fcn1(a, b, None), 2, [1.0, 1.0],
                                                jac=lambda a, b: P.jac1(a, b, None), jdelta=1)
    assert _same(ib1, ibo) and np.array_equal(x1, xo)
    x5, f5, ib5 = _solve_host(P.fcn1, 2, [1.0, 1.0], jac=P.jac1)
    assert ib1.jacobian_count > ib5.jacobian_count


@pytest.mark.parametrize("n,analytic,spread", [(16, True, 0.1), (64, True, 0.1), (64, False, 0.03), (256, True, 0.03),
                                               (256, True, 0.3)])
def test_dq_quasi_newton_batch_bitwise(ds, oracle, n, analytic, spread):
    """Square dense-quadratic systems (A <- 2I + A): x, fvec and every count equal the CPU path's bit for
    bit, including runs with Jacobian restarts."""
    nprob = 2
    A, b, xt, x0 = ds.generate(nprob, n, n, seed0=12345, sigma=0.0, spread=spread, square_shift=True)
    x = x0.clone()
    fvec, ibs, status = ds.quasi_newton_solve_batch(A, b, 0.5, x, analytic=analytic, opts=ds.options(max_evals=500))
    for p in range(nprob):
        Ah = np.asfortranarray(A[p].cpu().numpy().T)
        rc, xo, fo, ibo, _ = oracle.dq_quasi_newton_solve(Ah, b[p].cpu().numpy(), 0.5, x0[p].cpu().numpy(),
                                                          analytic=analytic, opts=oracle.default_options(max_evals=500))
        assert status[p] == rc
        for k in COUNT_KEYS:
            assert ibs[p][k] == ibo[k], (k, ibs[p], ibo)
        assert np.array_equal(x[p].cpu().numpy(), xo)
        assert np.array_equal(fvec[p].cpu().numpy(), fo)


def test_dq_quasi_newton_many_problems_concurrently(ds, oracle):
    """The batch entry points deal problems to worker threads with private streams (NLH_WORKERS, default 8): every
    problem must still come out bit-identical to the CPU path, whichever thread solved it and whatever ran beside it."""
    nprob, n = 24, 48
    A, b, xt, x0 = ds.generate(nprob, n, n, seed0=4321, sigma=0.0, spread=0.05, square_shift=True)
    x = x0.clone()
    fvec, ibs, status = ds.quasi_newton_solve_batch(A, b, 0.5, x, analytic=False, opts=ds.options(max_evals=500))
    for p in range(nprob):
        Ah = np.asfortranarray(A[p].cpu().numpy().T)
        rc, xo, fo, ibo, _ = oracle.dq_quasi_newton_solve(Ah, b[p].cpu().numpy(), 0.5, x0[p].cpu().numpy(), analytic=False,
                                                          opts=oracle.default_options(max_evals=500))
        assert status[p] == rc
        for k in COUNT_KEYS:
            assert ibs[p][k] == ibo[k], (p, k, ibs[p], ibo)
        assert np.array_equal(x[p].cpu().numpy(), xo), p
        assert np.array_equal(fvec[p].cpu().numpy(), fo), p


def test_host_readme_example_1_counts(oracle):
    """README.md:34-99 through the drop-in API on the GPU: 11 iterations, 15 function evaluations, 1 Jacobian evaluation
    (the counts the reference prints), x and f bit-identical to the CPU oracle."""
    x, f, ib = _solve_host(P.fcn1, 2, (1.0, 1.0), jdelta=20)
    assert (ib.iter_count, ib.fcn_count, ib.jacobian_count) == (11, 15, 1)
    rc, xo, fo, ibo = oracle.quasi_newton_solve(lambda a, b: P.fcn1(a, b, None), 2, [1.0, 1.0], jdelta=20)
    assert rc == 0 and _same(ib, ibo)
    assert np.array_equal(x, xo) and np.array_equal(f, fo)
    assert ("%.2e" % f[0], "%.2e" % f[1]) == ("3.23e-12", "7.05e-12")                         # README.md:94


@pytest.mark.parametrize("n,nprob,analytic,spread,jdelta", [(64, 40, True, 0.03, 5), (96, 24, False, 0.1, 5), (129, 32, True, 0.3, 2),
                                                            (200, 16, True, 1.0, 5)])
def test_quasi_newton_lockstep_batch_bitwise(ds, oracle, n, nprob, analytic, spread, jdelta):
    """quasi_newton_solver on a batch through the lock-step state machine (nlh_kernels_newton.h, broyden mode): problems
    that restart, update and back-track at different times share every launch.  Each must carry the bits, counts, flags
    and status the CPU path gives it alone."""
    A, b, xt, x0 = ds.generate(nprob, n, n, seed0=911, sigma=0.0, spread=spread, square_shift=True)
    x = x0.clone()
    fvec, ibs, status = ds.quasi_newton_solve_batch(A, b, 0.5, x, analytic=analytic, opts=ds.options(max_evals=80), jdelta=jdelta)
    xs, fs = x.cpu().numpy(), fvec.cpu().numpy()
    seen = set()
    for p in range(nprob):
        Ah = np.asfortranarray(A[p].cpu().numpy().T)
        rc, xo, fo, ibo, _ = oracle.dq_quasi_newton_solve(Ah, b[p].cpu().numpy(), 0.5, x0[p].cpu().numpy(), analytic=analytic,
                                                          opts=oracle.default_options(max_evals=80), jdelta=jdelta)
        assert status[p] == rc, (p, status[p], rc)
        for k in ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff"):
            assert ibs[p][k] == ibo[k], (p, k, ibs[p], ibo)
        assert np.array_equal(xs[p], xo, equal_nan=True), p
        assert np.array_equal(fs[p], fo, equal_nan=True), p
        seen.add((ibo["iter_count"], ibo["fcn_count"], ibo["jacobian_count"]))
    assert len(seen) > 1
