"""The dense building blocks of bfgs%solve on the device, each against the CPU restatement, bit for bit:
R = chol(B) in every form its dispatch can take (blocked with 4, 2, 1 thread groups per column; the column form with 4
and 8 columns per thread), its non-positive-pivot exit, batches, the two triangular solves of solve_cholesky, and the
solver end to end across the size where the blocked form's LDS ends (n = 608) and through refactorisations of a dense B.

Why equality is exact: both sides form a(j,c) - sum_k r(k,j) r(k,c) with k ascending, every term a separate multiply
and subtract, then one division by r(j,j); the solves subtract in ascending (forward) / the oracle's (backward) order.
No tolerance appears anywhere in this file.

Oracle times measured on the test host (one core): chol_factor_upper 1.8 s at n = 2100, 0.25 s at n = 1100;
dq_bfgs_solve with m = n: 1.3 s (n = 608, max_evals = 4), 1.5 s (n = 640, 4), 4.1 s (n = 1024, 3) per problem."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
COUNT_KEYS = ("iter_count", "fcn_count", "gradient_count", "converge_on_chng", "converge_on_zero_diff")

# n -> the form nlh_bf_chol_form must name: G (blocked, G thread groups per column) or -NC (column form)
FORMS = {1: 4, 2: 4, 15: 4, 16: 4, 17: 4, 31: 4, 33: 4, 63: 4,          # partial panel; one panel; panel boundary
         64: 4, 65: 4, 129: 4, 255: 4, 256: 4,                           # diagonal block in waves 1..3; last size of G = 4
         257: 2, 300: 2, 512: 2,
         513: 1, 608: 1,                                                 # 608: the last size whose LDS fits
         609: -4, 624: -4, 640: -4, 1000: -4, 1024: -4,                  # beyond the LDS bound: the column form
         1025: -4, 1100: -4, 2100: -4}                                   # 2100: a third column per thread


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    """Equality of every bit (so NaN equals the same NaN and -0 differs from +0)."""
    return a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def _dev(ds, a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(ds.device)     # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _spd(n, seed=None):
    """B = M^T M + n I, M standard normal, seeded by n; exactly symmetric; read-only (shared between tests)."""
    rng = np.random.default_rng(n if seed is None else seed)
    M = rng.standard_normal((n, n))
    B = M.T @ M + n * np.eye(n)
    B = np.triu(B) + np.triu(B, 1).T
    B.setflags(write=False)
    return B


_FACTORS = {}


def _oracle_factor(oracle, n, seed=None):
    """The oracle's factor of _spd(n, seed), computed once and left unchanged."""
    key = (n, seed)
    if key not in _FACTORS:
        rc, R = oracle.chol_factor_upper(_spd(n, seed))
        assert rc == 0
        R.setflags(write=False)
        _FACTORS[key] = R
    return _FACTORS[key]


def _check_spd_factor(ds, oracle, n, form):
    assert ds.bf_chol_form(n) == form
    Rt, info = ds.bf_chol_factor(_dev(ds, _spd(n)[None]))
    assert info == [0]
    assert _same_bits(Rt[0].cpu().numpy(), _oracle_factor(oracle, n))     # zeros below the diagonal included


@pytest.mark.parametrize("n", sorted(FORMS))
def test_chol_factor_dense_spd_bitwise(ds, oracle, n):
    _check_spd_factor(ds, oracle, n, FORMS[n])


def test_form_table_is_what_the_lds_bound_gives(ds):
    """The sizes above reach the forms they are named for because of two bounds: 1024 threads (G) and NLH_LDS_MAX
    (blocked or not); the edges of both."""
    assert [ds.bf_chol_form(n) for n in (256, 257, 512, 513, 608, 609, 1024, 1025, 4096)] == [4, 2, 2, 1, 1, -4, -4, -4, -4]
    assert ds.bf_chol_form(4097) == -8 and ds.bf_chol_form(8192) == -8
    assert ds.bf_chol_form(0) == 0 and ds.bf_chol_form(8193) == 0


_NC8 = '''
import sys
sys.path.insert(0, "tests")
from nonlin_amd.device import DeviceSolver
from oracle import pyoracle as O
import test_gpu_bfgs_dense as T
ds = DeviceSolver(0)
for n in (1100, 2100):
    T._check_spd_factor(ds, O, n, -8)
print("ok")
'''


def test_chol_factor_eight_columns_per_thread_bitwise():
    """k_bf_chol_factor<8> (n > 4096 in production), forced at n = 1100 and 2100 where the oracle is affordable; a fresh
    process because the variable is read once."""
    e = dict(os.environ)
    e["NLH_QN_FORCE_NC8"] = "1"
    out = subprocess.run([sys.executable, "-c", _NC8], capture_output=True, text=True, timeout=900, env=e,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ok" in out.stdout


# ---- non-positive pivots, placed exactly -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _integer_factor(n):
    """R0 upper triangular, entries in -2 .. 2, diagonal in 1 .. 3: B = R0^T R0 is exact in doubles and its factorisation
    reproduces R0 exactly (every intermediate is an integer far below 2^53)."""
    rng = np.random.default_rng(1000 + n)
    R0 = np.triu(rng.integers(-2, 3, size=(n, n)).astype(np.float64), 1)
    R0[np.arange(n), np.arange(n)] = rng.integers(1, 4, size=n).astype(np.float64)
    B = R0.T @ R0
    assert np.array_equal(B, B.T) and np.array_equal(B, np.rint(B))
    R0.setflags(write=False); B.setflags(write=False)
    return R0, B


def _pivot_rows(n):
    """Row 0; the first, a middle and the last row of a 16-row panel; the partial last panel (when n is no multiple of
    16) and the last row; from n > 64 the same inside a panel whose diagonal block sits in wave 1 or later."""
    last = ((n - 1) // 16) * 16
    rows = {0, 16, 24, 31, last, last + (n - 1 - last) // 2, n - 1}
    if n > 80:
        w = ((n // 2) // 64) * 64 if n >= 256 else 64              # a panel that starts a later wave
        rows |= {64, 72, 79, w, w + 16 + 5, w + 47}
    return sorted(r for r in rows if r < n)


@pytest.mark.parametrize("n", [40, 200, 300, 600, 640, 1100])
def test_chol_factor_bad_pivot_bitwise(ds, oracle, n):
    """A zero, a negative and a NaN pivot at chosen rows j, one n in each form (G = 4, 4, 2, 1, column, column): info is
    j + 1 on both sides and the upper triangle has the oracle's bits -- rows above j factored, rows from j on still B.
    (Below the diagonal the device has zeros and the oracle, which stops before it clears them, has B: not compared.)"""
    R0, B0 = _integer_factor(n)
    assert ds.bf_chol_form(n) == {40: 4, 200: 4, 300: 2, 600: 1, 640: -4, 1100: -4}[n]
    rc, R = oracle.chol_factor_upper(B0)
    assert rc == 0 and _same_bits(R, R0)                                 # the construction is exact
    Rt, info = ds.bf_chol_factor(_dev(ds, B0[None]))
    assert info == [0] and _same_bits(Rt[0].cpu().numpy(), R0)
    iu = np.triu_indices(n)
    rows = _pivot_rows(n)
    assert rows[0] == 0 and (n <= 80 or max(rows) >= 64)
    for j in rows:
        for kind in ("zero", "negative", "nan"):
            B = B0.copy()
            if kind == "zero":
                B[j, j] -= R0[j, j] ** 2
            elif kind == "negative":
                B[j, j] -= 2.0 * R0[j, j] ** 2
            else:
                B[j, j] = np.nan
            rc, R = oracle.chol_factor_upper(B)
            assert rc == j + 1, (n, j, kind, rc)                         # rows 0 .. j-1 do not see the change
            Rt, info = ds.bf_chol_factor(_dev(ds, B[None]))
            assert info == [rc], (n, j, kind, info)
            got = Rt[0].cpu().numpy()
            assert _same_bits(got[iu], R[iu]), (n, j, kind)
            assert _same_bits(got[:j][np.triu_indices(j, 0, n)], R0[:j][np.triu_indices(j, 0, n)]), (n, j, kind)


@pytest.mark.parametrize("n", [100, 300])
def test_chol_factor_batch_with_indefinite_neighbours(ds, oracle, n):
    """Five problems in one launch, problems 1 and 3 indefinite at different rows: every problem is what its own call
    gives and what the oracle gives -- an early exit disturbs nobody else."""
    nprob = 5
    Bs = [_spd(n, seed=(n, p)).copy() for p in range(nprob)]
    bad = {1: n // 3, 3: n - 2}
    for p, j in bad.items():
        Bs[p][j, j] = -Bs[p][j, j]
    Rt, info = ds.bf_chol_factor(_dev(ds, np.stack(Bs)))
    iu = np.triu_indices(n)
    for p in range(nprob):
        rc, R = oracle.chol_factor_upper(Bs[p])
        assert rc == (bad[p] + 1 if p in bad else 0)
        Rt1, info1 = ds.bf_chol_factor(_dev(ds, Bs[p][None]))
        assert info[p] == info1[0] == rc, (p, info, info1, rc)
        assert torch.equal(Rt[p].view(torch.int64), Rt1[0].view(torch.int64)), p
        got = Rt[p].cpu().numpy()
        assert _same_bits(got[iu], R[iu]), p
        assert not np.tril(got, -1).any(), p


# ---- solve_cholesky -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300, 1024, 1025, 1100, 2100])
def test_solve_cholesky_bitwise(ds, oracle, n):
    """x <- R^-T x, x <- R^-1 x as the solver launches them; from n > 1024 the 1024 threads stride over the columns."""
    R = _oracle_factor(oracle, n)
    b = np.random.default_rng(7000 + n).standard_normal(n)
    x = ds.bf_solve_cholesky(_dev(ds, R[None]), _dev(ds, b[None]))
    assert _same_bits(x[0].cpu().numpy(), oracle.solve_cholesky_upper(R, b))


def test_solve_cholesky_batch_bitwise(ds, oracle):
    n, nprob = 300, 3
    Rs = [_oracle_factor(oracle, n, seed=(n, p)) for p in range(nprob)]
    b = np.random.default_rng(7300).standard_normal((nprob, n))
    x = ds.bf_solve_cholesky(_dev(ds, np.stack(Rs)), _dev(ds, b)).cpu().numpy()
    for p in range(nprob):
        assert _same_bits(x[p], oracle.solve_cholesky_upper(Rs[p], b[p])), p


# ---- the factor of a dense matrix feeds the tested rank-one update ------------------------------------------------------

@pytest.mark.parametrize("n", [300, 640])
def test_rank1_update_of_the_device_factor_bitwise(ds, oracle, n):
    Rt, info = ds.bf_chol_factor(_dev(ds, _spd(n)[None]))
    assert info == [0]
    u = np.random.default_rng(8000 + n).standard_normal(n)
    assert ds.chol_rank1(Rt[0], _dev(ds, u), downdate=False) == 0
    assert _same_bits(Rt[0].cpu().numpy(), oracle.chol_update(_oracle_factor(oracle, n), u))


# ---- end to end ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,max_evals", [(608, 4), (640, 4), (1024, 3)])
def test_dq_bfgs_lockstep_across_the_lds_bound_bitwise(ds, oracle, n, max_evals):
    """The lock-step batch sends every problem through R = chol(B) in its first iteration: the last size of the blocked
    form, and two sizes beyond it, where the launch the dispatch used to make cannot be accepted.  max_evals: the second
    iteration's step comes out of that factor (three evaluations at least); no more than the oracle can do in seconds."""
    nprob, opts = 2, dict(max_evals=max_evals, gtol=1e-8, xtol=1e-12)
    A, b, xt, x0 = ds.generate(nprob, n, n, seed0=77, spread=0.1)
    x = x0.clone()
    fout, ibs, status = ds.bfgs_solve_batch(A, b, 0.5, x, opts=ds.options(**opts))
    for p in range(nprob):
        Ah = np.asfortranarray(A[p].cpu().numpy().T)
        rc, xo, fo, ibo, _ = oracle.dq_bfgs_solve(Ah, b[p].cpu().numpy(), 0.5, x0[p].cpu().numpy(), opts=oracle.default_options(**opts))
        assert ibo["iter_count"] >= 2
        assert status[p] == rc, (p, status[p], rc, ibs[p], ibo)
        for k in COUNT_KEYS:
            assert ibs[p][k] == ibo[k], (p, k, ibs[p], ibo)
        assert _same_bits(x[p].cpu().numpy(), xo), p
        assert fout[p] == fo, p


def _chain(n):
    """A smooth objective of n variables and its gradient, elementwise arithmetic and exactly rounded sums only, so that the
    device path and the oracle, which both call it, see the same bits whatever the alignment of the x they hand in."""
    import math
    i = np.arange(n, dtype=np.float64)
    c = 1.0 + 9.0 * i / max(n - 1, 1)
    t = np.cos(i)

    def f(x, args=None):
        y = x - t
        d = x[1:] - x[:-1]
        return math.fsum(0.5 * c * (y * y) + 0.25 * ((y * y) * (y * y))) + 0.5 * math.fsum(d * d)

    def g(x, out, args=None):
        y = x - t
        d = x[1:] - x[:-1]
        out[:] = c * y + (y * y) * y
        out[:-1] -= d
        out[1:] += d
    return f, g


def test_bfgs_one_problem_path_beyond_the_lds_bound_bitwise(oracle):
    """bfgs%solve for one problem (the lock-step driver behind the host callbacks) at n = 640, to convergence on the gradient: the factorisations go through
    the same dispatch -- the first iteration's, and later ones of a dense B (the oracle counts them); a launch that was
    refused would leave the stale factor and the iterates would part from the oracle's.  Status, counts, x and f."""
    import nonlin_amd as nl
    n, gtol = 640, 1e-6
    f, g = _chain(n)
    x0 = np.sin(np.arange(n, dtype=np.float64))
    oracle.bfgs_refactor_count(reset=True)
    rco, xo, fo, ibo = oracle.bfgs_solve(lambda v: f(v), n, x0, grad=lambda v, out: g(v, out),
                                         opts=oracle.default_options(max_evals=500, gtol=gtol))
    # (conditions on the input: it converges, and a dense B is refactorised on the way)
    assert rco == 0 and ibo["iter_count"] >= 10 and oracle.bfgs_refactor_count() >= 1
    obj = nl.fcnnvar_helper()
    obj.set_fcn(f, n)
    obj.set_gradient_fcn(g)
    s = nl.bfgs()
    s.set_tolerance(gtol)
    x = x0.copy()
    ib = nl.iteration_behavior()
    fout = s.solve(obj, x, ib)                                           # (raises unless the status is 0)
    assert all(getattr(ib, k) == ibo[k] for k in COUNT_KEYS), (ib.as_dict(), ibo)
    assert _same_bits(x, xo)
    assert fout == fo


@pytest.mark.parametrize("m,n,use_ls", [(300, 37, 0), (300, 37, 1), (120, 40, 1)])
def test_dq_bfgs_refactorisations_after_the_first_iteration_bitwise(ds, oracle, m, n, use_ls):
    """The branch y . dx <= 1e-10 after iteration 1: R = chol(R^T R) of a DENSE factor inside the solver.  The oracle counts
    how often each input takes it (a condition on the input, checked on the CPU); the device solve has the oracle's bits."""
    nprob, opts = 3, dict(max_evals=200, gtol=1e-8, xtol=1e-12, use_line_search=use_ls)
    A, b, xt, x0 = ds.generate(nprob, m, n, seed0=5, spread=0.1)
    x0 = xt + (x0 - xt) * 3.0                                            # a far start
    x = x0.clone()
    fout, ibs, status = ds.bfgs_solve_batch(A, b, 0.5, x, opts=ds.options(**opts))
    for p in range(nprob):
        Ah = np.asfortranarray(A[p].cpu().numpy().T)
        oracle.bfgs_refactor_count(reset=True)
        rc, xo, fo, ibo, _ = oracle.dq_bfgs_solve(Ah, b[p].cpu().numpy(), 0.5, x0[p].cpu().numpy(), opts=oracle.default_options(**opts))
        assert oracle.bfgs_refactor_count() >= 1, p
        assert status[p] == rc, (p, status[p], rc, ibs[p], ibo)
        for k in COUNT_KEYS:
            assert ibs[p][k] == ibo[k], (p, k, ibs[p], ibo)
        assert _same_bits(x[p].cpu().numpy(), xo), p
        assert fout[p] == fo, p


# ---- the stop "matrix not positive definite" (NL_INVALID_OPERATION_ERROR = 104) -------------------------------------------
# Reached where the first step crosses negative curvature: y . dx < 0 makes temp = sqrt(y . y / y . dx) NaN, R = NaN * I,
# and R = chol(B) meets a NaN pivot in row 1.  (No dense-quadratic input of a search over 1540 solves reached it.)

def test_bfgs_not_positive_definite_stop_one_problem(oracle):
    import math
    import nonlin_amd as nl
    f = lambda x, args=None: math.fsum(np.cos(x))                         # noqa: E731  (concave around the start)

    def g(x, out, args=None):
        out[:] = -np.sin(x)
    x0 = np.array([0.1, 0.2, -0.1])
    rco, xo, fo, ibo = oracle.bfgs_solve(lambda v: f(v), 3, x0, grad=lambda v, out: g(v, out))
    assert rco == 104 and ibo["iter_count"] == 1                         # (a condition on the input)
    obj = nl.fcnnvar_helper()
    obj.set_fcn(f, 3)
    obj.set_gradient_fcn(g)
    x = x0.copy()
    ib = nl.iteration_behavior()
    with pytest.raises(nl.NonlinError) as e:
        nl.bfgs().solve(obj, x, ib)
    assert e.value.code == rco
    assert all(getattr(ib, k) == ibo[k] for k in COUNT_KEYS), (ib.as_dict(), ibo)
    assert _same_bits(x, xo)


@pytest.mark.parametrize("analytic", [True, False])
def test_bfgs_not_positive_definite_stop_in_a_lockstep_batch(ds, oracle, analytic):
    """Chained Rosenbrock (a user's device fcnnvar), three problems; the middle one starts where its first step crosses
    negative curvature and stops with 104 in iteration 1, its neighbours converge: everything as the oracle has it."""
    import ctypes as C
    import user_models as UM
    so, dp = UM.lib(), C.POINTER(C.c_double)
    n, c = 2, np.array([1.1, 1.1, 1.1])
    x0 = np.array([[-0.5, -0.4], [-1.27, 1.68], [0.3, 0.2]])
    batch = UM.BtriBatch(c)
    try:
        x = _dev(ds, x0)
        grad = ds._devfcn(batch.crosen_launch_grad) if analytic else None
        fout, ibs, st = ds.bfgs_solve_batch_device(ds._devfcn(batch.crosen_launch), batch.ctx, x, grad=grad, opts=ds.options(max_evals=500))
        for p in range(3):
            cp = float(c[p])
            f_host = lambda xx: so.crosen_host_f(cp, n, np.ascontiguousarray(xx).ctypes.data_as(dp))              # noqa: E731
            g_host = (lambda xx, gg: so.crosen_host_grad(cp, n, np.ascontiguousarray(xx).ctypes.data_as(dp), gg.ctypes.data_as(dp))) if analytic else None
            rc, xo, fo, ibo = oracle.bfgs_solve(f_host, n, x0[p], grad=g_host, opts=oracle.default_options(max_evals=500))
            assert rc == (104 if p == 1 else 0)                          # (a condition on the input)
            assert st[p] == rc, (p, st, rc)
            for k in COUNT_KEYS:
                assert ibs[p][k] == ibo[k], (p, k, ibs[p], ibo)
            assert _same_bits(x[p].cpu().numpy(), xo), p
            assert fout[p] == fo, p
    finally:
        batch.close()
