"""The flush of the exact lmfactor's lane forms writes a second copy of the working matrix (NLH_QRX_OOP, nlh_qrx.hip): the
exact lmfactor and a full LM solve with the switch forced to in place (0) and out of place (1) must agree with each other
and with the CPU oracle BIT FOR BIT -- x, fvec, R, ipvt, every count --, on batches that reach a lane-form flush and put each
path at its edges (tests/flush_cases.py says which steps of each batch flush out of place; asserted here before the bits):
one window / rows not a multiple of 8 / a flush step inside an 8-row block (guarded tiles, row-wise stores); two to four
windows as the waves of one workgroup with whole tiles (1 KB stores); n + 1 = 0, 1 (mod 64); in-place forms that carry on on
copy 1; a batch where a quarter of the problems has left the factorisation; an interchange at every step (columns that live
left of the live range when the flush comes); the second copy denied (NLH_QRX_OOP=2: the in-place fall-back)."""
import numpy as np
import pytest
import torch

import flush_cases as FC
from nonlin_amd.device import DeviceSolver

pytestmark = pytest.mark.gpu
KEYS = ("iter_count", "fcn_count", "jacobian_count", "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")


def _graded(m, n, seed):
    """Column norms over six decades, shuffled: an interchange at most steps."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((m, n)) * 10.0 ** (-6.0 * rng.permutation(n) / max(n - 1, 1))[None, :]
    return np.asfortranarray(a), rng.standard_normal(m)


def _factor(ds, mode, a, f, copies):
    J = torch.tensor(np.ascontiguousarray(a.T)[None].repeat(copies, axis=0), device="cuda:0")
    F = torch.tensor(np.ascontiguousarray(f)[None].repeat(copies, axis=0), device="cuda:0")
    with FC.oop_mode(mode):
        return [t.cpu().numpy() for t in ds.lmfactor_exact(J, F)]     # R, ipvt, rdiag, acnorm, qtf, wa4


def _factor_both_ways(ds, oracle, a, f, copies, modes=(0, 1)):
    """lmfactor_exact on `copies` copies of a under each mode: every copy, every mode the same bits, and the oracle's."""
    import test_gpu_lmfactor_exact as T
    n = a.shape[1]
    outs = {mode: _factor(ds, mode, a, f, copies) for mode in modes}
    first = outs[modes[0]]
    for mode in modes:
        for t0, t in zip(first, outs[mode]):
            assert np.array_equal(t0, t), mode
    for t in first:
        assert (t == t[0:1]).all()
    R, ipvt, rdiag, acnorm, qtf, wa4 = [t[0] for t in first]
    ao, ip, rd, acn = oracle.lmfactor(a)
    qt, w = T._qtf_reference(ao, rd, f)
    up = np.triu_indices(n, 1)
    assert np.array_equal(ipvt, ip) and np.array_equal(rdiag, rd) and np.array_equal(acnorm, acn)
    assert np.array_equal(R.T[up], ao[:n, :n][up]) and np.array_equal(np.diag(R), rd)
    assert np.array_equal(qtf, qt) and np.array_equal(wa4, w)
    return ip


def _solve(ds, mode, A, b, x0, me):
    x = x0.clone()
    with FC.oop_mode(mode):
        # one lock-step batch: sub-batches would deal these problems into pieces too small for the lane forms
        fvec, ibs, status = ds.lm_solve_batch(A, b, 0.5, x, ds.options(max_evals=me, factor_policy=2, sub_batches=1))
    return x.cpu().numpy(), fvec.cpu().numpy(), ibs, status


def _solve_both_ways(ds, oracle, A, b, x0, base, modes=(0, 1)):
    """The LM solve of base problems, replicated, under each mode: the same bits and counts, and the oracle's for each base
    problem.  Returns the iteration counts of the base problems."""
    nprob, n, m = A.shape
    me = 40 * (n + 1)
    outs = {mode: _solve(ds, mode, A, b, x0, me) for mode in modes}
    x1, f1, ib1, st1 = outs[modes[0]]
    for mode in modes[1:]:
        x, f, ibs, st = outs[mode]
        assert np.array_equal(x, x1, equal_nan=True) and np.array_equal(f, f1, equal_nan=True), mode
        assert st == st1 and all(ibs[p][k] == ib1[p][k] for p in range(nprob) for k in KEYS), mode
    for p0 in range(base):
        assert np.array_equal(x1[p0::base], np.broadcast_to(x1[p0], x1[p0::base].shape), equal_nan=True)
        assert np.array_equal(f1[p0::base], np.broadcast_to(f1[p0], f1[p0::base].shape), equal_nan=True)
        assert all(st1[p] == st1[p0] and all(ib1[p][k] == ib1[p0][k] for k in KEYS) for p in range(p0, nprob, base))
        Ah = np.asfortranarray(A[p0].cpu().numpy().T)
        rc, xo, fo, ibo = oracle.dq_lm_solve(Ah, b[p0].cpu().numpy(), 0.5, x0[p0].cpu().numpy(),
                                             opts=oracle.default_options(max_evals=me))[:4]
        assert st1[p0] == rc and all(ib1[p0][k] == ibo[k] for k in KEYS), (p0, ib1[p0], ibo)
        assert np.array_equal(x1[p0], xo, equal_nan=True) and np.array_equal(f1[p0], fo, equal_nan=True), p0
    return [ib1[p0]["iter_count"] for p0 in range(base)]


def _replicated(ds, base, copies, m, n, seed, gens=({},)):
    parts = [ds.generate(1, m, n, seed0=seed + 17 * k, **gens[k % len(gens)]) for k in range(base)]
    A, b, x0 = (torch.cat([p[i] for p in parts]) for i in (0, 1, 3))
    return A.repeat(copies, 1, 1).contiguous(), b.repeat(copies, 1).contiguous(), x0.repeat(copies, 1).contiguous()


@pytest.mark.parametrize("name", list(FC.CASES))
def test_flush_out_of_place_bitwise(ds, oracle, name):
    nprob, m, n, oop_at, forms = FC.CASES[name]
    FC.check_case(name, False)                                  # lmfactor_exact's plan ...
    FC.check_case(name, True)                                   # ... and the LM solve's first factorisation
    a, f = _graded(m, n, 1000 + m + n)
    _factor_both_ways(ds, oracle, a, f, nprob)
    base = 2
    A, b, x0 = _replicated(ds, base, nprob // base, m, n, 4242 + n)
    _solve_both_ways(ds, oracle, A, b, x0, base)


def test_flush_out_of_place_skips_problems_that_left_the_factorisation(ds, oracle):
    """Four base problems of different difficulty, 90 copies each, one lock-step batch: the rounds after the first base
    problem has finished factor 270 (or 180) of the 360 with the lane forms, and the finished problems' matrices are neither
    read nor written -- their x, fvec and counts are the oracle's like everybody's."""
    base, copies, m, n = FC.STRAGGLERS
    gens = ({}, dict(sigma=0.0), dict(gamma=2.0, sigma=0.1, spread=5.0), dict(gamma=10.0, sigma=1.0, spread=50.0))
    A, b, x0 = _replicated(ds, base, copies, m, n, 777, gens)
    its = _solve_both_ways(ds, oracle, A, b, x0, base)
    print("iteration counts of the base problems:", its)
    assert sum(it > min(its) for it in its) >= 2, its            # at least 180 problems (540 pairs) went on without the first


def test_flush_out_of_place_with_an_interchange_at_every_step(ds, oracle):
    """Slot j's old column stays where it is and becomes slot kmax, so after nine steps with an interchange each the live
    range holds columns to the left of the slots they now are: the flush moves them to their slots' own positions in the
    OTHER copy.  (a) the smallest column first, the others in descending order: kmax = j + 1 at every step, one column
    travels through all slots; (b) columns in ascending order: kmax = n - 1 - j through the first half."""
    rng = np.random.default_rng(5)
    for nprob, m, n in ((520, 72, 24), (270, 136, 130)):
        scale = np.concatenate([[1e-4], 1.05 ** -np.arange(n - 1, dtype=float)])
        q = np.linalg.qr(rng.standard_normal((m, n)))[0]       # orthogonal columns: the down-dated norms keep the order
        f = rng.standard_normal(m)
        ip = _factor_both_ways(ds, oracle, np.asfortranarray(q * scale[None, :]), f, nprob)
        assert ip.tolist() == list(range(1, n)) + [0]
        ip = _factor_both_ways(ds, oracle, np.asfortranarray(q * (1.05 ** np.arange(n, dtype=float))[None, :]), f, nprob)
        assert ip.tolist() == list(range(n - 1, -1, -1))


def test_flush_falls_back_in_place_when_the_second_copy_is_denied(oracle):
    """A solver of its own: NLH_QRX_OOP=2 plans the out-of-place flushes but treats the allocation as denied -- no second
    copy appears and the bits are the in-place ones; 0 allocates none either; 1 allocates one of the first copy's size."""
    ds = DeviceSolver(0)
    nprob, m, n = FC.CASES["one_window"][:3]
    a, f = _graded(m, n, 31)
    A, b, x0 = _replicated(ds, 2, nprob // 2, m, n, 99)
    assert ds.qrx_second_matrix_bytes() == 0
    _factor_both_ways(ds, oracle, a, f, nprob, modes=(2, 0))
    _solve_both_ways(ds, oracle, A, b, x0, 2, modes=(2, 0))
    assert ds.qrx_second_matrix_bytes() == 0
    _factor_both_ways(ds, oracle, a, f, nprob, modes=(1, 2, None))
    ld = 64                                                         # 25 columns padded to a 64-column window
    assert ds.qrx_second_matrix_bytes() >= 8 * nprob * m * ld
    _solve_both_ways(ds, oracle, A, b, x0, 2, modes=(1, 2))
