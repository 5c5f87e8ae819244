"""The Householder steps behind every QR of the library (launch_house_steps in nlh_square.hip; stage entry
nlh_house_steps / DeviceSolver.house_steps) at the size and column edges of each of their five kernel forms, against the
CPU restatement nlo_qr_factor_cols -- every sum in ascending row order on both sides, so the comparison is bit for bit.

Every case passes three checks: nonlin_amd.device.house_plan -- the function the launch dispatches through -- names the
form the case's section of the grid (tests/house_cases.py) says, so a moved threshold fails here instead of silently
testing another kernel; A and E equal the restatement's to the bit (NaN where it has NaN); and the strict lower triangle
of A is exactly zero."""
import numpy as np
import pytest
import torch

import house_cases as HC
from nonlin_amd.device import house_plan

pytestmark = pytest.mark.gpu


def _first_diff(got, want):
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    i = tuple(bad[0])
    return "%d entries differ, first at %s: %r against %r" % (len(bad), list(i), float(got[i]), float(want[i]))


def _assert_plan(c):
    want = {"form": c.form, "tiles": c.tiles}
    assert HC.expected_plan(c.nprob, c.rows, c.ncA, c.ncE) == want, c
    assert house_plan(c.nprob, c.rows, c.ncA, c.ncE) == want, c


def _run(ds, oracle, c):
    _assert_plan(c)
    A, E = HC.make_data(c)
    Ad, Ed = torch.from_numpy(A).to(ds.device), torch.from_numpy(E).to(ds.device)
    ds.house_steps(Ad, Ed)
    Ag, Eg = Ad.cpu().numpy(), Ed.cpu().numpy()
    for p in range(c.nprob):
        ro, eo = oracle.qr_factor_cols(A[p], E[p])
        assert np.array_equal(Ag[p], ro, equal_nan=True), ("A", p, _first_diff(Ag[p], ro))
        assert np.array_equal(Eg[p], eo, equal_nan=True), ("E", p, _first_diff(Eg[p], eo))
        assert not np.tril(Ag[p], -1).any(), ("below the diagonal", p)
    return A, E, Ag, Eg


@pytest.mark.parametrize("c", HC.GRID_CASES, ids=HC.case_id)
def test_house_steps_bitwise(ds, oracle, c):
    """Dense problems, each with data of its own, at every row and column edge of the form."""
    _run(ds, oracle, c)


@pytest.mark.parametrize("c", HC.DEGENERATE_CASES, ids=HC.case_id)
def test_house_steps_degenerate_bitwise(ds, oracle, c):
    """H = I steps where the fused form's bookkeeping changes (first step, last step, two in a row, either side of a
    column-group edge), with and without a zero diagonal, and where only the SQUARES below the diagonal are zero (entries of
    size 1e-170: skipped all the same, and set to exact zeros in every form); A = 0; a NaN -- in the problems of even index, dense problems
    beside them in the same launch (house_cases.make_data)."""
    A, E, Ag, Eg = _run(ds, oracle, c)
    if c.pattern == "allzero":
        for p in range(0, c.nprob, 2):
            assert not Ag[p].any() and np.array_equal(Eg[p], E[p]), p
    elif c.pattern == "nan":
        assert np.isnan(Ag[0]).any() and (c.nprob < 2 or not np.isnan(Ag[1]).any())
    elif c.pattern.startswith("zero-"):
        assert not Ag[0][:, HC.pattern_steps(c)].any()           # a zero column stays zero, its diagonal included
    elif c.pattern.startswith("tiny-"):
        for j in HC.pattern_steps(c):                             # skipped: the diagonal stays tiny, no -(norm) replaces it
            assert 0.0 < abs(Ag[0][j, j]) < 1e-160, j


@pytest.mark.parametrize("n,form", [(767, "fused4"), (768, "fused16")])
def test_qr_factor_full_either_side_of_the_column_switch(ds, oracle, n, form):
    """The square factorisation of one problem, Q formed (nc = 2 n): n = 767 is the last size on fused<4> (384 workgroups),
    n = 768 the first on fused<16> with two tiles; both against nlo_qr_factor_full."""
    assert house_plan(1, n, n, n) == {"form": form, "tiles": 2} == HC.expected_plan(1, n, n, n)
    M = np.random.default_rng(n).standard_normal((n, n))
    B = torch.from_numpy(np.ascontiguousarray(M.T)).to(ds.device)[None]
    Q, Rt = ds.qr_factor_full(B)
    qo, ro = oracle.qr_factor_full(M)
    assert np.array_equal(Rt[0].cpu().numpy(), ro)
    assert np.array_equal(Q[0].cpu().numpy().T, qo)


def test_house_steps_refusals_touch_nothing(ds):
    """rows < 1, ncA < 1, ncE < 0, ncA > rows, nprob < 1: NLH_INVALID_INPUT_ERROR (201) before anything is written."""
    A = torch.full((2, 8, 3), 7.0, dtype=torch.float64, device=ds.device)
    E = torch.full((2, 8, 2), 5.0, dtype=torch.float64, device=ds.device)
    for nprob, rows, ncA, ncE in ((0, 8, 3, 2), (2, 0, 3, 2), (2, 8, 0, 2), (2, 8, 3, -1), (2, 2, 3, 2)):
        rc = ds.lib.nlh_house_steps(ds.h.ptr, nprob, rows, ncA, ncE, A.data_ptr(), E.data_ptr())
        assert rc == 201, (nprob, rows, ncA, ncE, rc)
    assert ds.lib.nlh_house_steps(ds.h.ptr, 65536, 8, 3, 2, A.data_ptr(), E.data_ptr()) == 202
    torch.cuda.synchronize()
    assert bool((A == 7.0).all()) and bool((E == 5.0).all())
    with pytest.raises(ValueError):
        ds.house_steps(torch.zeros((1, 2, 3), dtype=torch.float64, device=ds.device),
                       torch.zeros((1, 2, 1), dtype=torch.float64, device=ds.device))
