"""The kernel form of the Householder steps (nlh_house_plan / nonlin_amd.device.house_plan: the function
launch_house_steps itself dispatches through) for every shape tests/test_gpu_house.py runs, every threshold on both of
its sides, and the refusals.  Host code: needs no GPU."""
import numpy as np
import pytest

import house_cases as HC
from nonlin_amd.device import house_plan


def test_plan_names_the_form_of_every_case():
    """The form the section of the grid says, the restated rule and the library agree for every GPU case.  The plan takes
    the shape and nothing else, so the degenerate cases -- same shapes, other data -- cannot take another form."""
    for c in HC.GRID_CASES + HC.DEGENERATE_CASES:
        want = {"form": c.form, "tiles": c.tiles}
        assert HC.expected_plan(c.nprob, c.rows, c.ncA, c.ncE) == want, c
        assert house_plan(c.nprob, c.rows, c.ncA, c.ncE) == want, c
    forms = {(c.form, c.tiles) for c in HC.GRID_CASES}
    assert forms == {("fused4", 2), ("fused16", 1), ("fused16", 2), ("dot2", 2), ("dot_lds", 0), ("dot_global", 0)}
    assert {(c.form, c.tiles) for c in HC.DEGENERATE_CASES} == forms


@pytest.mark.parametrize("nprob,ncA,ncE", [(1, 5, 1), (3, 33, 40), (1, 20, 1516), (65, 40, 24)])
def test_row_thresholds(nprob, ncA, ncE):
    """4096 / 4097, 8192 / 8193, 18000 / 18001 rows, whatever the columns and the batch."""
    low = HC.expected_plan(nprob, 4096, ncA, ncE)
    assert low["form"] in ("fused4", "fused16")
    for rows, want in ((4096, low), (4097, {"form": "dot2", "tiles": 2}), (8192, {"form": "dot2", "tiles": 2}),
                       (8193, {"form": "dot_lds", "tiles": 0}), (18000, {"form": "dot_lds", "tiles": 0}),
                       (18001, {"form": "dot_global", "tiles": 0}), (70000, {"form": "dot_global", "tiles": 0}),
                       (1048560, {"form": "dot_global", "tiles": 0})):
        assert house_plan(nprob, rows, ncA, ncE) == want, rows


@pytest.mark.parametrize("rows", [1600, 4096])
def test_column_thresholds_of_the_fused_forms(rows):
    """nc * nprob = 1535 / 1536 (four columns a workgroup or sixteen) and ceil(nc / 16) * nprob = 256 / 257 (two product
    tiles or one), each reached through the columns and through the batch."""
    f4, f16_2, f16_1 = ({"form": "fused4", "tiles": 2}, {"form": "fused16", "tiles": 2}, {"form": "fused16", "tiles": 1})
    assert house_plan(1, rows, 20, 1515) == f4 and house_plan(1, rows, 20, 1516) == f16_2
    assert house_plan(1, rows, 1535, 0) == f4 and house_plan(1, rows, 1536, 0) == f16_2
    assert house_plan(3, rows, 500, 11) == f4 and house_plan(3, rows, 500, 12) == f16_2          # 1533, 1536
    assert house_plan(2, rows, 33, 734) == f4 and house_plan(2, rows, 33, 735) == f16_2          # 1534, 1536
    assert house_plan(23, rows, 40, 26) == f4 and house_plan(24, rows, 40, 24) == f16_2          # 1518, 1536
    assert house_plan(1, rows, 96, 4000) == f16_2 and house_plan(1, rows, 96, 4001) == f16_1     # 256, 257 groups
    assert house_plan(2, rows, 33, 2015) == f16_2 and house_plan(2, rows, 33, 2016) == f16_1     # 2 x 128, 2 x 129
    assert house_plan(64, rows, 40, 24) == f16_2 and house_plan(65, rows, 40, 24) == f16_1       # 256, 260
    assert house_plan(64, rows, 40, 25) == f16_1                                                 # 64 x 5
    assert house_plan(1, rows, rows, rows)["form"] == ("fused16" if 2 * rows >= 1536 else "fused4")
    # the square factorisation of one problem switches between n = 767 and 768
    assert house_plan(1, 767, 767, 767) == f4 and house_plan(1, 768, 768, 768) == f16_2


def test_refusals():
    for args in ((0, 8, 3, 1), (-1, 8, 3, 1), (1, 0, 1, 1), (1, 8, 0, 1), (1, 8, 3, -1), (1, 8, 9, 1), (1, 1, 2, 0),
                 (65536, 8, 3, 1), (1, 1048561, 3, 1), (1, 8, 3, 1 << 20), (1, 8, 3, 2 ** 31 - 1)):
        with pytest.raises(ValueError):
            house_plan(*args)
    # ... and their near sides are plans
    assert house_plan(1, 1, 1, 0) == {"form": "fused4", "tiles": 2}
    assert house_plan(1, 8, 8, 0)["form"] == "fused4" and house_plan(1, 8, 3, 0)["form"] == "fused4"
    assert house_plan(65535, 8, 3, 1) == {"form": "fused16", "tiles": 1}
    assert house_plan(1, 8, 3, (1 << 20) - 3) == {"form": "fused16", "tiles": 1}


@pytest.mark.parametrize("c", [c for c in HC.DEGENERATE_CASES if c.pattern[:4] in ("tri-", "zero", "tiny")], ids=HC.case_id)
def test_degenerate_patterns_make_the_steps_they_name_identity(oracle, c):
    """The data of the degenerate GPU cases does what its name says: when step j of pattern_steps comes, column j -- the
    reflectors of the columns before it applied -- is exactly zero below its diagonal (and on it, for the zero patterns;
    for the tiny patterns: nowhere zero, yet the squares below its diagonal are all zero and the restatement returns exact
    zeros there and the diagonal entry as it stood), the step before the first of them is a real reflector, and problem 1 carries no pattern.  The two long forms' cases
    are checked at 300 rows: make_data builds every row count the same way."""
    c = c._replace(rows=min(c.rows, 300), nprob=min(c.nprob, 2))
    A, _ = HC.make_data(c)
    js = HC.pattern_steps(c)
    for j in js:
        col = oracle.qr_factor_cols(A[0][:, :j], A[0][:, j:j + 1])[1][:, 0] if j else A[0][:, 0]
        if c.pattern.startswith("tiny-"):
            assert col[j:].all() and not (col[j + 1:] * col[j + 1:]).any(), j
            r = oracle.qr_factor_cols(A[0][:, :j + 1], A[0][:, :0])[0]
            assert r[j, j] == col[j] and not r[j + 1:, j].any(), j
        else:
            assert not col[j + 1:].any(), j
            assert (col[j] == 0.0) == c.pattern.startswith("zero-"), j
    if js[0] > 0:
        j = js[0] - 1
        col = oracle.qr_factor_cols(A[0][:, :j], A[0][:, j:j + 1])[1][:, 0] if j else A[0][:, 0]
        assert col[j + 1:].any()
    assert np.count_nonzero(A[1]) == A[1].size
