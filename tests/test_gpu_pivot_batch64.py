"""The batch instance of the 4096-row pivot kernel (k_qrx_pivot<64, false, false>: four workgroups per CU, NORM2's chain on
two waves of 32 terms per lane -- norm2_flang_block_lanes2 in nlh_common.h) against the CPU oracle, BIT FOR BIT, at the
edges of the two-wave layout: a chunk of 4096 elements is 128 runs of 32, runs 0 .. 63 on the first chain wave, 64 .. 127
on the second, and the column shortens by one element per step.

Row counts (n = 14 and 513 copies of one matrix: the pending count runs through 0 .. 9 and one flush happens -- 257
copies, the smallest batch that takes the batch form, flush with seven pending under the four-wave pass; the two
hand-over matrices below run at 257):
  4096        all 128 runs full at step 0
  4095, 4065  the last run ragged / holding one element
  2081, 2049  a run or two on the second chain wave (2049: one element, gone after step 0)
  2056        m - j goes from 2049 to 2048 during the factorisation: the second wave from one element to nothing
Data kinds name the path of the chain they exercise: random (plain adds), graded_rows (a new maximum in every run: the
general recurrence on both waves), graded_rows_down (the maximum is the first element), heavy_tail (new maxima late),
quantized (exact ties of the running sum), zero_cols and duplicates (zero reflectors; pivot ties, the lowest index
wins).  Two more matrices put the largest entry of the first pivot column exactly in run 63 and in run 64 -- either side
of the hand-over between the waves -- and between them run both branches of step 0's physical interchange."""
import numpy as np
import pytest

import qrx_cases as QC
from test_gpu_lmfactor_exact import _check, _matrix

pytestmark = pytest.mark.gpu

COPIES, N = 513, 14
ROWS = [4096, 4095, 4065, 2081, 2049, 2056]
KINDS = ["random", "graded_rows", "graded_rows_down", "heavy_tail", "quantized", "zero_cols", "duplicates"]


def _assert_batch64(m, n, copies):
    head, steps = QC.qrx_plan(copies, m, n)
    assert copies > 256 and m > 2048
    assert head["sweep"] == "lane"
    assert QC.pivot_runs(steps) == [("batch64", n)]
    assert max(s["np"] for s in steps) == (9 if copies > 512 else 7) and sum(1 for s in steps if s["flush"]) >= 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", ROWS)
def test_pivot_batch64_bitwise(ds, oracle, kind, m):
    _assert_batch64(m, N, COPIES)
    rng = np.random.default_rng(1000 * KINDS.index(kind) + m)
    a = _matrix(kind, m, N, rng)
    f = rng.standard_normal(m)
    _check(ds, oracle, a, f, copies=COPIES)


@pytest.mark.parametrize("run,col", [(63, 3), (64, 0)])
def test_pivot_batch64_maximum_beside_the_wave_handover(ds, oracle, run, col):
    """The largest entry of the first pivot column sits in run 63 (the first chain wave's last) or run 64 (the second
    wave's first); the other heavy-tail entries put new maxima late in later columns.  Column 3 as the first pivot: step 0
    interchanges physically; column 0 as the first pivot: it does not."""
    m, copies = 4096, 257
    _assert_batch64(m, N, copies)
    rng = np.random.default_rng(77 + run)
    a = _matrix("heavy_tail", m, N, rng)
    a[32 * run + 5, col] = 1e9                                   # dominates every column norm: the first pivot, its maximum in `run`
    f = rng.standard_normal(m)
    ip = oracle.lmfactor(a)[1]
    assert (ip[0] == ip.min()) == (col == 0)                     # is column 0 the first pivot?
    _check(ds, oracle, a, f, copies=copies)
