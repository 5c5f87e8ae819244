"""The batches tests/test_gpu_flush_out_of_place.py runs, and what the launch plan (nonlin_amd.device.qrx_plan) says of each:
which steps flush, which of those write the other copy of the working matrix, and through which pass forms.
tests/test_qrx_flush_plan_cpu.py asserts the same without a GPU."""
import contextlib
import os

from nonlin_amd.device import qrx_plan

LANE = ("wave", "wave_shared")          # the forms whose flush can write the other copy (k_qrx_pass)

# name -> (problems, m, n, the steps whose flush is out of place, the pass forms of the plan or None)
# QRX_C = 10: a lane-form launch flushes with nine updates pending, i.e. at steps 9, 18, 27, ...; a batch takes the lane
# forms while (problems x live 64-column windows) > 512; the live columns are slots lo .. n (lo = 1 at the start), so there
# are ceil((n + 1 - lo) / 64) windows and their count moves only at a flush.
NINES = [9 * k for k in range(1, 30)]
CASES = {
    # one window, two flushes; 72 rows: both flushes see only guarded tiles (row-wise stores)
    "one_window": (520, 72, 24, [9, 18], {"wave"}),
    # rows not a multiple of 8, j & 7 != 0 at both flushes: the first and the last tile are guarded and both store
    "ragged_rows": (520, 67, 24, [9, 18], {"wave"}),
    # three windows as the waves of one workgroup at the first flush (whole tiles: 1 KB stores); that flush empties the third
    # window, 360 pairs are left and the rest of the factorisation runs the in-place forms ON COPY 1
    "three_windows": (180, 136, 130, [9], {"wave_shared", "four_wave", "wide", "wide_half"}),
    # the same with 270 problems: the lane forms stay until one window is left (step 72, a flush with j & 7 == 0: no guarded
    # first tile), eight out-of-place flushes, two windows shared by a workgroup of which the second empties at step 63 / 72
    "three_windows_long": (270, 136, 130, NINES[:8], {"wave_shared", "four_wave"}),
    # n + 1 = 192 and 193 (a row block without padding column / with 63): with 140 problems both have three windows at the
    # start, 420 pairs: never a lane form, every flush in place on copy 0 ...
    "n1_mod64_0": (140, 200, 191, [], {"four_wave", "wide", "wide_half"}),
    "n1_mod64_1": (140, 200, 192, [], {"four_wave", "wide", "wide_half"}),
    # ... so the same shapes with 180 problems (540 pairs while three windows are live) ...
    "n1_mod64_0_lane": (180, 200, 191, NINES[:7], None),
    "n1_mod64_1_lane": (180, 200, 192, NINES[:8], None),
    # ... and n = 193 with 140: FOUR windows (the most a workgroup shares), the first with one live column
    "four_windows": (140, 200, 193, [9], None),
}
# (4 x 90) problems of 136 x 130 in the LM solve: with one base problem finished 270 are left (810 pairs, 540 with two windows)
STRAGGLERS = (4, 90, 136, 130)


@contextlib.contextmanager
def oop_mode(mode):
    """NLH_QRX_OOP for the calls inside (the library reads it per call); None: unset."""
    old = os.environ.pop("NLH_QRX_OOP", None)
    if mode is not None:
        os.environ["NLH_QRX_OOP"] = str(mode)
    try:
        yield
    finally:
        os.environ.pop("NLH_QRX_OOP", None)
        if old is not None:
            os.environ["NLH_QRX_OOP"] = old


def check_copies(steps):
    """The copy read at step j + 1 is the copy an out-of-place flush wrote at step j; it never moves otherwise; only flushes
    of the lane forms move it."""
    assert steps[0]["tcur"] == 0                                  # where the Jacobian is written
    for s, nxt in zip(steps, steps[1:]):
        assert nxt["tcur"] == s["tcur"] ^ s["oop"]
    for s in steps:
        assert s["oop"] in (0, 1) and s["tcur"] in (0, 1)
        if s["oop"]:
            assert s["flush"] == 1 and s["pass"] in LANE
        if s["pass"] not in LANE:
            assert s["oop"] == 0


def check_case(name, have_stages=False):
    nprob, m, n, oop_at, forms = CASES[name]
    with oop_mode(1):
        head, steps = qrx_plan(nprob, m, n, nprob if have_stages else 0, have_stages)
    assert head["sweep"] == "lane"
    check_copies(steps)
    assert [s["j"] for s in steps if s["oop"]] == oop_at
    assert all(s["np"] == 9 for s in steps if s["oop"])
    if forms is not None:
        assert {s["pass"] for s in steps} == forms
    return head, steps
