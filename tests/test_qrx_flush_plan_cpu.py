"""Which copy of the working matrix each step of the exact lmfactor reads, and which flushes write the other one
(nlh_qrx_plan's tcur / oop, host code): the copy read at step j + 1 is the copy an out-of-place flush wrote at step j, it
never moves otherwise, the in-place forms never move it, NLH_QRX_OOP=0 keeps every flush in place and changes nothing else
of a plan; and the batches of tests/test_gpu_flush_out_of_place.py flush where that test says they do."""
import pytest

import flush_cases as FC
import qrx_cases as QC
from nonlin_amd.device import qrx_plan


def shapes():
    out = set(QC.all_shapes()) | {(m, n, nprob) for nprob, m, n, _, _ in FC.CASES.values()}
    for m, n in ((4096, 256), (2048, 128)):
        out |= {(m, n, c) for c in (2048, 1024, 683, 512, 256, 129, 128, 47, 1)}
    b, c, m, n = FC.STRAGGLERS
    out |= {(m, n, b * c), (64, 64, 600), (2049, 7, 600), (5000, 1, 2000)}
    return sorted(out)


def test_copy_follows_the_out_of_place_flushes():
    for m, n, nprob in shapes():
        for nact, stages in ((0, False), (0, True), (max(1, 3 * nprob // 4), True), (1, True)):
            plans = {}
            for mode in (None, 0, 1, 2):
                with FC.oop_mode(mode):
                    plans[mode] = qrx_plan(nprob, m, n, nact, stages)
            assert plans[None] == plans[1] == plans[2]           # the default; 2 only denies the allocation (not a plan's business)
            head, steps = plans[1]
            FC.check_copies(steps)
            for s in steps:                                      # every flush of a lane form goes out of place, nothing else
                assert s["oop"] == int(s["flush"] == 1 and s["pass"] in FC.LANE)
            if head["sweep"] == "column":
                assert all(s["tcur"] == 0 for s in steps)
            head0, steps0 = plans[0]
            assert head0 == head and all(s["oop"] == 0 and s["tcur"] == 0 for s in steps0)
            strip = lambda ss: [{k: v for k, v in s.items() if k not in ("tcur", "oop")} for s in ss]
            assert strip(steps0) == strip(steps)                 # the switch moves nothing else


def test_headline_alternates_between_the_copies():
    with FC.oop_mode(None):
        head, steps = qrx_plan(2048, 4096, 256)
    flushes = [s["j"] for s in steps if s["flush"]]
    assert flushes == FC.NINES[:28] == [s["j"] for s in steps if s["oop"]]
    assert [s["tcur"] for s in steps] == [((j - 1) // 9) & 1 if j else 0 for j in range(256)]   # steps 0 .. 9: copy 0, 10 .. 18: copy 1, ...


@pytest.mark.parametrize("name", list(FC.CASES))
@pytest.mark.parametrize("stages", [False, True])
def test_gpu_test_batches_flush_where_they_say(name, stages):
    FC.check_case(name, stages)


def test_stragglers_batch_keeps_the_lane_forms_with_a_quarter_gone():
    b, c, m, n = FC.STRAGGLERS
    for nact in (b * c, (b - 1) * c):
        with FC.oop_mode(1):
            head, steps = qrx_plan(b * c, m, n, nact, True)
        assert [s["j"] for s in steps if s["oop"]] == FC.NINES[:8]


def test_a_bad_switch_value_is_ignored_with_one_line(capfd):
    with FC.oop_mode(1):
        want = qrx_plan(300, QC.PASS_FORM_M, QC.PASS_FORM_N)
    capfd.readouterr()
    for bad in ("3", "on", "", "10"):
        with FC.oop_mode(bad):
            got = qrx_plan(300, QC.PASS_FORM_M, QC.PASS_FORM_N)
        err = capfd.readouterr().err
        assert got == want and len([ln for ln in err.splitlines() if "NLH_QRX_OOP" in ln]) == 1, (bad, err)
