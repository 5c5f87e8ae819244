"""The kernel form and K-split count of the Gram family (nlh_gram_plan / nonlin_amd.device.gram_plan: the function
launch_gram itself dispatches through) for every shape tests/test_gpu_gram.py runs, and the two switches.  Host code:
needs no GPU."""
import pytest

import gram_cases as GC
from nonlin_amd.device import gram_plan


def _assert_plan(form, m, n):
    assert gram_plan(m, n) == GC.expected_plan(form, m), (form, m, n)


def test_plan_names_the_form_of_every_grid_shape():
    """The shape-to-form table and the switches, without a launch: NLH_GRAM_TRI=0 / NLH_GRAM512=0 send their shapes to the
    block kernel (and only theirs); unset or any other value is the default."""
    with GC.env(NLH_GRAM_TRI=None, NLH_GRAM512=None):
        for form, n, m in GC.GRID_CASES + GC.THIN_CASES:
            _assert_plan(form, m, n)
        assert [gram_plan(1024, n)["form"] for n in (96, 97, 128, 129, 224, 225, 256, 257, 512, 513)] == \
            ["block", "tri8", "tri8", "block", "block", "tri16", "tri16", "512", "512", "block"]
        with GC.env(NLH_GRAM_TRI="1"):
            assert gram_plan(1024, 113) == {"form": "tri8", "nsplit": 1, "direct": True}
        with GC.env(NLH_GRAM_TRI="0"):
            for form, n, m in GC.GRID_CASES:
                _assert_plan("block" if form in ("tri8", "tri16") else form, m, n)
        with GC.env(NLH_GRAM512="0"):
            for form, n, m in GC.GRID_CASES:
                _assert_plan("block" if form == "512" else form, m, n)
    with pytest.raises(ValueError):
        gram_plan(0, 4)
    with pytest.raises(ValueError):
        gram_plan(4, 0)
