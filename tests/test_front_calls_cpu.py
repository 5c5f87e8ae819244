"""CPU tests of the composed one-call paths: curve_fit_batch / expr_fit_batch with starts= or bins=, curve_boot_batch /
expr_boot_batch and every refusal of theirs and of the plain front hand the library exactly the sequence of calls they handed
it before they were put on one model binding and one launcher stack -- the same entry points in the same order, the same
scalars, host arrays and pointees, the same shapes coming back, the same record on the Starts object, the same refusal where
several apply.  The golden was recorded by tests/golden/make_front_calls.py on the commit before that change."""
import os

import pytest

import front_call_cases as FR

GOLDEN = FR.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_calls_parent.json"))
GROUPS = sorted({FR.group_of(k) for k in GOLDEN})


@pytest.fixture(scope="module")
def recorded():
    """Every case through the solver of this checkout, once."""
    return FR.record_all()


def test_the_golden_covers_the_cases():
    keys = [c[0] for c in FR.cases()]
    assert list(GOLDEN) == keys and len(set(keys)) == len(keys)
    calls = [c for v in GOLDEN.values() for c in v["trace"]]
    assert {c["entry"] for c in calls} == set(FR.REACHABLE)           # every entry point the three paths can reach
    refused = {k: v["raises"] for k, v in GOLDEN.items() if "raises" in v}
    listed = {k for k in GOLDEN if k.split(" ")[2] in FR.REFUSED[k.split(" ")[0]]}
    assert set(refused) == listed | {"fit expr " + c for c in FR.GUESS_CASES}
    for k, text in refused.items():                                   # a formula has no guess: x0=None without starts fails as it always did
        no_guess = k.startswith("fit expr x0none") and "stat+loss" not in k
        assert text == "AttributeError" if no_guess else text.startswith("ValueError: "), k
    for c in FR.GUESS_CASES:                                          # a curve guesses
        assert GOLDEN["fit curve " + c]["trace"][0]["entry"] == "nlh_curve_guess_batch"
    for model in FR.MODELS:
        mine = {k: v for k, v in GOLDEN.items() if k.split(" ")[1] == model and k not in refused}
        count = lambda lead: sum(k.split(" ")[2].split("+")[0] == lead for k in mine)
        assert count("starts") == len(FR.STARTS_CASES) and count("bins") == len(FR.BINS_CASES)
        assert sum(k.startswith("boot") for k in mine) == 2 * len(FR.BOOT_CASES + FR.BOOT_T[model])
        # a chunked bootstrap makes its three chunks, an unchunked one its one
        assert sum(c["entry"] == "nlh_boot_resample_batch" for c in mine["boot %s residual+reps2" % model]["trace"]) == 3
        assert sum(c["entry"] == "nlh_boot_resample_batch" for c in mine["boot %s residual" % model]["trace"]) == 1
        # a start per kept candidate, and the record on the Starts object
        assert sum("_fit_batch" in c["entry"] for c in mine["fit %s starts" % model]["trace"]) == FR.KEEP
        assert set(mine["fit %s starts" % model]["starts"]) == {"which", "index", "cost"}
    # where two refusals apply the golden says which one wins
    assert refused["fit curve starts+x0given+pmap"].startswith("ValueError: starts excludes x0")
    assert refused["fit expr starts4+group"].startswith("ValueError: starts excludes pmap and group")
    assert refused["fit curve bins+pmap+starts"].startswith("ValueError: bins excludes pmap")
    assert refused["fit expr bins+x0none+tgiven"].startswith("ValueError: bins excludes x0=None")
    assert refused["boot curve residual+stat+group"].startswith("ValueError: a bootstrap excludes stat and group")


@pytest.mark.parametrize("group", GROUPS)
def test_front_calls_match_the_parent(recorded, group):
    keys = [k for k in GOLDEN if FR.group_of(k) == group]
    assert keys
    for k in keys:
        want, got = GOLDEN[k], recorded[k]
        assert got.get("raises") == want.get("raises"), k
        assert [c["entry"] for c in got["trace"]] == [c["entry"] for c in want["trace"]], k
        for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
            assert len(g["args"]) == len(w["args"]), (k, i, w["entry"])
            for j, (ga, wa) in enumerate(zip(g["args"], w["args"])):
                assert ga == wa, (k, "call %d" % i, w["entry"], "argument %d" % j, ga, wa)
        assert got.get("ret") == want.get("ret"), k
        assert got.get("starts") == want.get("starts"), k
