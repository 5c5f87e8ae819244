"""CPU tests of the Python path into the one-call fits: DeviceSolver.curve_fit_batch / expr_fit_batch hand the library
exactly what they handed it before the front end was folded into one fit path -- the same entry point, scalars, pointers and
host arrays for every case of tests/fit_call_cases.py, or the same refusal -- and the ctypes signature table is the one it
was.  Both goldens were recorded by tests/golden/make_fit_calls.py on the commit before that change."""
import json
import os

import pytest

import fit_call_cases as FC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CALLS = FC.load(os.path.join(GOLDEN, "fit_calls_parent.json"))         # (packed by group in the file: every case, unpacked)
with open(os.path.join(GOLDEN, "lib_symbols_parent.json")) as _f:
    SYMBOLS = json.load(_f)
GROUPS = sorted({FC.group_of(k) for k in CALLS["cases"]})


@pytest.fixture(scope="module")
def recorded():
    """Every case through the solver of this checkout, once, as JSON gives it back."""
    from nonlin_amd import device
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(device, "_chk", FC.chk_any_device)                 # host tensors stand in for the device's
        return json.loads(json.dumps(FC.record_all()))


def test_the_golden_covers_the_cases():
    keys = [c[0] for c in FC.cases()]
    assert list(CALLS["cases"]) == keys and len(set(keys)) == len(keys)
    for model in FC.MODELS:                                           # the crossing: 64 subsets x 16 switch settings
        crossing = [v for k, v in CALLS["cases"].items() if k.startswith(model) and len(k.split(" ")) == 3]
        assert len(crossing) == 1024 and sum(isinstance(v, dict) for v in crossing) == 352
    calls = [v for v in CALLS["cases"].values() if isinstance(v, dict)]
    assert {c["entry"] for c in calls} == set(FC.ENTRY_NAMES) and len(FC.ENTRY_NAMES) == 14
    assert CALLS["refusals"] == list(FC.REFUSALS)
    assert {v for v in CALLS["cases"].values() if isinstance(v, int)} == set(range(len(FC.REFUSALS)))
    assert any(c["args"][1] != "default" for c in calls)              # options of the caller's get there
    scales = [dict(zip(FC.arg_names(c["entry"]), c["args"])) for c in calls]
    assert {a["shared_scale"] for a in scales if a.get("scale")} == {0, 1}
    assert {a["cv"]["shared_k"] for a in scales if a.get("cv")} == {0, 1}


def test_default_options_unchanged(recorded):
    assert recorded["default_options"] == CALLS["default_options"]


@pytest.mark.parametrize("group", GROUPS)
def test_fit_calls_match_the_parent(recorded, group):
    keys = [k for k in CALLS["cases"] if FC.group_of(k) == group]
    assert len(keys) >= 16
    for k in keys:
        want, got = CALLS["cases"][k], recorded["cases"][k]
        if isinstance(want, int) or isinstance(got, int):
            text = lambda v: FC.REFUSALS[v] if isinstance(v, int) else "a call of " + v["entry"]
            assert got == want, (k, text(got), text(want))
            continue
        assert got["entry"] == want["entry"], k
        names = FC.arg_names(want["entry"])
        assert len(got["args"]) == len(want["args"]) == len(names), k
        for nm, g, w in zip(names, got["args"], want["args"]):
            assert g == w, (k, want["entry"], nm, g, w)
        assert got["ret"] == want["ret"], k


# entry points added since the golden was recorded, with their signatures: nothing else may differ from it
ADDED = {"nlh_expr_plan": "i i i i i i I I I LP_c_long I LP_c_long",
         "nlh_chol_natural": "i p i i p p d i p p p p p",
         "nlh_ne_signs": "i p i i i p p p p p"}


def test_signature_table_matches_the_parent():
    got = FC.symbols_snapshot()
    assert got["types"] == SYMBOLS["types"]
    assert len(SYMBOLS["symbols"]) == 206 and set(got["symbols"]) == set(SYMBOLS["symbols"]) | set(ADDED)
    assert not set(ADDED) & set(SYMBOLS["symbols"])
    for name, sig in list(SYMBOLS["symbols"].items()) + list(ADDED.items()):
        assert got["symbols"][name] == sig, name
