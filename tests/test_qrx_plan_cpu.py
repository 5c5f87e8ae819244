"""The launch plan of the exact lmfactor (nlh_qrx_plan / nonlin_amd.device.qrx_plan: the stepper the factorisation itself
walks, host code that needs no GPU): its invariants over a sweep of shapes, the forms the shapes of
tests/test_gpu_lmfactor_exact.py are there to reach, that those shapes reach every form there is, and the range checks
of the NLH_QRX_* environment."""
import json
import os
import re
import subprocess
import sys

import pytest

import qrx_cases as QC
from nonlin_amd import device as D
from nonlin_amd.device import qrx_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QRX_C, RPW_MAXNP = 10, 4                   # reflector slots per bank; pending reflectors the wide form keeps (nlh_qrx.hip)
CAN_FLUSH = {1, 3, RPW_MAXNP, 7, QRX_C - 1}   # np with a flushing pass instance
WIDE = ("wide", "wide_half")
LDS_CU = 160 * 1024                        # LDS of a gfx950 compute unit


def check_invariants(nprob, m, n, head, steps):
    assert len(steps) == n and [s["j"] for s in steps] == list(range(n))
    assert head["sweep"] in D.QRX_SWEEPS and head["init"] in D.QRX_INITS
    assert head["ny"] == (head["nact"] if head["use_list"] else nprob) and 1 <= head["nact"] <= nprob
    for k, s in enumerate(steps):
        assert s["pivot"] in D.QRX_PIVOT_FORMS and s["pass"] in D.QRX_PASS_FORMS      # exactly one form each
        assert s["flush"] in (0, 1)
        # what the pass dispatch has instances for
        if head["sweep"] == "lane":
            assert s["np"] in CAN_FLUSH if s["flush"] else s["np"] <= QRX_C - 2
        if s["pass"] in WIDE:
            assert s["np"] <= RPW_MAXNP
        if s["pass"] == "four_wave":
            assert s["np"] < 8
        # dynamic LDS within what qrx_init_device allows the kernel (64 KB where it sets no attribute)
        assert 0 <= s["lds"] <= s["lds_max"] <= LDS_CU
        assert s["lds_max"] >= 65536 and (s["lds_max"] == 65536 or s["pass"] in WIDE + ("column",))
        nxt = steps[k + 1] if k + 1 < n else None
        if nxt:
            assert nxt["cur"] == s["cur"] ^ s["flush"]                               # the bank switches exactly on flushes
        if head["sweep"] == "column":
            assert s["pass"] == "column" and s["np"] == s["flush"] == s["pf"] == (1 if k else 0)
            assert s["gwin"] == n - k
            assert s["pivot"] in ("few32", "few64", "long_scaled", "long_split")
            continue
        assert s["pass"] != "column" and s["pivot"] not in ("long_scaled", "long_split")
        assert s["pf"] == s["flush"] | (2 if k and steps[k - 1]["flush"] else 0)
        live, half = QC.live_windows(s, n), (n + 1 - s["lo"] + 31) // 32
        assert s["gwin"] == (half if s["pass"] == "wide_half" else live)
        if s["pass"] == "wave_shared":
            assert 2 <= live <= 4                                                     # 64 threads per window, 256 at most
        if nxt:
            assert (nxt["np"], nxt["lo"]) == ((1, k + 1) if s["flush"] else (s["np"] + 1, s["lo"]))
    if head["sweep"] == "lane":
        assert (steps[0]["np"], steps[0]["lo"], steps[0]["cur"]) == (0, 1, 0)


def sweep_of_shapes():
    shapes = set(QC.all_shapes())
    for m, n in ((4096, 256), (2048, 128)):                     # BASELINE configs 2 and 4, full and per-rank batches
        shapes |= {(m, n, c) for c in (2048, 1024, 512, 256, 128, 47, 1)}
    shapes |= {(5000, 1, 3), (5000, 1, 2000), (300000, 3, 2), (300000, 3, 600), (2049, 7, 256), (2049, 7, 257), (64, 64, 24), (64, 64, 25)}
    return sorted(shapes)


def test_plan_invariants_over_shapes():
    for m, n, nprob in sweep_of_shapes():
        for nact, stages in ((0, False), (0, True), (1, True), (1, False), (max(1, nprob // 3), True), (max(1, nprob - 1), False)):
            head, steps = qrx_plan(nprob, m, n, nact, stages)
            check_invariants(nprob, m, n, head, steps)
            assert head["nact"] == (nact or nprob)
            assert head["use_list"] == int(stages and head["nact"] < nprob and head["init"] == "split")
    with pytest.raises(ValueError):
        qrx_plan(1, 3, 4)                                       # m < n


def test_plan_follows_the_active_count():
    """nact, not the batch, picks the forms: three stragglers of 2048 problems take the column sweep over a problem list."""
    head, steps = qrx_plan(2048, 4096, 256, 3, True)
    assert (head["sweep"], head["use_list"], head["ny"]) == ("column", 1, 3)
    assert qrx_plan(2048, 4096, 256, 3, False)[0]["use_list"] == 0           # no stages to compact by
    head, steps = qrx_plan(2048, 4096, 256, 47, True)
    assert (head["sweep"], head["init"], head["use_list"]) == ("lane", "split", 1)
    assert {s["pivot"] for s in steps} == {"few64"} and {s["pass"] for s in steps} <= set(WIDE)
    head, steps = qrx_plan(2048, 4096, 256)
    assert (head["sweep"], head["init"], head["use_list"], head["ny"]) == ("lane", "fused", 0, 2048)
    assert {s["pivot"] for s in steps} == {"batch64"} and {s["pass"] for s in steps} == {"wave_shared", "wave"}


@pytest.mark.parametrize("copies", list(QC.PASS_FORMS))
def test_gpu_test_batches_reach_their_pass_forms(copies):
    QC.check_pass_forms(copies)


def test_gpu_test_long_column_shapes_reach_their_pivot_forms():
    for m, n, copies in QC.LONG_COLUMNS:
        QC.check_long_columns(m, n, copies)
    for m, n in QC.CHAIN_FREE:
        QC.check_column_sweep_of_long_columns(m, n)


def test_gpu_test_shapes_reach_every_form():
    sweeps, inits, pivots, passes = set(), set(), set(), set()
    for m, n, copies in QC.all_shapes():
        head, steps = qrx_plan(copies, m, n)
        sweeps.add(head["sweep"]); inits.add(head["init"])
        pivots |= {s["pivot"] for s in steps}; passes |= {s["pass"] for s in steps}
    assert sweeps == set(D.QRX_SWEEPS) and inits == set(D.QRX_INITS)
    assert pivots == set(D.QRX_PIVOT_FORMS) and passes == set(D.QRX_PASS_FORMS)


def test_form_names_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "nonlin_hip.h")).read()
    for prefix, names in (("SWEEP", D.QRX_SWEEPS), ("INIT", D.QRX_INITS), ("PIVOT", D.QRX_PIVOT_FORMS), ("PASS", D.QRX_PASS_FORMS)):
        found = {name.lower(): int(v) for name, v in re.findall(r"\bNLH_QRX_%s_([A-Z0-9_]+) = (\d+)" % prefix, hdr)}
        assert found == {name: k for k, name in enumerate(names)}


def _plan_under(env, *args):
    """qrx_plan in a fresh process (the knobs are read once per process) -> (head, steps, stderr)."""
    code = "import json, sys; from nonlin_amd.device import qrx_plan; print(json.dumps(qrx_plan(*%r)))" % (args,)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("NLH_QRX_")}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(clean, PYTHONPATH=ROOT, **env), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    head, steps = json.loads(r.stdout.strip().splitlines()[-1])
    return head, steps, r.stderr


def test_knob_values_are_range_checked():
    shape = (300, QC.PASS_FORM_M, QC.PASS_FORM_N)
    head0, steps0, err = _plan_under({}, *shape)
    assert "NLH_QRX" not in err
    for bad in ({"NLH_QRX_PERIOD": "11"}, {"NLH_QRX_PERIOD": "0"}, {"NLH_QRX_PERIOD": "x"}, {"NLH_QRX_RP": "-5"}, {"NLH_QRX_FEW": "12q"}):
        head, steps, err = _plan_under(bad, *shape)
        (name,) = bad
        assert (head, steps) == (head0, steps0), bad                  # the default plan ...
        assert len([ln for ln in err.splitlines() if name in ln]) == 1, err     # ... and one line that names the variable
    # a period without a flushing instance at period - 1 stays legal: the flush comes at the first np that has one
    head, steps, err = _plan_under({"NLH_QRX_PERIOD": "6"}, *shape)
    assert "NLH_QRX" not in err
    check_invariants(*shape, head, steps)
    assert {s["np"] for s in steps if s["flush"]} == {7}
    for nprob in (40, 200, 300, 1100):
        head, steps, err = _plan_under({"NLH_QRX_RP": "0"}, nprob, *shape[1:])
        check_invariants(nprob, *shape[1:], head, steps)
        assert head["sweep"] == "lane" and {s["pass"] for s in steps} <= {"wave", "wave_shared"}
    # forms beyond what they hold fall to the next one inside the plan: a wide launch that inherits more than four pending
    # reflectors is four-wave, one that inherits eight or nine is one wave per window
    head, steps, err = _plan_under({"NLH_QRX_PERIOD": "10"}, 40, *shape[1:])
    check_invariants(40, *shape[1:], head, steps)
    assert {s["pass"] for s in steps if s["np"] <= 4} == {"wide_half"}
    assert {s["pass"] for s in steps if 4 < s["np"] < 8} == {"four_wave"}
    assert {s["pass"] for s in steps if s["np"] >= 8} == {"wave_shared", "wave"}
