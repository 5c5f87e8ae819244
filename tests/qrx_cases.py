"""The shapes tests/test_gpu_lmfactor_exact.py factors, and the kernel forms each is there to reach, as
nonlin_amd.device.qrx_plan reports them.  The GPU test asserts these before it compares bits; tests/test_qrx_plan_cpu.py
asserts them, and that together they reach every form, without a GPU.  A retuned threshold that moves a shape to another
form fails both until the shape (or the expectation) follows."""
from itertools import groupby

from nonlin_amd.device import qrx_plan

ADVERSARIAL = [(300, 37), (130, 129), (64, 64), (21, 4)]
BEYOND_LIMITS = [(4500, 40), (700, 300)]
CHAIN_FREE = [(40000, 6), (70001, 4)]

# (m, n, copies) -> (sweep, runs of the pivot form, pass forms).  A handful of problems: the column sweep, long columns
# (m - j > 4096) with the scaling as its own launch at step 0 and the search / gather / NORM2 / scaling split from step 1.
# 520 copies (more than 1536 (problem, column) pairs, more than 512 (problem, window) pairs): the long-column instance
# under one wave per window with up to nine pending reflectors; 257 copies of 2100 rows: the 64-term BATCH instance.
LONG_COLUMNS = {
    (9001, 24, 1): ("column", [("long_scaled", 1), ("long_split", 23)], {"column"}),
    (12290, 17, 3): ("column", [("long_scaled", 1), ("long_split", 16)], {"column"}),
    (4101, 30, 2): ("column", [("long_scaled", 1), ("long_split", 4), ("few64", 25)], {"column"}),
    (8200, 12, 40): ("column", [("long_scaled", 1), ("long_split", 11)], {"column"}),
    (2100, 33, 1): ("column", [("few64", 33)], {"column"}),
    (4096, 70, 3): ("column", [("few64", 70)], {"column"}),
    (8200, 12, 520): ("lane", [("long", 12)], {"wave"}),
    (2100, 6, 257): ("lane", [("batch64", 6)], {"four_wave"}),
}

# copies of the 520 x 70 matrix -> runs of (live 64-column windows, pass form); the window count changes only at a flush
PASS_FORM_M, PASS_FORM_N = 520, 70
PASS_FORMS = {
    1: [(0, "column")],
    20: [(0, "column")],
    40: [(2, "wide_half"), (1, "wide_half")],
    60: [(2, "wide_half"), (1, "wide_half")],
    100: [(2, "wide"), (1, "wide_half")],
    120: [(2, "wide"), (1, "wide_half")],
    200: [(2, "four_wave"), (1, "wide"), (1, "wide_half")],
    300: [(2, "wave_shared"), (1, "four_wave")],
    1100: [(2, "wave_shared"), (1, "wave")],
}


def all_shapes():
    """Every (m, n, copies) of the GPU test."""
    return ([(m, n, 1) for m, n in ADVERSARIAL + BEYOND_LIMITS + CHAIN_FREE] + list(LONG_COLUMNS)
            + [(PASS_FORM_M, PASS_FORM_N, c) for c in PASS_FORMS])


def live_windows(step, n):
    return (n + 1 - step["lo"] + 63) // 64


def pivot_runs(steps):
    return [(k, len(list(g))) for k, g in groupby(s["pivot"] for s in steps)]


def pass_runs(head, steps, n):
    """Runs of (live windows, pass form) over the steps; the column sweep has no windows (0)."""
    lane = head["sweep"] == "lane"
    return [k for k, _ in groupby((live_windows(s, n) if lane else 0, s["pass"]) for s in steps)]


def check_long_columns(m, n, copies):
    sweep, pivots, passes = LONG_COLUMNS[(m, n, copies)]
    head, steps = qrx_plan(copies, m, n)
    assert head["sweep"] == sweep
    assert pivot_runs(steps) == pivots
    assert {s["pass"] for s in steps} == passes
    if (m, n, copies) == (8200, 12, 520):
        assert max(s["np"] for s in steps) == 9


def check_column_sweep_of_long_columns(m, n):
    """One problem, every column longer than one NORM2 chunk: the split pivot step from step 1 on."""
    head, steps = qrx_plan(1, m, n)
    assert head["sweep"] == "column" and m - n >= 4096
    assert pivot_runs(steps) == [("long_scaled", 1), ("long_split", n - 1)]


def check_pass_forms(copies):
    head, steps = qrx_plan(copies, PASS_FORM_M, PASS_FORM_N)
    assert pass_runs(head, steps, PASS_FORM_N) == PASS_FORMS[copies]
