"""(CPU) The cases of tests/host_solve_cases.py through the CPU oracle: every case runs, and every labelled case does what
its label says -- so a case that silently stops exercising its branch fails here, without a GPU.  The recorded file
tests/golden/host_solves_parent.json must hold exactly these cases."""
import numpy as np
import pytest

import host_solve_cases as H

CASES = H.build_cases()
_runs = {}


def _run(oracle, c):
    if c["name"] not in _runs:
        oracle.bfgs_refactor_count(reset=True)
        points = []
        rec, kinds = H.run_case(c, H.OracleBackend(oracle), oracle, capture=False, points=points)
        _runs[c["name"]] = rec, kinds, oracle.bfgs_refactor_count(), points
    return _runs[c["name"]]


def _longest_ray(points):
    """Most consecutive residual calls whose points lie on one ray from the first of them: the point a search starts from
    (evaluated as the last trial of the search before), then its trials xold + alam dir with alam falling.  A run of r
    points is a search that backtracked r - 2 times."""
    xs = [x for kind, x in points if kind == "f"]
    best = 0
    for i in range(len(xs) - 1):
        d = xs[i + 1] - xs[i]
        nd = np.sqrt(d @ d)
        r = 2 if nd > 0 else 0
        for y in xs[i + 2:]:
            e = y - xs[i]
            ne = np.sqrt(e @ e)
            if not (0 < ne < nd and (d @ e) >= (1.0 - 1e-12) * nd * ne):
                break
            r, nd = r + 1, ne
        best = max(best, r)
    return best


def _longest_f_run(kinds):
    """Most residual / objective calls in a row between two Jacobian / gradient calls (analytic cases: a line search's trials)."""
    return max((len(r) for r in kinds.replace("j", " ").split()), default=0)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_does_what_its_label_says(oracle, c):
    rec, kinds, refactored, points = _run(oracle, c)
    ib = dict(zip(H.IB_FIELDS, rec["ib"]))
    x = H.unhex(rec["x"])
    assert rec["rc"] in (0, H.CONVERGENCE_ERROR), rec
    assert rec["calls"]["f"] >= 1 and (rec["calls"]["j"] >= 1) == (c["analytic"] and not (c["solver"] == "qn" and ib["iter_count"] == 0))
    assert np.isfinite(x).all()
    ngrad = ib["gradient_count"] if c["solver"] == "bfgs" else ib["jacobian_count"]
    for label in c["labels"]:
        if label == "backtracks2":                               # one search takes its first trial and two more at least
            assert c["analytic"] and c["opts"].get("use_line_search", 1) and _longest_f_run(kinds) >= 3, kinds
        elif label == "qn_backtracks":                           # (Broyden asks for few Jacobians: the trials of one search lie on one ray)
            assert rec["rc"] == 0 and c["opts"].get("use_line_search", 1) and _longest_ray(points) >= 4, _longest_ray(points)
        elif label == "cls_backtracks":                          # the projected backtracking: trial, then two halvings at least
            assert c["analytic"] and _longest_f_run(kinds) >= 3, kinds
        elif label == "max_evals":
            assert rec["rc"] == H.CONVERGENCE_ERROR and ib["fcn_count"] >= c["opts"]["max_evals"], (rec["rc"], ib)
            assert not (ib["converge_on_fcn"] or ib["converge_on_chng"] or ib["converge_on_zero_diff"])
        elif label == "at_start":
            assert rec["rc"] == 0 and ngrad <= 1 and np.array_equal(x, c["problem"](oracle).x0), (ib, x)
        elif label == "print":
            assert c["opts"]["print_status"] == 1 and ib["iter_count"] >= 2, ib
        elif label == "jdelta":
            assert c["extra"]["jdelta"] == 1 and ib["jacobian_count"] >= 3, ib
        elif label == "lower_active":
            lo = np.array(c["extra"]["lower"])
            assert rec["rc"] == 0 and (c["problem"](oracle).x0 > lo).all() and (x == lo).any() and ib["iter_count"] >= 3, (x, ib)
        elif label == "x0_outside":
            lo, hi, x0 = np.array(c["extra"]["lower"]), np.array(c["extra"]["upper"]), c["problem"](oracle).x0
            assert ((x0 < lo) | (x0 > hi)).any() and rec["rc"] == 0 and ((x > lo) & (x < hi)).all() and ib["iter_count"] >= 3, (x, ib)
        elif label == "update_branch":                           # an iteration after the first that did not refactorise
            assert ib["iter_count"] - 1 > refactored, (ib, refactored)
        elif label == "refactor_branch":
            assert refactored >= 1
        else:
            raise AssertionError("unknown label " + label)


def test_the_options_every_solver_is_run_with():
    """What the list promises per solver: with and without the user's Jacobian / gradient, with and without the line
    search, and one case of each label kind."""
    for solver, tag in (("newton", "nt"), ("qn", "qn"), ("lm", "lm"), ("cls", "cls"), ("bfgs", "bfgs")):
        mine = [c for c in CASES if c["solver"] == solver]
        assert all(c["name"].startswith(tag + "_") for c in mine)
        assert {c["analytic"] for c in mine} == {False, True}
        labels = {label for c in mine for label in c["labels"]}
        assert {"max_evals", "at_start", "print"} <= labels, (solver, labels)
        if solver in ("newton", "qn", "bfgs"):
            assert {c["opts"].get("use_line_search", 1) for c in mine} == {0, 1}
            assert labels & {"backtracks2", "qn_backtracks"}
    assert {c["opts"].get("factor_policy") for c in CASES if c["solver"] == "lm"} >= {0, 1, 2}
    assert {c["extra"]["jdelta"] for c in CASES if c["solver"] == "qn"} == {1, 5}
    cls = [c for c in CASES if c["solver"] == "cls"]
    assert any("lower" not in c["extra"] for c in cls) and {"lower_active", "x0_outside"} <= {l for c in cls for l in c["labels"]}
    assert {"update_branch", "refactor_branch"} <= {l for c in CASES for l in c["labels"]}


def test_recorded_file_holds_exactly_these_cases():
    gold = H.load()
    assert sorted(gold["cases"]) == sorted(c["name"] for c in CASES)
    for c in CASES:
        g = gold["cases"][c["name"]]
        assert set(g) == {"rc", "x", "out", "ib", "calls", "sha256", "stdout"}
        assert (g["stdout"].count("Iteration: ") >= 1) == bool(c["opts"].get("print_status")), c["name"]
    assert sorted(gold["refusals"]) == ["bfgs", "cls", "lm", "newton", "qn"]
    for solver, res in gold["refusals"].items():
        assert res["null_handle"][0] == res["all"][0] == H.BAD_HANDLE and res["null_fcn"][0] == H.UNDEFINED_FUNCTION
        assert res["null_options"][0] == res["n_zero"][0] == H.INVALID_INPUT
        assert res.get("lds_bound", [H.ARRAY_SIZE])[0] == res.get("qn_max_n", [H.ARRAY_SIZE])[0] == H.ARRAY_SIZE
        assert ("lds_bound" in res) == (solver == "lm") and ("qn_max_n" in res) == (solver in ("qn", "bfgs"))
        if solver in ("lm", "cls"):
            assert res["n_above_m"][0] == H.UNDERDEFINED
