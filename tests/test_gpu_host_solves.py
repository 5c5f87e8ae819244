"""The five single solves with a host callback (nlh_lm_solve, nlh_newton_solve, nlh_quasi_newton_solve, nlh_cls_solve,
nlh_bfgs_solve) against tests/golden/host_solves_parent.json: what they returned, and how they called the user's
function, on the commit before they were put on the lock-step drivers (tests/golden/make_host_solves.py recorded it on
the GPU).  Equality on everything: the return code, the bits of x and fvec / fout, the seven fields of ib, the number of
calls of each callback, the SHA-256 over (kind, bytes of x) of every call in order, and the printed status blocks."""
import pytest

import host_solve_cases as H

pytestmark = pytest.mark.gpu

CASES = H.build_cases()
_gold = {}


def _golden():
    if not _gold:
        _gold.update(H.load())
    return _gold


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_host_solve_matches_the_recorded_parent(ds, oracle, c):
    want = _golden()["cases"][c["name"]]
    got, _ = H.run_case(c, H.DeviceBackend(ds), oracle)
    for k in ("rc", "ib", "calls", "sha256", "x", "out", "stdout"):
        assert got[k] == want[k], (c["name"], k, got[k], want[k])


def test_refusal_ladders_match_the_recorded_parent(ds, oracle):
    """NULL handle, NULL fcn, NULL options, n < 1, m < 1, n > m -- one at a time and all at once: the codes of the parent, ib
    zeroed or left alone as the parent did, nothing called and nothing written."""
    assert H.run_refusals(H.DeviceBackend(ds), oracle) == _golden()["refusals"]


def test_bfgs_batch_of_one_prints_each_status_block_once(ds, capfd):
    """nlh_bfgs_solve_batch_device with one problem and print_status: one block per iteration that goes on
    (src/nonlin_optimize.f90:730-737), so iter_count - 1 of them, numbered 1, 2, ..., when the solve ends on a convergence
    test.  (The lock-step driver printed the last block twice: the round that ended the solve came back with it again.)"""
    import re

    import batch_entry_cases as BC
    pr = BC.Problems("crosen", 1)
    b = pr.batch(slice(None))
    try:
        a = BC.arguments(ds, "bfgs", False, pr, slice(None), b, analytic=True, opts=ds.options(max_evals=500, print_status=1))
        capfd.readouterr()
        assert BC.call("bfgs", False, a) == 0
        text = capfd.readouterr().out
        out = BC.outputs(a)
    finally:
        b.close()
    ib = dict(zip(H.IB_FIELDS, (int(v) for v in out["ib"][0])))
    assert out["st"][0] == 0 and (ib["converge_on_chng"] or ib["converge_on_zero_diff"]) and ib["iter_count"] >= 3, ib
    assert [int(v) for v in re.findall(r"^Iteration: (\d+)$", text, re.M)] == list(range(1, ib["iter_count"]))
