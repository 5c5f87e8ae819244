"""GPU tests of the shell every solver entry point that takes a user's launcher wraps around its lock-step driver
(tests/batch_entry_cases.py lists them: LM, the bounded solver, the covariance chain, Newton, quasi-Newton, BFGS,
Nelder-Mead, Brent and Newton-1var, each as a device-pointer form and a host-array twin): the slices of a batch larger than
NLH_MAX_LOCKSTEP, the staging of the host arrays, the order of the argument checks and the silence of a batch.  What these
tests hold is what the entry points did before the shell was shared."""
import ctypes as C

import numpy as np
import pytest

import batch_entry_cases as BC
import user_models as UM

pytestmark = pytest.mark.gpu

# (entry, analytic): every entry point with forward differences, and with the user's Jacobian / gradient / derivative
# launcher where the family has one
SOLVERS = [("lm", False), ("cls", False), ("covar", False), ("newton", True), ("newton", False), ("qn", True), ("qn", False),
           ("bfgs", True), ("bfgs", False), ("nm", False), ("brent", False), ("n1v", True), ("n1v", False)]
NO_ORACLE = ("nm", "brent", "n1v")
_problems, _solved = {}, {}


def _whole_batch(ds, entry, analytic, host):
    """All 65,541 problems through one form of an entry point: solved once, shared by the tests, never modified."""
    key = entry, analytic, host
    if key not in _solved:
        _solved[key] = BC.solve(ds, entry, host, _family(entry), analytic=analytic)
    return _solved[key]


def _family(entry):
    fam = BC.ENTRIES[entry][0]
    if fam not in _problems:
        _problems[fam] = BC.Problems(fam, BC.NP)
    return _problems[fam]


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint8)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("entry,analytic", SOLVERS, ids=[e + ("_jac" if a else "") for e, a in SOLVERS])
def test_across_the_slice_boundary(ds, oracle, entry, analytic, host):
    """65,541 problems of the family's smallest shape in one call: two slices of the lock-step driver (65,535 and 6).
    Problems 0, 1, 65534, 65535, 65536 and the last give, bit for bit in every output (x, fvec / fout, every field of ib,
    status; cov, sigma, rank, chi2 of the covariance), what the same problem gives alone in a batch of one through the same
    entry point, and what the CPU oracle gives driving the family's host twin.  The per-problem data of the problems around
    the boundary differ, so a slice that starts at the wrong problem cannot pass.

    Nelder-Mead, Brent and Newton-1var slice at 2^30 / (n + 1) and 2^28 problems, which no batch of a test reaches: for
    them this checks that a problem's bits do not depend on the batch around it, and the staging of the host twin, only.
    Nelder-Mead runs on simplexes built from x: a caller's simplex array (use_simplex = 1), whose per-slice offset would
    likewise need a second slice to show, is left out here (tests/test_gpu_nelder_mead.py has it in one slice)."""
    pr = _family(entry)
    for v in pr.data + ((pr.lim,) if pr.family == "cubic" else (pr.x0,)):
        rows = [_bits(v[p]).tobytes() for p in (65534, 65535, 65536)]
        assert len(set(rows)) == 3, "problems around the boundary must differ"
    got = _whole_batch(ds, entry, analytic, host)
    for p in BC.SAMPLE:
        one = BC.solve(ds, entry, host, pr, sel=[p], analytic=analytic)
        assert one.keys() == got.keys()
        for k in got:
            assert np.array_equal(_bits(one[k][0]), _bits(got[k][p])), (p, k, one[k][0], got[k][p])
        if entry not in NO_ORACLE:
            want = BC.oracle_solve(oracle, entry, pr, p, analytic)
            for k, w in want.items():
                assert np.array_equal(got[k][p], w, equal_nan=True), (p, k, got[k][p], w)


@pytest.mark.parametrize("entry,analytic", SOLVERS, ids=[e + ("_jac" if a else "") for e, a in SOLVERS])
def test_both_forms_agree(ds, entry, analytic):
    """The device-pointer form and the host-array twin of an entry point: the same bits in every output of all 65,541 problems."""
    dev, host = _whole_batch(ds, entry, analytic, False), _whole_batch(ds, entry, analytic, True)
    assert dev.keys() == host.keys()
    for k in dev:
        assert np.array_equal(_bits(dev[k]), _bits(host[k])), k


@pytest.mark.parametrize("entry,host", sorted(BC.LADDERS), ids=[e + ("_h" if h else "") for e, h in sorted(BC.LADDERS)])
def test_check_ladder(ds, entry, host):
    """The rungs of BC.LADDERS in order, on a batch of two.  Every rung is called twice: carrying the faults of the later
    rungs whose code differs, so that the code says which rung answered; and with its own fault alone, where ib (filled with
    sevens) is zeroed or untouched as the table says.  A refusal writes nothing to x, fvec / fout or the covariance's outputs,
    and the call the rungs were variations of is accepted."""
    import torch
    pr = BC.Problems(BC.ENTRIES[entry][0], 2)
    b = pr.batch(slice(None))
    try:
        row = BC.LADDERS[entry, host]
        assert "P0" in [r[0] for r in row]
        for i, (label, code, zeroed, *_) in enumerate(row):
            for carry in (True, False):
                a = BC.arguments(ds, entry, host, pr, slice(None), b)
                before = {k: v.copy() for k, v in BC.outputs(a).items()}
                assert BC.call(entry, host, BC.rung_arguments(a, row, i, carry)) == code, (label, carry)
                torch.cuda.synchronize()
                for k, v in BC.outputs(a).items():
                    if k == "ib" and not carry:
                        assert (v == (0 if zeroed else 7)).all(), (label, v)
                    elif k != "ib":
                        assert np.array_equal(_bits(v), _bits(before[k])), (label, carry, k)
        a = BC.arguments(ds, entry, host, pr, slice(None), b)
        assert BC.call(entry, host, a) == 0
        out = BC.outputs(a)
        assert not any((out[k] == 7).all() for k in out if k != "x")
    finally:
        b.close()


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_a_batch_stays_silent(ds, capfd, host):
    """print_status = 1: a batch of two prints nothing; a batch of one prints the status blocks of the single solve -- what
    nlh_lm_solve prints when it drives the family's host twin through the same iterations."""
    t, y, _, x0 = UM.lorentz_problems(2, 16, 1, seed=3)
    pr = BC.Problems("lorentz", 2)
    pr.m, pr.data, pr.x0 = 16, (t, y), x0
    o = ds.options(print_status=1)
    capfd.readouterr()
    texts = []
    for sel in (slice(None), [1]):
        b = pr.batch(sel)
        a = BC.arguments(ds, "lm", host, pr, sel, b, opts=o)
        assert BC.call("lm", host, a) == 0
        b.close()
        texts.append((capfd.readouterr().out, BC.outputs(a)))
    assert texts[0][0] == ""
    printed, one = texts[1]
    hc = UM.LorentzHost(16, t[1].ctypes.data_as(BC.dp), y[1].ctypes.data_as(BC.dp), 0)
    x, f, ib = x0[1].copy(), np.zeros(16), np.zeros(BC.IB, dtype=np.int32)
    rc = BC._function("nlh_lm_solve", "h o m n fcn jac ctx x f ib")(ds.h.ptr, C.addressof(o), 16, 3, C.cast(UM.lib().lorentz_host_fcn, C.c_void_p),
                                                                  None, C.addressof(hc), x.ctypes.data, f.ctypes.data, ib.ctypes.data)
    assert rc == one["st"][0] == 0 and np.array_equal(ib, one["ib"][0]) and np.array_equal(x, one["x"][0])
    assert printed == capfd.readouterr().out
    assert printed.count(" \nIteration: ") > 1 and ib[0] > 1
