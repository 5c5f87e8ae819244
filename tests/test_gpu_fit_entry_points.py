"""GPU tests of the twelve one-call fits nlh_{curve,expr}_fit_batch{,_pmap,_loss}{,_h} as one pipeline (nlh_fit.hip): the
batch of tests/fit_entry_cases.py -- three problems, the middle one without a degree of freedom, so that the runs of
solvable problems start at problems 0 and 2 -- through every entry point and configuration (map, Huber with a scale per
problem, forward differences and the analytic Jacobian, bounds, every error output) against the bits the commit before the
pipeline gave (tests/golden/fit_entry_points_parent.npz, made by tests/golden/make_fit_entry_points.py); problems 0 and 2
alone against the same problems inside the batch; and the documented ladder of error returns, rung by rung, the same for
all twelve."""
import os

import numpy as np
import pytest
import torch

import fit_entry_cases as FC
import nonlin_amd as nl

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BAD_HANDLE, INVALID, UNDERDEFINED = -3, 201, 212
IDS = [FC.entry_name(*e) for e in FC.ENTRIES]


@pytest.fixture(scope="module")
def case(ds):
    expr = nl.Expr(FC.FORMULA, FC.VARS, FC.PARAMS)
    pm = nl.ParamMap(FC.N, fixed=FC.MAP_FIXED, tied=FC.MAP_TIED)
    return dict(expr=expr, pm=pm, data=FC.batch(expr), got={})


def _batch(ds, case, entry):
    """The whole batch through one entry point: computed once, shared by the tests."""
    if entry not in case["got"]:
        case["got"][entry] = FC.run_entry(ds, case["data"], case["expr"], case["pm"], *entry)
    return case["got"][entry]


@pytest.mark.parametrize("entry", FC.ENTRIES, ids=IDS)
def test_same_bits_as_the_parent(ds, case, entry):
    """Every array of every configuration equals the recorded one, NaN rows of the refused problem included."""
    golden = np.load(os.path.join(HERE, "golden", "fit_entry_points_parent.npz"))
    got = _batch(ds, case, entry)
    for k in FC.ARRAYS:
        want = golden[FC.entry_name(*entry) + "." + k]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        assert np.array_equal(got[k].view(np.uint8), want.view(np.uint8)), (k, np.argwhere(got[k] != want)[:4].tolist())
    # the batch is what the generator says it is: problem 1 refused on its degrees of freedom, with NaN and rank -1
    assert (got["status"][:, FC.REFUSED] == INVALID).all() and (got["rank"][:, FC.REFUSED] == -1).all()
    assert np.isnan(got["sigma"].view(np.float64)[:, FC.REFUSED]).all() and np.isnan(got["chi2"].view(np.float64)[:, FC.REFUSED]).all()
    assert (got["ib"][:, FC.REFUSED] == 0).all() and (got["ib"][:, [0, 2], 0] > 0).all()


@pytest.mark.parametrize("entry", FC.ENTRIES, ids=IDS)
def test_runs_against_solo_fits(ds, case, entry):
    """Problems 0 and 2, each alone in a batch of 1, give the bits they give inside the batch of 3."""
    big = _batch(ds, case, entry)
    for p in (0, 2):
        one = FC.run_entry(ds, case["data"], case["expr"], case["pm"], *entry, sel=[p])
        for k in FC.ARRAYS:
            assert np.array_equal(one[k][:, 0].view(np.uint8), np.ascontiguousarray(big[k][:, p]).view(np.uint8)), (p, k)


@pytest.mark.parametrize("entry", FC.ENTRIES, ids=IDS)
def test_error_ladder(ds, entry):
    """The check order of the header, on the inputs of test_gpu_loss.py::test_error_returns (m = 6, N = 7, a map of another
    model, m = 4 < nfree = 5, loss 4 and -1, a NULL scale, a NULL x).  Every call of a rung also carries the faults of later
    rungs whose code differs, so the code says which rung answered; a rung a form has no argument for is skipped.  Nothing
    is written to x or fvec by a refusal."""
    model, variant, host = entry
    import curve_cases as CC
    nprob, N = 2, 7
    t, y, xt, x0 = CC.curve_problems("lorentz", 2, 0, 7, nprob=nprob)     # 7 rows allocated: the rungs use m = 4 .. 7 of them
    tt = np.ascontiguousarray(np.stack([t, t]))
    e = nl.Expr("a1/(1+((t-m1)/w1)^2) + a2/(1+((t-m2)/w2)^2) + c + 0*u", "t,u", "a1,m1,w1,a2,m2,w2,c")
    pm = nl.ParamMap(7, fixed=(6,), tied={5: (2, 1.25, 0.0)})           # nfree 5
    pm4 = nl.ParamMap(4)
    mapped, robust = variant != "fit", variant == "loss"
    m = 6 if mapped else 7                                              # what the rungs vary: accepted as it is
    dev = (lambda a: a) if host else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ds.device))
    dt, dy, dx, dc = dev(t if model == "curve" else tt), dev(y), dev(x0.copy()), dev(np.full(nprob, 0.1))
    f, sg = dev(np.full((nprob, 7), 7.0)), dev(np.full((nprob, N), 7.0))
    o = ds.options()

    def fit(mm=m, p=pm, loss=1, scale=dc, x=dx, handle=True, kind=1, ex=e, npb=nprob, opts=o, tq=dt, sigma=None):
        return FC.call(ds, model, variant, host, opts, ex, npb, mm, tq, dy, None, 1, None, None, p if mapped else None, loss if robust else 0,
                       scale if robust else None, 0, x, f, sigma, None, None, None, None, None, handle=handle, kind=kind, ncomp=2, nbase=0)

    # 1. the handle, whatever else is wrong
    assert fit(handle=False, kind=7, ex=None, mm=4, loss=4, x=None) == BAD_HANDLE
    # 2. the model, nprob < 0, m < 1 -- ahead of the degrees of freedom (m = 4 < nfree) and of the kind of loss
    assert fit(kind=7, ex=None, mm=4, loss=4) == INVALID
    assert fit(npb=-1, mm=4, loss=4) == INVALID and fit(mm=0, loss=4) == INVALID
    # 3. a map of another model, ahead of the degrees of freedom
    if mapped:
        assert fit(p=pm4, mm=2, loss=4) == INVALID
    # 4. the degrees of freedom, ahead of the kind of loss and of the NULL arrays
    if mapped:
        assert fit(mm=4, loss=4, x=None) == UNDERDEFINED                # m < nfree
    assert fit(mm=6, p=None, loss=-1, x=None) == UNDERDEFINED           # m < N without a map
    # 5. the kind of loss, ahead of nprob == 0
    if robust:
        assert fit(loss=4, npb=0) == INVALID and fit(loss=-1, npb=0) == INVALID
    # 6. nprob == 0 returns 0, ahead of the NULL arrays and of the errors without a degree of freedom
    mq = 5 if mapped else 7                                             # m == the unknowns: no degree of freedom for errors
    assert fit(npb=0, x=None, opts=None, scale=None, mm=mq, sigma=sg) == 0
    # 7. NULL opts and arrays; the scale only where a loss reads it
    assert fit(opts=None) == INVALID and fit(tq=None) == INVALID and fit(x=None) == INVALID
    if robust:
        assert fit(scale=None) == INVALID
    # 8. errors asked for without a degree of freedom
    assert fit(mm=mq, sigma=sg) == INVALID
    if robust and host:                                                 # host scales are checked: not finite, not positive
        for bad in ([0.1, 0.0], [0.1, -2.0], [np.inf, 0.1], [0.1, np.nan]):
            assert fit(scale=np.array(bad)) == INVALID
    if not host:
        torch.cuda.synchronize()
    cpu = (lambda a: a) if host else (lambda a: a.cpu().numpy())
    assert (cpu(f) == 7.0).all() and np.array_equal(cpu(dx), x0) and (cpu(sg) == 7.0).all()
    # and the call the rungs were variations of is accepted; LINEAR reads no scale
    assert fit() == 0
    if robust:
        assert fit(loss=0, scale=None) == 0
