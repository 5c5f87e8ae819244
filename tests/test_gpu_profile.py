"""GPU tests of the profile-likelihood intervals: the pin pair's kernels at their size edges against the equivalent fixed map on
data replicated by hand, bit for bit; the root finder's start and step against tests/profile_restatement.py, bit for bit after
every step; the one-call profiles end to end against the restatement over the CPU oracle's solver -- bit for bit on an exp-free
formula, flags and tolerance on the Poisson decays --; chunking, a mapped fit and a fit on its bound."""
import os

import numpy as np
import pytest
import torch

import boot_pois_cases as BC
import expr_restatement as ER
import pois_cases as PO
import profile_cases as PC
import profile_restatement as PR
import starts_restatement as S
import nonlin_amd as nl
from nonlin_amd import Profile, _lib
from nonlin_amd._lib import PROFILE_SYMBOLS  # noqa: F401  (the feature: without it nothing here runs)

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _dev(ds, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ds.device)


def _record(line):
    """Print a measured figure; append it to the file NLH_PROFILE_RATE_FILE names, when it names one (profiles/profile_rate.txt)."""
    print(line)
    path = os.environ.get("NLH_PROFILE_RATE_FILE")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


class _env:
    """Environment variables for the calls inside (the library reads them at every call)."""

    def __init__(self, **want):
        self.want = want

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in self.want}
        for k, v in self.want.items():
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------------------------------
# 6. the pin kernels at their edges
# ---------------------------------------------------------------------------------------------------------------------
def _formula(N):
    """An exp-free formula of N parameters in one variable: Michaelis-Menten for 2, with an offset for 3, else a sum of terms."""
    if N == 2:
        return nl.Expr(PC.MM_FORMULA, PC.MM_VARS, PC.MM_PARAMS)
    if N == 3:
        return nl.Expr("vmax*s/(km+s)+c", ("s",), ("vmax", "km", "c"))
    terms = [f"p{i}*s" if i % 2 == 0 else f"p{i}/(s+{i}.0)" for i in range(N)]
    return nl.Expr("+".join(terms), ("s",), tuple(f"p{i}" for i in range(N)))


NPROB, NEND = 5, 15


@pytest.mark.parametrize("N", [2, 3, 32])
@pytest.mark.parametrize("m", [1, 255, 256, 257, 2049])
def test_pin_kernels_equal_the_fixed_map_on_replicated_data(ds, m, N):
    """fd_jacobian_device through the pin pair -- the inner Jacobian launcher, and forward differences of the residual launcher
    -- against pmap_launchers(ParamMap(N, fixed=(pos,))) with full = theta on data replicated by hand, selected per pos: the
    same bits, for pos constant 0, constant N - 1 and varying per end, src = w % nprob and a permutation, and with
    NLH_PIN_SCRATCH so low that a Jacobian call runs in three slices."""
    e = _formula(N)
    rng = np.random.default_rng(100 * N + m)
    t = rng.uniform(0.25, 4.0, (NPROB, m))
    y = rng.uniform(0.5, 3.0, (NPROB, m))
    dt, dy = _dev(ds, t), _dev(ds, y)
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy)
    x = rng.uniform(0.8, 1.6, (NEND, N - 1))
    theta = rng.uniform(0.8, 1.6, NEND)
    dx = _dev(ds, x)
    cases = [(np.zeros(NEND, dtype=np.int32), np.arange(NEND) % NPROB),
             (np.full(NEND, N - 1, dtype=np.int32), rng.permutation(NEND) % NPROB),
             (rng.integers(0, N, NEND).astype(np.int32), rng.permutation(NEND) % NPROB)]
    cases[2][0][:2] = (0, N - 1)
    per = 8 * (N * (m + 1) + 1) + 4                                 # scratch bytes of a point of a Jacobian call
    for pos, src in cases:
        src = src.astype(np.int32)
        pf, pj, pctx = ds.pin_launchers(fcn, jac, ctx, N, _dev(ds, src), _dev(ds, pos), _dev(ds, theta))
        got = {}
        for slices in (None, per * 5):
            with _env(NLH_PIN_SCRATCH=slices):
                got[slices] = (ds.fd_jacobian_device(pf, pctx, m, dx, jac=pj).cpu().numpy(), ds.fd_jacobian_device(pf, pctx, m, dx).cpu().numpy())
        pctx.close()
        for k in (0, 1):
            assert np.array_equal(_bits(got[None][k]), _bits(got[per * 5][k])), (m, N, k)
        for ps in sorted(set(pos.tolist())):
            sel = np.flatnonzero(pos == ps)
            rf, rj, rctx = ds.expr_launchers(e, _dev(ds, t[src[sel]]), _dev(ds, y[src[sel]]))
            full = np.zeros((len(sel), N))
            full[:, ps] = theta[sel]
            mf, mj, mctx = ds.pmap_launchers(nl.ParamMap(N, fixed=(ps,)), rf, rj, rctx, _dev(ds, full))
            xs = _dev(ds, x[sel])
            want = (ds.fd_jacobian_device(mf, mctx, m, xs, jac=mj).cpu().numpy(), ds.fd_jacobian_device(mf, mctx, m, xs).cpu().numpy())
            mctx.close()
            for k in (0, 1):
                assert np.isfinite(want[k]).all()
                assert np.array_equal(_bits(got[None][k][sel]), _bits(want[k])), (m, N, ps, k)


def test_pin_set_swaps_the_tables_and_the_launchers_refuse(ds):
    e = _formula(3)
    rng = np.random.default_rng(1)
    m = 40
    dt, dy = _dev(ds, rng.uniform(0.25, 4.0, (NPROB, m))), _dev(ds, rng.uniform(0.5, 3.0, (NPROB, m)))
    fcn, jac, ctx = ds.expr_launchers(e, dt, dy)
    tabs = lambda k: (_dev(ds, (np.arange(k) % NPROB).astype(np.int32)), _dev(ds, (np.arange(k) % 3).astype(np.int32)), _dev(ds, rng.uniform(1, 2, k)))
    a, b = tabs(7), tabs(4)
    pf, pj, pctx = ds.pin_launchers(fcn, jac, ctx, 3, *a)
    xa, xb = _dev(ds, rng.uniform(0.8, 1.6, (7, 2))), _dev(ds, rng.uniform(0.8, 1.6, (4, 2)))
    Ja = ds.fd_jacobian_device(pf, pctx, m, xa, jac=pj).cpu().numpy()
    ds.pin_set(pctx, *b)
    Jb = ds.fd_jacobian_device(pf, pctx, m, xb, jac=pj).cpu().numpy()
    ds.pin_set(pctx, *a)
    assert np.array_equal(_bits(ds.fd_jacobian_device(pf, pctx, m, xa, jac=pj).cpu().numpy()), _bits(Ja))
    pctx.close()
    qf, qj, qctx = ds.pin_launchers(fcn, jac, ctx, 3, *b)
    assert np.array_equal(_bits(ds.fd_jacobian_device(qf, qctx, m, xb, jac=qj).cpu().numpy()), _bits(Jb))
    # the wrong number of unknowns is refused before any launch; without an inner Jacobian there is no Jacobian launcher
    with pytest.raises(Exception):
        ds.fd_jacobian_device(qf, qctx, m, _dev(ds, np.ones((4, 3))), jac=qj)
    qctx.close()
    nf, nj, nctx = ds.pin_launchers(fcn, None, ctx, 3, *b)
    assert nj is None
    nctx.close()
    with pytest.raises(ValueError):
        ds.pin_launchers(fcn, jac, ctx, 3, a[0], b[1], a[2])                  # tables of different lengths


# ---------------------------------------------------------------------------------------------------------------------
# 7. start and step against the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _same_state(dst, st, what):
    torch.cuda.synchronize()
    for k in PR.NAMES:
        got = dst[k].cpu().numpy()
        if k in PR.F64:
            assert np.array_equal(_bits(got), _bits(st[k])), (what, k, np.flatnonzero(_bits(got) != _bits(st[k]))[:5])
        else:
            assert np.array_equal(got, st[k]), (what, k, np.flatnonzero(got != st[k])[:5])


@pytest.mark.parametrize("nend", [1, 63, 64, 65, 257])
def test_start_and_step_equal_the_restatement(ds, nend):
    """The synthetic costs of tests/test_profile_cpu.py, the first nend ends of the batch stepped: every array of the state
    after the start and after every step, and the count of running ends."""
    x, sigma, C0, lower, upper, cost, wfac, kinds = PC.synthetic(nend)
    nprob, m = x.shape[0], 10
    e = nl.Expr("a+b*s", ("s",), ("a", "b"))
    rng = np.random.default_rng(nend)
    t, y = rng.uniform(0.0, 1.0, (nprob, m)), rng.uniform(0.0, 8.0, (nprob, m))
    prog = e.program()
    C0[:] = S.cost(np.stack([ER.residual(prog, x[p], [t[p]], y[p]) for p in range(nprob)]))      # what the device's start computes
    fcn, jac, ctx = ds.expr_launchers(e, _dev(ds, t), _dev(ds, y))
    prof = Profile(maxit=12)
    st = PR.start(C0, x, sigma, m, prof.crit, True, None, lower, upper)
    dst = ds.profile_start(fcn, ctx, m, _dev(ds, x), _dev(ds, sigma), prof, None, True, lower, upper)
    _same_state(dst, st, "start")
    first = np.arange(len(st["theta"])) < nend
    for rnd in range(prof.maxit + 2):
        act = np.flatnonzero((st["phase"] != PR.DONE) & first)
        if len(act) == 0:
            break
        got = [cost(int(k), st["theta"][k], st) for k in act]
        c, f = np.array([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int32)
        left = PR.step(st, act, c, f, prof.tol, prof.xtol, prof.max_expand, prof.maxit)
        assert ds.profile_step(dst, _dev(ds, act, np.int32), _dev(ds, c), _dev(ds, f), prof) == left
        _same_state(dst, st, ("step", rnd))
    assert not ((st["phase"] != PR.DONE) & first).any()
    # a step without a fail array on entries that are out of range or name a finished end: nothing changes
    done = int(np.flatnonzero(st["phase"] == PR.DONE)[0])
    idle = _dev(ds, np.array([done, -1, 10 ** 6], dtype=np.int32))
    assert ds.profile_step(dst, idle, _dev(ds, np.ones(3)), None, prof) == int((st["phase"] != PR.DONE).sum())
    _same_state(dst, st, "idle step")


# ---------------------------------------------------------------------------------------------------------------------
# 8. end to end, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mm(ds):
    """The first 64 Michaelis-Menten data sets at sigma = 0.15, their fit on the device, and its one-call profile."""
    e = nl.Expr(PC.MM_FORMULA, PC.MM_VARS, PC.MM_PARAMS)
    s, y, x0 = PC.mm_problems(1, PC.NGPU)
    ds_, dy = _dev(ds, s), _dev(ds, y)
    x, fvec, sigma, cov, chi2, rank, ibs, status = ds.expr_fit_batch(e, ds_, dy, _dev(ds, x0))
    assert set(status) == {0}
    out = ds.expr_profile_batch(e, ds_, dy, x, sigma, Profile())
    return e, s, y, ds_, dy, x, sigma, tuple(o.cpu().numpy() for o in out)


def test_expr_profile_equals_the_restatement_over_the_oracle(ds, oracle, mm):
    """expr_profile_batch with the analytic Jacobian on an exp-free formula: lo, hi, flags and nev are the restatement's over
    oracle.lm_solve, bit for bit -- the pin pair only copies, so the mapped fits' bit claim holds for every pinned refit.  No
    end of these 64 data sets may be other than OK."""
    e, s, y, ds_, dy, x, sigma, (lo, hi, flags, nev) = mm
    xh, sh = x.cpu().numpy(), sigma.cpu().numpy()
    res, jac = PC.mm_callbacks(e.program(), s, y)
    C0 = S.cost(np.stack([res(p, xh[p]) for p in range(PC.NGPU)]))
    rlo, rhi, rflags, rnev, _ = PR.drive(xh, sh, C0, PC.MM_M, PR.oracle_solve(oracle, PC.MM_M, PC.MM_N, res, jac), PC.CRIT, PC.TOL, PC.XTOL,
                                         PC.MAX_EXPAND, PC.MAXIT)
    assert (rflags == PR.OK).all() and (flags == _lib.PROFILE_OK).all()
    assert np.array_equal(flags, rflags) and np.array_equal(nev, rnev)
    assert np.array_equal(_bits(lo), _bits(rlo)) and np.array_equal(_bits(hi), _bits(rhi))
    assert (lo < xh).all() and (xh < hi).all()
    _record(f"mm 64 x 16 rows, sigma 0.15: refits per end {nev.mean():.3f}; median half-widths in sigma, below / above: "
            f"{np.median((xh - lo) / sh, axis=0).round(3).tolist()} / {np.median((hi - xh) / sh, axis=0).round(3).tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# 9. end to end, counts
# ---------------------------------------------------------------------------------------------------------------------
def test_curve_profile_of_counts_against_the_restatement(ds, oracle):
    """curve_profile_batch(..., stat=Poisson()) on the first 64 decays of truth (50, 1, 0.5) against the restatement over the
    oracle with the deviance residuals: equal flags -- at most 1 of the 384 ends may be left out for differing flags --, and
    ends within 2*tol*sqrt(crit)*sigma: two searches that stop anywhere inside |g| <= tol*delta differ by at most
    tol*sqrt(crit)*sigma/2 each under the quadratic cost, times 2 for the measured skew of these profiles."""
    t, y, xt, x0 = BC.problems(0)
    t, y, x0 = t[:PC.NGPU], y[:PC.NGPU], x0[:PC.NGPU]
    stat = nl.Poisson()
    dt, dy = _dev(ds, t), _dev(ds, y)
    x, fvec, sigma, cov, chi2, rank, ibs, status = ds.curve_fit_batch("expdecay", dt, dy, _dev(ds, x0), baseline=0, stat=stat)
    assert set(status) == {0}
    prof = Profile()
    lo, hi, flags, nev = (o.cpu().numpy() for o in ds.curve_profile_batch("expdecay", dt, dy, x, sigma, prof, baseline=0, stat=stat))
    xh, sh = x.cpu().numpy(), sigma.cpu().numpy()
    res, jac = PC.decay_callbacks(t, y)
    C0 = S.cost(np.stack([res(p, xh[p]) for p in range(PC.NGPU)]))
    rlo, rhi, rflags, rnev, _ = PR.drive(xh, sh, C0, PO.M, PR.oracle_solve(oracle, PO.M, PO.N, res, jac), prof.crit, prof.tol, prof.xtol,
                                         prof.max_expand, prof.maxit, scaled=False)
    same = flags == rflags
    end, rend = np.stack([lo, hi], axis=2), np.stack([rlo, rhi], axis=2)
    with np.errstate(invalid="ignore"):
        diff = np.abs(end - rend) / (np.sqrt(prof.crit) * sh[:, :, None])
    both = same & np.isfinite(end) & np.isfinite(rend)
    worst = float(diff[both].max())
    _record(f"decays (50, 1, 0.5), 64 x 64 rows, stat=Poisson: ends with differing flags {int((~same).sum())} of {same.size}; largest difference "
            f"of an end {worst:.3e} in units of sqrt(crit)*sigma (allowed {2 * prof.tol:.3e}); refits per end {nev.mean():.3f}; "
            f"flags {({int(k): int(v) for k, v in zip(*np.unique(flags, return_counts=True))})}")
    assert int((~same).sum()) <= 1
    assert (np.isfinite(end) == np.isfinite(rend))[same].all() and np.array_equal(end[same & ~both], rend[same & ~both], equal_nan=True)
    assert worst <= 2 * prof.tol


# ---------------------------------------------------------------------------------------------------------------------
# 10. chunking, a mapped fit, a fit on its bound
# ---------------------------------------------------------------------------------------------------------------------
def test_chunking_does_not_change_a_bit(ds, mm):
    e, s, y, ds_, dy, x, sigma, want = mm
    with _env(NLH_PROFILE_ENDS=7):
        got = tuple(o.cpu().numpy() for o in ds.expr_profile_batch(e, ds_, dy, x, sigma, Profile()))
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8))
    # and forward differences over the N - 1 unknowns find the same ends to the tolerance (other refits, the same profile)
    fd = tuple(o.cpu().numpy() for o in ds.expr_profile_batch(e, ds_, dy, x, sigma, Profile(), analytic=False))
    assert (fd[2] == _lib.PROFILE_OK).all()
    sh = sigma.cpu().numpy()
    assert (np.abs(fd[0] - want[0]) <= 2 * PC.TOL * np.sqrt(PC.CRIT) * sh).all() and (np.abs(fd[1] - want[1]) <= 2 * PC.TOL * np.sqrt(PC.CRIT) * sh).all()


def test_mapped_fit_profiles_the_free_parameters(ds, mm):
    """pmap= with one fixed parameter: NaN and NOT_FREE there; the other ends are those of the profile of the reduced formula."""
    e, s, y, ds_, dy, x, sigma, _ = mm
    e3 = nl.Expr("vmax*s/(km+s)+c", ("s",), ("vmax", "km", "c"))
    dy3 = dy + 0.25
    x3 = torch.cat([x, torch.full((PC.NGPU, 1), 0.25, dtype=torch.float64, device=ds.device)], dim=1).contiguous()
    s3 = torch.cat([sigma, torch.zeros((PC.NGPU, 1), dtype=torch.float64, device=ds.device)], dim=1).contiguous()
    lo, hi, flags, nev = (o.cpu().numpy() for o in ds.expr_profile_batch(e3, ds_, dy3, x3, s3, Profile(), pmap=nl.ParamMap.for_expr(e3, fixed=("c",))))
    assert np.isnan(lo[:, 2]).all() and np.isnan(hi[:, 2]).all() and (flags[:, 2] == _lib.PROFILE_NOT_FREE).all() and (nev[:, 2] == 0).all()
    er = nl.Expr("vmax*s/(km+s)+0.25", ("s",), ("vmax", "km"))
    rlo, rhi, rflags, rnev = (o.cpu().numpy() for o in ds.expr_profile_batch(er, ds_, dy3, x, sigma, Profile()))
    assert np.array_equal(_bits(lo[:, :2]), _bits(rlo)) and np.array_equal(_bits(hi[:, :2]), _bits(rhi))
    assert np.array_equal(flags[:, :2], rflags) and np.array_equal(nev[:, :2], rnev) and (rflags == _lib.PROFILE_OK).all()


def test_fit_on_its_bound_is_on_bound(ds, mm):
    """A bounded fit whose km ends on its upper bound: ON_BOUND with the bound as the end above, an ordinary end below, and the
    other parameter's refits stay inside the box."""
    e, s, y, ds_, dy, _, _, _ = mm
    lower, upper = np.array([0.0, 0.5]), np.array([50.0, 3.0])                 # the truth's km = 4 lies outside
    x0 = _dev(ds, np.tile(np.array([8.0, 2.0]), (PC.NGPU, 1)))
    x, fvec, sigma, cov, chi2, rank, ibs, status = ds.expr_fit_batch(e, ds_, dy, x0, lower=lower, upper=upper)
    xh = x.cpu().numpy()
    on = (xh[:, 1] == upper[1]) & np.array([st == 0 for st in status]) & np.isfinite(sigma.cpu().numpy()).all(axis=1)
    assert on.sum() >= 8
    lo, hi, flags, nev = (o.cpu().numpy() for o in ds.expr_profile_batch(e, ds_, dy, x, sigma, Profile(), lower=lower, upper=upper))
    assert ((flags[on, 1, 1] & 15) == _lib.PROFILE_ON_BOUND).all() and (hi[on, 1] == upper[1]).all() and (nev[on, 1, 1] == 0).all()
    assert ((flags[on, 1, 0] & 15) != _lib.PROFILE_ON_BOUND).all() and (nev[on, 1, 0] >= 1).all()
    fin = np.isfinite(lo) & np.isfinite(hi)
    assert (lo[fin] >= np.broadcast_to(lower, lo.shape)[fin]).all() and (hi[fin] <= np.broadcast_to(upper, hi.shape)[fin]).all()
