"""Profile-likelihood intervals (include/nonlin_hip_profile.h: nlh_pin_*, nlh_profile_*), restated in numpy: the copies of the pin
pair, the start and the step of the root finder -- one IEEE operation per statement, as the header states them --, and the
driver loop of DeviceSolver.profile_batch_device over a solve callback.  Test infrastructure, not part of the product."""
import math

import numpy as np

import starts_restatement as S

EXPAND, BRACKET, DONE = 0, 1, 2
OK, OPEN, OPEN_AT_BOUND, ON_BOUND, MAXIT, FIT_FAILED, NO_START, NOT_FREE = range(8)
LOWER = 16
F64 = ("C0", "delta", "xhat", "width", "bound", "theta", "a", "ga", "b", "gb", "end")
I32 = ("phase", "flag", "last", "nexp", "nev", "nfail")
NAMES = F64 + I32


def crit_of(level):
    """The squared normal quantile of (1 + level)/2: Profile's default."""
    import statistics
    z = statistics.NormalDist().inv_cdf((1.0 + level) / 2.0)
    return z * z


# ---- the pin pair: only copies -------------------------------------------------------------------------------------------
def pin_expand(x, pos, theta):
    """P [npoints, N] of x [npoints, N - 1]: below pos in place, theta at pos, the rest shifted by one."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([np.insert(x[q], int(pos[q]), theta[q]) for q in range(x.shape[0])]) if x.shape[0] else np.empty((0, x.shape[1] + 1))


def pin_delete(Jf, pos):
    """dJ [npoints, N - 1, m] of Jf [npoints, N, m]: column pos deleted per point."""
    return np.stack([np.delete(Jf[q], int(pos[q]), axis=0) for q in range(Jf.shape[0])])


# ---- the root finder -----------------------------------------------------------------------------------------------------
def _clip(theta, bound, s):
    if s == 0:
        return bound if theta < bound else theta
    return bound if theta > bound else theta


def _finish(st, e, code, end):
    st["flag"][e] |= code
    st["end"][e] = end
    st["phase"][e] = DONE


def start(C0, x, sigma, m, crit, scaled=True, dof=None, lower=None, upper=None):
    """The state after nlh_profile_start_batch_device, C0 [nprob] given (the cost of the fit by starts_restatement.cost)."""
    x, sigma = np.asarray(x, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    nprob, n = x.shape
    nend = nprob * n * 2
    st = {k: np.full(nprob if k in ("C0", "delta") else nend, np.nan) for k in F64}
    st.update({k: np.zeros(nend, dtype=np.int32) for k in I32})
    crit = np.float64(crit)
    rc = np.sqrt(crit)
    with np.errstate(all="ignore"):
        for p in range(nprob):
            c0 = np.float64(C0[p])
            d = int(dof[p]) if dof is not None else m - n
            delta = crit
            if scaled:
                delta = crit * c0
                delta = delta / np.float64(d)
            st["C0"][p], st["delta"][p] = c0, delta
            for j in range(n):
                for s in (0, 1):
                    e = (p * n + j) * 2 + s
                    xh, sg = x[p, j], sigma[p, j]
                    bound = np.float64((np.inf if upper is None else upper[j]) if s else (-np.inf if lower is None else lower[j]))
                    w = rc * sg
                    theta = _clip(xh + w if s else xh - w, bound, s)
                    st["xhat"][e], st["width"][e], st["bound"][e] = xh, w, bound
                    st["a"][e], st["ga"][e], st["theta"][e] = xh, -delta, theta
                    st["phase"][e] = EXPAND
                    ok = (np.isfinite(xh) and np.isfinite(sg) and sg > 0 and np.isfinite(c0) and c0 > 0 and np.isfinite(delta) and delta > 0
                          and d > 0 and np.isfinite(crit) and crit > 0)
                    if not ok:
                        _finish(st, e, NO_START, np.nan)
                    elif (xh >= bound) if s else (xh <= bound):
                        _finish(st, e, ON_BOUND, bound)
    return st


def step(st, act, cost, fail, tol, xtol, max_expand, maxit):
    """nlh_profile_step_batch on the state, in place; returns how many ends still run."""
    n = len(st["theta"]) // (2 * max(len(st["C0"]), 1))
    tol, xtol, half, two = np.float64(tol), np.float64(xtol), np.float64(0.5), np.float64(2.0)
    with np.errstate(all="ignore"):
        for i, e in enumerate(act):
            e = int(e)
            if e < 0 or e >= len(st["theta"]) or st["phase"][e] == DONE:
                continue
            s, p = e & 1, e // (2 * n)
            c = np.float64(cost[i])
            st["nev"][e] += 1
            nev = st["nev"][e]
            theta, a, b, ga, gb = (st[k][e] for k in ("theta", "a", "b", "ga", "gb"))
            if (fail is not None and fail[i] != 0) or not np.isfinite(c):
                st["nfail"][e] += 1
                if st["nfail"][e] > 3:
                    _finish(st, e, FIT_FAILED, np.nan)
                    continue
                d = theta - a
                d = d * half
                theta = a + d
                st["theta"][e] = theta
                if nev >= maxit:
                    _finish(st, e, MAXIT, theta)
                continue
            st["nfail"][e] = 0
            C0, delta = st["C0"][p], st["delta"][p]
            t = tol * delta
            g = c - C0
            g = g - delta
            if c < C0 - t:
                st["flag"][e] |= LOWER
            if abs(g) <= t:
                _finish(st, e, OK, theta)
                continue
            xh, bound, last = st["xhat"][e], st["bound"][e], st["last"][e]
            if st["phase"][e] == EXPAND:
                if g < 0:
                    st["a"][e], st["ga"][e] = theta, g
                    if theta == bound:
                        _finish(st, e, OPEN_AT_BOUND, bound)
                    elif st["nexp"][e] >= max_expand:
                        _finish(st, e, OPEN, np.inf if s else -np.inf)
                    else:
                        st["nexp"][e] += 1
                        d = theta - xh
                        d = two * d
                        theta = _clip(xh + d, bound, s)
                        st["theta"][e] = theta
                        if nev >= maxit:
                            _finish(st, e, MAXIT, theta)
                    continue
                b, gb, last = theta, g, 1
                st["phase"][e] = BRACKET
            elif g < 0:
                a, ga = theta, g
                if last == -1:
                    gb = gb * half
                last = -1
            else:
                b, gb = theta, g
                if last == 1:
                    ga = ga * half
                last = 1
            st["a"][e], st["ga"][e], st["b"][e], st["gb"][e], st["last"][e] = a, ga, b, gb, last
            u, v = a * gb, b * ga
            u = u - v
            v = gb - ga
            theta = u / v
            d = b - a
            if not ((a < theta < b) or (b < theta < a)):
                theta = a + d * half
            st["theta"][e] = theta
            if abs(d) <= xtol * st["width"][e]:
                _finish(st, e, OK, theta)
            elif nev >= maxit:
                _finish(st, e, MAXIT, theta)
    return int((st["phase"] != DONE).sum())


def drive(x, sigma, C0, m, solve, crit, tol=0.01, xtol=1e-3, max_expand=8, maxit=30, scaled=True, dof=None, lower=None, upper=None,
          on_step=None):
    """DeviceSolver.profile_batch_device's loop: start, then rounds of -- solve(p, j, theta, warm) -> (cost, fail, x_new) for every
    active end, from the solution of its latest successful refit (at first x without entry j) -- and step.  Returns
    (lo, hi [nprob, n], flags, nev [nprob, n, 2], state)."""
    x = np.asarray(x, dtype=np.float64)
    nprob, n = x.shape
    st = start(C0, x, sigma, m, crit, scaled, dof, lower, upper)
    warm = {}
    while True:
        act = np.flatnonzero(st["phase"] != DONE)
        if len(act) == 0:
            break
        cost, fail = np.empty(len(act)), np.zeros(len(act), dtype=np.int32)
        for i, e in enumerate(act):
            p, j = e // (2 * n), (e // 2) % n
            w0 = warm.get(e, np.delete(x[p], j))
            cost[i], fail[i], xn = solve(p, j, st["theta"][e], w0.copy())
            if not fail[i] and np.isfinite(cost[i]):
                warm[e] = np.array(xn, dtype=np.float64)
        step(st, act, cost, fail, tol, xtol, max_expand, maxit)
        if on_step is not None:
            on_step(st)
    end = st["end"].reshape(nprob, n, 2)
    return end[:, :, 0].copy(), end[:, :, 1].copy(), st["flag"].reshape(nprob, n, 2).copy(), st["nev"].reshape(nprob, n, 2).copy(), st


def oracle_solve(oracle, m, N, residual, jacobian=None, lower=None, upper=None, opts=None):
    """A solve callback for drive() over the CPU oracle's LM (cls with a box): residual(p, full) -> F [m] and
    jacobian(p, full) -> J [m, N] (None: forward differences) of inner problem p at the full parameters; the pinned refit of
    (p, j, theta) works on the N - 1 others, expanded and contracted as the pin pair does."""
    o = opts or oracle.default_options()

    def solve(p, j, theta, warm):
        def fcn(xr, f):
            f[:] = residual(p, np.insert(xr, j, theta))

        def jfull(xr, J):
            J[:, :] = np.delete(jacobian(p, np.insert(xr, j, theta)), j, axis=1)
        jac = None if jacobian is None else jfull
        with np.errstate(all="ignore"):
            if lower is None and upper is None:
                rc, xs, fv, ib = oracle.lm_solve(fcn, m, N - 1, warm, jac=jac, opts=o)[:4]
            else:
                lo = None if lower is None else np.delete(np.asarray(lower, dtype=np.float64), j)
                hi = None if upper is None else np.delete(np.asarray(upper, dtype=np.float64), j)
                rc, xs, fv, ib = oracle.cls_solve(fcn, m, N - 1, warm, jac=jac, opts=o, lower=lo, upper=hi)[:4]
        return S.cost(np.asarray(fv)[None])[0], int(rc != 0), xs
    return solve


def fit_cost(F):
    """C0 of residuals F [nprob, m]."""
    return S.cost(np.asarray(F, dtype=np.float64))
