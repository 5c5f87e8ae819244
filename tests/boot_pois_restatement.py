"""Poisson bootstrap (include/nonlin_hip_boot_pois.h: nlh_boot_poisson_*), restated in numpy: the generator in uint64 arithmetic
from boot_restatement, the setup and the draw vectorised over elements with the walks as masked loops, every floating-point
step one IEEE operation in the header's order.  Everything here is meant bit for bit.  Test infrastructure, not part of the
product."""
import numpy as np

import boot_restatement as B

MAX_MEAN = 2.0 ** 24
EPS = 2.0 ** -60
COPY, ZERO, ORDINARY = 0, 1, 2                                                  # what a row's draws are: y, +0.0, a walk


def bad_mean(mu):
    """A mean no draw is made from: a NaN, below 0 (not -0.0) or above 2^24."""
    mu = np.asarray(mu, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ~((mu >= 0.0) & (mu <= MAX_MEAN))


def setup(mu):
    """(M, L, T, kmin, kmax, r) of every element of mu, all of them inside (0, 2^24]:
    M = floor(mu);  r = 1/mu;  L = sum of q over k = M .. 1, q = (q*k)*r, until q < EPS;  U = 1 + sum of q over k = M+1 .., q = (q*mu)/k,
    until q < EPS;  T = L + U;  kmin = M - (terms of L);  kmax = M + (terms of U beyond the first)."""
    mu = np.asarray(mu, dtype=np.float64)
    assert ((mu > 0.0) & (mu <= MAX_MEAN)).all()
    with np.errstate(all="ignore"):                                           # (what a finished element goes on computing is dropped)
        return _setup(mu)


def _setup(mu):
    M, r = np.floor(mu), 1.0 / mu
    L, q, nd, k = np.zeros_like(mu), np.ones_like(mu), np.zeros_like(mu), M.copy()
    on = k >= 1.0
    while on.any():
        qn = (q * k) * r
        on = on & ~(qn < EPS)                                                  # a row that stops keeps its L and nd
        q = np.where(on, qn, q)
        L = np.where(on, L + q, L)
        nd = np.where(on, nd + 1.0, nd)
        k = k - 1.0
        on = on & (k >= 1.0)
    U, q, nu, k = np.ones_like(mu), np.ones_like(mu), np.zeros_like(mu), M + 1.0
    on = np.ones(mu.shape, dtype=bool)
    while on.any():
        qn = (q * mu) / k
        on = on & ~(qn < EPS)
        q = np.where(on, qn, q)
        U = np.where(on, U + q, U)
        nu = np.where(on, nu + 1.0, nu)
        k = k + 1.0
    return M, L, L + U, M - nd, M + nu, r


def walk(st, mu, z):
    """The draws of ordinary elements: st = setup(mu), z their uint64 draws (broadcast against st)."""
    with np.errstate(all="ignore"):                                           # (what a finished element goes on computing is dropped)
        return _walk(st, mu, z)


def _walk(st, mu, z):
    M, L, T, kmin, kmax, r = st
    u = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    t = u * T
    shape = t.shape
    M, L, kmin, kmax, r, mu = (np.broadcast_to(a, shape) for a in (M, L, kmin, kmax, r, mu))
    down = t < L
    # below the mode
    s, k, q = L - t, M - 1.0, M * r
    on = down & (s > q) & (k > kmin)
    while on.any():
        s = np.where(on, s - q, s)
        q = np.where(on, (q * k) * r, q)
        k = np.where(on, k - 1.0, k)
        on = on & (s > q) & (k > kmin)
    kd = k
    # the mode and above
    s, k, q = t - L, M.copy(), np.ones(shape)
    on = ~down & (s >= q) & (k < kmax)
    while on.any():
        s = np.where(on, s - q, s)
        k = np.where(on, k + 1.0, k)
        q = np.where(on, (q * mu) / k, q)
        on = on & (s >= q) & (k < kmax)
    return np.where(down, kd, k)


def classes(mu, w):
    """(class [m], bad [m]) of a problem's rows: COPY (inactive, or bad), ZERO, ORDINARY; bad: an active row with a bad mean."""
    mu = np.asarray(mu, dtype=np.float64)
    act = np.ones(mu.shape, dtype=bool) if w is None else (np.asarray(w) != 0.0)
    bad = act & bad_mean(mu)
    cls = np.where(~act | bad, COPY, np.where(mu == 0.0, ZERO, ORDINARY))
    return cls, bad


def draws(seed, p, b, first, mu):
    """nlh_boot_poisson_draws: out[j] the draw of row first + j for the mean mu[j]; a NaN for a bad mean."""
    mu = np.asarray(mu, dtype=np.float64)
    cls, bad = classes(mu, None)
    out = np.where(bad, np.nan, 0.0)
    o = cls == ORDINARY
    if o.any():
        z = B.raw(seed, p, b, first + np.flatnonzero(o))
        out[o] = walk(setup(mu[o]), mu[o], z)
    return out


def poisson_one(seed, p, b, mu, y, w):
    """(y* [m], bad) of replica b of problem p (its index in the whole data); w is None without weights."""
    ys, bad = poisson(seed, np.asarray(mu)[None], np.asarray(y)[None], None if w is None else np.asarray(w)[None], 1, prob0=p, rep0=b)
    return ys[0, 0], int(bad[0])


def poisson(seed, mu, y, w, nrep, prob0=0, rep0=0):
    """(y* [nrep, nprob, m], bad [nprob] int32): nlh_boot_poisson_batch.  A row's setup is made once for all its replicas."""
    mu, y = np.asarray(mu, dtype=np.float64), np.asarray(y, dtype=np.float64)
    nprob, m = y.shape
    ys = np.empty((nrep, nprob, m))
    nbad = np.zeros(nprob, dtype=np.int32)
    for p in range(nprob):
        cls, bad = classes(mu[p], None if w is None else w[p])
        nbad[p] = bad.sum()
        ys[:, p] = np.where(cls == ZERO, 0.0, y[p])[None, :]
        rows = np.flatnonzero(cls == ORDINARY)
        if len(rows) and nrep:
            mo = mu[p, rows]
            z = np.stack([B.raw(seed, prob0 + p, rep0 + r, rows) for r in range(nrep)])
            ys[:, p, rows] = walk(setup(mo), mo, z)
    return ys, nbad
