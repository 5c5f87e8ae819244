"""starts (include/nonlin_hip_starts.h: nlh_starts_*), restated in numpy: one IEEE operation per step in the header's order.  The
radical inverse and the linear map, the cost sum and the selection are meant bit for bit; a log dimension goes through the
host's libm and is compared within a few ulp.  Test infrastructure, not part of the product."""
import numpy as np

MAX_N, MAX_KEEP, MAX_CAND = 32, 8, 1 << 20
PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131)


def radical_inverse(i, p):
    """f = 1.0/p; r = +0.0; while i > 0: r = r + f*(i mod p); i = i div p; f = f/p."""
    f = np.float64(1.0) / np.float64(p)
    r = np.float64(0.0)
    i = int(i)
    while i > 0:
        r = r + f * np.float64(i % p)
        i = i // p
        f = f / np.float64(p)
    return r


def unit(first, count, n):
    """u [count, n]: coordinate d of candidate c is the radical inverse of c + 1 in the d-th prime."""
    return np.array([[radical_inverse(c + 1, PRIMES[d]) for d in range(n)] for c in range(first, first + count)], dtype=np.float64).reshape(count, n)


def candidates(lower, upper, log=(), first=0, count=1):
    """The table [count, n]: v = lo + u*(hi - lo), or lo*exp(u*log(hi/lo)) where log, clamped to the box."""
    lo, hi = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    u = unit(first, count, len(lo))
    out = np.empty_like(u)
    for d in range(len(lo)):
        if d in set(log):
            v = lo[d] * np.exp(u[:, d] * np.log(hi[d] / lo[d]))
        else:
            v = lo[d] + u[:, d] * (hi[d] - lo[d])
        v = np.where(v < lo[d], lo[d], v)
        out[:, d] = np.where(v > hi[d], hi[d], v)
    return out


def cost(F):
    """sum F_i^2 of every row of F [npoints, m]: 64 partials, partial j over the rows i = j (mod 64) in ascending i, then
    s_j = s_j + s_{j+off} for j < off, off = 32, 16, .., 1."""
    F = np.asarray(F, dtype=np.float64)
    npoints, m = F.shape
    part = np.zeros((npoints, 64))
    with np.errstate(over="ignore", invalid="ignore"):
        for i0 in range(0, m, 64):
            w = min(64, m - i0)
            part[:, :w] = part[:, :w] + F[:, i0:i0 + w] * F[:, i0:i0 + w]
        off = 32
        while off:
            part[:, :off] = part[:, :off] + part[:, off:2 * off]
            off //= 2
    return part[:, 0].copy()


def select(costs, keep):
    """(cost [keep], index [keep]) of one problem's costs [ncand]: a stable sort by cost over the finite ones -- ties keep
    the lower index --, the first `keep`; what is left over is +Inf / -1."""
    c = np.asarray(costs, dtype=np.float64)
    fin = np.flatnonzero(np.isfinite(c))
    order = fin[np.argsort(c[fin], kind="stable")][:keep]
    oc, oi = np.full(keep, np.inf), np.full(keep, -1, dtype=np.int32)
    oc[:len(order)] = c[order]
    oi[:len(order)] = order
    return oc, oi


def search(costs, table, keep):
    """(x0 [nprob, keep, n], cost [nprob, keep], index [nprob, keep]) of costs [nprob, ncand] and the table [ncand, n]."""
    nprob = costs.shape[0]
    oc = np.empty((nprob, keep))
    oi = np.empty((nprob, keep), dtype=np.int32)
    for p in range(nprob):
        oc[p], oi[p] = select(costs[p], keep)
    x0 = np.where((oi < 0)[:, :, None], np.nan, table[np.maximum(oi, 0)])
    return x0, oc, oi


def pick(costs):
    """which [nprob] of costs [keep, nprob]: the lowest k of the smallest finite cost, -1 when none is finite."""
    c = np.asarray(costs, dtype=np.float64)
    masked = np.where(np.isfinite(c), c, np.inf)
    return np.where(np.isfinite(c).any(axis=0), np.argmin(masked, axis=0), -1).astype(np.int32)


def take(src, which):
    """dst [nprob, ...] = src[which[p], p], NaN for -1."""
    src = np.asarray(src, dtype=np.float64)
    out = src[np.maximum(which, 0), np.arange(src.shape[1])]
    return np.where((np.asarray(which) < 0).reshape((-1,) + (1,) * (out.ndim - 1)), np.nan, out)
