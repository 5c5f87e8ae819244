"""bootstrap (include/nonlin_hip_boot.h: nlh_boot_*), restated in numpy: the generator in uint64 arithmetic, every floating-point
step one IEEE operation in the header's order.  Everything here is meant bit for bit.  Test infrastructure, not part of the
product."""
import numpy as np

RESIDUAL, WILD, PAIRS = 0, 1, 2
KINDS = {"residual": RESIDUAL, "wild": WILD, "pairs": PAIRS}
MAX_ROWS, MAX_REP = 16384, 4096
G = np.uint64(0x9E3779B97F4A7C15)
_C1, _C2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_MASK = (1 << 64) - 1


def _u(v):
    return np.uint64(int(v) & _MASK)


def mix(z):
    """z = (z ^ (z >> 30))*C1; z = (z ^ (z >> 27))*C2; z ^ (z >> 31), mod 2^64 (a scalar or an array of uint64)."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * _C1
        z = (z ^ (z >> np.uint64(27))) * _C2
        return z ^ (z >> np.uint64(31))


def key(seed, p, b):
    """key = mix(mix(seed + G*(p + 1)) + G*(b + 1))."""
    with np.errstate(over="ignore"):
        return mix(mix(_u(seed) + G * _u(p + 1)) + G * _u(b + 1))


def raw(seed, p, b, ks):
    """z of the draws ks (an integer array) of the stream (seed, p, b)."""
    with np.errstate(over="ignore"):
        return mix(key(seed, p, b) + G * (np.asarray(ks, dtype=np.uint64) + np.uint64(1)))


def index(z, cnt):
    """j = ((z >> 32)*cnt) >> 32."""
    return (((z >> np.uint64(32)) * np.uint64(cnt)) >> np.uint64(32)).astype(np.int64)


def draws(seed, p, b, first, count, cnt):
    """nlh_boot_draws: the indices below cnt, or with cnt == 0 the sign bits."""
    z = raw(seed, p, b, np.arange(first, first + count))
    return (index(z, cnt) if cnt else (z >> np.uint64(63)).astype(np.int64)).astype(np.int32)


def tree_sum(v):
    """The sum of v in the order of the starts cost: 64 partials, element i to partial i mod 64 ascending, then the tree."""
    part = np.zeros(64)
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i0 in range(0, len(v), 64):
            w = min(64, len(v) - i0)
            part[:w] = part[:w] + v[i0:i0 + w]
        off = 32
        while off:
            part[:off] = part[:off] + part[off:2 * off]
            off //= 2
    return part[0]


def active_sum(e, act):
    """... of the values e [m] of the active rows only, a row's partial being its ROW number mod 64."""
    part = np.zeros(64)
    for i0 in range(0, len(e), 64):
        idx = np.flatnonzero(act[i0:i0 + 64])
        part[idx] = part[idx] + e[i0 + idx]
    off = 32
    while off:
        part[:off] = part[:off] + part[off:2 * off]
        off //= 2
    return part[0]


def resample_one(kind, seed, p, b, mu, y, w, centre):
    """(y*, w*) [m] of replica b of problem p (its index in the whole data); w is None without weights."""
    y = np.asarray(y, dtype=np.float64)
    m = len(y)
    act = np.ones(m, dtype=bool) if w is None else (np.asarray(w) != 0.0)
    rows = np.flatnonzero(act)                                                 # active number -> row
    cnt = len(rows)
    ys, ws = y.copy(), (None if w is None else np.array(w, dtype=np.float64))
    if kind == PAIRS and ws is None:
        ws = np.ones(m)
    if cnt == 0:
        return ys, ws
    with np.errstate(all="ignore"):
        if kind == RESIDUAL:
            e = y - mu
            if w is not None:
                e = w * e
            if centre:
                ebar = active_sum(e, act) / np.float64(cnt)
                e = e - ebar
            j = index(raw(seed, p, b, np.arange(cnt)), cnt)
            ej = e[rows[j]]
            if w is not None:
                ej = ej / w[rows]
            ys[rows] = mu[rows] + ej
        elif kind == WILD:
            d = y - mu
            neg = (raw(seed, p, b, rows) >> np.uint64(63)).astype(bool)
            ys[rows] = np.where(neg, mu[rows] - d[rows], mu[rows] + d[rows])
        else:
            c = np.bincount(index(raw(seed, p, b, np.arange(cnt)), cnt), minlength=cnt)
            s = np.sqrt(c.astype(np.float64))
            ws[rows] = s if w is None else w[rows] * s
    return ys, ws


def resample(kind, seed, mu, y, w, centre, nrep, prob0=0, rep0=0):
    """(y* [nrep, nprob, m], w* the same or None): nlh_boot_resample_batch."""
    nprob, m = y.shape
    ys = np.empty((nrep, nprob, m))
    ws = np.empty((nrep, nprob, m)) if kind == PAIRS else None
    for r in range(nrep):
        for p in range(nprob):
            a, c = resample_one(kind, seed, prob0 + p, rep0 + r, None if mu is None else mu[p], y[p], None if w is None else w[p], centre)
            ys[r, p] = a
            if ws is not None:
                ws[r, p] = c
    return ys, ws


def stable_sort(v):
    """v ascending by IEEE <, equal values (+0.0 and -0.0 among them) in their given order."""
    v = np.asarray(v, dtype=np.float64)
    return v[np.argsort(v, kind="stable")]


def quantile(xs, q):
    """h = q*(cnt - 1); k = floor(h); g = h - k; v = x_k + g*(x_{min(k+1, cnt-1)} - x_k) of the sorted xs."""
    cnt = len(xs)
    h = np.float64(q) * np.float64(cnt - 1)
    k = int(np.floor(h))
    g = h - np.float64(k)
    with np.errstate(all="ignore"):
        return xs[k] + g * (xs[min(k + 1, cnt - 1)] - xs[k])


def summary(xs, level):
    """(lo, hi, mean, sd [nprob, n], nvalid [nprob]) of xs [nrep, nprob, n]: nlh_boot_summary_batch."""
    xs = np.asarray(xs, dtype=np.float64)
    nrep, nprob, n = xs.shape
    qlo = (np.float64(1.0) - np.float64(level)) / np.float64(2.0)
    qhi = np.float64(1.0) - qlo
    lo, hi, mean, sd = (np.full((nprob, n), np.nan) for _ in range(4))
    valid = np.isfinite(xs).all(axis=2)
    nvalid = valid.sum(axis=0).astype(np.int32)
    for p in range(nprob):
        cnt = int(nvalid[p])
        if cnt == 0:
            continue
        for j in range(n):
            v = stable_sort(xs[valid[:, p], p, j])
            mn = tree_sum(v) / np.float64(cnt)
            mean[p, j] = mn
            if cnt > 1:
                d = v - mn
                with np.errstate(all="ignore"):
                    sd[p, j] = np.sqrt(tree_sum(d * d) / np.float64(cnt - 1))
            lo[p, j], hi[p, j] = quantile(v, qlo), quantile(v, qhi)
    return lo, hi, mean, sd, nvalid
