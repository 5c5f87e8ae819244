"""The bin-summing transform (include/nonlin_hip_bin.h: nlh_bin_*) restated in numpy, step by step in the operation order the
header states: a loop over the nodes q ascending, each step one multiply and one add on whole arrays, so that the bits are
the device kernel's.  Columns are arrays whose LAST axis is the Q m node-major rows: entry q m + i is node q of bin i.  Test
infrastructure, not part of the product."""
import numpy as np

MAX_Q = 16
U = 2.0 ** -53


def reduce(v, c, s=None):
    """g_i = s_i * (sum over q ascending of c[q] * v[q m + i]) along the last axis of v [..., Q m]; s None (no scale), [m] or
    [..., m] broadcasting against v's leading axes (a scale per problem)."""
    v = np.asarray(v, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    Q = len(c)
    m = v.shape[-1] // Q
    assert v.shape[-1] == Q * m
    acc = np.zeros(v.shape[:-1] + (m,))
    with np.errstate(all="ignore"):
        for q in range(Q):
            t = c[q] * v[..., q * m:(q + 1) * m]
            acc = acc + t
        return acc if s is None else np.asarray(s, dtype=np.float64) * acc


def weigh(out, w):
    """out times the weights w (None: none); a bin with w == 0.0 is +0.0 whatever out holds."""
    if w is None:
        return out
    with np.errstate(all="ignore"):
        return np.where(w == 0.0, 0.0, w * out)


def residual(v, y, w, c, s=None):
    """F of the inner model values v [..., Q m]: g - y, times w; a zero-weight bin is +0.0."""
    with np.errstate(all="ignore"):
        return weigh(reduce(v, c, s) - y, w)


def jacobian(J, w, c, s=None):
    """J' of the inner Jacobian J [..., n, Q m] (a column per parameter, rows last); w, s [..., m] per problem or [m]."""
    s = None if s is None else (np.asarray(s) if np.ndim(s) == 1 else np.asarray(s)[..., None, :])
    return weigh(reduce(J, c, s), None if w is None else np.asarray(w)[..., None, :])


def scalar(v, c, s=None):
    """The same chain, one bin and one node at a time in Python floats (one column, one scale row)."""
    Q = len(c)
    m = len(v) // Q
    out = np.empty(m)
    for i in range(m):
        acc = 0.0
        for q in range(Q):
            t = float(c[q]) * float(v[q * m + i])
            acc = acc + t
        out[i] = float(s[i]) * acc if s is not None else acc
    return out


def nodes(lo, hi, xi):
    """tq [..., Q m]: mid + half * xi_q, node-major, with mid = 0.5 (lo + hi), half = 0.5 (hi - lo)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return np.concatenate([mid + half * x for x in xi], axis=-1)
