"""The instrument-response transform (include/nonlin_hip.h: nlh_conv_*) restated in numpy, step by step in the operation
order the header states: a loop over the taps j ascending, each step one multiply and one add on whole arrays, so that the
bits are the device kernels'.  Columns are arrays whose LAST axis is the m rows.  Test infrastructure, not part of the
product."""
import numpy as np

ZERO, HOLD = 0, 1
MAX_L = 1024
U = 2.0 ** -53


def convolve(v, k, origin, ext):
    """c_i = sum over j ascending of k[j] * v[i + origin - j], along the last axis of v; k [L], or [..., L] broadcasting against
    v's leading axes (a kernel per problem).  ZERO: a tap whose row lies outside 0 .. m-1 is skipped; HOLD: it reads the
    nearest edge row."""
    v = np.asarray(v, dtype=np.float64)
    k = np.asarray(k, dtype=np.float64)
    m, L = v.shape[-1], k.shape[-1]
    i = np.arange(m)
    acc = np.zeros(v.shape)
    with np.errstate(all="ignore"):
        for j in range(L):
            s = i + origin - j
            inside = (s >= 0) & (s < m)
            t = k[..., j:j + 1] * v[..., np.clip(s, 0, m - 1)]
            acc = acc + t if ext == HOLD else np.where(inside, acc + t, acc)
    return acc


def weigh(out, w):
    """out times the weights w (None: none); a row with w == 0.0 is +0.0 whatever out holds."""
    if w is None:
        return out
    with np.errstate(all="ignore"):
        return np.where(w == 0.0, 0.0, w * out)


def residual(r, y, w, k, origin, ext):
    """out of the inner residual r = model - y [..., m]: mu = r + y, c over mu, c - y, times w; a zero-weight row is +0.0."""
    mu = r + y
    return weigh(convolve(mu, k, origin, ext) - y, w)


def jacobian(J, w, k, origin, ext):
    """J' of the inner Jacobian J [..., n, m] (a column per parameter, rows last); w [..., m]; k [L] or [..., L] per problem."""
    k = np.asarray(k, dtype=np.float64)
    c = convolve(J, k if k.ndim == 1 else k[..., None, :], origin, ext)
    return weigh(c, None if w is None else np.asarray(w)[..., None, :])


def bound(v, k, origin, ext):
    """The first-order bound of the header's chain against the exact sum, per row: 2 L 2^-53 sum_j |k_j v_s| (L multiplies
    rounded once each, and a chain of L adds: at most L + (L - 1) roundings on any term)."""
    L = np.shape(k)[-1]
    return 2.0 * L * U * convolve(np.abs(v), np.abs(k), origin, ext)


def scalar(v, k, origin, ext):
    """The same chain, one row and one tap at a time in Python floats (one column, one kernel)."""
    m, L = len(v), len(k)
    out = np.empty(m)
    for i in range(m):
        acc = 0.0
        for j in range(L):
            s = i + origin - j
            if ext == ZERO and not 0 <= s < m:
                continue
            s = min(max(s, 0), m - 1)
            t = float(k[j]) * float(v[s])
            acc = acc + t
        out[i] = acc
    return out
