"""The arithmetic of the separable fits (include/nonlin_hip.h: nlh_sep_*), restated in numpy: one IEEE operation per step,
every sum over rows in the one fixed order.  The inner model comes in as two callables of the FULL parameters,
fcn(p) -> residual [m] (model - y) and jac(p) -> Jacobian [m, N]; tests feed it the curve restatement, or arrays the device's
own inner launchers produced (qr_solve and project take plain arrays)."""
import numpy as np

MAX_L = 32
DEAD = 2.0 ** -40


def tables(N, linear):
    """(lin, nl): the ascending full indices of the linear parameters and of the nonlinear unknowns."""
    lin = np.array(sorted(int(k) for k in linear), dtype=np.int64)
    nl = np.array([k for k in range(N) if k not in set(lin.tolist())], dtype=np.int64)
    return lin, nl


def rowsum(a, b, r=-1):
    """sum over the rows i > r of a_i*b_i: 256 partials, partial j = +0.0 and then s = s + a*b over the rows i = j (mod 256)
    in ascending i; combined as a 256-thread block sum: the tree 32, 16, .., 1 inside each 64, then the four in order."""
    m = len(a)
    part = np.zeros(256)
    for i0 in range(0, m, 256):
        idx = np.arange(i0, min(i0 + 256, m))
        on = idx > r
        j = idx[on] - i0
        part[j] = part[j] + a[idx[on]] * b[idx[on]]
    p = part.reshape(4, 64).copy()
    off = 32
    while off:
        p[:, :off] = p[:, :off] + p[:, off:2 * off]
        off >>= 1
    t = 0.0
    for w in range(4):
        t = t + p[w, 0]
    return t


def apply(v, r, tau, x):
    """The reflector (v, tau) at row position r on the column x, in place."""
    s = x[r] + rowsum(v, x, r)
    s = tau * s
    x[r] = x[r] - s
    x[r + 1:] = x[r + 1:] - s * v[r + 1:]


def qr_solve(Phi, f0):
    """Unpivoted Householder QR of Phi [m, L] applied to f0, dead columns skipped, back-substitution on the live ones.
    Returns (c [L], rank, V [m, L], tau [L], rpos [L]): column l of V holds the reflector of column l below its row position
    rpos[l] (-1 and tau 0.0: dead)."""
    W = np.array(Phi, dtype=np.float64, order="F", copy=True)
    f = np.array(f0, dtype=np.float64, copy=True)
    m, L = W.shape
    norm0 = [np.sqrt(rowsum(W[:, l], W[:, l])) for l in range(L)]
    tau, rpos = np.zeros(L), np.full(L, -1, dtype=np.int64)
    Rm = np.zeros((L, L + 1))
    r = 0
    for l in range(L):
        w = W[:, l]
        sigma = rowsum(w, w, r)
        wr = w[r]
        norm = np.sqrt(wr * wr + sigma)
        if norm <= DEAD * norm0[l]:
            continue
        beta = -np.copysign(norm, wr)
        d = wr - beta
        tau[l] = (beta - wr) / beta
        w[r + 1:] = w[r + 1:] / d
        rpos[l] = r
        Rm[r, l] = beta
        for k in range(l + 1, L + 1):
            x = W[:, k] if k < L else f
            apply(w, r, tau[l], x)
            Rm[r, k] = x[r]
        r += 1
    c = np.zeros(L)
    for j in range(L - 1, -1, -1):
        if rpos[j] < 0:
            continue
        rj = rpos[j]
        s = -Rm[rj, L]
        for k in range(j + 1, L):
            if rpos[k] >= 0:
                s = s - Rm[rj, k] * c[k]
        c[j] = s / Rm[rj, j]
    return c, r, W, tau, rpos


def project(V, tau, rpos, D):
    """Kaufman's projection of the columns of D [m, n]: the live reflectors in order, the leading rank entries to +0.0, the
    reflectors in reverse."""
    X = np.array(D, dtype=np.float64, order="F", copy=True)
    live = [l for l in range(len(tau)) if rpos[l] >= 0]
    for k in range(X.shape[1]):
        x = X[:, k]
        for l in live:
            apply(V[:, l], rpos[l], tau[l], x)
        x[:len(live)] = 0.0
        for l in reversed(live):
            apply(V[:, l], rpos[l], tau[l], x)
    return X


def expand(N, lin, nl, c, alpha):
    p = np.zeros(N)
    p[lin] = c
    p[nl] = alpha
    return p


def solve(fcn, jac, N, linear, alpha):
    """(p^ [N], rank, qr): basis at p0 = (+0.0, alpha), QR and solve."""
    lin, nl = tables(N, linear)
    p0 = expand(N, lin, nl, 0.0, alpha)
    Phi = np.asarray(jac(p0))[:, lin]
    f0 = np.asarray(fcn(p0))
    c, rank, V, tau, rpos = qr_solve(Phi, f0)
    return expand(N, lin, nl, c, alpha), rank, (V, tau, rpos)


def residual(fcn, jac, N, linear, alpha):
    """What nlh_sep_device_fcn writes: the inner residual at p^."""
    return np.asarray(fcn(solve(fcn, jac, N, linear, alpha)[0]))


def jacobian(fcn, jac, N, linear, alpha):
    """What nlh_sep_device_jac writes, as [m, n]."""
    lin, nl = tables(N, linear)
    ph, _, (V, tau, rpos) = solve(fcn, jac, N, linear, alpha)
    return project(V, tau, rpos, np.asarray(jac(ph))[:, nl])
