"""The nonlinear stage of curve_guess (include/nonlin_hip_guess.h: nlh_curve_guess_batch), restated in numpy: one IEEE operation per
step, every sum in the one order the header states.  The regression of the decays is sep_restatement.qr_solve, the routine
the device drives on the same panel.  The linear stage is nlh_sep_solve_batch and has its own restatement (sep_restatement);
linear_numpy below is a plain numpy least-squares stand-in for the CPU studies.  Test infrastructure, not part of the
product."""
import numpy as np

import curve_restatement as R
import sep_restatement as S

MAX_M = 8192
FALLBACK, RANKDEF, NONE = 1, 2, 4
FWHM_PER_SIGMA = 2.3548200450309493


def nnonlin(kind, K):
    return K if kind == R.EXPDECAY else 2 * K


def compact(t, y, w):
    """(t', y') over the rows with w != 0, ascending."""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if w is None:
        return t.copy(), y.copy()
    on = np.asarray(w) != 0
    return t[on], y[on]


def usable(n, tv, yv):
    """Not NLH_GUESS_NONE: at least n valid rows, all finite, t' strictly ascending."""
    return bool(len(tv) >= n and np.isfinite(tv).all() and np.isfinite(yv).all() and (np.diff(tv) > 0).all())


def seqmean(a):
    """s = +0.0; s = s + a_i ascending; s / count."""
    s = 0.0
    for v in a:
        s = s + v
    return s / float(len(a))


def detrend(B, tv, yv):
    mv = len(tv)
    if B < 0:
        return yv.copy()
    E = max(1, mv // 16)
    yl, yr = seqmean(yv[:E]), seqmean(yv[mv - E:])
    if B == 0:
        return yv - 0.5 * (yl + yr)
    tl, tr = seqmean(tv[:E]), seqmean(tv[mv - E:])
    c1 = (yr - yl) / (tr - tl)
    c0 = yl - c1 * tl
    return yv - (c0 + c1 * tv)


def smooth(d, h):
    """s_i = (+0.0, then + d_j for j = max(0, i-h) .. min(mv-1, i+h) ascending) / count; h = 0: d itself."""
    if h == 0:
        return d.copy()
    mv = len(d)
    i = np.arange(mv)
    acc = np.zeros(mv)
    cnt = np.zeros(mv)
    for off in range(-h, h + 1):
        j = i + off
        on = (j >= 0) & (j < mv)
        acc[on] = acc[on] + d[j[on]]
        cnt[on] += 1.0
    return acc / cnt


def peaks(kind, K, B, tv, yv, h):
    """(alpha = (mu_0, width_0, mu_1, ..), flag) of K peaks on the valid rows."""
    mv = len(tv)
    s = smooth(detrend(B, tv, yv), h)
    dead = np.zeros(mv, dtype=bool)
    span = tv[mv - 1] - tv[0]
    out, flag = [], 0
    for _ in range(K):
        key = np.where(dead | np.isnan(s), -np.inf, s)
        ist = int(np.argmax(key))                                   # the lowest index wins ties
        a = key[ist]
        half = 0.5 * a
        mu = tv[ist]
        F = np.nan
        if a > 0.0:
            hit = dead | (s < half)
            jr = next((j for j in range(ist + 1, mv) if hit[j]), mv)
            jl = next((j for j in range(ist - 1, -1, -1) if hit[j]), -1)
            tR = tL = None
            if jr < mv and not dead[jr]:
                tR = tv[jr - 1] + ((tv[jr] - tv[jr - 1]) * (s[jr - 1] - half)) / (s[jr - 1] - s[jr])
            if jl >= 0 and not dead[jl]:
                tL = tv[jl + 1] - ((tv[jl + 1] - tv[jl]) * (s[jl + 1] - half)) / (s[jl + 1] - s[jl])
            if tR is not None and tL is not None:
                F = tR - tL
            elif tR is not None:
                F = 2.0 * (tR - mu)
            elif tL is not None:
                F = 2.0 * (mu - tL)
        if not (F > 0.0 and np.isfinite(F)):
            F = 0.5 * span
            flag |= FALLBACK
        if kind == R.GAUSS:
            out += [mu, F / FWHM_PER_SIGMA]
            dead = dead | (np.abs(tv - mu) <= 1.5 * F)
        else:
            wd = 0.5 * F
            out += [mu, wd]
            dd = (tv - mu) / wd
            s = s - a / (1.0 + dd * dd)
            dead[ist] = True
    return np.array(out), flag


def trapezoid(v, tv):
    """q_0 = +0.0; q_i = (0.5*(v_i + v_{i-1}))*(t_i - t_{i-1})."""
    q = np.zeros(len(v))
    q[1:] = (0.5 * (v[1:] + v[:-1])) * (tv[1:] - tv[:-1])
    return q


def blocked_prefix(q):
    """The inclusive prefix sum in the stated order: c = ceil(mv/256) rows per chunk, sequential from +0.0 inside a chunk,
    the chunk totals combined sequentially from +0.0, S_i = o_j + l_i."""
    mv = len(q)
    c = (mv + 255) // 256
    nch = (mv + c - 1) // c
    loc = np.zeros(mv)
    run = np.zeros(nch)
    first = np.arange(nch) * c
    for step in range(c):
        idx = first + step
        on = idx < mv
        run[on] = run[on] + q[idx[on]]
        loc[idx[on]] = run[on]
    off = np.zeros(nch)
    for j in range(1, nch):
        off[j] = off[j - 1] + run[j - 1]
    return np.repeat(off, c)[:mv] + loc


def decay_panel(K, B, tv, yv, m):
    """(Phi [m, 2K + B + 1], f0 [m]): the columns S1, (S2), u^0 .. u^(K+B); rows >= mv are +0.0."""
    mv = len(tv)
    S1 = blocked_prefix(trapezoid(yv, tv))
    cols = [S1]
    if K == 2:
        cols.append(blocked_prefix(trapezoid(S1, tv)))
    u = tv - tv[0]
    p = np.ones(mv)
    for _ in range(K + B + 1):
        cols.append(p)
        p = p * u
    Phi = np.zeros((m, len(cols)))
    Phi[:mv] = np.stack(cols, axis=1)
    f0 = np.zeros(m)
    f0[:mv] = -yv
    return Phi, f0


def rates(K, c, dead_column, span):
    """(k [K], flag) from the regression's coefficients."""
    if K == 1:
        k = np.array([-c[0]])
        fb = np.array([2.0 / span])
    else:
        A, Bc = c[0], c[1]
        disc = A * A + 4.0 * Bc
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.sqrt(disc)
            k1 = 0.5 * (r - A)
            k2 = (-Bc) / k1
        k = np.array([k1, k2])
        fb = np.array([8.0 / span, 1.0 / span])
    if dead_column or not (np.isfinite(k).all() and (k > 0.0).all()):
        return fb, FALLBACK
    return k, 0


def decays(K, B, tv, yv, m, qr_solve=S.qr_solve):
    Phi, f0 = decay_panel(K, B, tv, yv, m)
    c, rank, _, _, _ = qr_solve(Phi, f0)
    return rates(K, c, rank < Phi.shape[1], tv[len(tv) - 1] - tv[0])


def nonlinear(kind, K, B, t, y, w=None, h=2, qr_solve=S.qr_solve):
    """One problem: (alpha [nnonlin], flag).  NLH_GUESS_NONE: alpha is NaN."""
    n = R.nparams(kind, K, B)
    tv, yv = compact(t, y, w)
    if not usable(n, tv, yv):
        return np.full(nnonlin(kind, K), np.nan), NONE
    if kind == R.EXPDECAY:
        return decays(K, B, tv, yv, len(np.asarray(y)), qr_solve)
    return peaks(kind, K, B, tv, yv, h)


def lin_positions(kind, K, B):
    per = R.nper(kind)
    n = R.nparams(kind, K, B)
    lin = [per * c for c in range(K)] + list(range(per * K, n))
    return np.array(lin), np.array([k for k in range(n) if k not in lin])


def linear_numpy(kind, K, B, alpha, t, y, w=None):
    """The best linear fit at alpha by numpy's least squares (the studies' stand-in for the device's stated QR)."""
    lin, nl = lin_positions(kind, K, B)
    p0 = np.zeros(R.nparams(kind, K, B))
    p0[nl] = alpha
    Phi = R.jacobian(kind, K, B, p0, t, w)[:, lin]
    f0 = R.residual(kind, K, B, p0, t, y, w)
    p0[lin] = np.linalg.lstsq(Phi, -f0, rcond=None)[0]
    return p0


def guess(kind, K, B, t, y, w=None, h=2):
    """(x0 [n], flag) of one problem, the linear stage by linear_numpy."""
    alpha, flag = nonlinear(kind, K, B, t, y, w, h)
    if flag & NONE:
        return np.full(R.nparams(kind, K, B), np.nan), flag
    return linear_numpy(kind, K, B, alpha, t, y, w), flag
