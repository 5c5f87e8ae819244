"""Plain-Python restatement of the batched polynomial root finder of nonlin_amd/csrc/nlh_kernels_polyroots.h
(polynomial%roots, src/nonlin_polynomials.f90:357-381: eigenvalues of the companion matrix of :346-353), of the batched
Horner evaluation (:283-286 real, :317-320 complex) and of the polynomial arithmetic of :454-779, one statement per
statement of the product, IEEE double arithmetic, left to right, no fused operations.  It is what the GPU tests compare
the kernels against bit for bit.  Test infrastructure, not part of the product.

The root finder, step by step (matrices are 1-based here as in LAPACK; h[r][c], row 0 and column 0 unused):

  1. companion column c(i) = -a(i) / a(n+1), i = 1..n (:351), ones on the subdiagonal (:352).
  2. DGEBAL('B').  Permutation: on a companion matrix the only row that can be isolated is row 1 (c(1) == 0: a zero
     constant coefficient), after which the same holds for the trailing companion matrix of p(x) / x, and no column can
     be isolated once c(kz+1) != 0.  DGEBAL moves such a row by a transposition, which leaves a full first column that
     DGEEV's DGEHRD then has to reduce; here it is moved by the cyclic shift instead, which leaves the trailing
     (n - kz) x (n - kz) companion matrix as the active window [1, n - kz], already upper Hessenberg, and the isolated
     diagonal entries (exact zeros) at positions n - kz + 1 .. n, where DGEEV reports them too.  Scaling: the loop of
     DGEBAL with the one-norm column / row sums of LAPACK up to 3.5.0 (later releases sum squares through DNRM2, whose
     scaled accumulation is not a statement of fixed order), radix 2, factor 0.95: exact in floating point.
  3. DLAHQR (LAPACK 3.x before 3.10: exceptional shifts at its == 10 and its == 20 counted per deflation), WANTT = WANTZ =
     .false., the Ahues-Tisseur deflation test, DLARFG with the classic scaled DNRM2 / DLAPY2 written out, DLANV2 (without
     the 3.7 overflow rescaling: the window is balanced) for every trailing 2 x 2 block.  Sweeps are limited to
     30 * max(10, nh) IN TOTAL for one polynomial.
  4. WR / WI order; on the sweep limit rows 1..i are NaN, info = 106.

info: 0; 106 (NL_CONVERGENCE_ERROR); 210 (NL_DIVIDE_BY_ZERO_ERROR: a(n+1) == 0); 201 (NL_INVALID_INPUT_ERROR: a
coefficient, or a quotient -a(i)/a(n+1), that is not finite).
"""
import math

EPS = 2.220446049250313e-16           # DLAMCH('P') = epsilon(1d0)
SAFMIN = 2.2250738585072014e-308      # DLAMCH('S')
NAN = math.nan

NL_INVALID_INPUT_ERROR = 201
NL_CONVERGENCE_ERROR = 106
NL_DIVIDE_BY_ZERO_ERROR = 210


def _sign(a, b):
    """Fortran SIGN(a, b)."""
    return math.copysign(abs(a), b)


def dlapy2(x, y):
    """DLAPY2 without its NaN branch (no NaN reaches it)."""
    xabs = abs(x)
    yabs = abs(y)
    w = max(xabs, yabs)
    z = min(xabs, yabs)
    if z == 0.0:
        return w
    q = z / w
    return w * math.sqrt(1.0 + q * q)


def dnrm2_2(nx, x1, x2):
    """DNRM2 of the reference BLAS (scaled sum of squares) for the nx = 1 or 2 entries a 3-row reflector has."""
    if nx == 1:
        return abs(x1)
    scale = 0.0
    ssq = 1.0
    for x in (x1, x2):
        if x != 0.0:
            absxi = abs(x)
            if scale < absxi:
                q = scale / absxi
                ssq = 1.0 + ssq * (q * q)
                scale = absxi
            else:
                q = absxi / scale
                ssq = ssq + q * q
    return scale * math.sqrt(ssq)


RF_SAFMIN = SAFMIN / (EPS * 0.5)      # DLARFG: DLAMCH('S') / DLAMCH('E')
RF_RSAFMN = 1.0 / RF_SAFMIN


def dlarfg(nr, alpha, x1, x2):
    """DLARFG for nr = 2 or 3: returns (beta, v2, v3, tau)."""
    xnorm = dnrm2_2(nr - 1, x1, x2)
    if xnorm == 0.0:
        return alpha, x1, x2, 0.0
    beta = -_sign(dlapy2(alpha, xnorm), alpha)
    knt = 0
    if abs(beta) < RF_SAFMIN:
        while True:
            knt += 1
            x1 = x1 * RF_RSAFMN
            x2 = x2 * RF_RSAFMN
            beta = beta * RF_RSAFMN
            alpha = alpha * RF_RSAFMN
            if not (abs(beta) < RF_SAFMIN and knt < 20):
                break
        xnorm = dnrm2_2(nr - 1, x1, x2)
        beta = -_sign(dlapy2(alpha, xnorm), alpha)
    tau = (beta - alpha) / beta
    sc = 1.0 / (alpha - beta)
    x1 = x1 * sc
    x2 = x2 * sc
    for _ in range(knt):
        beta = beta * RF_SAFMIN
    return beta, x1, x2, tau


def dlanv2(a, b, c, d):
    """DLANV2, eigenvalues only: (rt1r, rt1i, rt2r, rt2i)."""
    if c == 0.0:
        pass
    elif b == 0.0:
        temp = d
        d = a
        a = temp
        b = -c
        c = 0.0
    elif (a - d) == 0.0 and math.copysign(1.0, b) != math.copysign(1.0, c):
        pass
    else:
        temp = a - d
        p = 0.5 * temp
        bcmax = max(abs(b), abs(c))
        bcmis = min(abs(b), abs(c)) * math.copysign(1.0, b) * math.copysign(1.0, c)
        scale = max(abs(p), bcmax)
        z = (p / scale) * p + (bcmax / scale) * bcmis
        if z >= 4.0 * EPS:
            z = p + _sign(math.sqrt(scale) * math.sqrt(z), p)
            a = d + z
            d = d - (bcmax / z) * bcmis
            b = b - c
            c = 0.0
        else:
            sigma = b + c
            tau = dlapy2(sigma, temp)
            cs = math.sqrt(0.5 * (1.0 + abs(sigma) / tau))
            sn = -(p / (tau * cs)) * math.copysign(1.0, sigma)
            aa = a * cs + b * sn
            bb = -a * sn + b * cs
            cc = c * cs + d * sn
            dd = -c * sn + d * cs
            a = aa * cs + cc * sn
            b = bb * cs + dd * sn
            c = -aa * sn + cc * cs
            d = -bb * sn + dd * cs
            temp = 0.5 * (a + d)
            a = temp
            d = temp
            if c != 0.0:
                if b != 0.0:
                    if math.copysign(1.0, b) == math.copysign(1.0, c):
                        sab = math.sqrt(abs(b))
                        sac = math.sqrt(abs(c))
                        p = _sign(sab * sac, c)
                        a = temp + p
                        d = temp - p
                        b = b - c
                        c = 0.0
                else:
                    b = -c
                    c = 0.0
    rt1r = a
    rt2r = d
    if c == 0.0:
        rt1i = 0.0
        rt2i = 0.0
    else:
        rt1i = math.sqrt(abs(b)) * math.sqrt(abs(c))
        rt2i = -rt1i
    return rt1r, rt1i, rt2r, rt2i


BAL_SFMIN1 = SAFMIN / EPS
BAL_SFMAX1 = 1.0 / BAL_SFMIN1
BAL_SFMIN2 = BAL_SFMIN1 * 2.0
BAL_SFMAX2 = 1.0 / BAL_SFMIN2


def balance_scale(h, m):
    """The scaling loop of DGEBAL on the active window [1, m] (k = 1, l = m = n of the window)."""
    scale = [1.0] * (m + 1)
    while True:
        noconv = False
        for i in range(1, m + 1):
            c = 0.0
            r = 0.0
            ca = 0.0
            ra = 0.0
            for j in range(1, m + 1):
                if j != i:
                    c = c + abs(h[j][i])
                    r = r + abs(h[i][j])
                ca = max(ca, abs(h[j][i]))                    # |a(idamax column i)|
                ra = max(ra, abs(h[i][j]))                    # |a(idamax row i)|
            if c == 0.0 or r == 0.0:
                continue
            g = r / 2.0
            f = 1.0
            s = c + r
            while not (c >= g or max(f, c, ca) >= BAL_SFMAX2 or min(r, g, ra) <= BAL_SFMIN2):
                f = f * 2.0
                c = c * 2.0
                ca = ca * 2.0
                r = r / 2.0
                g = g / 2.0
                ra = ra / 2.0
            g = c / 2.0
            while not (g < r or max(r, ra) >= BAL_SFMAX2 or min(f, c, g, ca) <= BAL_SFMIN2):
                f = f / 2.0
                c = c / 2.0
                g = g / 2.0
                ca = ca / 2.0
                r = r * 2.0
                ra = ra * 2.0
            if (c + r) >= 0.95 * s:
                continue
            if f < 1.0 and scale[i] < 1.0:
                if f * scale[i] <= BAL_SFMIN1:
                    continue
            if f > 1.0 and scale[i] > 1.0:
                if scale[i] >= BAL_SFMAX1 / f:
                    continue
            g = 1.0 / f
            scale[i] = scale[i] * f
            noconv = True
            for j in range(1, m + 1):
                h[i][j] = h[i][j] * g
            for j in range(1, m + 1):
                h[j][i] = h[j][i] * f
        if not noconv:
            break
    return scale


def dlahqr(h, nh, wr, wi):
    """DLAHQR on the window [1, nh] of h, eigenvalues only.  Returns (info, sweeps): info = 0, or i where rows 1..i are
    not converged."""
    if nh == 1:
        wr[1] = h[1][1]
        wi[1] = 0.0
        return 0, 0
    ulp = EPS
    smlnum = SAFMIN * (float(nh) / ulp)
    itmax = 30 * max(10, nh)
    sweeps = 0
    i = nh
    while i >= 1:
        l = 1
        its = 0
        while True:
            k = i
            while k > l:                                              # a small subdiagonal element
                hkk1 = abs(h[k][k - 1])
                if hkk1 <= smlnum:
                    break
                tst = abs(h[k - 1][k - 1]) + abs(h[k][k])
                if tst == 0.0:
                    if k - 2 >= 1:
                        tst = tst + abs(h[k - 1][k - 2])
                    if k + 1 <= nh:
                        tst = tst + abs(h[k + 1][k])
                if hkk1 <= ulp * tst:                                 # Ahues & Tisseur
                    hk1k = abs(h[k - 1][k])
                    ab = max(hkk1, hk1k)
                    ba = min(hkk1, hk1k)
                    dkk = abs(h[k][k])
                    ddf = abs(h[k - 1][k - 1] - h[k][k])
                    aa = max(dkk, ddf)
                    bb = min(dkk, ddf)
                    s = aa + ab
                    if ba * (ab / s) <= max(smlnum, ulp * (bb * (aa / s))):
                        break
                k -= 1
            l = k
            if l > 1:
                h[l][l - 1] = 0.0
            if l >= i - 1:
                break
            if sweeps >= itmax:
                return i, sweeps
            sweeps += 1
            if its == 10:                                             # exceptional shift
                s = abs(h[l + 1][l]) + abs(h[l + 2][l + 1])
                h11 = 0.75 * s + h[l][l]
                h12 = -0.4375 * s
                h21 = s
                h22 = h11
            elif its == 20:
                s = abs(h[i][i - 1]) + abs(h[i - 1][i - 2])
                h11 = 0.75 * s + h[i][i]
                h12 = -0.4375 * s
                h21 = s
                h22 = h11
            else:
                h11 = h[i - 1][i - 1]
                h21 = h[i][i - 1]
                h12 = h[i - 1][i]
                h22 = h[i][i]
            s = abs(h11) + abs(h12) + abs(h21) + abs(h22)
            if s == 0.0:
                rt1r = 0.0
                rt1i = 0.0
                rt2r = 0.0
                rt2i = 0.0
            else:
                h11 = h11 / s
                h21 = h21 / s
                h12 = h12 / s
                h22 = h22 / s
                tr = (h11 + h22) / 2.0
                det = (h11 - tr) * (h22 - tr) - h12 * h21
                rtdisc = math.sqrt(abs(det))
                if det >= 0.0:
                    rt1r = tr * s
                    rt2r = rt1r
                    rt1i = rtdisc * s
                    rt2i = -rt1i
                else:
                    rt1r = tr + rtdisc
                    rt2r = tr - rtdisc
                    if abs(rt1r - h22) <= abs(rt2r - h22):
                        rt1r = rt1r * s
                        rt2r = rt1r
                    else:
                        rt2r = rt2r * s
                        rt1r = rt2r
                    rt1i = 0.0
                    rt2i = 0.0
            m = i - 2
            while True:                                               # two consecutive small subdiagonal elements
                hmm = h[m][m]
                h21s = abs(h[m + 1][m])
                s = abs(hmm - rt2r) + abs(rt2i) + h21s
                h21s = h[m + 1][m] / s
                v1 = h21s * h[m][m + 1] + (hmm - rt1r) * ((hmm - rt2r) / s) - rt1i * (rt2i / s)
                v2 = h21s * (hmm + h[m + 1][m + 1] - rt1r - rt2r)
                v3 = h21s * h[m + 2][m + 1]
                s = abs(v1) + abs(v2) + abs(v3)
                v1 = _ieee_div(v1, s)
                v2 = _ieee_div(v2, s)
                v3 = _ieee_div(v3, s)
                if m == l:
                    break
                if abs(h[m][m - 1]) * (abs(v2) + abs(v3)) <= \
                        ulp * abs(v1) * (abs(h[m - 1][m - 1]) + abs(hmm) + abs(h[m + 1][m + 1])):
                    break
                m -= 1
            for k in range(m, i):                                     # the double-shift QR step
                nr = min(3, i - k + 1)
                if k > m:
                    v1 = h[k][k - 1]
                    v2 = h[k + 1][k - 1]
                    v3 = h[k + 2][k - 1] if nr == 3 else 0.0
                v1, v2, v3, t1 = dlarfg(nr, v1, v2, v3)
                if k > m:
                    h[k][k - 1] = v1
                    h[k + 1][k - 1] = 0.0
                    if k < i - 1:
                        h[k + 2][k - 1] = 0.0
                elif m > l:
                    h[k][k - 1] = h[k][k - 1] * (1.0 - t1)
                t2 = t1 * v2
                if nr == 3:
                    t3 = t1 * v3
                    for j in range(k, i + 1):
                        sm = h[k][j] + v2 * h[k + 1][j] + v3 * h[k + 2][j]
                        h[k][j] = h[k][j] - sm * t1
                        h[k + 1][j] = h[k + 1][j] - sm * t2
                        h[k + 2][j] = h[k + 2][j] - sm * t3
                    for j in range(l, min(k + 3, i) + 1):
                        sm = h[j][k] + v2 * h[j][k + 1] + v3 * h[j][k + 2]
                        h[j][k] = h[j][k] - sm * t1
                        h[j][k + 1] = h[j][k + 1] - sm * t2
                        h[j][k + 2] = h[j][k + 2] - sm * t3
                else:
                    for j in range(k, i + 1):
                        sm = h[k][j] + v2 * h[k + 1][j]
                        h[k][j] = h[k][j] - sm * t1
                        h[k + 1][j] = h[k + 1][j] - sm * t2
                    for j in range(l, i + 1):
                        sm = h[j][k] + v2 * h[j][k + 1]
                        h[j][k] = h[j][k] - sm * t1
                        h[j][k + 1] = h[j][k + 1] - sm * t2
            its += 1
        if l == i:
            wr[i] = h[i][i]
            wi[i] = 0.0
        else:
            wr[i - 1], wi[i - 1], wr[i], wi[i] = dlanv2(h[i - 1][i - 1], h[i - 1][i], h[i][i - 1], h[i][i])
        i = l - 1
    return 0, sweeps


def _ieee_div(a, b):
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def poly_roots(coef, balance=True, stats=None):
    """coef: a(1..n+1), constant first.  Returns (roots as a list of n (re, im) pairs, info)."""
    n = len(coef) - 1
    if n <= 0:
        return [], 0
    bad = [(NAN, NAN)] * n
    for a in coef:
        if a != a or a in (math.inf, -math.inf):
            return bad, NL_INVALID_INPUT_ERROR
    lead = coef[n]
    if lead == 0.0:
        return bad, NL_DIVIDE_BY_ZERO_ERROR
    c = [0.0] * (n + 1)
    for i in range(1, n + 1):
        c[i] = -coef[i - 1] / lead                                    # :351
        if c[i] in (math.inf, -math.inf):
            return bad, NL_INVALID_INPUT_ERROR
    kz = 0                                                            # DGEBAL's isolated rows: see the module docstring
    while kz < n - 1 and c[kz + 1] == 0.0:
        kz += 1
    m = n - kz
    wr = [NAN] * (n + 1)
    wi = [NAN] * (n + 1)
    for i in range(m + 1, n + 1):
        wr[i] = 0.0                                                   # the isolated diagonal entries
        wi[i] = 0.0
    h = [[0.0] * (m + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        h[i][m] = c[kz + i]
        if i < m:
            h[i + 1][i] = 1.0                                         # :352
    if balance and m > 1:
        balance_scale(h, m)
    info, sweeps = dlahqr(h, m, wr, wi)
    if stats is not None:
        stats["sweeps"] = sweeps
        stats["itmax"] = 30 * max(10, m)
    if info:
        for i in range(1, info + 1):
            wr[i] = NAN
            wi[i] = NAN
    return [(wr[i], wi[i]) for i in range(1, n + 1)], (NL_CONVERGENCE_ERROR if info else 0)


# ---------------------------------------------------------------------------------------------------------------------
# Horner evaluation
# ---------------------------------------------------------------------------------------------------------------------
def poly_eval(coef, x):
    """:272-286, real x."""
    order = len(coef) - 1
    if order == -1:
        return 0.0
    if order == 0:
        return coef[0]
    y = coef[order] * x + coef[order - 1]
    for j in range(order - 2, -1, -1):
        y = y * x + coef[j]
    return y


def poly_eval_complex(coef, xr, xi):
    """:306-320, complex x = (xr, xi): y * x is the four-multiply form, the real coefficient joins the real part only."""
    order = len(coef) - 1
    if order == -1:
        return 0.0, 0.0
    if order == 0:
        return coef[0], 0.0
    yr = coef[order] * xr + coef[order - 1]
    yi = coef[order] * xi
    for j in range(order - 2, -1, -1):
        tr = yr * xr - yi * xi
        ti = yr * xi + yi * xr
        yr = tr + coef[j]
        yi = ti
    return yr, yi


# ---------------------------------------------------------------------------------------------------------------------
# arithmetic (coefficient lists, constant first; None: an uninitialised polynomial, order -1)
# ---------------------------------------------------------------------------------------------------------------------
def _order(x):
    return -1 if x is None else len(x) - 1


def poly_add_sub(x, y, sub):
    """poly_poly_add (:501-553) / poly_poly_subtract (:556-608)."""
    x_ord = _order(x)
    y_ord = _order(y)
    max_ord = max(x_ord, y_ord)
    if x_ord == -1 and y_ord == -1:
        return None                                                   # initialize(-1)
    z = [0.0] * (max_ord + 1)
    if x_ord == -1:
        for i in range(max_ord + 1):
            z[i] = y[i]                                               # :523 and, for subtract, :578: +y, not -y
        return z
    if y_ord == -1:
        for i in range(max_ord + 1):
            z[i] = x[i]
        return z
    if x_ord > y_ord:
        for i in range(1, y_ord + 2):
            z[i - 1] = x[i - 1] - y[i - 1] if sub else x[i - 1] + y[i - 1]
        for i in range(y_ord + 2, x_ord + 1):                         # :538 / :593: stops at x_ord, z(x_ord + 1) stays 0
            z[i - 1] = x[i - 1]
    elif x_ord < y_ord:
        for i in range(1, x_ord + 2):
            z[i - 1] = x[i - 1] - y[i - 1] if sub else x[i - 1] + y[i - 1]
        for i in range(x_ord + 2, y_ord + 2):
            z[i - 1] = -y[i - 1] if sub else y[i - 1]
    else:
        for i in range(1, max_ord + 2):
            z[i - 1] = x[i - 1] - y[i - 1] if sub else x[i - 1] + y[i - 1]
    return z


def poly_mult(x, y):
    """poly_poly_mult (:611-636)."""
    n = len(x)
    m = len(y)
    z = [0.0] * (n + m - 1)
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            z[i + j - 2] = z[i + j - 2] + x[i - 1] * y[j - 1]
    return z


def poly_scale(x, s):
    """poly_dbl_mult / dbl_poly_mult (:639-678)."""
    return [xi * s for xi in x]


def poly_divide(num, den):
    """poly_divide (:681-779): (quotient, remainder); raises ZeroDivisionError where the reference stops with
    NL_DIVIDE_BY_ZERO_ERROR."""
    lead = den[-1]
    if abs(lead) <= EPS:
        raise ZeroDivisionError(NL_DIVIDE_BY_ZERO_ERROR)
    n = len(num) - 1
    m = len(den) - 1
    if n < m:
        return [0.0], list(num)
    q = [0.0] * (n - m + 1)
    r = list(num)
    for i in range(n - m, -1, -1):
        coeff = r[i + m] / lead
        q[i] = coeff
        for j in range(1, m + 2):
            r[i + j - 1] = r[i + j - 1] - coeff * den[j - 1]

    def trim(v):
        last = 0
        for i in range(len(v), 0, -1):
            if abs(v[i - 1]) > EPS:
                last = i
                break
        return [0.0] if last == 0 else v[:last]
    return trim(q), trim(r)
