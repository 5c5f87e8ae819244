"""Plain-Python restatement of brent_solver%solve (brent_solve, src/nonlin_solve.f90:643-835), newton_1var_solver%solve
(newt1var_solve, :840-1032) and fcn1var_helper%diff (f1h_diff_fcn, src/nonlin_single_var.f90:154-200), one statement
per reference statement, IEEE double arithmetic in the reference's order (left to right, no fused operations).  It is
what the GPU tests compare the device state machine against bit for bit.  Test infrastructure, not part of the product.

fcn(x, args) -> float, diff(x, args) -> float (None: forward differences).  Every solve returns a dict: x, f, the seven
iteration_behavior fields, status (0, 106 or 201), status_lines (the print_status blocks, as (iter, neval, njac, xnorm,
fnorm)), points (every point fcn was evaluated at, in order: forward-difference points included), dpoints (every
point diff was called at) and exit (the statement that ended the solve: brent "fcn" :745, "xm" :750, "max_evals" :813;
newton "endpoint" :906-923, "bisection" :953, "newton_step" :964, "fcn" :978, "dx" :982, "diff" :986, "max_evals"
:1004; both "invalid").
"""
import math

from nm_restatement import format_e10_3

EPS = 2.220446049250313e-16          # epsilon(1d0)
SQRT_EPS = math.sqrt(EPS)            # 1.4901161193847656e-08, exact


def _div(a, b):
    """a / b with IEEE semantics (Python raises on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
    return -math.inf if neg else math.inf


def f1h_diff(fcn, x, f=None, diff=None, args=None, points=None):
    """f1h_diff_fcn (:154-200).  points: list the evaluation points are appended to (the forward-difference point is not
    counted by the solvers)."""
    epsmch = EPS                                              # :180
    eps = SQRT_EPS                                            # :181
    if diff is not None:                                      # :184
        return float(diff(x, args))                           # :186
    h = eps * abs(x)                                          # :189
    if h < epsmch:                                            # :190
        h = eps
    temp = x + h                                              # :191
    if points is not None:
        points.append(temp)
    f1 = float(fcn(temp, args))                               # :192
    if f is not None:                                         # :193-197
        f0 = f
    else:
        if points is not None:
            points.append(x)
        f0 = float(fcn(x, args))
    return _div(f1 - f0, h)                                   # :198: divided by h, not by temp - x


def _result(x, f, it, neval, njac, fcnvrg, xcnvrg, dcnvrg, status, lines, points, dpoints, exit_):
    return {"exit": exit_, "x": x, "f": f, "iter_count": it, "fcn_count": neval, "jacobian_count": njac, "gradient_count": 0,
            "converge_on_fcn": bool(fcnvrg), "converge_on_chng": bool(xcnvrg), "converge_on_zero_diff": bool(dcnvrg),
            "status": status, "status_lines": lines, "points": points, "dpoints": dpoints}


def brent_solve(fcn, x1, x2, max_evals=100, ftol=1e-8, xtol=1e-12, args=None):
    """brent_solve with f present.  x = 0 unless the solve converged (:691, :746, :751)."""
    pts, lines = [], []
    fcnvrg = False                                            # :689
    xcnvrg = False                                            # :690
    x = 0.0                                                   # :691
    a = min(x1, x2)                                           # :692
    b = max(x1, x2)                                           # :693
    neval = 0                                                 # :694
    it = 0                                                    # :695
    eps = EPS                                                 # :696
    maxeval = max_evals                                       # :699
    f = 0.0                                                   # :700
    if abs(a - b) < eps:                                      # :713 (absolute epsilon)
        return _result(x, f, it, neval, 0, fcnvrg, xcnvrg, False, 201, lines, pts, [], "invalid")
    c = d = e = 0.0     # read unset on the first pass when fb == 0 exactly (ftol <= 0) or fb is NaN: 0 here and on the device
    flag = 0                                                  # :716
    pts.append(a)
    fa = float(fcn(a, args))                                  # :717
    pts.append(b)
    fb = float(fcn(b, args))                                  # :718
    neval = 2                                                 # :719
    fc = fb                                                   # :720
    while True:
        it = it + 1                                           # :723
        if (fb > 0.0 and fc >= 0.0) or (fb < 0.0 and fc < 0.0):   # :726-727
            c = a                                             # :728
            fc = fa                                           # :729
            d = b - a                                         # :730
            e = d                                             # :731
        if abs(fc) < abs(fb):                                 # :733
            a = b                                             # :734
            b = c                                             # :735
            c = a                                             # :736
            fa = fb                                           # :737
            fb = fc                                           # :738
            fc = fa                                           # :739
        tol1 = 2.0 * eps * abs(b) + 0.5 * xtol                # :743
        xm = 0.5 * (c - b)                                    # :744
        if abs(fb) < ftol:                                    # :745
            x = b                                             # :746
            fcnvrg = True
            exit_ = "fcn"
            break
        if abs(xm) <= tol1:                                   # :750
            x = b                                             # :751
            xcnvrg = True
            exit_ = "xm"
            break
        if abs(e) >= tol1 and abs(fa) > abs(fb):              # :757
            s = _div(fb, fa)                                  # :760
            if abs(a - c) < eps:                              # :761 (a == c)
                p = 2.0 * xm * s                              # :762
                q = 1.0 - s                                   # :763
            else:
                q = _div(fa, fc)                              # :765
                r = _div(fb, fc)                              # :766
                p = s * (2.0 * xm * q * (q - r) - (b - a) * (r - 1.0))   # :767
                q = (q - 1.0) * (r - 1.0) * (s - 1.0)         # :768
            if p > 0.0:                                       # :772
                q = -q
            p = abs(p)                                        # :773
            mn1 = 3.0 * xm * q - abs(tol1 * q)                # :774
            mn2 = abs(e * q)                                  # :775
            if mn1 < mn2:                                     # :776-780
                temp = mn1
            else:
                temp = mn2
            if 2.0 * p < temp:                                # :781
                e = d                                         # :783
                d = _div(p, q)                                # :784
            else:
                d = xm                                        # :787
                e = d                                         # :788
        else:
            d = xm                                            # :792
            e = d                                             # :793
        a = b                                                 # :797
        fa = fb                                               # :798
        if abs(d) > tol1:                                     # :799
            b = b + d                                         # :800
        else:
            b = b + math.copysign(tol1, xm)                   # :802: sign(tol1, xm), a negative zero included
        pts.append(b)
        fb = float(fcn(b, args))                              # :804
        neval = neval + 1                                     # :805
        lines.append((it, neval, 0, xm, fb))                  # :808-810
        if neval >= maxeval:                                  # :813
            flag = 1
            exit_ = "max_evals"
            break
    f = fb                                                    # :820
    return _result(x, f, it, neval, 0, fcnvrg, xcnvrg, False, 106 if flag else 0, lines, pts, [], exit_)


def newt1var_solve(fcn, x1, x2, diff=None, max_evals=100, ftol=1e-8, xtol=1e-12, dtol=1e-12, args=None, want_f=True,
                   x_in=0.0):
    """newt1var_solve.  want_f: the optional f is present (one more evaluation after the loop, :1011-1014).  x_in: x as it
    came in (left untouched by an invalid bracket)."""
    pts, dpts, lines = [], [], []
    fcnvrg = xcnvrg = dcnvrg = False                          # :873-875
    neval = 0                                                 # :876
    ndiff = 0                                                 # :877
    it = 0                                                    # :878
    maxeval = max_evals                                       # :882
    f = 0.0 if want_f else None                               # :883
    lo = min(x1, x2)                                          # :893
    hi = max(x1, x2)                                          # :894
    eps = EPS                                                 # :895
    x = x_in
    if abs(lo - hi) < eps:                                    # :899
        return _result(x, f, it, neval, ndiff, False, False, False, 201, lines, pts, dpts, "invalid")

    def evaluate(xx):
        pts.append(xx)
        ff = float(fcn(xx, args))
        if diff is not None:
            dpts.append(xx)
        return ff, f1h_diff(fcn, xx, f=ff, diff=diff, args=args, points=pts)

    flag = 0                                                  # :902
    pts.append(lo)
    fl = float(fcn(lo, args))                                 # :903
    pts.append(hi)
    fh = float(fcn(hi, args))                                 # :904
    neval = 2                                                 # :905
    if abs(fl) < ftol:                                        # :906-914
        return _result(lo, fl if want_f else None, 0, 2, 0, True, False, False, 0, lines, pts, dpts, "endpoint")
    if abs(fh) < ftol:                                        # :915-923
        return _result(hi, fh if want_f else None, 0, 2, 0, True, False, False, 0, lines, pts, dpts, "endpoint")
    if fl < 0.0:                                              # :926-932
        xl = lo
        xh = hi
    else:
        xl = hi
        xh = lo
    x = 0.5 * (lo + hi)                                       # :933
    dxold = abs(hi - lo)                                      # :934
    dx = dxold                                                # :935
    ff, df = evaluate(x)                                      # :936-937
    neval = neval + 1                                         # :938
    ndiff = ndiff + 1                                         # :939
    while True:
        it = it + 1                                           # :942
        if (((x - xh) * df - ff) * ((x - xl) * df - ff) > 0.0) or (abs(2.0 * ff) > abs(dxold * df)):   # :946-948
            dxold = dx                                        # :950
            dx = 0.5 * (xh - xl)                              # :951
            x = xl + dx                                       # :952
            if abs(xl - x) < xtol:                            # :953
                xcnvrg = True
                exit_ = "bisection"
                break
        else:
            dxold = dx                                        # :960
            dx = _div(ff, df)                                 # :961
            temp = x                                          # :962
            x = x - dx                                        # :963
            if abs(temp - x) < xtol:                          # :964
                xcnvrg = True
                exit_ = "newton_step"
                break
        ff, df = evaluate(x)                                  # :972-973
        neval = neval + 1                                     # :974
        ndiff = ndiff + 1                                     # :975
        if abs(ff) < ftol:                                    # :978
            fcnvrg = True
            exit_ = "fcn"
            break
        if abs(dx) < xtol:                                    # :982
            xcnvrg = True
            exit_ = "dx"
            break
        if abs(df) < dtol:                                    # :986
            dcnvrg = True
            exit_ = "diff"
            break
        if ff < 0.0:                                          # :992-997
            xl = x
        else:
            xh = x
        lines.append((it, neval, ndiff, dx, ff))              # :999-1001 (only iterations that pass every test)
        if neval >= maxeval:                                  # :1004
            flag = 1
            exit_ = "max_evals"
            break
    if want_f:                                                # :1011-1014
        pts.append(x)
        fcn(x, args)
        neval = neval + 1
        f = ff                                                # :1017: the fresh value is discarded
    return _result(x, f, it, neval, ndiff, fcnvrg, xcnvrg, dcnvrg, 106 if flag else 0, lines, pts, dpts, exit_)


def status_text(result):
    """The print_status output of a solve (src/nonlin_helper.f90:17-33)."""
    out = []
    for it, ne, nj, xn, fn in result["status_lines"]:
        jl = "Jacobian Evaluations: %d\n" % nj if nj > 0 else ""
        out.append(" \nIteration: %d\nFunction Evaluations: %d\n%sChange in Variable: %s\nResidual: %s\n"
                   % (it, ne, jl, format_e10_3(xn), format_e10_3(fn)))
    return "".join(out)


# the reference's test functions (tests/nonlin_test_solve.f90:164-186) and the newton1d example (examples/
# example_problems.f90:95-100, x**3 spelled out as products)
def sinx_over_x(x, args=None):
    return math.sin(x) / x


def a_sinx_over_x(x, args):
    return args * math.sin(x) / x


def example_cubic(x, args=None):
    return x * x * x - 2.0 * x - 1.0


def cubic(c):
    """The device test family c0 + x (c1 + x (c2 + x c3)) and its derivative c1 + x (2 c2 + x 3 c3)."""
    c0, c1, c2, c3 = (float(v) for v in c)

    def f(x, args=None):
        return c0 + x * (c1 + x * (c2 + x * c3))

    def df(x, args=None):
        return c1 + x * (2.0 * c2 + x * (3.0 * c3))
    return f, df
