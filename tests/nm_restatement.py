"""Plain-Python restatement of nelder_mead%solve (nm_solve, src/nonlin_optimize.f90:104-340) and nm_extrapolate
(:343-399), one statement per reference statement, IEEE double arithmetic in the reference's order (explicit products,
no fused operations, pcent summed over the vertices in ascending order).  It is what the GPU tests compare the device
state machine against bit for bit.  Test infrastructure, not part of the product.

simplex: a list of npts = n + 1 vertices (column i of the reference's m_simplex), each a list of n floats.
"""
import math


def initial_simplex(x, init_size=1.0):
    """:205-213: column 1 is x, column i+1 is x plus init_size in coordinate i."""
    n = len(x)
    s = [[float(v) for v in x] for _ in range(n + 1)]         # :206-209
    for i in range(n):
        s[i + 1][i] = s[i + 1][i] + init_size                 # :210-212
    return s


def _sum_vertices(simplex, n):
    """pcent(i) = sum(m_simplex(i,:)) (:222-224, :300-302), ascending vertex order."""
    pcent = []
    for i in range(n):
        t = 0.0
        for v in simplex:
            t = t + v[i]
        pcent.append(t)
    return pcent


def _extrapolate(fcn, simplex, y, pcent, ihi, fac, counters, work, args):
    """nm_extrapolate (:343-399); counters = [neval]."""
    ndim = len(simplex[0])
    fac1 = (1.0 - fac) / float(ndim)                          # :382
    fac2 = fac1 - fac                                         # :383
    for i in range(ndim):
        work[i] = pcent[i] * fac1 - simplex[ihi][i] * fac2    # :385
    ytry = float(fcn(list(work), args))                       # :388
    counters[0] = counters[0] + 1                             # :389
    if ytry < y[ihi]:                                         # :390
        y[ihi] = ytry                                         # :391
        for i in range(ndim):
            pcent[i] = pcent[i] + work[i] - simplex[ihi][i]   # :393 (left to right)
            simplex[ihi][i] = work[i]                         # :394
    return ytry


def nm_solve(fcn, x, simplex=None, init_size=1.0, max_evals=500, tol=1e-12, args=None):
    """nm_solve.  fcn(x_list, args) -> float.  simplex: None (built from x) or the object's simplex of the right shape
    (then x is ignored).  Returns a dict: x (list), fout, simplex (the final one), iter_count, fcn_count, converge_on_fcn,
    status (0 or 106), shrinks (number of shrink steps), status_lines (what print_status would print, per iteration)."""
    n = len(x)
    npts = n + 1
    x = [float(v) for v in x]
    if simplex is None:
        simplex = initial_simplex(x, init_size)               # :180-213
    else:
        simplex = [[float(c) for c in v] for v in simplex]
    f = [0.0] * npts
    work = [0.0] * n
    for i in range(npts):
        f[i] = float(fcn(list(simplex[i]), args))             # :216-218
    counters = [npts]                                         # :219 neval
    fval = f[0]                                               # :220
    pcent = _sum_vertices(simplex, n)                         # :222-224
    flag = 0                                                  # :227
    fcnvrg = False
    it = 0
    shrinks = 0
    blocks = []
    while True:
        it = it + 1                                           # :230
        ilo = 0                                               # :233 (0-based from here on)
        if f[0] > f[1]:                                       # :234-240
            ihi, ihi2 = 0, 1
        else:
            ihi, ihi2 = 1, 0
        for i in range(npts):                                 # :241-249
            if f[i] <= f[ilo]:
                ilo = i
            if f[i] > f[ihi]:
                ihi2 = ihi
                ihi = i
            elif f[i] > f[ihi2]:
                if i != ihi:
                    ihi2 = i
        rtol = abs(f[ihi] - f[ilo])                           # :256
        if rtol < tol:                                        # :257
            f[0], f[ilo] = f[ilo], f[0]                       # :258-260
            simplex[0], simplex[ilo] = simplex[ilo], simplex[0]   # :261-264 (coordinate-wise swap)
            x = list(simplex[0])                              # :264
            fval = f[0]                                       # :266
            fcnvrg = True
            break
        ftry = _extrapolate(fcn, simplex, f, pcent, ihi, -1.0, counters, work, args)        # :273-274
        if ftry <= f[ilo]:                                    # :275
            _extrapolate(fcn, simplex, f, pcent, ihi, 2.0, counters, work, args)            # :279-280
        elif ftry >= f[ihi2]:                                 # :281
            fsave = f[ihi]                                    # :284
            ftry = _extrapolate(fcn, simplex, f, pcent, ihi, 0.5, counters, work, args)     # :285-286
            if ftry >= fsave:                                 # :287
                shrinks += 1
                for i in range(npts):                         # :290-297
                    if i != ilo:
                        mid = [0.5 * (simplex[i][k] + simplex[ilo][k]) for k in range(n)]
                        simplex[i] = mid
                        f[i] = float(fcn(list(mid), args))
                counters[0] = counters[0] + npts              # :299 (npts, not npts - 1)
                pcent = _sum_vertices(simplex, n)             # :300-302
        blocks.append((it, counters[0], fval, rtol))          # :306-313 (stale fval)
        if counters[0] >= max_evals:                          # :316
            flag = 1
            break
    return {
        "x": x, "fout": fval, "simplex": simplex, "iter_count": it, "fcn_count": counters[0], "converge_on_fcn": fcnvrg,
        "status": 106 if flag else 0, "shrinks": shrinks, "status_lines": blocks,
    }


def format_e10_3(v):
    """Fortran E10.3 as flang writes it (what the library's format_e10_3 produces)."""
    if math.isnan(v):
        return "%10s" % "NaN"
    if math.isinf(v):
        return "%10s" % ("-Inf" if v < 0 else "Inf")
    sci = "%.2e" % abs(v)
    ex = int(sci[5:])
    if v != 0.0:
        ex += 1
    sign = "-" if (math.copysign(1.0, v) < 0 and v != 0.0) else " "
    if abs(ex) < 100:
        body = "%s0.%s%s%sE%s%02d" % (sign, sci[0], sci[2], sci[3], "-" if ex < 0 else "+", abs(ex))
    else:
        body = "%s0.%s%s%s%s%03d" % (sign, sci[0], sci[2], sci[3], "-" if ex < 0 else "+", abs(ex))
    return "%10s" % body


def status_text(result):
    """The print_status output of a solve (:306-313): ` ` (print *, ""), then four lines per iteration."""
    out = []
    for it, ne, fv, rt in result["status_lines"]:
        out.append(" \nIteration: %d\nFunction Evaluations: %d\nFunction Value: %s\nConvergence Parameter: %s\n"
                   % (it, ne, format_e10_3(fv), format_e10_3(rt)))
    return "".join(out)


# the reference's test objectives (tests/nonlin_test_optimize.f90)
def rosenbrock(x, args=None):
    """f = 100 (x2 - x1^2)^2 + (x1 - 1)^2, as in the reference's test (powers spelled out as products)."""
    a = x[1] - x[0] * x[0]
    b = x[0] - 1.0
    return 1.0e2 * (a * a) + b * b


def beale(x, args=None):
    a = 1.5 - x[0] + x[0] * x[1]
    b = 2.25 - x[0] + x[0] * (x[1] * x[1])
    c = 2.625 - x[0] + x[0] * (x[1] * x[1] * x[1])
    return a * a + b * b + c * c
