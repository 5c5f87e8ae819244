"""Formulas at the documented limits of the formula models (include/nonlin_hip.h: 256 instructions, 64 constants, stack depth
16, 4 variables, 32 parameters), their seeded data, and the restatement of a whole point list at once (tests/
test_expr_limits_cpu.py, tests/test_gpu_expr_limits.py).  Every program is in the bit-exact class -- no library function --
so the device is held to the restatement bit for bit.  tests/expr_cases.py keeps the everyday formulas.  Test
infrastructure, not part of the product."""
import numpy as np

import pwfun_restatement as PW

_P32 = ",".join("p%d" % k for k in range(32))
_c = lambda i: repr(0.5 + i / 64.0)                                 # (exact in binary: the literal is the value)
_PEAKS = 16


def _deep16():
    """p0*t+(p1*t+( ... (p14*t) ... )): 14 sums wait on the stack while the innermost product is formed."""
    return "".join("p%d*t+(" % k for k in range(14)) + "p14*t" + ")" * 14


def _wide32():
    """Sixteen Lorentzians of unit width: the amplitude a_k is parameter 2k, the centre m_k parameter 2k + 1."""
    return "+".join("a%d/(1.0+(t-m%d)*(t-m%d))" % (k, k, k) for k in range(_PEAKS))


def _full256():
    """-c0*t+c1*p0+c2*t+c3*p1+ ... +c63*p31: the last instruction, the last constant, an operand root up to 252."""
    return "-%s*t" % _c(0) + "".join("+%s*%s" % (_c(i), "p%d" % (i // 2) if i % 2 else "t") for i in range(1, 64))


def _where256():
    """where(t-0.5, S1, S2): S1 names p0 .. p30 and ends at instruction 131, S2 names p31 .. p1; 256 instructions."""
    s1 = "+".join("%s*p%d" % (_c(i), i) for i in range(31)) + "+t+t+t"
    s2 = "+".join("%s*p%d" % (_c(31 + i), 31 - i) for i in range(31))
    return "where(t-0.5,%s,%s)" % (s1, s2)


def _vars4():
    """A polynomial of degree 8 without a constant term in each of four variables: parameter 8 v + k - 1 times var_v^k."""
    return "+".join("p%d*%s" % (8 * v + k - 1, name if k == 1 else "%s^%d" % (name, k)) for v, name in enumerate("xyzu") for k in range(1, 9))


# name: (formula, vars, params, t range, (low, high) of every true parameter, (nvar, n, ninstr, nconst, depth), root mask,
# relative spread of x0 about the truth)
ALL32 = 0xffffffff
FORMULAS = {
    "deep16": (_deep16(), "t", ",".join("p%d" % k for k in range(15)), (0.0, 1.0), [(0.5, 1.5)] * 15, (1, 15, 59, 0, 16), 0x7fff, 0.05),
    "wide32": (_wide32(), "t", ",".join("a%d,m%d" % (k, k) for k in range(_PEAKS)), (0.0, 64.0),
               [b for k in range(_PEAKS) for b in ((0.5, 1.5), (4.0 * k + 1.5, 4.0 * k + 2.5))], (1, 32, 191, 16, 6), ALL32, 0.02),
    "full256": (_full256(), "t", _P32, (0.0, 2.0), [(0.5, 1.5)] * 32, (1, 32, 256, 64, 3), ALL32, 0.05),
    "where256": (_where256(), "t", _P32, (0.0, 1.0), [(0.5, 1.5)] * 32, (1, 32, 256, 63, 5), ALL32, 0.05),
    "vars4": (_vars4(), "x,y,z,u", _P32, (-1.0, 1.0), [(0.5, 1.5)] * 32, (4, 32, 155, 0, 3), ALL32, 0.05),
    "sparse32": ("p31*t-p0", "t", _P32, (0.0, 2.0), [(0.5, 1.5)] * 32, (1, 32, 5, 0, 2), 0x80000001, 0.05),
}
# the largest launch the kernels make, 131,072 bytes of LDS: deep16 over 32 names (17 of them unused) at m = 1
DEEP16_PADDED = (_deep16(), "t", ",".join(["p%d" % k for k in range(15)] + ["u%d" % k for k in range(15, 32)]))
# (max of the operand-root fields: aroot over the program, broot of the last instruction)
ROOTS = {"deep16": (42, 0), "wide32": (184, 0), "full256": (252, 0), "where256": (251, 131), "vars4": (150, 0), "sparse32": (2, 0)}
# the solves at n = 32 (tests/test_expr_limits_cpu.py holds the reference's solver to this family first)
SOLVE_NAME, SOLVE_M, SOLVE_NPROB, MAX_EVALS = "wide32", 128, 8, 500


def compile_formula(name):
    import nonlin_amd as nl
    f, v, p = FORMULAS[name][:3]
    return nl.Expr(f, v, p)


def limit_problems(name, m, nprob=5, seed=2026, sigma=1e-3, prog=None):
    """nprob data sets of a limit formula on m rows, as expr_cases.expr_problems makes them: prog, t [nvar, nprob, m],
    y [nprob, m], x_true, x0 [nprob, n].  One variable: a jittered grid over the formula's range; vars4: the four variables
    drawn from U(-1, 1), and its parameters of either sign."""
    if prog is None:
        e = compile_formula(name)
        prog = e.program()
        e.close()
    f, v, p, (lo, hi), box, shape, mask, spread = FORMULAS[name]
    rng = np.random.default_rng(seed)
    nvar = shape[0]
    if nvar == 1:
        step = (hi - lo) / m
        t = (np.tile(np.linspace(lo + 0.25 * step, hi - 0.25 * step, m), (nprob, 1)) + rng.uniform(-0.2, 0.2, (nprob, m)) * step)[None]
    else:
        t = rng.uniform(lo, hi, (nvar, nprob, m))
    box = np.array(box)
    xt = rng.uniform(box[:, 0], box[:, 1], (nprob, len(box)))
    if name == "vars4":
        xt *= rng.choice([-1.0, 1.0], xt.shape)
    y = np.empty((nprob, m))
    for q in range(nprob):
        y[q] = PW.value(prog, xt[q], t[:, q])
        y[q] += sigma * np.abs(y[q]).max() * rng.uniform(-1, 1, m)
    x0 = xt * (1.0 + spread * rng.uniform(-1, 1, xt.shape))
    return prog, np.ascontiguousarray(t), np.ascontiguousarray(y), xt, np.ascontiguousarray(x0)


def restate(prog, X, t, y=None, w=None):
    """The restatement on a whole point list in one pass per column: X [npoints, n] at the rows t [nvar, npoints, m] (every
    operation is elementwise, so a point's bits are those of a pass of its own) -> F [npoints, m] -- the residual with
    y [npoints, m], the model value without -- and J [npoints, n, m] as the launchers lay it out; w [npoints, m] or None."""
    x = [X[:, k:k + 1] for k in range(X.shape[1])]
    tv = [np.asarray(t[v]) for v in range(len(t))]
    F = PW.run(prog, x, tv)[0]
    if y is not None:
        F = F - y
    if w is not None:
        F = w * F
    J = np.zeros((X.shape[0], X.shape[1], tv[0].shape[1]))
    for j in range(X.shape[1]):
        d = PW.run(prog, x, tv, j)[1]
        if d is not None:
            J[:, j] = w * d if w is not None else d
        elif w is not None:
            J[:, j] = w * J[:, j]
    return F, J
