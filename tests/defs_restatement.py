"""Definitions in formulas (include/nonlin_hip.h: name = expr; ... and NLH_EXPR_LOAD) restated by substitution: expand()
replaces every LOAD k of a program by the instructions of statement k and drops the definition statements from the front,
which gives the LOAD-free postfix of the formula with each definition substituted in parentheses -- of any length, the 256
instructions are the compiler's limit, not the restatement's.  tests/pwfun_restatement.py runs that as it stands (its run is
stack-driven and needs no operand roots), so the oracle of a formula with definitions is PW on expand(program).
substituted() does the same to the formula's text.  Test infrastructure, not part of the product."""
import re

import numpy as np

import pwfun_restatement as PW

EXPR_DEF_OPS = ("LOAD",)
OPS = PW.OPS + EXPR_DEF_OPS
LOAD = 27
_LEAVES = (0, 1, 2, LOAD)                                           # CONST, VAR, PARAM, LOAD: push one
_BINARY = (4, 5, 6, 7, PW.POW, PW.ATAN2, PW.MIN, PW.MAX)            # pop two, push one
_TERNARY = (21, PW.WHERE)                                           # VOIGT, WHERE: pop three, push one


def definition_roots(op):
    """The instruction that produced each definition, from the stack alone: statement k leaves its root in slot k, so it is
    the last instruction after which k + 1 slots are in use; the model value ends in slot ndef."""
    sp, after = 0, []
    for o in op:
        o = int(o)
        sp += 1 if o in _LEAVES else (-1 if o in _BINARY else (-2 if o in _TERNARY else 0))
        after.append(sp)
    ndef = after[-1] - 1
    return [max(pc for pc, s in enumerate(after) if s == k + 1) for k in range(ndef)]


def frame(op):
    """The most slots in use over the program, definitions included: what nlh_expr_shape reports as depth."""
    sp = most = 0
    for o in op:
        o = int(o)
        sp += 1 if o in _LEAVES else (-1 if o in _BINARY else (-2 if o in _TERNARY else 0))
        most = max(most, sp)
    return most


def expand(prog, aroot):
    """(op, arg, consts, mask) without LOAD: every LOAD k replaced by the instruction range of statement k -- from the
    instruction after definition k - 1's root up to definition k's own root --, recursively, and the definition statements
    dropped from the front.  aroot (Expr.roots()[0]) is checked on the way: a LOAD's names the root of its definition, and
    its mask is that root's."""
    op, arg, consts, mask = prog
    roots = definition_roots(op)
    body = []                                                       # body[k]: the expanded instruction indices of statement k
    for k in range(len(roots) + 1):
        lo = roots[k - 1] + 1 if k else 0
        hi = roots[k] + 1 if k < len(roots) else len(op)
        out = []
        for pc in range(lo, hi):
            if int(op[pc]) == LOAD:
                d = int(arg[pc])
                assert 0 <= d < k and int(aroot[pc]) == roots[d] and int(mask[pc]) == int(mask[roots[d]]), (pc, d)
                out += body[d]
            else:
                out.append(pc)
        body.append(out)
    idx = np.array(body[-1], dtype=np.int64)
    return op[idx], arg[idx], consts, mask[idx]


def substituted(formula):
    """The formula's text with each definition substituted in parentheses, in order: one expression without ';'."""
    *defs, last = formula.split(";")
    for k, st in enumerate(defs):
        name, body = st.split("=")
        rest = [re.sub(r"\b%s\b" % name.strip(), lambda _: "(" + body.strip() + ")", s) for s in defs[k + 1:] + [last]]
        defs[k + 1:], last = rest[:-1], rest[-1]
    return last.strip()


def same_program(a, b):
    """Two LOAD-free programs are one: ops, args and masks equal, constants compared by value (a substituted string writes a
    definition's literals once per use)."""
    (oa, aa, ca, ma), (ob, ab, cb, mb) = a, b
    if len(oa) != len(ob) or not (np.array_equal(oa, ob) and np.array_equal(ma, mb)):
        return False
    for o, x, y in zip(oa, aa, ab):
        if int(o) in (0, 9):                                        # CONST, POWC: arg indexes the constants
            if np.float64(ca[x]).view(np.uint64) != np.float64(cb[y]).view(np.uint64):
                return False
        elif int(x) != int(y):
            return False
    return True
