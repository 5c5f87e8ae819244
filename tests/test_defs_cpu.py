"""CPU tests of definitions in formulas (include/nonlin_hip.h: formula := (name '=' expr ';')* expr, NLH_EXPR_LOAD): what the
compiler makes of them -- listing, masks, roots, the frame --, that the expanded program (tests/defs_restatement.py) is the
program of the formula with each definition substituted in parentheses, the exact class against Python's own exec, the
refusals with their columns, the limits counted on what is written, and that a formula without ';' compiles to what the
commit before made of it (tests/golden/expr_programs_parent.json)."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

import defs_cases as DC
import defs_restatement as D
import pwfun_restatement as PW

HERE = os.path.dirname(os.path.abspath(__file__))
NL_INVALID_INPUT_ERROR = 201


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _expr(formula, vars, params):
    import nonlin_amd as nl
    return nl.Expr(formula, vars, params)


def _listing(e):
    op, arg, consts, mask = e.program()
    return [(D.OPS[o], int(a)) for o, a in zip(op, arg)]


# ------------------------------------------------------------------------------------------------ 1. the compiler
def test_exports():
    import nonlin_amd as nl
    assert nl.EXPR_DEF_OPS == ("LOAD",) == D.EXPR_DEF_OPS and "EXPR_DEF_OPS" in nl.__all__
    assert D.OPS == nl.EXPR_OPS + nl.EXPR_SPECIAL_OPS + nl.EXPR_EXTENDED_OPS + nl.EXPR_DEF_OPS and D.OPS[D.LOAD] == "LOAD" and D.LOAD == 27
    assert "dx = x-x0" in nl.Expr.__doc__ and "formula := (name '=' expr ';')* expr" in nl.Expr.__doc__


# name: (listing, masks, aroot, (instruction, broot) or None, defs, nconst, depth)
LISTINGS = {
    # the Gaussian with u = (t-mu)/s: the definition's five instructions, then the model value on top of slot 0
    "gauss_u": ([("VAR", 0), ("PARAM", 1), ("SUB", 0), ("PARAM", 2), ("DIV", 0), ("PARAM", 0), ("LOAD", 0), ("IPOW", 2), ("NEG", 0),
                 ("CONST", 0), ("DIV", 0), ("EXP", 0), ("MUL", 0), ("PARAM", 3), ("ADD", 0)],
                [0, 2, 2, 4, 6, 1, 6, 6, 6, 0, 6, 6, 7, 8, 15], [0, 0, 0, 0, 2, 0, 4, 0, 0, 0, 8, 0, 5, 0, 12], None, ("u",), 1, 4),
    # a definition that uses an earlier one; v twice
    "chain": ([("VAR", 0), ("PARAM", 1), ("SUB", 0), ("LOAD", 0), ("PARAM", 2), ("DIV", 0), ("PARAM", 0), ("CONST", 0), ("LOAD", 1),
               ("LOAD", 1), ("MUL", 0), ("ADD", 0), ("DIV", 0), ("PARAM", 3), ("ADD", 0)],
              [0, 2, 2, 2, 4, 6, 1, 0, 6, 6, 6, 6, 7, 8, 15], [0, 0, 0, 2, 0, 3, 0, 0, 5, 5, 8, 7, 6, 0, 12], None, ("u", "v"), 1, 6),
    # a bare parameter: the definition is its PARAM, the LOADs carry its mask
    "bare_param": ([("PARAM", 0), ("LOAD", 0), ("VAR", 0), ("MUL", 0), ("LOAD", 0), ("PARAM", 1), ("MUL", 0), ("ADD", 0)],
                   [1, 1, 0, 1, 1, 2, 3, 3], [0, 0, 0, 1, 0, 0, 4, 3], None, ("k",), 0, 4),
    # a bare constant: no tangent anywhere in it
    "bare_const": ([("CONST", 0), ("LOAD", 0), ("PARAM", 0), ("MUL", 0), ("VAR", 0), ("MUL", 0), ("LOAD", 0), ("ADD", 0)],
                   [0, 0, 1, 1, 0, 1, 0, 1], [0, 0, 0, 1, 0, 3, 0, 5], None, ("h",), 1, 3),
    # an unused definition: it is computed, its parameter b is in its masks and not in the root's
    "unused": ([("PARAM", 1), ("VAR", 0), ("MUL", 0), ("PARAM", 0), ("VAR", 0), ("MUL", 0), ("CONST", 0), ("ADD", 0)],
               [2, 0, 2, 1, 0, 1, 0, 1], [0, 0, 0, 0, 0, 3, 0, 5], None, ("z",), 1, 3),
    # LOAD as the lower operand of a binary instruction (aroot names the LOAD) and as the top one
    "lower": ([("PARAM", 0), ("VAR", 0), ("MUL", 0), ("LOAD", 0), ("PARAM", 1), ("SUB", 0), ("PARAM", 1), ("LOAD", 0), ("SUB", 0),
               ("MUL", 0)], [1, 0, 1, 1, 2, 3, 2, 1, 3, 3], [0, 0, 0, 2, 0, 3, 0, 2, 6, 5], None, ("u",), 0, 4),
    # LOAD as voigt's sigma: broot names the LOAD
    "voigt_mid": ([("PARAM", 2), ("CONST", 0), ("ADD", 0), ("PARAM", 0), ("VAR", 0), ("PARAM", 1), ("SUB", 0), ("LOAD", 0), ("PARAM", 3),
                   ("VOIGT", 0), ("MUL", 0), ("PARAM", 4), ("ADD", 0)],
                  [4, 0, 4, 1, 0, 2, 2, 4, 8, 14, 15, 16, 31], [0, 0, 0, 0, 0, 0, 4, 2, 0, 6, 3, 0, 10], (9, 7), ("w",), 1, 5),
    # LOAD as where's first branch: broot names the LOAD
    "where_mid": ([("PARAM", 0), ("VAR", 0), ("MUL", 0), ("VAR", 0), ("PARAM", 1), ("SUB", 0), ("LOAD", 0), ("PARAM", 2), ("WHERE", 0)],
                  [1, 0, 1, 0, 2, 2, 1, 4, 7], [0, 0, 0, 0, 0, 3, 2, 0, 5], (8, 6), ("u",), 0, 4),
    # LOAD under a unary instruction and under ^2: their operand is the instruction before, the LOAD
    "unary": ([("PARAM", 0), ("VAR", 0), ("MUL", 0), ("PARAM", 1), ("ADD", 0), ("LOAD", 0), ("ABS", 0), ("LOAD", 0), ("IPOW", 2),
               ("ADD", 0), ("LOAD", 0), ("NEG", 0), ("SUB", 0)],
              [1, 0, 1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3], [0, 0, 0, 0, 2, 4, 0, 4, 0, 6, 4, 0, 9], None, ("u",), 0, 3),
}


@pytest.mark.parametrize("name", DC.SMALL)
def test_listings(name):
    listing, masks, aroot, b, defs, nconst, depth = LISTINGS[name]
    e = DC.compile_formula(name)
    op, arg, consts, mask = e.program()
    assert _listing(e) == listing
    assert [int(k) for k in mask] == masks
    ar, br = e.roots()
    assert [int(k) for k in ar] == aroot
    want_b = [0] * len(listing)
    if b:
        want_b[b[0]] = b[1]
    assert [int(k) for k in br] == want_b
    assert (e.defs, e.nconst, e.depth, e.ninstr) == (defs, nconst, depth, len(listing))
    assert D.frame(op) == e.depth                                       # the frame: the most slots in use, definitions included
    for pc, (o, k) in enumerate(listing):                               # the code word of LOAD k
        if o == "LOAD":
            root = D.definition_roots(op)[k]
            assert int(op[pc]) == 27 and ar[pc] == root and mask[pc] == mask[root]


def test_defs_attribute_and_blanks():
    import nonlin_amd as nl
    assert nl.Expr("a*t", "t", "a").defs == ()
    e = nl.Expr(DC.ROT2D, "x,y", "a,x0,y0,sx,sy,th,b")                  # three lines
    assert e.defs == ("dx", "dy", "c", "s", "u", "v") and (e.ninstr, e.nconst, e.depth) == (45, 2, 12)
    assert e.defs == DC.compile_formula("rot2d").defs
    assert _listing(nl.Expr(" u\t=\n a*t ;\r\n u + u ", "t", "a")) == _listing(nl.Expr("u=a*t;u+u", "t", "a"))
    assert nl.Expr("_u1 = a; _u1*t", "t", "a").defs == ("_u1",)          # the name rule


# ------------------------------------------------------------------------------------------------ 2. expansion
@pytest.mark.parametrize("name", list(DC.FORMULAS))
def test_expansion_is_the_substituted_program(name):
    """expand(program) is LOAD-free and is, instruction for instruction, what the compiler makes of the substituted string
    -- wherever that compiles: over256 does not, and its expansion is longer than any program."""
    e = DC.compile_formula(name)
    x = DC.expanded(e)
    assert not (x[0] == D.LOAD).any() and D.definition_roots(x[0]) == []
    text = D.substituted(DC.FORMULAS[name][0])
    assert ";" not in text and "=" not in text
    if name == "over256":
        assert len(x[0]) == 321
        with pytest.raises(ValueError, match="more than 256 instructions"):
            DC.compile_formula(name, substituted=True)
        return
    s = DC.compile_formula(name, substituted=True)
    assert s.defs == () and D.same_program(x, s.program()), name
    assert D.frame(x[0]) == s.depth


def test_substituted_text():
    assert D.substituted("u = t-mu; v = u/s; a/(1+v*v)+c") == "a/(1+((t-mu)/s)*((t-mu)/s))+c"
    assert D.substituted("s = a; sx*s + s") == "sx*(a) + (a)"            # whole names only
    assert D.substituted("a*t") == "a*t"


# ------------------------------------------------------------------------------------------------ 3. the exact class
PY_FORMULAS = ["u = a*t; u+u*b", "u = t-a; v = u*u; v/(1+v)+c*u", "h = max(t-a,0); b*h+c*h*h", "u = a*t; v = u-b; where(v,u,c)*min(u,v)",
               "k = a; z = 0.5; k*t+z*k", "u = b/t; unused = c*t; where(a-t,u,c*t)+min(t,a)+u", "p = a+b; q = p*c; r = q-p; r/q+p*t"]


@pytest.mark.parametrize("formula", PY_FORMULAS)
def test_exact_class_against_python(formula):
    """Over + - * /, min, max and where the statements are Python's: exec of each on float64 arrays, min / max / where as the
    header's selects (tests/test_pwfun_cpu.py::test_exact_class_against_python), gives the bits of the restatement of the
    expanded program, with running bound 0."""
    e = _expr(formula, "t", "a,b,c")
    prog = DC.expanded(e)
    rng = np.random.default_rng(len(formula))
    t = np.sort(rng.uniform(0.1, 4.0, 257))
    t[::16] = 1.5
    env = {"max": lambda a, b: np.where(b > a, b, a), "min": lambda a, b: np.where(b < a, b, a),
           "where": lambda c, a, b: np.where(np.asarray(c) >= 0.0, a, b), "t": t}
    *defs, last = formula.split(";")
    code = "\n".join(s.strip() for s in defs) + "\nmodel_value = " + last.strip()
    for x in (np.array([1.5, 2.25, 3.0]), np.array([1.5, 0.5, 0.75]), rng.uniform(0.5, 3.0, 3)):
        scope = dict(env, a=np.full(257, x[0]), b=np.full(257, x[1]), c=np.full(257, x[2]))
        exec(code, {"__builtins__": {}}, scope)
        want = scope["model_value"] + np.zeros(257)
        assert np.array_equal(_bits(PW.value(prog, x, [t])), _bits(want)), formula
        r, eb = PW.residual_bound(prog, x, [t], np.zeros(257))
        assert np.array_equal(_bits(r), _bits(want)) and (eb == 0.0).all()


# ------------------------------------------------------------------------------------------------ 4. refusals
REFUSALS = [("t = 1; a*t", "t", "a", "col 0: 't' is a variable"), ("u = t; a = u; a*t", "t", "a", "col 7: 'a' is a parameter"),
            ("exp = a; exp*t", "t", "a", "col 0: 'exp' is a function"), (" where = a; t", "t", "a", "col 1: 'where' is a function"),
            ("pi = 3; a*t", "t", "a", "col 0: 'pi' is the constant"),
            ("u = a*t; u = u+1; u", "t", "a", "col 9: 'u' is already defined"),
            ("v = u; u = a*t; v", "t", "a", "col 4: unknown name 'u'"), ("u+a", "t", "a", "col 0: unknown name 'u'"),
            ("u = u+a; u", "t", "a", "col 4: unknown name 'u'"),                       # no recursion: u is defined after its statement
            ("u = a*t;", "t", "a", "col 8: unexpected end of the formula"), ("u = a*t; ", "t", "a", "col 9: unexpected end of the formula"),
            ("u = a*t;; u", "t", "a", "col 8: unexpected ';'"), ("; a", "t", "a", "col 0: unexpected ';'"),
            ("u = ; a", "t", "a", "col 4: unexpected ';'"), ("u = a*t", "t", "a", "col 7: ';' expected after the definition of 'u'"),
            ("u = a*t; v = u", "t", "a", "col 14: ';' expected after the definition of 'v'"),
            ("2 = a; t", "t", "a", "col 2: unexpected '='"), ("u = a $ t; u", "t", "a", "col 6: ';' expected"),
            ("a$t", "t", "a", "col 1: unexpected '$'"), ("a t", "t", "a", "col 2: unexpected 't'"),
            ("a+sinh(t)", "t", "a", "col 2: unknown name 'sinh'"), ("u = a; u+sinh(t)", "t", "a", "col 9: unknown name 'sinh'")]


@pytest.mark.parametrize("formula,vars,params,message", REFUSALS)
def test_refusals_name_the_column(formula, vars, params, message):
    from nonlin_amd import _lib
    import nonlin_amd as nl
    L = _lib.load()
    e = C.c_void_p(7)
    assert L.nlh_expr_compile(formula.encode(), vars.encode(), params.encode(), C.byref(e)) == NL_INVALID_INPUT_ERROR
    got = L.nlh_expr_error().decode()
    assert not e.value and got.startswith(message), got
    with pytest.raises(ValueError, match="^" + re.escape(message)):
        nl.Expr(formula, vars, params)


# ------------------------------------------------------------------------------------------------ 5. limits
def test_limits_count_what_is_written():
    import nonlin_amd as nl
    e = DC.compile_formula("frame16")                                   # eight definitions under an expression eight deep
    assert (e.depth, len(e.defs), e.nparams) == (16, 8, 32) and D.frame(e.program()[0]) == 16
    with pytest.raises(ValueError, match="deeper than 16"):
        nl.Expr(DC.FRAME17, "t", DC.FORMULAS["frame16"][2])
    deep = lambda d: "a+(" * (d - 1) + "a" + ")" * (d - 1)
    assert nl.Expr("u = a; " + deep(15), "t", "a").depth == 16           # an unused definition takes its slot all the same
    with pytest.raises(ValueError, match="deeper than 16"):
        nl.Expr("u = a; " + deep(16), "t", "a")
    assert nl.Expr(deep(16), "t", "a").depth == 16
    e = DC.compile_formula("over256")                                   # 56 instructions as written, 321 substituted
    assert (e.ninstr, e.depth, e.defs) == (56, 6, ("u",))
    with pytest.raises(ValueError, match="more than 256 instructions"):
        DC.compile_formula("over256", substituted=True)
    # a definition's instructions and constants count once, and they count: 256 and 64 are reached and passed as written
    assert nl.Expr("u = a" + "+a" * 126 + "; u+u", "t", "a").ninstr == 256     # 127 PARAM and 126 ADD, then LOAD LOAD ADD
    with pytest.raises(ValueError, match="more than 256 instructions"):
        nl.Expr("u = a" + "+a" * 126 + "; u+u+u", "t", "a")
    assert nl.Expr("u = a" + "+1" * 63 + "; u*u+1", "t", "a").nconst == 64
    with pytest.raises(ValueError, match="more than 64 constants"):
        nl.Expr("u = a" + "+1" * 63 + "; u*u+1+1", "t", "a")


def test_peaks_that_fit():
    """The largest sums of peaks that compile, with definitions and substituted (profiles/defs_rate.txt records them): the
    pseudo-Voigt and the EMG end at the 32 parameters either way; the rotated Gaussian with all six definitions per peak ends
    at the frame -- six slots a peak --, substituted at the parameters."""
    got = {k: DC.most_peaks(*v) for k, v in DC.PEAKS.items()}
    assert got == {"rot2d": (1, 5), "emg": (7, 7), "pvoigt": (7, 7)}, got


# ------------------------------------------------------------------------------------------------ 6. unchanged formulas
def test_formulas_without_definitions_compile_as_before():
    """Every formula of tests/expr_cases.py and tests/expr_limit_cases.py: the op, arg, mask and root arrays, the constants
    and the shape the commit before definitions recorded (tests/golden/make_expr_programs.py)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_expr_programs as M
    with open(os.path.join(HERE, "golden", "expr_programs_parent.json")) as f:
        want = json.load(f)
    got = M.record()
    assert set(got) == set(want) and len(want) == 17
    for name in want:
        assert got[name] == want[name], name
