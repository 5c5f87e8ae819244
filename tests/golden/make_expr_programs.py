"""Records tests/golden/expr_programs_parent.json, on any machine (no GPU): what nlh_expr_compile makes of every formula of
tests/expr_cases.py and tests/expr_limit_cases.py -- op, arg, mask, aroot, broot per instruction, the constants, the shape --
as this checkout's library, or the one named, has it.  Run once, on the commit BEFORE definitions were added to the grammar;
tests/test_defs_cpu.py holds every later commit to it: a formula without ';' compiles to the program it always did.
    python tests/golden/make_expr_programs.py [LIBRARY]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def record():
    import expr_cases as EC
    import expr_limit_cases as LC
    import nonlin_amd as nl
    cases = {"expr_cases." + k: v[:3] for k, v in EC.FORMULAS.items()}
    cases.update({"expr_limit_cases." + k: v[:3] for k, v in LC.FORMULAS.items()})
    cases["expr_limit_cases.DEEP16_PADDED"] = LC.DEEP16_PADDED
    rec = {}
    for name, (f, v, p) in cases.items():
        e = nl.Expr(f, v, p)
        op, arg, consts, mask = e.program()
        aroot, broot = e.roots()
        rec[name] = {"shape": [e.nvar, e.nparams, e.ninstr, e.nconst, e.depth], "op": op.tolist(), "arg": arg.tolist(),
                     "mask": mask.tolist(), "aroot": aroot.tolist(), "broot": broot.tolist(), "consts": [float(c).hex() for c in consts]}
        e.close()
    return rec


def main():
    if len(sys.argv) > 1:
        from nonlin_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    rec = record()
    with open(os.path.join(HERE, "expr_programs_parent.json"), "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rec.items()) + "\n}\n")   # a line per formula
    print(len(rec), "formulas,", sum(v["shape"][2] for v in rec.values()), "instructions")


if __name__ == "__main__":
    main()
