"""Records tests/golden/fit_calls_parent.json and tests/golden/lib_symbols_parent.json, on any machine (no GPU): what
DeviceSolver.curve_fit_batch / expr_fit_batch hand to the library for every case of tests/fit_call_cases.py, and the ctypes
signature table _lib.SYMBOLS, as this checkout has them.  Run once, on the commit BEFORE the Python front end was folded into
one fit path; tests/test_fit_calls_cpu.py holds every later commit to both.
    python tests/golden/make_fit_calls.py [OUT_DIR]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import fit_call_cases as FC
    from nonlin_amd import device
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    device._chk = FC.chk_any_device                                   # host tensors stand in for the device's
    rec = FC.record_all()
    FC.dump(rec, os.path.join(out, "fit_calls_parent.json"))
    assert FC.load(os.path.join(out, "fit_calls_parent.json")) == json.loads(json.dumps(rec))    # packed without loss
    calls = [v for v in rec["cases"].values() if isinstance(v, dict)]
    print(len(rec["cases"]), "cases,", len(calls), "reach the library:", sorted({c["entry"] for c in calls}))
    for model in FC.MODELS:
        plain = [v for k, v in rec["cases"].items() if k.startswith(model) and len(k.split(" ")) == 3]
        print(model, "crossing:", sum(isinstance(v, dict) for v in plain), "of", len(plain), "reach the library")
    sym = FC.symbols_snapshot()
    with open(os.path.join(out, "lib_symbols_parent.json"), "w") as f:
        f.write('{"types": %s,\n"symbols": {\n' % json.dumps(sym["types"]))
        f.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sym["symbols"].items()) + "\n}}\n")   # a line per name
    print(len(sym["symbols"]), "symbols, from", device.__file__)


if __name__ == "__main__":
    main()
