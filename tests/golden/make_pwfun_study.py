"""Writes tests/golden/pwfun_study.json: the power-law data of tests/pwfun_cases.py fitted on the CPU oracle as a*pow(t,b)+c
and as a*exp(b*log(t))+c, analytic Jacobian, on the grid with its t = 0 row and without it -- per (form, grid) the number of
failed fits among 64 and the bias and scatter of the fitted exponent (pwfun_cases.study).  The test reads the file only.
Needs the built library and oracle, no GPU.
Run: python tests/golden/make_pwfun_study.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import pwfun_cases as PC  # noqa: E402
from oracle import pyoracle  # noqa: E402

if __name__ == "__main__":
    pyoracle.lib()
    out = PC.study(pyoracle)
    with open(os.path.join(HERE, "pwfun_study.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))
