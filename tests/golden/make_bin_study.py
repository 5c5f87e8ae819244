"""Re-measures the study of the bin-integrated fits (tests/bin_cases.py: study) on the CPU oracle and rewrites
tests/golden/bin_study.json, which tests/test_bin_cpu.py compares its own run with.
    python tests/golden/make_bin_study.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import bin_cases as BC  # noqa: E402
from oracle import pyoracle  # noqa: E402

if __name__ == "__main__":
    pyoracle.lib()
    res = BC.study(pyoracle)
    with open(BC.STUDY_GOLDEN, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(BC.STUDY_GOLDEN, json.dumps(res, indent=1, sort_keys=True))
