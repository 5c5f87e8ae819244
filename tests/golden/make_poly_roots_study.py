"""Writes tests/golden/poly_roots_study.json: per family of tests/polyroots_cases.py the largest backward-error-style
ratio r(z) of LAPACK's roots (numpy.linalg.eigvals on the companion matrix), of the restatement's
(tests/polyroots_restatement.py), and their quotient; for families a and c the same for the forward error against
mpmath.polyroots.  tests/test_polyroots_cpu.py derives its bound M from the quotients (the smallest power of two that is
at least twice the largest, never above 16) and recomputes both sides live.

    python tests/golden/make_poly_roots_study.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import scipy  # noqa: E402
import mpmath  # noqa: E402

import polyroots_measure as pm  # noqa: E402


def main():
    study = {"numpy": np.__version__, "scipy": scipy.__version__, "mpmath": mpmath.__version__, "eps": pm.EPS,
             "statistic": "r(z) = |p(z)| / sum_k |a_k| |z|^k at 60 digits; ratio = max r(ours) / max(max r(LAPACK), eps)",
             "families": {}}
    for name in ("a", "b", "c", "d", "e"):
        study["families"][name] = pm.measure_family(name, forward=name in ("a", "c"))
        print(name, study["families"][name], flush=True)
    study["M"] = pm.bound_from_study(study)
    with open(os.path.join(HERE, "poly_roots_study.json"), "w") as f:
        json.dump(study, f, indent=1, sort_keys=True)
        f.write("\n")
    print("M =", study["M"])


if __name__ == "__main__":
    main()
