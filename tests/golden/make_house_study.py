"""Writes tests/golden/house_study.json: for every shape of house_cases.STUDY_SHAPES the column-wise residuals of A = Q R
and of Q^T Q = I (house_cases.residuals) that the CPU restatement of the Householder steps (nlo_qr_factor_cols on [A | I])
leaves, those numpy.linalg.qr (LAPACK) leaves on the same matrix, and their quotients.  tests/test_oracle.py allows the
restatement four times the largest recorded quotient over what LAPACK leaves, both sides recomputed live: LAPACK's blocked
sums and the restatement's ascending sums differ by the order of reduction only, which moves a residual by small factors,
not by orders.

    python tests/golden/make_house_study.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import house_cases as HC  # noqa: E402
from oracle import pyoracle  # noqa: E402


def main():
    study = {"numpy": np.__version__,
             "statistic": "fac = max_k ||(A - Q R)[:, k]|| / ||A[:, k]||, orth = max_k ||(Q^T Q - I)[:, k]||; ratio = ours / LAPACK's",
             "shapes": []}
    for m, n in HC.STUDY_SHAPES:
        a = HC.study_matrix(m, n)
        ours, lap = HC.oracle_residuals(pyoracle, a), HC.lapack_residuals(a)
        rec = {"m": m, "n": n, "ours": list(ours), "lapack": list(lap), "ratio": [ours[0] / lap[0], ours[1] / lap[1]]}
        study["shapes"].append(rec)
        print(rec, flush=True)
    study["worst_ratio"] = max(max(s["ratio"]) for s in study["shapes"])
    with open(os.path.join(HERE, "house_study.json"), "w") as f:
        json.dump(study, f, indent=1, sort_keys=True)
        f.write("\n")
    print("worst ratio =", study["worst_ratio"])


if __name__ == "__main__":
    main()
