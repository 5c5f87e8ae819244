"""Records tests/golden/fit_entry_points_parent.npz on a GPU: the batch of tests/fit_entry_cases.py through the twelve
one-call fits, every configuration, as this checkout computes it.  Run once, on the commit BEFORE the fit pipeline of
nlh_fit.hip replaced the twelve hand-written bodies; tests/test_gpu_fit_entry_points.py holds every later commit to it bit
for bit.
    python tests/golden/make_fit_entry_points.py [OUT.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import fit_entry_cases as FC
    import nonlin_amd as nl
    from nonlin_amd.device import DeviceSolver
    ds = DeviceSolver(0)
    expr = nl.Expr(FC.FORMULA, FC.VARS, FC.PARAMS)
    pm = nl.ParamMap(FC.N, fixed=FC.MAP_FIXED, tied=FC.MAP_TIED)
    data = FC.batch(expr)
    out = {}
    for model, variant, host in FC.ENTRIES:
        for k, v in FC.run_entry(ds, data, expr, pm, model, variant, host).items():
            out[FC.entry_name(model, variant, host) + "." + k] = v
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "fit_entry_points_parent.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
    st = out["nlh_curve_fit_batch.status"]
    print("status of nlh_curve_fit_batch:", st.tolist())


if __name__ == "__main__":
    main()
