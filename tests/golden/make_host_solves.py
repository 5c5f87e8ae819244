"""Records tests/golden/host_solves_parent.json on a machine with the GPU: what the five single solves with a host callback
(nlh_lm_solve, nlh_newton_solve, nlh_quasi_newton_solve, nlh_cls_solve, nlh_bfgs_solve) return, and how they call the
user's function, for every case and refusal of tests/host_solve_cases.py, as this checkout computes them.  Run once, on
the commit BEFORE those entry points were put on the lock-step drivers; tests/test_gpu_host_solves.py holds every later
commit to it.
    python tests/golden/make_host_solves.py [OUT_DIR]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    import host_solve_cases as H
    from nonlin_amd.device import DeviceSolver
    from oracle import pyoracle as O
    out = os.path.join(sys.argv[1] if len(sys.argv) > 1 else HERE, "host_solves_parent.json")
    ds = DeviceSolver(0)
    rec = H.record_all(ds, O)
    H.dump(rec, out)
    assert H.load(out) == rec                                         # packed without loss
    assert H.record_all(ds, O) == rec                                 # and the same on a second run: nothing of this process in it
    bad = {k: v["rc"] for k, v in rec["cases"].items() if v["rc"] not in (0, H.CONVERGENCE_ERROR)}
    print(len(rec["cases"]), "cases,", sum(len(v) for v in rec["refusals"].values()), "refusals,", os.path.getsize(out), "bytes; other codes:", bad)
    for solver, res in sorted(rec["refusals"].items()):
        print("  ", solver, {k: v[0] for k, v in res.items()})


if __name__ == "__main__":
    main()
