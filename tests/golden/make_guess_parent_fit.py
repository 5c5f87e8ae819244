"""Records tests/golden/guess_parent_fit.npz on a GPU: curve_fit_batch with a caller's x0 on the case of
tests/guess_cases.parent_fit_case, as this checkout computes it.  Run once, on the commit BEFORE curve_fit_batch learned
x0=None; tests/test_gpu_guess.py holds every later commit to it bit for bit.  NONLIN_AMD_ROOT: the checkout whose package is
recorded (default: this one).
    python tests/golden/make_guess_parent_fit.py [OUT.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get("NONLIN_AMD_ROOT", os.path.dirname(os.path.dirname(HERE))))
sys.path.insert(1, os.path.dirname(HERE))


def main():
    import guess_cases as GC
    import nonlin_amd
    from nonlin_amd.device import DeviceSolver
    out = GC.run_parent_fit(DeviceSolver(0))
    path = sys.argv[1] if len(sys.argv) > 1 else GC.PARENT_GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes, package", nonlin_amd.__file__)
    print("status:", out["status"].tolist())


if __name__ == "__main__":
    main()
