"""The cases of the robust-loss tests (tests/test_loss_cpu.py, tests/test_gpu_loss.py, profiles/scripts/loss_rate.py): a
Lorentzian on a constant with Gaussian noise and a few large positive outliers per spectrum -- the cosmic-ray spikes a robust
loss is for.  Test infrastructure, not part of the product."""
import numpy as np

import curve_restatement as R

KIND, K, B = "lorentz", 1, 0                    # parameters: a, mu, w, c0
SIGMA = 0.02
SCALE = 3.0 * SIGMA                             # the scale c of every loss: three noise sigmas
# (m, outliers per spectrum): 100 problems each
FAMILIES = [(64, 4), (200, 12)]
NPROB, SEED = 100, 7


def outlier_problems(m, nout, nprob=NPROB, seed=SEED):
    """t, y [nprob, m], x_true, x0 [nprob, 4]: y = model + SIGMA N(0, 1), plus U(0.5, 1.5) at nout random rows; x0 within 5 %
    of the truth."""
    rng = np.random.default_rng(seed)
    t = np.tile(np.linspace(-3.0, 3.0, m), (nprob, 1))
    xt, x0, y = np.empty((nprob, 4)), np.empty((nprob, 4)), np.empty((nprob, m))
    for p in range(nprob):
        xt[p] = [2.0 + rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5), 0.6 + rng.uniform(-0.1, 0.1), 0.3]
        y[p] = R.model(R.LORENTZ, K, B, xt[p], t[p]) + SIGMA * rng.standard_normal(m)
        idx = rng.choice(m, nout, replace=False)
        y[p, idx] += rng.uniform(0.5, 1.5, nout)
        x0[p] = xt[p] * (1.0 + 0.05 * rng.uniform(-1, 1, 4))
    return np.ascontiguousarray(t), y, xt, x0
