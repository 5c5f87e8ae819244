"""CPU tests of the Poisson likelihood fits (include/nonlin_hip.h: nlh_pois_*): the numpy restatement
(tests/pois_restatement.py) against 60-digit decimal arithmetic and the bound derived from the stated operations, the
properties the header promises, the validation of the Python Poisson, the error codes that need no device, and the decay
family of tests/pois_cases.py on the CPU oracle's solver with the restated transform as a host callback: status, the area
rule, the bias study and the perturbation study recorded under tests/golden/."""
import ctypes as C
import json

import numpy as np
import pytest

import curve_restatement as R
import pois_cases as PC
import pois_restatement as PR

F = PR.MU_FLOOR
NL_INVALID_INPUT_ERROR, NLH_ERR_BAD_HANDLE = 201, -3
dp = C.POINTER(C.c_double)
AREA_BOUND = PC.AREA_BOUND


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _domain(rng, n):
    """y in [0.01, 1e6] and e = rr / y with |e| in [1e-12, 1e6], e + 1 >= 1e-12, spread evenly in the logarithm, and a cluster
    on both sides of the series switch and of e = -0.5."""
    y = np.exp(rng.uniform(np.log(0.01), np.log(1e6), n))
    e = np.exp(rng.uniform(np.log(1e-12), np.log(1e6), n)) * rng.choice([-1.0, 1.0], n)
    neg = e <= -1.0
    e[neg] = -1.0 + np.exp(rng.uniform(np.log(1e-12), 0.0, int(neg.sum())))
    k = n // 10
    e[:k] = rng.choice([-1.0, 1.0], k) * PR.SWITCH * (1.0 + rng.uniform(-1e-3, 1e-3, k))
    e[k:2 * k] = -0.5 * (1.0 + rng.uniform(-1e-3, 1e-3, k))
    return y, e * y


def test_restatement_against_exact_arithmetic():
    """d and g of the restatement against decimal arithmetic at 60 digits over the documented domain: within the derived
    first-order bound, row by row, and the bound itself at most 2^-44 (numpy's log1p and log taken as 1 ulp, the entry the
    device functions are held to)."""
    rng = np.random.default_rng(0)
    y, r = _domain(rng, 6000)
    tiny = 2.0 ** -1000                                               # a floor below the whole domain: mu reaches 1e-14 here
    out, g, D, br = PR.apply(y, None, tiny, r)
    assert set(np.unique(br)) == {2, 3, 4} and ((r + y) >= tiny).all()
    bd, bg = PR.exact_bounds(y, r, ufn=1)
    assert bd.max() <= 2.0 ** -44 and bg.max() <= 2.0 ** -44, (np.log2(bd.max()), np.log2(bg.max()))
    bd_dev, bg_dev = PR.exact_bounds(y, r)                           # the device's entries
    assert bd_dev.max() <= 2.0 ** -44 and bg_dev.max() <= 2.0 ** -44
    worst = {2: [0.0, 0.0], 3: [0.0, 0.0], 4: [0.0, 0.0]}
    for i in range(len(y)):
        d_, g_ = PR.exact(y[i], r[i])
        ed, eg = PR.rel_err(out[i], d_), PR.rel_err(g[i], g_)
        assert ed <= bd[i] and eg <= bg[i], (i, y[i], r[i] / y[i], ed, bd[i], eg, bg[i])
        w = worst[int(br[i])]
        w[0], w[1] = max(w[0], ed), max(w[1], eg)
    print("poisson restatement against exact arithmetic, worst relative error (log2) of d, g: "
          + ", ".join(f"{PR.BRANCHES[b]} {np.log2(v[0]):.1f} {np.log2(v[1]):.1f}" for b, v in worst.items())
          + f"; bound at most {np.log2(max(bd.max(), bg.max())):.1f}")
    assert max(worst[2]) <= 2.0 ** -50                                  # the series: a handful of roundings
    # y = 0 and e = 0
    for yy, rr in ((0.0, 3.5), (0.0, 1e-3), (7.0, 0.0)):
        o, gg, DD, b = PR.apply(np.array([yy]), None, F, np.array([rr]))
        d_, g_ = PR.exact(yy, rr)
        bd1, bg1 = PR.exact_bounds(np.array([yy]), np.array([rr]))
        assert (PR.rel_err(o[0], d_) if d_ != 0 else abs(o[0])) <= bd1[0] and PR.rel_err(gg[0], g_) <= bg1[0]


def test_g_is_the_derivative_of_d():
    """g against a central difference of d in r with step h = 1e-5 max(|r|, y): truncation h^2 |d'''| / 6 and rounding
    eps |d| / h are both below 1e-8 of g away from the floor and from mu -> 0 (here mu >= 0.05 y), and 1e-6 is asserted; the
    difference is taken on the exact arithmetic's d, so that it tests the formula of g, not the rounding of d."""
    rng = np.random.default_rng(1)
    y = np.exp(rng.uniform(np.log(0.5), np.log(1e4), 300))
    e = np.concatenate([rng.uniform(-0.95, 3.0, 200), rng.choice([-1, 1], 100) * np.exp(rng.uniform(np.log(1e-4), 0, 100)) * 0.9])
    r = e * y
    g = PR.apply(y, None, F, r)[1]
    for i in range(len(y)):
        h = 1e-5 * max(abs(r[i]), y[i]) * min(1.0, 1.0 + e[i])
        dp_, dm_ = PR.exact(y[i], r[i] + h)[0], PR.exact(y[i], r[i] - h)[0]
        fd = float((dp_ - dm_)) / ((r[i] + h) - (r[i] - h))
        assert abs(fd - g[i]) <= 1e-6 * g[i], (i, e[i], fd, g[i])
    # y = 0: d = sqrt(2 mu), g = 1 / d
    o, gg, DD, b = PR.apply(np.zeros(3), None, F, np.array([0.5, 2.0, 1e-3]))
    assert (b == 1).all() and np.allclose(o * gg, 1.0, rtol=4 * PR.U, atol=0) and np.allclose(o * o, DD, rtol=4 * PR.U, atol=0)
    # the Jacobian rule: a row of J times its g; a masked row is +0.0 whatever J holds
    J = rng.standard_normal((5, 3))
    J[2] = np.nan
    yy, rr, w = np.array([3.0, 0.0, 5.0, 9.0, 2.0]), np.array([0.5, 1.5, 0.1, -4.0, 7.0]), np.array([1.0, 1.0, 0.0, 1.0, 1.0])
    Jw = PR.jacobian(yy, w, F, rr, J)
    gg = PR.apply(yy, w, F, rr)[1]
    assert np.array_equal(_bits(Jw[2]), _bits(np.zeros(3))) and np.array_equal(_bits(Jw[[0, 1, 3, 4]]), _bits((gg[:, None] * J)[[0, 1, 3, 4]]))


def test_continuity_across_the_switches():
    """d and g are continuous where the table changes path: |e| = 2^-6 (series / log1p), e = -0.5 (log1p / log), y -> 0 and
    mu = floor.  Neighbouring doubles on the two sides of a switch differ by the function's own slope times one spacing, and by
    the two paths' errors: within the sum of the two exact bounds, plus 4 ulp for the step itself."""
    y = np.array([0.37, 1.0, 12.0, 1e3, 7.7e5])
    for e0 in (PR.SWITCH, -PR.SWITCH, -0.5):
        lo, hi = np.nextafter(e0, -np.inf), np.nextafter(e0, np.inf)
        for ea, eb in ((lo, e0), (e0, hi)):
            ra, rb = ea * y, eb * y
            oa, ga, Da, ba = PR.apply(y, None, F, ra)
            ob, gb, Db, bb = PR.apply(y, None, F, rb)
            bda, bga = PR.exact_bounds(y, ra)
            bdb, bgb = PR.exact_bounds(y, rb)
            assert (np.abs(oa - ob) <= (bda + bdb + 4 * PR.U / abs(e0)) * np.abs(oa)).all(), e0
            assert (np.abs(ga - gb) <= (bga + bgb + 4 * PR.U / abs(e0)) * np.abs(ga)).all(), e0
        seen = {int(PR.apply(np.ones(1), None, F, np.array([ev]))[3][0]) for ev in (lo, e0, hi)}     # (y = 1: r / y is e itself)
        assert len(seen) == 2, (e0, seen)                            # the neighbours take the two paths
    # y -> 0 at a fixed model value mu: d^2 -> 2 mu, g -> 1 / sqrt(2 mu); the y > 0 rows differ from the y = 0 row by
    # O(y log(mu / y) / mu) relative
    mu = np.array([0.3, 2.0, 40.0])
    o0, g0, D0, b0 = PR.apply(np.zeros(3), None, F, mu)
    for yy in (1e-9, 1e-12, 1e-15):
        o1, g1, D1, b1 = PR.apply(np.full(3, yy), None, F, mu - yy)
        tol = 2.0 * yy * (1.0 + np.abs(np.log(mu / yy))) / mu
        assert (b1 == 3).all() and (np.abs(o1 - o0) <= tol * o0).all() and (np.abs(g1 - g0) <= tol * g0).all(), yy
    # mu = floor: on the floor and one spacing below it the extension continues d with slope g (C1): the values differ by g
    # times the step, to within the roundings of the extension; well below the floor out is linear in mu with slope g
    for yy in (0.0, 1.0, 250.0):
        ya = np.array([yy])
        r_on = np.array([F - yy])
        mu_on = float(r_on[0] + yy)
        r_below = np.array([np.nextafter(r_on[0], -np.inf)])
        o_on, g_on, D_on, b_on = PR.apply(ya, None, F, r_on)
        o_be, g_be, D_be, b_be = PR.apply(ya, None, F, r_below)
        low_on, low_be = PR.branches(ya, None, F, r_on)[1][0], PR.branches(ya, None, F, r_below)[1][0]
        assert mu_on >= F or low_on
        assert low_be
        step = abs((r_below[0] + yy) - F)
        assert abs(o_be[0] - o_on[0]) <= abs(g_be[0]) * (step + np.spacing(yy + F)) * (1 + 1e-6) + 8 * PR.U * abs(o_on[0]), yy
        assert abs(g_be[0] - g_on[0]) <= 1e-6 * abs(g_on[0]) + np.spacing(yy + F) * abs(g_on[0]) / F * 4
        far = PR.apply(ya, None, F, np.array([-3.0 - yy, -5.0 - yy]))
        assert far[1][0] == far[1][1] and abs((far[0][0] - far[0][1]) - 2.0 * far[1][0]) <= 8 * PR.U * abs(far[0][1])
        assert np.isfinite(far[0]).all() and (far[0] < 0).all() if yy > 0 else np.isfinite(far[0]).all()


def test_masks_and_nan_rules():
    y = np.array([3.0, 0.0, 5.0, 2.0, 1.0, 4.0])
    r = np.array([0.5, 1.5, np.nan, np.inf, -0.25, 2.0])
    w = np.array([1.0, 1.0, 0.0, 0.0, 1.0, 1.0])
    out, g, D, br = PR.apply(y, w, F, r)
    assert np.array_equal(_bits(out[2:4]), _bits(np.zeros(2))) and np.array_equal(_bits(g[2:4]), _bits(np.zeros(2)))   # +0.0, not -0.0
    assert (br[2:4] == 0).all() and np.isfinite(out[[0, 1, 4, 5]]).all()
    plain = PR.apply(y[[0, 1, 4, 5]], None, F, r[[0, 1, 4, 5]])
    for a, b in zip((out, g, D), plain[:3]):
        assert np.array_equal(_bits(a[[0, 1, 4, 5]]), _bits(b))      # an unmasked row is the row without a mask
    for bad_w in (0.5, 2.0, -1.0, np.nan, np.inf):
        o, gg, DD, b = PR.apply(np.array([3.0, 3.0]), np.array([bad_w, 1.0]), F, np.array([0.5, 0.5]))
        assert np.isnan(o[0]) and np.isnan(gg[0]) and not np.isnan(o[1])
    for bad_y in (-1.0, -1e-300, np.nan, np.inf):
        o, gg, DD, b = PR.apply(np.array([bad_y, 3.0]), None, F, np.array([0.5, 0.5]))
        assert np.isnan(o[0]) and np.isnan(gg[0]) and not np.isnan(o[1])
        o, gg, DD, b = PR.apply(np.array([bad_y, 3.0]), np.array([0.0, 1.0]), F, np.array([0.5, 0.5]))
        assert _bits(o[:1])[0] == 0 and _bits(gg[:1])[0] == 0        # the mask comes first: a masked row may hold anything
    for bad_f in (0.0, -1.0, np.nan, np.inf):
        for v in PR.apply(y, w, bad_f, r)[:3]:
            assert np.isnan(v).all()


def test_sum_of_squares_is_the_deviance():
    """sum out^2 = sum 2 [mu - y + y log(y / mu)], the deviance in 60-digit arithmetic at the model values mu = r + y the rows
    hold, above the floor: out is the root of D within the bound of d, so out^2 is within twice that, and one rounding of the
    square, of D; the sign of out is the sign of mu - y."""
    import decimal
    rng = np.random.default_rng(3)
    mu = np.exp(rng.uniform(np.log(0.05), np.log(500.0), 1500))
    y = rng.poisson(mu).astype(np.float64)
    r = mu - y
    out = PR.residual(y, None, F, r)
    bd = PR.exact_bounds(y, r)[0]
    assert (y == 0).any() and (y > 0).any() and (np.sign(out) == np.sign(r)).all()
    with decimal.localcontext() as c:
        c.prec = 60
        total_got = total_want = decimal.Decimal(0)
        for i in range(len(y)):
            Y, Rr = decimal.Decimal(float(y[i])), decimal.Decimal(float(r[i]))
            M = Y + Rr
            want = 2 * (M - Y + (Y * (Y / M).ln() if Y > 0 else 0))
            got = decimal.Decimal(float(out[i])) ** 2
            assert abs(got - want) <= decimal.Decimal(float(2 * bd[i] + PR.U)) * want, (i, y[i], r[i])
            total_got += got
            total_want += want
        assert abs(total_got - total_want) <= decimal.Decimal(float(2 * bd.max() + PR.U)) * total_want


def test_poisson_validation():
    import nonlin_amd as nl
    assert nl.Poisson().mu_floor == 2.0 ** -20 == PR.MU_FLOOR
    assert nl.Poisson(0.5).mu_floor == 0.5 and nl.Poisson(np.float64(1e-3)).mu_floor == 1e-3 and nl.Poisson(1).mu_floor == 1.0
    for bad in (0.0, -1.0, float("inf"), float("nan"), None, "low", "1.0", True, [1.0]):
        with pytest.raises(ValueError):
            nl.Poisson(bad)


def test_library_loads_and_refuses_device_work_without_a_handle():
    from nonlin_amd import _lib
    L = _lib.load()
    one = np.ones(16)
    p = one.ctypes.data_as(dp)
    o = _lib.default_options()
    out = C.c_void_p(7)
    fcn = C.cast(L.nlh_curve_device_fcn, _lib.DEVFCN)
    none = C.cast(None, _lib.DEVFCN)
    assert L.nlh_pois_wrap(None, None, None, F, fcn, none, None, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    assert L.nlh_pois_apply_batch(None, 1, 1, None, None, F, None, None, None, None) == NLH_ERR_BAD_HANDLE
    out = C.c_void_p(7)
    assert L.nlh_pois_model_create(None, None, p, None, F, C.byref(out)) == NLH_ERR_BAD_HANDLE and not out.value
    assert L.nlh_curve_fit_batch_pois(None, C.byref(o), 2, 1, 0, 1, 8, None, 0, None, None, 1, None, None, None, F, None, None, None, None,
                                      None, None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_curve_fit_batch_pois_h(None, C.byref(o), 2, 1, 0, 1, 8, p, 0, p, None, 1, None, None, None, F, p, p, None, None, None, None,
                                        None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_fit_batch_pois(None, C.byref(o), None, 1, 8, None, 0, None, None, 1, None, None, None, F, None, None, None, None, None,
                                     None, None, None) == NLH_ERR_BAD_HANDLE
    assert L.nlh_expr_fit_batch_pois_h(None, C.byref(o), None, 1, 8, p, 0, p, None, 1, None, None, None, F, p, p, None, None, None, None,
                                       None, None) == NLH_ERR_BAD_HANDLE
    # a malformed context is refused by the launchers before any launch (no device is touched: this runs without one)
    for fn in (L.nlh_pois_device_fcn, L.nlh_pois_device_jac):
        assert fn(None, None, 1, None, 2, None, 8, None) == NL_INVALID_INPUT_ERROR
        junk = (C.c_uint32 * 64)()
        assert fn(C.byref(junk), None, 1, None, 2, 1, 8, 1) == NL_INVALID_INPUT_ERROR
    L.nlh_pois_unwrap(None)


@pytest.mark.parametrize("analytic", [True, False])
@pytest.mark.parametrize("a", PC.AMPLITUDES)
def test_decay_family_on_the_reference_path(oracle, a, analytic):
    """The decay family on the oracle's lm_solve under default options, the restated transform as the callback: status 0 on
    every problem, no model value touches the floor, and the area rule sum mu = sum y within AREA_BOUND."""
    nprob = PC.PERT_NPROB
    t, y, xt, x0 = PC.decay_problems(a, nprob)
    touched, worst = [], 0.0
    for p in range(nprob):
        fcn, jac = PC.callbacks(t[p], y[p], "poisson", analytic, touched=touched)
        rc, xo, fo, ib = oracle.lm_solve(fcn, PC.M, PC.N, x0[p], jac=jac, opts=oracle.default_options())
        assert rc == 0, (a, analytic, p, rc)
        area = abs(R.model(R.EXPDECAY, PC.K, PC.B, xo, t[p]).sum() - y[p].sum()) / y[p].sum()
        worst = max(worst, float(area))
        assert area <= AREA_BOUND[a], (a, analytic, p, area)
    print(f"poisson area rule a ~ {a:g} {'analytic' if analytic else 'forward differences'}: worst |sum mu - sum y| / sum y = {worst:.3g}")
    assert not touched


def test_bias_study(oracle):
    """The README's table, re-measured on the oracle: 300 decays at the truth (50, 1, 0.5).  Asserted is the ordering only:
    the rate bias of weighted least squares exceeds three of its standard errors, the Poisson fit's is within three; and that
    tests/golden/pois_bias_study.json records what is measured here."""
    got = PC.bias_study(oracle)
    est = got["estimators"]
    for k, v in est.items():
        print(f"bias study {k}: k {100 * v['k_bias']:+.2f} % +- {100 * v['k_stderr']:.2f} % (scatter {v['k_scatter']:.3f}), "
              f"c {100 * v['c_bias']:+.1f} % +- {100 * v['c_stderr']:.1f} %")
        assert v["failed"] == 0
    assert abs(est["wls"]["k_bias"]) > 3 * est["wls"]["k_stderr"]
    assert abs(est["poisson"]["k_bias"]) <= 3 * est["poisson"]["k_stderr"]
    with open(PC.BIAS_GOLDEN) as fh:
        rec = json.load(fh)
    for k, v in est.items():
        for name, val in v.items():
            assert rec["estimators"][k][name] == pytest.approx(val, rel=1e-6, abs=1e-9), (k, name)


def test_perturbation_study(oracle):
    """What a last-bit change of log1p / log does to a fit, re-measured: tests/golden/pois_perturbation.json records at least
    what is measured here (it is what the GPU comparisons take their tolerance from), and not ten times more."""
    got = PC.perturbation_study(oracle)
    print("perturbation study, worst relative change of x: " + ", ".join(f"{k} {v:.3g}" for k, v in got["worst"].items()))
    with open(PC.PERT_GOLDEN) as fh:
        rec = json.load(fh)
    for key in ("analytic", "fd"):
        assert got[key] <= rec[key] * (1 + 1e-9) and rec[key] <= 10 * got[key], (key, got[key], rec[key])
    assert PC.recorded_tolerance(True) == 4 * rec["analytic"] and PC.recorded_tolerance(False) == 4 * rec["fd"]
