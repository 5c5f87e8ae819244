"""GPU tests of curve_guess (include/nonlin_hip_guess.h: nlh_curve_guess_batch).  Everything is bit for bit; the file uses no
tolerance.  The nonlinear stage against the numpy restatement (tests/guess_restatement.py) for the three kinds at the chunk
edges of the prefix sum and the LDS maximum, every K, B and smooth, both shared_t settings, with and without weights that
zero scattered rows and a ragged tail, alone and in a batch of 700; the linear stage against sep_restatement.qr_solve fed the
device's own curve Jacobian columns at (0, alpha) and its f0, so that the exp kinds need no tolerance; the flags, each with
neighbours that must not notice; curve_fit_batch(x0=None) as the composition it stands for, and a caller's x0 against what
the commit before computed (tests/golden/guess_parent_fit.npz); the error returns with a real handle.  There is one
workgroup form, so no form switch is exercised."""
import ctypes as C

import numpy as np
import pytest
import torch

import curve_restatement as R
import guess_cases as GC
import guess_restatement as G
import sep_restatement as SR
from nonlin_amd import _lib

pytestmark = pytest.mark.gpu

NL_INVALID_INPUT_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR = 201, 212
KINDS = {"gauss": R.GAUSS, "lorentz": R.LORENTZ, "expdecay": R.EXPDECAY}
M_EDGES = ("n", 63, 64, 65, 255, 256, 257, 512, 513, 8192)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _dev(ds, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(ds.device)


def _launch(ds, fcn, ctx, X, m, jac=False):
    """The curve launcher on one point per problem: F [nprob, m] or J [nprob, n, m]."""
    npts, n = X.shape
    dX, dprob = _dev(ds, X), _dev(ds, np.arange(npts), np.int32)
    out = torch.full((npts, n, m) if jac else (npts, m), np.nan, dtype=torch.float64, device=ds.device)
    stream = torch.cuda.current_stream(ds.device).cuda_stream
    rc = fcn(ds._ctxp(ctx), C.c_void_p(stream), npts, C.c_void_p(dprob.data_ptr()), n, C.c_void_p(dX.data_ptr()), m,
             C.c_void_p(out.data_ptr()))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy()


def make_data(kind, K, B, nprob, m, shared, weighted, seed):
    """t [m] or [nprob, m] (uneven steps when not shared), y of K components on a baseline with noise, w or None: scattered
    zeros and a ragged tail, at least n + 2 rows left wherever the data have that many."""
    rng = np.random.default_rng(seed)
    n = R.nparams(kind, K, B)
    if shared:
        t = np.linspace(0.25, 8.0, m) if kind == R.EXPDECAY else np.linspace(-5.0, 5.0, m)
        tt = np.tile(t, (nprob, 1))
    else:
        tt = np.cumsum(rng.uniform(0.5, 1.5, (nprob, m)), axis=1)
        tt = tt / tt[:, -1:] * (8.0 if kind == R.EXPDECAY else 10.0) - (0.0 if kind == R.EXPDECAY else 5.0)
        t = tt
    y = np.empty((nprob, m))
    for p in range(nprob):
        if kind == R.EXPDECAY:
            x = np.concatenate([[v for k in range(K) for v in (rng.uniform(50, 500), (1.5, 0.3)[k] * rng.uniform(0.8, 1.2))],
                                rng.uniform(-1, 1, B + 1) * 3.0 ** -np.arange(B + 1)])
        else:
            x = np.concatenate([[v for k in range(K) for v in (rng.uniform(20, 60), rng.uniform(-4, 4), rng.uniform(0.3, 0.8))],
                                rng.uniform(-1, 1, B + 1) * 3.0 ** -np.arange(B + 1)])
        y[p] = R.model(kind, K, B, x, tt[p]) + rng.standard_normal(m)
    w = None
    if weighted:
        w = rng.uniform(0.5, 2.0, (nprob, m))
        spare = m - (n + 2)
        for p in range(nprob):
            z = min(max(spare, 0), 1 + (p * 7) % 23)
            if z > 0:
                w[p, m - z:] = 0.0
            if spare > 8:
                w[p, rng.integers(0, m - z, 3)] = 0.0
    return t, y, w


def check_guess(ds, kind, K, B, nprob, m, shared, weighted, smooth, seed=1):
    """One call of curve_guess against the restatement: the nonlinear values, the flags, and the linear stage restated on the
    device's own Phi and f0."""
    n = R.nparams(kind, K, B)
    t, y, w = make_data(kind, K, B, nprob, m, shared, weighted, seed)
    dt, dy, dw = _dev(ds, t), _dev(ds, y), (_dev(ds, w) if w is not None else None)
    x, flag = ds.curve_guess(kind, dt, dy, ncomp=K, baseline=B, weights=dw, smooth=smooth)
    torch.cuda.synchronize()
    x, flag = x.cpu().numpy(), flag.cpu().numpy()
    lin, nl = G.lin_positions(kind, K, B)
    want = [G.nonlinear(kind, K, B, t if shared else t[p], y[p], None if w is None else w[p], smooth) for p in range(nprob)]
    alpha = np.stack([a for a, _ in want])
    wflag = np.array([f for _, f in want])
    what = (kind, K, B, nprob, m, shared, weighted, smooth)
    none = (wflag & G.NONE) != 0
    assert np.array_equal(_bits(x[:, nl]), _bits(alpha)), what
    assert np.array_equal(flag & G.NONE, wflag & G.NONE) and np.array_equal(flag & G.FALLBACK, wflag & G.FALLBACK), what
    assert np.array_equal(_bits(x[none]), _bits(np.full((int(none.sum()), n), np.nan))) and (flag[none] == G.NONE).all(), what
    # the linear stage on the device's own basis
    fcn, jac, ctx = ds.curve_launchers(kind, K, B, dt, dy, dw)
    P0 = np.zeros((nprob, n))
    P0[:, nl] = np.where(none[:, None], 1.0, alpha)                # (a problem that was not guessed: any finite point will do)
    J0, F0 = _launch(ds, jac, ctx, P0, m, jac=True), _launch(ds, fcn, ctx, P0, m)
    for p in np.flatnonzero(~none):
        c, rank, _, _, _ = SR.qr_solve(J0[p][lin].T, F0[p])
        assert np.array_equal(_bits(x[p, lin]), _bits(c)), what + (p,)
        assert bool(flag[p] & G.RANKDEF) == (rank < len(lin)), what + (p,)
    return x, flag


def _m_of(kind, K, B, m):
    return R.nparams(kind, K, B) if m == "n" else m


def _edge_cases():
    """Every m of M_EDGES for every kind; K, B, smooth, shared_t and the weights rotate so that each value of each meets
    each kind; nprob 3, 1 at some, never more than 3 at m = 8192."""
    out = []
    for kname, kind in KINDS.items():
        Ks = (1, 2) if kind == R.EXPDECAY else (1, 2, 3)
        for i, m in enumerate(M_EDGES):
            K, B, h = Ks[i % len(Ks)], (-1, 0, 1, 3)[(i + (i // 4)) % 4], (0, 2, 5)[(i + 1) % 3]
            out.append(pytest.param(kind, K, B, 1 if i % 4 == 3 else 3, m, i % 2 == 0, m != "n" and i % 3 != 0, h,
                                    id=f"{kname}-m{m}-K{K}-B{B}-h{h}"))
    return out


@pytest.mark.parametrize("kind,K,B,nprob,m,shared,weighted,smooth", _edge_cases())
def test_against_the_restatement_at_the_size_edges(ds, kind, K, B, nprob, m, shared, weighted, smooth):
    check_guess(ds, kind, K, B, nprob, _m_of(kind, K, B, m), shared, weighted, smooth)


@pytest.mark.parametrize("K,B,m", [(2, 0, 2048), (1, -1, 4600), (2, 3, 2102), (2, 3, 2103)])
def test_decay_regression_where_its_panel_leaves_the_lds(ds, K, B, m):
    """The regression's kernel keeps the panel [m, 2 K + B + 2] in LDS while it fits: 98 KB and 110 KB (above the 64 KB a kernel
    gets unasked), then the last m that fits beside the kernel's own 10 KB and the first that goes through global memory."""
    check_guess(ds, R.EXPDECAY, K, B, 2, m, True, m % 2 == 0, 2, seed=m)


@pytest.mark.parametrize("kname", sorted(KINDS))
def test_weighted_at_the_most_rows(ds, kname):
    """m = 8192 with zero weights: the compaction, and a smoothing window and prefix chunks that do not line up with the rows."""
    check_guess(ds, KINDS[kname], 2, 1, 2, G.MAX_M, False, True, 5, seed=8)


@pytest.mark.parametrize("kname", sorted(KINDS))
def test_every_K_B_smooth(ds, kname):
    """The whole product of K, B and smooth at m = 257 (two rows per chunk of the prefix sum, the last chunk short), three
    problems each, the weights and shared_t alternating."""
    kind = KINDS[kname]
    i = 0
    for K in ((1, 2) if kind == R.EXPDECAY else (1, 2, 3)):
        for B in (-1, 0, 1, 3):
            for h in (0, 2, 5):
                check_guess(ds, kind, K, B, 3, 257, i % 2 == 0, i % 3 == 0, h, seed=10 + i)
                i += 1


@pytest.mark.parametrize("kname", sorted(KINDS))
@pytest.mark.parametrize("weighted", [False, True])
def test_batch_of_700(ds, kname, weighted):
    """700 problems of 65 rows: the bits of a problem do not depend on the batch it is in."""
    kind = KINDS[kname]
    x, flag = check_guess(ds, kind, 2, 0, 700, 65, not weighted, weighted, 2, seed=5)
    t, y, w = make_data(kind, 2, 0, 700, 65, not weighted, weighted, 5)
    for p in (0, 350, 699):
        x1, f1 = ds.curve_guess(kind, _dev(ds, t if t.ndim == 1 else t[p:p + 1]), _dev(ds, y[p:p + 1]), ncomp=2, baseline=0,
                                weights=_dev(ds, w[p:p + 1]) if w is not None else None)
        assert np.array_equal(_bits(x1.cpu().numpy()[0]), _bits(x[p])) and int(f1[0]) == flag[p]


def test_weights_are_a_mask_for_the_nonlinear_stage(ds):
    """The nonlinear values with weights w equal those of the data with the zero-weight rows cut out."""
    kind, K, B, m = R.LORENTZ, 2, 0, 200
    t, y, w = make_data(kind, K, B, 1, m, True, True, 3)
    on = w[0] != 0
    _, nl = G.lin_positions(kind, K, B)
    xa, fa = ds.curve_guess(kind, _dev(ds, t), _dev(ds, y), ncomp=K, baseline=B, weights=_dev(ds, w))
    xb, fb = ds.curve_guess(kind, _dev(ds, t[on]), _dev(ds, y[:, on]), ncomp=K, baseline=B)
    assert np.array_equal(_bits(xa.cpu().numpy()[:, nl]), _bits(xb.cpu().numpy()[:, nl]))


# ---------------------------------------------------------------------------------------------------------------------
# the flags
# ---------------------------------------------------------------------------------------------------------------------
def _with_neighbours(ds, kind, K, B, t, y_special, t_special=None, w_special=None):
    """The special problem between two ordinary ones: (x, flag) of the three, after checking that the ordinary ones come out
    as they do in a batch without the special one."""
    m = len(t)
    _, yo, _ = make_data(kind, K, B, 2, m, True, False, 11)
    tt = np.tile(t, (3, 1))
    if t_special is not None:
        tt[1] = t_special
    y = np.stack([yo[0], y_special, yo[1]])
    w = None
    if w_special is not None:
        w = np.ones((3, m))
        w[1] = w_special
    x, flag = ds.curve_guess(kind, _dev(ds, tt), _dev(ds, y), ncomp=K, baseline=B, weights=_dev(ds, w) if w is not None else None)
    x2, flag2 = ds.curve_guess(kind, _dev(ds, tt[[0, 2]]), _dev(ds, y[[0, 2]]), ncomp=K, baseline=B,
                               weights=_dev(ds, w[[0, 2]]) if w is not None else None)
    x, flag, x2, flag2 = x.cpu().numpy(), flag.cpu().numpy(), x2.cpu().numpy(), flag2.cpu().numpy()
    assert np.array_equal(_bits(x[[0, 2]]), _bits(x2)) and np.array_equal(flag[[0, 2]], flag2)
    assert np.isfinite(x2).all() and (flag2 & G.NONE == 0).all()
    return x, flag


@pytest.mark.parametrize("kname", sorted(KINDS))
def test_flat_data_fall_back(ds, kname):
    kind = KINDS[kname]
    t = np.linspace(0.5, 6.5, 96)
    x, flag = _with_neighbours(ds, kind, 1, 0, t, np.full(96, 3.0))
    assert flag[1] & G.FALLBACK and not flag[1] & G.NONE
    _, nl = G.lin_positions(kind, 1, 0)
    assert np.array_equal(_bits(x[1, nl]), _bits(G.nonlinear(kind, 1, 0, t, np.full(96, 3.0))[0]))
    if kind == R.EXPDECAY:
        assert x[1, 1] == 2.0 / 6.0


def test_identical_positions_are_rank_deficient(ds):
    """One broad Gaussian and three components asked for: the first mask (1.5 FWHM either side) leaves no live row, so the
    second and the third component both take the documented fallback at t'[0] -- two identical columns, the later one dead."""
    t = np.linspace(-5.0, 5.0, 128)
    y = R.model(R.GAUSS, 1, -1, np.array([10.0, 0.0, 4.0 / G.FWHM_PER_SIGMA]), t)
    x, flag = _with_neighbours(ds, R.GAUSS, 3, -1, t, y)
    assert flag[1] == G.FALLBACK | G.RANKDEF
    assert x[1, 4] == x[1, 7] == t[0] and x[1, 5] == x[1, 8] == 0.5 * (t[-1] - t[0]) / G.FWHM_PER_SIGMA
    assert _bits(x[1, 6]) == _bits(0.0) and x[1, 3] != 0.0                                  # the dead amplitude is +0.0


@pytest.mark.parametrize("kname", sorted(KINDS))
@pytest.mark.parametrize("why", ["nan_y", "inf_t", "descending_t", "repeated_t", "too_few_rows"])
def test_not_guessed(ds, kname, why):
    kind = KINDS[kname]
    K, B, m = 2, 0, 80
    n = R.nparams(kind, K, B)
    t = np.linspace(0.5, 6.5, m)
    y = make_data(kind, K, B, 1, m, True, False, 12)[1][0]
    ts, ws = t.copy(), None
    if why == "nan_y":
        y[17] = np.nan
    elif why == "inf_t":
        ts[m - 1] = np.inf
    elif why == "descending_t":
        ts[30], ts[31] = t[31], t[30]
    elif why == "repeated_t":
        ts[40] = t[39]
    else:
        ws = np.where(np.arange(m) < n - 1, 1.0, 0.0)
    x, flag = _with_neighbours(ds, kind, K, B, t, y, t_special=ts, w_special=ws)
    assert flag[1] == G.NONE and np.array_equal(_bits(x[1]), _bits(np.full(n, np.nan)))


def test_a_bad_value_in_a_zero_weight_row_is_not_seen(ds):
    t = np.linspace(0.5, 6.5, 80)
    y = make_data(R.EXPDECAY, 1, 0, 1, 80, True, False, 13)[1][0]
    y[17] = np.nan
    x, flag = _with_neighbours(ds, R.EXPDECAY, 1, 0, t, y, w_special=np.where(np.arange(80) == 17, 0.0, 1.0))
    _, nl = G.lin_positions(R.EXPDECAY, 1, 0)
    assert flag[1] == 0 and np.isfinite(x[1, nl]).all()


# ---------------------------------------------------------------------------------------------------------------------
# curve_fit_batch
# ---------------------------------------------------------------------------------------------------------------------
def test_x0_none_is_the_composition(ds):
    """64 problems of study (b): curve_fit_batch(x0=None) equals curve_fit_batch(x0=curve_guess(...)[0]), every output."""
    kind, K, B, t, y, _ = GC.parent_fit_case()
    dt, dy = _dev(ds, t), _dev(ds, y)
    x0, flag = ds.curve_guess(kind, dt, dy, ncomp=K, baseline=B)
    assert int((flag & G.NONE).sum()) == 0
    a = ds.curve_fit_batch(kind, dt, dy, None, ncomp=K, baseline=B)
    b = ds.curve_fit_batch(kind, dt, dy, x0, ncomp=K, baseline=B)
    for u, v in zip(a[:6], b[:6]):
        assert np.array_equal(u.cpu().numpy().view(np.uint8), v.cpu().numpy().view(np.uint8))
    assert a[6] == b[6] and a[7] == b[7]
    with pytest.raises(ValueError):
        ds.curve_fit_batch(kind, dt, dy, None, ncomp=K, baseline=B, pmap=_lib.ParamMap(5, fixed=[4]))


def test_a_caller_s_x0_goes_the_way_it_went(ds):
    """The same call on the commit before curve_guess, recorded in tests/golden/guess_parent_fit.npz."""
    got = GC.run_parent_fit(ds)
    rec = np.load(GC.PARENT_GOLDEN)
    assert sorted(rec.files) == sorted(got)
    for k in rec.files:
        assert rec[k].dtype == got[k].dtype and np.array_equal(rec[k].view(np.uint8), got[k].view(np.uint8)), k


# ---------------------------------------------------------------------------------------------------------------------
# the error returns
# ---------------------------------------------------------------------------------------------------------------------
def test_error_returns_with_a_real_handle(ds):
    m = 64
    t, y = _dev(ds, np.linspace(0.0, 1.0, m)), _dev(ds, np.ones((2, m)))
    x = torch.full((2, 16), 7.0, dtype=torch.float64, device=ds.device)
    fl = torch.full((2,), 9, dtype=torch.int32, device=ds.device)

    def call(kind=0, K=1, B=0, nprob=2, mm=m, tp=t.data_ptr(), yp=y.data_ptr(), smooth=2, xp=x.data_ptr()):
        return ds.lib.nlh_curve_guess_batch(ds.h.ptr, kind, K, B, nprob, mm, tp, 1, yp, None, smooth, xp, fl.data_ptr())
    for bad in (dict(kind=5), dict(K=0), dict(B=9), dict(nprob=-1), dict(mm=0), dict(tp=None), dict(yp=None), dict(xp=None),
                dict(smooth=-1), dict(mm=G.MAX_M + 1), dict(kind=1, K=31, B=1, mm=128), dict(kind=2, K=3)):
        assert call(**bad) == NL_INVALID_INPUT_ERROR, bad
    assert call(kind=0, K=2, B=0, mm=6) == NL_UNDERDEFINED_PROBLEM_ERROR
    assert call(nprob=0) == 0
    torch.cuda.synchronize()
    assert (x == 7.0).all() and (fl == 9).all()                              # a refused call writes nothing
    assert ds.lib.nlh_curve_guess_batch(None, 0, 1, 0, 2, m, t.data_ptr(), 1, y.data_ptr(), None, 2, x.data_ptr(), None) == -3
    # the flags may be left out, and the host twin gives the same bits
    tn, yn, _ = make_data(R.LORENTZ, 1, 1, 2, m, True, False, 14)
    dtn, dyn = _dev(ds, tn), _dev(ds, yn)
    xd, fd = ds.curve_guess(R.LORENTZ, dtn, dyn, ncomp=1, baseline=1)
    xn = torch.empty((2, 5), dtype=torch.float64, device=ds.device)
    ds._call("nlh_curve_guess_batch", R.LORENTZ, 1, 1, 2, m, dtn.data_ptr(), 1, dyn.data_ptr(), None, 2, xn.data_ptr(), None)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(xn.cpu().numpy()), _bits(xd.cpu().numpy()))
    xh, fh = np.empty((2, 5)), np.empty(2, dtype=np.int32)
    ds._call("nlh_curve_guess_batch_h", R.LORENTZ, 1, 1, 2, m, tn.ctypes.data_as(_lib.c_double_p), 1, yn.ctypes.data_as(_lib.c_double_p),
             None, 2, xh.ctypes.data_as(_lib.c_double_p), fh.ctypes.data_as(_lib.c_int32_p))
    assert np.array_equal(_bits(xh), _bits(xd.cpu().numpy())) and np.array_equal(fh, fd.cpu().numpy())
