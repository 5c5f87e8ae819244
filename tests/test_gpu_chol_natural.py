"""The factorisation kernels of the normal-equations policy (NLH_FACTOR_AUTO) on their own, at the sizes where their
code changes path: k_chol_nopiv and k_chol_mc_* through the stage-level entry nlh_chol_natural (the solver's launches on
caller-supplied G and g), k_chol_factor through nlh_chol_factor, ne_recover_signs through nlh_ne_signs.  The references
and the entry-by-entry bounds are in tests/chol_cases.py.

Where the edges come from (nlh_kernels_factor.h unless another file is named; NB = 16):

  k_chol_nopiv
    * `for (jb = 0; jb < n; jb += NB)`, `nbk = min(NB, n - jb)`: n = 1, 2, 15 no full block; 16 exactly one; 17 one block
      plus a last block of one; 31, 32, 33 the same one block further.  A last block of one column has an empty block row
      but the gradient (`k <= n`), and no trailing tile.
    * `factor_threads(n) = n >= 96 ? 1024 : 256` (nlh_internal.h): 95 | 96, 97.
    * chol_nopiv_threads (nlh_lm.hip): 512 threads when factor_threads is 1024 and more than 256 problems are active:
      300 problems at n = 100.
    * the trailing tiles, `nt = (n - t0 + 15) / 16`, `ntile = nt (nt + 1) / 2`, a wave per tile: n = 191 (ntile = 66 at
      the first step: more tiles than the 16 waves) and 529 (nt = 33 = 528 + 1 columns: a last tile column of one).
    * block row `for (k = jb + nbk + tid; k <= n; k += BS)`: a second trip from n - 16 >= 1024; n = 1109 has it.
    * chol_nopiv_lds (nlh_lm.hip) = 8 (17 n + 336) B <= 150 KB = 153,600: n = 1109 asks 153,512 B, n = 1110 153,648 B:
      NLH_ARRAY_SIZE_ERROR.
  k_chol_mc_begin / _step / _end
    * chol_mc_serves (nlh_lm.hip): n >= 192; 191 is refused for this form.
    * `vec = (nbk == NB) && ((n & 1) == 0)`: an odd n loads the block row with scalar loads at every step (193, 207, 209,
      513, 527, 529, 1109), an even n with double2 loads but for a partial last block (192, 208, 512, 528).
    * 207, 208, 209: a last block of fifteen columns, none (thirteen full blocks), and of one.
    * prefetched tiles: 512-thread workgroups have nw = 8 waves, NWG = 32, `tix = 1 + wg nw + wid + u NWG nw`, u < TPW = 2:
      tiles 1 .. 512 (tile 0 is the look-ahead's).  The tail `for (tix = 1 + wg nw + wid + TPW NWG nw; tix < ntile; ...)`
      runs once ntile > 513, i.e. nt >= 32 (nt = 31: 496 tiles, nt = 32: 528 tiles -- the 528 of the source's comment is
      this tile count, not an n).  At the first step t0 = 16 and nt = ceil((n - 16) / 16): nt = 31 up to n = 512, nt = 32
      from n = 513.  So 512 | 513.
    * copy-back of the previous panel, `kcb = pj + tid`, `for (k = kcb + BS; k < n; k += BS)` with BS = 512 and pj = 0 at
      step 1: columns beyond the first trip exist from n = 513.  Again 512 | 513.
    * block row `k1 = t0 + tid`, `for (k = k1; k < kend; k += BS)`, kend = n (n + 1 in the gradient's workgroup), t0 = 16
      at the first step: 527 everything in the first trip; 528 the gradient column (k = n = 528) in a second trip; 529 the
      matrix column 528 too.
    * k_chol_mc_end copies the last block with `for (k = pj + tid; k < n; k += BS)`, n - pj <= 16 < BS: it has no second trip
      at any n; its 1024 threads and LDS row of n doubles are exercised at every size, the largest at n = 1109.
    * two side buffers by step parity: every size here has more than two steps.
  k_chol_factor: factor_threads 95 | 96; CW = 8 columns per wave and trip: n = 1, 2, 9; 257 beyond the existing tests' 128.
  ne_recover_signs (nlh_kernels_lm.h): `for (; k + 8 <= c; k += 8)` the unrolled dot from column 8: n = 7, 8, 9;
    CG = 4 column groups per wave: n = 1, 2, 3; lmpar_threads 256 | 512 at n = 64 | 65, 512 | 1024 at 128 | 129; 200.

sqrt_rsqrt (nlh_common.h), the derivation of E_R.  y = rsq(x) = (1 + delta) / sqrt(x), |delta| <= 2^-20 is all that is
needed (the hardware estimate is good to about 2^-24).  Write g_i = sqrt(x)(1 + b_i), h_i = (1 + a_i) / (2 sqrt(x)); u = 2^-53,
every rho below is one rounding, |rho| <= u.
    g0 = x y (1 + rho1), h0 = y / 2 exactly:                         b0 - a0 = rho1
    e0 = fma(-h0, g0, 1/2) = -(a0 + b0) / 2 to second order (its own rounding is relative to e0: below 2^-72)
    g1 = g0 (1 + e0)(1 + rho2), h1 = h0 (1 + e0)(1 + rho3):         a1, b1 = O(delta^2) <= 2^-39, b1 - a1 = rho1 + rho2 - rho3
    e1 = -(a1 + b1) / 2 + O(2^-78)
    h2 = h1 (1 + e1)(1 + rho5):  a2 = a1 - (a1 + b1) / 2 + rho5 + O(2^-78) = (a1 - b1) / 2 + rho5,  |a2| <= 2.5 u + O(2^-78)
r = 2 h2 exactly, so |r - 1 / sqrt(x)| <= 2.5 u / sqrt(x) (1 + tiny) <= 2.5 ulp, and against the correctly rounded
1 / sqrt(x) (itself within 1/2 ulp) a whole number of ulps: E_R = 3.  g2 = sqrt(x)(1 + b2) with |b2| <= 2.5 u likewise, and
the closing correction s = fma(x - g2^2, h2, g2) = sqrt(x)(1 + O(u^2)) rounded once: within 1 ulp (1/2 but for near-ties).
"""
import hashlib

import numpy as np
import pytest
import torch

import chol_cases as CC

pytestmark = pytest.mark.gpu
NLH_ARRAY_SIZE_ERROR = 202
LD = CC.LD


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _stack(problems):
    G = np.stack([p[0] for p in problems])
    g = np.stack([p[1] for p in problems])
    return G, g


def _natural(ds, G, g, form, tol=0.0):
    """Runs one form on host arrays G [nprob, n, n] (symmetric), g [nprob, n].  Returns host arrays
    (Rfull [p][r, c], qtf, acnorm, ipvt, info)."""
    Gd = torch.from_numpy(np.ascontiguousarray(G)).cuda()
    gd = torch.from_numpy(np.ascontiguousarray(g)).cuda()
    G0 = Gd.clone()
    R, ipvt, acnorm, qtf, info = ds.chol_natural(Gd, gd, pivot_tol=tol, form=form)
    torch.cuda.synchronize()
    assert torch.equal(Gd, G0) or bool(torch.isnan(G0).any())          # the input is not modified
    return (R.cpu().numpy().transpose(0, 2, 1), qtf.cpu().numpy(), acnorm.cpu().numpy(), ipvt.cpu().numpy(),
            info.cpu().numpy())


_verdicts = {}                                          # identical bits need no second longdouble product


def _check(tag, n, Rfull, qtf, acnorm, ipvt, G, g):
    h = hashlib.sha1()
    for a in (Rfull, qtf, acnorm, G, g):
        h.update(np.ascontiguousarray(a).tobytes())
    key = (n, h.hexdigest())
    if key not in _verdicts:
        _verdicts[key] = CC.check_natural(Rfull, qtf, acnorm, ipvt, G, g, what=tag)
    else:
        CC.assert_structure(Rfull, G, acnorm, ipvt, what=tag)
    return _verdicts[key]


# ---- sqrt_rsqrt -----------------------------------------------------------------------------------------------------------------
def test_sqrt_rsqrt_through_tiny_factorisations(ds):
    """n = 1: R = s(x); n = 2 with G = [[x, 1], [1, 2 / x + 1]]: R12 = 1 * r(x) exactly.  x = 2^-500 .. 2^500 and 4096
    random mantissas at random exponents of that range, one batched call per n."""
    rng = np.random.default_rng(7)
    x = np.concatenate([np.ldexp(1.0, np.arange(-500, 501)),
                        np.ldexp(1.0 + rng.random(4096), rng.integers(-500, 501, 4096)),
                        np.ldexp(np.nextafter(2.0, 1.0), np.arange(-500, 501, 50)),      # all-ones mantissas
                        np.ldexp(np.nextafter(1.0, 2.0), np.arange(-499, 501, 50))])
    N = len(x)
    G1 = x.reshape(N, 1, 1)
    R1, q1, acn1, ip1, info1 = _natural(ds, G1, np.ones((N, 1)), 0)
    G2 = np.empty((N, 2, 2))
    G2[:, 0, 0] = x
    G2[:, 0, 1] = G2[:, 1, 0] = 1.0
    G2[:, 1, 1] = 2.0 / x + 1.0
    R2, q2, acn2, ip2, info2 = _natural(ds, G2, np.ones((N, 2)), 0)
    assert not info1.any() and not info2.any()
    s, r = R1[:, 0, 0], R2[:, 0, 1]
    assert _same_bits(R2[:, 0, 0], s)                   # the same function of the same x
    xl = x.astype(LD)
    sref, rref = np.sqrt(xl), 1 / np.sqrt(xl)

    def ulps(dev, ref):
        rd = ref.astype(np.float64)                     # the correctly rounded value (but for one double rounding in 2^11)
        return np.abs(dev.astype(LD) - ref) / np.spacing(rd), np.abs(dev - rd) / np.spacing(rd)
    s_true, s_rn = ulps(s, sref)
    r_true, r_rn = ulps(r, rref)
    print(f"sqrt_rsqrt over {N} arguments: s max {float(s_true.max()):.3f} ulp from sqrt(x), {int(s_rn.max())} ulp from its "
          f"rounding ({int((s_rn != 0).sum())} arguments not correctly rounded); r max {float(r_true.max()):.3f} ulp from "
          f"1/sqrt(x), {int(r_rn.max())} ulp from its rounding; histogram of r's ulps {np.bincount(r_rn.astype(int)).tolist()}")
    assert s_rn.max() <= 1
    assert r_rn.max() <= CC.E_R
    assert CC.E_R <= 4


# ---- k_chol_nopiv ------------------------------------------------------------------------------------------------------------
NOPIV_N = [1, 2, 15, 16, 17, 31, 32, 33, 95, 96, 97, 191, 529, 1109]


@pytest.mark.parametrize("n", NOPIV_N)
def test_single_workgroup_form_against_the_helpers(ds, n):
    G, g = CC.batch(n, 3)
    R, qtf, acn, ip, info = _natural(ds, G, g, 0)
    assert not info.any(), info
    for p in range(3):
        rb, rg = _check(f"nopiv n={n} p={p}", n, R[p], qtf[p], acn[p], ip[p], G[p], g[p])
        print(f"nopiv n={n} p={p}: backward {rb:.2f}, gradient {rg:.2f}, bound {CC.gamma_units(n)}")


def test_single_workgroup_form_512_threads(ds):
    """300 problems at n = 100: factor_threads(100) = 1024 and more than 256 active problems, so the solver's rule
    (chol_nopiv_threads) gives 512-thread workgroups."""
    n, nprob = 100, 300
    G, g = _stack([CC.problem(n, p) for p in range(nprob)])
    R, qtf, acn, ip, info = _natural(ds, G, g, 0)
    assert not info.any()
    worst = max(_check(f"nopiv 512 threads p={p}", n, R[p], qtf[p], acn[p], ip[p], G[p], g[p]) for p in range(nprob))
    print(f"nopiv n=100 x 300 (512 threads): backward {worst[0]:.2f}, bound {CC.gamma_units(n)}")
    # the same problems three at a time take 1024 threads: thread-per-column and wave-per-tile work in another
    # distribution, the same operations on every entry
    R3, q3, a3, i3, info3 = _natural(ds, G[:3], g[:3], 0)
    assert _same_bits(R3, R[:3]) and _same_bits(q3, qtf[:3])


@pytest.mark.parametrize("n,form", [(1110, 0), (1110, 1), (191, 1), (3000, 0)])
def test_sizes_the_natural_forms_do_not_serve(ds, n, form):
    f64 = dict(dtype=torch.float64, device=ds.device)
    G = torch.eye(n, **f64).unsqueeze(0).contiguous()
    g = torch.ones((1, n), **f64)
    R = torch.full((1, n, n), -7.0, **f64)
    qtf = torch.full((1, n), -7.0, **f64)
    acn = torch.full((1, n), -7.0, **f64)
    ip = torch.full((1, n), -7, dtype=torch.int32, device=ds.device)
    info = torch.full((1,), -7, dtype=torch.int32, device=ds.device)
    rc = ds.lib.nlh_chol_natural(ds.h.ptr, 1, n, G.data_ptr(), g.data_ptr(), 0.0, form, R.data_ptr(), ip.data_ptr(),
                                 acn.data_ptr(), qtf.data_ptr(), info.data_ptr())
    torch.cuda.synchronize()
    assert rc == NLH_ARRAY_SIZE_ERROR
    assert bool((R == -7.0).all()) and bool((qtf == -7.0).all()) and bool((acn == -7.0).all())
    assert bool((ip == -7).all()) and int(info[0]) == -7


# ---- k_chol_mc_* -------------------------------------------------------------------------------------------------------------
MC_N = [192, 193, 207, 208, 209, 512, 513, 527, 528, 529, 1109]


@pytest.mark.parametrize("nprob", [1, 3, 32])
@pytest.mark.parametrize("n", MC_N)
def test_multi_cu_form_same_bits_and_against_the_helpers(ds, n, nprob):
    """R (the whole array), qtf, acnorm, ipvt and info of the two forms bit for bit, for every problem; the helpers on
    the shared bits: every problem of a batch of up to three, and of the 32 the first three and the last (the first and
    the last above n = 600, a longdouble product costing a second there) -- the others are held by the bitwise
    comparison with a form that passes the helpers on its first problems through the same code."""
    G, g = CC.batch(n, nprob)
    R0, q0, a0, i0, info0 = _natural(ds, G, g, 0)
    R1, q1, a1, i1, info1 = _natural(ds, G, g, 1)
    assert not info0.any() and not info1.any(), (info0, info1)
    for p in range(nprob):
        assert _same_bits(R1[p], R0[p]), (n, p, "R", int((_bits(R1[p]) != _bits(R0[p])).sum()))
    assert _same_bits(q1, q0) and _same_bits(a1, a0) and np.array_equal(i1, i0)
    which = range(nprob) if nprob <= 3 else ((0, 1, 2, nprob - 1) if n <= 600 else (0, nprob - 1))
    for p in which:
        rb, rg = _check(f"mc n={n} nprob={nprob} p={p}", n, R1[p], q1[p], a1[p], i1[p], G[p], g[p])
        print(f"mc n={n} nprob={nprob} p={p}: backward {rb:.2f}, gradient {rg:.2f}, bound {CC.gamma_units(n)}")


# ---- bad pivots --------------------------------------------------------------------------------------------------------------
TOL = 1e-8
BAD_CASES = [
    # n, column j0 of each of three problems (None: a regular problem), forms
    (209, (5, None, 208), (0, 1)),      # first block (the begin kernel's); the last block, of one column
    (209, (16, 31, 100), (0, 1)),       # first and last column of the first block the look-ahead factors; a middle block
    (200, (195, None, 32), (0, 1)),     # inside a last block of eight; a block's first column
    (529, (528, 527, None), (0, 1)),    # the last block of one column behind 33 full ones; a block's last column
    (33, (32, None, 17), (0,)),         # below the multi-CU form's range
    (20, (17, 3, None), (0,)),
]


@pytest.mark.parametrize("n,j0s,forms", BAD_CASES)
def test_bad_pivot_index(ds, n, j0s, forms):
    """Column j0 of J an exact copy of column j0 // 2: the Schur diagonal at j0 is zero but for rounding, far below
    pivot_tol * acnorm^2 with pivot_tol = 1e-8, and every earlier one far above it."""
    probs = [CC.problem(n, 10 + p) if j0 is None else CC.singular_problem(n, 10 + p, j0, j0 // 2) for p, j0 in enumerate(j0s)]
    G, g = _stack(probs)
    want = []
    unit = CC.gamma_units(n) * CC.U                     # the rounding a computed Schur diagonal can carry, relative to G[j, j]
    for p, j0 in enumerate(j0s):
        Rr, d, info = CC.ref_chol(G[p], pivot_tol=TOL)
        assert info == (0 if j0 is None else j0 + 1)
        last = n if info == 0 else info
        dg = np.diagonal(G[p]).astype(LD)
        margin = np.abs(d[:last] - LD(TOL) * dg[:last]) / (LD(unit) * dg[:last])
        assert margin.min() >= 1e3, (p, float(margin.min()))           # no decision hangs on rounding
        want.append(info)
    out = {f: _natural(ds, G, g, f, tol=TOL) for f in forms}
    for f in forms:
        R, qtf, acn, ip, info = out[f]
        assert info.tolist() == want, (f, info.tolist(), want)
        for p, j0 in enumerate(j0s):
            if j0 is None:
                _check(f"bad-pivot batch n={n} p={p}", n, R[p], qtf[p], acn[p], ip[p], G[p], g[p])
            else:
                CC.assert_structure(R[p], G[p], acn[p], ip[p], what=f"bad pivot form {f} p={p}")
    if len(forms) == 2:
        assert np.array_equal(out[0][4], out[1][4]) and _same_bits(out[0][2], out[1][2])
        for p, j0 in enumerate(j0s):
            if j0 is None:
                assert _same_bits(out[0][0][p], out[1][0][p]) and _same_bits(out[0][1][p], out[1][1][p])


def test_nan_input_is_flagged(ds):
    """What a NaN Jacobian produces: a NaN above the diagonal reaches the Schur diagonal of its column, a NaN on the
    diagonal is one; both forms flag that column and return, the problems next to them are untouched by it."""
    n = 209
    G, g = _stack([CC.problem(n, 20 + p) for p in range(3)])
    G = G.copy()
    G[1, 7, 9] = G[1, 9, 7] = np.nan                    # enters R(7, 9), then the pivot of column 9
    G[2, 150, 150] = np.nan
    for form in (0, 1):
        R, qtf, acn, ip, info = _natural(ds, G, g, form)
        assert info.tolist() == [0, 10, 151], (form, info)
        _check(f"nan batch form {form}", n, R[0], qtf[0], acn[0], ip[0], G[0], g[0])


# ---- k_chol_factor -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 9, 95, 96, 97, 257])
def test_pivoted_form_order_and_identities(ds, n):
    nprob = 3
    G, g = _stack([CC.problem(n, 30 + p) for p in range(nprob)])
    Gd = torch.from_numpy(G).cuda()
    gd = torch.from_numpy(g).cuda()
    ipvt, acnorm, qtf, info = ds.chol_factor(Gd, gd)
    torch.cuda.synchronize()
    assert not info.cpu().numpy().any()
    Rall, ipvt, acnorm, qtf = Gd.cpu().numpy().transpose(0, 2, 1), ipvt.cpu().numpy(), acnorm.cpu().numpy(), qtf.cpu().numpy()
    for p in range(nprob):
        perm, Rref, margin = CC.ref_chol_pivoted(G[p])
        assert margin >= 1e-6, (p, margin)              # no tie a rounding could flip
        assert np.array_equal(ipvt[p], perm), (p, ipvt[p], perm)
        want = np.sqrt(np.maximum(np.diagonal(G[p]), 0.0))
        assert _same_bits(acnorm[p], want)
        # true divisions and square roots: no reciprocal term in the bound
        rb = CC.assert_backward(Rall[p], G[p][np.ix_(perm, perm)], c=0, what=f"pivoted n={n} p={p}")
        rg = CC.assert_gradient(Rall[p], qtf[p], g[p][perm], c=0, what=f"pivoted n={n} p={p}")
        print(f"pivoted n={n} p={p}: backward {rb:.2f}, gradient {rg:.2f}, bound {CC.gamma_units(n, 0)}, margin {margin:.2e}")


# ---- ne_recover_signs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 37])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 64, 65, 128, 129, 200])
def test_sign_recovery_against_lmfactor(ds, oracle, n, extra):
    m = n + extra
    Jh, fh = CC.wellcond_jac(m, n, 40)
    J = torch.from_numpy(np.ascontiguousarray(Jh.T)).cuda().unsqueeze(0).contiguous()       # [1, n, m]
    f = torch.from_numpy(fh).cuda().unsqueeze(0).contiguous()
    G, g = ds.gram(J, f)
    ipvt, acnorm, qtf, info = ds.chol_factor(G, g)
    torch.cuda.synchronize()
    assert int(info[0]) == 0
    R0, q0 = G[0].cpu().numpy().T.copy(), qtf[0].cpu().numpy().copy()
    sign = ds.ne_signs(J, ipvt, G, qtf)
    torch.cuda.synchronize()
    R1, q1, sign = G[0].cpu().numpy().T, qtf[0].cpu().numpy(), sign[0].cpu().numpy()

    a, ip, rdiag, acn = oracle.lmfactor(np.asfortranarray(Jh))
    assert np.array_equal(ipvt[0].cpu().numpy(), ip)
    # the pivot entry Householder saw at step j, relative to its column's norm: the reflector's leading entry is
    # |a_jj| / norm + 1 (lmfactor :644-646)
    lead = np.array([a[j, j] - 1.0 for j in range(n)])
    assert lead.min() >= 1e-6, lead.min()               # no sign is a coin toss
    want = np.sign(rdiag)
    assert np.array_equal(np.sign(np.diagonal(R1)), want)
    assert np.array_equal(sign, want)
    il = np.tril_indices(n, -1)
    assert _same_bits(R1[il], R0[il])                   # below the diagonal: untouched
    for i in range(n):
        assert _same_bits(R1[i, i:], want[i] * R0[i, i:]), i
    assert _same_bits(q1, want * q0)
    Ro = np.triu(a[:n, :n], 1) + np.diag(rdiag)
    np.testing.assert_allclose(np.triu(R1), Ro, rtol=0, atol=1e-11 * np.abs(Ro).max())
    w = fh.copy()                                       # qtf: the reflectors applied to f on the host
    for j in range(n):
        if a[j, j] != 0.0:
            t = -np.dot(a[j:, j], w[j:]) / a[j, j]
            w[j:] += a[j:, j] * t
    np.testing.assert_allclose(q1, w[:n], rtol=0, atol=1e-11 * np.abs(w).max())
    if n >= 8:
        assert (want > 0).any() and (want < 0).any()    # both signs occur: the recovery is not a constant
