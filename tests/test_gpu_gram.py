"""G = J^T J on the fp64 MFMA and g = J^T f (nlh_kernels_gram.h, launch_gram, stage entry nlh_gram / DeviceSolver.gram)
at the size edges of each of its four kernel forms.  The CPU oracle has no such operation and the MFMA's internal order
is not a reference's, so the family is held three ways instead:

1. exact-integer data, on which every correct kernel, whatever its order of summation, agrees with the host's float64
   product to the bit (gram_cases.int_data explains why);
2. real-valued data spanning 24 decades against the derived componentwise bound
   |G - Gref| <= (m + nsplit + 2) 2^-53 |J|^T |J| with a reference of higher precision (gram_cases.bound_violations);
3. structure: batch invariance, NaN containment, no stray writes, f = NULL, symmetry, repeatability, and the bits of
   the forms against each other (NLH_GRAM_TRI=0, NLH_GRAM512=0 send a shape to the block kernel).

Which form a shape takes is asserted through nonlin_amd.device.gram_plan -- the function the launch dispatches through --
before anything is compared, so a moved threshold fails here instead of silently testing another kernel."""
import pytest
import torch

import gram_cases as GC
from nonlin_amd.device import gram_plan

pytestmark = pytest.mark.gpu

# one shape per form for the structural checks (n, [m]): n is no multiple of 16 and leaves several columns in the last
# partial tile; m = 1025 is two splits, m = 1024 the triangle forms' direct path (one split, no reduce)
FORM_SHAPES = [("block", 70, 1025), ("tri8", 117, 1024), ("tri8", 117, 1025), ("tri16", 245, 1024), ("tri16", 245, 1025),
               ("512", 389, 1025)]
SENTINEL = -12345.675          # no integer, so no entry of an exact-integer G or g


def _id(case):
    return "%s-n%d-m%d" % case


def _assert_plan(form, m, n):
    assert gram_plan(m, n) == GC.expected_plan(form, m), (form, m, n)


def _poison(ds, nprob, m, n):
    """Fill the library's split-K slabs for this shape with NaN, so that an entry the next launch fails to write cannot be
    covered by what an earlier launch of the same shape -- the other form of a comparison, say -- left there.  A launch
    on all-NaN data, always by the block kernel (every form writes the same slabs): it does not lean on the form under test."""
    J = torch.full((nprob, n, m), float("nan"), dtype=torch.float64, device="cuda")
    with GC.env(NLH_GRAM512="0", NLH_GRAM_TRI="0"):
        ds.gram(J, J[:, 0, :].contiguous())
        torch.cuda.synchronize()


def _run_exact(ds, form, n, m, nprob=1, seed=1):
    _assert_plan(form, m, n)
    J, f = GC.int_data(nprob, m, n, seed + 7 * n + m)
    Gref, gref = GC.cpu_product(J, f)
    Jd, fd = J.cuda(), f.cuda()
    _poison(ds, nprob, m, n)
    G, g = ds.gram(Jd, fd)
    G2, g2 = ds.gram(Jd, fd)
    G, g, G2, g2 = G.cpu(), g.cpu(), G2.cpu(), g2.cpu()
    for p in range(nprob):
        assert torch.equal(G[p], Gref[p]), (p, _first_diff(G[p], Gref[p]))
        assert torch.equal(g[p], gref[p]), (p, _first_diff(g[p], gref[p]))
    assert torch.equal(G, G.transpose(1, 2))
    assert torch.equal(G, G2) and torch.equal(g, g2)


def _first_diff(a, b):
    bad = torch.nonzero(~(a == b))
    return "%d entries differ, first at %s: %r against %r" % (len(bad), bad[0].tolist(), float(a[tuple(bad[0])]),
                                                             float(b[tuple(bad[0])]))


# ---------------------------------------------------------------- 1. exact-integer parity

@pytest.mark.parametrize("case", GC.GRID_CASES, ids=_id)
def test_exact_integer_parity(ds, case):
    """Zero tolerance: G and g equal the host's product on integer data, are symmetric to the bit and repeat."""
    form, n, m = case
    _run_exact(ds, form, n, m)


@pytest.mark.parametrize("case", GC.THIN_CASES, ids=_id)
def test_exact_integer_parity_long_thin(ds, case):
    """32 splits with one row in the last (the reduce's 8-at-a-time loop alone) and 10 splits (its remainder loop)."""
    form, n, m = case
    assert GC.nsplit_of(m) == {31745: 32, 9217: 10}[m]
    _run_exact(ds, form, n, m)


@pytest.mark.parametrize("nprob", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("form,n", [("block", 65), ("tri8", 113), ("tri16", 241), ("512", 385)])
def test_exact_integer_parity_batch(ds, form, n, nprob):
    """Two splits a problem: 2, 6, 8, 10, 18 work items -- a full group of eight of the XCD mapping, one short by two,
    one over by two (masked tail items); every problem has its own data and every one is exact."""
    _run_exact(ds, form, n, 1025, nprob=nprob, seed=100 + nprob)


# ---------------------------------------------------------------- 2. componentwise rounding bound

BOUND_SHAPES = [(33, 17), (1024, 113), (2049, 127), (1024, 241), (2049, 256), (17, 385), (2049, 512), (2049, 513)]


@pytest.mark.parametrize("m,n", BOUND_SHAPES)
def test_componentwise_bound(ds, m, n):
    """Real-valued J whose columns span 10^-6 .. 10^6: every entry of G within (m + nsplit + 2) 2^-53 of |J|^T |J|, every
    entry of g of |J|^T |f| -- an entry of two small columns is held relative to ITS size, not to the largest."""
    J, f = GC.real_data(1, m, n, 11 + n)
    G, g = ds.gram(J.cuda(), f.cuda())
    GC.assert_bound(G, g, J, f, GC.route(full=True))
    if m <= 64:                                   # the sampled exact route is run wherever it is cheap, whatever the platform
        GC.assert_bound(G, g, J, f, "exact")


# ---------------------------------------------------------------- 3. structure

@pytest.mark.parametrize("form,n,m", FORM_SHAPES)
def test_batch_invariance(ds, form, n, m):
    """A problem's bits depend on its shape only: problem p of a batch of five equals the same J run alone."""
    _assert_plan(form, m, n)
    J, f = GC.real_data(5, m, n, 21 + n)
    Jd, fd = J.cuda(), f.cuda()
    G, g = ds.gram(Jd, fd)
    for p in range(5):
        G1, g1 = ds.gram(Jd[p:p + 1].contiguous(), fd[p:p + 1].contiguous())
        assert torch.equal(G1[0], G[p]) and torch.equal(g1[0], g[p]), p


@pytest.mark.parametrize("form,n,m", FORM_SHAPES)
def test_nan_problem_stays_in_its_problem(ds, form, n, m):
    """Problem 1 of three is all NaN: problems 0 and 2 are exact, problem 1 is NaN throughout."""
    _assert_plan(form, m, n)
    J, f = GC.int_data(3, m, n, 31 + n)
    J[1], f[1] = float("nan"), float("nan")
    Gref, gref = GC.cpu_product(J, f)
    G, g = (t.cpu() for t in ds.gram(J.cuda(), f.cuda()))
    for p in (0, 2):
        assert torch.equal(G[p], Gref[p]) and torch.equal(g[p], gref[p]), p
    assert bool(torch.isnan(G[1]).all()) and bool(torch.isnan(g[1]).all())


@pytest.mark.parametrize("form,n,m", FORM_SHAPES)
def test_nan_column_stays_in_its_row_and_column(ds, form, n, m):
    """NaN in one column c of J, c in the last partial tile (next to the zero padding): only row c and column c of G
    and g[c] are NaN -- the host product's pattern -- and every other entry is exact."""
    _assert_plan(form, m, n)
    c = (n // 16) * 16 + 1
    assert n % 16 and c < n - 1
    J, f = GC.int_data(1, m, n, 41 + n)
    J[0, c, :] = float("nan")
    Gref, gref = GC.cpu_product(J, f)
    want = torch.zeros((n, n), dtype=torch.bool)
    want[c, :] = True
    want[:, c] = True
    assert torch.equal(torch.isnan(Gref[0]), want) and torch.isnan(gref[0]).nonzero().flatten().tolist() == [c]
    G, g = (t.cpu() for t in ds.gram(J.cuda(), f.cuda()))
    assert torch.equal(torch.isnan(G[0]), want) and torch.equal(torch.isnan(g[0]), torch.isnan(gref[0]))
    assert torch.equal(G[0][~want], Gref[0][~want])
    keep = ~torch.isnan(gref[0])
    assert torch.equal(g[0][keep], gref[0][keep])


@pytest.mark.parametrize("form,n,m", FORM_SHAPES)
def test_no_stray_writes_and_null_f(ds, form, n, m):
    """nlh_gram with G and g carved out of larger sentinel-filled buffers: the margins (more than n n doubles on either
    side) are untouched; with f = NULL, G is the same and no entry of the g buffer is written."""
    _assert_plan(form, m, n)
    nprob, pad = 2, n * n + 64
    J, f = GC.int_data(nprob, m, n, 51 + n)
    Gref, gref = GC.cpu_product(J, f)
    Jd, fd = J.cuda(), f.cuda()

    def call(with_f):
        Gbuf = torch.full((2 * pad + nprob * n * n,), SENTINEL, dtype=torch.float64, device="cuda")
        gbuf = torch.full((2 * pad + nprob * n,), SENTINEL, dtype=torch.float64, device="cuda")
        _poison(ds, nprob, m, n)
        ds.h.check(ds.lib.nlh_gram(ds.h.ptr, nprob, m, n, Jd.data_ptr(), fd.data_ptr() if with_f else None,
                                   Gbuf[pad:].data_ptr(), gbuf[pad:].data_ptr()), "nlh_gram")
        torch.cuda.synchronize()
        return Gbuf.cpu(), gbuf.cpu()

    for with_f in (True, False):
        Gbuf, gbuf = call(with_f)
        assert bool((Gbuf[:pad] == SENTINEL).all()) and bool((Gbuf[pad + nprob * n * n:] == SENTINEL).all())
        assert torch.equal(Gbuf[pad:pad + nprob * n * n].view(nprob, n, n), Gref)
        if with_f:
            assert bool((gbuf[:pad] == SENTINEL).all()) and bool((gbuf[pad + nprob * n:] == SENTINEL).all())
            assert torch.equal(gbuf[pad:pad + nprob * n].view(nprob, n), gref)
        else:
            assert bool((gbuf == SENTINEL).all())


# ---------------------------------------------------------------- 4. the forms against each other

@pytest.mark.parametrize("m", [5, 1024, 1025, 2049])
@pytest.mark.parametrize("n", [97, 113, 128, 225, 241, 256])
def test_tri_same_bits_as_block_kernel(ds, m, n):
    """The header's "bitwise the same G and g as k_gram_mfma" for k_gram_tri<8> / <16>, the direct path (m <= 1024: G
    mirrored in the kernel, no reduce) against block kernel + reduce included."""
    J, f = GC.real_data(2, m, n, 61 + n)
    Jd, fd = J.cuda(), f.cuda()
    with GC.env(NLH_GRAM_TRI="0"):
        _assert_plan("block", m, n)
        _poison(ds, 2, m, n)
        G0, g0 = ds.gram(Jd, fd)
        torch.cuda.synchronize()
    with GC.env(NLH_GRAM_TRI=None):
        _assert_plan("tri8" if n <= 128 else "tri16", m, n)
        _poison(ds, 2, m, n)
        G1, g1 = ds.gram(Jd, fd)
        torch.cuda.synchronize()
    assert torch.equal(G0, G1) and torch.equal(g0, g1)


@pytest.mark.parametrize("m", [1, 17, 33, 1025])
@pytest.mark.parametrize("n", [257, 383, 384, 385, 512])
def test_512_same_bits_as_block_kernel_at_the_edges(ds, m, n):
    """k_gram_512 against k_gram_mfma where its units change shape: unit 3 absent (n <= 384), one column wide (385),
    one to three 16-row tiles.  G to the bit; g to rounding, not to the bit (sixteen partial sums per column and split
    against four): the two differ by no more than the componentwise bound either must meet."""
    J, f = GC.real_data(2, m, n, 71 + n)
    Jd, fd = J.cuda(), f.cuda()
    with GC.env(NLH_GRAM512="0"):
        _assert_plan("block", m, n)
        _poison(ds, 2, m, n)
        G0, g0 = ds.gram(Jd, fd)
        torch.cuda.synchronize()
    with GC.env(NLH_GRAM512=None):
        _assert_plan("512", m, n)
        _poison(ds, 2, m, n)
        G1, g1 = ds.gram(Jd, fd)
        torch.cuda.synchronize()
    assert torch.equal(G0, G1)
    for p in range(2):
        diff = (g0[p] - g1[p]).abs().cpu().numpy()
        assert (diff <= (m + GC.nsplit_of(m) + 2) * GC.U * GC.abs_jtf(J[p], f[p])).all(), p
    GC.assert_bound(G1, g1, J, f, GC.route(full=False))
    GC.assert_bound(G0, g0, J, f, GC.route(full=False))
