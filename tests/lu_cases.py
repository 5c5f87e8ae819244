"""What the LU tests (tests/test_gpu_lu_edges.py, tests/test_lu_cases_cpu.py) share: seeded matrices that steer the
pivot search and the interchanges, right-hand sides and packed factors that steer the solve's exact-zero skips, a host
restatement of the launch plan of lu_blocked, a numpy restatement of the two substitution sweeps, and the backward
identity in numpy.longdouble.

Layout as everywhere: a problem is column-major on the device, A[p, c, r] = a(r, c).  The matrix kinds below return plain
row-major numpy arrays, a[r, c] = a(r, c) (`dev_layout` converts); packed factors are built directly in
the device layout, M[c, r] = lu(r, c), which is also what the oracle reads as a column-major n-by-n array.

The backward identity.  Higham (Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 9.3): the factors of
Gaussian elimination computed in any order of Doolittle's sums satisfy |L U - P A| <= gamma_n |L| |U| entry by entry,
gamma_n = n u / (1 - n u), u = 2^-53.  The proof writes every entry as y = (c - sum_{k<m} a_k b_k) / b_m with m <= n and
counts one rounding per product, per subtraction and for the division; a fused multiply-add has fewer roundings than the
pair it replaces, so the bound also holds for the contracted kernels.  Here the multiplier is not a quotient: it is
a * fl(1 / pivot), two roundings where the theorem has one -- one more unit, n + 1.  The longdouble product that stands for
the exact L U is itself off by at most n 2^-64 |L| |U| = (n / 2048) u |L| |U|, at most one unit for n <= 2048: n + 2.  What
is left -- the 1 / (1 - n u) of gamma, the float64 evaluation of the scale |L| |U| (n u relative), the rounding of the
longdouble difference -- is below 1e-9 units at these sizes; the bound n + 3 leaves it a whole unit."""
import collections
import ctypes as C
import functools

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the backward identity needs an extended-precision long double"
U = 2.0 ** -53
LU_NB = 32                              # panel width of the global-memory panel (k_lu_panel)
LU_PNB = 16                             # panel width of the LDS panel (k_lu_panel_lds)
LU_PROWS = 1024                         # most rows of an LDS or a register panel
LUS_W = 16                              # column block of k_lu_solve
NOISE = 1e-3


def backward_bound(n):
    """The bound of the backward identity in units of 2^-53 |L| |U| (module docstring)."""
    return n + 3


# ---- matrix kinds: kind(n, seed) -> a[r, c] --------------------------------------------------------------------------------
def _rng(tag, n, seed):
    return np.random.default_rng([20250917, tag, n, seed])


def normal(n, seed):
    return _rng(1, n, seed).standard_normal((n, n))


def scaled_rows(n, seed):
    """Rows scaled over sixteen decades: the pivot search compares entries of very different exponents."""
    rng = _rng(2, n, seed)
    return rng.standard_normal((n, n)) * 10.0 ** rng.uniform(-8.0, 8.0, (n, 1))


def dominant(n, seed):
    """normal + 2 n I: diagonally dominant by columns, and so is every Schur complement -- no interchange, ipvt[j] == j."""
    return _rng(3, n, seed).standard_normal((n, n)) + 2.0 * n * np.eye(n)


def shift(n, seed):
    """a(i, j) = 1 where i == (j + 1) mod n, plus noise: ipvt[j] == j + 1 for j < n - 1.  The row that starts at position 0
    is displaced at every step: inside a register panel a chain of nb position swaps that ends in ONE move entry."""
    a = NOISE * _rng(4, n, seed).standard_normal((n, n))
    j = np.arange(n)
    a[(j + 1) % n, j] += 1.0
    return a


def reverse(n, seed):
    """a(i, j) = 1 where i == n - 1 - j, plus noise: ipvt[j] == n - 1 - j for j < n // 2 -- every step of the early panels
    sends a row below the block row (a move list with exactly nb entries)."""
    a = NOISE * _rng(5, n, seed).standard_normal((n, n))
    j = np.arange(n)
    a[n - 1 - j, j] += 1.0
    return a


def block_perm(n, seed):
    """A random permutation inside every aligned 16-row block, plus noise: every pivot stays inside its block (hence inside
    the block row of any panel: an EMPTY move list), yet ipvt[j] != j for most j."""
    rng = _rng(6, n, seed)
    a = NOISE * rng.standard_normal((n, n))
    for b0 in range(0, n, 16):
        w = min(16, n - b0)
        a[b0 + rng.permutation(w), b0 + np.arange(w)] += 1.0
    return a


def ties(n, seed):
    """Integers in [-3, 3]: whole keys tie in every pivot search, the first maximum wins."""
    return _rng(7, n, seed).integers(-3, 4, size=(n, n)).astype(np.float64)


LOW_WORD_KMAX = 2 ** 20


def low_word(n, seed):
    """Entries s (1 + k 2^-52), k integer in [0, 2^20), s a random sign: every |a| has the high word 0x3ff00000, so the low
    word decides and, among equal keys, the position.  In column 0 the largest k stands twice, first with a minus sign and
    then with a plus sign (`low_word_tie_rows`): a whole-key tie between -x and +x that the smaller position wins."""
    rng = _rng(8, n, seed)
    k = rng.integers(0, LOW_WORD_KMAX - 1, size=(n, n))          # (the planted maximum below stays strictly the largest)
    s = rng.choice([-1.0, 1.0], size=(n, n))
    if n >= 3:
        i1, i2 = low_word_tie_rows(n, seed)
        k[i1, 0] = k[i2, 0] = LOW_WORD_KMAX - 1
        s[i1, 0], s[i2, 0] = -1.0, 1.0
    return s * (1.0 + k * 2.0 ** -52)


def low_word_tie_rows(n, seed):
    """The two rows (i1 < i2) of low_word's column 0 that hold the largest key."""
    i1, i2 = sorted(_rng(9, n, seed).choice(np.arange(1, n), size=2, replace=False))
    return int(i1), int(i2)


def two_zero_cols(n, seed):
    """Columns 5 and n - 3 exactly zero: two zero pivots, in different panels for n >= 41; info must stay 6."""
    a = normal(n, seed).copy()
    a[:, 5] = 0.0
    a[:, n - 3] = 0.0
    return a


def neg_zero_col(n, seed):
    a = normal(n, seed).copy()
    a[:, n // 2] = -0.0
    return a


def nan_scattered(n, seed):
    a = normal(n, seed).copy()
    a[_rng(10, n, seed).random((n, n)) < 0.002] = np.nan
    return a


def denormal_col(n, seed):
    """One column scaled by 2^-1060: a denormal pivot whose reciprocal overflows, in the oracle as on the device."""
    a = normal(n, seed).copy()
    a[:, n // 3] *= 2.0 ** -1060
    return a


KINDS = {f.__name__: f for f in (normal, scaled_rows, dominant, shift, reverse, block_perm, ties, low_word, two_zero_cols,
                                 neg_zero_col, nan_scattered, denormal_col)}


def matrix(kind, n, seed=0):
    return KINDS[kind](n, seed)


def dev_layout(a):
    """a[r, c] -> the device's problem storage A[c, r] (contiguous)."""
    return np.ascontiguousarray(a.T)


# ---- the factor cases of the device tests ------------------------------------------------------------------------------------
FACTOR_SIZES = (1, 63, 64, 65, 95, 96, 127, 128, 129, 143, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1056, 1057)
ENGINEERED_SIZES = (129, 257, 513, 1025, 1057)
ENGINEERED_KINDS = ("shift", "reverse", "block_perm", "dominant", "low_word", "two_zero_cols")
SMALL_KINDS = ("neg_zero_col", "denormal_col", "scaled_rows")
KEY_SIZES = (143, 300, 1024)            # ties and scattered NaNs: a short last panel, a middle size, exactly 1024 rows


def factor_cases():
    """(n, kind) of the in-process factor test (the default panel mode)."""
    cases = [(n, "normal") for n in FACTOR_SIZES]
    cases += [(n, k) for n in ENGINEERED_SIZES for k in ENGINEERED_KINDS]
    cases += [(n, k) for n in (40, 300) for k in SMALL_KINDS]
    cases += [(n, k) for n in KEY_SIZES for k in ("ties", "nan_scattered")]
    cases += [(1024, "low_word")]           # four full waves of k_lu_panel_reg<4,16,256> (mode 2: eight of <2,16,512>) from column 0 on
    return cases


def child_factor_cases():
    """The same list for a child process that forces a panel mode: n >= 128 (below, the mode changes nothing), and above
    1024 -- where the oracle's O(n^3) loop takes a second a matrix -- only the kinds whose point is the first, global-memory
    panels or the pair of zero columns either side of the switch."""
    keep_big = {(1025, "shift"), (1025, "reverse"), (1025, "two_zero_cols"), (1057, "block_perm"), (1057, "two_zero_cols")}
    return [(n, k) for n, k in factor_cases() if n >= 128 and (n <= 1024 or k == "normal" or (n, k) in keep_big)]


# ---- the oracle on a case (shared by every test of a process) ----------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def oracle_factor(oracle, a):
    """nlo_lu_factor on a[r, c].  Returns (lu[r, c] Fortran-ordered, ipvt 0-based int32, info)."""
    n = a.shape[0]
    lu = np.array(a, dtype=np.float64, order="F")
    ipvt = np.zeros(n, dtype=np.int32)
    info = oracle.lib().nlo_lu_factor(n, _dp(lu), n, _ip(ipvt))
    return lu, ipvt, int(info)


def oracle_solve(oracle, M, ipvt, b):
    """nlo_lu_solve on a packed factor in the device layout M[c, r] (= column-major lu).  Returns x."""
    n = len(b)
    assert M.flags.c_contiguous and M.shape == (n, n)
    x = np.array(b, dtype=np.float64)
    oracle.lib().nlo_lu_solve(n, _dp(M), n, _ip(np.ascontiguousarray(ipvt, dtype=np.int32)), _dp(x))
    return x


@functools.lru_cache(maxsize=None)
def _reference(oracle, kind, n, seed):
    a = matrix(kind, n, seed)
    lu, ipvt, info = oracle_factor(oracle, a)
    b = rhs("dense", n, seed)
    with np.errstate(all="ignore"):
        x = oracle_solve(oracle, dev_layout(lu), ipvt, b)
    for arr in (a, lu, ipvt, b, x):
        arr.setflags(write=False)
    return a, lu, ipvt, info, b, x


def reference(oracle, kind, n, seed=0):
    """(a, lu, ipvt, info, b, x): the matrix, the oracle's factors of it, the dense right-hand side and the oracle's solution.
    Computed once per process and read-only."""
    return _reference(oracle, kind, n, seed)


def same_bits(got, want):
    """Bit for bit, so -0.0 is not 0.0.  A NaN must face a NaN: its sign and payload are not compared (the host and the
    device choose them differently); every other entry is compared on its bit pattern."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.int64)[~gn], want.view(np.int64)[~wn]))


def device_factor_mismatches(ds, oracle, n, kind, seed=0):
    """lu_factor and a dense solve of one case on the device against the oracle: the list of what differs, out of "info",
    "ipvt", "factors" and "solution" (empty: bit-identical).  With scattered NaNs the solution is not compared: the oracle's
    ordered skips meet NaN right-hand-side entries, whose comparisons the two sides need not order alike."""
    import torch
    a, lu, ipvt, info, b, x = reference(oracle, kind, n, seed)
    Ad = torch.tensor(dev_layout(a), device=ds.device).unsqueeze(0)
    bd = torch.tensor(b, device=ds.device).unsqueeze(0)
    ipd, infod = ds.lu_factor(Ad)
    ds.lu_solve(Ad, ipd, bd)
    torch.cuda.synchronize()
    bad = []
    if int(infod[0]) != info:
        bad.append(f"info {int(infod[0])} != {info}")
    if not np.array_equal(ipd[0].cpu().numpy(), ipvt):
        bad.append("ipvt")
    if not same_bits(Ad[0].cpu().numpy().T, lu):
        bad.append("factors")
    if kind != "nan_scattered" and not same_bits(bd[0].cpu().numpy(), x):
        bad.append("solution")
    return bad


BATCH_KINDS = ("normal", "ties", "two_zero_cols", "nan_scattered", "dominant")
BATCH_SIZES = (200, 520)


def device_batch_mismatches(ds, oracle, n, kinds=BATCH_KINDS):
    """One lu_factor launch on a batch with one problem of each kind: the list of (kind, what) that differ from the oracle,
    `what` out of "info", "ipvt" and "factors" (a panel writes info only where it is still zero, problem by problem)."""
    import torch
    refs = [reference(oracle, k, n) for k in kinds]
    Ad = torch.tensor(np.stack([dev_layout(r[0]) for r in refs]), device=ds.device)
    ipd, infod = ds.lu_factor(Ad)
    torch.cuda.synchronize()
    bad = []
    for p, (k, r) in enumerate(zip(kinds, refs)):
        if int(infod[p]) != r[3]:
            bad.append((k, f"info {int(infod[p])} != {r[3]}"))
        if not np.array_equal(ipd[p].cpu().numpy(), r[2]):
            bad.append((k, "ipvt"))
        if not same_bits(Ad[p].cpu().numpy().T, r[1]):
            bad.append((k, "factors"))
    return bad


# ---- right-hand sides and packed factors for the solve -------------------------------------------------------------------------
def rhs_kinds(n):
    """The names `rhs` takes at size n (a unit vector only where its index exists, each index once)."""
    return ["dense", "zeros"] + [f"e{k}" for k in sorted({0, 15, 16, n - 1}) if k < n] + ["neg_zero", "ints"]


def rhs(kind, n, seed=0):
    rng = _rng(11, n, seed)
    if kind == "dense":
        return rng.standard_normal(n)
    if kind == "zeros":
        return np.zeros(n)
    if kind[0] == "e" and kind[1:].isdigit():
        b = np.zeros(n)
        b[int(kind[1:])] = 1.0
        return b
    if kind == "neg_zero":                      # -0.0 but for n // 8 entries (n < 8: the all -0.0 vector): the leading run of
        b = np.full(n, -0.0)                    # P b is skipped only if -0.0 counts as zero, and x keeps its sign there
        at = rng.choice(n, size=n // 8, replace=False)
        b[at] = rng.standard_normal(n // 8)
        return b
    if kind == "ints":                          # with the factors of `ties` and with `int_lu`: exact cancellation to zero mid-sweep
        return rng.integers(-3, 4, size=n).astype(np.float64)
    raise KeyError(kind)


def packed_lu(n, seed=0):
    """A packed LU built directly (no factorisation, O(n^2) on both sides): unit-lower L and upper U with off-diagonal entries
    of size 1/n, a diagonal in [1, 2), random valid pivots (0-based, j <= ipvt[j] < n).  Returns (M[c, r], ipvt int32)."""
    rng = _rng(12, n, seed)
    M = rng.random((n, n))
    M -= 0.5
    M *= 2.0 / n
    M.flat[::n + 1] = 1.0 + rng.random(n)
    ipvt = (np.arange(n) + np.floor(rng.random(n) * (n - np.arange(n)))).astype(np.int32)
    return M, ipvt


def int_lu(n, seed=0):
    """A packed LU of small integers built directly: a diagonal of +-1, entries in {-1, 0, 1} on the first sub- and
    superdiagonal and, one in four, at distances 16 and 17 (across the column block of k_lu_solve), zeros elsewhere.  With
    an integer right-hand side both sweeps stay in small integers, so entries cancel to EXACT zeros in mid-sweep, dozens of
    times at n = 1041, forward and backward.  Returns (M[c, r], ipvt int32)."""
    rng = _rng(13, n, seed)
    M = np.zeros((n, n))
    i = np.arange(n)
    M[i, i] = rng.choice([-1.0, 1.0], size=n)
    for d, pr in ((1, 1.0), (16, 0.25), (17, 0.25)):
        if n > d:
            k = n - d
            M[i[:k], i[:k] + d] = rng.integers(-1, 2, size=k) * (rng.random(k) < pr)       # l(i + d, i)
            M[i[:k] + d, i[:k]] = rng.integers(-1, 2, size=k) * (rng.random(k) < pr)       # u(i, i + d)
    ipvt = (np.arange(n) + np.floor(rng.random(n) * (n - np.arange(n)))).astype(np.int32)
    return M, ipvt


def ties_lu(oracle, n, seed=0):
    """The oracle's packed factors of `ties` in the device layout: (M[c, r], ipvt, info)."""
    _, lu, ipvt, info, _, _ = reference(oracle, "ties", n, seed)
    return dev_layout(lu), ipvt, info


def apply_pivots(ipvt, b):
    """P b: the interchanges in order."""
    x = np.array(b, dtype=np.float64)
    for j in range(len(x)):
        p = int(ipvt[j])
        if p != j:
            x[j], x[p] = x[p], x[j]
    return x


def solve_sweeps(M, ipvt, b):
    """nlo_lu_solve restated in numpy on M[c, r]: the interchanges, L y = P b and U x = y, a step skipped where b(j) is
    exactly zero, separate multiply and subtract.  Returns (x, forward steps skipped, back steps skipped)."""
    n = len(b)
    x = apply_pivots(ipvt, b)
    fskip, bskip = [], []
    with np.errstate(all="ignore"):
        for j in range(n):
            if x[j] != 0.0:
                x[j + 1:] = x[j + 1:] - x[j] * M[j, j + 1:]
            else:
                fskip.append(j)
        for j in range(n - 1, -1, -1):
            if x[j] != 0.0:
                x[j] = x[j] / M[j, j]
                x[:j] = x[:j] - x[j] * M[j, :j]
            else:
                bskip.append(j)
    return x, fskip, bskip


def poison(M, ipvt, b):
    """A copy of the packed factor M[c, r] with NaN in everything the sequential loops never read for this b: the strictly
    lower entries of every L column whose forward step is skipped, and the whole U column, diagonal included, of every
    column whose back step is skipped.  The correct answer is the unpoisoned one, bit for bit; a skip that is not honoured
    turns it NaN."""
    _, fskip, bskip = solve_sweeps(M, ipvt, b)
    P = M.copy()
    for j in fskip:
        P[j, j + 1:] = np.nan
    for j in bskip:
        P[j, :j + 1] = np.nan
    return P


# ---- the launch plan of lu_blocked, restated -----------------------------------------------------------------------------------
Panel = collections.namedtuple("Panel", "jb nb form threads trsm gemm")


def lu_panel_reg_width(rows):
    if rows <= 0 or rows > 1024:
        return 0
    return min(32 if rows <= 512 else 16, rows)


def _round64(x):
    return (x + 63) & ~63


def panel_plan(n, mode=1):
    """The kernels launch_lu_factor launches for an n-by-n problem under NLH_LU_PANEL = mode, panel by panel:
    Panel(jb, nb, form, threads, trsm, gemm) with `form` the panel kernel (template arguments included), `trsm` the kernel
    that applies the panel's interchanges and solves the block row, `gemm` whether a trailing update follows.  n < 128: the
    one unblocked kernel."""
    if n < 128:
        return [Panel(0, n, "k_lu_factor", 1024 if n >= 96 else 256, None, False)]
    plan, jb = [], 0
    while jb < n:
        rows = n - jb
        if mode >= 1 and rows <= 1024:
            if rows <= 256:
                rpt, pw, tmax = 1, 32, 256
            elif rows <= 512:
                rpt, pw, tmax = 2, 32, 256
            elif mode >= 2:
                rpt, pw, tmax = 2, 16, 512
            else:
                rpt, pw, tmax = 4, 16, 256
            nb = min(pw, rows)
            assert nb == lu_panel_reg_width(rows)
            threads = max(64, _round64((rows + rpt - 1) // rpt))
            assert threads <= tmax
            form, trsm = f"k_lu_panel_reg<{rpt},{pw},{tmax}>", f"k_lu_move_trsm<{16 if nb <= 16 else 32}>"
        else:
            lds = mode == 0 and rows <= LU_PROWS
            nb = min(LU_PNB if lds else LU_NB, rows)
            threads = min(1024, _round64(rows)) if lds else 1024
            form, trsm = ("k_lu_panel_lds" if lds else "k_lu_panel"), "k_lu_swap_trsm"
        plan.append(Panel(jb, nb, form, threads, trsm, n - jb - nb > 0))
        jb += nb
    return plan


def kernels_of(n, mode=1):
    """The set of kernel instances `panel_plan` launches (the trailing update as "k_lu_gemm")."""
    s = set()
    for p in panel_plan(n, mode):
        s.add(p.form)
        if p.trsm:
            s.add(p.trsm)
        if p.gemm:
            s.add("k_lu_gemm")
    return s


def move_list_counts(ipvt, plan):
    """For every register panel of `plan`, the number of rows the interchanges ipvt[jb .. jb + nb) leave BELOW the panel's
    block row at another place than they started: the count k_lu_panel_reg writes at mv[32].  Returns {jb: count}."""
    n = len(ipvt)
    out = {}
    for p in plan:
        if not p.form.startswith("k_lu_panel_reg"):
            continue
        at = np.arange(n - p.jb)                      # at[i]: the starting place of the row now at panel position i
        for c in range(p.nb):
            q = int(ipvt[p.jb + c]) - p.jb
            at[c], at[q] = at[q], at[c]
        out[p.jb] = int(np.count_nonzero(at[p.nb:] != np.arange(p.nb, n - p.jb)))
    return out


# ---- the backward identity -----------------------------------------------------------------------------------------------------
def _lu_product(L, Um, B=128):
    """L Um for a lower-triangular L and an upper-triangular Um in their precision, touching only the blocks that are not
    zero by structure (a third of the full product's work)."""
    n = L.shape[0]
    out = np.zeros((n, n), dtype=L.dtype)
    for i0 in range(0, n, B):
        i1 = min(n, i0 + B)
        for j0 in range(0, n, B):
            j1 = min(n, j0 + B)
            k1 = min(i1, j1)
            out[i0:i1, j0:j1] = L[i0:i1, :k1] @ Um[:k1, j0:j1]
    return out


def permuted(a, ipvt):
    """P a: the interchanges ipvt applied to the rows of a[r, c] in order."""
    pa = np.array(a)
    for j, p in enumerate(ipvt):
        if p != j:
            pa[[j, p], :] = pa[[p, j], :]
    return pa


def backward_ratio(a, lu, ipvt):
    """max |P a - L U| / (2^-53 |L| |U|) entry by entry, a[r, c] the matrix, lu[r, c] its packed factors; the product in
    longdouble.  An entry whose scale is zero must be exact; a NaN anywhere gives inf."""
    n = a.shape[0]
    L = np.tril(lu, -1) + np.eye(n)
    Um = np.triu(lu)
    diff = np.abs(_lu_product(L.astype(LD), Um.astype(LD)) - permuted(a, ipvt).astype(LD))
    scale = _lu_product(np.abs(L), np.abs(Um)).astype(LD)        # the scale: float64 is ample
    if not (np.isfinite(diff).all() and np.isfinite(scale).all()):
        return np.inf
    zero = scale == 0
    if np.any(diff[zero] != 0):
        return np.inf
    return float(np.max(np.where(zero, LD(0), diff / np.where(zero, LD(1), scale)))) / U


# ---- a float64 model of the blocked factorisation, with the faults backward_ratio is for ---------------------------------------
def blocked_lu_model(a, nb=32, fault=None):
    """Right-looking blocked LU with partial pivoting in float64 (panels of nb columns, interchanges outside the panel
    deferred to the end of the panel, trailing update in 64 x 64 tiles).  fault = ("tile", step, tr, tc): that panel leaves
    trailing tile (tr, tc) un-updated; fault = ("swap", j): the interchange of step j is not applied outside the panel.
    Returns (lu[r, c], ipvt)."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    ipvt = np.zeros(n, dtype=np.int32)
    for step, jb in enumerate(range(0, n, nb)):
        t0 = min(n, jb + nb)
        for j in range(jb, t0):
            p = j + int(np.argmax(np.abs(a[j:, j])))
            ipvt[j] = p
            if p != j:
                a[[j, p], jb:t0] = a[[p, j], jb:t0]
            a[j + 1:, j] = a[j + 1:, j] * (1.0 / a[j, j])
            a[j + 1:, j + 1:t0] -= np.outer(a[j + 1:, j], a[j, j + 1:t0])
        for j in range(jb, t0):
            p = ipvt[j]
            if p != j and fault != ("swap", j):
                a[[j, p], :jb] = a[[p, j], :jb]
                a[[j, p], t0:] = a[[p, j], t0:]
        for j in range(jb, t0):                        # the block row: unit lower triangular solve, j ascending
            a[j + 1:t0, t0:] -= np.outer(a[j + 1:t0, j], a[j, t0:])
        for tr in range((n - t0 + 63) // 64):
            for tc in range((n - t0 + 63) // 64):
                if fault == ("tile", step, tr, tc):
                    continue
                r = slice(t0 + 64 * tr, min(n, t0 + 64 * tr + 64))
                c = slice(t0 + 64 * tc, min(n, t0 + 64 * tc + 64))
                a[r, c] -= a[r, jb:t0] @ a[jb:t0, c]
    return a, ipvt
