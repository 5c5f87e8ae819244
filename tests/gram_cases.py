"""What the Gram tests (tests/test_gpu_gram.py, and the two older Gram tests) share: the shape grid with the kernel form
every shape must take, exact-integer data, and the componentwise rounding bound with its two high-precision references.

Layout as everywhere: J [nprob, n, m] holds each problem column-major m-by-n (J[p, j, i] = J_p(i, j)), so
G[p] = J[p] @ J[p].T and g[p] = J[p] @ f[p]."""
import contextlib
import math
import os

import numpy as np
import torch

U = 2.0 ** -53                      # unit roundoff of float64


def nsplit_of(m):
    """K-splits of the Gram contraction: 1024 rows each (gram_splits in nlh_lm.hip), restated here on purpose."""
    return max(1, (m + 1023) // 1024)


# ---- section 1 of the grid: form -> (the n it must take, the m to run) ----
MS_SMALL = (1, 3, 4, 5, 31, 32, 33, 1024, 1025, 2049)
MS_TRI = (1, 5, 33, 1024, 1025, 2049)                    # 1024: one split, the direct path
MS_512 = (1, 15, 16, 17, 31, 32, 33, 48, 1025, 2049)     # <= 48 rows: one, two, three 16-row tiles
GRID = {
    "block": ((1, 15, 16, 17, 63, 64, 65, 96, 129, 224, 513), MS_SMALL),
    "tri8": ((97, 112, 113, 127, 128), MS_TRI),
    "tri16": ((225, 240, 241, 255, 256), MS_TRI),
    "512": ((257, 272, 383, 384, 385, 400, 511, 512), MS_512),
}
GRID_CASES = [(form, n, m) for form, (ns, ms) in GRID.items() for n in ns for m in ms]
# long and thin: 32 splits of which the last holds one row (the reduce's 8-at-a-time loop, no remainder); 10 splits
# (remainder 2)
THIN_CASES = [("block", 4, 31745), ("tri8", 100, 31745), ("block", 20, 9217)]


def expected_plan(form, m):
    ns = nsplit_of(m)
    return {"form": form, "nsplit": ns, "direct": form in ("tri8", "tri16") and ns == 1}


@contextlib.contextmanager
def env(**kv):
    """Set (value) or unset (None) environment variables for the block; the library reads them at each launch."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def int_data(nprob, m, n, seed):
    """Integers in [-2048, 2048] as float64 (CPU tensors).  Every product is an integer below 2^22 and every partial sum,
    in any order, an integer below 2^22 m: exactly representable while 2^22 m < 2^53, so a correct kernel and the CPU
    product agree to the bit whatever the order of their sums."""
    assert 2 ** 22 * m < 2 ** 53
    g = torch.Generator(device="cpu").manual_seed(seed)
    J = torch.randint(-2048, 2049, (nprob, n, m), generator=g).to(torch.float64)
    f = torch.randint(-2048, 2049, (nprob, m), generator=g).to(torch.float64)
    return J, f


def real_data(nprob, m, n, seed):
    """randn with the columns scaled by 10^(-6 .. 6) in shuffled order (entries of G span 24 decades), f = randn."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    J = torch.randn((nprob, n, m), dtype=torch.float64, generator=g)
    f = torch.randn((nprob, m), dtype=torch.float64, generator=g)
    scale = 10.0 ** torch.linspace(-6, 6, n, dtype=torch.float64)
    for p in range(nprob):
        J[p] *= scale[torch.randperm(n, generator=g)].unsqueeze(1)
    return J, f


def cpu_product(J, f):
    """G and g in float64 on the host (J, f CPU tensors)."""
    return torch.matmul(J, J.transpose(1, 2)), torch.matmul(J, f.unsqueeze(-1)).squeeze(-1)


# ---- the componentwise bound |G - Gref| <= (m + nsplit + 2) 2^-53 |J|^T |J| ----
# The a-priori bound of an inner product of length m summed in any order with fused or unfused multiply-adds
# (gamma_m ~ m u) plus one add per split in the reduce; the same for g with |J|^T |f|.  It is derived, not measured.

def longdouble_ok():
    return bool(np.finfo(np.longdouble).eps <= 2.0 ** -63)


def route(full=True):
    """The reference a test takes: numpy.longdouble where it has a 64-bit significand (every entry, or the sample for
    shapes where every entry would take seconds), the sampled exact route otherwise."""
    if longdouble_ok():
        return "longdouble" if full else "longdouble-sample"
    return "exact"


def sample_pairs(n, seed=20240):
    """The fixed sample of entries (row, column) of G: the whole diagonal, the first and last row and column, every entry
    whose row or column index is 0 or 15 modulo 16 with row - column in {0, 1, 15, 16}, and 2000 seeded random ones."""
    pairs = set()
    for i in range(n):
        pairs.update(((i, i), (0, i), (i, 0), (n - 1, i), (i, n - 1)))
    for r in range(n):
        for d in (0, 1, 15, 16):
            c = r - d
            if 0 <= c and (r % 16 in (0, 15) or c % 16 in (0, 15)):
                pairs.add((r, c))
    rng = np.random.RandomState(seed)
    pairs.update(zip(rng.randint(0, n, 2000).tolist(), rng.randint(0, n, 2000).tolist()))
    ij = np.array(sorted(pairs), dtype=np.int64)
    return ij[:, 0], ij[:, 1]


def _two_product(a, b):
    """Dekker: p + e = a b exactly (p = fl(a b)), by Veltkamp splitting; no fused multiply-add needed."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _exact_err_and_s(A, B, got):
    """Rows of A and B are the vector pairs, got[k] the computed inner product.  Returns |sum_i A[k,i] B[k,i] - got[k]|
    and sum_i |A[k,i] B[k,i]|, each the correctly rounded value of the exact quantity (error-free products, math.fsum)."""
    err, s = np.empty(len(got)), np.empty(len(got))
    for k0 in range(0, len(got), 256):
        p, e = _two_product(A[k0:k0 + 256], B[k0:k0 + 256])
        sp = np.where(p < 0, -e, e)
        p, e, ap, sp = p.tolist(), e.tolist(), np.abs(p).tolist(), sp.tolist()
        for k in range(len(p)):
            err[k0 + k] = abs(math.fsum(p[k] + e[k] + [-float(got[k0 + k])]))
            s[k0 + k] = math.fsum(ap[k] + sp[k])
    return err, s


def abs_jtf(J, f):
    """|J|^T |f| of one problem (J [n, m], f [m]) in the precision of route()."""
    J, f = np.abs(np.asarray(J, dtype=np.float64)), np.abs(np.asarray(f, dtype=np.float64))
    if longdouble_ok():
        return J.astype(np.longdouble) @ f.astype(np.longdouble)
    return _exact_err_and_s(J, np.broadcast_to(f, J.shape), np.zeros(len(J)))[1]


def bound_violations(G, g, J, f, nsplit, route):
    """One problem: G [n, n], g [n] as computed, J [n, m], f [m] (CPU tensors or arrays).  Returns the list of entries that
    miss the bound, worst first, as (what, row, column, error / bound).

    route "longdouble": every entry, reference and |J|^T |J| accumulated in numpy.longdouble (the caller has asserted
    longdouble_ok(): 64-bit significand, so the reference's own error is below 2^-11 of the bound).
    route "longdouble-sample": the same arithmetic on the sample of sample_pairs and all of g (large shapes).
    route "exact": that sample, error-free products summed by math.fsum (needs no extended type)."""
    G, g, J, f = (np.asarray(t, dtype=np.float64) for t in (G, g, J, f))
    n, m = J.shape
    fac = (m + nsplit + 2) * U
    if route == "longdouble":
        assert longdouble_ok()
        L, fl = J.astype(np.longdouble), f.astype(np.longdouble)
        La = np.abs(L)
        ii, jj = (a.ravel() for a in np.indices((n, n)))
        eG = np.abs(np.einsum("im,jm->ij", L, L) - G.astype(np.longdouble)).ravel()
        sG = np.einsum("im,jm->ij", La, La).ravel()
        eg = np.abs(L @ fl - g.astype(np.longdouble))
        sg = La @ np.abs(fl)
    elif route == "longdouble-sample":
        assert longdouble_ok()
        L, fl = J.astype(np.longdouble), f.astype(np.longdouble)
        ii, jj = sample_pairs(n)
        eG, sG = np.empty(len(ii), dtype=np.longdouble), np.empty(len(ii), dtype=np.longdouble)
        for k0 in range(0, len(ii), 512):
            P = L[ii[k0:k0 + 512]] * L[jj[k0:k0 + 512]]
            eG[k0:k0 + 512] = np.abs(P.sum(axis=1) - G[ii[k0:k0 + 512], jj[k0:k0 + 512]])
            sG[k0:k0 + 512] = np.abs(P).sum(axis=1)
        eg = np.abs(L @ fl - g.astype(np.longdouble))
        sg = np.abs(L) @ np.abs(fl)
    else:
        assert route == "exact"
        ii, jj = sample_pairs(n)
        eG, sG = _exact_err_and_s(J[ii], J[jj], G[ii, jj])
        eg, sg = _exact_err_and_s(J, np.broadcast_to(f, J.shape), g)
    bad = [("G", int(ii[k]), int(jj[k]), float(eG[k] / (fac * sG[k])) if sG[k] else math.inf)
           for k in np.nonzero(~(eG <= fac * sG))[0]]
    bad += [("g", int(k), -1, float(eg[k] / (fac * sg[k])) if sg[k] else math.inf) for k in np.nonzero(~(eg <= fac * sg))[0]]
    return sorted(bad, key=lambda b: -b[3])


def assert_bound(G, g, J, f, route):
    """Every problem of a batch (G, g from the device or the host; J, f CPU tensors) meets the componentwise bound."""
    nprob, n, m = J.shape
    G, g = G.cpu(), g.cpu()
    for p in range(nprob):
        bad = bound_violations(G[p], g[p], J[p], f[p], nsplit_of(m), route)
        assert not bad, f"problem {p} of {m} x {n}: {len(bad)} entries miss the bound; (what, row, col, error/bound): {bad[:5]}"
