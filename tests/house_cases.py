"""What the Householder-step tests share (tests/test_gpu_house.py, tests/test_house_plan_cpu.py, the LAPACK-relative check
of tests/test_oracle.py and tests/golden/make_house_study.py): the shape grid with the kernel form every shape must take,
the data with its degenerate patterns, and the residuals of a factorisation.  numpy only -- no torch, no GPU.

Layout: the work arrays are ROW-major, A [nprob, rows, ncA] and E [nprob, rows, ncE]: A[p] and E[p] are the matrices.
nc = ncA + ncE is the total column count."""
import collections

import numpy as np

# ---- the dispatch rule of launch_house_steps (nlh_square.hip), restated here on purpose ----
FUSED_MAXROWS, DOT2_MAXROWS, LDS_ROWS = 4096, 8192, 18000
SKINNY_BELOW = 1536                 # nc * nprob below this: four columns a workgroup
TWO_TILES_UPTO = 256                # ceil(nc / 16) * nprob up to this: two product tiles
COLUMN_GROUP = {"fused4": 4, "fused16": 16, "dot2": 16, "dot_lds": 128, "dot_global": 128}


def expected_plan(nprob, rows, ncA, ncE):
    nc = ncA + ncE
    if rows <= FUSED_MAXROWS:
        if nc * nprob < SKINNY_BELOW:
            return {"form": "fused4", "tiles": 2}
        return {"form": "fused16", "tiles": 1 if -(-nc // 16) * nprob > TWO_TILES_UPTO else 2}
    if rows <= DOT2_MAXROWS:
        return {"form": "dot2", "tiles": 2}
    return {"form": "dot_lds" if rows <= LDS_ROWS else "dot_global", "tiles": 0}


# form and tiles: what the section of the grid the case stands in says it takes; pattern: see make_data
Case = collections.namedtuple("Case", "form tiles nprob rows ncA ncE pattern")


def case_id(c):
    return "%s-t%d-p%d-r%d-%dx%d-%s" % c


def _grid(form, tiles, nprobs, rowss, pairs, skip=()):
    return [Case(form, tiles, nprob, rows, ncA, ncE, "dense") for nprob in nprobs for rows in rowss for ncA, ncE in pairs
            if ncA <= rows and (rows, ncA, ncE) not in skip]


# fused<4>: 1024-row tiles, 16 x 256 prologue rows; the A/E boundary on a 4-column group edge ((4,4), (8,1)) and inside one,
# the last group partly empty ((1,1), (3,2), (9,4)); (5,0): no E at all
GRID_FUSED4 = _grid("fused4", 2, (3,), (2, 3, 17, 64, 65, 1024, 1025, 1026, 2049, 4095, 4096),
                    ((1, 1), (3, 2), (4, 4), (5, 7), (8, 1), (9, 4))) + _grid("fused4", 2, (3,), (17, 4096), ((5, 0),)) + \
    _grid("fused4", 2, (3,), (1,), ((1, 3), (1, 0)))           # one row: no step at all, nothing may change
# fused<16>, one product tile (ceil(64 / 16) * 65 = 260 workgroups): 256-row tiles
GRID_FUSED16_ONE = _grid("fused16", 1, (65,), (41, 256, 257, 258, 513), ((40, 24), (33, 31), (16, 48))) + \
    _grid("fused16", 1, (65,), (257,), ((64, 0),))                     # no E at all
# fused<16>, two product tiles: nc * nprob >= 1536 with at most 256 workgroups
GRID_FUSED16_TWO = (_grid("fused16", 2, (2,), (34, 256, 257, 513, 4096), ((33, 767),)) +
                    _grid("fused16", 2, (1,), (34, 256, 257, 513, 4096), ((20, 1516), (17, 1519))) +
                    _grid("fused16", 2, (1,), (257,), ((40, 1496),)) +
                    _grid("fused16", 2, (16,), (257,), ((96, 0),)))    # no E at all: 16 x 96 = 1536 columns, 96 workgroups
# dot2: 256-row tiles, 16-column groups
GRID_DOT2 = _grid("dot2", 2, (1, 3), (4097, 4098, 4352, 4353, 8191, 8192), ((5, 1), (16, 16), (17, 15), (33, 40))) + \
    _grid("dot2", 2, (3,), (4097,), ((20, 0),))
# dot<false> / dot<true>: 128 columns a workgroup ((20,108): exactly one; (20,109), (130,1), (64,70): two), 32-row load groups
_DOT_PAIRS = ((20, 107), (20, 108), (20, 109), (130, 1), (64, 70))
GRID_DOT_LDS = _grid("dot_lds", 0, (2,), (8193, 8225, 17999, 18000), _DOT_PAIRS) + _grid("dot_lds", 0, (2,), (8193,), ((20, 0),))
GRID_DOT_GLOBAL = _grid("dot_global", 0, (2,), (18001, 18033), _DOT_PAIRS) + \
    _grid("dot_global", 0, (1,), (70000,), _DOT_PAIRS, skip=((70000, 130, 1),)) + _grid("dot_global", 0, (2,), (18001,), ((20, 0),))
GRID_CASES = GRID_FUSED4 + GRID_FUSED16_ONE + GRID_FUSED16_TWO + GRID_DOT2 + GRID_DOT_LDS + GRID_DOT_GLOBAL

# ---- degenerate steps: every form at its smallest row count ----
# (form, tiles, nprob, rows, (ncA, ncE), (ncA, ncE) for the patterns that need steps beyond the column group)
DEGENERATE_SHAPES = (("fused4", 2, 3, 17, (9, 4), (9, 4)),
                     ("fused16", 1, 65, 41, (40, 24), (40, 24)),
                     ("fused16", 2, 2, 34, (33, 767), (33, 767)),
                     ("dot2", 2, 3, 4097, (33, 40), (33, 40)),
                     ("dot_lds", 0, 2, 8193, (20, 109), (130, 1)),
                     ("dot_global", 0, 2, 18001, (20, 109), (130, 1)))
# tri: H = I steps whose diagonal entry is not zero (the column is exactly zero BELOW its diagonal when its step comes);
# zero: the column is zero everywhere, its diagonal included; tiny: the column is of size 1e-170 everywhere, so that the
# squares below its diagonal underflow and sum to exactly zero although no entry is zero.  first / last: step 0 / the
# last step; pair: the two consecutive steps CG - 1 and CG, either side of a column-group edge; cg / cg1: step j with
# j - 1 = CG - 1 / CG (the workgroup that finishes column j - 1 is, for j = CG, not the one that owns column j).
PATTERNS_NARROW = ("tri-first", "tri-last", "zero-first", "zero-last", "tiny-first", "tiny-last", "allzero", "nan")
PATTERNS_WIDE = ("tri-pair", "tri-cg", "tri-cg1", "zero-pair", "zero-cg", "zero-cg1", "tiny-pair", "tiny-cg", "tiny-cg1")
DEGENERATE_CASES = [Case(form, tiles, nprob, rows, *(narrow if pat in PATTERNS_NARROW else wide), pat)
                    for form, tiles, nprob, rows, narrow, wide in DEGENERATE_SHAPES
                    for pat in PATTERNS_NARROW + PATTERNS_WIDE]


def pattern_steps(c):
    """The steps the pattern of case c makes H = I (in the problems that carry it)."""
    cg, last = COLUMN_GROUP[c.form], min(c.ncA, c.rows - 1) - 1
    kind = c.pattern.split("-")[-1]
    js = {"first": [0], "last": [last], "pair": [cg - 1, cg], "cg": [cg], "cg1": [cg + 1]}[kind]
    assert 0 <= min(js) and max(js) <= last, (c, js)
    return js


def make_data(c, seed=0):
    """A [nprob, rows, ncA], E [nprob, rows, ncE] of case c: standard normal, every problem its own.  A pattern other than
    "dense" is carried by the problems of even index only, so that a launch holds degenerate and ordinary problems side
    by side:

    tri-*   the steps js = pattern_steps(c) meet a column that is exactly zero below its diagonal: columns 0 .. js[0] are zero
            below row js[0] (so the reflectors before it are zero there and leave those zeros alone: 0 - 0 w = 0), every
            further column j of js below row j.  The other columns, and E, are dense.  (The reflectors BEFORE the first of
            these steps are therefore zero beyond row js[0]: at the long forms' row counts the pending update that is
            folded in around the identity step multiplies by zero in every row tile but the first, so these cases do not
            exercise that update across tiles -- the zero-* and tiny-* cases, whose reflectors are dense, do.)
    zero-*  the columns js are zero in every row -- and stay so under every reflector -- the rest is dense.
    tiny-*  the columns js are 1e-170 times a standard normal in every row -- and stay of that size under every reflector
            (w is of that size, v of size one) -- the rest is dense.  No entry is zero, but every square below the
            diagonal underflows to zero, so the steps js are skipped; what was below the diagonal must come back as
            exact zeros and the diagonal entry as it stood, in every form.
    allzero A = 0: every step is H = I and E comes back as it went in.
    nan     one NaN in a middle column and row of A."""
    rng = np.random.default_rng([seed, c.nprob, c.rows, c.ncA, c.ncE])
    A = rng.standard_normal((c.nprob, c.rows, c.ncA))
    E = rng.standard_normal((c.nprob, c.rows, c.ncE))
    if c.pattern == "dense":
        return A, E
    for p in range(0, c.nprob, 2):
        if c.pattern == "allzero":
            A[p] = 0.0
        elif c.pattern == "nan":
            A[p, c.rows // 2, c.ncA // 2] = np.nan
        elif c.pattern.startswith("zero-"):
            A[p][:, pattern_steps(c)] = 0.0
        elif c.pattern.startswith("tiny-"):
            A[p][:, pattern_steps(c)] *= 1e-170
        else:
            js = pattern_steps(c)
            A[p][js[0] + 1:, :js[0] + 1] = 0.0
            for j in js[1:]:
                A[p][j + 1:, j] = 0.0
    return A, E


# ---- residuals of a factorisation, for the LAPACK-relative check ----
STUDY_SHAPES = ((5, 3), (40, 40), (64, 17), (129, 40), (300, 40), (257, 33))


def study_matrix(m, n):
    return np.random.default_rng([2024, m, n]).standard_normal((m, n))


def residuals(a, q, r):
    """Column-wise residuals of a = q r (a m x n, q m x m, r m x n upper triangular): the largest over the columns of
    ||(a - q r)[:, k]|| / ||a[:, k]||, and the largest column norm of q^T q - I."""
    fac = np.linalg.norm(a - q @ r, axis=0) / np.linalg.norm(a, axis=0)
    orth = np.linalg.norm(q.T @ q - np.eye(q.shape[0]), axis=0)
    return float(fac.max()), float(orth.max())


def lapack_residuals(a):
    q, r = np.linalg.qr(a, mode="complete")
    return residuals(a, q, r)


def oracle_residuals(oracle, a):
    """The restatement on [a | I]: E = I comes back as Q^T."""
    r, qt = oracle.qr_factor_cols(a, np.eye(a.shape[0]))
    assert not np.tril(r, -1).any()
    return residuals(a, np.ascontiguousarray(qt.T), r)
