"""The launch shape of the formula kernels (nlh_expr_plan / nonlin_amd.device.expr_plan: the function the launchers
themselves dispatch through, host code) over every depth, every n and every m up to 600, held to what include/nonlin_hip.h
and the launchers' comments say of it -- not to a copy of the code: the LDS a launch asks for and its cap, the chunk of
Jacobian columns as the most that fits half of the cap, the two overrides, the forms and the grid.  No GPU."""
import ctypes as C
import itertools

import pytest

from nonlin_amd import _lib
from nonlin_amd.device import expr_plan

LDS_MAX = 160 * 1024 - 2048                  # NLH_LDS_MAX (nlh_internal.h): what a workgroup may ask for
HALF = LDS_MAX // 2                          # two workgroups per compute unit
DEPTHS, NS = range(1, 17), range(1, 33)
MS = list(range(1, 601)) + [1023, 1024, 1025]
MS_ENV = [1, 2, 3, 5, 51, 64, 85, 86, 127, 128, 129, 200, 255, 256, 257, 512, 513, 1025]
NPOINTS = 7                                   # (a count no ppw of the sweep but 1 and 7 divides)
NL_INVALID_INPUT_ERROR = 201


class _Raw:
    """nlh_expr_plan with its outputs allocated once: the sweep makes 600,000 calls."""

    def __init__(self):
        self.fn = _lib.load().nlh_expr_plan
        self.i = [C.c_int32() for _ in range(4)]
        self.l = [C.c_int64() for _ in range(2)]
        f, p, b, c = (C.byref(v) for v in self.i)
        g, s = (C.byref(v) for v in self.l)
        self.out = (f, p, b, g, c, s)

    def __call__(self, depth, n, m, jac, npoints=NPOINTS):
        assert self.fn(depth, n, m, npoints, jac, *self.out) == 0, (depth, n, m, jac)
        return self.i[0].value, self.i[1].value, self.i[2].value, self.l[0].value, self.i[3].value, self.l[1].value


def _lds(ppw, n, depth, chunk):
    return 8 * (ppw * n + 256 * depth * (1 + chunk))


def _check(what, depth, n, m, jac, got, flat_want):
    """What holds of every plan, under any override.  Returns (chunk, lds_bytes)."""
    flat, ppw, nblk, grid, chunk, lds = got
    assert bool(flat) == flat_want, what
    if flat:
        assert ppw == 256 // m and nblk == 1 and grid == -(-NPOINTS // ppw), what
    else:
        assert ppw == 1 and nblk == -(-m // 256) and grid == NPOINTS * nblk, what
    assert lds == _lds(ppw, n, depth, chunk) and lds <= LDS_MAX, what
    if not jac:
        assert chunk == 0, what
    else:
        assert 1 <= chunk <= min(n, 8), what
        assert chunk == 1 or lds <= HALF, what                          # only one column per pass may exceed the half
    return chunk, lds


def test_every_depth_n_and_m(monkeypatch):
    monkeypatch.delenv("NLH_EXPR_FORM", raising=False)
    monkeypatch.delenv("NLH_EXPR_CHUNK", raising=False)
    plan = _Raw()
    top, at = 0, []
    for depth, n, m in itertools.product(DEPTHS, NS, MS):
        for jac in (0, 1):
            got = plan(depth, n, m, jac)
            what = (depth, n, m, jac, got)
            chunk, lds = _check(what, depth, n, m, jac, got, m <= 128)
            if jac and chunk < min(n, 8):                               # the chunk is the most: one more breaks the half
                assert _lds(got[1], n, depth, chunk + 1) > HALF, what
            if lds > top:
                top, at = lds, []
            if lds == top:
                at.append((depth, n, m, jac))
    assert top == 131072 and at == [(16, 32, 1, 1)]


def test_overrides(monkeypatch):
    monkeypatch.delenv("NLH_EXPR_FORM", raising=False)
    monkeypatch.delenv("NLH_EXPR_CHUNK", raising=False)
    plan = _Raw()
    cases = list(itertools.product(DEPTHS, NS, MS_ENV))
    default = {c: plan(*c, 1) for c in cases}
    for form in ("row", "flat"):
        monkeypatch.setenv("NLH_EXPR_FORM", form)
        for depth, n, m in cases:
            for jac in (0, 1):
                got = plan(depth, n, m, jac)
                what = (form, depth, n, m, jac, got)
                chunk, lds = _check(what, depth, n, m, jac, got, form == "flat" and m <= 256)   # flat falls back above 256
                if jac and chunk < min(n, 8):
                    assert _lds(got[1], n, depth, chunk + 1) > HALF, what
    monkeypatch.delenv("NLH_EXPR_FORM")
    for k in (1, 2, 3, 5, 9):
        monkeypatch.setenv("NLH_EXPR_CHUNK", str(k))
        for c in cases:
            got, base = plan(*c, 1), default[c]
            what = (k, c, got, base)
            _check(what, *c, 1, got, c[2] <= 128)
            assert got[4] == min(k, base[4]) and got[:4] == base[:4], what
            assert got == base or k < base[4], what                     # k >= the default changes nothing
            _check(what, *c, 0, plan(*c, 0), c[2] <= 128)               # (the residual kernel has no chunk to ask fewer of)


def test_spot_values(monkeypatch):
    """By hand from the rule: 1 + chunk stacks of 2,048 * depth bytes and x fit 80,896 bytes.  Row form, x = 8 n bytes."""
    monkeypatch.delenv("NLH_EXPR_FORM", raising=False)
    monkeypatch.delenv("NLH_EXPR_CHUNK", raising=False)
    chunk = lambda depth, n, m=200: expr_plan(depth, n, m)["chunk"]
    assert chunk(3, 32) == 8                                            # 9 x 6,144 + 256 = 55,552 (13 would fit: 8 at most)
    assert chunk(6, 32) == 5                                            # 6 x 12,288 + 256 = 73,984; 7 x: 86,272
    assert chunk(7, 32) == 4                                            # 5 x 14,336 + 256 = 71,936; 6 x: 86,272
    assert chunk(8, 32) == 3 and chunk(8, 3) == 3 and chunk(8, 2) == 2  # 4 x 16,384 + 256 = 65,792; 5 x: 82,176
    assert chunk(9, 32) == 3                                            # 4 x 18,432 + 256 = 73,984; 5 x: 92,416
    for depth in range(10, 14):                                         # 3 x 20,480 .. 3 x 26,624 + 256 = 80,128; 4 x 20,480: 82,176
        assert all(chunk(depth, n) == 2 for n in range(2, 33)) and chunk(depth, 1) == 1, depth
    for depth in (14, 15, 16):                                          # 3 x 28,672 = 86,016
        assert all(chunk(depth, n) == 1 for n in (1, 2, 32)), depth
    assert expr_plan(6, 32, 5) == {"flat": True, "ppw": 51, "nblk": 1, "grid": 1, "chunk": 4, "lds_bytes": 8 * 51 * 32 + 5 * 12288}
    assert expr_plan(6, 32, 1)["chunk"] == 1 and expr_plan(6, 32, 1)["lds_bytes"] == 65536 + 2 * 12288      # x alone: 65,536
    assert expr_plan(16, 32, 1, 300) == {"flat": True, "ppw": 256, "nblk": 1, "grid": 2, "chunk": 1, "lds_bytes": 131072}
    assert expr_plan(16, 32, 1, 300, jac=False) == {"flat": True, "ppw": 256, "nblk": 1, "grid": 2, "chunk": 0, "lds_bytes": 98304}
    assert expr_plan(4, 5, 513, 7) == {"flat": False, "ppw": 1, "nblk": 3, "grid": 21, "chunk": 5, "lds_bytes": 40 + 6 * 8192}
    assert expr_plan(4, 5, 85, 7)["ppw"] == 3 and expr_plan(4, 5, 85, 7)["grid"] == 3 and expr_plan(4, 5, 86, 7)["grid"] == 4
    assert expr_plan(4, 5, 64, 0)["grid"] == 0


def test_refusals():
    for args in ((0, 4, 8), (17, 4, 8), (4, 0, 8), (4, 33, 8), (4, 4, 0), (4, 4, 8, -1)):
        with pytest.raises(ValueError, match="nlh_expr_plan"):
            expr_plan(*args)
    with pytest.raises(ValueError):
        expr_plan(4, 4, 1 << 20, 1 << 30)                               # more workgroups than a grid holds
    fn = _lib.load().nlh_expr_plan
    i, l = [C.c_int32() for _ in range(4)], [C.c_int64() for _ in range(2)]
    out = [C.byref(i[0]), C.byref(i[1]), C.byref(i[2]), C.byref(l[0]), C.byref(i[3]), C.byref(l[1])]
    assert fn(4, 4, 8, 1, 1, *out) == 0
    for k in range(6):
        assert fn(4, 4, 8, 1, 1, *[None if j == k else o for j, o in enumerate(out)]) == NL_INVALID_INPUT_ERROR, k
