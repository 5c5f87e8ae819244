"""Loader and problem generator for the user-side fcn1var family of tests/device_1var/scalar_models.hip: a per-problem cubic
c0 + x (c1 + x (c2 + x c3)) and its derivative as device launchers (include/nonlin_hip.h: nlh_device_vecfcn /
nlh_device_jacfcn with n = m = 1), their host twins, and a counting wrapper that records the points it is handed.  Test /
bench infrastructure, not part of the product."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "device_1var", "libscalar_models.so")
dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)

_so = None


def lib():
    global _so
    if _so is None:
        if not os.path.exists(SO):
            subprocess.check_call(["make", "-C", os.path.dirname(SO), "-s"])
        try:
            import torch  # noqa: F401  (its HIP runtime first, as for libnonlin_hip.so)
        except ImportError:
            pass
        so = C.CDLL(SO)
        so.cubic_create.restype = C.c_void_p
        so.cubic_create.argtypes = [C.c_int32, dp]
        so.cubic_destroy.argtypes = [C.c_void_p]
        so.cubic_host_f.restype = C.c_double
        so.cubic_host_f.argtypes = [dp, C.c_double]
        so.cubic_host_df.restype = C.c_double
        so.cubic_host_df.argtypes = [dp, C.c_double]
        so.counting_create.restype = C.c_void_p
        so.counting_create.argtypes = [C.c_void_p]
        so.counting_destroy.argtypes = [C.c_void_p]
        so.counting_size.restype = C.c_int64
        so.counting_size.argtypes = [C.c_void_p]
        so.counting_calls.restype = C.c_int64
        so.counting_calls.argtypes = [C.c_void_p, C.c_int32]
        so.counting_get.argtypes = [C.c_void_p, dp, ip]
        so.counting_call_sizes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        _so = so
    return _so


def cubic_problems(nprob, seed=7):
    """nprob cubics and brackets [nprob, 2] in eight kinds by p % 8: one bracketed real root (0, 5: a wide bracket, 7:
    the limits reversed), a root exactly at an endpoint (1), an invalid bracket |x1 - x2| < eps (2), a flat triple root
    (3), no root in the bracket (4; every other one a line on a bracket of a few 1e-9, which newton bisects until its
    bisection exit), three real roots (6).  Returns c [nprob, 4], lim [nprob, 2]."""
    rng = np.random.default_rng(seed)
    c = np.zeros((nprob, 4))
    lim = np.zeros((nprob, 2))
    r = rng.uniform(-2.0, 2.0, nprob)
    a = rng.uniform(0.25, 2.0, nprob)
    u1 = rng.uniform(0.1, 3.0, nprob)
    u2 = rng.uniform(0.1, 3.0, nprob)
    v = rng.uniform(-1e-16, 1e-16, nprob)
    k = np.arange(nprob) % 8
    one = np.isin(k, (0, 5, 7))
    c[one] = np.stack([-r * a, a, -r, np.ones(nprob)], 1)[one]
    lim[one] = np.stack([r - u1, r + u2], 1)[one]
    m = k == 5
    lim[m] = np.stack([r - 40 * u1, r + 40 * u2], 1)[m]
    m = k == 7
    lim[m] = np.stack([r + u2, r - u1], 1)[m]
    m = k == 1
    c[m] = np.stack([np.zeros(nprob), a, -r, np.ones(nprob)], 1)[m]
    lim[m] = np.where((np.arange(nprob) % 16 == 1)[:, None], np.stack([np.zeros(nprob), u1], 1),
                      np.stack([-u2, np.zeros(nprob)], 1))[m]
    m = k == 2
    c[m] = np.stack([-r * a, a, -r, np.ones(nprob)], 1)[m]
    lim[m] = np.stack([v, v * 0.5], 1)[m]
    m = k == 3
    s = 0.5 + 0.75 * a
    c[m] = np.stack([-s * r ** 3, 3 * s * r * r, -3 * s * r, s], 1)[m]
    lim[m] = np.stack([r - u1, r + u2], 1)[m]
    m = k == 4
    c[m] = np.stack([5.0 + a, np.zeros(nprob), a, np.zeros(nprob)], 1)[m]
    lim[m] = np.stack([-u1, u2], 1)[m]
    m = np.arange(nprob) % 16 == 12                           # no root in a bracket of a few 1e-9: newton bisects to :953
    c[m] = np.stack([5.0 + a, np.ones(nprob), np.zeros(nprob), np.zeros(nprob)], 1)[m]
    lim[m] = np.stack([r, r + 1e-9 * (1.0 + a)], 1)[m]
    m = k == 6
    r1, r2, r3 = r, r + 1.0, r - 1.5
    c[m] = np.stack([-r1 * r2 * r3, r1 * r2 + r1 * r3 + r2 * r3, -(r1 + r2 + r3), np.ones(nprob)], 1)[m]
    lim[m] = np.stack([r3 - u1, r2 + u2], 1)[m]
    return np.ascontiguousarray(c), np.ascontiguousarray(lim)


class CubicBatch:
    """Device context of one batch of cubics (and, with count=True, the counting wrapper around it)."""

    def __init__(self, c, count=False):
        so = lib()
        self.c = np.ascontiguousarray(c, dtype=np.float64)
        self.nprob = len(self.c)
        self.inner = so.cubic_create(self.nprob, self.c.ctypes.data_as(dp))
        if not self.inner:
            raise RuntimeError("cubic_create failed (no GPU?)")
        self.counter = so.counting_create(self.inner) if count else None
        self.ctx = self.counter or self.inner
        self.launch = so.counting_launch if count else so.cubic_launch
        self.launch_diff = so.counting_launch_diff if count else so.cubic_launch_diff

    def points(self):
        so = lib()
        n = so.counting_size(self.counter)
        xs = np.zeros(n)
        pr = np.zeros(n, dtype=np.int32)
        so.counting_get(self.counter, xs.ctypes.data_as(dp), pr.ctypes.data_as(ip))
        return xs, pr

    def call_sizes(self):
        sz = np.zeros(self.calls(), dtype=np.int64)
        lib().counting_call_sizes(self.counter, sz.ctypes.data_as(C.POINTER(C.c_int64)))
        return sz

    def calls(self, deriv=False):
        return lib().counting_calls(self.counter, 1 if deriv else 0)

    def close(self):
        so = lib()
        if self.counter:
            so.counting_destroy(self.counter)
            self.counter = None
        if self.inner:
            so.cubic_destroy(self.inner)
            self.inner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
