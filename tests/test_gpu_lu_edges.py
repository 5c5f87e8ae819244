"""The LU kernels (nlh_kernels_lu.h) exactly at every form's size, pivot and skip edges, against the oracle's nlo_lu_factor /
nlo_lu_solve on the inputs of tests/lu_cases.py: ipvt, info, every element of the packed factors and the solution bit for
bit (a NaN must face a NaN).  No tolerance anywhere but in the contract-mode test, which holds the FMA kernels to the
backward identity.  tests/test_lu_cases_cpu.py shows on the host that the inputs reach what they are built for and which
kernel forms every size launches (`panel_plan`).

NLH_LU_PANEL and NLH_LU_CONTRACT are read once per process, so every other panel mode runs in a child process: a fresh
interpreter with its own time limit, run once.

One test that launches each kernel instance, read off `panel_plan` and the launchers (not off a trace); `factor` stands for
test_lu_factor_default_mode_is_the_oracle_bit_for_bit, `modes` for test_lu_factor_forced_panel_modes_are_the_oracle_bit_for_bit,
`contract` for test_lu_contract_mode_satisfies_the_backward_identity:
  k_lu_factor, 256 / 1024 threads            factor[63-normal] / factor[96-normal]
  k_lu_solve<false>                          test_lu_solve_on_packed_factors_is_the_oracle_bit_for_bit[17]
  k_lu_solve<true>                           test_lu_solve_global_memory_form_batch_of_two
  k_lu_panel, k_lu_swap_trsm                 factor[1025-normal] (below 1025 rows: modes[0])
  k_lu_panel_lds                             modes[0]
  k_lu_gemm<false> / <true>                  factor[128-normal] / contract[1-cases0]
  k_lu_panel_reg<1,32,256,false> / true      factor[128-normal] / contract[1-cases0]
  k_lu_panel_reg<2,32,256,false> / true      factor[257-normal] / contract[1-cases0]
  k_lu_panel_reg<4,16,256,false> / true      factor[513-normal] / contract[1-cases0]
  k_lu_panel_reg<2,16,512,false> / true      modes[2] / contract[2-cases1]
  k_lu_move_trsm<32,false> / true            factor[128-normal] / contract[1-cases0]
  k_lu_move_trsm<16,false> / true            factor[129-normal] (its 1-by-1 last panel) / contract[1-cases0] (n = 513)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lu_cases as LC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- factor, default mode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", LC.factor_cases())
def test_lu_factor_default_mode_is_the_oracle_bit_for_bit(ds, oracle, n, kind):
    """Register panels with 1, 2 and 4 rows per thread, the global-memory panel above 1024 rows, both block-row widths,
    1-by-1 last panels, the unblocked kernel on both sides of its block-size switch; interchange patterns that leave move
    lists of 0, 1 and nb entries; keys decided by the low word and by the position; two zero columns in different panels
    (info stays 6); -0.0 and denormal pivots.  Each case is followed by a dense solve."""
    if kind == "two_zero_cols":
        assert LC.reference(oracle, kind, n)[3] == 6
    assert LC.device_factor_mismatches(ds, oracle, n, kind) == []


_FACTOR_CHILD = '''
import sys
sys.path.insert(0, "tests")
import lu_cases as LC
from nonlin_amd.device import DeviceSolver
from oracle import pyoracle as O
ds = DeviceSolver(0)
cases = LC.child_factor_cases()
bad = [(n, kind, what) for n, kind in cases for what in LC.device_factor_mismatches(ds, O, n, kind)]
bad += [(n, "batch: " + kind, what) for n in LC.BATCH_SIZES for kind, what in LC.device_batch_mismatches(ds, O, n)]
for b in bad:
    print("MISMATCH", b)
print("cases", len(cases), "mismatches", len(bad))
sys.exit(1 if bad else 0)
'''


def _child(code, env, *args, timeout=300):
    out = subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, timeout=timeout,
                         env=dict(os.environ, **env), cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    return out.stdout


@pytest.mark.parametrize("mode", [0, 2])
def test_lu_factor_forced_panel_modes_are_the_oracle_bit_for_bit(mode):
    """NLH_LU_PANEL=0: k_lu_panel_lds (short last panels at n = 129 and 143, exactly 1024 rows, ties and scattered NaNs, whose
    DPP arg-max drops NaNs differently from the key form) and k_lu_swap_trsm below 1025 rows -- the form launch_lu_factor also
    falls back to without its move-list workspace.  NLH_LU_PANEL=2: k_lu_panel_reg<2,16,512>.  The case list of the default
    mode from n = 128 on and the mixed batches, every mismatch reported as (n, kind, what)."""
    out = _child(_FACTOR_CHILD, {"NLH_LU_PANEL": str(mode)})
    assert f"cases {len(LC.child_factor_cases())} mismatches 0" in out


@pytest.mark.parametrize("n", LC.BATCH_SIZES)
def test_lu_mixed_batch(ds, oracle, n):
    """Five problems of different kinds in one launch (a regular one, ties, two zero columns, scattered NaNs, no interchange
    at all): info, ipvt and factors per problem.  The forced-mode children run the same batches."""
    refs = {k: LC.reference(oracle, k, n) for k in LC.BATCH_KINDS}
    assert refs["two_zero_cols"][3] == 6 and refs["normal"][3] == 0 and refs["dominant"][3] == 0
    assert LC.device_batch_mismatches(ds, oracle, n) == []


# ---- solve on packed factors built directly ------------------------------------------------------------------------------------
SOLVE_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 95, 96, 97, 1040, 1041, 1057)
POISON_SIZES = (17, 33, 96, 1041)


def _dev_solve(ds, M, ipvt, B):
    """One launch: len(B) right-hand sides on copies of the packed factor M[c, r] (a list of factors: one each)."""
    Ms = M if isinstance(M, list) else [M] * len(B)
    ips = ipvt if isinstance(ipvt, list) else [ipvt] * len(B)
    LUd = torch.tensor(np.stack(Ms), device=ds.device)
    ipd = torch.tensor(np.stack(ips).astype(np.int32), device=ds.device)
    bd = torch.tensor(np.stack(B), device=ds.device)
    ds.lu_solve(LUd, ipd, bd)
    torch.cuda.synchronize()
    return bd.cpu().numpy()


def _solve_cases(oracle, n):
    """(name, M, ipvt, [(rhs name, b)]): the packed factor with every right-hand-side kind, the integer factor and the oracle's
    factors of `ties` with the integer right-hand sides."""
    out = [("packed", *LC.packed_lu(n), [(k, LC.rhs(k, n)) for k in LC.rhs_kinds(n)])]
    ints = [(f"ints{s}", LC.rhs("ints", n, s)) for s in range(3)] + [(k, LC.rhs(k, n)) for k in LC.rhs_kinds(n) if k[0] == "e"]
    out.append(("int", *LC.int_lu(n), ints))
    if n >= 2:
        Mt, ipt, _ = LC.ties_lu(oracle, n)
        out.append(("ties", Mt, ipt, ints))
    return out


@pytest.mark.parametrize("n", SOLVE_SIZES)
def test_lu_solve_on_packed_factors_is_the_oracle_bit_for_bit(ds, oracle, n):
    """k_lu_solve<false> without a factorisation: the 16-column block at 15 / 16 / 17 and 31 / 32 / 33, the thread count at
    95 / 96 / 97, the second-trip branches (rows read from global memory) above 1040; dense, zero, unit, -0.0 and integer
    right-hand sides, so that forward and back steps are skipped at the start, at block boundaries and in mid-sweep.  At
    n in {17, 33, 96, 1041} also on factors with NaN in everything a skipped step must not read: the answer must stay the
    unpoisoned oracle's, finite."""
    bad = []
    for name, M, ipvt, rhss in _solve_cases(oracle, n):
        with np.errstate(all="ignore"):
            wants = [LC.oracle_solve(oracle, M, ipvt, b) for _, b in rhss]
        gots = _dev_solve(ds, M, ipvt, [b for _, b in rhss])
        bad += [(n, name, k, "solution") for (k, _), g, w in zip(rhss, gots, wants) if not LC.same_bits(g, w)]
        if n in POISON_SIZES:
            Ps = [LC.poison(M, ipvt, b) for _, b in rhss]
            assert sum(int(np.isnan(P).sum()) for P in Ps) > 0
            gots = _dev_solve(ds, Ps, [ipvt] * len(Ps), [b for _, b in rhss])
            for (k, _), g, w in zip(rhss, gots, wants):
                if not (np.isfinite(w).all() and LC.same_bits(g, w)):
                    bad.append((n, name, k, "poisoned", int(np.isnan(g).sum())))
    assert bad == []


@pytest.mark.parametrize("n,k", [(33, 20), (1041, 1030), (1041, 7)])
def test_lu_solve_zero_diagonal_propagates_as_in_the_oracle(ds, oracle, n, k):
    """u(k, k) exactly zero under a non-zero b(k): x(k) is an infinity, and infinities and NaNs spread through the rest of
    the back substitution exactly as in the sequential loop."""
    M, ipvt = LC.packed_lu(n)
    M[k, k] = 0.0
    b = LC.rhs("dense", n)
    with np.errstate(all="ignore"):
        want = LC.oracle_solve(oracle, M, ipvt, b)
    assert np.isinf(want[k]) and (k == 0 or not np.isfinite(want[:k]).all())
    got = _dev_solve(ds, M, ipvt, [b])[0]
    assert LC.same_bits(got, want)


def test_lu_solve_batch_of_three(ds, oracle):
    """Three problems at n = 33 with different factors, pivots and right-hand sides in one launch."""
    n = 33
    fac = [LC.packed_lu(n, 0), LC.packed_lu(n, 1), LC.int_lu(n, 2)]
    B = [LC.rhs("dense", n, 0), LC.rhs("e16", n), LC.rhs("ints", n, 2)]
    assert not np.array_equal(fac[0][1], fac[1][1])
    got = _dev_solve(ds, [f[0] for f in fac], [f[1] for f in fac], B)
    for p in range(3):
        assert LC.same_bits(got[p], LC.oracle_solve(oracle, fac[p][0], fac[p][1], B[p])), p


def test_lu_solve_global_memory_form_batch_of_two(ds, oracle):
    """k_lu_solve<true> (n = 13138: P b and the pivots in global memory) with two problems: the second one's slice of the
    workspace.  Problem 1 has a right-hand side that is mostly -0.0, so the global-memory form also takes skips.  (One
    n-by-n host array alive at a time: 1.4 GB each.)"""
    n = 13138
    LUd = torch.empty((2, n, n), dtype=torch.float64, device=ds.device)
    ips, B, want = [], [LC.rhs("dense", n), LC.rhs("neg_zero", n, 1)], []
    for p in range(2):
        M, ipvt = LC.packed_lu(n, p)
        want.append(LC.oracle_solve(oracle, M, ipvt, B[p]))
        LUd[p].copy_(torch.from_numpy(M))
        torch.cuda.synchronize()
        ips.append(ipvt)
        del M
    ipd = torch.tensor(np.stack(ips), device=ds.device)
    bd = torch.tensor(np.stack(B), device=ds.device)
    ds.lu_solve(LUd, ipd, bd)
    torch.cuda.synchronize()
    del LUd
    got = bd.cpu().numpy()
    for p in range(2):
        assert np.isfinite(want[p]).all()
        assert LC.same_bits(got[p], want[p]), p


# ---- contract mode -------------------------------------------------------------------------------------------------------------
_CONTRACT_CHILD = '''
import json, sys
sys.path.insert(0, "tests")
import numpy as np, torch
import lu_cases as LC
from nonlin_amd.device import DeviceSolver
ds = DeviceSolver(0)
bad = []
for n, kind in json.loads(sys.argv[1]):
    a = LC.matrix(kind, n)
    Ad = torch.tensor(LC.dev_layout(a), device=ds.device).unsqueeze(0)
    ipd, infod = ds.lu_factor(Ad)
    torch.cuda.synchronize()
    ip, lu = ipd[0].cpu().numpy(), Ad[0].cpu().numpy().T
    valid = bool((ip >= np.arange(n)).all() and (ip < n).all())
    r = LC.backward_ratio(a, lu, ip) if valid else float("inf")
    print(f"contract n={n} {kind}: backward ratio {r:.3f} (units of 2^-53 |L||U|), bound {LC.backward_bound(n)}", flush=True)
    if int(infod[0]) != 0:
        bad.append((n, kind, "info", int(infod[0])))
    if not valid:
        bad.append((n, kind, "ipvt"))
    if not r <= LC.backward_bound(n):
        bad.append((n, kind, "backward ratio", r))
for b in bad:
    print("FAILED", b)
print("cases done, failures", len(bad))
sys.exit(1 if bad else 0)
'''


@pytest.mark.parametrize("mode,cases", [(1, [(n, k) for n in (257, 513, 1025) for k in ("normal", "scaled_rows", "shift")]),
                                        (2, [(n, k) for n in (513, 1025) for k in ("normal", "shift")])])
def test_lu_contract_mode_satisfies_the_backward_identity(mode, cases):
    """NLH_LU_CONTRACT=1 instantiates every FAST = true template (mode 2: k_lu_panel_reg<2,16,512,true> as well): the bits
    change, so neither bits nor pivots are asserted -- info == 0, j <= ipvt[j] < n, and
    |P A - L U| <= (n + 3) 2^-53 |L| |U| entry by entry, the bound derived in tests/lu_cases.py, which holds with fused
    multiply-adds and inside which tests/test_lu_cases_cpu.py shows the oracle's own factors of the same inputs."""
    out = _child(_CONTRACT_CHILD, {"NLH_LU_CONTRACT": "1", "NLH_LU_PANEL": str(mode)}, json.dumps(cases))
    assert "cases done, failures 0" in out and out.count("backward ratio") == len(cases)
