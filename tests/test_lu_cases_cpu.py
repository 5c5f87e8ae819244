"""The inputs and helpers of tests/lu_cases.py on the host: every engineered matrix reaches the pivot sequence and the
move-list count it is built for (by the oracle's own factorisation), `panel_plan` names the expected kernel forms on both
sides of every size switch, `backward_ratio` passes the oracle's factors inside the bound and fails two faulty factors of
the kind it is for, the numpy restatement of the solve sweeps is nlo_lu_solve bit for bit, and `poison` leaves the oracle's
answer untouched.  Needs no GPU."""
import numpy as np
import pytest

import lu_cases as LC


def _ipvt(oracle, kind, n):
    return LC.reference(oracle, kind, n)[2]


# ---- the engineered pivot sequences ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 257, 513])
def test_engineered_kinds_pivot_as_stated(oracle, n):
    j = np.arange(n)
    for kind in ("dominant", "shift", "reverse", "block_perm"):
        assert LC.reference(oracle, kind, n)[3] == 0, kind
    assert np.array_equal(_ipvt(oracle, "dominant", n), j)
    assert np.array_equal(_ipvt(oracle, "shift", n)[:n - 1], j[:n - 1] + 1) and _ipvt(oracle, "shift", n)[n - 1] == n - 1
    assert np.array_equal(_ipvt(oracle, "reverse", n)[:n // 2], n - 1 - j[:n // 2])
    ip = _ipvt(oracle, "block_perm", n)
    assert np.array_equal(ip // 16, j // 16)               # every pivot inside its aligned 16-row block
    assert np.mean(ip != j) > 0.5                          # (expected: 1 - H_16 / 16 = 0.79)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n", [129, 257, 513, 1025, 1057])
def test_move_list_counts_of_the_engineered_kinds(oracle, n, mode):
    """The count a register panel leaves at mv[32]: 0 with no interchange at all, 0 with interchanges that stay inside the
    block row, exactly 1 for the chain of `shift` (0 in the last panel, whose displaced row ends inside it), nb for the
    first register panel of `reverse`.  Above 1024 only the stated sequences are used (the oracle's loop takes a second a
    matrix there, and the CPU test above checks them where it is cheap)."""
    plan = LC.panel_plan(n, mode)
    reg = [p for p in plan if p.form.startswith("k_lu_panel_reg")]
    assert reg and reg[-1].jb + reg[-1].nb == n
    j = np.arange(n)
    if n <= 513:
        seqs = {k: _ipvt(oracle, k, n) for k in ("dominant", "block_perm", "shift", "reverse")}
    else:
        seqs = {"dominant": j, "shift": np.minimum(j + 1, n - 1), "reverse": np.where(j < n // 2, n - 1 - j, j)}
    assert set(LC.move_list_counts(seqs["dominant"], plan).values()) == {0}
    if "block_perm" in seqs:
        assert not np.array_equal(seqs["block_perm"], j)
        assert set(LC.move_list_counts(seqs["block_perm"], plan).values()) == {0}
    cs = LC.move_list_counts(seqs["shift"], plan)
    assert [cs[p.jb] for p in reg] == [1] * (len(reg) - 1) + [0]
    cr = LC.move_list_counts(seqs["reverse"], plan)
    if reg[0].jb < n // 2:
        assert cr[reg[0].jb] == reg[0].nb
    # and the helper itself: a lone interchange into the block row displaces nothing, one below it displaces one row
    one = j.copy()
    one[reg[0].jb] = reg[0].jb + reg[0].nb - 1
    assert LC.move_list_counts(one, plan)[reg[0].jb] == 0
    one[reg[0].jb] = n - 1
    assert LC.move_list_counts(one, plan)[reg[0].jb] == (1 if n - 1 >= reg[0].jb + reg[0].nb else 0)


@pytest.mark.parametrize("n", [129, 513, 1057])
def test_low_word_first_pivot_is_decided_by_the_low_word_then_the_position(oracle, n):
    """Column 0 of `low_word`: the largest key stands at two rows, -x first and +x second, and the first wins; the runner-up
    among the other rows has the same high word and a smaller low word."""
    a = LC.matrix("low_word", n)
    bits = np.abs(a[:, 0]).view(np.uint64)
    hi, lo = bits >> np.uint64(32), bits & np.uint64(0xffffffff)
    i1, i2 = LC.low_word_tie_rows(n, 0)
    assert (hi == 0x3ff00000).all()
    assert bits[i1] == bits[i2] == bits.max() and a[i1, 0] < 0 < a[i2, 0]
    rest = np.delete(bits, [i1, i2])
    runner = rest.max()
    assert runner >> np.uint64(32) == hi[i1] and (runner & np.uint64(0xffffffff)) < lo[i1]
    assert int(np.argmax(np.abs(a[:, 0]))) == i1
    if n <= 513:
        assert _ipvt(oracle, "low_word", n)[0] == i1
        assert LC.reference(oracle, "low_word", n)[3] == 0


def test_two_zero_columns_report_the_first(oracle):
    for n in (129, 257):
        assert LC.reference(oracle, "two_zero_cols", n)[3] == 6
    plan = LC.panel_plan(1057, 1)
    owner = lambda c: next(p for p in plan if p.jb <= c < p.jb + p.nb)
    assert owner(5).form == "k_lu_panel" and owner(1054).form.startswith("k_lu_panel_reg")


# ---- the launch plan ---------------------------------------------------------------------------------------------------------
def test_panel_plan_on_both_sides_of_every_switch():
    P = LC.panel_plan
    assert [p.form for p in P(127)] == ["k_lu_factor"] and P(127)[0].threads == 1024
    assert P(95)[0].threads == 256 and P(96)[0].threads == 1024
    for mode in (0, 1, 2):
        assert P(127, mode) == P(127, 1)
    # 128: the blocked path starts; one row per thread up to 256 rows, 32 wide
    assert [(p.jb, p.nb, p.form, p.threads) for p in P(128)] == [(0, 32, "k_lu_panel_reg<1,32,256>", 128), (32, 32, "k_lu_panel_reg<1,32,256>", 128),
                                                                 (64, 32, "k_lu_panel_reg<1,32,256>", 64), (96, 32, "k_lu_panel_reg<1,32,256>", 64)]
    assert not P(128)[-1].gemm and P(128)[0].gemm
    # 129: a last panel of one row and one column on 64 threads, through the 16-wide block-row kernel
    last = P(129)[-1]
    assert (last.jb, last.nb, last.form, last.threads, last.trsm, last.gemm) == (128, 1, "k_lu_panel_reg<1,32,256>", 64, "k_lu_move_trsm<16>", False)
    assert P(129)[0].trsm == "k_lu_move_trsm<32>"
    # 256 / 257: one to two rows per thread
    assert P(256)[0].form == "k_lu_panel_reg<1,32,256>" and P(256)[0].threads == 256
    assert P(257)[0].form == "k_lu_panel_reg<2,32,256>" and P(257)[0].threads == 192
    assert P(257)[1].form == "k_lu_panel_reg<1,32,256>"
    # 512 / 513: 32 to 16 wide, two to four rows per thread (mode 2: two rows on up to 512 threads)
    assert (P(512)[0].form, P(512)[0].nb, P(512)[0].threads) == ("k_lu_panel_reg<2,32,256>", 32, 256)
    assert (P(513)[0].form, P(513)[0].nb, P(513)[0].threads) == ("k_lu_panel_reg<4,16,256>", 16, 192)
    assert (P(513, 2)[0].form, P(513, 2)[0].threads) == ("k_lu_panel_reg<2,16,512>", 320)
    assert P(513)[0].trsm == "k_lu_move_trsm<16>" and P(513)[1].form == "k_lu_panel_reg<2,32,256>"
    # 1024 / 1025: register to global-memory panel
    assert (P(1024)[0].form, P(1024)[0].threads) == ("k_lu_panel_reg<4,16,256>", 256)
    assert (P(1024, 2)[0].form, P(1024, 2)[0].threads) == ("k_lu_panel_reg<2,16,512>", 512)
    assert (P(1025)[0].form, P(1025)[0].nb, P(1025)[0].trsm) == ("k_lu_panel", 32, "k_lu_swap_trsm")
    assert P(1025)[1].form == "k_lu_panel_reg<4,16,256>" and P(1025)[1].jb == 32
    assert [p.form for p in P(1057)[:3]] == ["k_lu_panel", "k_lu_panel", "k_lu_panel_reg<4,16,256>"]
    # mode 0: the LDS panel (16 wide, a thread per row) up to 1024 rows, short last panels at 129 and 143
    assert {p.form for p in P(1024, 0)} == {"k_lu_panel_lds"} and P(1024, 0)[0].threads == 1024
    assert [p.form for p in P(1025, 0)[:2]] == ["k_lu_panel", "k_lu_panel_lds"] and P(1025, 0)[1].jb == 32
    assert (P(129, 0)[-1].nb, P(129, 0)[-1].threads) == (1, 64) and P(143, 0)[-1].nb == 15
    assert {p.trsm for p in P(300, 0)} == {"k_lu_swap_trsm"}
    for n in (128, 129, 143, 257, 513, 1024, 1025, 1057):
        for mode in (0, 1, 2):
            plan = P(n, mode)
            assert plan[0].jb == 0 and all(a.jb + a.nb == b.jb for a, b in zip(plan, plan[1:])) and plan[-1].jb + plan[-1].nb == n


def test_the_case_list_launches_every_kernel_instance():
    """Every panel form and both block-row widths are launched by a size of the lists the device tests run."""
    seen = {m: set().union(*(LC.kernels_of(n, m) for n, _ in (LC.factor_cases() if m == 1 else LC.child_factor_cases()))) for m in (0, 1, 2)}
    assert seen[1] >= {"k_lu_factor", "k_lu_panel", "k_lu_swap_trsm", "k_lu_gemm", "k_lu_panel_reg<1,32,256>", "k_lu_panel_reg<2,32,256>",
                       "k_lu_panel_reg<4,16,256>", "k_lu_move_trsm<16>", "k_lu_move_trsm<32>"}
    assert seen[0] == {"k_lu_panel", "k_lu_panel_lds", "k_lu_swap_trsm", "k_lu_gemm"}
    assert "k_lu_panel_reg<2,16,512>" in seen[2] and "k_lu_panel_reg<4,16,256>" not in seen[2]
    assert min(n for n, _ in LC.child_factor_cases()) == 128


# ---- the backward identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "scaled_rows", "shift"])
def test_oracle_factors_satisfy_the_backward_identity(oracle, kind):
    """|P A - L U| <= (n + 3) 2^-53 |L| |U| entry by entry for the oracle's own factors at n = 257: n from Higham's Theorem
    9.3, one unit for the multiplier formed as a * fl(1 / pivot) instead of a quotient, one for the longdouble product that
    stands for the exact one, one for what is left (derived in tests/lu_cases.py).  The contract-mode device test holds
    the FMA kernels to the same bound on the same inputs."""
    n = 257
    a, lu, ipvt, info = LC.reference(oracle, kind, n)[:4]
    assert info == 0
    r = LC.backward_ratio(a, lu, ipvt)
    print(f"oracle {kind} n={n}: backward ratio {r:.3f} (units of 2^-53 |L||U|), bound {LC.backward_bound(n)}")
    assert r <= LC.backward_bound(n)


def test_backward_ratio_sees_the_faults_it_is_for(oracle):
    """A float64 model of the blocked factorisation passes; the same model with one 64 x 64 trailing tile left un-updated by
    one panel fails, and so does one with a single interchange not applied outside its panel."""
    n = 257
    a = LC.matrix("normal", n)
    lu, ipvt = LC.blocked_lu_model(a)
    assert np.array_equal(ipvt, _ipvt(oracle, "normal", n))
    assert LC.backward_ratio(a, lu, ipvt) <= LC.backward_bound(n)
    for fault in (("tile", 0, 0, 0), ("tile", 3, 1, 2), ("tile", 6, 0, 0)):        # (step 6: a 33 x 33 trailing matrix, its only tile)
        lf, ipf = LC.blocked_lu_model(a, fault=fault)
        assert LC.backward_ratio(a, lf, ipf) > LC.backward_bound(n), fault
    for j in (0, 100, 250):
        assert ipvt[j] != j
        lf, ipf = LC.blocked_lu_model(a, fault=("swap", j))
        assert ipf[j] == ipvt[j]                       # (later pivots may differ: the model goes on with the rows it has)
        assert LC.backward_ratio(a, lf, ipf) > LC.backward_bound(n), j
    # and a wrong interchange sequence with the right factors
    wrong = np.array(ipvt)
    wrong[7] = 7 if ipvt[7] != 7 else 8
    assert LC.backward_ratio(a, lu, wrong) > LC.backward_bound(n)


# ---- the solve: restatement, skips, poison -------------------------------------------------------------------------------------
def _factors(oracle, which, n):
    if which == "ties":
        M, ipvt, _ = LC.ties_lu(oracle, n)
        return M, ipvt
    if which == "int":
        return LC.int_lu(n)
    return LC.packed_lu(n)


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 96, 130])
def test_sweep_restatement_is_the_oracle_bit_for_bit(oracle, n):
    for which in ("packed", "ties", "int"):
        M, ipvt = _factors(oracle, which, n)
        assert (ipvt >= np.arange(n)).all() and (ipvt < n).all()
        for kind in LC.rhs_kinds(n):
            b = LC.rhs(kind, n)
            with np.errstate(all="ignore"):
                want = LC.oracle_solve(oracle, M, ipvt, b)
            got, fskip, bskip = LC.solve_sweeps(M, ipvt, b)
            assert LC.same_bits(got, want), (which, n, kind)
            if kind == "zeros":
                assert fskip == list(range(n)) and bskip == list(range(n - 1, -1, -1))
            if kind == "dense" and which == "packed":
                assert not fskip and not bskip


@pytest.mark.parametrize("n", [17, 33, 96, 1041])
def test_right_hand_sides_take_the_skips_they_are_for(oracle, n):
    """Unit vectors skip every forward step before their index (as P b places it); -0.0 entries are skipped as zeros; the
    integer right-hand side on the factors of `ties` cancels to an exact zero in mid-sweep, at a step whose entry of P b was
    not zero."""
    M, ipvt = LC.packed_lu(n)
    for kind in LC.rhs_kinds(n):
        if kind[0] == "e":
            _, fskip, _ = LC.solve_sweeps(M, ipvt, LC.rhs(kind, n))
            pb = LC.solve_sweeps(np.zeros_like(M) + np.eye(n), ipvt, LC.rhs(kind, n))[0]      # (identity factors: x = P b)
            k = int(np.flatnonzero(pb)[0])
            assert fskip == list(range(k)), (n, kind)
    b = LC.rhs("neg_zero", n)
    pb = LC.apply_pivots(ipvt, b)
    x, fskip, bskip = LC.solve_sweeps(M, ipvt, b)
    assert fskip and all(pb[j] == 0.0 and np.signbit(pb[j]) for j in fskip), (n, "no -0.0 entry skipped")
    # integers: the factors of `ties` meet a cancellation now and then, the integer factors at every size, both ways
    hits = [0, 0]
    for seed in range(3):
        b = LC.rhs("ints", n, seed)
        Mi, ipi = LC.int_lu(n)
        x, fskip, bskip = LC.solve_sweeps(Mi, ipi, b)
        pb = LC.apply_pivots(ipi, b)
        assert np.isfinite(x).all() and np.abs(x).max() < 2.0 ** 40
        hits[0] += sum(pb[j] != 0.0 for j in fskip)
        hits[1] += len(bskip)
    assert hits[0] > 0 and hits[1] > 0, (n, hits)
    if n <= 96:
        Mt, ipt, info = LC.ties_lu(oracle, n)
        assert info == 0
        got = 0
        for seed in range(6):
            b = LC.rhs("ints", n, seed)
            x, fskip, bskip = LC.solve_sweeps(Mt, ipt, b)
            pb = LC.apply_pivots(ipt, b)
            got += sum(pb[j] != 0.0 for j in fskip)
            assert np.isfinite(x).all()
        assert got > 0, (n, "no cancellation to zero in the forward sweep")


@pytest.mark.parametrize("n", [17, 33, 96, 1041])
def test_poison_leaves_the_oracle_answer_bit_identical_and_finite(oracle, n):
    cases = [("packed", k) for k in LC.rhs_kinds(n)] + [("int", "ints"), ("int", "e16")] + ([("ties", "ints"), ("ties", "e16")] if n <= 96 else [])
    planted = 0
    for which, kind in cases:
        M, ipvt = _factors(oracle, which, n)
        b = LC.rhs(kind, n)
        P = LC.poison(M, ipvt, b)
        planted += int(np.isnan(P).sum())
        if kind == "dense":
            assert not np.isnan(P).any()
        if kind == "zeros":
            assert np.isnan(P).sum() == n * n
        want = LC.oracle_solve(oracle, M, ipvt, b)
        got = LC.oracle_solve(oracle, P, ipvt, b)
        assert np.isfinite(want).all() and LC.same_bits(got, want), (which, n, kind)
    assert planted > 0
    # the poison is live: the dense right-hand side on a factor poisoned for the zero vector turns NaN
    M, ipvt = LC.packed_lu(n)
    P = LC.poison(M, ipvt, LC.rhs("zeros", n))
    assert np.isnan(LC.oracle_solve(oracle, P, ipvt, LC.rhs("dense", n))).any()
