"""CPU tests of the limit formulas (tests/expr_limit_cases.py): what the compiler makes of them -- shapes, root masks, the
operand-root fields at and above 128, the last constant -- the restatement of a whole point list against a point at a time,
its Jacobian against a complex step of its own values, every generated value finite, and the reference's solver on the
32-parameter family the device solves are held to (tests/test_gpu_expr_limits.py)."""
import numpy as np
import pytest

import expr_limit_cases as LC
import expr_restatement as R
import pwfun_restatement as PW

EPS = 2.0 ** -52


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


@pytest.mark.parametrize("name", list(LC.FORMULAS))
def test_shapes_masks_and_roots(name):
    shape, root_mask = LC.FORMULAS[name][5:7]
    e = LC.compile_formula(name)
    assert (e.nvar, e.nparams, e.ninstr, e.nconst, e.depth) == shape
    op, arg, consts, mask = e.program()
    aroot, broot = e.roots()
    assert int(mask[-1]) == root_mask
    assert (int(aroot.max()), int(broot[-1])) == LC.ROOTS[name] and int(broot[:-1].max(initial=0)) == 0
    assert (aroot <= np.maximum(np.arange(e.ninstr) - 2, 0)).all()    # a lower operand lies at least two instructions back
    if name == "full256":                                             # c63 * p31, the last ADD: constant 63, roots 251 and 252
        assert [PW.OPS[o] for o in op[-4:]] == ["CONST", "PARAM", "MUL", "ADD"] and list(arg[-4:-2]) == [63, 31]
        assert list(aroot[-2:]) == [252, 251] and consts[63] == 0.5 + 63 / 64.0 and list(consts) == [0.5 + i / 64.0 for i in range(64)]
    if name == "where256":                                            # c at 2, the first branch ends at 131, the second at 254
        assert PW.OPS[op[-1]] == "WHERE" and (int(aroot[-1]), int(broot[-1])) == (2, 131)
        assert int(mask[2]) == 0 and int(mask[131]) == 0x7fffffff and int(mask[254]) == 0xfffffffe
    if name == "sparse32":
        assert [(PW.OPS[o], int(a)) for o, a in zip(op, arg)] == [("PARAM", 31), ("VAR", 0), ("MUL", 0), ("PARAM", 0), ("SUB", 0)]
    if name == "deep16":
        import nonlin_amd as nl
        p = nl.Expr(*LC.DEEP16_PADDED)
        assert (p.nparams, p.ninstr, p.depth) == (32, 59, 16) and int(p.program()[3][-1]) == 0x7fff
        assert all(np.array_equal(a, b) for a, b in zip(p.program(), e.program()))


@pytest.mark.parametrize("m", [1, 5, 129])
@pytest.mark.parametrize("name", list(LC.FORMULAS))
def test_generated_values_are_finite_and_a_list_is_its_points(name, m):
    """Every residual and every Jacobian entry of the restatement is finite on the generated data, at the truth and at the
    start; restate() on a list of points gives the bits of a pass per point."""
    nprob = 5
    prog, t, y, xt, x0 = LC.limit_problems(name, m, nprob=nprob, seed=11 + m)
    w = np.random.default_rng(m).uniform(0.5, 2.0, (nprob, m))
    w[:, ::3] = 0.0
    for X in (xt, x0):
        for wq in (None, w):
            F, J = LC.restate(prog, X, t, y, wq)
            assert F.shape == (nprob, m) and J.shape == (nprob, X.shape[1], m)
            assert np.isfinite(F).all() and np.isfinite(J).all() and np.isfinite(LC.restate(prog, X, t)[0]).all()
            for q in range(nprob):
                wp = wq[q] if wq is not None else None
                assert np.array_equal(_bits(F[q]), _bits(PW.residual(prog, X[q], t[:, q], y[q], wp)))
                assert np.array_equal(_bits(J[q]), _bits(PW.jacobian(prog, X[q], t[:, q], wp).T))
    F, J = LC.restate(prog, x0, t, y)
    unnamed = [j for j in range(x0.shape[1]) if not (LC.FORMULAS[name][6] >> j) & 1]
    assert (_bits(J[:, unnamed]) == 0).all()                          # a column the formula does not name: +0.0


def _complex_step(prog, x, tv, y, w, J):
    """The bound of test_expr_cpu.py: 64 eps |entry| + 64 eps times the column's largest."""
    h = 1e-30
    for j in range(J.shape[1]):
        xc = x.astype(np.complex128)
        xc[j] += 1j * h
        col = R.residual(prog, xc, tv, y, w).imag / h
        bound = 64 * EPS * np.abs(col) + 64 * EPS * np.abs(col).max()
        assert (np.abs(J[:, j] - col) <= bound).all(), (j, (np.abs(J[:, j] - col) / bound).max())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", [k for k in LC.FORMULAS if k != "where256"])
def test_analytic_jacobian_against_complex_step(name, weighted):
    m = 129
    prog, t, y, xt, x0 = LC.limit_problems(name, m, nprob=2)
    rng = np.random.default_rng(5)
    for p in range(2):
        w = rng.uniform(0.5, 2.0, m) if weighted else None
        J = PW.jacobian(prog, x0[p], t[:, p], w)
        assert J.shape == (m, x0.shape[1])
        assert np.array_equal(_bits(J), _bits(R.jacobian(prog, x0[p], t[:, p], w)))      # (both restatements: the same table)
        _complex_step(prog, x0[p], t[:, p], y[p], w, J)


def test_where256_is_its_two_sides():
    """A comparison has no complex step: where256's value and Jacobian are, row by row, those of the branch the row selects
    -- the first where t - 0.5 >= 0 -- and each branch alone agrees with its complex step."""
    import nonlin_amd as nl
    m = 129
    f, v, p = LC.FORMULAS["where256"][:3]
    s1, s2 = f[len("where(t-0.5,"):-1].split(",")
    prog, t, y, xt, x0 = LC.limit_problems("where256", m, nprob=2)
    sides = [nl.Expr(s, v, p).program() for s in (s1, s2)]
    for q in range(2):
        tv = t[:, q]
        first = tv[0] - 0.5 >= 0.0
        assert 40 <= first.sum() <= m - 40                           # both branches are taken
        J = PW.jacobian(prog, x0[q], tv)
        F = PW.value(prog, x0[q], tv)
        Js = [R.jacobian(s, x0[q], tv) for s in sides]
        for s, Jside in zip(sides, Js):
            _complex_step(s, x0[q], tv, y[q], None, Jside)
        assert np.array_equal(_bits(F), _bits(np.where(first, R.value(sides[0], x0[q], tv), R.value(sides[1], x0[q], tv))))
        assert np.array_equal(_bits(J), _bits(np.where(first[:, None], Js[0], Js[1])))
        assert (_bits(J[first, 31]) == 0).all() and (_bits(J[~first, 0]) == 0).all()      # the branch that does not name it: +0.0
        assert (J[first, 0] != 0).all() and (J[~first, 31] != 0).all()


@pytest.mark.parametrize("analytic", [False, True])
def test_reference_solver_fits_the_32_parameter_family(oracle, analytic):
    """As test_expr_cpu.py::test_reference_solver_fits_the_generated_cases: the reference's lm_solve returns 0 for every
    problem of the wide32 family in 1 .. 30 Jacobian evaluations and fits to the noise level, with either Jacobian."""
    m, n = LC.SOLVE_M, 32
    prog, t, y, xt, x0 = LC.limit_problems(LC.SOLVE_NAME, m, nprob=LC.SOLVE_NPROB)
    o = oracle.default_options(max_evals=LC.MAX_EVALS)
    counts = []
    for p in range(LC.SOLVE_NPROB):
        tv = t[:, p]
        fcn = lambda x, f: f.__setitem__(slice(None), R.residual(prog, x, tv, y[p]))
        jac = (lambda x, J: J.__setitem__((slice(None), slice(None)), R.jacobian(prog, x, tv))) if analytic else None
        rc, x, f, ib = oracle.lm_solve(fcn, m, n, x0[p], jac=jac, opts=o)
        assert rc == 0 and 1 <= ib["jacobian_count"] <= 30, (p, rc, ib)
        assert np.abs(f).max() <= 2e-3 * np.abs(y[p]).max(), (p, np.abs(f).max() / np.abs(y[p]).max())
        counts.append(ib["jacobian_count"])
    print("wide32 reference solves: Jacobian evaluations", counts)
