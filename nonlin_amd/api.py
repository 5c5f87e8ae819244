"""Host-side mirror of nonlin's plugin / solver interface for the hot path.

Same names, argument meaning and error behaviour as the reference types
(src/nonlin_multi_eqn_mult_var.f90, src/nonlin_least_squares.f90, src/nonlin_solve.f90,
src/nonlin_linesearch.f90, src/nonlin_types.f90), bound to the C ABI of
include/nonlin_hip.h.  Where the reference `error stop`s with an NL_* code this module
raises NonlinError(code).  All numerical work happens in libnonlin_hip.so on the GPU.

User callbacks follow the Fortran subroutines:
    fcn(x, f, args)      -- fill f (length m) in place             (vecfcn,      :14-25)
    jac(x, jac, args)    -- fill jac (m x n, Fortran order)        (jacobianfcn, :27-38)
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CURVE_GAUSS, CURVE_LORENTZ, CURVE_EXPDECAY, CURVE_KINDS, curve_nparams  # noqa: F401  (built-in curve models)
from ._lib import Expr, EXPR_OPS, EXPR_SPECIAL_OPS, EXPR_EXTENDED_OPS, EXPR_DEF_OPS, EXPR_SPECIAL2_OPS, wofz  # noqa: F401  (formula models, their special functions)
from ._lib import ParamMap, PMAP_FREE, PMAP_FIXED, PMAP_TIED  # noqa: F401  (parameter maps)
from ._lib import Group  # noqa: F401  (global fits)
from ._lib import GUESS_FALLBACK, GUESS_RANKDEF, GUESS_NONE, GUESS_MAX_M  # noqa: F401  (flags of DeviceSolver.curve_guess)
from ._lib import Loss, LOSS_LINEAR, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY, LOSS_KINDS  # noqa: F401  (robust losses)
from ._lib import Poisson  # noqa: F401  (Poisson likelihood fits)
from ._lib import Convolve, CONV_ZERO, CONV_HOLD  # noqa: F401  (instrument-response fits)
from ._lib import Separable  # noqa: F401  (separable fits)
from ._lib import Binned  # noqa: F401  (bin-integrated fits)

# src/nonlin_error_handling.f90:10-38
NL_NO_ERROR = 0
NL_INVALID_INPUT_ERROR = 201
NL_ARRAY_SIZE_ERROR = 202
NL_OUT_OF_MEMORY_ERROR = 105
NL_INVALID_OPERATION_ERROR = 104
NL_CONVERGENCE_ERROR = 106
NL_DIVERGENT_BEHAVIOR_ERROR = 206
NL_SPURIOUS_CONVERGENCE_ERROR = 207
NL_TOLERANCE_TOO_SMALL_ERROR = 208
NL_INDEX_OUT_OF_RANGE_ERROR = 209
NL_DIVIDE_BY_ZERO_ERROR = 210
NL_UNDEFINED_FUNCTION_ERROR = 211
NL_UNDERDEFINED_PROBLEM_ERROR = 212


class NonlinError(RuntimeError):
    """Raised where the reference executes `error stop <code>`."""

    def __init__(self, code):
        super().__init__(f"nonlin error stop {code}")
        self.code = code


class iteration_behavior:
    """src/nonlin_types.f90:8-29."""

    def __init__(self):
        self.iter_count = 0
        self.fcn_count = 0
        self.jacobian_count = 0
        self.gradient_count = 0
        self.converge_on_fcn = False
        self.converge_on_chng = False
        self.converge_on_zero_diff = False

    def _fill(self, c):
        self.iter_count = int(c.iter_count)
        self.fcn_count = int(c.fcn_count)
        self.jacobian_count = int(c.jacobian_count)
        self.gradient_count = int(c.gradient_count)
        self.converge_on_fcn = bool(c.converge_on_fcn)
        self.converge_on_chng = bool(c.converge_on_chng)
        self.converge_on_zero_diff = bool(c.converge_on_zero_diff)

    def as_dict(self):
        return dict(self.__dict__)


_default_handle = None


def default_handle():
    global _default_handle
    if _default_handle is None:
        _default_handle = _lib.Handle(0)
    return _default_handle


def _dp(a):
    return a.ctypes.data_as(_lib.c_double_p)


class vecfcn_helper:
    """src/nonlin_multi_eqn_mult_var.f90:41-65."""

    def __init__(self):
        self._fcn = None
        self._jac = None
        self._nfcn = 0
        self._nvar = 0

    def set_fcn(self, fcn, nfcn, nvar):          # :126-140
        self._fcn = fcn
        self._nfcn = int(nfcn)
        self._nvar = int(nvar)

    def set_jacobian(self, jac):                 # :143-153
        self._jac = jac

    def is_fcn_defined(self):                    # :156-164
        return self._fcn is not None

    def is_jacobian_defined(self):               # :167-175
        return self._jac is not None

    def get_equation_count(self):                # :280-287
        return self._nfcn

    def get_variable_count(self):                # :290-297
        return self._nvar

    def fcn(self, x, f, args=None):              # :178-195 (silently does nothing if unset)
        if self._fcn is not None:
            self._fcn(x, f, args)

    # -- C trampolines -----------------------------------------------------
    def _c_fcn(self, args):
        user = self._fcn
        if user is None:
            return C.cast(None, _lib.VECFCN)

        def tramp(ctx, n, xp, m, fp):
            x = np.ctypeslib.as_array(xp, shape=(n,))
            f = np.ctypeslib.as_array(fp, shape=(m,))
            user(x, f, args)
        return _lib.VECFCN(tramp)

    def _c_jac(self, args):
        user = self._jac
        if user is None:
            return C.cast(None, _lib.JACFCN)

        def tramp(ctx, n, xp, m, jp):
            x = np.ctypeslib.as_array(xp, shape=(n,))
            J = np.ctypeslib.as_array(jp, shape=(n, m)).T   # Fortran-order m x n view
            user(x, J, args)
        return _lib.JACFCN(tramp)

    def jacobian(self, x, jac, fv=None, args=None, handle=None):
        """vfh_jac_fcn (:198-277): analytic dispatch or forward differences (GPU column write).
        x is perturbed in place and restored; jac must be an m x n Fortran-order float64 array."""
        m, n = self._nfcn, self._nvar
        if x.shape != (n,):
            raise NonlinError(2)                 # :232-233
        if jac.shape != (m, n):
            raise NonlinError(3)                 # :234-235
        if not self.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)   # :240
        if not (jac.flags.f_contiguous and jac.dtype == np.float64):
            raise ValueError("jac must be a Fortran-order float64 array")
        h = handle or default_handle()
        cf, cj = self._c_fcn(args), self._c_jac(args)
        fvp = _dp(np.ascontiguousarray(fv, dtype=np.float64)) if fv is not None else None
        rc = h.lib.nlh_fd_jacobian(h.ptr, m, n, cf, cj, None, _dp(x), fvp, _dp(jac))
        h.check(rc, "nlh_fd_jacobian")
        if rc:
            raise NonlinError(rc)


class equation_solver:
    """src/nonlin_multi_eqn_mult_var.f90:67-91; defaults :69-77."""

    def __init__(self):
        self._max_eval = 100
        self._fcn_tol = 1.0e-8
        self._xtol = 1.0e-12
        self._gtol = 1.0e-12
        self._print_status = False
        self.handle = None
        # extension: 2 = NLH_FACTOR_EXACT (default: reference operation order, bit-identical results),
        # 0 = NLH_FACTOR_AUTO (J^T J + Cholesky), 1 = NLH_FACTOR_QR
        self.factor_policy = 2

    def get_max_fcn_evals(self): return self._max_eval
    def set_max_fcn_evals(self, n): self._max_eval = int(n)
    def get_fcn_tolerance(self): return self._fcn_tol
    def set_fcn_tolerance(self, x): self._fcn_tol = float(x)
    def get_var_tolerance(self): return self._xtol
    def set_var_tolerance(self, x): self._xtol = float(x)
    def get_gradient_tolerance(self): return self._gtol
    def set_gradient_tolerance(self, x): self._gtol = float(x)
    def get_print_status(self): return self._print_status
    def set_print_status(self, x): self._print_status = bool(x)

    def _options(self):
        o = _lib.default_options()
        o.max_evals = self._max_eval
        o.ftol = self._fcn_tol
        o.xtol = self._xtol
        o.gtol = self._gtol
        o.print_status = 1 if self._print_status else 0
        o.factor_policy = int(self.factor_policy)
        return o

    def _handle(self):
        return self.handle or default_handle()


def _check_xf(fcn, x, fvec):
    if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
        raise ValueError("x must be a contiguous float64 numpy array (it is updated in place)")
    if not (isinstance(fvec, np.ndarray) and fvec.dtype == np.float64 and fvec.flags.c_contiguous):
        raise ValueError("fvec must be a contiguous float64 numpy array (it is filled in place)")


class least_squares_solver(equation_solver):
    """src/nonlin_least_squares.f90:20-31."""

    def __init__(self):
        super().__init__()
        self._factor = 100.0                      # :25

    def get_step_scaling_factor(self):           # :80-93
        return self._factor

    def set_step_scaling_factor(self, x):        # :96-115
        x = float(x)
        self._factor = 0.1 if x < 0.1 else (100.0 if x > 100.0 else x)

    def solve(self, fcn, x, fvec, ib=None, args=None):
        """lss_solve (:118-391).  x: initial estimate -> solution; fvec: F at the solution."""
        _check_xf(fcn, x, fvec)
        if not fcn.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)   # :188
        m, n = fcn.get_equation_count(), fcn.get_variable_count()
        if n > m:
            raise NonlinError(NL_UNDERDEFINED_PROBLEM_ERROR)  # :189
        if x.shape != (n,):
            raise NonlinError(3)                  # :191-192
        if fvec.shape != (m,):
            raise NonlinError(4)                  # :193-194
        o = self._options()
        o.factor = self._factor
        h = self._handle()
        cib = _lib.IterationBehavior()
        cf, cj = fcn._c_fcn(args), fcn._c_jac(args)
        rc = h.lib.nlh_lm_solve(h.ptr, C.byref(o), m, n, cf, cj, None, _dp(x), _dp(fvec), C.byref(cib))
        h.check(rc, "nlh_lm_solve")
        if ib is not None:
            ib._fill(cib)
        if rc:
            raise NonlinError(rc)                 # :388-390


    def covariance(self, fcn, x, scaled=True, tol=None, args=None):
        """Parameter covariance of the fit at x (extension; MINPACK's covar on a fresh lmfactor of the Jacobian at x --
        NOT the last Jacobian of a solve).  fcn: the vecfcn_helper solve takes; x [n] is perturbed in place and restored.
        Returns (cov [n, n], sigma [n], rank, chi2): cov = (J^T J)^-1, times chi2 = ||F(x)||^2 / (m - n) when scaled;
        rows and columns of variables the data do not determine to within tol (default: machine epsilon, relative to the
        largest pivot) are zero and rank < n."""
        if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
            raise ValueError("x must be a contiguous float64 numpy array")
        if not fcn.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)
        m, n = fcn.get_equation_count(), fcn.get_variable_count()
        if x.shape != (n,):
            raise NonlinError(3)
        h = self._handle()
        cov = np.empty((n, n))
        sigma = np.empty(n)
        rank = C.c_int32(0)
        chi2 = C.c_double(0.0)
        cf, cj = fcn._c_fcn(args), fcn._c_jac(args)
        rc = h.lib.nlh_lm_covariance(h.ptr, m, n, cf, cj, None, _dp(x), int(bool(scaled)), 0.0 if tol is None else float(tol),
                                     _dp(cov), _dp(sigma), C.byref(rank), C.byref(chi2))
        h.check(rc, "nlh_lm_covariance")
        if rc:
            raise NonlinError(rc)
        return cov, sigma, int(rank.value), float(chi2.value)


class constrained_equation_solver(least_squares_solver):
    """src/nonlin_least_squares.f90:33-53 (bounds holder)."""

    def __init__(self):
        super().__init__()
        self._upper = np.zeros(0)
        self._lower = np.zeros(0)

    def get_upper_limits(self): return self._upper.copy()                                  # :796-808
    def set_upper_limits(self, x): self._upper = np.array(x, dtype=np.float64).ravel()      # :811-824
    def get_lower_limits(self): return self._lower.copy()                                  # :827-839
    def set_lower_limits(self, x): self._lower = np.array(x, dtype=np.float64).ravel()      # :842-855

    def apply_limits(self, x):                                                             # :858-883
        nl, nu = min(x.size, self._lower.size), min(x.size, self._upper.size)
        for i in range(nl):
            if x[i] < self._lower[i]:
                x[i] = self._lower[i]
        for i in range(nu):
            if x[i] > self._upper[i]:
                x[i] = self._upper[i]


class constrained_least_squares_solver(constrained_equation_solver):
    """src/nonlin_least_squares.f90:55-74."""

    def __init__(self):
        super().__init__()
        self._delta = 1.0                         # :60
        self._scaling = 1.0                       # :61

    def get_trust_region_radius(self): return self._delta                    # :888-895
    def set_trust_region_radius(self, x): self._delta = 1.0 if x <= 0.0 else float(x)       # :898-910
    def get_step_scaling_factor(self): return self._scaling                  # :913-920 (overrides the LM factor)
    def set_step_scaling_factor(self, x): self._scaling = 1.0 if x <= 0.0 else float(x)     # :923-935

    def solve(self, fcn, x, fvec, ib=None, args=None):
        """cls_solve (:938-1176)."""
        _check_xf(fcn, x, fvec)
        if not fcn.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)   # :988
        m, n = fcn.get_equation_count(), fcn.get_variable_count()
        if n > m:
            raise NonlinError(NL_UNDERDEFINED_PROBLEM_ERROR)  # :989
        if x.shape != (n,):
            raise NonlinError(3)
        if fvec.shape != (m,):
            raise NonlinError(4)
        big = float(np.finfo(np.float64).max)
        if self._lower.size != n:                 # :999-1009: wrong-sized limits are replaced (and stored)
            self.set_lower_limits(np.full(n, -big))
        if self._upper.size != n:
            self.set_upper_limits(np.full(n, big))
        lo = np.ascontiguousarray(self._lower)
        hi = np.ascontiguousarray(self._upper)
        o = self._options()
        h = self._handle()
        cib = _lib.IterationBehavior()
        cf, cj = fcn._c_fcn(args), fcn._c_jac(args)
        rc = h.lib.nlh_cls_solve(h.ptr, C.byref(o), self._delta, self._scaling, _dp(lo), _dp(hi), m, n, cf, cj, None,
                                 _dp(x), _dp(fvec), C.byref(cib))
        h.check(rc, "nlh_cls_solve")
        if ib is not None:
            ib._fill(cib)
        if rc:
            raise NonlinError(rc)                 # :1173-1175


class line_search:
    """src/nonlin_linesearch.f90:18-65 (configuration; the search runs inside newton_solver)."""

    def __init__(self):
        self._max_eval = 100                      # :35
        self._alpha = 1.0e-4                      # :38
        self._factor = 0.1                        # :46

    def get_max_fcn_evals(self): return self._max_eval
    def set_max_fcn_evals(self, x): self._max_eval = int(x)
    def get_scaling_factor(self): return self._alpha
    def set_scaling_factor(self, x): self._alpha = float(x)
    def get_distance_factor(self): return self._factor

    def set_distance_factor(self, x):            # :133-149
        x = float(x)
        self._factor = 0.1 if x <= 0.0 else (0.99 if x >= 1.0 else x)


class line_search_solver(equation_solver):
    """src/nonlin_solve.f90:20-41, 92-151."""

    def __init__(self):
        super().__init__()
        self._line_search = None
        self._use_line_search = True              # :30

    def get_line_search(self):                   # :92-100 (returns a copy)
        if self._line_search is None:
            return None
        ls = line_search()
        ls.__dict__.update(self._line_search.__dict__)
        return ls

    def set_line_search(self, ls):               # :103-111
        c = line_search()
        c.__dict__.update(ls.__dict__)
        self._line_search = c

    def set_default_line_search(self):           # :114-121
        self.set_line_search(line_search())

    def is_line_search_defined(self):            # :124-131
        return self._line_search is not None

    def get_use_line_search(self): return self._use_line_search
    def set_use_line_search(self, x): self._use_line_search = bool(x)


class quasi_newton_solver(line_search_solver):
    """src/nonlin_solve.f90:43-58."""

    def __init__(self):
        super().__init__()
        self._jdelta = 5                                      # m_jDelta, :51

    def get_jacobian_interval(self): return self._jdelta      # :429-436
    def set_jacobian_interval(self, n): self._jdelta = int(n)  # :439-447

    def solve(self, fcn, x, fvec, ib=None, args=None):
        """qns_solve (:156-427)."""
        _check_xf(fcn, x, fvec)
        if self.get_use_line_search() and not self.is_line_search_defined():
            self.set_default_line_search()        # :233-237
        if not fcn.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)   # :240
        m, n = fcn.get_equation_count(), fcn.get_variable_count()
        if n != m:
            raise NonlinError(NL_INVALID_INPUT_ERROR)        # :241
        if x.shape != (n,):
            raise NonlinError(3)
        if fvec.shape != (m,):
            raise NonlinError(4)
        o = self._options()
        o.use_line_search = 1 if self._use_line_search else 0
        if self._line_search is not None:
            o.ls_max_evals = self._line_search._max_eval
            o.ls_alpha = self._line_search._alpha
            o.ls_factor = self._line_search._factor
        h = self._handle()
        cib = _lib.IterationBehavior()
        cf, cj = fcn._c_fcn(args), fcn._c_jac(args)
        rc = h.lib.nlh_quasi_newton_solve(h.ptr, C.byref(o), self._jdelta, n, cf, cj, None, _dp(x), _dp(fvec),
                                          C.byref(cib))
        h.check(rc, "nlh_quasi_newton_solve")
        if ib is not None:
            ib._fill(cib)
        if rc:
            raise NonlinError(rc)


class newton_solver(line_search_solver):
    """src/nonlin_solve.f90:60-67."""

    def solve(self, fcn, x, fvec, ib=None, args=None):
        """ns_solve (:452-638)."""
        _check_xf(fcn, x, fvec)
        if self.get_use_line_search() and not self.is_line_search_defined():
            self.set_default_line_search()        # :511-515
        if not fcn.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)   # :518
        m, n = fcn.get_equation_count(), fcn.get_variable_count()
        if n != m:
            raise NonlinError(NL_INVALID_INPUT_ERROR)        # :519
        if x.shape != (n,):
            raise NonlinError(3)
        if fvec.shape != (m,):
            raise NonlinError(4)
        o = self._options()
        o.use_line_search = 1 if self._use_line_search else 0
        if self._line_search is not None:
            o.ls_max_evals = self._line_search._max_eval
            o.ls_alpha = self._line_search._alpha
            o.ls_factor = self._line_search._factor
        h = self._handle()
        cib = _lib.IterationBehavior()
        cf, cj = fcn._c_fcn(args), fcn._c_jac(args)
        rc = h.lib.nlh_newton_solve(h.ptr, C.byref(o), n, cf, cj, None, _dp(x), _dp(fvec), C.byref(cib))
        h.check(rc, "nlh_newton_solve")
        if ib is not None:
            ib._fill(cib)
        if rc:
            raise NonlinError(rc)


class polynomial:
    """src/nonlin_polynomials.f90:39-72: initialize, order, fit, fit_thru_zero, evaluate (real and complex), companion_mtx,
    roots, get, get_all, set, assignment (copy / assign), + - *, divide.  Coefficients are c(1) + c(2) x + ... as in the
    reference (get / set are 1-based).  fit and roots run on the device; the arithmetic is host code that follows the
    reference statement by statement, including where it is odd: for x of HIGHER order than y, x + y and x - y leave the
    leading coefficient of the result 0 (:538, :593), and x - y with x uninitialised returns +y (:576-580).
    roots() returns complex128 in the order LAPACK's DGEEV has them (a complex pair as (re, +im), (re, -im); the exact
    zero roots of zero low coefficients last)."""

    def __init__(self, order=None):
        self._c = None
        if order is not None:
            self.initialize(order)

    def initialize(self, order_or_coeffs):                    # :69-109
        if np.ndim(order_or_coeffs) == 0:
            if order_or_coeffs < 0:
                raise NonlinError(2)
            self._c = np.zeros(int(order_or_coeffs) + 1)
        else:
            self._c = np.array(order_or_coeffs, dtype=np.float64).ravel().copy()

    def order(self):                                          # :112-143
        return -1 if self._c is None else self._c.size - 1

    def _fit(self, x, y, order, thru_zero):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.size != x.size:
            raise NonlinError(3)                              # :159-162
        if order >= x.size or order < 1:
            raise NonlinError(4)                              # :163-166
        if self.order() != order:
            self.initialize(order)
        h = default_handle()
        rc = h.lib.nlh_poly_fit(h.ptr, x.size, int(order), int(thru_zero), _dp(x), _dp(y), _dp(self._c))
        h.check(rc, "nlh_poly_fit")
        if rc:
            raise NonlinError(rc)

    def fit(self, x, y, order): self._fit(x, y, order, False)                 # :146-190
    def fit_thru_zero(self, x, y, order): self._fit(x, y, order, True)        # :193-238

    def evaluate(self, x):                                    # :241-321, Horner from the top
        if np.iscomplexobj(x):
            return self._evaluate_complex(np.asarray(x, dtype=np.complex128))
        x = np.asarray(x, dtype=np.float64)
        order = self.order()
        if order == -1:
            return np.zeros_like(x)
        if order == 0:
            return np.full_like(x, self._c[0])
        y = self._c[order] * x + self._c[order - 1]
        for j in range(order - 2, -1, -1):
            y = y * x + self._c[j]
        return y

    def _evaluate_complex(self, x):                           # :290-321: y x as (yr xr - yi xi, yr xi + yi xr), c to the real part
        order = self.order()
        if order == -1:
            return np.zeros_like(x)
        if order == 0:
            return np.full_like(x, self._c[0])
        xr, xi = x.real, x.imag
        yr = self._c[order] * xr + self._c[order - 1]
        yi = self._c[order] * xi
        for j in range(order - 2, -1, -1):
            tr = yr * xr - yi * xi
            ti = yr * xi + yi * xr
            yr = tr + self._c[j]
            yi = ti
        y = np.empty(x.shape, dtype=np.complex128)
        y.real = yr
        y.imag = yi
        return y

    def companion_mtx(self):                                  # :324-354
        n = self.order()
        if n == -1:
            return np.zeros((0, 0))
        c = np.zeros((n, n))
        for i in range(n):
            c[i, n - 1] = -self._c[i] / self._c[n]
            if i < n - 1:
                c[i + 1, i] = 1.0
        return c

    def roots(self):                                          # :357-381
        n = self.order()
        if n <= 0:
            return np.zeros(0, dtype=np.complex128)           # :373
        z = np.empty(n, dtype=np.complex128)
        info = C.c_int32(0)
        h = default_handle()
        coef = np.ascontiguousarray(self._c, dtype=np.float64)
        rc = h.lib.nlh_poly_roots(h.ptr, n, _dp(coef), z.ctypes.data_as(_lib.c_double_p), C.byref(info))
        h.check(rc, "nlh_poly_roots")
        if rc:
            raise NonlinError(rc)
        if info.value:
            raise NonlinError(info.value)
        return z

    def get(self, i): return float(self._c[i - 1])            # 1-based like the reference
    def get_all(self): return self._c.copy()
    def set(self, i, v): self._c[i - 1] = float(v)

    # ---- assignment(=), :454-498 -------------------------------------------------------------------------------
    def copy(self):                                           # poly_equals
        z = polynomial()
        if self._c is not None:
            z._c = self._c.copy()
        return z

    def assign(self, y):
        """x = y for y a polynomial (:454-470), a number (every coefficient, :473-488) or an array (:491-498)."""
        if isinstance(y, polynomial):
            self._c = None if y._c is None else y._c.copy()
        elif np.ndim(y) == 0:
            if self._c is not None:
                self._c[:] = float(y)
        else:
            self.initialize(y)
        return self

    # ---- operators, :501-678 -----------------------------------------------------------------------------------
    @staticmethod
    def _of(c):
        z = polynomial()
        z._c = c
        return z

    def _add_sub(self, y, sub):                               # poly_poly_add :501-553, poly_poly_subtract :556-608
        x_ord, y_ord = self.order(), y.order()
        max_ord = max(x_ord, y_ord)
        if x_ord == -1 and y_ord == -1:
            return polynomial()
        z = np.zeros(max_ord + 1)
        if x_ord == -1:
            z[:] = y._c                                       # :523, and :578 for subtract: +y
        elif y_ord == -1:
            z[:] = self._c
        elif x_ord > y_ord:
            lo = self._c[:y_ord + 1]
            z[:y_ord + 1] = lo - y._c if sub else lo + y._c
            z[y_ord + 1:x_ord] = self._c[y_ord + 1:x_ord]     # :538 / :593: do i = y_ord + 2, x_ord -- z(x_ord + 1) stays 0
        elif x_ord < y_ord:
            lo = y._c[:x_ord + 1]
            z[:x_ord + 1] = self._c - lo if sub else self._c + lo
            z[x_ord + 1:] = -y._c[x_ord + 1:] if sub else y._c[x_ord + 1:]
        else:
            z[:] = self._c - y._c if sub else self._c + y._c
        return polynomial._of(z)

    def __add__(self, y):
        return self._add_sub(y, False) if isinstance(y, polynomial) else NotImplemented

    def __sub__(self, y):
        return self._add_sub(y, True) if isinstance(y, polynomial) else NotImplemented

    def __mul__(self, y):
        if isinstance(y, polynomial):                         # poly_poly_mult :611-636
            n, m = self.order() + 1, y.order() + 1
            if n + m - 2 < 0:
                raise NonlinError(2)                          # initialize(order < 0)
            z = np.zeros(n + m - 1)
            for i in range(n):
                for j in range(m):
                    z[i + j] = z[i + j] + self._c[i] * y._c[j]
            return polynomial._of(z)
        if np.ndim(y) == 0 and not isinstance(y, complex):    # poly_dbl_mult :639-657
            if self._c is None:
                raise NonlinError(2)
            return polynomial._of(self._c * float(y))
        return NotImplemented

    def __rmul__(self, x):                                    # dbl_poly_mult :660-678
        return self.__mul__(x)

    def divide(self, divisor):                                # poly_divide :681-779
        """(quotient, remainder) of self / divisor."""
        if self.order() == -1:
            raise NonlinError(1)                              # :710
        if divisor.order() == -1:
            raise NonlinError(2)                              # :711
        num, den = self._c, divisor._c
        eps = np.finfo(np.float64).eps
        lead = den[-1]
        if abs(lead) <= eps:
            raise NonlinError(NL_DIVIDE_BY_ZERO_ERROR)        # :717
        n, m = num.size - 1, den.size - 1
        if n < m:
            return polynomial(0), polynomial._of(num.copy())  # :722-728
        q = np.zeros(n - m + 1)
        r = num.copy()
        for i in range(n - m, -1, -1):
            coeff = r[i + m] / lead
            q[i] = coeff
            for j in range(m + 1):
                r[i + j] = r[i + j] - coeff * den[j]

        def trim(v):                                          # :744-778
            nz = np.nonzero(np.abs(v) > eps)[0]
            return polynomial(0) if nz.size == 0 else polynomial._of(v[:nz[-1] + 1].copy())
        return trim(q), trim(r)


class fcnnvar_helper:
    """src/nonlin_multi_var.f90:29-43: holder of a scalar objective fcn(x, args) -> float and an optional
    gradient routine grad(x, g, args)."""

    def __init__(self):
        self._fcn = None
        self._grad = None
        self._nvar = 0

    def set_fcn(self, fcn, nvar):                             # :99-106
        self._fcn = fcn
        self._nvar = int(nvar)

    def set_gradient_fcn(self, grad): self._grad = grad       # :116-120
    def is_fcn_defined(self): return self._fcn is not None
    def is_gradient_defined(self): return self._grad is not None
    def get_variable_count(self): return self._nvar

    def fcn(self, x, args=None):                              # :81-89
        return float(self._fcn(x, args)) if self._fcn is not None else 0.0

    def _c_fcn(self, args):
        f = self._fcn

        def _cb(ctx, n, xp):
            return float(f(np.ctypeslib.as_array(xp, shape=(n,)), args))
        return _lib.FCNNVAR(_cb)

    def _c_grad(self, args):
        if self._grad is None:
            return C.cast(None, _lib.GRADFCN)
        g = self._grad

        def _cb(ctx, n, xp, gp):
            g(np.ctypeslib.as_array(xp, shape=(n,)), np.ctypeslib.as_array(gp, shape=(n,)), args)
        return _lib.GRADFCN(_cb)


class equation_optimizer:
    """src/nonlin_multi_var.f90:45-57."""

    def __init__(self):
        self._max_eval = 500                      # :46
        self._tol = 1.0e-12                       # :47
        self._print = False
        self.handle = None

    def get_max_fcn_evals(self): return self._max_eval
    def set_max_fcn_evals(self, n): self._max_eval = int(n)
    def get_tolerance(self): return self._tol
    def set_tolerance(self, x): self._tol = float(x)
    def get_print_status(self): return self._print
    def set_print_status(self, x): self._print = bool(x)


class line_search_optimizer(equation_optimizer):
    """src/nonlin_optimize.f90:44-61."""

    def __init__(self):
        super().__init__()
        self._line_search = None
        self._use_line_search = True              # :46
        self._xtol = 1.0e-12                      # :47

    def get_line_search(self):
        if self._line_search is None:
            return None
        ls = line_search()
        ls.__dict__.update(self._line_search.__dict__)
        return ls

    def set_line_search(self, ls):
        c = line_search()
        c.__dict__.update(ls.__dict__)
        self._line_search = c

    def set_default_line_search(self): self._line_search = line_search()
    def is_line_search_defined(self): return self._line_search is not None
    def get_use_line_search(self): return self._use_line_search
    def set_use_line_search(self, x): self._use_line_search = bool(x)
    def get_var_tolerance(self): return self._xtol
    def set_var_tolerance(self, x): self._xtol = float(x)


class bfgs(line_search_optimizer):
    """src/nonlin_optimize.f90:69-72."""

    def solve(self, fcn, x, ib=None, args=None):
        """bfgs_solve (:557-770).  x: initial estimate -> minimiser.  Returns fout."""
        if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
            raise ValueError("x must be a contiguous float64 numpy array (it is updated in place)")
        if self.get_use_line_search() and not self.is_line_search_defined():
            self.set_default_line_search()        # :604-608
        if not fcn.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)   # :614
        n = fcn.get_variable_count()
        if x.shape != (n,):
            raise NonlinError(NL_INVALID_INPUT_ERROR)        # :615
        o = _lib.default_options()
        o.max_evals = self._max_eval
        o.gtol = self._tol
        o.xtol = self._xtol
        o.print_status = 1 if self._print else 0
        o.use_line_search = 1 if self._use_line_search else 0
        if self._line_search is not None:
            o.ls_max_evals = self._line_search._max_eval
            o.ls_alpha = self._line_search._alpha
            o.ls_factor = self._line_search._factor
        h = self.handle or default_handle()
        cib = _lib.IterationBehavior()
        fout = C.c_double(0.0)
        cf, cg = fcn._c_fcn(args), fcn._c_grad(args)
        rc = h.lib.nlh_bfgs_solve(h.ptr, C.byref(o), n, cf, cg, None, _dp(x), C.cast(C.byref(fout), _lib.c_double_p),
                                  C.byref(cib))
        h.check(rc, "nlh_bfgs_solve")
        if ib is not None:
            ib._fill(cib)
        if rc:
            raise NonlinError(rc)                 # :765-767
        return fout.value


class nelder_mead(equation_optimizer):
    """src/nonlin_optimize.f90:24-41: the Nelder-Mead simplex method.  The simplex is object state: a second solve
    continues from the final simplex of the first (:180-203)."""

    def __init__(self):
        super().__init__()
        self._simplex = None                      # m_simplex (n x n+1, Fortran order), unallocated
        self._init_size = 1.0                     # m_initSize

    def get_simplex(self):                        # :402-418
        return None if self._simplex is None else self._simplex.copy()

    def set_simplex(self, x):                     # :421-437
        self._simplex = None if x is None else np.array(x, dtype=np.float64, order="F", copy=True)

    def get_initial_size(self): return self._init_size          # :440-451
    def set_initial_size(self, x): self._init_size = float(x)   # :454-466

    def solve(self, fcn, x, ib=None, args=None):
        """nm_solve (:104-340).  x: initial estimate -> minimiser (in place; untouched when max evaluations stop the
        solve).  Returns fout.  NonlinError(106) is raised after ib and the object's simplex are stored."""
        if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous):
            raise ValueError("x must be a contiguous float64 numpy array (it is updated in place)")
        if ib is not None:
            ib._fill(_lib.IterationBehavior())    # :159-167
        if not fcn.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)   # :170
        n = fcn.get_variable_count()
        if x.shape != (n,):
            raise NonlinError(NL_INVALID_INPUT_ERROR)        # :171
        o = _lib.default_options()
        o.max_evals = self._max_eval
        o.gtol = self._tol
        o.print_status = 1 if self._print else 0
        h = self.handle or default_handle()
        use = self._simplex is not None and self._simplex.shape == (n, n + 1)      # :176-188
        # vertex-major [n+1][n] == the Fortran n x (n+1) matrix in column-major order
        sim = np.ascontiguousarray(self._simplex.T) if use else np.zeros((n + 1, n))
        cib = _lib.IterationBehavior()
        fout = C.c_double(0.0)
        rc = h.lib.nlh_nelder_mead_solve(h.ptr, C.byref(o), self._init_size, n, fcn._c_fcn(args), None, _dp(x), _dp(sim),
                                         1 if use else 0, C.cast(C.byref(fout), _lib.c_double_p), C.byref(cib))
        h.check(rc, "nlh_nelder_mead_solve")
        self._simplex = np.asfortranarray(sim.T)
        if ib is not None:
            ib._fill(cib)
        if rc:
            raise NonlinError(rc)                 # :335-337
        return fout.value


# ---------------------------------------------------------------------------------------------- equations of one variable
class value_pair:
    """src/nonlin_types.f90:31-36: a pair of values (the search limits of the one-variable solvers)."""

    def __init__(self, x1=0.0, x2=0.0):
        self.x1 = float(x1)
        self.x2 = float(x2)


class fcn1var_helper:
    """src/nonlin_single_var.f90:25-43: holder of an equation of one variable fcn(x, args) -> float and, optionally, its
    derivative diff(x, args) -> float."""

    def __init__(self):
        self._fcn = None
        self._diff = None

    def set_fcn(self, fcn): self._fcn = fcn                   # :132-141
    def set_diff(self, diff): self._diff = diff               # :203-212
    def is_fcn_defined(self): return self._fcn is not None    # :121-129
    def is_derivative_defined(self): return self._diff is not None   # :143-152

    def fcn(self, x, args=None):                              # :103-118 (silently 0 if unset)
        return float(self._fcn(float(x), args)) if self._fcn is not None else 0.0

    def diff(self, x, f=None, args=None):
        """f1h_diff_fcn (:154-200): the user's derivative, or a forward difference (h = sqrt(eps)|x|, divided by h).  Runs
        on the host through nlh_fd_derivative; needs no GPU."""
        if f is not None:
            fv = C.c_double(float(f))
            fvp = C.cast(C.byref(fv), _lib.c_double_p)
        else:
            fvp = None
        df = C.c_double(0.0)
        rc = _lib.load().nlh_fd_derivative(self._c_fcn(args), self._c_diff(args), None, float(x), fvp,
                                           C.cast(C.byref(df), _lib.c_double_p))
        if rc:
            raise NonlinError(rc)
        return df.value

    def _c_fcn(self, args):
        f = self._fcn
        if f is None:
            return C.cast(None, _lib.FCNNVAR)
        return _lib.FCNNVAR(lambda ctx, n, xp: float(f(xp[0], args)))

    def _c_diff(self, args):
        d = self._diff
        if d is None:
            return C.cast(None, _lib.FCNNVAR)
        return _lib.FCNNVAR(lambda ctx, n, xp: float(d(xp[0], args)))


class equation_solver_1var:
    """src/nonlin_single_var.f90:45-69; defaults :47-54."""

    def __init__(self):
        self._max_eval = 100
        self._fcn_tol = 1.0e-8
        self._xtol = 1.0e-12
        self._difftol = 1.0e-12
        self._print = False
        self.handle = None

    def get_max_fcn_evals(self): return self._max_eval
    def set_max_fcn_evals(self, n): self._max_eval = int(n)
    def get_fcn_tolerance(self): return self._fcn_tol
    def set_fcn_tolerance(self, x): self._fcn_tol = float(x)
    def get_var_tolerance(self): return self._xtol
    def set_var_tolerance(self, x): self._xtol = float(x)
    def get_diff_tolerance(self): return self._difftol
    def set_diff_tolerance(self, x): self._difftol = float(x)
    def get_print_status(self): return self._print
    def set_print_status(self, x): self._print = bool(x)

    def _options(self):
        o = _lib.default_options()
        o.max_evals = self._max_eval
        o.ftol = self._fcn_tol
        o.xtol = self._xtol
        o.gtol = self._difftol
        o.print_status = 1 if self._print else 0
        return o

    def _solve(self, entry, fcn, lim, ib, args, with_diff):
        """The reference's solve with f present.  Returns (x, f); NonlinError after ib is filled."""
        if ib is not None:
            ib._fill(_lib.IterationBehavior())
        if not fcn.is_fcn_defined():
            raise NonlinError(NL_UNDEFINED_FUNCTION_ERROR)
        x1, x2 = (lim.x1, lim.x2) if isinstance(lim, value_pair) else (float(lim[0]), float(lim[1]))
        h = self.handle or default_handle()
        o = self._options()
        x, f = C.c_double(0.0), C.c_double(0.0)
        cib = _lib.IterationBehavior()
        cargs = [fcn._c_fcn(args)] + ([fcn._c_diff(args)] if with_diff else [])
        rc = getattr(h.lib, entry)(h.ptr, C.byref(o), *cargs, None, float(x1), float(x2), C.cast(C.byref(x), _lib.c_double_p),
                                   C.cast(C.byref(f), _lib.c_double_p), C.byref(cib))
        h.check(rc, entry)
        if ib is not None:
            ib._fill(cib)
        if rc:
            raise NonlinError(rc)
        return x.value, f.value


class brent_solver(equation_solver_1var):
    """src/nonlin_solve.f90:69-76: Brent's method."""

    def solve(self, fcn, lim, ib=None, args=None):
        """brent_solve (:643-835).  lim: value_pair (or a pair).  Returns (x, f)."""
        return self._solve("nlh_brent_solve", fcn, lim, ib, args, False)


class newton_1var_solver(equation_solver_1var):
    """src/nonlin_solve.f90:78-86: Newton's method for one variable, bracketed (bisection when a step leaves the bracket)."""

    def solve(self, fcn, lim, ib=None, args=None):
        """newt1var_solve (:840-1032) with f present (one more evaluation after the loop, its value discarded).  Returns
        (x, f)."""
        return self._solve("nlh_newton_1var_solve", fcn, lim, ib, args, True)
