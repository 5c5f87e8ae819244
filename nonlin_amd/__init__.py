"""nonlin_amd -- MI355X (gfx950) implementation of nonlin's Jacobian-evaluate + linear-solve
inner loop (least_squares_solver / newton_solver / vecfcn_helper%jacobian) behind the C ABI of
include/nonlin_hip.h.  See DESIGN.md.  There is no CPU fallback."""
from ._lib import NonlinHipUnavailable, LIB_PATH  # noqa: F401
from ._lib import Starts, STARTS_MAX_N, STARTS_MAX_KEEP, STARTS_MAX_CAND  # noqa: F401  (the box scan: starting values)
from ._lib import PoissonBootstrap, BOOT_POIS_MAX_MEAN  # noqa: F401  (parametric count replicas for stat= fits)
from ._lib import bca_levels, BOOT_INTERVALS, BCA_DEGENERATE, BCA_NO_ACCEL, BCA_BAD_DENOM, BCA_NO_REPLICA  # noqa: F401  (studentised / BCa intervals)
from ._lib import Bootstrap, BOOT_RESIDUAL, BOOT_WILD, BOOT_PAIRS, BOOT_MAX_ROWS, BOOT_MAX_REP  # noqa: F401  (resampled-data intervals)
from ._lib import Binned, BinStruct, bin_rule, BIN_MAX_Q, BIN_MAX_ORDER  # noqa: F401  (bin-integrated fits)
from ._lib import (Profile, PROFILE_OK, PROFILE_OPEN, PROFILE_OPEN_AT_BOUND, PROFILE_ON_BOUND, PROFILE_MAXIT,  # noqa: F401
                   PROFILE_FIT_FAILED, PROFILE_NO_START, PROFILE_NOT_FREE, PROFILE_LOWER, PROFILE_FLAGS)  # (profile-likelihood intervals)
from .api import (  # noqa: F401
    NonlinError, iteration_behavior, vecfcn_helper, equation_solver, least_squares_solver,
    line_search, line_search_solver, newton_solver, quasi_newton_solver,
    constrained_equation_solver, constrained_least_squares_solver, polynomial,
    fcnnvar_helper, equation_optimizer, line_search_optimizer, bfgs, nelder_mead,
    value_pair, fcn1var_helper, equation_solver_1var, brent_solver, newton_1var_solver,
    CURVE_GAUSS, CURVE_LORENTZ, CURVE_EXPDECAY, CURVE_KINDS, curve_nparams,
    Expr, EXPR_OPS, EXPR_SPECIAL_OPS, EXPR_EXTENDED_OPS, EXPR_DEF_OPS, EXPR_SPECIAL2_OPS, wofz,
    ParamMap, PMAP_FREE, PMAP_FIXED, PMAP_TIED,
    Loss, LOSS_LINEAR, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY, LOSS_KINDS,
    Poisson,
    Convolve, CONV_ZERO, CONV_HOLD,
    Group,
    Separable,
    GUESS_FALLBACK, GUESS_RANKDEF, GUESS_NONE, GUESS_MAX_M,
    NL_NO_ERROR, NL_INVALID_INPUT_ERROR, NL_ARRAY_SIZE_ERROR, NL_OUT_OF_MEMORY_ERROR,
    NL_INVALID_OPERATION_ERROR, NL_CONVERGENCE_ERROR, NL_DIVERGENT_BEHAVIOR_ERROR,
    NL_SPURIOUS_CONVERGENCE_ERROR, NL_TOLERANCE_TOO_SMALL_ERROR, NL_INDEX_OUT_OF_RANGE_ERROR,
    NL_DIVIDE_BY_ZERO_ERROR, NL_UNDEFINED_FUNCTION_ERROR, NL_UNDERDEFINED_PROBLEM_ERROR,
)

__all__ = [n for n in dir() if not n.startswith("_")]
