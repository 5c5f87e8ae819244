"""ctypes loader for libnonlin_hip.so (the C ABI declared in include/nonlin_hip.h).

The product path has no CPU fallback: if the shared library is missing, or no GPU is
visible when a compute entry point is called, this module raises.
"""
import ctypes as C
import math
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnonlin_hip.so")

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)

VECFCN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, c_double_p, C.c_int32, c_double_p)
JACFCN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, c_double_p, C.c_int32, c_double_p)
FCNNVAR = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_int32, c_double_p)
GRADFCN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, c_double_p, c_double_p)
# nlh_device_vecfcn / nlh_device_jacfcn: launchers (ctx, hip_stream, npoints, dprob, n, dX, m, dF | dJ) -> int
DEVFCN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p)


class IterationBehavior(C.Structure):
    """nlh_iteration_behavior == iteration_behavior (src/nonlin_types.f90:8-29)."""
    _fields_ = [(k, C.c_int32) for k in (
        "iter_count", "fcn_count", "jacobian_count", "gradient_count",
        "converge_on_fcn", "converge_on_chng", "converge_on_zero_diff")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class DqDeviceCtx(C.Structure):
    """nlh_dq_device_ctx: the dense-quadratic family behind the launchers nlh_dq_device_fcn / nlh_dq_device_jac."""
    _fields_ = [("dA", C.c_void_p), ("db", C.c_void_p), ("gamma", C.c_double)]


class CurveCtx(C.Structure):
    """nlh_curve_ctx: a built-in curve model behind the launchers nlh_curve_device_fcn / nlh_curve_device_jac."""
    _fields_ = [("kind", C.c_int32), ("ncomp", C.c_int32), ("nbase", C.c_int32), ("shared_t", C.c_int32), ("m", C.c_int32),
                ("dt", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p)]


class ExprCtx(C.Structure):
    """nlh_expr_ctx: a formula model behind the launchers nlh_expr_device_fcn / nlh_expr_device_jac."""
    _fields_ = [("e", C.c_void_p), ("shared_t", C.c_int32), ("m", C.c_int32), ("dt", C.c_void_p), ("dy", C.c_void_p), ("dw", C.c_void_p),
                ("dt_stride", C.c_int64)]


class Options(C.Structure):
    """nlh_options."""
    _fields_ = [("max_evals", C.c_int32), ("ftol", C.c_double), ("xtol", C.c_double),
                ("gtol", C.c_double), ("print_status", C.c_int32), ("factor", C.c_double),
                ("use_line_search", C.c_int32), ("ls_max_evals", C.c_int32),
                ("ls_alpha", C.c_double), ("ls_factor", C.c_double),
                ("factor_policy", C.c_int32), ("ne_pivot_tol", C.c_double), ("fuse_fd", C.c_int32),
                ("sub_batches", C.c_int32)]


class QrxPlanHead(C.Structure):
    """nlh_qrx_plan_head."""
    _fields_ = [(k, C.c_int32) for k in ("sweep", "init", "use_list", "ny", "nact")]


class QrxPlanStep(C.Structure):
    """nlh_qrx_plan_step."""
    _fields_ = [(k, C.c_int32) for k in ("j", "cur", "np", "lo", "flush", "pf", "pivot", "pass", "gwin", "lds", "lds_max",
                                             "tcur", "oop")]


_H = C.c_void_p
# a launcher that is a symbol of the library: DEVFCN's signature, (ctx, hip_stream, npoints, dprob, n, dX, m, dF | dJ) -> int
_LAUNCHER = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p])
# nlh_*_destroy and nlh_*_unwrap: what gives a pointer of the library's back to it
_RELEASE = (None, [C.c_void_p])

# The argument list of a one-call fit nlh_{curve,expr}_fit_batch{variant}{,_h} after the handle, as "name:type" -- the model,
# the data, what the variant adds, the outputs.  The ctypes signatures below come from it, and so do the argument values of
# DeviceSolver's fit path.  Types: i int32, d double, p void*, O nlh_options*, D double* (host), B nlh_iteration_behavior*,
# S int32* (host); A and I are arrays of doubles and of int32 on the device (void*) or, in the _h form, on the host.
FIT_MODEL = {"curve": "kind:i ncomp:i nbase:i", "expr": "expr:p"}
FIT_DATA = "nprob:i m:i t:A shared_t:i y:A w:A analytic:i xl:D xu:D"
FIT_VARIANT = {"": "",
               "_pmap": "pm:p",
               "_loss": "pm:p loss:i scale:A shared_scale:i",
               "_pois": "pm:p mu_floor:d",
               "_group": "g:p loss:i scale:A shared_scale:i stat:i mu_floor:d",
               "_conv": "g:p pm:p cv:p loss:i scale:A shared_scale:i stat:i mu_floor:d",
               "_sep": "g:p cv:p sp:p"}
FIT_OUTPUTS = "x:A fvec:A sigma:A cov:A chi2:A rank:I ib:B status:S"


def fit_args(model, variant):
    """[(name, type)] of the arguments of nlh_<model>_fit_batch<variant> after the handle."""
    spec = " ".join(("opts:O", FIT_MODEL[model], FIT_DATA, FIT_VARIANT[variant], FIT_OUTPUTS))
    return [tuple(a.split(":")) for a in spec.split()]


def _fit_signature(model, variant, host):
    types = {"i": C.c_int32, "d": C.c_double, "p": C.c_void_p, "O": C.POINTER(Options), "D": c_double_p,
             "B": C.POINTER(IterationBehavior), "S": c_int32_p,
             "A": c_double_p if host else C.c_void_p, "I": c_int32_p if host else C.c_void_p}
    return (C.c_int, [_H] + [types[t] for _, t in fit_args(model, variant)])


# every symbol include/nonlin_hip.h declares: name -> (restype, argtypes); the 28 one-call fits are added below the table
SYMBOLS = {
    "nlh_default_options": (None, [C.POINTER(Options)]),
    "nlh_format_status": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_char_p, C.c_int32]),
    "nlh_create": (C.c_int, [C.POINTER(_H), C.c_int32, C.c_void_p]),
    "nlh_destroy": _RELEASE,
    "nlh_device_count": (C.c_int, []),
    "nlh_last_error": (C.c_char_p, [_H]),
    "nlh_version": (C.c_char_p, []),
    "nlh_fd_jacobian": (C.c_int, [_H, C.c_int32, C.c_int32, VECFCN, JACFCN, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "nlh_lm_solve": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, VECFCN, JACFCN, C.c_void_p,
                               c_double_p, c_double_p, C.POINTER(IterationBehavior)]),
    "nlh_newton_solve": (C.c_int, [_H, C.POINTER(Options), C.c_int32, VECFCN, JACFCN, C.c_void_p,
                                   c_double_p, c_double_p, C.POINTER(IterationBehavior)]),
    "nlh_quasi_newton_solve": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, VECFCN, JACFCN, C.c_void_p,
                                         c_double_p, c_double_p, C.POINTER(IterationBehavior)]),
    "nlh_cls_solve": (C.c_int, [_H, C.POINTER(Options), C.c_double, C.c_double, c_double_p, c_double_p, C.c_int32, C.c_int32,
                                VECFCN, JACFCN, C.c_void_p, c_double_p, c_double_p, C.POINTER(IterationBehavior)]),
    "nlh_fd_gradient": (C.c_int, [C.c_int32, FCNNVAR, GRADFCN, C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "nlh_bfgs_solve": (C.c_int, [_H, C.POINTER(Options), C.c_int32, FCNNVAR, GRADFCN, C.c_void_p, c_double_p, c_double_p,
                                 C.POINTER(IterationBehavior)]),
    "nlh_dq_lm_solve_batch": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                        C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_newton_solve_batch": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_quasi_newton_solve_batch": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                  C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_cls_solve_batch": (C.c_int, [_H, C.POINTER(Options), C.c_double, C.c_double, c_double_p, c_double_p, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                         C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_bfgs_solve_batch": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_double, C.c_void_p, c_double_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_generate": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.c_double, C.c_double,
                                  C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_dq_residual": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                  C.c_void_p, C.c_void_p]),
    "nlh_dq_fd_panel": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double,
                                  C.c_void_p, C.c_void_p]),
    "nlh_fd_jacobian_panel": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "nlh_dq_jacobian": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_void_p,
                                  C.c_void_p]),
    "nlh_gram": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_gram_plan": (C.c_int32, [C.c_int32, C.c_int32, c_int32_p, c_int32_p]),
    "nlh_chol_factor": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "nlh_chol_natural": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_ne_signs": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "nlh_qr_factor": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_lmfactor_exact": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_qrx_second_matrix_bytes": (C.c_int64, [_H]),
    "nlh_qrx_plan": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(QrxPlanHead),
                                 C.POINTER(QrxPlanStep), C.c_int32]),
    "nlh_lmpar": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_lu_factor": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_lu_solve": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_qr_factor_full": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_qr_rank1_update": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_solve_upper": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_house_steps": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_house_plan": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p]),
    "nlh_chol_rank1": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, c_int32_p]),
    "nlh_bf_chol_factor": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, c_int32_p]),
    "nlh_bf_solve_cholesky": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_bf_chol_form": (C.c_int32, [C.c_int32]),
    "nlh_poly_fit": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, c_double_p]),
    "nlh_poly_fit_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_poly_roots": (C.c_int, [_H, C.c_int32, c_double_p, c_double_p, C.POINTER(C.c_int32)]),
    "nlh_poly_roots_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_poly_eval_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_poly_eval_complex_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_dq_model_create": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, C.c_double, C.POINTER(C.c_void_p)]),
    "nlh_device_set_create": (C.c_int, [C.POINTER(C.c_void_p), c_int32_p, C.c_int32]),
    "nlh_device_set_destroy": _RELEASE,
    "nlh_device_set_size": (C.c_int32, [C.c_void_p]),
    "nlh_device_set_handle": (C.c_void_p, [C.c_void_p, C.c_int32]),
    "nlh_device_set_last_error": (C.c_char_p, [C.c_void_p]),
    "nlh_dq_model_create_on": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p, C.c_double,
                                         C.POINTER(C.c_void_p)]),
    "nlh_dq_model_device_count": (C.c_int32, [C.c_void_p]),
    "nlh_dq_model_destroy": _RELEASE,
    "nlh_dq_model_shape": (None, [C.c_void_p, c_int32_p, c_int32_p, c_int32_p]),
    "nlh_dq_model_eval": (C.c_int, [_H, C.c_void_p, c_double_p, c_double_p]),
    "nlh_dq_model_lm_solve": (C.c_int, [_H, C.POINTER(Options), C.c_void_p, c_double_p, c_double_p,
                                        C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_model_newton_solve": (C.c_int, [_H, C.POINTER(Options), C.c_void_p, C.c_int32, c_double_p, c_double_p,
                                            C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_model_quasi_newton_solve": (C.c_int, [_H, C.POINTER(Options), C.c_void_p, C.c_int32, C.c_int32, c_double_p, c_double_p,
                                                  C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_model_cls_solve": (C.c_int, [_H, C.POINTER(Options), C.c_void_p, C.c_double, C.c_double, c_double_p, c_double_p,
                                         c_double_p, c_double_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_model_bfgs_solve": (C.c_int, [_H, C.POINTER(Options), C.c_void_p, c_double_p, c_double_p, c_double_p,
                                          C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_fd_jacobian_device": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "nlh_lm_solve_batch_device": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_newton_solve_batch_device": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_quasi_newton_solve_batch_device": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_cls_solve_batch_device": (C.c_int, [_H, C.POINTER(Options), C.c_double, C.c_double, c_double_p, c_double_p, C.c_int32, C.c_int32,
                                             C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_cls_solve_batch_device_h": (C.c_int, [_H, C.POINTER(Options), C.c_double, C.c_double, c_double_p, c_double_p, C.c_int32, C.c_int32,
                                               C.c_int32, DEVFCN, DEVFCN, C.c_void_p, c_double_p, c_double_p,
                                               C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_bfgs_solve_batch_device": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.c_void_p, c_double_p,
                                              C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_bfgs_solve_batch_device_h": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, c_double_p, c_double_p,
                                                C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_nelder_mead_solve": (C.c_int, [_H, C.POINTER(Options), C.c_double, C.c_int32, FCNNVAR, C.c_void_p, c_double_p, c_double_p,
                                        C.c_int32, c_double_p, C.POINTER(IterationBehavior)]),
    "nlh_nelder_mead_solve_batch_device": (C.c_int, [_H, C.POINTER(Options), C.c_double, C.c_int32, C.c_int32, DEVFCN, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_int32, c_double_p, C.POINTER(IterationBehavior),
                                                     c_int32_p]),
    "nlh_dq_model_nelder_mead_solve": (C.c_int, [_H, C.POINTER(Options), C.c_double, C.c_void_p, c_double_p, c_double_p,
                                                 C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_brent_solve": (C.c_int, [_H, C.POINTER(Options), FCNNVAR, C.c_void_p, C.c_double, C.c_double, c_double_p, c_double_p,
                                  C.POINTER(IterationBehavior)]),
    "nlh_newton_1var_solve": (C.c_int, [_H, C.POINTER(Options), FCNNVAR, FCNNVAR, C.c_void_p, C.c_double, C.c_double, c_double_p,
                                        c_double_p, C.POINTER(IterationBehavior)]),
    "nlh_brent_solve_batch_device": (C.c_int, [_H, C.POINTER(Options), C.c_int32, DEVFCN, C.c_void_p, C.c_void_p, C.c_void_p,
                                               c_double_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_newton_1var_solve_batch_device": (C.c_int, [_H, C.POINTER(Options), C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, c_double_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_model_brent_solve": (C.c_int, [_H, C.POINTER(Options), C.c_void_p, c_double_p, c_double_p, c_double_p,
                                           C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_dq_model_newton_1var_solve": (C.c_int, [_H, C.POINTER(Options), C.c_void_p, c_double_p, c_double_p, c_double_p,
                                                 C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_fd_derivative": (C.c_int, [FCNNVAR, FCNNVAR, C.c_void_p, C.c_double, c_double_p, c_double_p]),
    "nlh_lm_solve_batch_device_h": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p,
                                              c_double_p, c_double_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_newton_solve_batch_device_h": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p,
                                                  c_double_p, c_double_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_quasi_newton_solve_batch_device_h": (C.c_int, [_H, C.POINTER(Options), C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN,
                                                        C.c_void_p, c_double_p, c_double_p, C.POINTER(IterationBehavior), c_int32_p]),
    "nlh_device_fcn_model_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_dq_device_fcn": _LAUNCHER,
    "nlh_dq_device_jac": _LAUNCHER,
    "nlh_covar": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "nlh_covar_lds_bytes": (C.c_int64, [C.c_int32]),
    "nlh_lm_covariance_batch_device": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.c_void_p,
                                                 C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_lm_covariance_batch_device_h": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, c_double_p,
                                                   C.c_int32, C.c_double, c_double_p, c_double_p, c_int32_p, c_double_p]),
    "nlh_lm_covariance": (C.c_int, [_H, C.c_int32, C.c_int32, VECFCN, JACFCN, C.c_void_p, c_double_p, C.c_int32, C.c_double,
                                    c_double_p, c_double_p, c_int32_p, c_double_p]),
    "nlh_dq_model_lm_covariance": (C.c_int, [_H, C.c_void_p, c_double_p, C.c_int32, C.c_double, c_double_p, c_double_p, c_int32_p,
                                             c_double_p]),
    "nlh_curve_device_fcn": _LAUNCHER,
    "nlh_curve_device_jac": _LAUNCHER,
    "nlh_curve_nparams": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32]),
    "nlh_curve_model_create": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_double_p, C.c_int32, c_double_p,
                                         c_double_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "nlh_curve_eval_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p]),
    "nlh_expr_compile": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "nlh_expr_error": (C.c_char_p, []),
    "nlh_expr_destroy": _RELEASE,
    "nlh_expr_shape": (None, [C.c_void_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "nlh_expr_program": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, c_double_p]),
    "nlh_expr_masks": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "nlh_expr_roots": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p]),
    "nlh_faddeeva": (C.c_int, [C.c_double, C.c_double, c_double_p, c_double_p]),
    "nlh_faddeeva_table": (None, [c_double_p, c_double_p]),
    "nlh_faddeeva_batch": (C.c_int, [_H, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_expr_device_fcn": _LAUNCHER,
    "nlh_expr_device_jac": _LAUNCHER,
    "nlh_expr_plan": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p, c_int32_p, c_int32_p,
                                  C.POINTER(C.c_int64), c_int32_p, C.POINTER(C.c_int64)]),
    "nlh_expr_model_create": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, c_double_p, C.c_int32, c_double_p, c_double_p, C.c_int32,
                                        C.POINTER(C.c_void_p)]),
    "nlh_expr_eval_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_propagate": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_propagate_batch_device": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_propagate_batch_device_h": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, c_double_p, c_double_p,
                                               c_double_p, c_double_p, c_double_p]),
    "nlh_curve_band_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_expr_band_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "nlh_dq_model_propagate": (C.c_int, [_H, C.c_void_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "nlh_pmap_create": (C.c_int, [C.c_int32, c_int32_p, c_int32_p, c_double_p, c_double_p, C.POINTER(C.c_void_p)]),
    "nlh_pmap_destroy": _RELEASE,
    "nlh_pmap_shape": (None, [C.c_void_p, c_int32_p, c_int32_p, c_int32_p]),
    "nlh_pmap_tables": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p, c_double_p, c_double_p, c_int32_p]),
    "nlh_pmap_wrap": (C.c_int, [_H, C.c_void_p, DEVFCN, DEVFCN, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "nlh_pmap_unwrap": _RELEASE,
    "nlh_pmap_device_fcn": _LAUNCHER,
    "nlh_pmap_device_jac": _LAUNCHER,
    "nlh_pmap_gather_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_pmap_expand_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "nlh_pmap_cov_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_pmap_model_create": (C.c_int, [_H, C.c_void_p, C.c_void_p, c_double_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "nlh_sep_model_create": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_sep_create": (C.c_int, [C.c_int32, C.c_int32, c_int32_p, C.POINTER(C.c_void_p)]),
    "nlh_sep_destroy": _RELEASE,
    "nlh_sep_shape": (None, [C.c_void_p, c_int32_p, c_int32_p, c_int32_p]),
    "nlh_sep_tables": (C.c_int, [C.c_void_p, c_int32_p, c_int32_p]),
    "nlh_sep_wrap": (C.c_int, [_H, C.c_void_p, DEVFCN, DEVFCN, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_sep_unwrap": _RELEASE,
    "nlh_sep_device_fcn": _LAUNCHER,
    "nlh_sep_device_jac": _LAUNCHER,
    "nlh_sep_gather_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_sep_solve_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_loss_wrap": (C.c_int, [_H, C.c_int32, C.c_void_p, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_loss_unwrap": _RELEASE,
    "nlh_loss_device_fcn": _LAUNCHER,
    "nlh_loss_device_jac": _LAUNCHER,
    "nlh_loss_apply_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "nlh_loss_model_create": (C.c_int, [_H, C.c_void_p, C.c_int32, c_double_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "nlh_pois_wrap": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_double, DEVFCN, DEVFCN, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_pois_unwrap": _RELEASE,
    "nlh_pois_device_fcn": _LAUNCHER,
    "nlh_pois_device_jac": _LAUNCHER,
    "nlh_pois_apply_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "nlh_pois_model_create": (C.c_int, [_H, C.c_void_p, c_double_p, c_double_p, C.c_double, C.POINTER(C.c_void_p)]),
    "nlh_conv_wrap": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, DEVFCN, DEVFCN, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_conv_unwrap": _RELEASE,
    "nlh_conv_device_fcn": _LAUNCHER,
    "nlh_conv_device_jac": _LAUNCHER,
    "nlh_conv_apply_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_group_create": (C.c_int, [C.c_int32, C.c_int32, c_int32_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "nlh_group_destroy": _RELEASE,
    "nlh_group_shape": (None, [C.c_void_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p]),
    "nlh_group_index": (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    "nlh_group_wrap": (C.c_int, [_H, C.c_void_p, DEVFCN, DEVFCN, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_group_unwrap": _RELEASE,
    "nlh_group_device_fcn": _LAUNCHER,
    "nlh_group_device_jac": _LAUNCHER,
    "nlh_group_gather_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_group_expand_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_group_sigma_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_conv_model_create": (C.c_int, [_H, C.c_void_p, C.c_void_p, c_double_p, c_double_p, C.POINTER(C.c_void_p)]),
    "nlh_group_model_create": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_timing_enable": (None, [_H, C.c_int32]),
    "nlh_timing_reset": (None, [_H]),
    "nlh_timing_get": (C.c_int, [_H, C.c_int32, c_double_p, C.POINTER(C.c_int64)]),
    "nlh_timing_samples": (C.c_int64, [_H, C.c_int32, C.POINTER(C.c_float), C.c_int64]),
    "nlh_kernel_name": (C.c_char_p, [C.c_int32]),
}
SYMBOLS.update({f"nlh_{model}_fit_batch{variant}{h}": _fit_signature(model, variant, bool(h))
                for model in FIT_MODEL for variant in FIT_VARIANT for h in ("", "_h")})

# The entry points of include/nonlin_hip_guess.h (the part of the ABI that nonlin_hip.h includes): SYMBOLS is the table of what
# nonlin_hip.h itself declares, and tests hold it to that header and to a recorded table.
GUESS_SYMBOLS = {
    "nlh_curve_guess_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_curve_guess_batch_h": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_double_p, C.c_int32, c_double_p,
                                          c_double_p, C.c_int32, c_double_p, c_int32_p]),
}

# The entry points of include/nonlin_hip_starts.h, the part of the ABI that holds the box scan: bound beside GUESS_SYMBOLS.
_STARTS_BOX = [c_double_p, c_double_p, c_int32_p]                      # xl, xu, logscale: host arrays [n]
STARTS_SYMBOLS = {
    "nlh_starts_candidates": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + _STARTS_BOX + [c_double_p]),
    "nlh_starts_search_batch_device": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, DEVFCN, C.c_void_p] + _STARTS_BOX +
                                       [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_starts_search_batch_device_h": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, DEVFCN, C.c_void_p] + _STARTS_BOX +
                                         [C.c_int32, C.c_int32, c_double_p, c_double_p, c_int32_p]),
    "nlh_starts_cost_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_starts_pick_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_starts_take_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# The entry points of include/nonlin_hip_boot.h, the part of the ABI that holds the bootstrap: bound beside STARTS_SYMBOLS.
BOOT_SYMBOLS = {
    "nlh_boot_draws": (C.c_int, [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_int32_p]),
    "nlh_boot_resample_batch": (C.c_int, [_H, C.c_int32, C.c_uint64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_boot_summary_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
}

# The entry points of include/nonlin_hip_bin.h, the part of the ABI that holds the bin-integrated fits: bound beside BOOT_SYMBOLS.
BIN_SYMBOLS = {
    "nlh_bin_rule": (C.c_int, [C.c_int32, c_double_p, c_double_p]),
    "nlh_bin_wrap": (C.c_int, [_H, C.c_void_p, C.c_void_p, C.c_void_p, DEVFCN, DEVFCN, C.c_void_p, C.POINTER(C.c_void_p)]),
    "nlh_bin_unwrap": _RELEASE,
    "nlh_bin_device_fcn": _LAUNCHER,
    "nlh_bin_device_jac": _LAUNCHER,
    "nlh_bin_apply_batch": (C.c_int, [_H, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
}

# The entry points of include/nonlin_hip_boot_pois.h, the part of the ABI that holds the Poisson bootstrap: bound beside BIN_SYMBOLS.
BOOT_POIS_SYMBOLS = {
    "nlh_boot_poisson_draws": (C.c_int, [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, c_double_p, c_double_p]),
    "nlh_boot_poisson_batch": (C.c_int, [_H, C.c_uint64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
}

# The entry points of include/nonlin_hip_boot_ci.h, the part of the ABI that holds the studentised and the BCa interval of the
# bootstrap: bound beside PROFILE_SYMBOLS.
BOOT_CI_SYMBOLS = {
    "nlh_boot_bca_levels": (C.c_int, [C.c_int32, C.c_int32, C.c_double, C.c_double, c_double_p, c_double_p, c_double_p, c_int32_p]),
    "nlh_boot_student_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_boot_jackknife_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "nlh_boot_accel_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_boot_bca_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}


class ProfileState(C.Structure):
    """nlh_profile_state (include/nonlin_hip_profile.h): the addresses of the device arrays of a profile's root finder."""
    _fields_ = [(k, C.c_void_p) for k in ("C0", "delta", "xhat", "width", "bound", "theta", "a", "ga", "b", "gb", "end",
                                          "phase", "flag", "last", "nexp", "nev", "nfail")]


# The entry points of include/nonlin_hip_profile.h, the part of the ABI that holds the profile-likelihood intervals -- the pin
# pair and the root finder --: bound beside BOOT_POIS_SYMBOLS.
PROFILE_SYMBOLS = {
    "nlh_pin_wrap": (C.c_int, [_H, C.c_int32, DEVFCN, DEVFCN, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_void_p)]),
    "nlh_pin_set": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nlh_pin_unwrap": _RELEASE,
    "nlh_pin_device_fcn": _LAUNCHER,
    "nlh_pin_device_jac": _LAUNCHER,
    "nlh_profile_start_batch_device": (C.c_int, [_H, DEVFCN, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_double, C.c_int32, c_double_p, c_double_p, C.POINTER(ProfileState)]),
    "nlh_profile_step_batch": (C.c_int, [_H, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ProfileState),
                                         C.c_double, C.c_double, C.c_int32, C.c_int32, c_int32_p]),
}

KERNEL_IDS = {
    "dq_residual": 0, "dq_panel": 1, "fd_jacobian": 2, "gram": 3, "gram_reduce": 4, "jtf": 5,
    "chol": 6, "lmpar": 7, "qr": 8, "update": 9, "lu": 10, "dq_jacobian": 11, "qrx_pass": 12, "qrx_pivot": 13,
    "polyroots": 14, "covar": 15,
}

_lib = None


class NonlinHipUnavailable(RuntimeError):
    pass


def load():
    """Load libnonlin_hip.so and bind every declared symbol.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NonlinHipUnavailable(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C nonlin_amd/csrc` (there is no CPU fallback)")
    # PyTorch ships its own HIP runtime.  Two runtimes in one process coexist only if torch's is loaded first (the other way
    # round torch.cuda reports no device, or this library does): import torch before the library whenever it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in (list(SYMBOLS.items()) + list(GUESS_SYMBOLS.items()) + list(STARTS_SYMBOLS.items()) + list(BOOT_SYMBOLS.items()) +
                              list(BIN_SYMBOLS.items()) + list(BOOT_POIS_SYMBOLS.items()) + list(PROFILE_SYMBOLS.items()) +
                              list(BOOT_CI_SYMBOLS.items())):
        fn = getattr(lib, name)       # AttributeError if the ABI and this table drift
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def default_options():
    o = Options()
    load().nlh_default_options(C.byref(o))
    return o


# kinds of the built-in curve models (include/nonlin_hip.h: NLH_CURVE_*), as constants and by name
CURVE_GAUSS, CURVE_LORENTZ, CURVE_EXPDECAY = 0, 1, 2
CURVE_KINDS = {"gauss": CURVE_GAUSS, "lorentz": CURVE_LORENTZ, "expdecay": CURVE_EXPDECAY}


def curve_kind(kind):
    """A curve kind as its NLH_CURVE_* value: one of the constants, or "gauss" / "lorentz" / "expdecay"."""
    if isinstance(kind, str):
        if kind not in CURVE_KINDS:
            raise ValueError(f"unknown curve kind {kind!r}: one of {sorted(CURVE_KINDS)}")
        return CURVE_KINDS[kind]
    return int(kind)


def curve_nparams(kind, ncomp=1, baseline=-1):
    """n of a curve model (nlh_curve_nparams: host code, needs no GPU); raises ValueError for a bad kind or counts."""
    n = load().nlh_curve_nparams(curve_kind(kind), int(ncomp), int(baseline))
    if n < 0:
        raise ValueError(f"no curve model of kind {kind!r} with {ncomp} components and baseline degree {baseline}")
    return n


# flags of a guessed problem (include/nonlin_hip.h: NLH_GUESS_*) and the most rows curve_guess takes
GUESS_FALLBACK, GUESS_RANKDEF, GUESS_NONE = 1, 2, 4
GUESS_MAX_M = 8192


# opcodes of a compiled formula (include/nonlin_hip.h: NLH_EXPR_*), in order
EXPR_OPS = ("CONST", "VAR", "PARAM", "NEG", "ADD", "SUB", "MUL", "DIV", "IPOW", "POWC", "EXP", "LOG", "SQRT", "SIN", "COS", "TANH",
            "ATAN", "ABS")
# ... and of the special functions, numbered on from len(EXPR_OPS) = 18 (NLH_EXPR_ERF ..)
EXPR_SPECIAL_OPS = ("ERF", "ERFC", "ERFCX", "VOIGT")
# ... and of the fitted exponent, the four-quadrant angle and the selections, numbered on from 22 (NLH_EXPR_POW ..)
EXPR_EXTENDED_OPS = ("POW", "ATAN2", "MIN", "MAX", "WHERE")
# ... and of a use of a definition, 27 (NLH_EXPR_LOAD)
EXPR_DEF_OPS = ("LOAD",)
# ... and of the Bessel functions, the log-gamma function and the two cancellation-free forms, numbered on from 28 (NLH_EXPR_J0 ..)
EXPR_SPECIAL2_OPS = ("J0", "J1", "I0E", "I1E", "LGAMMA", "EXPM1", "LOG1P")


def faddeeva_table():
    """(L, a): the constants of the library's Faddeeva function, a [40] highest power first (nlh_faddeeva_table)."""
    import numpy as np
    L, a = C.c_double(), np.zeros(40)
    load().nlh_faddeeva_table(C.byref(L), a.ctypes.data_as(c_double_p))
    return L.value, a


def wofz(z):
    """The Faddeeva function w(z) = exp(-z^2) erfc(-iz) of a complex number or array with Im z >= 0, on the host
    (nlh_faddeeva: needs no GPU; the bits of DeviceSolver.wofz_batch and of the formulas' voigt).  ValueError below the axis."""
    import numpy as np
    lib = load()
    zz = np.asarray(z, dtype=np.complex128)
    out = np.empty(zz.shape, dtype=np.complex128)
    wr, wi = C.c_double(), C.c_double()
    flat, oflat = zz.reshape(-1), out.reshape(-1)
    for k in range(flat.size):
        if lib.nlh_faddeeva(flat[k].real, flat[k].imag, C.byref(wr), C.byref(wi)):
            raise ValueError(f"wofz: Im z >= 0 is required, got {flat[k]!r}")
        oflat[k] = complex(wr.value, wi.value)
    return out if out.ndim else complex(out)


def _names(v):
    return ",".join(v) if isinstance(v, (tuple, list)) else str(v)


class Owner:
    """Owns one pointer of the library's, the attribute _slot names: close() gives it back through the library's function
    _free names, once; so does garbage collection."""
    _slot, _free = "ptr", None

    def close(self):
        p = getattr(self, self._slot, None)
        if p is not None and p.value:
            getattr(self.lib, self._free)(p)
            setattr(self, self._slot, C.c_void_p())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Expr(Owner):
    """A formula model (nlh_expr_compile: host code, needs no GPU): formula is an expression over the variables vars (1 .. 4
    names) and the parameters params (1 .. 32 names, in the order of x), e.g. Expr("a*exp(-k*t)+c", ("t",), ("a", "k", "c")).
    Operators + - * / ^ (a literal exponent), functions exp log sqrt sin cos tanh atan abs erf erfc erfcx of one argument
    and voigt(x, sigma, gamma) -- the unit-area Voigt profile, Gaussian sigma and Lorentzian half width gamma -- the constant
    pi.  pow(a, b) is a power whose exponent may be fitted (its Jacobian is finite at a = 0, where exp(b*log(a))'s is NaN;
    a < 0 with a fitted exponent is outside its domain), atan2(y, x) the four-quadrant angle, min(a, b) and max(a, b) the
    smaller and the larger (a hinge is max(t-t0, 0)), where(c, a, b) is a where c >= 0 and b elsewhere (an onset at t0:
    where(t-t0, ..., 0)); both branches are evaluated, and a NaN in the one not taken reaches neither the value nor the
    Jacobian.  j0 and j1 are the Bessel functions of the first kind, i0e(a) = exp(-|a|) I0(a) and i1e(a) = exp(-|a|) I1(a) the
    scaled modified ones (I0 itself overflows at 713), lgamma the logarithm of |Gamma| (its Jacobian is digamma, for a > 0),
    expm1(a) = exp(a) - 1 and log1p(a) = log(1 + a) without the cancellation at small a.  2*j1(u)/u is 0/0 at u = 0: write
    where(abs(u)-1e-4, 2*j1(u)/u, 1-u^2/8).  Function names and pi are reserved: no variable or parameter may carry one.

    Definitions, formula := (name '=' expr ';')* expr, name a value that is computed once (blanks and newlines are ignored):

        Expr("dx = x-x0; dy = y-y0; c = cos(th); s = sin(th);"
             "u = dx*c + dy*s;  v = dy*c - dx*s;"
             "b + a*exp(-(u^2/(2*sx^2) + v^2/(2*sy^2)))", "x,y", "a,x0,y0,sx,sy,th,b")

    A definition's name is not a variable, a parameter, a function, pi or an earlier definition; it may be used in every later
    statement, any number of times.  The last statement is the model value.  defs is the tuple of the definitions' names, in
    order.  Statement k leaves its value in slot k of the stack, where LOAD k reads it, so depth counts the definitions' slots
    (the frame, 16 at most) and a definition counts once toward the 256 instructions and 64 constants.  The value and every
    Jacobian column are, bit for bit, those of the formula with each definition substituted in parentheses.

    Raises ValueError with the compiler's message ("col 17: unknown name 'foo'").  close() frees it (so does garbage
    collection)."""
    _free = "nlh_expr_destroy"

    def __init__(self, formula, vars=("t",), params=()):
        self.lib = load()
        self.formula, self.vars, self.params = formula, _names(vars), _names(params)
        self.ptr = C.c_void_p()
        rc = self.lib.nlh_expr_compile(formula.encode(), self.vars.encode(), self.params.encode(), C.byref(self.ptr))
        if rc:
            self.ptr = C.c_void_p()
            raise ValueError(self.lib.nlh_expr_error().decode())
        s = [C.c_int32() for _ in range(5)]
        self.lib.nlh_expr_shape(self.ptr, *[C.byref(v) for v in s])
        self.nvar, self.nparams, self.ninstr, self.nconst, self.depth = (v.value for v in s)
        self.defs = tuple(st.split("=")[0].strip() for st in formula.split(";")[:-1])    # (it compiled: name '=' expr ';' each)
        if len(self.defs) != self._ndef():                            # the compiler's own count: the slot the model value ends in
            raise RuntimeError(f"Expr: {len(self.defs)} names read from the text, {self._ndef()} definitions in the program")

    def _ndef(self):
        """The definitions of the compiled program, from the program alone: every statement leaves one slot in use, so the
        stack ends ndef + 1 deep."""
        sp = 0
        for o in self.program()[0]:
            sp += 1 if o <= 2 or o == 27 else (-1 if 4 <= o <= 7 or 22 <= o <= 25 else (-2 if o in (21, 26) else 0))
        return sp - 1

    def program(self):
        """(op, arg, consts, mask): the postfix program as int32 arrays [ninstr], its constants [nconst] and per instruction
        the uint32 mask of the parameters its subtree names.  LOAD k (a use of definition k): arg = k, the mask of the
        instruction that produced the definition."""
        import numpy as np
        op, arg = np.zeros(self.ninstr, dtype=np.int32), np.zeros(self.ninstr, dtype=np.int32)
        consts, mask = np.zeros(self.nconst), np.zeros(self.ninstr, dtype=np.uint32)
        rc = self.lib.nlh_expr_program(self.ptr, op.ctypes.data_as(c_int32_p), arg.ctypes.data_as(c_int32_p), consts.ctypes.data_as(c_double_p))
        rc = rc or self.lib.nlh_expr_masks(self.ptr, mask.ctypes.data_as(C.POINTER(C.c_uint32)))
        if rc:
            raise RuntimeError(f"nlh_expr_program returned {rc}")
        return op, arg, consts, mask

    def roots(self):
        """(aroot, broot), int32 [ninstr]: the instruction that produced a binary instruction's lower operand or VOIGT's x, and
        the one that produced VOIGT's sigma (nlh_expr_roots).  WHERE has its condition c in aroot and its first branch a in
        broot; the second branch is the instruction before it.  LOAD k has the instruction that produced definition k in
        aroot."""
        import numpy as np
        a, b = np.zeros(self.ninstr, dtype=np.int32), np.zeros(self.ninstr, dtype=np.int32)
        if self.lib.nlh_expr_roots(self.ptr, a.ctypes.data_as(c_int32_p), b.ctypes.data_as(c_int32_p)):
            raise RuntimeError("nlh_expr_roots failed")
        return a, b


# kinds of a parameter of a map (include/nonlin_hip.h: NLH_PMAP_*)
PMAP_FREE, PMAP_FIXED, PMAP_TIED = 0, 1, 2


class ParamMap(Owner):
    """A parameter map (nlh_pmap_create: host code, needs no GPU): which of a model's nfull parameters are free, fixed at a
    per-problem value, or tied to another one by p_k = scale * p_src + offset.  fixed: the indices of the fixed parameters;
    tied: {k: (src, scale, offset)}.  E.g. ParamMap(7, fixed=(6,), tied={5: (2, 1.25, 0.0)}).  Raises ValueError for what the
    library refuses (an index out of range, a chain of ties, a tie with scale 0, no free parameter, ...).  Free unknown j
    is the j-th free parameter in ascending index.  close() frees it (so does garbage collection)."""
    _free = "nlh_pmap_destroy"

    def __init__(self, nfull, fixed=(), tied=None):
        import numpy as np
        self.lib = load()
        self.ptr = C.c_void_p()
        nfull = int(nfull)
        tied = dict(tied or {})
        fixed = [int(k) for k in fixed]
        if nfull < 1 or any(not 0 <= int(k) < nfull for k in list(fixed) + list(tied)) or set(fixed) & set(int(k) for k in tied):
            raise ValueError(f"ParamMap: bad nfull ({nfull}), an index outside 0 .. nfull - 1, or a parameter both fixed and tied")
        kind = np.zeros(nfull, dtype=np.int32)
        src = np.zeros(nfull, dtype=np.int32)
        scale, offset = np.ones(nfull), np.zeros(nfull)
        kind[fixed] = PMAP_FIXED
        for k, (sk, sc, of) in tied.items():
            kind[int(k)], src[int(k)], scale[int(k)], offset[int(k)] = PMAP_TIED, int(sk), float(sc), float(of)
        rc = self.lib.nlh_pmap_create(nfull, kind.ctypes.data_as(c_int32_p), src.ctypes.data_as(c_int32_p),
                                      scale.ctypes.data_as(c_double_p), offset.ctypes.data_as(c_double_p), C.byref(self.ptr))
        if rc:
            self.ptr = C.c_void_p()
            raise ValueError(f"ParamMap: the library refuses this map (nlh_pmap_create returned {rc}): a tie must name a free or "
                             "fixed source other than itself, with a finite non-zero scale and a finite offset, and at least one "
                             f"parameter must stay free (nfull <= {8192})")
        s = [C.c_int32() for _ in range(3)]
        self.lib.nlh_pmap_shape(self.ptr, *[C.byref(v) for v in s])
        self.nfull, self.nfree, self.ntied = (v.value for v in s)

    @classmethod
    def for_expr(cls, expr, fixed=(), tied=None):
        """The same by the parameter names of an Expr: ParamMap.for_expr(e, fixed=("b",), tied={"w2": ("w1", 1.25, 0.0)})."""
        names = [v.strip() for v in expr.params.split(",")]

        def at(name):
            if name not in names:
                raise ValueError(f"ParamMap: {name!r} is not a parameter of the formula ({', '.join(names)})")
            return names.index(name)
        return cls(len(names), fixed=[at(k) for k in fixed], tied={at(k): (at(v[0]), v[1], v[2]) for k, v in (tied or {}).items()})

    def tables(self):
        """(kind, index, scale, offset, free_to_full): the read-back of nlh_pmap_tables as numpy arrays."""
        import numpy as np
        kind, index = np.zeros(self.nfull, dtype=np.int32), np.zeros(self.nfull, dtype=np.int32)
        scale, offset = np.zeros(self.nfull), np.zeros(self.nfull)
        f2f = np.zeros(self.nfree, dtype=np.int32)
        rc = self.lib.nlh_pmap_tables(self.ptr, kind.ctypes.data_as(c_int32_p), index.ctypes.data_as(c_int32_p),
                                      scale.ctypes.data_as(c_double_p), offset.ctypes.data_as(c_double_p), f2f.ctypes.data_as(c_int32_p))
        if rc:
            raise RuntimeError(f"nlh_pmap_tables returned {rc}")
        return kind, index, scale, offset, f2f


class Group(Owner):
    """A group of data sets for a global fit (nlh_group_create: host code, needs no GPU): nsets data sets of one model with
    nparams parameters, of which the ones listed in shared have one value for the whole group and the others are free per data
    set.  E.g. Group(3, shared=(1,), nsets=8): eight decays a*exp(-k*t)+c with one k.  The outer unknowns are nouter =
    S + nsets * (nparams - S): the shared parameters first, in ascending index, then the local ones of data set 0, 1, ...,
    each in ascending index; index(set, k) is the outer unknown of parameter k of data set `set`.  Raises ValueError for what
    the library refuses (an index out of range or repeated, nsets < 1).  A group's Jacobian is dense to the solver: nsets of
    tens, not thousands.  close() frees it (so does garbage collection)."""
    _free = "nlh_group_destroy"

    def __init__(self, nparams, shared=(), nsets=1):
        import numpy as np
        self.lib = load()
        self.ptr = C.c_void_p()
        sh = np.ascontiguousarray([int(k) for k in shared], dtype=np.int32)
        rc = self.lib.nlh_group_create(int(nparams), len(sh), sh.ctypes.data_as(c_int32_p), int(nsets), C.byref(self.ptr))
        if rc:
            self.ptr = C.c_void_p()
            raise ValueError(f"Group: the library refuses this group (nlh_group_create returned {rc}): nparams must be 1 .. 8192, "
                             "shared must hold distinct indices in 0 .. nparams - 1, nsets must be at least 1, and the outer "
                             "unknowns S + nsets * (nparams - S) must fit 31 bits")
        s = [C.c_int32() for _ in range(4)]
        self.lib.nlh_group_shape(self.ptr, *[C.byref(v) for v in s])
        self.nparams, self.nshared, self.nsets, self.nouter = (v.value for v in s)

    @classmethod
    def for_expr(cls, expr, shared=(), nsets=1):
        """The same by the parameter names of an Expr: Group.for_expr(e, shared=("k",), nsets=8)."""
        names = [v.strip() for v in expr.params.split(",")]
        for name in shared:
            if name not in names:
                raise ValueError(f"Group: {name!r} is not a parameter of the formula ({', '.join(names)})")
        return cls(len(names), shared=[names.index(k) for k in shared], nsets=nsets)

    def index(self, set, k):
        """The outer unknown of parameter k of data set `set` (nlh_group_index)."""
        j = self.lib.nlh_group_index(self.ptr, int(set), int(k))
        if j < 0:
            raise IndexError(f"Group.index({set}, {k}): outside {self.nsets} data sets of {self.nparams} parameters")
        return j


SEP_MAX_L = 32


class Separable(Owner):
    """Which of a model's nparams parameters are linear (nlh_sep_create: host code, needs no GPU), for a separable fit:
    variable projection solves for them exactly at every trial point, the solver iterates over the others.  linear: their
    indices, in any order.  E.g. Separable(5, linear=(0, 2, 4)) for a1*exp(-k1*t) + a2*exp(-k2*t) + c.  The nonlinear unknowns
    are the other parameters in ascending index.  "Linear" is a declaration: the model must be affine in those parameters at
    fixed nonlinear ones (DeviceSolver.sep_check measures it).  Raises ValueError for what the library refuses (no or more than
    32 linear parameters, none left nonlinear, an index out of range or repeated).  close() frees it (so does garbage
    collection)."""
    _free = "nlh_sep_destroy"

    def __init__(self, nparams, linear=()):
        import numpy as np
        self.lib = load()
        self.ptr = C.c_void_p()
        idx = [int(k) for k in linear]
        lin = np.ascontiguousarray(sorted(idx), dtype=np.int32)
        rc = self.lib.nlh_sep_create(int(nparams), len(lin), lin.ctypes.data_as(c_int32_p), C.byref(self.ptr))
        if rc:
            self.ptr = C.c_void_p()
            raise ValueError(f"Separable: the library refuses this declaration (nlh_sep_create returned {rc}): linear must hold "
                             f"1 .. {SEP_MAX_L} distinct indices in 0 .. nparams - 1 and leave at least one parameter nonlinear")
        s = [C.c_int32() for _ in range(3)]
        self.lib.nlh_sep_shape(self.ptr, *[C.byref(v) for v in s])
        self.nparams, self.nlin, self.nnonlin = (v.value for v in s)

    @classmethod
    def for_curve(cls, kind, ncomp=1, baseline=-1):
        """The amplitudes and the baseline coefficients of a built-in curve model."""
        k = curve_kind(kind)
        n = curve_nparams(k, ncomp, baseline)
        per = 2 if k == CURVE_EXPDECAY else 3
        return cls(n, linear=[per * c for c in range(int(ncomp))] + list(range(per * int(ncomp), n)))

    @classmethod
    def for_expr(cls, expr, linear=()):
        """The same by the parameter names of an Expr: Separable.for_expr(e, linear=("a", "c"))."""
        names = [v.strip() for v in expr.params.split(",")]
        for name in linear:
            if name not in names:
                raise ValueError(f"Separable: {name!r} is not a parameter of the formula ({', '.join(names)})")
        return cls(len(names), linear=[names.index(k) for k in linear])

    def tables(self):
        """(linear, nonlinear): the full indices of the linear parameters and of the nonlinear unknowns (nlh_sep_tables)."""
        import numpy as np
        lin, nl = np.zeros(self.nlin, dtype=np.int32), np.zeros(self.nnonlin, dtype=np.int32)
        rc = self.lib.nlh_sep_tables(self.ptr, lin.ctypes.data_as(c_int32_p), nl.ctypes.data_as(c_int32_p))
        if rc:
            raise RuntimeError(f"nlh_sep_tables returned {rc}")
        return lin, nl


# limits of the box scan (include/nonlin_hip_starts.h: NLH_STARTS_*)
STARTS_MAX_N, STARTS_MAX_KEEP, STARTS_MAX_CAND = 32, 8, 1 << 20


class Starts:
    """The box scan that makes starting values (include/nonlin_hip_starts.h: nlh_starts_*; host data only, needs no GPU):
    the cost of the model at ncand candidate points of the box lower .. upper, for every problem at once, and a fit from the
    keep best of them, of which the best result is returned.  The box is over the model's full parameter vector, one box for
    every problem; it is the scan's alone and independent of a fit's own lower / upper.  log: the indices of the parameters
    whose candidates are spread evenly in the logarithm (they need lower > 0).  E.g.

        Starts(lower=(0.1, 1.0, -pi, -2.0), upper=(10.0, 60.0, pi, 2.0), ncand=4096, log=(0,))

    The candidates are the unscrambled Halton sequence, which degrades as the dimensions grow: scan few parameters -- with
    sep= only the nonlinear ones are scanned -- or give the ones that are known a tight box (lower == upper is allowed).
    Raises ValueError for what the library refuses: no or more than 32 parameters, a bound that is not finite, lower > upper,
    a log parameter with lower <= 0, ncand outside 1 .. 2^20, keep outside 1 .. 8 or above ncand.
    After curve_fit_batch / expr_fit_batch(..., starts=s) the record of that call is on s: s.which [nprob] (int32, the k of
    the start whose fit was returned, -1: no fit ended with a finite cost), s.index [nprob, keep] (int32, the candidates
    kept, -1: none) and s.cost [nprob, keep] (their cost in the scan), device tensors."""

    def __init__(self, lower, upper, ncand=256, keep=1, log=()):
        import numpy as np
        try:
            lo, hi = np.array(lower, dtype=np.float64), np.array(upper, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("Starts: lower and upper must be sequences of numbers") from None
        if lo.ndim != 1 or lo.shape != hi.shape:
            raise ValueError("Starts: lower and upper are 1-D and of one length, the model's parameters")
        for v, name in ((ncand, "ncand"), (keep, "keep")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Starts: {name} must be an integer, not {v!r}")
        n = len(lo)
        lg = np.zeros(n, dtype=np.int32)
        for k in log:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) < n:
                raise ValueError(f"Starts: log holds indices in 0 .. {n - 1}, not {k!r}")
            lg[int(k)] = 1
        self.lower, self.upper, self.logscale = np.ascontiguousarray(lo), np.ascontiguousarray(hi), lg
        self.n, self.ncand, self.keep = n, int(ncand), int(keep)
        self.which = self.index = self.cost = None
        if not 1 <= self.ncand <= STARTS_MAX_CAND:
            raise ValueError(f"Starts: ncand must be in 1 .. {STARTS_MAX_CAND}, not {ncand}")
        if not 1 <= self.keep <= min(STARTS_MAX_KEEP, self.ncand):
            raise ValueError(f"Starts: keep must be in 1 .. {STARTS_MAX_KEEP} and at most ncand, not {keep}")
        if self._candidates(self.lower, self.upper, lg, 0, 0) is None:
            raise ValueError(f"Starts: the library refuses this box (1 .. {STARTS_MAX_N} parameters, finite bounds, lower <= upper, "
                             "lower > 0 where log)")

    @classmethod
    def for_expr(cls, expr, lower, upper, ncand=256, keep=1, log=()):
        """The same by the parameter names of an Expr: lower and upper are dicts that name every parameter, log names.
        Starts.for_expr(e, lower={"a": 0.1, "k": 0.01}, upper={"a": 10.0, "k": 100.0}, log=("k",))."""
        names = [v.strip() for v in expr.params.split(",")]
        for given in (lower, upper, log):
            for name in given:
                if name not in names:
                    raise ValueError(f"Starts: {name!r} is not a parameter of the formula ({', '.join(names)})")
        for given in (lower, upper):
            for name in names:
                if name not in given:
                    raise ValueError(f"Starts: the box has no bound for the parameter {name!r}")
        return cls([lower[k] for k in names], [upper[k] for k in names], ncand, keep, [names.index(k) for k in log])

    @staticmethod
    def _candidates(lo, hi, lg, first, count):
        """nlh_starts_candidates: the table [count, n], or None when the library refuses."""
        import numpy as np
        out = np.empty((count, len(lo)))
        rc = load().nlh_starts_candidates(len(lo), first, count, lo.ctypes.data_as(c_double_p), hi.ctypes.data_as(c_double_p),
                                          lg.ctypes.data_as(c_int32_p), out.ctypes.data_as(c_double_p))
        return None if rc else out

    def box(self, positions=None):
        """(lower, upper, logscale) as the library reads them, of the parameters at `positions` (None: all), in that order:
        dimension d of the scan is positions[d]."""
        import numpy as np
        if positions is None:
            return self.lower, self.upper, self.logscale
        pos = [int(k) for k in positions]
        if not pos or any(not 0 <= k < self.n for k in pos) or len(set(pos)) != len(pos):
            raise ValueError(f"Starts: positions holds distinct indices in 0 .. {self.n - 1}")
        return tuple(np.ascontiguousarray(a[pos]) for a in (self.lower, self.upper, self.logscale))

    def candidates(self, first=0, count=None, positions=None):
        """The candidates first .. first + count - 1 (count None: up to ncand) as a table [count, n] -- or over the parameters
        at `positions` alone -- (nlh_starts_candidates: host code)."""
        count = self.ncand - first if count is None else count
        out = self._candidates(*self.box(positions), int(first), int(count))
        if out is None:
            raise ValueError(f"Starts.candidates: first >= 0, count >= 0 and first + count <= {STARTS_MAX_CAND}")
        return out


# kinds of a robust loss (include/nonlin_hip.h: NLH_LOSS_*)
LOSS_LINEAR, LOSS_HUBER, LOSS_SOFT_L1, LOSS_CAUCHY = 0, 1, 2, 3
LOSS_KINDS = {"linear": LOSS_LINEAR, "huber": LOSS_HUBER, "soft_l1": LOSS_SOFT_L1, "cauchy": LOSS_CAUCHY}


# kinds and limits of the bootstrap (include/nonlin_hip_boot.h: NLH_BOOT_*)
BOOT_RESIDUAL, BOOT_WILD, BOOT_PAIRS = 0, 1, 2
BOOT_KINDS = {"residual": BOOT_RESIDUAL, "wild": BOOT_WILD, "pairs": BOOT_PAIRS}
BOOT_MAX_ROWS, BOOT_MAX_REP = 16384, 4096
# the intervals of the one-call bootstraps, and the flags of a BCa interval (include/nonlin_hip_boot_ci.h: NLH_BCA_*)
BOOT_INTERVALS = ("percentile", "student", "bca")
BCA_DEGENERATE, BCA_NO_ACCEL, BCA_BAD_DENOM, BCA_NO_REPLICA = 1, 2, 4, 8


def bca_levels(c2, cnt, a, level=0.95):
    """nlh_boot_bca_levels (host code, needs no GPU): (z0, alpha_lo, alpha_hi, flag) of a BCa interval from c2 = 2*#{replicas
    below the fit} + #{equal to it}, cnt valid replicas, the acceleration a and the level -- what boot_bca computes per problem
    and parameter --, or None when the library refuses."""
    try:
        args = [int(c2), int(cnt), float(a), float(level)]
    except (TypeError, ValueError):
        return None
    if any(not -(1 << 31) <= v < (1 << 31) for v in args[:2]):
        return None
    z0, alo, ahi, flag = C.c_double(), C.c_double(), C.c_double(), C.c_int32()
    rc = load().nlh_boot_bca_levels(*args, C.byref(z0), C.byref(alo), C.byref(ahi), C.byref(flag))
    return (z0.value, alo.value, ahi.value, int(flag.value)) if rc == 0 else None


class Bootstrap:
    """The bootstrap of a fit (include/nonlin_hip_boot.h: nlh_boot_*; host data only, needs no GPU): nrep resampled copies of
    every data set are refitted and the spread of their parameters is the uncertainty -- no linearisation, no Gaussian.  kind:
    "residual" (the fit's weighted residuals, drawn with replacement, are added back to the fitted values: noise of one size),
    "wild" (every residual keeps its row and takes a random sign: noise whose size varies along the rows), "pairs" (rows are
    drawn with replacement: a row drawn c times weighs sqrt(c) times its weight) or a BOOT_* constant.  seed: any integer,
    taken mod 2^64; a replica depends on (seed, problem, replica) alone.  level: the coverage of the percentile interval,
    inside (0, 1).  centre: subtract the mean residual before drawing ("residual" only).  interval: which interval the one-call
    bootstraps return (include/nonlin_hip_boot_ci.h) -- "percentile" (the quantiles of the refits), "student" (bootstrap-t: the
    quantiles of (x* - x)/sigma*, which needs every refit's covariance and the fit's own sigma) or "bca" (bias-corrected and
    accelerated: the percentile levels moved by the share of refits below x and by the skewness of m delete-one refits per data
    set).  E.g.
        Bootstrap(nrep=200, kind="wild", seed=7)
    Raises ValueError for what the library refuses."""

    def __init__(self, nrep=200, kind="residual", seed=0, level=0.95, centre=True, interval="percentile"):
        import numpy as np
        if not isinstance(interval, str) or interval not in BOOT_INTERVALS:
            raise ValueError(f"Bootstrap: unknown interval {interval!r} (one of {', '.join(BOOT_INTERVALS)})")
        self.interval = interval
        if isinstance(kind, str):
            if kind.lower() not in BOOT_KINDS:
                raise ValueError(f"Bootstrap: unknown kind {kind!r} (one of {', '.join(BOOT_KINDS)})")
            kind = BOOT_KINDS[kind.lower()]
        if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or not BOOT_RESIDUAL <= int(kind) <= BOOT_PAIRS:
            raise ValueError(f"Bootstrap: unknown kind {kind!r}")
        for name, v in (("nrep", nrep), ("seed", seed)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Bootstrap: {name} must be an integer, not {v!r}")
        if not 1 <= int(nrep) <= BOOT_MAX_REP:
            raise ValueError(f"Bootstrap: nrep must be in 1 .. {BOOT_MAX_REP}, not {nrep}")
        if isinstance(level, (bool, str)) or not hasattr(level, "__float__") or not 0.0 < float(level) < 1.0:
            raise ValueError(f"Bootstrap: level must be a number inside (0, 1), not {level!r}")
        self.kind, self.nrep, self.seed = int(kind), int(nrep), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.level, self.centre = float(level), bool(centre)

    @property
    def name(self):
        return next(k for k, v in BOOT_KINDS.items() if v == self.kind)

    def draws(self, p, b, first, count, cnt):
        """nlh_boot_draws: the draws first .. first + count - 1 of the stream of problem p and replica b as int32 [count] --
        indices below cnt, or with cnt == 0 the sign bits --, or None when the library refuses."""
        import numpy as np
        try:
            args = [int(p), int(b), int(first), int(count), int(cnt)]
        except (TypeError, ValueError):
            return None
        if not -(1 << 63) <= args[0] < (1 << 63) or any(not -(1 << 31) <= a < (1 << 31) for a in args[1:]):
            return None
        out = np.empty((max(args[3], 0),), dtype=np.int32)
        rc = load().nlh_boot_draws(self.seed, *args, out.ctypes.data_as(c_int32_p))
        return out if rc == 0 else None


# the largest mean the Poisson bootstrap draws from (include/nonlin_hip_boot_pois.h: NLH_BOOT_POIS_MAX_MEAN)
BOOT_POIS_MAX_MEAN = 1 << 24


class PoissonBootstrap:
    """The parametric bootstrap of a fit of counts (include/nonlin_hip_boot_pois.h: nlh_boot_poisson_*; host data only, needs no
    GPU): every replica holds counts y* ~ Poisson(mu) drawn from the fitted values mu, and is refitted with the same deviance
    (stat=Poisson()).  For counting data the kinds of Bootstrap are wrong -- a resampled residual added to a fitted value is
    not a count and can be negative --, and at low counts, where the likelihood is skewed, the linearised x +- 1.96 sigma is
    least trustworthy.  nrep, seed, level and interval are Bootstrap's; a replica depends on (seed, problem, replica, mu) alone.  A
    fitted value that is a NaN, negative or above BOOT_POIS_MAX_MEAN = 2^24 on an unmasked row makes its problem's bootstrap
    invalid (above 2^24 counts are Gaussian to 2.5e-4: Bootstrap("wild") with weights 1/sqrt(mu) serves).  E.g.
        PoissonBootstrap(nrep=200, seed=7)
    Raises ValueError for what the library refuses."""

    def __init__(self, nrep=200, seed=0, level=0.95, interval="percentile"):
        try:
            base = Bootstrap(nrep=nrep, seed=seed, level=level, interval=interval)     # the shared fields: Bootstrap's validation
        except ValueError as exc:
            raise ValueError("Poisson" + str(exc)) from None
        self.nrep, self.seed, self.level, self.interval = base.nrep, base.seed, base.level, base.interval

    def draws(self, p, b, first, mu):
        """nlh_boot_poisson_draws: the draws of the rows first .. first + len(mu) - 1 of the stream of problem p and replica b
        for the means mu, as float64 [len(mu)] -- a NaN for a mean that is a NaN, negative or above 2^24 --, or None when the
        library refuses."""
        import numpy as np
        try:
            args = [int(p), int(b), int(first)]
            mu = np.ascontiguousarray(mu, dtype=np.float64)
        except (TypeError, ValueError):
            return None
        if mu.ndim != 1 or not -(1 << 63) <= args[0] < (1 << 63) or any(not -(1 << 31) <= a < (1 << 31) for a in args[1:]):
            return None
        out = np.empty(mu.shape, dtype=np.float64)
        rc = load().nlh_boot_poisson_draws(self.seed, *args, len(mu), mu.ctypes.data_as(c_double_p), out.ctypes.data_as(c_double_p))
        return out if rc == 0 else None


# the flags of a profile's ends (include/nonlin_hip_profile.h: NLH_PROFILE_*): one code, plus the bit PROFILE_LOWER
(PROFILE_OK, PROFILE_OPEN, PROFILE_OPEN_AT_BOUND, PROFILE_ON_BOUND, PROFILE_MAXIT, PROFILE_FIT_FAILED, PROFILE_NO_START,
 PROFILE_NOT_FREE) = range(8)
PROFILE_LOWER = 16
PROFILE_FLAGS = ("OK", "OPEN", "OPEN_AT_BOUND", "ON_BOUND", "MAXIT", "FIT_FAILED", "NO_START", "NOT_FREE")
PROFILE_EXPAND, PROFILE_BRACKET, PROFILE_DONE = 0, 1, 2


class Profile:
    """The profile-likelihood interval of a fit (include/nonlin_hip_profile.h: nlh_profile_*; host data only, needs no GPU): every
    parameter in turn is moved away from its fitted value, all the others are refitted at each trial value, and the interval ends
    where the cost has risen by a fixed amount -- MINUIT's MINOS, lmfit's conf_interval.  It is asymmetric when the problem is, and
    open when the data do not bound the parameter.  level: the coverage, inside (0, 1).  crit: the rise that defines the end, in
    units of the cost's scale -- None: the squared normal quantile of (1 + level)/2 (3.84 at 0.95); with few degrees of freedom
    pass a squared Student-t quantile; 1.0 is the Delta = 1 convention.  tol: an end is found when the rise is within tol*delta of
    delta.  xtol: or when its bracket is below xtol*sqrt(crit)*sigma.  max_expand: doublings of the first step sqrt(crit)*sigma before an
    end is declared open.  maxit: evaluations per end at the most.  E.g.
        Profile(level=0.68, crit=1.0)
    Raises ValueError for malformed values."""

    def __init__(self, level=0.95, crit=None, tol=0.01, xtol=1e-3, max_expand=8, maxit=30):
        import math
        import statistics

        def number(name, v, lo_open, hi_open=None):
            if isinstance(v, (bool, str)) or not hasattr(v, "__float__") or not math.isfinite(float(v)) or not float(v) > lo_open or \
                    (hi_open is not None and not float(v) < hi_open):
                raise ValueError(f"Profile: {name} must be a finite number above {lo_open}" +
                                 (f" and below {hi_open}" if hi_open is not None else "") + f", not {v!r}")
            return float(v)
        self.level = number("level", level, 0.0, 1.0)
        if crit is None:
            z = statistics.NormalDist().inv_cdf((1.0 + self.level) / 2.0)
            crit = z * z
        self.crit = number("crit", crit, 0.0)
        self.tol = number("tol", tol, 0.0, 1.0)
        self.xtol = number("xtol", xtol, 0.0, 1.0)
        for name, v, least in (("max_expand", max_expand, 0), ("maxit", maxit, 1)):
            if isinstance(v, bool) or not isinstance(v, int) or not least <= v < (1 << 31):
                raise ValueError(f"Profile: {name} must be an integer of at least {least}, not {v!r}")
        self.max_expand, self.maxit = int(max_expand), int(maxit)


class Loss:
    """A robust loss (include/nonlin_hip.h: nlh_loss_*; host data only, needs no GPU): kind -- "linear", "huber", "soft_l1",
    "cauchy" or a LOSS_* constant -- and the scale c: one positive finite number for every problem, or a sequence with one
    per problem.  Residuals well inside c are treated as least squares treats them; far outside, their pull is bounded.
    E.g. Loss("huber", 3 * sigma_noise).  Raises ValueError for an unknown kind and for a scale that is not finite or not
    positive (what the library's host-array entry points refuse); "linear" ignores the scale."""

    def __init__(self, kind, scale=1.0):
        import numpy as np
        if isinstance(kind, str):
            if kind.lower() not in LOSS_KINDS:
                raise ValueError(f"Loss: unknown kind {kind!r} (one of {', '.join(LOSS_KINDS)})")
            kind = LOSS_KINDS[kind.lower()]
        if isinstance(kind, bool) or not isinstance(kind, (int, np.integer)) or not LOSS_LINEAR <= int(kind) <= LOSS_CAUCHY:
            raise ValueError(f"Loss: unknown kind {kind!r}")
        self.kind = int(kind)
        try:
            sc = np.array(scale, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"Loss: the scale must be a number or a sequence of numbers, not {scale!r}") from None
        if sc.ndim > 1 or sc.size == 0:
            raise ValueError("Loss: the scale is one number, or one number per problem")
        if not (np.isfinite(sc).all() and (sc > 0.0).all()):
            raise ValueError("Loss: the scale must be finite and positive")
        self.shared = sc.ndim == 0
        self.scale = np.ascontiguousarray(sc.reshape(-1))

    def scale_for(self, nprob):
        """The host scales a call on nprob problems passes: ([1], shared = 1) or ([nprob], shared = 0)."""
        if not self.shared and len(self.scale) != nprob:
            raise ValueError(f"Loss: {len(self.scale)} scales for {nprob} problems")
        return self.scale, int(self.shared)


class Poisson:
    """The Poisson likelihood as the statistic of a fit (include/nonlin_hip.h: nlh_pois_*; host data only, needs no GPU): the
    fit minimises the Poisson deviance of the counts y instead of a sum of squares.  mu_floor: below this model value the
    deviance residual is continued linearly (C1), so that a model that strays to zero or below keeps a slope.  The default,
    2^-20, is far below one count, so no meaningful model touches it, and large enough that the extension's slope stays
    finite; it is a default, not a measurement.  Raises ValueError for a floor that is not finite or not positive (what the
    library's entry points refuse)."""

    def __init__(self, mu_floor=2.0 ** -20):
        if isinstance(mu_floor, (bool, str)) or not hasattr(mu_floor, "__float__"):
            raise ValueError(f"Poisson: mu_floor must be a number, not {mu_floor!r}")
        try:
            f = float(mu_floor)
        except (TypeError, ValueError):
            raise ValueError(f"Poisson: mu_floor must be a number, not {mu_floor!r}") from None
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError("Poisson: mu_floor must be finite and positive")
        self.mu_floor = f


# extensions of an instrument response beyond the rows of the data (include/nonlin_hip.h: NLH_CONV_*)
CONV_ZERO, CONV_HOLD = 0, 1
CONV_EXTENDS = {"zero": CONV_ZERO, "hold": CONV_HOLD}
CONV_MAX_L = 1024


class ConvStruct(C.Structure):
    """nlh_conv."""
    _fields_ = [("L", C.c_int32), ("origin", C.c_int32), ("ext", C.c_int32), ("shared_k", C.c_int32), ("k", C.c_void_p)]


class Convolve:
    """An instrument response as the transform of a fit (include/nonlin_hip.h: nlh_conv_*; host data only, needs no GPU): the
    model is convolved along its rows with `kernel` before it is compared with the data.  kernel: 1-D, one for every problem,
    or 2-D [nprob, L], one per problem; L = 1 .. 1024 taps.  origin: the tap that sits on the output row -- 0 a causal
    response (an IRF), (L - 1) // 2 a centred one (a line shape).  extend: "zero" (rows outside the data contribute nothing)
    or "hold" (they take the nearest edge row's value).  The kernel is used as given; normalize=True divides each kernel by
    the sequential sum of its taps first.  Raises ValueError for what the library refuses: no taps or too many, an origin
    outside 0 .. L - 1, an unknown extension, a tap that is not finite (a sum that is zero or not finite, with normalize)."""

    def __init__(self, kernel, origin=0, extend="zero", normalize=False):
        import numpy as np
        try:
            k = np.array(kernel, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"Convolve: the kernel must be a sequence of numbers, not {kernel!r}") from None
        if k.ndim not in (1, 2) or k.shape[-1] < 1 or k.shape[0] < 1:
            raise ValueError("Convolve: the kernel is 1-D [L], or 2-D [nprob, L], with at least one tap")
        if k.shape[-1] > CONV_MAX_L:
            raise ValueError(f"Convolve: {k.shape[-1]} taps, at most {CONV_MAX_L}")
        if not np.isfinite(k).all():
            raise ValueError("Convolve: every tap must be finite")
        if isinstance(origin, bool) or not isinstance(origin, (int, np.integer)) or not 0 <= int(origin) < k.shape[-1]:
            raise ValueError(f"Convolve: origin must be an integer in 0 .. {k.shape[-1] - 1}, not {origin!r}")
        if isinstance(extend, str) and extend.lower() in CONV_EXTENDS:
            ext = CONV_EXTENDS[extend.lower()]
        elif not isinstance(extend, (bool, str)) and isinstance(extend, (int, np.integer)) and int(extend) in (CONV_ZERO, CONV_HOLD):
            ext = int(extend)
        else:
            raise ValueError(f"Convolve: unknown extension {extend!r} (one of {', '.join(CONV_EXTENDS)})")
        self.shared = k.ndim == 1
        k = np.ascontiguousarray(k.reshape(-1, k.shape[-1]))
        if normalize:
            tot = np.zeros(len(k))
            with np.errstate(over="ignore"):
                for j in range(k.shape[1]):                          # the sequential sum, tap by tap
                    tot = tot + k[:, j]
            if not (np.isfinite(tot).all() and (tot != 0.0).all()):
                raise ValueError("Convolve: normalize needs taps whose sum is finite and not zero")
            k = k / tot[:, None]
        self.kernel = k                                              # [1, L] or [nprob, L]
        self.L, self.origin, self.ext = int(k.shape[1]), int(origin), ext

    def kernel_for(self, nprob):
        """The host taps a call on nprob problems passes: ([L], shared = 1) or ([nprob, L], shared = 0)."""
        if not self.shared and len(self.kernel) != nprob:
            raise ValueError(f"Convolve: kernels for {len(self.kernel)} problems, the call has {nprob}")
        return (self.kernel[0] if self.shared else self.kernel), int(self.shared)

    def struct(self, kptr):
        """nlh_conv with the taps at kptr (a device or host address, as the entry point wants them)."""
        return ConvStruct(self.L, self.origin, self.ext, int(self.shared), kptr)


# limits of a bin-integrated fit (include/nonlin_hip_bin.h: NLH_BIN_MAX_Q; nlh_bin_rule has the orders 1 .. 8)
BIN_MAX_Q, BIN_MAX_ORDER = 16, 8
BIN_MODES = ("integral", "mean")


class BinStruct(C.Structure):
    """nlh_bin."""
    _fields_ = [("Q", C.c_int32), ("c", C.c_double * BIN_MAX_Q), ("s", C.c_void_p), ("shared_s", C.c_int32)]


def bin_rule(order):
    """(xi, c): the Gauss-Legendre nodes (ascending) and weights on [-1, 1] of `order` nodes, 1 .. 8 (nlh_bin_rule: host code,
    needs no GPU).  ValueError for another order."""
    import numpy as np
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= int(order) <= BIN_MAX_ORDER:
        raise ValueError(f"Binned: order must be an integer in 1 .. {BIN_MAX_ORDER}, not {order!r}")
    xi, c = np.zeros(int(order)), np.zeros(int(order))
    if load().nlh_bin_rule(int(order), xi.ctypes.data_as(c_double_p), c.ctypes.data_as(c_double_p)):
        raise ValueError(f"Binned: the library has no rule of order {order!r}")
    return xi, c


class Binned:
    """The bins of histogrammed data as the transform of a fit (include/nonlin_hip_bin.h: nlh_bin_*; host data only, needs no
    GPU): the model is integrated over every bin lo .. hi (mode "integral": a density against counts) or averaged over it
    (mode "mean": a pixel against an image) by a quadrature rule before it is compared with the data, instead of being
    evaluated at one point.  lo, hi: the edges of the bins, [m] for every problem or [nprob, m], lo < hi.  order: the nodes of
    the Gauss-Legendre rule per bin, 1 .. 8 (order 1 is the centre value: times the width, or as it is); the rule is exact for
    polynomials up to degree 2 order - 1 across a bin.  rule=(xi, c): a caller's own nodes and weights on [-1, 1] instead, at
    most 16 (order is then not read).  With mid = 0.5 (lo + hi) and half = 0.5 (hi - lo) the nodes are mid + half xi_q;
    "integral" scales every bin's sum by half, "mean" halves the weights (exactly) and has no scale.
    Raises ValueError for edges that are not finite numbers of one shape [m] or [nprob, m], for lo >= hi, an unknown mode, an
    order outside 1 .. 8 and a rule that is not two finite sequences of one length 1 .. 16.
    Attributes: m, Q, xi, c [Q] (the weights the device reads), scale (None or [1 | nprob, m]), shared, nvar (1; 2 for
    pixels)."""

    def __init__(self, lo, hi, order=3, mode="integral", rule=None):
        import numpy as np
        lo, hi = self._edges((lo, hi), "lo and hi")
        xi, c = self._rule(order, rule)
        mode = self._mode(mode)
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
        tq = np.concatenate([mid + half * xi[q] for q in range(len(xi))], axis=-1)
        self._set(tq, xi, c if mode == "integral" else 0.5 * c, half if mode == "integral" else None, mode, 1)

    @staticmethod
    def _edges(arrays, what):
        """The edge arrays as float64 [1 | nprob, m] of one shape, checked."""
        import numpy as np
        try:
            out = [np.array(a, dtype=np.float64) for a in arrays]
        except (TypeError, ValueError):
            raise ValueError(f"Binned: {what} must be sequences of numbers") from None
        if out[0].ndim not in (1, 2) or out[0].shape[-1] < 1 or out[0].shape[0] < 1 or any(a.shape != out[0].shape for a in out):
            raise ValueError(f"Binned: {what} are [m] or [nprob, m], of one shape, with at least one bin")
        if not all(np.isfinite(a).all() for a in out):
            raise ValueError(f"Binned: every edge of {what} must be finite")
        for lo, hi in zip(out[0::2], out[1::2]):
            if not (lo < hi).all():
                raise ValueError("Binned: every bin needs lo < hi")
        return [np.ascontiguousarray(a.reshape(-1, a.shape[-1])) if a.ndim == 2 else a[None, :].copy() for a in out]

    @staticmethod
    def _mode(mode):
        if not isinstance(mode, str) or mode.lower() not in BIN_MODES:
            raise ValueError(f"Binned: unknown mode {mode!r} (one of {', '.join(BIN_MODES)})")
        return mode.lower()

    @staticmethod
    def _rule(order, rule):
        import numpy as np
        if rule is None:
            return bin_rule(order)
        try:
            xi, c = (np.array(a, dtype=np.float64) for a in rule)
        except (TypeError, ValueError):
            raise ValueError("Binned: rule must be (xi, c), two sequences of numbers") from None
        if xi.ndim != 1 or c.shape != xi.shape or not 1 <= len(xi) <= BIN_MAX_Q:
            raise ValueError(f"Binned: rule is (xi, c), two 1-D sequences of one length 1 .. {BIN_MAX_Q}")
        if not (np.isfinite(xi).all() and np.isfinite(c).all()):
            raise ValueError("Binned: every node and weight of the rule must be finite")
        return xi, c

    def _set(self, tq, xi, c, scale, mode, nvar):
        import numpy as np
        self._tq = np.ascontiguousarray(tq)                          # [1 | nprob, Q m], or [2, 1 | nprob, Q m] for pixels
        self.xi, self.c = xi, np.ascontiguousarray(c)
        self.Q = len(self.c)
        self.m = self._tq.shape[-1] // self.Q
        self.scale = None if scale is None else np.ascontiguousarray(scale)
        self.shared = self._tq.shape[-2] == 1
        self.mode, self.nvar = mode, nvar

    @classmethod
    def edges(cls, e, order=3, mode="integral", rule=None):
        """The bins between m + 1 ascending edges e, one set for every problem: Binned(e[:-1], e[1:], ...)."""
        import numpy as np
        try:
            e = np.array(e, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("Binned.edges: the edges must be a sequence of numbers") from None
        if e.ndim != 1 or len(e) < 2:
            raise ValueError("Binned.edges: m + 1 edges in one 1-D sequence, m >= 1")
        return cls(e[:-1], e[1:], order=order, mode=mode, rule=rule)

    @classmethod
    def pixels(cls, x, y, order=2, mode="mean"):
        """The pixels xlo .. xhi by ylo .. yhi of an image for a formula of two variables: x = (xlo, xhi), y = (ylo, yhi), each
        [m] or [nprob, m] (the pixels of an image in any order, flattened).  The rule is the tensor product of the
        Gauss-Legendre rule of `order` nodes, 1 .. 4, with itself: Q = order^2 nodes, node q = a order + b at (x node a,
        y node b) with weight c_a c_b -- a quarter of it under "mean" --, and the scale half_x half_y under "integral".
        nodes() is then [2, Q m] or [2, nprob, Q m]: the two variables of the formula."""
        import numpy as np
        if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= int(order) <= 4:
            raise ValueError(f"Binned.pixels: order must be an integer in 1 .. 4, not {order!r}")
        try:
            (xlo, xhi), (ylo, yhi) = x, y
        except (TypeError, ValueError):
            raise ValueError("Binned.pixels: x = (xlo, xhi) and y = (ylo, yhi)") from None
        xlo, xhi, ylo, yhi = cls._edges((xlo, xhi, ylo, yhi), "the pixel edges")
        mode = cls._mode(mode)
        xi, c1 = bin_rule(order)
        mx, hx, my, hy = 0.5 * (xlo + xhi), 0.5 * (xhi - xlo), 0.5 * (ylo + yhi), 0.5 * (yhi - ylo)
        K = int(order)
        tx = np.concatenate([mx + hx * xi[a] for a in range(K) for b in range(K)], axis=-1)
        ty = np.concatenate([my + hy * xi[b] for a in range(K) for b in range(K)], axis=-1)
        c = np.array([c1[a] * c1[b] for a in range(K) for b in range(K)])
        self = cls.__new__(cls)
        self._set(np.stack([tx, ty]), xi, c if mode == "integral" else 0.25 * c, hx * hy if mode == "integral" else None, mode, 2)
        return self

    def nodes(self):
        """The abscissae the inner model is bound on, node-major -- entry q m + i is node q of bin i --: [Q m], or
        [nprob, Q m] with edges per problem (pixels: [2, Q m] or [2, nprob, Q m])."""
        t = self._tq[..., 0, :] if self.shared else self._tq
        return t.copy()

    def nodes_for(self, nprob):
        """nodes(), checked against the nprob problems of a call."""
        if not self.shared and self._tq.shape[-2] != nprob:
            raise ValueError(f"Binned: bins for {self._tq.shape[-2]} problems, the call has {nprob}")
        return self.nodes()

    def scale_for(self, nprob):
        """The host scale a call on nprob problems passes: (None | [m] | [nprob, m], shared flag)."""
        if not self.shared and self._tq.shape[-2] != nprob:
            raise ValueError(f"Binned: bins for {self._tq.shape[-2]} problems, the call has {nprob}")
        if self.scale is None:
            return None, 1
        return (self.scale[0] if self.shared else self.scale), int(self.shared)

    def struct(self, sptr, shared):
        """nlh_bin with the scale at sptr (a device address, or None)."""
        arr = (C.c_double * BIN_MAX_Q)(*([float(v) for v in self.c] + [0.0] * (BIN_MAX_Q - self.Q)))
        return BinStruct(self.Q, arr, sptr, int(shared))


class Handle(Owner):
    """Owns an nlh_handle bound to a device and (optionally) an existing HIP stream."""
    _slot, _free = "_h", "nlh_destroy"

    def __init__(self, device=0, stream=None):
        lib = load()
        if lib.nlh_device_count() <= 0:
            raise NonlinHipUnavailable("no HIP device visible: the nonlin_amd compute path needs a GPU "
                                       "(there is no CPU fallback)")
        self._h = C.c_void_p()
        rc = lib.nlh_create(C.byref(self._h), int(device), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise NonlinHipUnavailable(f"nlh_create failed with {rc}")
        self.lib = lib

    @property
    def ptr(self):
        return self._h

    def check(self, rc, what):
        if rc < 0:
            raise RuntimeError(f"{what}: library error {rc}: {self.lib.nlh_last_error(self._h).decode()}")
        return rc

    def timing_enable(self, on=True, kernels=None):
        """on: every kernel group; kernels=[names]: only those groups (two event records per timed launch)."""
        if kernels:
            mask = 0
            for k in kernels:
                mask |= 1 << (KERNEL_IDS[k] + 1)
            self.lib.nlh_timing_enable(self._h, mask)
        else:
            self.lib.nlh_timing_enable(self._h, 1 if on else 0)

    def timing_reset(self):
        self.lib.nlh_timing_reset(self._h)

    def timing(self, kernel):
        """Returns (total_ms, launches) measured with HIP events on the handle's stream."""
        ms = C.c_double(0.0)
        cnt = C.c_int64(0)
        self.lib.nlh_timing_get(self._h, KERNEL_IDS[kernel], C.byref(ms), C.byref(cnt))
        return ms.value, cnt.value

    def timing_samples(self, kernel, select_only=False):
        """Per-launch durations (ms, launch order) of one kernel group since the last timing_reset.  The group must have
        been selected before the launches (select_only=True) and be enabled in timing_enable."""
        kid = KERNEL_IDS[kernel]
        n = self.lib.nlh_timing_samples(self._h, kid, None, 0)
        if select_only or n <= 0:
            return []
        buf = (C.c_float * n)()
        n = self.lib.nlh_timing_samples(self._h, kid, buf, n)
        return [float(buf[i]) for i in range(n)]
