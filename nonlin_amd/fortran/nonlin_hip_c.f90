! nonlin_hip_c.f90 -- ISO_C_BINDING view of include/nonlin_hip.h (libnonlin_hip.so).
! One interface body per C entry point the Fortran shim uses; struct layouts mirror the header.
module nonlin_hip_c
    use, intrinsic :: iso_c_binding
    implicit none
    public

    type, bind(C) :: nlh_iteration_behavior
        integer(c_int32_t) :: iter_count, fcn_count, jacobian_count, gradient_count
        integer(c_int32_t) :: converge_on_fcn, converge_on_chng, converge_on_zero_diff
    end type

    type, bind(C) :: nlh_options
        integer(c_int32_t) :: max_evals
        real(c_double) :: ftol, xtol, gtol
        integer(c_int32_t) :: print_status
        real(c_double) :: factor
        integer(c_int32_t) :: use_line_search, ls_max_evals
        real(c_double) :: ls_alpha, ls_factor
        integer(c_int32_t) :: factor_policy
        real(c_double) :: ne_pivot_tol
        integer(c_int32_t) :: fuse_fd
        integer(c_int32_t) :: sub_batches
    end type

    integer(c_int32_t), parameter :: NLH_FACTOR_AUTO = 0, NLH_FACTOR_QR = 1, NLH_FACTOR_EXACT = 2
    ! kinds of the built-in curve models (include/nonlin_hip.h: NLH_CURVE_*)
    integer(c_int32_t), parameter :: NLH_CURVE_GAUSS = 0, NLH_CURVE_LORENTZ = 1, NLH_CURVE_EXPDECAY = 2
    ! kinds of a parameter of a map (include/nonlin_hip.h: NLH_PMAP_*)
    integer(c_int32_t), parameter :: NLH_PMAP_FREE = 0, NLH_PMAP_FIXED = 1, NLH_PMAP_TIED = 2
    ! kinds of a robust loss (include/nonlin_hip.h: NLH_LOSS_*)
    integer(c_int32_t), parameter :: NLH_LOSS_LINEAR = 0, NLH_LOSS_HUBER = 1, NLH_LOSS_SOFT_L1 = 2, NLH_LOSS_CAUCHY = 3
    ! extensions of an instrument response beyond the rows of the data, and the transform itself (include/nonlin_hip.h: nlh_conv)
    integer(c_int32_t), parameter :: NLH_CONV_ZERO = 0, NLH_CONV_HOLD = 1
    type, bind(C) :: nlh_conv
        integer(c_int32_t) :: L
        integer(c_int32_t) :: origin
        integer(c_int32_t) :: ext
        integer(c_int32_t) :: shared_k
        type(c_ptr) :: k
    end type

    interface
        subroutine nlh_default_options(opts) bind(C, name="nlh_default_options")
            import :: nlh_options
            type(nlh_options), intent(out) :: opts
        end subroutine
        function nlh_create(h, device, stream) bind(C, name="nlh_create") result(rc)
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), intent(out) :: h
            integer(c_int32_t), value :: device
            type(c_ptr), value :: stream
            integer(c_int) :: rc
        end function
        subroutine nlh_destroy(h) bind(C, name="nlh_destroy")
            import :: c_ptr
            type(c_ptr), value :: h
        end subroutine
        function nlh_fd_jacobian(h, m, n, fcn, jacfcn, ctx, x, fv, jac) bind(C, name="nlh_fd_jacobian") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: m, n
            type(c_funptr), value :: fcn, jacfcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*)
            type(c_ptr), value :: fv
            real(c_double), intent(out) :: jac(*)
            integer(c_int) :: rc
        end function
        function nlh_lm_solve(h, opts, m, n, fcn, jacfcn, ctx, x, fvec, ib) bind(C, name="nlh_lm_solve") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            integer(c_int32_t), value :: m, n
            type(c_funptr), value :: fcn, jacfcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*)
            type(nlh_iteration_behavior), intent(out) :: ib
            integer(c_int) :: rc
        end function
        function nlh_newton_solve(h, opts, n, fcn, jacfcn, ctx, x, fvec, ib) bind(C, name="nlh_newton_solve") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            integer(c_int32_t), value :: n
            type(c_funptr), value :: fcn, jacfcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*)
            type(nlh_iteration_behavior), intent(out) :: ib
            integer(c_int) :: rc
        end function
        function nlh_bfgs_solve(h, opts, n, fcn, gradfcn, ctx, x, fout, ib) bind(C, name="nlh_bfgs_solve") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            integer(c_int32_t), value :: n
            type(c_funptr), value :: fcn, gradfcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fout
            type(nlh_iteration_behavior), intent(out) :: ib
            integer(c_int) :: rc
        end function
        function nlh_fd_gradient(n, fcn, gradfcn, ctx, x, fv, g) bind(C, name="nlh_fd_gradient") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double
            integer(c_int32_t), value :: n
            type(c_funptr), value :: fcn, gradfcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*)
            type(c_ptr), value :: fv
            real(c_double), intent(out) :: g(*)
            integer(c_int) :: rc
        end function
        function nlh_poly_fit(h, npts, order, thru_zero, x, y, coef) bind(C, name="nlh_poly_fit") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: npts, order, thru_zero
            real(c_double), intent(in) :: x(*), y(*)
            real(c_double), intent(out) :: coef(*)
            integer(c_int) :: rc
        end function
        function nlh_poly_roots(h, order, coef, z, info) bind(C, name="nlh_poly_roots") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: order
            real(c_double), intent(in) :: coef(*)
            real(c_double), intent(out) :: z(2, *)
            integer(c_int32_t), intent(out) :: info
            integer(c_int) :: rc
        end function
        function nlh_cls_solve(h, opts, delta0, stepscale0, xl, xu, m, n, fcn, jacfcn, ctx, x, fvec, ib) &
                bind(C, name="nlh_cls_solve") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            real(c_double), value :: delta0, stepscale0
            real(c_double), intent(in) :: xl(*), xu(*)
            integer(c_int32_t), value :: m, n
            type(c_funptr), value :: fcn, jacfcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*)
            type(nlh_iteration_behavior), intent(out) :: ib
            integer(c_int) :: rc
        end function
        function nlh_quasi_newton_solve(h, opts, jdelta, n, fcn, jacfcn, ctx, x, fvec, ib) &
                bind(C, name="nlh_quasi_newton_solve") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            integer(c_int32_t), value :: jdelta, n
            type(c_funptr), value :: fcn, jacfcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*)
            type(nlh_iteration_behavior), intent(out) :: ib
            integer(c_int) :: rc
        end function
        ! ---- device residual models behind host arrays (include/nonlin_hip.h: nlh_dq_model_*) ----
        function nlh_dq_model_create(h, nprob, m, n, a, b, gamma, model) bind(C, name="nlh_dq_model_create") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: nprob, m, n
            real(c_double), intent(in) :: a(*), b(*)
            real(c_double), value :: gamma
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        ! a built-in curve model on host data (include/nonlin_hip.h: nlh_curve_model_create; w: c_null_ptr for no weights)
        function nlh_curve_model_create(h, kind, ncomp, nbase, nprob, m, t, shared_t, y, w, analytic, model) &
                bind(C, name="nlh_curve_model_create") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: kind, ncomp, nbase, nprob, m, shared_t, analytic
            real(c_double), intent(in) :: t(*), y(*)
            type(c_ptr), value :: w
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        ! starting values for a curve model from host data (include/nonlin_hip_guess.h: nlh_curve_guess_batch_h; w: c_null_ptr for no
        ! weights; flag: c_null_ptr when the flags are not wanted)
        function nlh_curve_guess_batch_h(h, kind, ncomp, nbase, nprob, m, t, shared_t, y, w, smooth, x, flag) &
                bind(C, name="nlh_curve_guess_batch_h") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: kind, ncomp, nbase, nprob, m, shared_t, smooth
            real(c_double), intent(in) :: t(*), y(*)
            type(c_ptr), value :: w
            real(c_double), intent(out) :: x(*)
            type(c_ptr), value :: flag
            integer(c_int) :: rc
        end function
        ! formula models (include/nonlin_hip.h: nlh_expr_*): compile on the host, then a model object on host data
        function nlh_expr_compile(formula, vars, params, e) bind(C, name="nlh_expr_compile") result(rc)
            import :: c_ptr, c_int, c_char
            character(kind=c_char), intent(in) :: formula(*), vars(*), params(*)
            type(c_ptr), intent(out) :: e
            integer(c_int) :: rc
        end function
        function nlh_expr_error() bind(C, name="nlh_expr_error") result(msg)
            import :: c_ptr
            type(c_ptr) :: msg
        end function
        subroutine nlh_expr_destroy(e) bind(C, name="nlh_expr_destroy")
            import :: c_ptr
            type(c_ptr), value :: e
        end subroutine
        subroutine nlh_expr_shape(e, nvar, nparams, ninstr, nconst, depth) bind(C, name="nlh_expr_shape")
            import :: c_ptr, c_int32_t
            type(c_ptr), value :: e
            integer(c_int32_t), intent(out) :: nvar, nparams, ninstr, nconst, depth
        end subroutine
        function nlh_expr_model_create(h, e, nprob, m, t, shared_t, y, w, analytic, model) &
                bind(C, name="nlh_expr_model_create") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h, e
            integer(c_int32_t), value :: nprob, m, shared_t, analytic
            real(c_double), intent(in) :: t(*), y(*)
            type(c_ptr), value :: w
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        ! parameter maps (include/nonlin_hip.h: nlh_pmap_*): the map object (host code), and a model of its free unknowns
        ! over a launcher-backed model (src is 0-based here)
        function nlh_pmap_create(nfull, kind, src, scale, offset, pm) bind(C, name="nlh_pmap_create") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            integer(c_int32_t), value :: nfull
            integer(c_int32_t), intent(in) :: kind(*), src(*)
            real(c_double), intent(in) :: scale(*), offset(*)
            type(c_ptr), intent(out) :: pm
            integer(c_int) :: rc
        end function
        subroutine nlh_pmap_destroy(pm) bind(C, name="nlh_pmap_destroy")
            import :: c_ptr
            type(c_ptr), value :: pm
        end subroutine
        subroutine nlh_pmap_shape(pm, nfull, nfree, ntied) bind(C, name="nlh_pmap_shape")
            import :: c_ptr, c_int32_t
            type(c_ptr), value :: pm
            integer(c_int32_t), intent(out) :: nfull, nfree, ntied
        end subroutine
        function nlh_pmap_model_create(h, inner, pm, full, shared_full, model) bind(C, name="nlh_pmap_model_create") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h, inner, pm
            real(c_double), intent(in) :: full(*)
            integer(c_int32_t), value :: shared_full
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        ! global fits (include/nonlin_hip.h: nlh_group_*): the group object (host code), and a model of its outer unknowns
        ! over a launcher-backed model (shared is 0-based here)
        function nlh_group_create(nfull, nshared, shared, nsets, g) bind(C, name="nlh_group_create") result(rc)
            import :: c_ptr, c_int, c_int32_t
            integer(c_int32_t), value :: nfull, nshared, nsets
            integer(c_int32_t), intent(in) :: shared(*)
            type(c_ptr), intent(out) :: g
            integer(c_int) :: rc
        end function
        subroutine nlh_group_destroy(g) bind(C, name="nlh_group_destroy")
            import :: c_ptr
            type(c_ptr), value :: g
        end subroutine
        subroutine nlh_group_shape(g, nfull, nshared, nsets, nouter) bind(C, name="nlh_group_shape")
            import :: c_ptr, c_int32_t
            type(c_ptr), value :: g
            integer(c_int32_t), intent(out) :: nfull, nshared, nsets, nouter
        end subroutine
        function nlh_group_model_create(h, inner, g, model) bind(C, name="nlh_group_model_create") result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: h, inner, g
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        ! separable fits (include/nonlin_hip.h: nlh_sep_*): the object, a model of the nonlinear unknowns over a launcher-backed
        ! model, and the one-call fits behind host arrays (every array argument a C address: c_loc, or c_null_ptr where the
        ! header allows NULL)
        function nlh_sep_create(nfull, nlin, lin, sp) bind(C, name="nlh_sep_create") result(rc)
            import :: c_ptr, c_int, c_int32_t
            integer(c_int32_t), value :: nfull, nlin
            integer(c_int32_t), intent(in) :: lin(*)
            type(c_ptr), intent(out) :: sp
            integer(c_int) :: rc
        end function
        subroutine nlh_sep_destroy(sp) bind(C, name="nlh_sep_destroy")
            import :: c_ptr
            type(c_ptr), value :: sp
        end subroutine
        subroutine nlh_sep_shape(sp, nfull, nlin, nnonlin) bind(C, name="nlh_sep_shape")
            import :: c_ptr, c_int32_t
            type(c_ptr), value :: sp
            integer(c_int32_t), intent(out) :: nfull, nlin, nnonlin
        end subroutine
        function nlh_sep_model_create(h, inner, sp, model) bind(C, name="nlh_sep_model_create") result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: h, inner, sp
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        function nlh_curve_fit_batch_sep_h(h, opts, kind, ncomp, nbase, nprob, m, t, shared_t, y, w, analytic, xl, xu, g, cv, sp, x, fvec, &
                sigma, cov, chi2, rank, ib, status) bind(C, name="nlh_curve_fit_batch_sep_h") result(rc)
            import :: c_ptr, c_int, c_int32_t, nlh_options
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            integer(c_int32_t), value :: kind, ncomp, nbase, nprob, m, shared_t, analytic
            type(c_ptr), value :: t, y, w, xl, xu, g, cv, sp, x, fvec, sigma, cov, chi2, rank, ib, status
            integer(c_int) :: rc
        end function
        function nlh_expr_fit_batch_sep_h(h, opts, e, nprob, m, t, shared_t, y, w, analytic, xl, xu, g, cv, sp, x, fvec, sigma, cov, chi2, &
                rank, ib, status) bind(C, name="nlh_expr_fit_batch_sep_h") result(rc)
            import :: c_ptr, c_int, c_int32_t, nlh_options
            type(c_ptr), value :: h, e
            type(nlh_options), intent(in) :: opts
            integer(c_int32_t), value :: nprob, m, shared_t, analytic
            type(c_ptr), value :: t, y, w, xl, xu, g, cv, sp, x, fvec, sigma, cov, chi2, rank, ib, status
            integer(c_int) :: rc
        end function
        ! robust losses (include/nonlin_hip.h: nlh_loss_*): a model with a loss over a launcher-backed model
        function nlh_loss_model_create(h, inner, kind, scale, shared_scale, model) bind(C, name="nlh_loss_model_create") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h, inner
            integer(c_int32_t), value :: kind
            real(c_double), intent(in) :: scale(*)
            integer(c_int32_t), value :: shared_scale
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        ! Poisson likelihood fits (include/nonlin_hip.h: nlh_pois_*): a model minimising the deviance of counts over an unweighted model
        function nlh_pois_model_create(h, inner, y, w, mu_floor, model) bind(C, name="nlh_pois_model_create") result(rc)
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h, inner
            real(c_double), intent(in) :: y(*)
            type(c_ptr), value :: w
            real(c_double), value :: mu_floor
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        ! instrument-response fits (include/nonlin_hip.h: nlh_conv_*): an unweighted model convolved with a kernel along its rows
        function nlh_conv_model_create(h, inner, cv, y, w, model) bind(C, name="nlh_conv_model_create") result(rc)
            import :: c_ptr, c_int, c_double, nlh_conv
            type(c_ptr), value :: h, inner
            type(nlh_conv), intent(in) :: cv
            real(c_double), intent(in) :: y(*)
            type(c_ptr), value :: w
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        function nlh_curve_nparams(kind, ncomp, nbase) bind(C, name="nlh_curve_nparams") result(n)
            import :: c_int32_t
            integer(c_int32_t), value :: kind, ncomp, nbase
            integer(c_int32_t) :: n
        end function
        ! a USER'S device residual (launchers, include/nonlin_hip.h: nlh_device_vecfcn / nlh_device_jacfcn) as a model object
        function nlh_device_fcn_model_create(nprob, m, n, fcn, jacfcn, ctx, model) &
                bind(C, name="nlh_device_fcn_model_create") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t
            integer(c_int32_t), value :: nprob, m, n
            type(c_funptr), value :: fcn, jacfcn
            type(c_ptr), value :: ctx
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        ! ---- several GPUs behind the boundary (include/nonlin_hip.h: nlh_device_set_*) ----
        function nlh_device_set_create(set, devices, ndev) bind(C, name="nlh_device_set_create") result(rc)
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), intent(out) :: set
            integer(c_int32_t), intent(in) :: devices(*)
            integer(c_int32_t), value :: ndev
            integer(c_int) :: rc
        end function
        subroutine nlh_device_set_destroy(set) bind(C, name="nlh_device_set_destroy")
            import :: c_ptr
            type(c_ptr), value :: set
        end subroutine
        function nlh_device_set_size(set) bind(C, name="nlh_device_set_size") result(n)
            import :: c_ptr, c_int32_t
            type(c_ptr), value :: set
            integer(c_int32_t) :: n
        end function
        function nlh_device_count() bind(C, name="nlh_device_count") result(n)
            import :: c_int
            integer(c_int) :: n
        end function
        function nlh_dq_model_create_on(set, nprob, m, n, a, b, gamma, model) bind(C, name="nlh_dq_model_create_on") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: set
            integer(c_int32_t), value :: nprob, m, n
            real(c_double), intent(in) :: a(*), b(*)
            real(c_double), value :: gamma
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        subroutine nlh_dq_model_destroy(model) bind(C, name="nlh_dq_model_destroy")
            import :: c_ptr
            type(c_ptr), value :: model
        end subroutine
        function nlh_dq_model_eval(h, model, x, f) bind(C, name="nlh_dq_model_eval") result(rc)
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h, model
            real(c_double), intent(in) :: x(*)
            real(c_double), intent(out) :: f(*)
            integer(c_int) :: rc
        end function
        function nlh_dq_model_lm_solve(h, opts, model, x, fvec, ib, status) bind(C, name="nlh_dq_model_lm_solve") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h, model
            type(nlh_options), intent(in) :: opts
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*)
            type(nlh_iteration_behavior), intent(out) :: ib(*)
            integer(c_int32_t), intent(out) :: status(*)
            integer(c_int) :: rc
        end function
        function nlh_lm_covariance(h, m, n, fcn, jacfcn, ctx, x, scaled, tol, cov, sigma, rank, chi2) &
                bind(C, name="nlh_lm_covariance") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h
            integer(c_int32_t), value :: m, n
            type(c_funptr), value :: fcn, jacfcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*)
            integer(c_int32_t), value :: scaled
            real(c_double), value :: tol
            real(c_double), intent(out) :: cov(*), sigma(*), chi2(*)
            integer(c_int32_t), intent(out) :: rank(*)
            integer(c_int) :: rc
        end function
        function nlh_dq_model_lm_covariance(h, model, x, scaled, tol, cov, sigma, rank, chi2) &
                bind(C, name="nlh_dq_model_lm_covariance") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: h, model
            real(c_double), intent(in) :: x(*)
            integer(c_int32_t), value :: scaled
            real(c_double), value :: tol
            real(c_double), intent(out) :: cov(*), sigma(*), chi2(*)
            integer(c_int32_t), intent(out) :: rank(*)
            integer(c_int) :: rc
        end function
        function nlh_dq_model_propagate(h, model, x, cov, noise, val, sd) &
                bind(C, name="nlh_dq_model_propagate") result(rc)
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: h, model
            real(c_double), intent(in) :: x(*), cov(*)
            type(c_ptr), value :: noise, val                 ! real(c_double) arrays, or c_null_ptr: none
            real(c_double), intent(out) :: sd(*)
            integer(c_int) :: rc
        end function
        function nlh_dq_model_newton_solve(h, opts, model, analytic, x, fvec, ib, status) &
                bind(C, name="nlh_dq_model_newton_solve") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h, model
            type(nlh_options), intent(in) :: opts
            integer(c_int32_t), value :: analytic
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*)
            type(nlh_iteration_behavior), intent(out) :: ib(*)
            integer(c_int32_t), intent(out) :: status(*)
            integer(c_int) :: rc
        end function
        function nlh_dq_model_quasi_newton_solve(h, opts, model, jdelta, analytic, x, fvec, ib, status) &
                bind(C, name="nlh_dq_model_quasi_newton_solve") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h, model
            type(nlh_options), intent(in) :: opts
            integer(c_int32_t), value :: jdelta, analytic
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*)
            type(nlh_iteration_behavior), intent(out) :: ib(*)
            integer(c_int32_t), intent(out) :: status(*)
            integer(c_int) :: rc
        end function
        function nlh_dq_model_cls_solve(h, opts, model, delta0, stepscale0, xl, xu, x, fvec, ib, status) &
                bind(C, name="nlh_dq_model_cls_solve") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h, model
            type(nlh_options), intent(in) :: opts
            real(c_double), value :: delta0, stepscale0
            real(c_double), intent(in) :: xl(*), xu(*)
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*)
            type(nlh_iteration_behavior), intent(out) :: ib(*)
            integer(c_int32_t), intent(out) :: status(*)
            integer(c_int) :: rc
        end function
        function nlh_nelder_mead_solve(h, opts, init_size, n, fcn, ctx, x, simplex, use_simplex, fout, ib) &
                bind(C, name="nlh_nelder_mead_solve") result(rc)
            import :: c_ptr, c_funptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            real(c_double), value :: init_size
            integer(c_int32_t), value :: n
            type(c_funptr), value :: fcn
            type(c_ptr), value :: ctx
            real(c_double), intent(inout) :: x(*), simplex(*)
            integer(c_int32_t), value :: use_simplex
            real(c_double), intent(out) :: fout
            type(nlh_iteration_behavior), intent(out) :: ib
            integer(c_int) :: rc
        end function
        function nlh_brent_solve(h, opts, fcn, ctx, x1, x2, x, f, ib) bind(C, name="nlh_brent_solve") result(rc)
            import :: c_ptr, c_funptr, c_int, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            type(c_funptr), value :: fcn
            type(c_ptr), value :: ctx
            real(c_double), value :: x1, x2
            real(c_double), intent(inout) :: x
            real(c_double), intent(out) :: f
            type(nlh_iteration_behavior), intent(out) :: ib
            integer(c_int) :: rc
        end function
        function nlh_newton_1var_solve(h, opts, fcn, diff, ctx, x1, x2, x, f, ib) &
                bind(C, name="nlh_newton_1var_solve") result(rc)
            import :: c_ptr, c_funptr, c_int, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h
            type(nlh_options), intent(in) :: opts
            type(c_funptr), value :: fcn, diff
            type(c_ptr), value :: ctx
            real(c_double), value :: x1, x2
            real(c_double), intent(inout) :: x
            type(c_ptr), value :: f
            type(nlh_iteration_behavior), intent(out) :: ib
            integer(c_int) :: rc
        end function
        function nlh_dq_model_brent_solve(h, opts, model, lim, x, fout, ib, status) &
                bind(C, name="nlh_dq_model_brent_solve") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h, model
            type(nlh_options), intent(in) :: opts
            real(c_double), intent(in) :: lim(*)
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fout(*)
            type(nlh_iteration_behavior), intent(out) :: ib(*)
            integer(c_int32_t), intent(out) :: status(*)
            integer(c_int) :: rc
        end function
        function nlh_dq_model_newton_1var_solve(h, opts, model, lim, x, fout, ib, status) &
                bind(C, name="nlh_dq_model_newton_1var_solve") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h, model
            type(nlh_options), intent(in) :: opts
            real(c_double), intent(in) :: lim(*)
            real(c_double), intent(inout) :: x(*)
            type(c_ptr), value :: fout
            type(nlh_iteration_behavior), intent(out) :: ib(*)
            integer(c_int32_t), intent(out) :: status(*)
            integer(c_int) :: rc
        end function
        function nlh_fd_derivative(fcn, diff, ctx, x, fv, df) bind(C, name="nlh_fd_derivative") result(rc)
            import :: c_ptr, c_funptr, c_int, c_double
            type(c_funptr), value :: fcn, diff
            type(c_ptr), value :: ctx
            real(c_double), value :: x
            type(c_ptr), value :: fv
            real(c_double), intent(out) :: df
            integer(c_int) :: rc
        end function
        function nlh_dq_model_nelder_mead_solve(h, opts, init_size, model, x, fout, ib, status) &
                bind(C, name="nlh_dq_model_nelder_mead_solve") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h, model
            type(nlh_options), intent(in) :: opts
            real(c_double), value :: init_size
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fout(*)
            type(nlh_iteration_behavior), intent(out) :: ib(*)
            integer(c_int32_t), intent(out) :: status(*)
            integer(c_int) :: rc
        end function
        function nlh_dq_model_bfgs_solve(h, opts, model, x, fvec, fout, ib, status) &
                bind(C, name="nlh_dq_model_bfgs_solve") result(rc)
            import :: c_ptr, c_int, c_int32_t, c_double, nlh_options, nlh_iteration_behavior
            type(c_ptr), value :: h, model
            type(nlh_options), intent(in) :: opts
            real(c_double), intent(inout) :: x(*)
            real(c_double), intent(out) :: fvec(*), fout(*)
            type(nlh_iteration_behavior), intent(out) :: ib(*)
            integer(c_int32_t), intent(out) :: status(*)
            integer(c_int) :: rc
        end function
    end interface

    type(c_ptr), save, private :: default_handle = c_null_ptr
    type(c_ptr), save, private :: default_set = c_null_ptr
    logical, save, private :: default_set_decided = .false.

contains
    !> Extension: the GPUs that device_model_batch%create deals a batch over (solve_batch then runs one host thread
    !> per GPU inside this process).  devices = device ids, 0-based; an empty list selects every visible GPU.  Without
    !> this call the environment variable NLH_DEVICES decides ("all", or a comma-separated id list); unset: one GPU
    !> (device 0, the default handle).  Models created earlier keep the devices they were created on: the previous set is
    !> released here, and the library keeps its handles alive until the last model dealt over it has been destroyed.
    subroutine nlh_use_devices(devices)
        integer(c_int32_t), intent(in), dimension(:) :: devices
        integer(c_int) :: rc
        integer(c_int32_t) :: none(1)
        none = 0
        if (c_associated(default_set)) then
            call nlh_device_set_destroy(default_set)
            default_set = c_null_ptr
        end if
        if (size(devices) > 0) then
            rc = nlh_device_set_create(default_set, devices, int(size(devices), c_int32_t))
        else
            rc = nlh_device_set_create(default_set, none, 0_c_int32_t)
        end if
        if (rc /= 0) then
            print '(A,I0,A)', "nonlin_hip: nlh_device_set_create returned ", rc, " (no such HIP device?)"
            error stop 1
        end if
        default_set_decided = .true.
    end subroutine

    !> The device set models are dealt over, or c_null_ptr when a single GPU (the default handle) is in use.
    function nlh_default_device_set() result(set)
        type(c_ptr) :: set
        character(len=256) :: spec
        integer :: length, stat, i, k, cnt
        integer(c_int32_t) :: ids(64)
        if (.not.default_set_decided) then
            default_set_decided = .true.
            call get_environment_variable("NLH_DEVICES", spec, length, stat)
            if (stat == 0 .and. length > 0) then
                cnt = 0
                if (spec(1:length) /= "all") then
                    k = 1
                    do i = 1, length + 1
                        if (i > length .or. spec(i:min(i, length)) == ",") then
                            if (i > k) then
                                if (cnt >= size(ids)) then
                                    print '(A,I0,A)', "nonlin_hip: NLH_DEVICES lists more than ", size(ids), " devices"
                                    error stop 1
                                end if
                                cnt = cnt + 1
                                read (spec(k:i - 1), *, iostat = stat) ids(cnt)
                                if (stat /= 0 .or. verify(trim(adjustl(spec(k:i - 1))), "0123456789") /= 0) then
                                    print '(3A)', "nonlin_hip: NLH_DEVICES must be 'all' or a comma-separated list of device ids, got '", &
                                        spec(1:length), "'"
                                    error stop 1
                                end if
                            else if (i <= length .or. k > 1) then      ! an empty entry ("0,,1", a trailing comma)
                                print '(3A)', "nonlin_hip: NLH_DEVICES has an empty entry: '", spec(1:length), "'"
                                error stop 1
                            end if
                            k = i + 1
                        end if
                    end do
                end if
                call nlh_use_devices(ids(1:cnt))
            end if
        end if
        set = default_set
    end function

    !> Lazily created process-wide handle on device 0, default stream.
    function nlh_default_handle() result(h)
        type(c_ptr) :: h
        integer(c_int) :: rc
        if (.not.c_associated(default_handle)) then
            rc = nlh_create(default_handle, 0_c_int32_t, c_null_ptr)
            if (rc /= 0) then
                print '(A,I0)', "nonlin_hip: no usable HIP device (nlh_create returned ", rc
                error stop 1
            end if
        end if
        h = default_handle
    end function
end module
