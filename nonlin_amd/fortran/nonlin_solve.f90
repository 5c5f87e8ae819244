! line_search_solver, newton_solver and quasi_newton_solver: the public types and bindings of
! src/nonlin_solve.f90:20-67.  `solve` marshals to nlh_newton_solve / nlh_dq_model_newton_solve (ns_solve on
! the GPU, :452-638) and nlh_quasi_newton_solve (qns_solve, :156-427); the line search the solver owns is only
! a parameter record here (nonlin_linesearch), the search runs behind the C ABI.  brent_solver and newton_1var_solver
! (:69-86) marshal to nlh_brent_solve / nlh_newton_1var_solve (brent_solve :643-835, newt1var_solve :840-1032: the
! solver's statements on the device, the user's function on this thread through the nonlin_single_var trampolines).
module nonlin_solve
    use iso_fortran_env
    use, intrinsic :: iso_c_binding
    use nonlin_error_handling
    use nonlin_multi_eqn_mult_var
    use nonlin_linesearch
    use nonlin_types
    use nonlin_hip_c
    use nonlin_shim_support
    use nonlin_single_var
    implicit none
    private
    public :: line_search_solver
    public :: newton_solver
    public :: quasi_newton_solver
    public :: brent_solver
    public :: newton_1var_solver

    type, abstract, extends(equation_solver) :: line_search_solver
        class(line_search), private, allocatable :: search_
        logical, private :: search_on_ = .true.
    contains
        procedure, public :: get_line_search => lsx_copy_search
        procedure, public :: set_line_search => lsx_put_search
        procedure, public :: set_default_line_search => lsx_default_search
        procedure, public :: is_line_search_defined => lsx_has_search
        procedure, public :: get_use_line_search => lsx_enabled
        procedure, public :: set_use_line_search => lsx_enable
        procedure, public :: export_search_options => lsx_export
    end type

    type, extends(line_search_solver) :: newton_solver
    contains
        procedure, public :: solve => newton_solve_one
        procedure, public :: solve_batch => newton_solve_many
    end type

    type, extends(line_search_solver) :: quasi_newton_solver
        integer(int32), private :: refresh_every_ = 5    ! iterations between fresh Jacobians (reference default, :51)
    contains
        procedure, public :: solve => broyden_solve_one
        procedure, public :: solve_batch => broyden_solve_many
        procedure, public :: get_jacobian_interval => broyden_refresh
        procedure, public :: set_jacobian_interval => broyden_put_refresh
    end type


    type, extends(equation_solver_1var) :: brent_solver
    contains
        procedure, public :: solve => brent_solve_one
        procedure, public :: solve_batch => brent_solve_many
    end type

    type, extends(equation_solver_1var) :: newton_1var_solver
    contains
        procedure, public :: solve => newt1var_solve_one
        procedure, public :: solve_batch => newt1var_solve_many
    end type

contains
    ! ---- line_search_solver -------------------------------------------------------------------------------------
    pure logical function lsx_has_search(this)
        class(line_search_solver), intent(in) :: this
        lsx_has_search = allocated(this%search_)
    end function

    !> ls = a copy of the solver's search object; left unallocated while none has been set.
    subroutine lsx_copy_search(this, ls)
        class(line_search_solver), intent(in) :: this
        class(line_search), intent(out), allocatable :: ls
        if (this%is_line_search_defined()) allocate(ls, source = this%search_)
    end subroutine

    subroutine lsx_put_search(this, ls)
        class(line_search_solver), intent(inout) :: this
        class(line_search), intent(in) :: ls
        if (this%is_line_search_defined()) deallocate(this%search_)
        allocate(this%search_, source = ls)
    end subroutine

    subroutine lsx_default_search(this)
        class(line_search_solver), intent(inout) :: this
        call this%set_line_search(line_search())
    end subroutine

    pure logical function lsx_enabled(this)
        class(line_search_solver), intent(in) :: this
        lsx_enabled = this%search_on_
    end function

    subroutine lsx_enable(this, x)
        class(line_search_solver), intent(inout) :: this
        logical, intent(in) :: x
        this%search_on_ = x
    end subroutine

    !> Extension: export_options plus the search settings.  As in the reference (:511-515, :233-237) a solver that
    !> searches but has no search object yet gets the default one, and keeps it.
    subroutine lsx_export(this, opts, quiet)
        class(line_search_solver), intent(inout) :: this
        type(nlh_options), intent(out) :: opts
        logical, intent(in), optional :: quiet
        call this%export_options(opts, quiet)
        opts%use_line_search = merge(1, 0, this%search_on_)
        if (.not.this%search_on_) return
        if (.not.this%is_line_search_defined()) call this%set_default_line_search()
        opts%ls_max_evals = this%search_%get_max_fcn_evals()
        opts%ls_alpha = this%search_%get_scaling_factor()
        opts%ls_factor = this%search_%get_distance_factor()
    end subroutine

    !> Checks every square-system solve makes before it crosses the boundary (:518-525, :240-247).
    subroutine require_square_system(fcn, nx, nf)
        class(vecfcn_helper), intent(in) :: fcn
        integer(int32), intent(in) :: nx, nf
        if (.not.fcn%is_fcn_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        if (fcn%get_variable_count() /= fcn%get_equation_count()) error stop NL_INVALID_INPUT_ERROR
        call require_vector_sizes(nx, nf, fcn%get_variable_count(), fcn%get_equation_count())
    end subroutine

    ! ---- newton_solver -----------------------------------------------------------------------------------------
    subroutine newton_solve_one(this, fcn, x, fvec, ib, args)
        class(newton_solver), intent(inout) :: this
        class(vecfcn_helper), intent(in), target :: fcn
        real(real64), intent(inout), dimension(:) :: x
        real(real64), intent(out), dimension(:) :: fvec
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional, target :: args

        type(nlh_options) :: opts
        type(nlh_iteration_behavior) :: counters(1)
        type(nlh_callback_ctx), target :: ctx
        type(device_model_batch) :: onchip
        type(c_funptr) :: jac_entry
        real(c_double), allocatable :: xwork(:), fwork(:)
        integer(c_int32_t) :: outcome(1)
        integer(c_int) :: rc
        integer(int32) :: n

        n = fcn%get_variable_count()
        if (present(ib)) call behavior_clear(ib)
        call this%export_search_options(opts)
        call require_square_system(fcn, size(x), size(fvec))
        allocate(xwork(n), source = x)
        allocate(fwork(n))
        if (fcn%is_device_model_defined()) then
            ! residuals, Jacobian (the model's own when it was bound with analytic = .true., forward differences
            ! otherwise) and the LU solve on the GPU, no host callback
            onchip = fcn%device_model()
            rc = nlh_dq_model_newton_solve(nlh_default_handle(), opts, onchip%c_handle(), &
                merge(1_c_int32_t, 0_c_int32_t, onchip%uses_analytic_jacobian()), xwork, fwork, counters, outcome)
            if (rc == 0) rc = outcome(1)
        else
            ctx%helper => fcn
            if (present(args)) ctx%args => args
            jac_entry = c_null_funptr
            if (fcn%is_jacobian_defined()) jac_entry = c_funloc(nlh_jacfcn_trampoline)
            rc = nlh_newton_solve(nlh_default_handle(), opts, n, c_funloc(nlh_vecfcn_trampoline), jac_entry, &
                c_loc(ctx), xwork, fwork, counters(1))
        end if
        x = xwork
        fvec = fwork
        if (present(ib)) call behavior_import(ib, counters(1))
        if (rc /= 0) error stop rc      ! the reference's stops at :604-608, :635-637 and inside the line search
    end subroutine

    !> Extension: newton_solver%solve (ns_solve, :452-638) for every (square) problem of a device model batch.
    !> Arguments as least_squares_solver%solve_batch.
    subroutine newton_solve_many(this, model, x, fvec, ib, status)
        class(newton_solver), intent(inout) :: this
        class(device_model_batch), intent(in) :: model
        real(real64), intent(inout), dimension(:,:) :: x
        real(real64), intent(out), dimension(:,:) :: fvec
        type(iteration_behavior), intent(out), dimension(:), optional :: ib
        integer(int32), intent(out), dimension(:), optional :: status

        type(nlh_options) :: opts
        type(nlh_iteration_behavior), allocatable :: counters(:)
        integer(c_int32_t), allocatable :: outcome(:)
        real(c_double), allocatable :: xwork(:,:), fwork(:,:)
        integer(c_int) :: rc
        integer(int32) :: n, count

        if (.not.model%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        n = model%get_variable_count()
        count = model%get_problem_count()
        if (model%get_equation_count() /= n) error stop NL_INVALID_INPUT_ERROR
        if (any(shape(x) /= [n, count])) error stop 3
        if (any(shape(fvec) /= [n, count])) error stop 4
        call this%export_search_options(opts, quiet = .true.)
        allocate(counters(count), outcome(count), fwork(n, count))
        allocate(xwork(n, count), source = x)
        rc = nlh_dq_model_newton_solve(nlh_default_handle(), opts, model%c_handle(), &
            merge(1_c_int32_t, 0_c_int32_t, model%uses_analytic_jacobian()), xwork, fwork, counters, outcome)
        if (rc /= 0) error stop rc
        x = xwork
        fvec = fwork
        if (present(status)) status = outcome
        if (present(ib)) call behavior_import(ib, counters)
    end subroutine

    ! ---- quasi_newton_solver -----------------------------------------------------------------------------------
    !> Extension: quasi_newton_solver%solve (qns_solve, :156-427) for every (square) problem of a device model batch.
    !> Arguments as least_squares_solver%solve_batch.
    subroutine broyden_solve_many(this, model, x, fvec, ib, status)
        class(quasi_newton_solver), intent(inout) :: this
        class(device_model_batch), intent(in) :: model
        real(real64), intent(inout), dimension(:,:) :: x
        real(real64), intent(out), dimension(:,:) :: fvec
        type(iteration_behavior), intent(out), dimension(:), optional :: ib
        integer(int32), intent(out), dimension(:), optional :: status

        type(nlh_options) :: opts
        type(nlh_iteration_behavior), allocatable :: counters(:)
        integer(c_int32_t), allocatable :: outcome(:)
        real(c_double), allocatable :: xwork(:,:), fwork(:,:)
        integer(c_int) :: rc
        integer(int32) :: n, count

        if (.not.model%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        n = model%get_variable_count()
        count = model%get_problem_count()
        if (model%get_equation_count() /= n) error stop NL_INVALID_INPUT_ERROR
        if (any(shape(x) /= [n, count])) error stop 3
        if (any(shape(fvec) /= [n, count])) error stop 4
        call this%export_search_options(opts, quiet = .true.)
        allocate(counters(count), outcome(count), fwork(n, count))
        allocate(xwork(n, count), source = x)
        rc = nlh_dq_model_quasi_newton_solve(nlh_default_handle(), opts, model%c_handle(), this%refresh_every_, &
            merge(1_c_int32_t, 0_c_int32_t, model%uses_analytic_jacobian()), xwork, fwork, counters, outcome)
        if (rc /= 0) error stop rc
        x = xwork
        fvec = fwork
        if (present(status)) status = outcome
        if (present(ib)) call behavior_import(ib, counters)
    end subroutine

    subroutine broyden_solve_one(this, fcn, x, fvec, ib, args)
        class(quasi_newton_solver), intent(inout) :: this
        class(vecfcn_helper), intent(in), target :: fcn
        real(real64), intent(inout), dimension(:) :: x
        real(real64), intent(out), dimension(:) :: fvec
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional, target :: args

        type(nlh_options) :: opts
        type(nlh_iteration_behavior) :: counters
        type(nlh_callback_ctx), target :: ctx
        type(c_funptr) :: jac_entry
        real(c_double), allocatable :: xwork(:), fwork(:)
        integer(c_int) :: rc
        integer(int32) :: n

        n = fcn%get_variable_count()
        if (present(ib)) call behavior_clear(ib)
        call this%export_search_options(opts)
        call require_square_system(fcn, size(x), size(fvec))
        allocate(xwork(n), source = x)
        allocate(fwork(n))
        if (fcn%is_device_model_defined()) then
            ! a device residual (set_device_model / set_device_fcn): Broyden's iteration entirely on the GPU
            block
                type(device_model_batch) :: onchip
                type(nlh_iteration_behavior) :: c1(1)
                integer(c_int32_t) :: outcome(1)
                onchip = fcn%device_model()
                rc = nlh_dq_model_quasi_newton_solve(nlh_default_handle(), opts, onchip%c_handle(), this%refresh_every_, &
                    merge(1_c_int32_t, 0_c_int32_t, onchip%uses_analytic_jacobian()), xwork, fwork, c1, outcome)
                if (rc == 0) rc = outcome(1)
                counters = c1(1)
            end block
        else
            ctx%helper => fcn
            if (present(args)) ctx%args => args
            jac_entry = c_null_funptr
            if (fcn%is_jacobian_defined()) jac_entry = c_funloc(nlh_jacfcn_trampoline)
            rc = nlh_quasi_newton_solve(nlh_default_handle(), opts, this%refresh_every_, n, &
                c_funloc(nlh_vecfcn_trampoline), jac_entry, c_loc(ctx), xwork, fwork, counters)
        end if
        x = xwork
        fvec = fwork
        if (present(ib)) call behavior_import(ib, counters)
        if (rc /= 0) error stop rc      ! the reference's stops at :376, :425-427 and inside the line search
    end subroutine

    pure integer(int32) function broyden_refresh(this)
        class(quasi_newton_solver), intent(in) :: this
        broyden_refresh = this%refresh_every_
    end function

    subroutine broyden_put_refresh(this, n)
        class(quasi_newton_solver), intent(inout) :: this
        integer(int32), intent(in) :: n
        this%refresh_every_ = n
    end subroutine
    ! ---- equations of one variable ----------------------------------------------------------------------------
    function es1_options(this) result(opts)
        class(equation_solver_1var), intent(in) :: this
        type(nlh_options) :: opts
        call nlh_default_options(opts)
        opts%max_evals = this%get_max_fcn_evals()
        opts%ftol = this%get_fcn_tolerance()
        opts%xtol = this%get_var_tolerance()
        opts%gtol = this%get_diff_tolerance()
        opts%print_status = merge(1, 0, this%get_print_status())
    end function

    !> brent_solve (:643-835).  x = 0 unless the solve converged (:691, :746, :751); a failing solve error-stops with its
    !> code after x, f and ib are stored.  The binding has the reference's dummies (nonlin_solver_1var); the work is done
    !> by brent_solve_c, whose TARGET dummies the trampolines' context points at for the length of the call.
    subroutine brent_solve_one(this, fcn, x, lim, f, ib, args)
        class(brent_solver), intent(inout) :: this
        class(fcn1var_helper), intent(in) :: fcn
        real(real64), intent(inout) :: x
        type(value_pair), intent(in) :: lim
        real(real64), intent(out), optional :: f
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional :: args
        call brent_solve_c(this, fcn, x, lim, f, ib, args)
    end subroutine

    subroutine brent_solve_c(this, fcn, x, lim, f, ib, args)
        class(brent_solver), intent(inout) :: this
        class(fcn1var_helper), intent(in), target :: fcn
        real(real64), intent(inout) :: x
        type(value_pair), intent(in) :: lim
        real(real64), intent(out), optional :: f
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional, target :: args
        type(nlh_iteration_behavior) :: counters
        type(nlh_scalar1_ctx), target :: ctx
        real(c_double) :: xv, fv
        integer(c_int) :: rc
        x = 0.0d0                                                                  ! :691
        if (present(f)) f = 0.0d0                                                  ! :700
        if (present(ib)) call behavior_clear(ib)                                   ! :701-709
        if (.not.fcn%is_fcn_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR    ! :712
        ctx%helper => fcn
        if (present(args)) ctx%args => args
        xv = 0.0d0
        rc = nlh_brent_solve(nlh_default_handle(), es1_options(this), c_funloc(nlh_fcn1var_trampoline), c_loc(ctx), &
            lim%x1, lim%x2, xv, fv, counters)
        if (rc < 0) error stop rc
        x = xv
        if (present(f)) f = fv                                                     ! :820
        if (present(ib)) call behavior_import(ib, counters)
        if (rc /= 0) error stop rc                                                 ! :713, :832-834
    end subroutine

    !> newt1var_solve (:840-1032); f present: one more evaluation after the loop, its value discarded (:1011-1017).
    !> The reference's dummies; the work is done by newt1var_solve_c (TARGET dummies, as brent_solve_c).
    subroutine newt1var_solve_one(this, fcn, x, lim, f, ib, args)
        class(newton_1var_solver), intent(inout) :: this
        class(fcn1var_helper), intent(in) :: fcn
        real(real64), intent(inout) :: x
        type(value_pair), intent(in) :: lim
        real(real64), intent(out), optional :: f
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional :: args
        call newt1var_solve_c(this, fcn, x, lim, f, ib, args)
    end subroutine

    subroutine newt1var_solve_c(this, fcn, x, lim, f, ib, args)
        class(newton_1var_solver), intent(inout) :: this
        class(fcn1var_helper), intent(in), target :: fcn
        real(real64), intent(inout) :: x
        type(value_pair), intent(in) :: lim
        real(real64), intent(out), optional :: f
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional, target :: args
        type(nlh_iteration_behavior) :: counters
        type(nlh_scalar1_ctx), target :: ctx
        type(c_funptr) :: diff_entry
        type(c_ptr) :: f_entry
        real(c_double), target :: fv
        real(c_double) :: xv
        integer(c_int) :: rc
        if (present(f)) f = 0.0d0                                                  ! :883
        if (present(ib)) call behavior_clear(ib)                                   ! :884-892
        if (.not.fcn%is_fcn_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR    ! :898
        ctx%helper => fcn
        if (present(args)) ctx%args => args
        diff_entry = c_null_funptr
        if (fcn%is_derivative_defined()) diff_entry = c_funloc(nlh_diff1var_trampoline)
        f_entry = c_null_ptr
        if (present(f)) f_entry = c_loc(fv)
        xv = x
        rc = nlh_newton_1var_solve(nlh_default_handle(), es1_options(this), c_funloc(nlh_fcn1var_trampoline), diff_entry, &
            c_loc(ctx), lim%x1, lim%x2, xv, f_entry, counters)
        if (rc < 0) error stop rc
        x = xv
        if (present(f)) f = fv                                                     ! :1017
        if (present(ib)) call behavior_import(ib, counters)
        if (rc /= 0) error stop rc                                                 ! :899, :1027-1029
    end subroutine

    !> Extension: brent_solver%solve on every problem of a batch created from the user's own device function of one
    !> equation in one unknown (device_model_batch%create_from_device_fcn with nfcn = nvar = 1): lim(count), x(count),
    !> f(count), status(count): the code each solve would have stopped with (0: converged).
    subroutine brent_solve_many(this, model, lim, x, f, ib, status)
        class(brent_solver), intent(inout) :: this
        class(device_model_batch), intent(in) :: model
        type(value_pair), intent(in), dimension(:) :: lim
        real(real64), intent(inout), dimension(:) :: x
        real(real64), intent(out), dimension(:), optional :: f
        type(iteration_behavior), intent(out), dimension(:), optional :: ib
        integer(int32), intent(out), dimension(:), optional :: status
        call root1v_many(es1_options(this), 0, model, lim, x, f, ib, status)
    end subroutine

    !> Extension: newton_1var_solver%solve on every problem of such a batch (the model's Jacobian launcher, if any, is the
    !> derivative; forward differences otherwise).  f present: the final evaluation of :1011-1014 is made.
    subroutine newt1var_solve_many(this, model, lim, x, f, ib, status)
        class(newton_1var_solver), intent(inout) :: this
        class(device_model_batch), intent(in) :: model
        type(value_pair), intent(in), dimension(:) :: lim
        real(real64), intent(inout), dimension(:) :: x
        real(real64), intent(out), dimension(:), optional :: f
        type(iteration_behavior), intent(out), dimension(:), optional :: ib
        integer(int32), intent(out), dimension(:), optional :: status
        call root1v_many(es1_options(this), 1, model, lim, x, f, ib, status)
    end subroutine

    subroutine root1v_many(opts, newton, model, lim, x, f, ib, status)
        type(nlh_options), intent(in) :: opts
        integer, intent(in) :: newton
        class(device_model_batch), intent(in) :: model
        type(value_pair), intent(in), dimension(:) :: lim
        real(real64), intent(inout), dimension(:) :: x
        real(real64), intent(out), dimension(:), optional :: f
        type(iteration_behavior), intent(out), dimension(:), optional :: ib
        integer(int32), intent(out), dimension(:), optional :: status
        type(nlh_iteration_behavior), allocatable :: counters(:)
        integer(c_int32_t), allocatable :: outcome(:)
        real(c_double), allocatable :: lw(:,:), xwork(:)
        real(c_double), allocatable, target :: fw(:)
        type(c_ptr) :: f_entry
        integer(c_int) :: rc
        integer(int32) :: count, k
        if (.not.model%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        count = model%get_problem_count()
        if (size(lim) /= count .or. size(x) /= count) error stop NL_INVALID_INPUT_ERROR
        allocate(counters(count), outcome(count), fw(count), lw(2, count))
        allocate(xwork(count), source = x)
        do k = 1, count
            lw(1, k) = lim(k)%x1
            lw(2, k) = lim(k)%x2
        end do
        if (newton == 0) then
            rc = nlh_dq_model_brent_solve(nlh_default_handle(), opts, model%c_handle(), lw, xwork, fw, counters, outcome)
        else
            f_entry = c_null_ptr
            if (present(f)) f_entry = c_loc(fw)
            rc = nlh_dq_model_newton_1var_solve(nlh_default_handle(), opts, model%c_handle(), lw, xwork, f_entry, counters, &
                outcome)
        end if
        if (rc /= 0) error stop rc
        x = xwork
        if (present(f)) f = fw
        if (present(status)) status = outcome
        if (present(ib)) call behavior_import(ib, counters)
    end subroutine

end module
