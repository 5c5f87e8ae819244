! nelder_mead, line_search_optimizer and bfgs: the public types and bindings of src/nonlin_optimize.f90:24-72, 400-556.
! nelder_mead%solve marshals to nlh_nelder_mead_solve (nm_solve behind the C ABI, :104-340; the simplex stays object
! state here, as m_simplex does in the reference); bfgs%solve to nlh_bfgs_solve (bfgs_solve, :557-770); the line search
! is a parameter record here.
module nonlin_optimize
    use iso_fortran_env
    use, intrinsic :: iso_c_binding
    use nonlin_linesearch
    use nonlin_error_handling
    use nonlin_multi_var
    use nonlin_multi_eqn_mult_var, only : device_model_batch
    use nonlin_types
    use nonlin_hip_c
    use nonlin_shim_support
    implicit none
    private
    public :: nelder_mead
    public :: line_search_optimizer
    public :: bfgs

    type, extends(equation_optimizer) :: nelder_mead
        real(real64), private, allocatable, dimension(:,:) :: m_simplex
        real(real64), private :: m_initSize = 1.0d0
    contains
        procedure, public :: solve => nm_solve_one
        procedure, public :: solve_batch => nm_solve_many
        procedure, public :: get_simplex => nm_get_simplex
        procedure, public :: set_simplex => nm_set_simplex
        procedure, public :: get_initial_size => nm_get_size
        procedure, public :: set_initial_size => nm_set_size
    end type

    type, abstract, extends(equation_optimizer) :: line_search_optimizer
        class(line_search), private, allocatable :: search_
        logical, private :: search_on_ = .true.
        real(real64), private :: step_tol_ = 1.0d-12         ! convergence on the change in x
    contains
        procedure, public :: get_line_search => lsopt_copy_search
        procedure, public :: set_line_search => lsopt_put_search
        procedure, public :: set_default_line_search => lsopt_default_search
        procedure, public :: is_line_search_defined => lsopt_has_search
        procedure, public :: get_use_line_search => lsopt_enabled
        procedure, public :: set_use_line_search => lsopt_enable
        procedure, public :: get_var_tolerance => lsopt_step_tol
        procedure, public :: set_var_tolerance => lsopt_put_step_tol
        procedure, public :: export_options => lsopt_export
    end type

    type, extends(line_search_optimizer) :: bfgs
    contains
        procedure, public :: solve => bfgs_solve_one
        procedure, public :: solve_batch => bfgs_solve_many
    end type

contains
    pure function nm_get_simplex(this) result(p)               ! :402-416
        class(nelder_mead), intent(in) :: this
        real(real64), allocatable, dimension(:,:) :: p
        if (allocated(this%m_simplex)) then
            allocate(p(size(this%m_simplex, 1), size(this%m_simplex, 2)))
            p = this%m_simplex
        end if
    end function

    subroutine nm_set_simplex(this, x)                         ! :419-440
        class(nelder_mead), intent(inout) :: this
        real(real64), dimension(:,:) :: x
        if (allocated(this%m_simplex)) deallocate(this%m_simplex)
        allocate(this%m_simplex(size(x, 1), size(x, 2)))
        this%m_simplex = x
    end subroutine

    pure function nm_get_size(this) result(x)                  ! :445-455
        class(nelder_mead), intent(in) :: this
        real(real64) :: x
        x = this%m_initSize
    end function

    subroutine nm_set_size(this, x)                            ! :458-468
        class(nelder_mead), intent(inout) :: this
        real(real64), intent(in) :: x
        this%m_initSize = x
    end subroutine

    !> nm_solve (:104-340): the simplex logic runs on the device, the objective on this thread through the trampoline.
    !> An m_simplex of the right shape (ndim x npts) is the start and x is ignored (:176-188); otherwise the simplex is
    !> built from x (:205-213).  Either way the final simplex is kept for the next call.
    subroutine nm_solve_one(this, fcn, x, fout, ib, args)
        class(nelder_mead), intent(inout) :: this
        class(fcnnvar_helper), intent(in), target :: fcn
        real(real64), intent(inout), dimension(:) :: x
        real(real64), intent(out), optional :: fout
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional, target :: args

        type(nlh_options) :: opts
        type(nlh_iteration_behavior) :: counters
        type(nlh_scalar_ctx), target :: ctx
        real(c_double), allocatable :: xwork(:)
        real(c_double) :: fmin
        integer(c_int) :: rc
        integer(c_int32_t) :: use_simplex
        integer(int32) :: n

        n = fcn%get_variable_count()
        if (present(ib)) call behavior_clear(ib)                                   ! :159-167
        if (.not.fcn%is_fcn_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR    ! :170
        if (size(x) /= n) error stop NL_INVALID_INPUT_ERROR                      ! :171
        use_simplex = 0
        if (allocated(this%m_simplex)) then                                        ! :176-188
            if (size(this%m_simplex, 1) == n .and. size(this%m_simplex, 2) == n + 1) then
                use_simplex = 1
            else
                deallocate(this%m_simplex)
            end if
        end if
        if (.not.allocated(this%m_simplex)) allocate(this%m_simplex(n, n + 1))
        call nlh_default_options(opts)
        opts%max_evals = this%get_max_fcn_evals()
        opts%gtol = this%get_tolerance()
        opts%print_status = merge(1, 0, this%get_print_status())
        ctx%helper => fcn
        if (present(args)) ctx%args => args
        allocate(xwork(n), source = x)
        rc = nlh_nelder_mead_solve(nlh_default_handle(), opts, this%m_initSize, n, c_funloc(nlh_fcnnvar_trampoline), &
            c_loc(ctx), xwork, this%m_simplex, use_simplex, fmin, counters)
        if (rc < 0) error stop rc
        x = xwork
        if (present(fout)) fout = fmin                                             ! :333
        if (present(ib)) call behavior_import(ib, counters)                        ! :322-330
        if (rc /= 0) error stop rc                                                 ! :335-337
    end subroutine

    !> Extension: nelder_mead%solve on every problem of a batch created from the user's own device function with ONE
    !> function per problem (device_model_batch%create_from_device_fcn, nfcn = 1): the launcher is the user's fcnnvar.
    !> Each problem's simplex is built from its column of x(n, count) with get_initial_size() (the object's simplex is
    !> neither read nor changed).  fout(count), status(count): the code each solve would have stopped with (0: converged).
    subroutine nm_solve_many(this, model, x, fout, ib, status)
        class(nelder_mead), intent(inout) :: this
        class(device_model_batch), intent(in) :: model
        real(real64), intent(inout), dimension(:,:) :: x
        real(real64), intent(out), dimension(:), optional :: fout
        type(iteration_behavior), intent(out), dimension(:), optional :: ib
        integer(int32), intent(out), dimension(:), optional :: status

        type(nlh_options) :: opts
        type(nlh_iteration_behavior), allocatable :: counters(:)
        integer(c_int32_t), allocatable :: outcome(:)
        real(c_double), allocatable :: xwork(:,:), fmin(:)
        integer(c_int) :: rc
        integer(int32) :: n, count

        if (.not.model%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        n = model%get_variable_count()
        count = model%get_problem_count()
        if (any(shape(x) /= [n, count])) error stop NL_INVALID_INPUT_ERROR
        call nlh_default_options(opts)
        opts%max_evals = this%get_max_fcn_evals()
        opts%gtol = this%get_tolerance()
        allocate(counters(count), outcome(count), fmin(count))
        allocate(xwork(n, count), source = x)
        rc = nlh_dq_model_nelder_mead_solve(nlh_default_handle(), opts, this%m_initSize, model%c_handle(), xwork, fmin, &
            counters, outcome)
        if (rc /= 0) error stop rc
        x = xwork
        if (present(fout)) fout = fmin
        if (present(status)) status = outcome
        if (present(ib)) call behavior_import(ib, counters)
    end subroutine

    pure logical function lsopt_has_search(this)
        class(line_search_optimizer), intent(in) :: this
        lsopt_has_search = allocated(this%search_)
    end function

    !> ls = a copy of the optimizer's search object; left unallocated while none has been set.
    subroutine lsopt_copy_search(this, ls)
        class(line_search_optimizer), intent(in) :: this
        class(line_search), intent(out), allocatable :: ls
        if (this%is_line_search_defined()) allocate(ls, source = this%search_)
    end subroutine

    subroutine lsopt_put_search(this, ls)
        class(line_search_optimizer), intent(inout) :: this
        class(line_search), intent(in) :: ls
        if (this%is_line_search_defined()) deallocate(this%search_)
        allocate(this%search_, source = ls)
    end subroutine

    subroutine lsopt_default_search(this)
        class(line_search_optimizer), intent(inout) :: this
        call this%set_line_search(line_search())
    end subroutine

    pure logical function lsopt_enabled(this)
        class(line_search_optimizer), intent(in) :: this
        lsopt_enabled = this%search_on_
    end function

    subroutine lsopt_enable(this, x)
        class(line_search_optimizer), intent(inout) :: this
        logical, intent(in) :: x
        this%search_on_ = x
    end subroutine

    pure real(real64) function lsopt_step_tol(this)
        class(line_search_optimizer), intent(in) :: this
        lsopt_step_tol = this%step_tol_
    end function

    subroutine lsopt_put_step_tol(this, x)
        class(line_search_optimizer), intent(inout) :: this
        real(real64), intent(in) :: x
        this%step_tol_ = x
    end subroutine

    !> Extension: this optimizer's settings as the C ABI's option record.  As in the reference (:603-608) an
    !> optimizer that searches but has no search object yet gets the default one, and keeps it.
    subroutine lsopt_export(this, opts)
        class(line_search_optimizer), intent(inout) :: this
        type(nlh_options), intent(out) :: opts
        call nlh_default_options(opts)
        opts%max_evals = this%get_max_fcn_evals()
        opts%gtol = this%get_tolerance()
        opts%xtol = this%step_tol_
        opts%print_status = merge(1, 0, this%get_print_status())
        opts%use_line_search = merge(1, 0, this%search_on_)
        if (.not.this%search_on_) return
        if (.not.this%is_line_search_defined()) call this%set_default_line_search()
        opts%ls_max_evals = this%search_%get_max_fcn_evals()
        opts%ls_alpha = this%search_%get_scaling_factor()
        opts%ls_factor = this%search_%get_distance_factor()
    end subroutine

    subroutine bfgs_solve_one(this, fcn, x, fout, ib, args)
        class(bfgs), intent(inout) :: this
        class(fcnnvar_helper), intent(in), target :: fcn
        real(real64), intent(inout), dimension(:) :: x
        real(real64), intent(out), optional :: fout
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional, target :: args

        type(nlh_options) :: opts
        type(nlh_iteration_behavior) :: counters
        type(nlh_scalar_ctx), target :: ctx
        type(c_funptr) :: grad_entry
        real(c_double), allocatable :: xwork(:)
        real(c_double) :: fmin
        integer(c_int) :: rc
        integer(int32) :: n

        n = fcn%get_variable_count()
        if (present(ib)) call behavior_clear(ib)
        call this%export_options(opts)
        if (.not.fcn%is_fcn_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR    ! reference :614
        if (size(x) /= n) error stop NL_INVALID_INPUT_ERROR                      ! reference :615
        ctx%helper => fcn
        if (present(args)) ctx%args => args
        grad_entry = c_null_funptr
        if (fcn%is_gradient_defined()) grad_entry = c_funloc(nlh_gradfcn_trampoline)
        allocate(xwork(n), source = x)
        rc = nlh_bfgs_solve(nlh_default_handle(), opts, n, c_funloc(nlh_fcnnvar_trampoline), grad_entry, c_loc(ctx), &
            xwork, fmin, counters)
        x = xwork
        if (present(fout)) fout = fmin
        if (present(ib)) then
            call behavior_import(ib, counters)      ! jacobian_count = 0, gradient_count filled by the C side
            ib%converge_on_fcn = .false.            ! bfgs has no such test (reference :751-759)
        end if
        if (rc /= 0) error stop rc      ! as at :765-767
    end subroutine

    !> Extension: bfgs%solve (bfgs_solve, :557-770) on the objective 0.5 ||F(x)||^2 of every problem of a device model
    !> batch (forward-difference gradient) -- or, for a batch created from the user's own device function with ONE
    !> function per problem (device_model_batch%create_from_device_fcn, nfcn = 1), on that function itself: the launcher is
    !> the user's fcnnvar, its optional second launcher the gradient (set_gradient_fcn).  x(n, count) in / out,
    !> fout(count): the objective values, status(count): the code each solve would have stopped with (0: converged).
    subroutine bfgs_solve_many(this, model, x, fout, ib, status)
        class(bfgs), intent(inout) :: this
        class(device_model_batch), intent(in) :: model
        real(real64), intent(inout), dimension(:,:) :: x
        real(real64), intent(out), dimension(:), optional :: fout
        type(iteration_behavior), intent(out), dimension(:), optional :: ib
        integer(int32), intent(out), dimension(:), optional :: status

        type(nlh_options) :: opts
        type(nlh_iteration_behavior), allocatable :: counters(:)
        integer(c_int32_t), allocatable :: outcome(:)
        real(c_double), allocatable :: xwork(:,:), fwork(:,:), fmin(:)
        integer(c_int) :: rc
        integer(int32) :: m, n, count, k

        if (.not.model%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        m = model%get_equation_count()
        n = model%get_variable_count()
        count = model%get_problem_count()
        if (any(shape(x) /= [n, count])) error stop NL_INVALID_INPUT_ERROR
        call this%export_options(opts)
        opts%print_status = 0
        allocate(counters(count), outcome(count), fwork(m, count), fmin(count))
        allocate(xwork(n, count), source = x)
        rc = nlh_dq_model_bfgs_solve(nlh_default_handle(), opts, model%c_handle(), xwork, fwork, fmin, counters, outcome)
        if (rc /= 0) error stop rc
        x = xwork
        if (present(fout)) fout = fmin
        if (present(status)) status = outcome
        if (present(ib)) then
            call behavior_import(ib, counters)
            do k = 1, count
                ib(k)%converge_on_fcn = .false.
            end do
        end if
    end subroutine
end module
