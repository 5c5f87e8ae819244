! fcn1var, fcn1var_helper, equation_solver_1var and nonlin_solver_1var with the reference's public interface
! (src/nonlin_single_var.f90); the bind(C) trampolines at the bottom let the C layer call the user's procedures.
module nonlin_single_var
    use iso_fortran_env
    use, intrinsic :: iso_c_binding
    use nonlin_types
    use nonlin_error_handling
    use nonlin_hip_c, only : nlh_fd_derivative
    implicit none
    private
    public :: fcn1var
    public :: fcn1var_helper
    public :: equation_solver_1var
    public :: nonlin_solver_1var
    public :: nlh_scalar1_ctx
    public :: nlh_fcn1var_trampoline
    public :: nlh_diff1var_trampoline

    interface
        function fcn1var(x, args) result(f)
            use, intrinsic :: iso_fortran_env, only : real64
            real(real64), intent(in) :: x
            class(*), intent(inout), optional :: args
            real(real64) :: f
        end function
    end interface

    type fcn1var_helper
        procedure(fcn1var), private, pointer, nopass :: m_fcn => null()
        procedure(fcn1var), private, pointer, nopass :: m_diff => null()
    contains
        procedure, public :: fcn => f1h_fcn
        procedure, public :: is_fcn_defined => f1h_is_fcn_defined
        procedure, public :: set_fcn => f1h_set_fcn
        procedure, public :: is_derivative_defined => f1h_is_diff_defined
        procedure, public :: diff => f1h_diff_fcn
        procedure, public :: set_diff => f1h_set_diff
        procedure, public :: call_diff => f1h_user_diff
    end type

    !> What the C layer hands back to the trampolines through its void* ctx.
    type nlh_scalar1_ctx
        class(fcn1var_helper), pointer :: helper => null()
        class(*), pointer :: args => null()
    end type

    type, abstract :: equation_solver_1var                    ! defaults: src/nonlin_single_var.f90:47-54
        integer(int32), private :: m_maxEval = 100
        real(real64), private :: m_fcnTol = 1.0d-8
        real(real64), private :: m_xtol = 1.0d-12
        real(real64), private :: m_difftol = 1.0d-12
        logical, private :: m_printStatus = .false.
    contains
        procedure, public :: get_max_fcn_evals => es1_get_max_eval
        procedure, public :: set_max_fcn_evals => es1_set_max_eval
        procedure, public :: get_fcn_tolerance => es1_get_fcn_tol
        procedure, public :: set_fcn_tolerance => es1_set_fcn_tol
        procedure, public :: get_var_tolerance => es1_get_var_tol
        procedure, public :: set_var_tolerance => es1_set_var_tol
        procedure, public :: get_print_status => es1_get_print_status
        procedure, public :: set_print_status => es1_set_print_status
        procedure(nonlin_solver_1var), deferred, public, pass :: solve
        procedure, public :: get_diff_tolerance => es1_get_diff_tol
        procedure, public :: set_diff_tolerance => es1_set_diff_tol
    end type

    interface
        subroutine nonlin_solver_1var(this, fcn, x, lim, f, ib, args)
            use, intrinsic :: iso_fortran_env, only : real64
            use nonlin_types, only : iteration_behavior, value_pair
            import equation_solver_1var
            import fcn1var_helper
            class(equation_solver_1var), intent(inout) :: this
            class(fcn1var_helper), intent(in) :: fcn
            real(real64), intent(inout) :: x
            type(value_pair), intent(in) :: lim
            real(real64), intent(out), optional :: f
            type(iteration_behavior), optional :: ib
            class(*), intent(inout), optional :: args
        end subroutine
    end interface

contains
    function f1h_fcn(this, x, args) result(f)                  ! :103-118
        class(fcn1var_helper), intent(in) :: this
        real(real64), intent(in) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: f
        f = 0.0d0
        if (associated(this%m_fcn)) f = this%m_fcn(x, args)
    end function

    function f1h_is_fcn_defined(this) result(x)               ! :121-129
        class(fcn1var_helper), intent(in) :: this
        logical :: x
        x = associated(this%m_fcn)
    end function

    subroutine f1h_set_fcn(this, fcn)                         ! :132-141
        class(fcn1var_helper), intent(inout) :: this
        procedure(fcn1var), intent(in), pointer :: fcn
        this%m_fcn => fcn
    end subroutine

    function f1h_is_diff_defined(this) result(x)              ! :143-152
        class(fcn1var_helper), intent(in) :: this
        logical :: x
        x = associated(this%m_diff)
    end function

    !> f1h_diff_fcn (:154-200) through nlh_fd_derivative: the user's derivative, or the forward difference (the
    !> function at x + h, then at x unless f is given; divided by h).  The reference's dummies; the C call is made by
    !> f1h_diff_c, whose TARGET dummies the trampolines' context points at for the length of the call.
    function f1h_diff_fcn(this, x, f, args) result(df)
        class(fcn1var_helper), intent(in) :: this
        real(real64), intent(in) :: x
        real(real64), intent(in), optional :: f
        class(*), intent(inout), optional :: args
        real(real64) :: df
        df = f1h_diff_c(this, x, f, args)
    end function

    function f1h_diff_c(this, x, f, args) result(df)
        class(fcn1var_helper), intent(in), target :: this
        real(real64), intent(in) :: x
        real(real64), intent(in), optional :: f
        class(*), intent(inout), optional, target :: args
        real(real64) :: df
        type(nlh_scalar1_ctx), target :: ctx
        type(c_funptr) :: diff_entry
        real(c_double), target :: f0, dfv
        type(c_ptr) :: f0_entry
        integer(c_int) :: rc
        if (.not.this%is_fcn_defined() .and. .not.this%is_derivative_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        ctx%helper => this
        if (present(args)) ctx%args => args
        diff_entry = c_null_funptr
        if (this%is_derivative_defined()) diff_entry = c_funloc(nlh_diff1var_trampoline)
        f0_entry = c_null_ptr
        if (present(f)) then
            f0 = f
            f0_entry = c_loc(f0)
        end if
        rc = nlh_fd_derivative(c_funloc(nlh_fcn1var_trampoline), diff_entry, c_loc(ctx), x, f0_entry, dfv)
        if (rc /= 0) error stop rc
        df = dfv
    end function

    subroutine f1h_set_diff(this, diff)                       ! :203-212
        class(fcn1var_helper), intent(inout) :: this
        procedure(fcn1var), pointer, intent(in) :: diff
        this%m_diff => diff
    end subroutine

    !> The user's derivative itself (what the C layer calls; 0 when none is set).
    function f1h_user_diff(this, x, args) result(df)
        class(fcn1var_helper), intent(in) :: this
        real(real64), intent(in) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: df
        df = 0.0d0
        if (associated(this%m_diff)) df = this%m_diff(x, args)
    end function

    pure function es1_get_max_eval(this) result(n)
        class(equation_solver_1var), intent(in) :: this
        integer(int32) :: n
        n = this%m_maxEval
    end function
    subroutine es1_set_max_eval(this, n)
        class(equation_solver_1var), intent(inout) :: this
        integer(int32), intent(in) :: n
        this%m_maxEval = n
    end subroutine
    pure function es1_get_fcn_tol(this) result(x)
        class(equation_solver_1var), intent(in) :: this
        real(real64) :: x
        x = this%m_fcnTol
    end function
    subroutine es1_set_fcn_tol(this, x)
        class(equation_solver_1var), intent(inout) :: this
        real(real64), intent(in) :: x
        this%m_fcnTol = x
    end subroutine
    pure function es1_get_var_tol(this) result(x)
        class(equation_solver_1var), intent(in) :: this
        real(real64) :: x
        x = this%m_xtol
    end function
    subroutine es1_set_var_tol(this, x)
        class(equation_solver_1var), intent(inout) :: this
        real(real64), intent(in) :: x
        this%m_xtol = x
    end subroutine
    pure function es1_get_print_status(this) result(x)
        class(equation_solver_1var), intent(in) :: this
        logical :: x
        x = this%m_printStatus
    end function
    subroutine es1_set_print_status(this, x)
        class(equation_solver_1var), intent(inout) :: this
        logical, intent(in) :: x
        this%m_printStatus = x
    end subroutine
    pure function es1_get_diff_tol(this) result(x)
        class(equation_solver_1var), intent(in) :: this
        real(real64) :: x
        x = this%m_difftol
    end function
    subroutine es1_set_diff_tol(this, x)
        class(equation_solver_1var), intent(inout) :: this
        real(real64), intent(in) :: x
        this%m_difftol = x
    end subroutine

    ! ---- bind(C) trampolines: nlh_fcnnvar (ctx, n = 1, x) -> f
    function nlh_fcn1var_trampoline(ctx, n, x) bind(C) result(f)
        type(c_ptr), value :: ctx
        integer(c_int32_t), value :: n
        real(c_double), intent(in) :: x(n)
        real(c_double) :: f
        type(nlh_scalar1_ctx), pointer :: c
        call c_f_pointer(ctx, c)
        if (associated(c%args)) then
            f = c%helper%fcn(x(1), c%args)
        else
            f = c%helper%fcn(x(1))
        end if
    end function

    function nlh_diff1var_trampoline(ctx, n, x) bind(C) result(df)
        type(c_ptr), value :: ctx
        integer(c_int32_t), value :: n
        real(c_double), intent(in) :: x(n)
        real(c_double) :: df
        type(nlh_scalar1_ctx), pointer :: c
        call c_f_pointer(ctx, c)
        if (associated(c%args)) then
            df = c%helper%call_diff(x(1), c%args)
        else
            df = c%helper%call_diff(x(1))
        end if
    end function
end module
