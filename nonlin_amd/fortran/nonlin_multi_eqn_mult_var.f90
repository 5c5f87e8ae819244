! Problem-definition layer with the reference's public names and signatures
! (src/nonlin_multi_eqn_mult_var.f90): vecfcn, jacobianfcn, vecfcn_helper, equation_solver,
! nonlin_solver.  vecfcn_helper%jacobian marshals to nlh_fd_jacobian (GPU column write);
! the bind(C) trampolines at the bottom let the C layer call the user's Fortran procedures.
module nonlin_multi_eqn_mult_var
    use iso_fortran_env
    use, intrinsic :: iso_c_binding
    use nonlin_types
    use nonlin_error_handling
    use nonlin_hip_c
    implicit none
    private
    public :: vecfcn
    public :: jacobianfcn
    public :: vecfcn_helper
    public :: equation_solver
    public :: nonlin_solver
    public :: nlh_callback_ctx
    public :: device_model_batch
    public :: NLH_MODEL_DENSE_QUADRATIC
    public :: NLH_CURVE_GAUSS, NLH_CURVE_LORENTZ, NLH_CURVE_EXPDECAY   ! kinds of device_model_batch%create_curve (from nonlin_hip_c)
    public :: NLH_PMAP_FREE, NLH_PMAP_FIXED, NLH_PMAP_TIED             ! kinds of a parameter, device_model_batch%create_mapped
    public :: NLH_LOSS_LINEAR, NLH_LOSS_HUBER, NLH_LOSS_SOFT_L1, NLH_LOSS_CAUCHY   ! kinds of device_model_batch%create_robust
    public :: NLH_CONV_ZERO, NLH_CONV_HOLD                             ! extensions of device_model_batch%create_convolved
    public :: NLH_FACTOR_AUTO, NLH_FACTOR_QR, NLH_FACTOR_EXACT     ! values of equation_solver%factor_policy (from nonlin_hip_c)
    public :: nlh_use_devices
    public :: nlh_vecfcn_trampoline
    public :: nlh_jacfcn_trampoline

    interface
        subroutine vecfcn(x, f, args)
            use, intrinsic :: iso_fortran_env, only : real64
            real(real64), intent(in), dimension(:) :: x
            real(real64), intent(out), dimension(:) :: f
            class(*), intent(inout), optional :: args
        end subroutine

        subroutine jacobianfcn(x, jac, args)
            use, intrinsic :: iso_fortran_env, only : real64
            real(real64), intent(in), dimension(:) :: x
            real(real64), intent(out), dimension(:,:) :: jac
            class(*), intent(inout), optional :: args
        end subroutine
    end interface

    !> Registered device residual families (SURVEY.md 8(d)): 1 = dense quadratic,
    !> r_i = (u_i + gamma u_i u_i) - b_i with u = A x accumulated in ascending column order.
    integer(int32), parameter :: NLH_MODEL_DENSE_QUADRATIC = 1

    !> Extension (no counterpart in the reference): the data of nprob independent problems of a registered
    !> residual family, resident on the GPU.  What least_squares_solver%solve_batch / newton_solver%solve_batch
    !> solve in one call, and what vecfcn_helper%set_device_model wraps for a single problem.
    type device_model_batch
        type(c_ptr), private :: model_ = c_null_ptr
        integer(int32), private :: nprob_ = 0
        integer(int32), private :: neqn_ = 0
        integer(int32), private :: nvar_ = 0
        logical, private :: analytic_ = .false.
    contains
        procedure, public :: create => dmb_create
        procedure, public :: create_from_device_fcn => dmb_create_fcn
        procedure, public :: create_curve => dmb_create_curve
        procedure, public :: create_expr => dmb_create_expr
        procedure, public :: create_mapped => dmb_create_mapped
        procedure, public :: create_global => dmb_create_global
        procedure, public :: create_separable => dmb_create_separable
        procedure, public :: create_robust => dmb_create_robust
        procedure, public :: create_poisson => dmb_create_poisson
        procedure, public :: create_convolved => dmb_create_convolved
        procedure, public :: destroy => dmb_destroy
        procedure, public :: is_defined => dmb_defined
        procedure, public :: get_problem_count => dmb_nprob
        procedure, public :: get_equation_count => dmb_neqn
        procedure, public :: get_variable_count => dmb_nvar
        procedure, public :: uses_analytic_jacobian => dmb_analytic
        procedure, public :: evaluate => dmb_eval
        procedure, public :: c_handle => dmb_handle
    end type

    type vecfcn_helper
        procedure(vecfcn), private, pointer, nopass :: fcn_ptr_ => null()
        procedure(jacobianfcn), private, pointer, nopass :: jac_ptr_ => null()
        integer(int32), private :: neqn_ = 0
        integer(int32), private :: nvar_ = 0
        type(device_model_batch), private :: model_      ! set_device_model: one problem on the device
    contains
        procedure, public :: set_device_model => helper_bind_model
        procedure, public :: set_device_fcn => helper_bind_device_fcn
        procedure, public :: set_device_curve => helper_bind_curve
        procedure, public :: set_device_expr => helper_bind_expr
        procedure, public :: clear_device_model => helper_drop_model
        procedure, public :: is_device_model_defined => helper_has_model
        procedure, public :: device_model => helper_model
        procedure, public :: set_fcn => helper_bind_fcn
        procedure, public :: set_jacobian => helper_bind_jac
        procedure, public :: is_fcn_defined => helper_has_fcn
        procedure, public :: is_jacobian_defined => helper_has_jac
        procedure, public :: fcn => helper_eval
        procedure, public :: jacobian => helper_jacobian
        procedure, public :: get_equation_count => helper_neqn
        procedure, public :: get_variable_count => helper_nvar
        procedure, public :: call_jacobian => helper_user_jac
    end type

    !> What the C layer hands back to the trampolines through its void* ctx.
    type nlh_callback_ctx
        class(vecfcn_helper), pointer :: helper => null()
        class(*), pointer :: args => null()
    end type

    type, abstract :: equation_solver
        integer(int32), private :: max_evals_ = 100
        real(real64), private :: ftol_ = 1.0d-8
        real(real64), private :: xtol_ = 1.0d-12
        real(real64), private :: gtol_ = 1.0d-12
        logical, private :: verbose_ = .false.
        !> Extension: NLH_FACTOR_EXACT (default; reference operation order, bit-identical
        !> results), NLH_FACTOR_AUTO (J^T J + Cholesky) or NLH_FACTOR_QR.
        integer(int32), public :: factor_policy = NLH_FACTOR_EXACT
    contains
        procedure, public :: get_max_fcn_evals => cfg_max_evals
        procedure, public :: set_max_fcn_evals => cfg_put_max_evals
        procedure, public :: get_fcn_tolerance => cfg_ftol
        procedure, public :: set_fcn_tolerance => cfg_put_ftol
        procedure, public :: get_var_tolerance => cfg_xtol
        procedure, public :: set_var_tolerance => cfg_put_xtol
        procedure, public :: get_gradient_tolerance => cfg_gtol
        procedure, public :: set_gradient_tolerance => cfg_put_gtol
        procedure, public :: get_print_status => cfg_verbose
        procedure, public :: set_print_status => cfg_put_verbose
        procedure, public :: export_options => cfg_export
        procedure(nonlin_solver), deferred, public, pass :: solve
    end type

    interface
        subroutine nonlin_solver(this, fcn, x, fvec, ib, args)
            use, intrinsic :: iso_fortran_env, only : real64
            use nonlin_types, only : iteration_behavior
            import equation_solver
            import vecfcn_helper
            class(equation_solver), intent(inout) :: this
            class(vecfcn_helper), intent(in), target :: fcn
            real(real64), intent(inout), dimension(:) :: x
            real(real64), intent(out), dimension(:) :: fvec
            type(iteration_behavior), optional :: ib
            class(*), intent(inout), optional, target :: args
        end subroutine
    end interface

contains
    subroutine helper_bind_fcn(this, fcn, nfcn, nvar)
        class(vecfcn_helper), intent(inout) :: this
        procedure(vecfcn), intent(in), pointer :: fcn
        integer(int32), intent(in) :: nfcn
        integer(int32), intent(in) :: nvar
        this%fcn_ptr_ => fcn
        this%neqn_ = nfcn
        this%nvar_ = nvar
    end subroutine

    subroutine helper_bind_jac(this, jac)
        class(vecfcn_helper), intent(inout) :: this
        procedure(jacobianfcn), intent(in), pointer :: jac
        this%jac_ptr_ => jac
    end subroutine

    function helper_has_fcn(this) result(x)
        class(vecfcn_helper), intent(in) :: this
        logical :: x
        x = associated(this%fcn_ptr_) .or. this%model_%is_defined()
    end function

    !> Extension: instead of a host procedure, the residual is a registered device model (kind =
    !> NLH_MODEL_DENSE_QUADRATIC: a(m,n), b(m), gamma).  solver%solve then runs the whole iteration on the GPU
    !> (no host callbacks); analytic = .true. makes newton_solver use the model's own Jacobian, as set_jacobian would.
    subroutine helper_bind_model(this, kind, a, b, gamma, analytic)
        class(vecfcn_helper), intent(inout) :: this
        integer(int32), intent(in) :: kind
        real(real64), intent(in), dimension(:,:) :: a
        real(real64), intent(in), dimension(:) :: b
        real(real64), intent(in) :: gamma
        logical, intent(in), optional :: analytic
        real(real64), allocatable :: a3(:,:,:), b2(:,:)
        allocate(a3(size(a, 1), size(a, 2), 1), b2(size(b), 1))
        a3(:,:,1) = a
        b2(:,1) = b
        call this%model_%create(kind, a3, b2, gamma, analytic)
        this%neqn_ = size(a, 1)
        this%nvar_ = size(a, 2)
    end subroutine

    !> Extension: the residual is the USER'S OWN device function -- the device form of set_fcn (reference :126-140).  fcn is a
    !> launcher with the C signature nlh_device_vecfcn of include/nonlin_hip.h (a host procedure, bind(C) or written in
    !> C / HIP, that enqueues the user's kernel on the stream it is handed), ctx whatever that launcher needs (its device
    !> data); jac, optional, a launcher for the analytic Jacobian (the device form of set_jacobian, :143-153).
    !> solver%solve(obj, x, fvec, ib) stays the reference's call; the whole iteration then runs on the GPU.
    subroutine helper_bind_device_fcn(this, fcn, ctx, nfcn, nvar, jac)
        class(vecfcn_helper), intent(inout) :: this
        type(c_funptr), intent(in) :: fcn
        type(c_ptr), intent(in) :: ctx
        integer(int32), intent(in) :: nfcn
        integer(int32), intent(in) :: nvar
        type(c_funptr), intent(in), optional :: jac
        call this%model_%create_from_device_fcn(fcn, ctx, 1, nfcn, nvar, jac)
        this%neqn_ = nfcn
        this%nvar_ = nvar
    end subroutine

    !> Extension: the residual is a built-in curve model on ONE data set t(m), y(m), optional weights w(m) -- see
    !> device_model_batch%create_curve.  solver%solve(obj, x, fvec, ib) and covariance then run on the GPU.
    subroutine helper_bind_curve(this, kind, ncomp, baseline, t, y, w, analytic)
        class(vecfcn_helper), intent(inout) :: this
        integer(int32), intent(in) :: kind, ncomp, baseline
        real(real64), intent(in), dimension(:) :: t, y
        real(real64), intent(in), dimension(:), optional :: w
        logical, intent(in), optional :: analytic
        if (present(w)) then
            call this%model_%create_curve(kind, ncomp, baseline, reshape(t, [size(t), 1]), reshape(y, [size(y), 1]), &
                reshape(w, [size(w), 1]), analytic)
        else
            call this%model_%create_curve(kind, ncomp, baseline, reshape(t, [size(t), 1]), reshape(y, [size(y), 1]), &
                analytic = analytic)
        end if
        this%neqn_ = this%model_%get_equation_count()
        this%nvar_ = this%model_%get_variable_count()
    end subroutine

    !> Extension: the residual is a formula (see device_model_batch%create_expr) on ONE data set: t(m, nvar) -- a column per
    !> variable --, y(m), optional weights w(m).  solver%solve(obj, x, fvec, ib) and covariance then run on the GPU.
    subroutine helper_bind_expr(this, formula, vars, params, t, y, w, analytic)
        class(vecfcn_helper), intent(inout) :: this
        character(len=*), intent(in) :: formula, vars, params
        real(real64), intent(in), dimension(:,:) :: t
        real(real64), intent(in), dimension(:) :: y
        real(real64), intent(in), dimension(:), optional :: w
        logical, intent(in), optional :: analytic
        if (present(w)) then
            call this%model_%create_expr(formula, vars, params, reshape(t, [size(t, 1), 1, size(t, 2)]), reshape(y, [size(y), 1]), &
                reshape(w, [size(w), 1]), analytic)
        else
            call this%model_%create_expr(formula, vars, params, reshape(t, [size(t, 1), 1, size(t, 2)]), reshape(y, [size(y), 1]), &
                analytic = analytic)
        end if
        this%neqn_ = this%model_%get_equation_count()
        this%nvar_ = this%model_%get_variable_count()
    end subroutine

    subroutine helper_drop_model(this)
        class(vecfcn_helper), intent(inout) :: this
        call this%model_%destroy()
    end subroutine

    function helper_has_model(this) result(x)
        class(vecfcn_helper), intent(in) :: this
        logical :: x
        x = this%model_%is_defined() .and. .not.associated(this%fcn_ptr_)
    end function

    function helper_model(this) result(md)
        class(vecfcn_helper), intent(in) :: this
        type(device_model_batch) :: md
        md = this%model_
    end function

    ! ---- device_model_batch -------------------------------------------------------------------
    subroutine dmb_create(this, kind, a, b, gamma, analytic)
        class(device_model_batch), intent(inout) :: this
        integer(int32), intent(in) :: kind
        real(real64), intent(in), dimension(:,:,:) :: a      ! (m, n, nprob)
        real(real64), intent(in), dimension(:,:) :: b        ! (m, nprob)
        real(real64), intent(in) :: gamma
        logical, intent(in), optional :: analytic
        integer(c_int) :: rc
        real(c_double), allocatable :: ac(:,:,:), bc(:,:)
        if (kind /= NLH_MODEL_DENSE_QUADRATIC) error stop NL_INVALID_INPUT_ERROR
        if (size(b, 1) /= size(a, 1) .or. size(b, 2) /= size(a, 3)) error stop NL_ARRAY_SIZE_ERROR
        call this%destroy()
        ac = a                                               ! contiguous copies: the dummies may be sections
        bc = b
        if (c_associated(nlh_default_device_set())) then         ! nlh_use_devices / NLH_DEVICES: dealt over several GPUs
            rc = nlh_dq_model_create_on(nlh_default_device_set(), int(size(a, 3), c_int32_t), int(size(a, 1), c_int32_t), &
                int(size(a, 2), c_int32_t), ac, bc, gamma, this%model_)
        else
            rc = nlh_dq_model_create(nlh_default_handle(), int(size(a, 3), c_int32_t), int(size(a, 1), c_int32_t), &
                int(size(a, 2), c_int32_t), ac, bc, gamma, this%model_)
        end if
        if (rc /= 0) error stop rc
        this%neqn_ = size(a, 1)
        this%nvar_ = size(a, 2)
        this%nprob_ = size(a, 3)
        this%analytic_ = .false.
        if (present(analytic)) this%analytic_ = analytic
    end subroutine

    !> nprob problems of the user's own device residual family (launchers: see vecfcn_helper%set_device_fcn); the user's
    !> kernel tells the problems apart by the index the launcher is handed for every point (0-based, position in x(:, k)).
    subroutine dmb_create_fcn(this, fcn, ctx, nprob, nfcn, nvar, jac)
        class(device_model_batch), intent(inout) :: this
        type(c_funptr), intent(in) :: fcn
        type(c_ptr), intent(in) :: ctx
        integer(int32), intent(in) :: nprob, nfcn, nvar
        type(c_funptr), intent(in), optional :: jac
        type(c_funptr) :: jentry
        integer(c_int) :: rc
        if (.not.c_associated(fcn)) error stop NL_UNDEFINED_FUNCTION_ERROR
        call this%destroy()
        jentry = c_null_funptr
        if (present(jac)) jentry = jac
        rc = nlh_device_fcn_model_create(int(nprob, c_int32_t), int(nfcn, c_int32_t), int(nvar, c_int32_t), fcn, jentry, ctx, &
            this%model_)
        if (rc /= 0) error stop rc
        this%neqn_ = nfcn
        this%nvar_ = nvar
        this%nprob_ = nprob
        this%analytic_ = c_associated(jentry)
    end subroutine

    !> A built-in curve model fitted to nprob data sets: kind NLH_CURVE_GAUSS (a, mu, sigma per component), NLH_CURVE_LORENTZ
    !> (a, mu, w) or NLH_CURVE_EXPDECAY (a, k), ncomp components, baseline = degree of a polynomial baseline (-1: none);
    !> the parameters of a problem are the components in order, then the baseline coefficients c_0 ...  t(m, nprob) --
    !> or t(m, 1): the same abscissae for every problem --, y(m, nprob), optional weights w(m, nprob) (a row of weight 0
    !> pads a shorter data set).  analytic (default .true.): the model's own Jacobian, otherwise forward differences.
    !> The model owns device copies of the data; solve_batch, covariance_batch, evaluate and set_device_model take it as
    !> they take any device model.
    subroutine dmb_create_curve(this, kind, ncomp, baseline, t, y, w, analytic)
        class(device_model_batch), intent(inout) :: this
        integer(int32), intent(in) :: kind, ncomp, baseline
        real(real64), intent(in), dimension(:,:) :: t, y
        real(real64), intent(in), dimension(:,:), optional :: w
        logical, intent(in), optional :: analytic
        integer(c_int) :: rc
        integer(c_int32_t) :: n, shared, use_jac
        real(c_double), allocatable, target :: tc(:,:), yc(:,:), wc(:,:)
        type(c_ptr) :: wp
        n = nlh_curve_nparams(int(kind, c_int32_t), int(ncomp, c_int32_t), int(baseline, c_int32_t))
        if (n < 0) error stop NL_INVALID_INPUT_ERROR
        if (size(t, 1) /= size(y, 1) .or. (size(t, 2) /= size(y, 2) .and. size(t, 2) /= 1)) error stop NL_ARRAY_SIZE_ERROR
        shared = 0
        if (size(t, 2) == 1 .and. size(y, 2) /= 1) shared = 1
        use_jac = 1
        if (present(analytic)) use_jac = merge(1, 0, analytic)
        call this%destroy()
        tc = t                                               ! contiguous copies: the dummies may be sections
        yc = y
        wp = c_null_ptr
        if (present(w)) then
            if (any(shape(w) /= shape(y))) error stop NL_ARRAY_SIZE_ERROR
            wc = w
            wp = c_loc(wc)
        end if
        rc = nlh_curve_model_create(nlh_default_handle(), int(kind, c_int32_t), int(ncomp, c_int32_t), int(baseline, c_int32_t), &
            int(size(y, 2), c_int32_t), int(size(y, 1), c_int32_t), tc, shared, yc, wp, use_jac, this%model_)
        if (rc /= 0) error stop rc
        this%neqn_ = size(y, 1)
        this%nvar_ = n
        this%nprob_ = size(y, 2)
        this%analytic_ = use_jac /= 0
    end subroutine

    !> A formula model fitted to nprob data sets: formula is an expression over the variables vars and the parameters params
    !> (comma-separated names; the order of params is the order of a problem's x), e.g. "a*exp(-k*t)+c", "t", "a,k,c" --
    !> operators + - * / ^ (a literal exponent), exp log sqrt sin cos tanh atan abs, pi (INTEGRATION.md 6h has the grammar and
    !> the stated arithmetic).  t(m, nprob, nvar) -- or t(m, 1, nvar): the same abscissae for every problem --, y(m, nprob),
    !> optional weights w(m, nprob) (a row of weight 0 pads a shorter data set).  analytic (default .true.): the formula's
    !> own forward-mode Jacobian, otherwise forward differences.  A formula the compiler refuses stops the program with
    !> NL_INVALID_INPUT_ERROR after printing the compiler's message (the column is 0-based).  The model owns the compiled
    !> program and device copies of the data.
    subroutine dmb_create_expr(this, formula, vars, params, t, y, w, analytic)
        class(device_model_batch), intent(inout) :: this
        character(len=*), intent(in) :: formula, vars, params
        real(real64), intent(in), dimension(:,:,:) :: t
        real(real64), intent(in), dimension(:,:) :: y
        real(real64), intent(in), dimension(:,:), optional :: w
        logical, intent(in), optional :: analytic
        integer(c_int) :: rc
        integer(c_int32_t) :: nvar, n, ninstr, nconst, depth, shared, use_jac
        real(c_double), allocatable, target :: tc(:,:,:), yc(:,:), wc(:,:)
        type(c_ptr) :: wp, e, msg
        character(kind=c_char), pointer :: text(:)
        integer :: k
        rc = nlh_expr_compile(trim(formula)//c_null_char, trim(vars)//c_null_char, trim(params)//c_null_char, e)
        if (rc /= 0) then
            msg = nlh_expr_error()
            call c_f_pointer(msg, text, [512])
            k = 1
            do while (k < 512 .and. text(k) /= c_null_char)
                k = k + 1
            end do
            write(error_unit, '(A,512A1)') "formula: ", text(1:k - 1)
            error stop NL_INVALID_INPUT_ERROR
        end if
        call nlh_expr_shape(e, nvar, n, ninstr, nconst, depth)
        if (size(t, 3) /= nvar .or. size(t, 1) /= size(y, 1) .or. (size(t, 2) /= size(y, 2) .and. size(t, 2) /= 1)) then
            call nlh_expr_destroy(e)
            error stop NL_ARRAY_SIZE_ERROR
        end if
        shared = 0
        if (size(t, 2) == 1 .and. size(y, 2) /= 1) shared = 1
        use_jac = 1
        if (present(analytic)) use_jac = merge(1, 0, analytic)
        call this%destroy()
        tc = t                                               ! contiguous copies: the dummies may be sections
        yc = y
        wp = c_null_ptr
        if (present(w)) then
            if (any(shape(w) /= shape(y))) error stop NL_ARRAY_SIZE_ERROR
            wc = w
            wp = c_loc(wc)
        end if
        rc = nlh_expr_model_create(nlh_default_handle(), e, int(size(y, 2), c_int32_t), int(size(y, 1), c_int32_t), tc, shared, yc, wp, &
            use_jac, this%model_)
        call nlh_expr_destroy(e)                             ! (the model keeps its own copy of the program)
        if (rc /= 0) error stop rc
        this%neqn_ = size(y, 1)
        this%nvar_ = n
        this%nprob_ = size(y, 2)
        this%analytic_ = use_jac /= 0
    end subroutine

    !> Fixed and tied parameters for a launcher-backed model (create_curve, create_expr, create_from_device_fcn): a model of
    !> the FREE unknowns of a parameter map over inner, which must outlive it.  kind(N): NLH_PMAP_FREE, NLH_PMAP_FIXED or
    !> NLH_PMAP_TIED per full parameter of inner; a tied parameter k is p(k) = scale(k) * p(src(k)) + offset(k), src 1-based
    !> (src, scale, offset are read at tied positions only); full(N, nprob) -- or full(N, 1): the same for every problem --
    !> holds the values of the fixed parameters.  The free unknowns are numbered in ascending full index
    !> (get_variable_count() of them); solve_batch, covariance_batch and evaluate take x(nfree, nprob).  A map the library
    !> refuses (INTEGRATION.md 6i) stops the program with NL_INVALID_INPUT_ERROR.
    subroutine dmb_create_mapped(this, inner, kind, src, scale, offset, full)
        class(device_model_batch), intent(inout) :: this
        class(device_model_batch), intent(in) :: inner
        integer(int32), intent(in), dimension(:) :: kind, src
        real(real64), intent(in), dimension(:) :: scale, offset
        real(real64), intent(in), dimension(:,:) :: full
        integer(c_int) :: rc
        integer(c_int32_t) :: nfull, nfree, ntied, shared
        integer(c_int32_t), allocatable :: kc(:), sc(:)
        real(c_double), allocatable :: fc(:,:), scl(:), off(:)
        type(c_ptr) :: pm
        if (.not.inner%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        nfull = inner%nvar_
        if (size(kind) /= nfull .or. size(src) /= nfull .or. size(scale) /= nfull .or. size(offset) /= nfull) &
            error stop NL_ARRAY_SIZE_ERROR
        if (size(full, 1) /= nfull .or. (size(full, 2) /= inner%nprob_ .and. size(full, 2) /= 1)) error stop NL_ARRAY_SIZE_ERROR
        shared = 0
        if (size(full, 2) == 1 .and. inner%nprob_ /= 1) shared = 1
        kc = kind
        sc = src - 1
        scl = scale
        off = offset
        fc = full
        rc = nlh_pmap_create(nfull, kc, sc, scl, off, pm)
        if (rc /= 0) error stop NL_INVALID_INPUT_ERROR
        call nlh_pmap_shape(pm, nfull, nfree, ntied)
        call this%destroy()
        rc = nlh_pmap_model_create(nlh_default_handle(), inner%model_, pm, fc, shared, this%model_)
        call nlh_pmap_destroy(pm)                            ! (the model keeps its own copies of the tables)
        if (rc /= 0) error stop rc
        this%neqn_ = inner%neqn_
        this%nvar_ = nfree
        this%nprob_ = inner%nprob_
        this%analytic_ = inner%analytic_
    end subroutine

    !> A global fit over a launcher-backed model (create_curve, create_expr, create_from_device_fcn, create_mapped,
    !> create_robust, create_poisson): a model of the OUTER unknowns of groups of nsets consecutive problems of inner, which
    !> must outlive it.  shared(:): the 1-based parameters of inner that have one value for a whole group (distinct, in any
    !> order; size 0: nothing shared); the others are free per data set.  The model has nprob / nsets problems of nsets * m
    !> equations and S + nsets * (N - S) unknowns: the shared parameters first, in ascending index, then per data set its local
    !> ones, in ascending index (INTEGRATION.md 6l).  solve_batch, covariance_batch and evaluate take x(nouter, nprob / nsets)
    !> and fvec(nsets * m, nprob / nsets).  A group the library refuses, or an inner problem count that is no multiple of
    !> nsets, stops the program with NL_INVALID_INPUT_ERROR.
    subroutine dmb_create_global(this, inner, shared, nsets)
        class(device_model_batch), intent(inout) :: this
        class(device_model_batch), intent(in) :: inner
        integer(int32), intent(in), dimension(:) :: shared
        integer(int32), intent(in) :: nsets
        integer(c_int) :: rc
        integer(c_int32_t) :: nfull, nshared, g, nouter
        integer(c_int32_t), allocatable :: sc(:)
        type(c_ptr) :: grp
        if (.not.inner%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        if (nsets < 1) error stop NL_INVALID_INPUT_ERROR
        if (mod(inner%nprob_, nsets) /= 0) error stop NL_INVALID_INPUT_ERROR
        allocate(sc(max(size(shared), 1)))
        sc = 0
        sc(1:size(shared)) = shared - 1
        rc = nlh_group_create(int(inner%nvar_, c_int32_t), int(size(shared), c_int32_t), sc, nsets, grp)
        if (rc /= 0) error stop NL_INVALID_INPUT_ERROR
        call nlh_group_shape(grp, nfull, nshared, g, nouter)
        call this%destroy()
        rc = nlh_group_model_create(nlh_default_handle(), inner%model_, grp, this%model_)
        call nlh_group_destroy(grp)                          ! (the model keeps its own copies of the tables)
        if (rc /= 0) error stop rc
        this%neqn_ = inner%neqn_ * nsets
        this%nvar_ = nouter
        this%nprob_ = inner%nprob_ / nsets
        this%analytic_ = inner%analytic_
    end subroutine

    !> A separable fit over a launcher-backed model that has its analytic Jacobian (create_curve, create_expr, create_convolved,
    !> create_from_device_fcn with a Jacobian launcher): a model of the NONLINEAR unknowns of inner, which must outlive it.
    !> linear(:): the 1-based parameters of inner the model is linear in (distinct, in any order; 1 .. 32 of them, at least one
    !> parameter left); they are solved for exactly at every trial point (variable projection, INTEGRATION.md 6n) and the
    !> solvers iterate over the others, in ascending index: solve_batch and evaluate take x(N - size(linear), nprob).  A
    !> declaration the library refuses stops the program with NL_INVALID_INPUT_ERROR.
    subroutine dmb_create_separable(this, inner, linear)
        class(device_model_batch), intent(inout) :: this
        class(device_model_batch), intent(in) :: inner
        integer(int32), intent(in), dimension(:) :: linear
        integer(c_int) :: rc
        integer(c_int32_t) :: nfull, nlin, nnl, v
        integer(c_int32_t), allocatable :: lc(:)
        integer :: i, j
        type(c_ptr) :: sp
        if (.not.inner%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        if (size(linear) < 1) error stop NL_INVALID_INPUT_ERROR
        allocate(lc(size(linear)))
        lc = linear - 1
        do i = 2, size(lc)                                   ! ascending, as the library wants them
            v = lc(i)
            j = i - 1
            do while (j >= 1)
                if (lc(j) <= v) exit
                lc(j + 1) = lc(j)
                j = j - 1
            end do
            lc(j + 1) = v
        end do
        rc = nlh_sep_create(int(inner%nvar_, c_int32_t), int(size(lc), c_int32_t), lc, sp)
        if (rc /= 0) error stop NL_INVALID_INPUT_ERROR
        call nlh_sep_shape(sp, nfull, nlin, nnl)
        call this%destroy()
        rc = nlh_sep_model_create(nlh_default_handle(), inner%model_, sp, this%model_)
        call nlh_sep_destroy(sp)                             ! (the model keeps its own copy of the tables)
        if (rc /= 0) error stop rc
        this%neqn_ = inner%neqn_
        this%nvar_ = nnl
        this%nprob_ = inner%nprob_
        this%analytic_ = .true.
    end subroutine

    !> A robust loss for a launcher-backed model (create_curve, create_expr, create_from_device_fcn, create_mapped): a model
    !> of the same unknowns over inner, which must outlive it, whose residuals are transformed so that the unchanged solvers
    !> minimise the robust cost (INTEGRATION.md 6j).  kind: NLH_LOSS_LINEAR, NLH_LOSS_HUBER, NLH_LOSS_SOFT_L1 or
    !> NLH_LOSS_CAUCHY; scale(nprob) -- or scale(1): the same for every problem -- is the residual size beyond which the loss
    !> bends, finite and positive.  solve_batch then returns the transformed residuals, covariance_batch the errors of the
    !> transformed problem.  A kind or a scale the library refuses stops the program with NL_INVALID_INPUT_ERROR.
    subroutine dmb_create_robust(this, inner, kind, scale)
        class(device_model_batch), intent(inout) :: this
        class(device_model_batch), intent(in) :: inner
        integer(int32), intent(in) :: kind
        real(real64), intent(in), dimension(:) :: scale
        integer(c_int) :: rc
        integer(c_int32_t) :: shared
        real(c_double), allocatable :: sc(:)
        if (.not.inner%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        if (size(scale) /= inner%nprob_ .and. size(scale) /= 1) error stop NL_ARRAY_SIZE_ERROR
        shared = 0
        if (size(scale) == 1 .and. inner%nprob_ /= 1) shared = 1
        sc = scale
        call this%destroy()
        rc = nlh_loss_model_create(nlh_default_handle(), inner%model_, kind, sc, shared, this%model_)
        if (rc /= 0) error stop rc
        this%neqn_ = inner%neqn_
        this%nvar_ = inner%nvar_
        this%nprob_ = inner%nprob_
        this%analytic_ = inner%analytic_
    end subroutine

    !> The Poisson likelihood for a launcher-backed model created WITHOUT weights (create_curve, create_expr,
    !> create_from_device_fcn) on the same counts y(m, nprob): a model of the same unknowns over inner, which must outlive it,
    !> whose residuals are the deviance residuals, so that the unchanged solvers minimise -2 log L (INTEGRATION.md 6k).  w(m,
    !> nprob), optional, is the mask of the rows: 1 counts, 0 does not.  mu_floor, optional (default 2**(-20)): below this model
    !> value the residual is continued linearly.  solve_batch then returns the deviance residuals; call covariance_batch with
    !> scaled = .false.: the inverse Fisher information.  Counts that are negative or not finite on a row the mask keeps (a
    !> masked row may hold anything), a mask entry that is neither 0 nor 1 or a floor that is not finite or not positive stop
    !> the program with NL_INVALID_INPUT_ERROR.
    subroutine dmb_create_poisson(this, inner, y, w, mu_floor)
        class(device_model_batch), intent(inout) :: this
        class(device_model_batch), intent(in) :: inner
        real(real64), intent(in), dimension(:,:) :: y
        real(real64), intent(in), dimension(:,:), optional :: w
        real(real64), intent(in), optional :: mu_floor
        integer(c_int) :: rc
        real(c_double) :: floor_
        real(c_double), allocatable, target :: yc(:,:), wc(:,:)
        type(c_ptr) :: wp
        if (.not.inner%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        if (any(shape(y) /= [inner%neqn_, inner%nprob_])) error stop NL_ARRAY_SIZE_ERROR
        floor_ = 2.0d0**(-20)
        if (present(mu_floor)) floor_ = mu_floor
        yc = y
        wp = c_null_ptr
        if (present(w)) then
            if (any(shape(w) /= [inner%neqn_, inner%nprob_])) error stop NL_ARRAY_SIZE_ERROR
            wc = w
            wp = c_loc(wc)
        end if
        call this%destroy()
        rc = nlh_pois_model_create(nlh_default_handle(), inner%model_, yc, wp, floor_, this%model_)
        if (rc /= 0) error stop rc
        this%neqn_ = inner%neqn_
        this%nvar_ = inner%nvar_
        this%nprob_ = inner%nprob_
        this%analytic_ = inner%analytic_
    end subroutine

    !> An instrument response for a launcher-backed model created WITHOUT weights (create_curve, create_expr,
    !> create_from_device_fcn) on the same data y(m, nprob): a model of the same unknowns over inner, which must outlive it,
    !> whose residuals are conv(model) - y, times w(m, nprob) when given (INTEGRATION.md 6m).  k(L, 1) is one kernel for every
    !> problem, k(L, nprob) one per problem, L = 1 .. 1024, used as given; origin = 0 .. L - 1 is the tap that sits on the output
    !> row, counted from 0 as in nonlin_hip.h (0: a causal response, (L - 1) / 2: a centred one); ext is NLH_CONV_ZERO (rows
    !> outside the data contribute nothing) or NLH_CONV_HOLD (they take the nearest edge row's value).  The rows must lie on one
    !> uniform grid and y must be finite on every row.  create_robust, create_poisson, create_mapped and create_global take
    !> the result.  What the library refuses stops the program with NL_INVALID_INPUT_ERROR.
    subroutine dmb_create_convolved(this, inner, k, origin, ext, y, w)
        class(device_model_batch), intent(inout) :: this
        class(device_model_batch), intent(in) :: inner
        real(real64), intent(in), dimension(:,:) :: k
        integer(int32), intent(in) :: origin, ext
        real(real64), intent(in), dimension(:,:) :: y
        real(real64), intent(in), dimension(:,:), optional :: w
        integer(c_int) :: rc
        real(c_double), allocatable, target :: kc(:,:), yc(:,:), wc(:,:)
        type(c_ptr) :: wp
        type(nlh_conv) :: cv
        if (.not.inner%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        if (any(shape(y) /= [inner%neqn_, inner%nprob_])) error stop NL_ARRAY_SIZE_ERROR
        if (size(k, 2) /= 1 .and. size(k, 2) /= inner%nprob_) error stop NL_ARRAY_SIZE_ERROR
        kc = k
        yc = y
        wp = c_null_ptr
        if (present(w)) then
            if (any(shape(w) /= [inner%neqn_, inner%nprob_])) error stop NL_ARRAY_SIZE_ERROR
            wc = w
            wp = c_loc(wc)
        end if
        cv%L = size(k, 1)
        cv%origin = origin
        cv%ext = ext
        cv%shared_k = merge(1, 0, size(k, 2) == 1)
        cv%k = c_loc(kc)
        call this%destroy()
        rc = nlh_conv_model_create(nlh_default_handle(), inner%model_, cv, yc, wp, this%model_)
        if (rc /= 0) error stop rc
        this%neqn_ = inner%neqn_
        this%nvar_ = inner%nvar_
        this%nprob_ = inner%nprob_
        this%analytic_ = inner%analytic_
    end subroutine

    subroutine dmb_destroy(this)
        class(device_model_batch), intent(inout) :: this
        if (c_associated(this%model_)) call nlh_dq_model_destroy(this%model_)
        this%model_ = c_null_ptr
        this%nprob_ = 0; this%neqn_ = 0; this%nvar_ = 0
    end subroutine

    pure function dmb_defined(this) result(x)
        class(device_model_batch), intent(in) :: this
        logical :: x
        x = c_associated(this%model_)
    end function

    pure function dmb_nprob(this) result(n)
        class(device_model_batch), intent(in) :: this
        integer(int32) :: n
        n = this%nprob_
    end function

    pure function dmb_neqn(this) result(n)
        class(device_model_batch), intent(in) :: this
        integer(int32) :: n
        n = this%neqn_
    end function

    pure function dmb_nvar(this) result(n)
        class(device_model_batch), intent(in) :: this
        integer(int32) :: n
        n = this%nvar_
    end function

    pure function dmb_analytic(this) result(x)
        class(device_model_batch), intent(in) :: this
        logical :: x
        x = this%analytic_
    end function

    function dmb_handle(this) result(h)
        class(device_model_batch), intent(in) :: this
        type(c_ptr) :: h
        h = this%model_
    end function

    !> vecfcn of every problem: f(:,k) = F_k(x(:,k)).
    subroutine dmb_eval(this, x, f)
        class(device_model_batch), intent(in) :: this
        real(real64), intent(in), dimension(:,:) :: x        ! (n, nprob)
        real(real64), intent(out), dimension(:,:) :: f       ! (m, nprob)
        integer(c_int) :: rc
        real(c_double), allocatable :: xc(:,:), fc(:,:)
        if (.not.this%is_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR
        if (size(x, 1) /= this%nvar_ .or. size(x, 2) /= this%nprob_) error stop NL_ARRAY_SIZE_ERROR
        if (size(f, 1) /= this%neqn_ .or. size(f, 2) /= this%nprob_) error stop NL_ARRAY_SIZE_ERROR
        xc = x
        allocate(fc(this%neqn_, this%nprob_))
        rc = nlh_dq_model_eval(nlh_default_handle(), this%model_, xc, fc)
        if (rc /= 0) error stop rc
        f = fc
    end subroutine

    function helper_has_jac(this) result(x)
        class(vecfcn_helper), intent(in) :: this
        logical :: x
        x = associated(this%jac_ptr_)
    end function

    subroutine helper_eval(this, x, f, args)
        class(vecfcn_helper), intent(in) :: this
        real(real64), intent(in), dimension(:) :: x
        real(real64), intent(out), dimension(:) :: f
        class(*), intent(inout), optional :: args
        real(real64), allocatable :: x2(:,:), f2(:,:)
        if (associated(this%fcn_ptr_)) then
            call this%fcn_ptr_(x, f, args)
        else if (this%model_%is_defined()) then                 ! device model: one evaluation on the GPU
            allocate(x2(size(x), 1), f2(size(f), 1))
            x2(:,1) = x
            call this%model_%evaluate(x2, f2)
            f = f2(:,1)
        end if
    end subroutine

    !> Invokes the user's analytic Jacobian routine (used by the C-side trampoline).
    subroutine helper_user_jac(this, x, jac, args)
        class(vecfcn_helper), intent(in) :: this
        real(real64), intent(in), dimension(:) :: x
        real(real64), intent(out), dimension(:,:) :: jac
        class(*), intent(inout), optional :: args
        if (associated(this%jac_ptr_)) call this%jac_ptr_(x, jac, args)
    end subroutine

    !> helper_jacobian (src/nonlin_multi_eqn_mult_var.f90:198-277): analytic dispatch, or n
    !> perturbed evaluations on the host + the (f1 - f0)/h column write on the GPU.
    subroutine helper_jacobian(this, x, jac, fv, args)
        class(vecfcn_helper), intent(in), target :: this
        real(real64), intent(inout), dimension(:) :: x
        real(real64), intent(out), dimension(:,:) :: jac
        real(real64), intent(in), dimension(:), optional, target :: fv
        class(*), intent(inout), optional, target :: args

        integer(int32) :: m, n, flag
        integer(c_int) :: rc
        type(nlh_callback_ctx), target :: ctx
        real(c_double), allocatable, target :: xc(:), jc(:,:), fvc(:)
        type(c_funptr) :: cjac
        type(c_ptr) :: fvp

        m = this%get_equation_count()
        n = this%get_variable_count()
        flag = 0
        if (size(x) /= n) then
            flag = 2
        else if (size(jac, 1) /= m .or. size(jac, 2) /= n) then
            flag = 3
        end if
        if (flag /= 0) error stop flag
        if (.not.this%is_fcn_defined()) error stop NL_UNDEFINED_FUNCTION_ERROR

        ctx%helper => this
        if (present(args)) ctx%args => args
        allocate(xc(n), jc(m, n))
        xc = x
        cjac = c_null_funptr
        if (associated(this%jac_ptr_)) cjac = c_funloc(nlh_jacfcn_trampoline)
        fvp = c_null_ptr
        if (present(fv)) then
            allocate(fvc(m))
            fvc = fv(1:m)
            fvp = c_loc(fvc)
        end if
        rc = nlh_fd_jacobian(nlh_default_handle(), m, n, c_funloc(nlh_vecfcn_trampoline), cjac, &
            c_loc(ctx), xc, fvp, jc)
        if (rc /= 0) error stop rc
        x = xc
        jac = jc
    end subroutine

    function helper_neqn(this) result(n)
        class(vecfcn_helper), intent(in) :: this
        integer(int32) :: n
        n = this%neqn_
    end function

    function helper_nvar(this) result(n)
        class(vecfcn_helper), intent(in) :: this
        integer(int32) :: n
        n = this%nvar_
    end function

    pure function cfg_max_evals(this) result(n)
        class(equation_solver), intent(in) :: this
        integer(int32) :: n
        n = this%max_evals_
    end function

    subroutine cfg_put_max_evals(this, n)
        class(equation_solver), intent(inout) :: this
        integer(int32), intent(in) :: n
        this%max_evals_ = n
    end subroutine

    pure function cfg_ftol(this) result(x)
        class(equation_solver), intent(in) :: this
        real(real64) :: x
        x = this%ftol_
    end function

    subroutine cfg_put_ftol(this, x)
        class(equation_solver), intent(inout) :: this
        real(real64), intent(in) :: x
        this%ftol_ = x
    end subroutine

    pure function cfg_xtol(this) result(x)
        class(equation_solver), intent(in) :: this
        real(real64) :: x
        x = this%xtol_
    end function

    subroutine cfg_put_xtol(this, x)
        class(equation_solver), intent(inout) :: this
        real(real64), intent(in) :: x
        this%xtol_ = x
    end subroutine

    pure function cfg_gtol(this) result(x)
        class(equation_solver), intent(in) :: this
        real(real64) :: x
        x = this%gtol_
    end function

    subroutine cfg_put_gtol(this, x)
        class(equation_solver), intent(inout) :: this
        real(real64), intent(in) :: x
        this%gtol_ = x
    end subroutine

    pure function cfg_verbose(this) result(x)
        class(equation_solver), intent(in) :: this
        logical :: x
        x = this%verbose_
    end function

    subroutine cfg_put_verbose(this, x)
        class(equation_solver), intent(inout) :: this
        logical, intent(in) :: x
        this%verbose_ = x
    end subroutine

    !> Extension used by every solve body of the shim: the C ABI's option record with this solver's settings
    !> (library defaults for everything the base type does not hold); quiet = .true. suppresses print_status.
    subroutine cfg_export(this, opts, quiet)
        class(equation_solver), intent(in) :: this
        type(nlh_options), intent(out) :: opts
        logical, intent(in), optional :: quiet
        call nlh_default_options(opts)
        opts%max_evals = this%max_evals_
        opts%ftol = this%ftol_
        opts%xtol = this%xtol_
        opts%gtol = this%gtol_
        opts%print_status = merge(1, 0, this%verbose_)
        if (present(quiet)) then
            if (quiet) opts%print_status = 0
        end if
        opts%factor_policy = this%factor_policy
    end subroutine

    ! ---- trampolines: the C layer's nlh_vecfcn / nlh_jacfcn --------------------------------
    subroutine nlh_vecfcn_trampoline(ctx, n, x, m, f) bind(C)
        type(c_ptr), value :: ctx
        integer(c_int32_t), value :: n, m
        real(c_double), intent(in) :: x(n)
        real(c_double), intent(out) :: f(m)
        type(nlh_callback_ctx), pointer :: c
        call c_f_pointer(ctx, c)
        if (associated(c%args)) then
            call c%helper%fcn(x, f, c%args)
        else
            call c%helper%fcn(x, f)
        end if
    end subroutine

    subroutine nlh_jacfcn_trampoline(ctx, n, x, m, jac) bind(C)
        type(c_ptr), value :: ctx
        integer(c_int32_t), value :: n, m
        real(c_double), intent(in) :: x(n)
        real(c_double), intent(out) :: jac(m, n)
        type(nlh_callback_ctx), pointer :: c
        call c_f_pointer(ctx, c)
        if (associated(c%args)) then
            call c%helper%call_jacobian(x, jac, c%args)
        else
            call c%helper%call_jacobian(x, jac)
        end if
    end subroutine
end module
