! Drop-in program for brent_solver / newton_1var_solver through the Fortran shim (tests/test_gpu_root1v.py compiles it).
! It solves polynomials with solve (host callbacks: fcn1var, its derivative, class(*) args) and with solve_batch on a
! batch created from the user's own device function (device_model_batch%create_from_device_fcn with one equation in one
! unknown: cubic_launch of tests/device_1var/scalar_models.hip), and sin(x)/x as the reference's test_brent_1 /
! test_newton_1var_1 do.  Each line: name status iter fcn jac grad fcnvrg xcnvrg dcnvrg x f (x and f as hex bits).
! With the argument "errstop" it runs one solve that stops on max evaluations (error stop NL_CONVERGENCE_ERROR).
! A user's own solver type, declared with the reference's nonlin_solver_1var dummies (src/nonlin_single_var.f90:72-95):
! it must conform to the deferred binding of the shim's equation_solver_1var.  It delegates to brent_solver.
module root1v_user_solver
    use iso_fortran_env
    use nonlin
    implicit none
    type, extends(equation_solver_1var) :: user_brent
    contains
        procedure, public :: solve => user_solve
    end type
contains
    subroutine user_solve(this, fcn, x, lim, f, ib, args)
        class(user_brent), intent(inout) :: this
        class(fcn1var_helper), intent(in) :: fcn
        real(real64), intent(inout) :: x
        type(value_pair), intent(in) :: lim
        real(real64), intent(out), optional :: f
        type(iteration_behavior), optional :: ib
        class(*), intent(inout), optional :: args
        type(brent_solver) :: inner
        call inner%set_max_fcn_evals(this%get_max_fcn_evals())
        call inner%solve(fcn, x, lim, f, ib, args)
    end subroutine
end module

program root1v_suite
    use iso_fortran_env
    use, intrinsic :: iso_c_binding
    use nonlin
    use root1v_user_solver
    implicit none

    interface   ! the user's library (tests/device_1var/scalar_models.hip)
        function cubic_create(nprob, c) bind(C, name="cubic_create") result(ctx)
            import :: c_int32_t, c_double, c_ptr
            integer(c_int32_t), value :: nprob
            real(c_double), intent(in) :: c(*)
            type(c_ptr) :: ctx
        end function
        subroutine cubic_destroy(ctx) bind(C, name="cubic_destroy")
            import :: c_ptr
            type(c_ptr), value :: ctx
        end subroutine
        function cubic_launch(ctx, stream, npoints, dprob, n, dx, m, df) bind(C, name="cubic_launch") result(rc)
            import :: c_ptr, c_int32_t, c_int
            type(c_ptr), value :: ctx, stream, dprob, dx, df
            integer(c_int32_t), value :: npoints, n, m
            integer(c_int) :: rc
        end function
        function cubic_launch_diff(ctx, stream, npoints, dprob, n, dx, m, dj) bind(C, name="cubic_launch_diff") result(rc)
            import :: c_ptr, c_int32_t, c_int
            type(c_ptr), value :: ctx, stream, dprob, dx, dj
            integer(c_int32_t), value :: npoints, n, m
            integer(c_int) :: rc
        end function
    end interface

    integer(int32), parameter :: nprob = 5
    type(brent_solver) :: brent
    type(user_brent) :: ubrent
    type(newton_1var_solver) :: newton
    type(fcn1var_helper) :: obj, objd, obja, objs
    procedure(fcn1var), pointer :: fcn
    type(device_model_batch) :: batch, batchd
    type(iteration_behavior) :: ib, ibs(nprob)
    type(value_pair) :: lim, lims(nprob)
    real(real64) :: x, f, a, c(4, nprob), xs(nprob), fs(nprob)
    integer(int32) :: st(nprob), k
    character(len=32) :: arg
    type(c_ptr) :: cctx

    fcn => cubic
    call obj%set_fcn(fcn)
    lim%x1 = 2.0d0
    lim%x2 = -2.0d0
    if (command_argument_count() > 0) then
        call get_command_argument(1, arg)
        if (trim(arg) == "errstop") then
            call brent%set_max_fcn_evals(5)
            call brent%solve(obj, x, lim, f, ib)
            print '(A)', "not reached"
        end if
        stop
    end if

    call brent%solve(obj, x, lim, f, ib)
    call report("brent_cubic", 0, ib, x, f)
    call ubrent%solve(obj, x, lim, f, ib)                    ! through a user's extension of equation_solver_1var
    call report("user_brent_cubic", 0, ib, x, f)
    call newton%solve(obj, x, lim, f, ib)
    call report("newton_cubic", 0, ib, x, f)
    objd = obj
    fcn => cubic_diff
    call objd%set_diff(fcn)
    call newton%solve(objd, x, lim, f, ib)
    call report("newton_cubic_diff", 0, ib, x, f)
    fcn => cubic_args
    call obja%set_fcn(fcn)
    a = 3.0d0
    call newton%solve(obja, x, lim, f, ib, a)
    call report("newton_cubic_args", 0, ib, x, f)

    ! ---- the reference's test_brent_1 / test_newton_1var_1: sin(x)/x on [1.5, 5]
    fcn => sinc
    call objs%set_fcn(fcn)
    lim%x1 = 1.5d0
    lim%x2 = 5.0d0
    call brent%solve(objs, x, lim, f, ib)
    call report("brent_sin", 0, ib, x, f)
    call newton%solve(objs, x, lim, f, ib)
    call report("newton_sin", 0, ib, x, f)

    ! ---- solve_batch on the device model: c(:,k) = (-1 - k/8, -2, 0, 1), lim = (2, -2)
    do k = 1, nprob
        c(:, k) = [-1.0d0 - real(k, real64) / 8.0d0, -2.0d0, 0.0d0, 1.0d0]
        lims(k)%x1 = 2.0d0
        lims(k)%x2 = -2.0d0
    end do
    cctx = cubic_create(nprob, c)
    call batch%create_from_device_fcn(c_funloc(cubic_launch), cctx, nprob, 1, 1)
    call batchd%create_from_device_fcn(c_funloc(cubic_launch), cctx, nprob, 1, 1, c_funloc(cubic_launch_diff))
    xs = 0.0d0
    call brent%solve_batch(batch, lims, xs, fs, ibs, st)
    do k = 1, nprob
        call report("brent_batch", st(k), ibs(k), xs(k), fs(k))
    end do
    xs = 0.0d0
    call newton%solve_batch(batch, lims, xs, fs, ibs, st)
    do k = 1, nprob
        call report("newton_batch", st(k), ibs(k), xs(k), fs(k))
    end do
    xs = 0.0d0
    call newton%solve_batch(batchd, lims, xs, fs, ibs, st)
    do k = 1, nprob
        call report("newton_batch_diff", st(k), ibs(k), xs(k), fs(k))
    end do
    call batch%destroy()
    call batchd%destroy()
    call cubic_destroy(cctx)

contains
    function cubic(x, args) result(f)             ! x**3 - 2x - 1 as the device family writes it
        real(real64), intent(in) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: f
        f = -1.0d0 + x * (-2.0d0 + x * (0.0d0 + x * 1.0d0))
    end function

    function cubic_diff(x, args) result(f)
        real(real64), intent(in) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: f
        f = -2.0d0 + x * (2.0d0 * 0.0d0 + x * (3.0d0 * 1.0d0))
    end function

    function cubic_args(x, args) result(f)        ! args: the leading coefficient
        real(real64), intent(in) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: f, a
        a = 1.0d0
        if (present(args)) then
            select type (args)
            type is (real(real64))
                a = args
            end select
        end if
        f = -1.0d0 + x * (-2.0d0 + x * (0.0d0 + x * a))
    end function

    function sinc(x, args) result(f)
        real(real64), intent(in) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: f
        f = sin(x) / x
    end function

    subroutine report(name, st, b, x, f)
        character(len=*), intent(in) :: name
        integer(int32), intent(in) :: st
        type(iteration_behavior), intent(in) :: b
        real(real64), intent(in) :: x, f
        print '(A,1X,I0,4(1X,I0),3(1X,L1),2(1X,Z16.16))', name, st, b%iter_count, b%fcn_count, b%jacobian_count, &
            b%gradient_count, b%converge_on_fcn, b%converge_on_chng, b%converge_on_zero_diff, x, f
    end subroutine
end program
