! User-side program for nelder_mead through the drop-in layer: README Example 4 (a fixed start instead of
! random_number), the reference's test_nelder_mead_1 / _2 / _3 (tests/nonlin_test_optimize.f90:54-181), a second solve
! on the same object (it continues from the first's simplex; x is ignored), and nelder_mead%solve_batch on a batch made
! from the user's own device function (device_model_batch%create_from_device_fcn with one function: crosen_launch of
! tests/device_model/user_models.hip).  Prints name, status, counts, flags, fout and the bit patterns of x.
! With the argument "errstop" it runs one solve that stops on max evaluations (error stop NL_CONVERGENCE_ERROR).
program nm_suite
    use iso_fortran_env
    use, intrinsic :: iso_c_binding
    use nonlin
    implicit none

    interface   ! the user's library (tests/device_model/user_models.hip)
        function btri_create(nprob, c) bind(C, name="btri_create") result(ctx)
            import :: c_ptr, c_int32_t, c_double
            integer(c_int32_t), value :: nprob
            real(c_double), intent(in) :: c(*)
            type(c_ptr) :: ctx
        end function
        subroutine btri_destroy(ctx) bind(C, name="btri_destroy")
            import :: c_ptr
            type(c_ptr), value :: ctx
        end subroutine
        function crosen_launch(ctx, stream, npoints, dprob, n, dx, m, df) bind(C, name="crosen_launch") result(rc)
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: ctx, stream, dprob, dx, df
            integer(c_int32_t), value :: npoints, n, m
            integer(c_int) :: rc
        end function
    end interface

    integer(int32), parameter :: nprob = 5, nq = 3
    type(nelder_mead) :: solver, s1, s2, s3, sb
    type(fcnnvar_helper) :: obj, obj2, obj3
    procedure(fcnnvar), pointer :: fcn
    type(device_model_batch) :: batch
    type(iteration_behavior) :: ib, ibs(nprob)
    real(real64) :: x(2), fout, a, c(nprob), xs(nq, nprob), fmin(nprob)
    real(real64), allocatable :: simplex(:,:)
    integer(int32) :: st(nprob), i, k
    character(len=32) :: arg
    type(c_ptr) :: bctx

    fcn => rosenbrock
    call obj%set_fcn(fcn, 2)
    if (command_argument_count() > 0) then
        call get_command_argument(1, arg)
        if (trim(arg) == "errstop") then
            call solver%set_max_fcn_evals(40)
            x = 0.0d0
            call solver%solve(obj, x, fout, ib)
            print '(A)', "not reached"
        end if
        stop
    end if

    ! ---- README Example 4
    x = [0.25d0, 0.75d0]
    call solver%solve(obj, x, fout, ib)
    print '(A,F7.5,A,F7.5,A)', "# Minimum: (", x(1), ", ", x(2), ")"
    print '(A,E9.3)', "# Function Value: ", fout
    print '(A,I0)', "# Iterations: ", ib%iter_count
    print '(A,I0)', "# Function Evaluations: ", ib%fcn_count
    call report("ex4", ib, fout, x)

    ! ---- test_nelder_mead_1: Rosenbrock from 0
    x = 0.0d0
    call s1%solve(obj, x, fout, ib)
    call report("nm1", ib, fout, x)
    simplex = s1%get_simplex()
    print '(A,*(1X,Z16.16))', "nm1_simplex", simplex

    ! ---- the same object again, on Beale's function: x is ignored, the solve starts from nm1's final simplex
    fcn => beale
    call obj2%set_fcn(fcn, 2)
    x = [7.0d0, -3.0d0]
    call s1%solve(obj2, x, fout, ib)
    call report("nm1_again", ib, fout, x)

    ! ---- test_nelder_mead_2: Beale from 1
    x = 1.0d0
    call s2%solve(obj2, x, fout, ib)
    call report("nm2", ib, fout, x)

    ! ---- test_nelder_mead_3: Rosenbrock with args = 100
    fcn => rosenbrock2
    call obj3%set_fcn(fcn, 2)
    a = 1.0d2
    x = 0.0d0
    call s3%solve(obj3, x, fout, ib, args = a)
    call report("nm3", ib, fout, x)

    ! ---- solve_batch on the user's device objective (chained Rosenbrock, one c per problem)
    do k = 1, nprob
        c(k) = 1.0d0 + 0.125d0 * k
        do i = 1, nq
            xs(i, k) = -0.5d0 + 0.0625d0 * (i + k)
        end do
    end do
    bctx = btri_create(nprob, c)
    call batch%create_from_device_fcn(c_funloc(crosen_launch), bctx, nprob, 1, nq)
    call sb%solve_batch(batch, xs, fmin, ibs, st)
    do k = 1, nprob
        call report_batch("nm_batch", ibs(k), st(k), fmin(k), xs(:, k))
    end do
    call batch%destroy()
    call btri_destroy(bctx)

contains
    ! The objectives of the reference's tests with the powers spelled out as products (the same bits as the tests'
    ! Python versions)
    function rosenbrock(x, args) result(f)
        real(real64), intent(in), dimension(:) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: f, t, u
        t = x(2) - x(1) * x(1)
        u = x(1) - 1.0d0
        f = 1.0d2 * (t * t) + u * u
    end function

    function rosenbrock2(x, args) result(f)
        real(real64), intent(in), dimension(:) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: f, a, t, u
        a = 0.0d0
        select type (args)
        type is (real(real64))
            a = args
        end select
        t = x(2) - x(1) * x(1)
        u = x(1) - 1.0d0
        f = a * (t * t) + u * u
    end function

    function beale(x, args) result(f)
        real(real64), intent(in), dimension(:) :: x
        class(*), intent(inout), optional :: args
        real(real64) :: f, p, q, r
        p = 1.5d0 - x(1) + x(1) * x(2)
        q = 2.25d0 - x(1) + x(1) * (x(2) * x(2))
        r = 2.625d0 - x(1) + x(1) * (x(2) * x(2) * x(2))
        f = p * p + q * q + r * r
    end function

    subroutine report(name, b, fv, x)
        character(len=*), intent(in) :: name
        type(iteration_behavior), intent(in) :: b
        real(real64), intent(in) :: fv, x(:)
        print '(A,1X,I0,4(1X,I0),3(1X,L1),*(1X,Z16.16))', name, 0, b%iter_count, b%fcn_count, b%jacobian_count, &
            b%gradient_count, b%converge_on_fcn, b%converge_on_chng, b%converge_on_zero_diff, fv, x
    end subroutine

    subroutine report_batch(name, b, st, fv, x)
        character(len=*), intent(in) :: name
        type(iteration_behavior), intent(in) :: b
        integer(int32), intent(in) :: st
        real(real64), intent(in) :: fv, x(:)
        print '(A,1X,I0,4(1X,I0),3(1X,L1),*(1X,Z16.16))', name, st, b%iter_count, b%fcn_count, b%jacobian_count, &
            b%gradient_count, b%converge_on_fcn, b%converge_on_chng, b%converge_on_zero_diff, fv, x
    end subroutine
end program
