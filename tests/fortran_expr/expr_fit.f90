! A user program of the formula models through the Fortran shim (nonlin_amd/fortran): a batch of two-dimensional Gaussian
! spots -- two variables, five parameters, the model written as a string -- fitted in one call, then the standard errors of
! every parameter.  No device code of the user's, no compiler at run time.
! Reads what tests/test_gpu_expr.py writes (stream binary: nprob, m, nvar, n (int32), t(m,nprob,nvar), y(m,nprob),
! x0(n,nprob)) and prints, per problem,
!   x <k> <n values, ES24.16>      sigma <k> <n values, ES24.16>      counts <k> <iterations> <evaluations> <Jacobians> <rank>
! which the test compares digit for digit with the Python front end's results for the same inputs.
program expr_fit
    use iso_fortran_env
    use nonlin
    implicit none

    character(len=*), parameter :: formula = "b + a*exp(-((x-x0)^2 + (y-y0)^2)/(2*s^2))"
    character(len=512) :: path
    integer(int32) :: nprob, m, nvar, n, k, u
    real(real64), allocatable :: t(:,:,:), y(:,:), x(:,:), fvec(:,:), cov(:,:,:), sigma(:,:), chi2(:), x1(:), f1(:)
    type(vecfcn_helper) :: one
    type(iteration_behavior) :: ib1
    integer(int32), allocatable :: rank(:), status(:)
    type(iteration_behavior), allocatable :: ib(:)
    type(device_model_batch) :: batch
    type(least_squares_solver) :: lm

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, m, nvar, n
    allocate(t(m, nprob, nvar), y(m, nprob), x(n, nprob))
    read(u) t
    read(u) y
    read(u) x
    close(u)

    x1 = x(:,1)
    call batch%create_expr(formula, "x,y", "a,x0,y0,s,b", t, y)
    if (batch%get_variable_count() /= n .or. batch%get_equation_count() /= m) error stop 3
    if (.not.batch%uses_analytic_jacobian()) error stop 4

    allocate(fvec(m, nprob), ib(nprob), status(nprob), cov(n, n, nprob), sigma(n, nprob), chi2(nprob), rank(nprob))
    call lm%set_max_fcn_evals(500)
    call lm%solve_batch(batch, x, fvec, ib, status)
    if (any(status /= 0)) error stop 5
    call lm%covariance_batch(batch, x, cov, sigma, rank, chi2)
    do k = 1, nprob
        print '(A,1X,I0,*(ES24.16))', "x", k, x(:,k)
        print '(A,1X,I0,*(ES24.16))', "sigma", k, sigma(:,k)
        print '(A,5(1X,I0))', "counts", k, ib(k)%iter_count, ib(k)%fcn_count, ib(k)%jacobian_count, rank(k)
    end do
    call batch%destroy()

    ! one data set through the reference's own call: the same bits as inside the batch
    call one%set_device_expr(formula, "x,y", "a,x0,y0,s,b", t(:,1,:), y(:,1))
    allocate(f1(m))
    call lm%solve(one, x1, f1, ib1)
    if (any(x1 /= x(:,1)) .or. any(f1 /= fvec(:,1)) .or. ib1%jacobian_count /= ib(1)%jacobian_count) error stop 6
    call one%clear_device_model()
    print '(A)', "done"
end program
