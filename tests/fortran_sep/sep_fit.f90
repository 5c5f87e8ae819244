! A user program of the separable fits through the Fortran shim (nonlin_amd/fortran): a batch of Lorentzian doublets on a
! line, the amplitudes and the baseline projected out (variable projection), no device code of the user's -- first through the
! model objects (create_curve, create_separable, solve_batch over the four nonlinear unknowns, covariance_batch of the
! projected problem), then through the one-call interface nlh_curve_fit_batch_sep_h, which returns full arrays.
! Reads what tests/test_gpu_sep_fortran.py writes (stream binary: nprob, m (int32), t(m,nprob), y(m,nprob), x0(8,nprob)) and
! prints, per problem,
!   a <k> <4 values>   asigma <k> <4 values>   acounts <k> <iterations> <evaluations> <Jacobians> <rank>        (the models)
!   x <k> <8 values>   sigma <k> <8 values>    counts <k> <iterations> <evaluations> <Jacobians> <rank>         (the one call)
! (reals ES24.16), which the test compares digit for digit with the Python front end's.
program sep_fit
    use iso_fortran_env
    use iso_c_binding
    use nonlin
    use nonlin_hip_c
    implicit none

    integer(int32), parameter :: nfull = 8, n = 4
    integer(int32), parameter :: linear(4) = [7, 1, 8, 4]          ! a1, a2, c0, c1, 1-based, in any order
    integer(int32), parameter :: nonlinear(4) = [2, 3, 5, 6]
    integer(c_int32_t), parameter :: lin0(4) = [0, 3, 6, 7]
    character(len=512) :: path
    integer(int32) :: nprob, m, i, u
    integer(c_int) :: rc
    real(real64), allocatable, target :: t(:,:), y(:,:), x(:,:), fvec(:,:), cov(:,:,:), sigma(:,:), chi2(:)
    real(real64), allocatable :: a(:,:), acov(:,:,:), asigma(:,:), achi2(:), afvec(:,:)
    integer(int32), allocatable, target :: rank(:), status(:)
    integer(int32), allocatable :: arank(:), astatus(:)
    type(iteration_behavior), allocatable :: aib(:)
    type(nlh_iteration_behavior), allocatable, target :: ib(:)
    type(nlh_options) :: opts
    type(c_ptr) :: sp
    type(device_model_batch) :: peaks, projected
    type(least_squares_solver) :: lm

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, m
    allocate(t(m, nprob), y(m, nprob), x(nfull, nprob))
    read(u) t
    read(u) y
    read(u) x
    close(u)

    call peaks%create_curve(NLH_CURVE_LORENTZ, 2, 1, t, y)
    call projected%create_separable(peaks, linear)
    if (projected%get_variable_count() /= n .or. projected%get_equation_count() /= m .or. projected%get_problem_count() /= nprob) error stop 3
    if (.not.projected%uses_analytic_jacobian()) error stop 4
    allocate(a(n, nprob), afvec(m, nprob), aib(nprob), astatus(nprob), acov(n, n, nprob), asigma(n, nprob), achi2(nprob), arank(nprob))
    a = x(nonlinear, :)
    call lm%set_max_fcn_evals(500)
    call lm%solve_batch(projected, a, afvec, aib, astatus)
    if (any(astatus /= 0)) error stop 5
    call lm%covariance_batch(projected, a, acov, asigma, arank, achi2)
    do i = 1, nprob
        print '(A,1X,I0,*(ES24.16))', "a", i, a(:,i)
        print '(A,1X,I0,*(ES24.16))', "asigma", i, asigma(:,i)
        print '(A,5(1X,I0))', "acounts", i, aib(i)%iter_count, aib(i)%fcn_count, aib(i)%jacobian_count, arank(i)
    end do
    call projected%destroy()
    call peaks%destroy()

    allocate(fvec(m, nprob), ib(nprob), status(nprob), cov(nfull, nfull, nprob), sigma(nfull, nprob), chi2(nprob), rank(nprob))
    call nlh_default_options(opts)
    opts%max_evals = 500
    rc = nlh_sep_create(nfull, 4, lin0, sp)
    if (rc /= 0) error stop 6
    rc = nlh_curve_fit_batch_sep_h(nlh_default_handle(), opts, NLH_CURVE_LORENTZ, 2, 1, nprob, m, c_loc(t), 0, c_loc(y), c_null_ptr, 1, &
                                   c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, sp, c_loc(x), c_loc(fvec), c_loc(sigma), c_loc(cov), &
                                   c_loc(chi2), c_loc(rank), c_loc(ib), c_loc(status))
    if (rc /= 0) error stop 7
    if (any(status /= 0)) error stop 8
    call nlh_sep_destroy(sp)
    do i = 1, nprob
        print '(A,1X,I0,*(ES24.16))', "x", i, x(:,i)
        print '(A,1X,I0,*(ES24.16))', "sigma", i, sigma(:,i)
        print '(A,5(1X,I0))', "counts", i, ib(i)%iter_count, ib(i)%fcn_count, ib(i)%jacobian_count, rank(i)
    end do
    print '(A)', "done"
end program
