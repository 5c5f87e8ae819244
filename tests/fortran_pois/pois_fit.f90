! A user program of the Poisson likelihood fits through the Fortran shim (nonlin_amd/fortran): a batch of photon-counting
! decays on a constant baseline, ragged through a 0 / 1 mask, fitted by minimising the Poisson deviance -- create_curve
! (without weights), create_poisson, solve_batch, covariance_batch with scaled = .false., no device code of the user's.
! Reads what tests/test_gpu_pois.py writes (stream binary: nprob, m (int32), t(m,nprob), y(m,nprob), w(m,nprob), x0(3,nprob))
! and prints, per problem,
!   x <k> <3 values, ES24.16>      sigma <k> <3 values, ES24.16>      counts <k> <iterations> <evaluations> <Jacobians> <rank>
! which the test compares digit for digit with the Python front end's.
program pois_fit
    use iso_fortran_env
    use nonlin
    implicit none

    integer(int32), parameter :: n = 3
    character(len=512) :: path
    integer(int32) :: nprob, m, k, u
    real(real64), allocatable :: t(:,:), y(:,:), w(:,:), x(:,:), fvec(:,:), cov(:,:,:), sigma(:,:), chi2(:)
    integer(int32), allocatable :: rank(:), status(:)
    type(iteration_behavior), allocatable :: ib(:)
    type(device_model_batch) :: decay, counts
    type(least_squares_solver) :: lm

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, m
    allocate(t(m, nprob), y(m, nprob), w(m, nprob), x(n, nprob))
    read(u) t
    read(u) y
    read(u) w
    read(u) x
    close(u)

    ! parameters of the decay: a, k, c0
    call decay%create_curve(NLH_CURVE_EXPDECAY, 1, 0, t, y)
    call counts%create_poisson(decay, y, w)
    if (counts%get_variable_count() /= n .or. counts%get_equation_count() /= m .or. counts%get_problem_count() /= nprob) error stop 3
    if (.not.counts%uses_analytic_jacobian()) error stop 4

    allocate(fvec(m, nprob), ib(nprob), status(nprob), cov(n, n, nprob), sigma(n, nprob), chi2(nprob), rank(nprob))
    call lm%set_max_fcn_evals(500)
    call lm%solve_batch(counts, x, fvec, ib, status)
    if (any(status /= 0)) error stop 5
    call lm%covariance_batch(counts, x, cov, sigma, rank, chi2, scaled=.false.)
    do k = 1, nprob
        print '(A,1X,I0,*(ES24.16))', "x", k, x(:,k)
        print '(A,1X,I0,*(ES24.16))', "sigma", k, sigma(:,k)
        print '(A,5(1X,I0))', "counts", k, ib(k)%iter_count, ib(k)%fcn_count, ib(k)%jacobian_count, rank(k)
    end do
    call counts%destroy()
    call decay%destroy()
    print '(A)', "done"
end program
