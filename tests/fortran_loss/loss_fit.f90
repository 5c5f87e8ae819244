! A user program of the robust losses through the Fortran shim (nonlin_amd/fortran): a batch of Lorentzian peaks on a constant
! baseline with a few spikes in every spectrum, fitted with a Huber loss whose scale differs per spectrum -- create_curve,
! create_robust, solve_batch, covariance_batch, no device code of the user's.
! Reads what tests/test_gpu_loss.py writes (stream binary: nprob, m (int32), t(m,nprob), y(m,nprob), x0(4,nprob),
! scale(nprob)) and prints, per problem,
!   x <k> <4 values, ES24.16>      sigma <k> <4 values, ES24.16>      counts <k> <iterations> <evaluations> <Jacobians> <rank>
! which the test compares digit for digit with the Python front end's.
program loss_fit
    use iso_fortran_env
    use nonlin
    implicit none

    integer(int32), parameter :: n = 4
    character(len=512) :: path
    integer(int32) :: nprob, m, k, u
    real(real64), allocatable :: t(:,:), y(:,:), x(:,:), scale(:), fvec(:,:), cov(:,:,:), sigma(:,:), chi2(:)
    integer(int32), allocatable :: rank(:), status(:)
    type(iteration_behavior), allocatable :: ib(:)
    type(device_model_batch) :: peak, robust
    type(least_squares_solver) :: lm

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, m
    allocate(t(m, nprob), y(m, nprob), x(n, nprob), scale(nprob))
    read(u) t
    read(u) y
    read(u) x
    read(u) scale
    close(u)

    ! parameters of the peak: a, mu, w, c0
    call peak%create_curve(NLH_CURVE_LORENTZ, 1, 0, t, y)
    call robust%create_robust(peak, NLH_LOSS_HUBER, scale)
    if (robust%get_variable_count() /= n .or. robust%get_equation_count() /= m .or. robust%get_problem_count() /= nprob) error stop 3
    if (.not.robust%uses_analytic_jacobian()) error stop 4

    allocate(fvec(m, nprob), ib(nprob), status(nprob), cov(n, n, nprob), sigma(n, nprob), chi2(nprob), rank(nprob))
    call lm%set_max_fcn_evals(500)
    call lm%solve_batch(robust, x, fvec, ib, status)
    if (any(status /= 0)) error stop 5
    call lm%covariance_batch(robust, x, cov, sigma, rank, chi2)
    do k = 1, nprob
        print '(A,1X,I0,*(ES24.16))', "x", k, x(:,k)
        print '(A,1X,I0,*(ES24.16))', "sigma", k, sigma(:,k)
        print '(A,5(1X,I0))', "counts", k, ib(k)%iter_count, ib(k)%fcn_count, ib(k)%jacobian_count, rank(k)
    end do
    call robust%destroy()
    call peak%destroy()
    print '(A)', "done"
end program
