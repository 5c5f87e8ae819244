! A user program of the instrument-response fits through the Fortran shim (nonlin_amd/fortran): a batch of photon-counting
! decays on a constant baseline, recorded through an instrument response, fitted by reconvolution under the Poisson deviance
! -- create_curve (without weights), create_convolved, create_poisson, solve_batch, covariance_batch with scaled = .false.,
! no device code of the user's.
! Reads what tests/test_gpu_conv.py writes (stream binary: nprob, m, L, origin, ext (int32), t(m,nprob), y(m,nprob),
! w(m,nprob), k(L), x0(3,nprob)) and prints, per problem,
!   x <k> <3 values, ES24.16>      sigma <k> <3 values, ES24.16>      counts <k> <iterations> <evaluations> <Jacobians> <rank>
! which the test compares digit for digit with the Python front end's.
program conv_fit
    use iso_fortran_env
    use nonlin
    implicit none

    integer(int32), parameter :: n = 3
    character(len=512) :: path
    integer(int32) :: nprob, m, L, origin, ext, i, u
    real(real64), allocatable :: t(:,:), y(:,:), w(:,:), k(:,:), x(:,:), fvec(:,:), cov(:,:,:), sigma(:,:), chi2(:)
    integer(int32), allocatable :: rank(:), status(:)
    type(iteration_behavior), allocatable :: ib(:)
    type(device_model_batch) :: decay, recorded, counts
    type(least_squares_solver) :: lm

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, m, L, origin, ext
    allocate(t(m, nprob), y(m, nprob), w(m, nprob), k(L, 1), x(n, nprob))
    read(u) t
    read(u) y
    read(u) w
    read(u) k
    read(u) x
    close(u)

    ! parameters of the decay: a, k, c0; the mask stays with the Poisson model
    call decay%create_curve(NLH_CURVE_EXPDECAY, 1, 0, t, y)
    call recorded%create_convolved(decay, k, origin, ext, y)
    call counts%create_poisson(recorded, y, w)
    if (counts%get_variable_count() /= n .or. counts%get_equation_count() /= m .or. counts%get_problem_count() /= nprob) error stop 3
    if (.not.counts%uses_analytic_jacobian()) error stop 4

    allocate(fvec(m, nprob), ib(nprob), status(nprob), cov(n, n, nprob), sigma(n, nprob), chi2(nprob), rank(nprob))
    call lm%set_max_fcn_evals(500)
    call lm%solve_batch(counts, x, fvec, ib, status)
    if (any(status /= 0)) error stop 5
    call lm%covariance_batch(counts, x, cov, sigma, rank, chi2, scaled=.false.)
    do i = 1, nprob
        print '(A,1X,I0,*(ES24.16))', "x", i, x(:,i)
        print '(A,1X,I0,*(ES24.16))', "sigma", i, sigma(:,i)
        print '(A,5(1X,I0))', "counts", i, ib(i)%iter_count, ib(i)%fcn_count, ib(i)%jacobian_count, rank(i)
    end do
    call counts%destroy()
    call recorded%destroy()
    call decay%destroy()
    print '(A)', "done"
end program
