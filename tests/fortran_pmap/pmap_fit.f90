! A user program of the parameter maps through the Fortran shim (nonlin_amd/fortran): a batch of Lorentzian doublets on a
! constant baseline whose second width is tied to the first (w2 = ratio * w1) and whose baseline was measured beforehand
! (fixed, a value per spectrum) -- create_curve, create_mapped, solve_batch, covariance_batch, no device code of the user's.
! Reads what tests/test_gpu_pmap.py writes (stream binary: nprob, m (int32), ratio (real64), t(m,nprob), y(m,nprob),
! full(7,nprob): the starting values, the baseline at its measured value) and prints, per problem,
!   x <k> <5 values, ES24.16>      sigma <k> <5 values, ES24.16>      counts <k> <iterations> <evaluations> <Jacobians> <rank>
! for the five free unknowns (a1, mu1, w1, a2, mu2), which the test compares digit for digit with the Python front end's.
program pmap_fit
    use iso_fortran_env
    use nonlin
    implicit none

    integer(int32), parameter :: nfull = 7
    character(len=512) :: path
    integer(int32) :: nprob, m, n, k, j, u
    integer(int32) :: kind(nfull), src(nfull)
    real(real64) :: ratio, scale(nfull), offset(nfull)
    real(real64), allocatable :: t(:,:), y(:,:), full(:,:), x(:,:), fvec(:,:), cov(:,:,:), sigma(:,:), chi2(:)
    integer(int32), allocatable :: rank(:), status(:)
    type(iteration_behavior), allocatable :: ib(:)
    type(device_model_batch) :: doublet, mapped
    type(least_squares_solver) :: lm

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, m
    read(u) ratio
    allocate(t(m, nprob), y(m, nprob), full(nfull, nprob))
    read(u) t
    read(u) y
    read(u) full
    close(u)

    ! parameters of the doublet: a1, mu1, w1, a2, mu2, w2, c0
    call doublet%create_curve(NLH_CURVE_LORENTZ, 2, 0, t, y)
    kind = NLH_PMAP_FREE
    src = 1; scale = 1.0d0; offset = 0.0d0
    kind(6) = NLH_PMAP_TIED; src(6) = 3; scale(6) = ratio       ! w2 = ratio * w1
    kind(7) = NLH_PMAP_FIXED                                     ! the baseline keeps full(7,:)
    call mapped%create_mapped(doublet, kind, src, scale, offset, full)
    n = mapped%get_variable_count()
    if (n /= 5 .or. mapped%get_equation_count() /= m .or. mapped%get_problem_count() /= nprob) error stop 3
    if (.not.mapped%uses_analytic_jacobian()) error stop 4

    allocate(x(n, nprob), fvec(m, nprob), ib(nprob), status(nprob), cov(n, n, nprob), sigma(n, nprob), chi2(nprob), rank(nprob))
    j = 0
    do k = 1, nfull                                              ! the free unknowns, in ascending full index
        if (kind(k) == NLH_PMAP_FREE) then
            j = j + 1
            x(j,:) = full(k,:)
        end if
    end do
    call lm%set_max_fcn_evals(500)
    call lm%solve_batch(mapped, x, fvec, ib, status)
    if (any(status /= 0)) error stop 5
    call lm%covariance_batch(mapped, x, cov, sigma, rank, chi2)
    do k = 1, nprob
        print '(A,1X,I0,*(ES24.16))', "x", k, x(:,k)
        print '(A,1X,I0,*(ES24.16))', "sigma", k, sigma(:,k)
        print '(A,5(1X,I0))', "counts", k, ib(k)%iter_count, ib(k)%fcn_count, ib(k)%jacobian_count, rank(k)
    end do
    call mapped%destroy()
    call doublet%destroy()
    print '(A)', "done"
end program
