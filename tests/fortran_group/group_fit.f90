! A user program of the global fits through the Fortran shim (nonlin_amd/fortran): groups of nsets Lorentzian doublets on a
! constant baseline whose two peak positions are common to the group -- create_curve, create_global, solve_batch,
! covariance_batch, no device code of the user's.  Reads what tests/test_gpu_group_fortran.py writes (stream binary: nprob, m,
! nsets (int32), t(m,nprob), y(m,nprob), x0(7,nprob): the starting values per data set) and prints, per group,
!   x <k> <n values, ES24.16>      sigma <k> <n values, ES24.16>      counts <k> <iterations> <evaluations> <Jacobians> <rank>
! for the n = 2 + 5 nsets outer unknowns (mu1, mu2, then a1, w1, a2, w2, c0 of every data set), which the test compares digit
! for digit with the Python front end's.
program group_fit
    use iso_fortran_env
    use nonlin
    implicit none

    integer(int32), parameter :: nfull = 7
    integer(int32), parameter :: shared(2) = [5, 2]              ! mu2 and mu1 (1-based, in any order)
    integer(int32), parameter :: local(5) = [1, 3, 4, 6, 7]
    character(len=512) :: path
    integer(int32) :: nprob, m, nsets, ngroup, n, k, g, l, u
    real(real64), allocatable :: t(:,:), y(:,:), x0(:,:), x(:,:), fvec(:,:), cov(:,:,:), sigma(:,:), chi2(:)
    integer(int32), allocatable :: rank(:), status(:)
    type(iteration_behavior), allocatable :: ib(:)
    type(device_model_batch) :: doublet, global
    type(least_squares_solver) :: lm

    if (command_argument_count() < 1) error stop 2
    call get_command_argument(1, path)
    open(newunit=u, file=trim(path), access="stream", form="unformatted", status="old")
    read(u) nprob, m, nsets
    allocate(t(m, nprob), y(m, nprob), x0(nfull, nprob))
    read(u) t
    read(u) y
    read(u) x0
    close(u)

    ! parameters of the doublet: a1, mu1, w1, a2, mu2, w2, c0
    call doublet%create_curve(NLH_CURVE_LORENTZ, 2, 0, t, y)
    call global%create_global(doublet, shared, nsets)
    ngroup = nprob / nsets
    n = global%get_variable_count()
    if (n /= 2 + 5 * nsets .or. global%get_equation_count() /= nsets * m .or. global%get_problem_count() /= ngroup) error stop 3
    if (.not.global%uses_analytic_jacobian()) error stop 4

    allocate(x(n, ngroup), fvec(nsets * m, ngroup), ib(ngroup), status(ngroup), cov(n, n, ngroup), sigma(n, ngroup), chi2(ngroup), &
        rank(ngroup))
    do k = 1, ngroup                                             ! the shared parameters from data set 1, then the local ones
        x(1, k) = x0(2, (k - 1) * nsets + 1)
        x(2, k) = x0(5, (k - 1) * nsets + 1)
        do g = 1, nsets
            do l = 1, 5
                x(2 + (g - 1) * 5 + l, k) = x0(local(l), (k - 1) * nsets + g)
            end do
        end do
    end do
    call lm%set_max_fcn_evals(500)
    call lm%solve_batch(global, x, fvec, ib, status)
    if (any(status /= 0)) error stop 5
    call lm%covariance_batch(global, x, cov, sigma, rank, chi2)
    do k = 1, ngroup
        print '(A,1X,I0,*(ES24.16))', "x", k, x(:,k)
        print '(A,1X,I0,*(ES24.16))', "sigma", k, sigma(:,k)
        print '(A,5(1X,I0))', "counts", k, ib(k)%iter_count, ib(k)%fcn_count, ib(k)%jacobian_count, rank(k)
    end do
    call global%destroy()
    call doublet%destroy()
    print '(A)', "done"
end program
